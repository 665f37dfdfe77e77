"""The pair kernel (csrc/er_pairwise.hip) on the GPU, driven through loss_builder.build, against the fp64 CPU evaluation
of the torch compositions (builders/pairwise_loss.py, pinned to the reference by tests/test_pairwise_loss_pins.py)
differentiated by autograd; and two estimator steps on the kernel against two on the composition.

Bars: 1e-5 of the expected loss, 1e-4 of the largest expected gradient; where the fp32 formula itself misses those
(printed per case), four times the fp32 composition's own measured error on the same inputs.

Inputs keep the fp64 reference alone unambiguous (asserted on it): labels are multiples of 0.5, logits multiples of 1 / 64
within +/- 4, temperatures powers of two and the constant margins off that grid by 1 / 256 - so no pair lies within 1e-3
of focal's hinge_margin boundary or of a constant-margin hinge's kink, and a label-margin hinge meets its kink exactly
(derivative 0 on both sides of the comparison)."""
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.builders import loss_builder  # noqa: E402
from easyrec_amd.builders import pairwise_loss as pwl  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.protos import loss_pb2  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402

logging.disable(logging.WARNING)
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = 'EASYREC_AMD_FUSED_PAIRWISE'
LT = loss_pb2.LossType
SCALE = 0.75
OFF = 1.0 / 256

# kind -> (loss type, its parameter as the plain cases use it, its parameter with T != 1 and a constant margin)
KINDS = {
    'pair_wise': (LT.PAIR_WISE_LOSS, None, loss_pb2.PairwiseLoss(margin=0.5 + OFF, temperature=2.0)),
    'logistic': (LT.PAIRWISE_LOGISTIC_LOSS, loss_pb2.PairwiseLogisticLoss(use_label_margin=True),
                 loss_pb2.PairwiseLogisticLoss(hinge_margin=0.5 + OFF, temperature=0.5)),
    'hinge': (LT.PAIRWISE_HINGE_LOSS, None,
              loss_pb2.PairwiseHingeLoss(use_label_margin=False, margin=1.0 + OFF, temperature=2.0)),
    'focal': (LT.PAIRWISE_FOCAL_LOSS, loss_pb2.PairwiseFocalLoss(hinge_margin=1.0 + OFF, gamma=2.0),
              loss_pb2.PairwiseFocalLoss(hinge_margin=0.5 + OFF, gamma=1.5, alpha=0.25, temperature=2.0)),
}
SIZES = (1, 2, 255, 256, 257, 513, 2049)  # one example, one pair, a tile edge, several row blocks and ragged column splits
CASES = [(k, B, keyed, weighted, 'plain') for k in KINDS for B in SIZES for keyed in (False, True) for weighted in (False, True)]
CASES += [(k, 257, True, True, v) for k in KINDS for v in ('equal_labels', 'temperature_margin')]


def _inputs(B, keyed, weighted, variant):
  rng = np.random.default_rng(B * 8 + keyed * 4 + weighted * 2 + len(variant))
  z = torch.from_numpy(rng.integers(-256, 257, size=B) / 64.0)
  y = torch.from_numpy(rng.integers(0, 4, size=B) * 0.5)  # graded, with ties
  if B == 2:
    y = torch.tensor([0.0, 1.0], dtype=torch.float64)     # the one pair
  if variant == 'equal_labels':
    y = torch.full((B,), 0.5, dtype=torch.float64)
  keys = None
  if keyed:
    keys = torch.from_numpy(rng.integers(0, max(B // 8, 1), size=B)) * 7919 - 5
    keys[B // 2] = 1 << 40  # a singleton session, beyond 32 bits
    if B == 2:
      keys[:] = 3
  w = None
  if weighted:
    w = torch.from_numpy(np.round(rng.random(B) * 2, 2) + 0.25)
    w[torch.from_numpy(rng.random(B) < 0.2)] = 0.0  # a few zeros
  return z, y, keys, w


def _reference(loss_type, param, z, y, keys, w, dtype):
  """-> (loss, d loss / d z, the pair mask's sum) of the composition on the CPU in `dtype`"""
  p = pwl.params_of(loss_type, param)
  zr = z.to(dtype).clone().requires_grad_(True)
  loss = pwl.compose(loss_type, y.to(dtype), zr, keys, None if w is None else w.to(dtype), p) * SCALE
  dz, = torch.autograd.grad(loss, zr)
  s = z / p['temperature']
  d = s[:, None] - s[None, :]
  mask = pwl._pair_mask(y, keys)
  edge = p['hinge_margin'] if loss_type == LT.PAIRWISE_FOCAL_LOSS else \
      p['margin'] if loss_type == LT.PAIRWISE_HINGE_LOSS and not p['use_label_margin'] else None
  if edge is not None and bool(mask.any()):
    assert float((d[mask] - edge).abs().min()) > 1e-3  # no pair near the boundary where it drops out / the hinge's kink
  if loss_type == LT.PAIRWISE_FOCAL_LOSS and edge is not None:
    mask = mask & (d < edge)
  return loss.detach(), dz, int(mask.sum())


def _rel(got, want):
  return float((got.double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _on_kernel(loss_type, param, z, y, keys, w):
  d = lambda t, dt: None if t is None else t.to(DEV, dt)  # noqa: E731
  loss, dz = loss_builder.build(loss_type, d(y, torch.float32), d(z, torch.float32), 1.0 if w is None else d(w, torch.float32),
                                loss_scale=SCALE, loss_param=param, session_ids=d(keys, torch.int64))
  extras = loss._er_extras
  assert extras is not None and loss._er_partials[1:] == (1.0, 1.0)  # the kernel ran; the loss tail sums its partials
  return loss._er_partials[0].clone(), dz, extras['pair_count']


@pytest.mark.parametrize('kind,B,keyed,weighted,variant', CASES, ids=lambda v: str(v))
def test_kernel_against_fp64_composition(kind, B, keyed, weighted, variant):
  loss_type, plain, temp = KINDS[kind]
  param = temp if variant == 'temperature_margin' else plain
  z, y, keys, w = _inputs(B, keyed, weighted, variant)
  assert float(z.abs().max()) <= 4.0 and bool(((y * 2) == (y * 2).round()).all())
  want_loss, want_dz, want_pairs = _reference(loss_type, param, z, y, keys, w, torch.float64)
  comp_loss, comp_dz, _ = _reference(loss_type, param, z, y, keys, w, torch.float32)
  partials, dz, pairs = _on_kernel(loss_type, param, z, y, keys, w)
  again = _on_kernel(loss_type, param, z, y, keys, w)
  assert all(torch.equal(a, b) for a, b in zip((partials, dz, pairs), again))  # two runs: the same bits
  assert int(pairs) == want_pairs
  got_loss = partials.double().sum().cpu()
  assert bool(torch.isfinite(got_loss)) and bool(torch.isfinite(dz).all())
  assert (want_pairs > 0) == (variant != 'equal_labels') or B <= 2
  if float(want_loss) == 0.0 and float(want_dz.abs().max()) == 0.0:  # no pair (B = 1, equal labels): exactly nothing
    assert float(got_loss) == 0.0 and float(dz.abs().max()) == 0.0
    return
  errs = (_rel(got_loss, want_loss), _rel(comp_loss, want_loss), _rel(dz, want_dz), _rel(comp_dz, want_dz))
  print('  %s B %d pairs %d: loss kernel %.2e composition %.2e | dlogits kernel %.2e composition %.2e' %
        ((kind, B, want_pairs) + errs))
  assert errs[0] <= max(1e-5, 4.0 * errs[1]) and errs[2] <= max(1e-4, 4.0 * errs[3])


def test_runs_and_graph_replay_bit_identical():
  z, y, keys, w = _inputs(513, True, True, 'plain')
  zd, yd, kd, wd = z.to(DEV, torch.float32), y.to(DEV, torch.float32), keys.to(DEV), w.to(DEV, torch.float32)

  def run():
    o = kernels.hip().pairwise_loss(zd, yd, kd, wd, kernels.PAIR_FOCAL, kernels.PAIR_HINGE_MARGIN, hinge_margin=1.0 + OFF)
    return [o['loss_partials'], o['dlogits'], o['pair_count']]
  assert_runs_and_replay_bit_identical(run)


def test_grid_is_zero_outside_the_envelope():
  be = kernels.hip()
  assert be.pairwise_grid(8193) == 0 and be.pairwise_grid(0) == 0
  assert be.pairwise_grid(4096) == 256 and be.pairwise_grid(8192) >= 256 and be.pairwise_grid(1) == 1


def _two_steps(fused):
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'multi_tower_f1_pairwise_criteo_small.config'))
  entry = cfg.model_config.losses[1]
  assert entry.loss_type == LT.PAIR_WISE_LOSS
  entry.loss_type = LT.PAIRWISE_LOGISTIC_LOSS
  entry.pairwise_logistic_loss.session_name = 'C1'
  before = os.environ.get(SWITCH)
  os.environ[SWITCH] = '1' if fused else '0'
  be, calls = kernels.hip(), []
  inner = be.pairwise_loss
  be.pairwise_loss = lambda *a, **k: (calls.append(a[2] is not None), inner(*a, **k))[1]  # (were session keys given?)
  try:
    est = EasyRecEstimator(cfg, device=DEV, batch_size=192, seed=11).build()
    gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=192, seed=111)
    losses = []
    for _ in range(2):
      est.train_step(gen.next_batch())
      losses.append(est.loss_values())
      if len(losses) == 1:
        first = {k: v for k, v in est.state_dict(slots=True).items() if k.endswith('/m')}
    return losses, first, calls
  finally:
    del be.pairwise_loss  # (the instance attribute: the class's method shows again)
    if before is None:
      del os.environ[SWITCH]
    else:
      os.environ[SWITCH] = before


def test_estimator_on_the_kernel_against_the_composition():
  """PAIRWISE_LOGISTIC_LOSS keyed by an id feature, two steps each way; tests/_oracle_steps.first_steps' bars: every loss
  1e-5 (first step) / 1e-4 (second) of max(1e-3, |expected|), every variable's first moment after the first step 2e-4 of
  its own scale + 2e-6 of the largest"""
  got, got_m, launched = _two_steps(True)
  want, want_m, composed = _two_steps(False)
  assert launched == [True, True] and not composed, (launched, composed)
  for step, tol in ((0, 1e-5), (1, 1e-4)):
    assert set(got[step]) == set(want[step]) and 'pairwise_logistic_loss' in want[step]
    for k in want[step]:
      print(step, k, got[step][k], want[step][k])
      assert np.isfinite(got[step][k])
      assert abs(got[step][k] - want[step][k]) <= tol * max(1e-3, abs(want[step][k])), (step, k)
  assert set(got_m) == set(want_m) and got_m
  largest = max(float(np.abs(v).max()) for v in want_m.values())
  assert largest > 0
  for k, v in want_m.items():
    err = float(np.abs(got_m[k] - v).max())
    assert err <= 2e-4 * float(np.abs(v).max()) + 2e-6 * largest, (k, err)
