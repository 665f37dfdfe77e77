"""The sorted-segment kernel (csrc/er_listwise.hip) on the GPU, through the autograd function over it
(builders/listwise_loss.fused), against fp64 torch autograd of the reference's literal form: a loop over the unique keys
with one boolean mask each.

Bars: 1e-5 of the expected loss, 1e-4 of the largest expected d loss / d logits; where the fp32 formula itself misses
those, four times the fp32 composition's own measured error on the same inputs.  The two scale
gradients are sums over the batch whose terms cancel - scale_b's is zero in exact arithmetic, softmax being shift
invariant - so they are held to 1e-4 of the sum of their terms' magnitudes, sum |g_i z_i| and sum |g_i| of the fp64
reference: the scale an fp32 sum's rounding has."""
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.builders import listwise_loss as lwl  # noqa: E402
from easyrec_amd.builders import loss_builder  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.protos import loss_pb2  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402

logging.disable(logging.ERROR)
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT = loss_pb2.LossType
SCALE = 0.75
I64 = np.iinfo(np.int64)
RANK = lambda **kw: (LT.LISTWISE_RANK_LOSS, loss_pb2.ListwiseRankLoss(session_name='u', **kw))  # noqa: E731
DISTILL = lambda **kw: (LT.LISTWISE_DISTILL_LOSS, loss_pb2.ListwiseDistillLoss(session_name='u', **kw))  # noqa: E731
# (loss type, parameter), scale (w, b) or None: both kinds x label_is_logits x scale (w negative once) x temperature
CONFIGS = ((RANK(), None), (RANK(label_is_logits=True, temperature=0.5), (-1.5, 0.25)), (RANK(temperature=0.5), (1.25, -0.5)),
           (RANK(label_is_logits=True), None), (DISTILL(), (0.75, 0.5)), (DISTILL(temperature=0.5, label_clip_max_value=64.0), None))
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 8192)  # padding to 2^k; 1, 2, 4, 8 records a lane; wave and workgroup carries
PATTERNS = ('one', 'distinct', 'runs', 'interleaved', 'wide')
CASES = [(B, pat, (i * len(PATTERNS) + j) % len(CONFIGS)) for i, B in enumerate(SIZES) for j, pat in enumerate(PATTERNS)]
CASES += [(1025, 'interleaved', c) for c in range(len(CONFIGS))] + [(8192, 'runs', c) for c in range(len(CONFIGS))]


def _keys(pattern, B, rng):
  i = np.arange(B, dtype=np.int64)
  if pattern == 'one':
    return np.full(B, -7, dtype=np.int64)
  if pattern == 'distinct':
    return rng.permutation(B).astype(np.int64) * 3 - B  # (negative keys among them)
  if pattern == 'runs':  # sorted already; run lengths that end on element, lane, wave and quarter-workgroup edges and off them
    lengths = np.resize(np.array([1, 7, 8, 56, 64, 3, 61, 448, 512, 5, 2043]), B)
    return np.repeat(np.arange(B, dtype=np.int64), lengths)[:B] - 11
  if pattern == 'interleaved':  # a session's members B / 8 apart: the scatter back is no identity
    return (i % max(B // 8, 1)) * 7919 - 5
  keys = ((i % 5) << 33) * np.where(i % 2 == 0, 1, -1)  # differ only above bit 32, both signs
  keys[::7] = I64.max
  keys[B // 2::11] = I64.min
  return keys


def _inputs(B, pattern, kind):
  rng = np.random.default_rng(B * 16 + len(pattern))
  keys = _keys(pattern, B, rng)
  z = rng.standard_normal(B) * 2.0
  z[keys == keys[0]] *= np.where(rng.random(int((keys == keys[0]).sum())) < 0.5, 40.0, 1.0)  # magnitudes up to ~80 in one session
  z[0] = 80.0
  if kind == LT.LISTWISE_DISTILL_LOSS:
    y = np.exp(rng.random(B) * 8.0 - 1.4)  # rank positions 0.25 .. 700: below 1 and above either clip
  else:
    y = np.round(rng.random(B) * 3.0, 2)   # graded relevance (as logits under label_is_logits)
  exact = lambda v: torch.from_numpy(v.astype(np.float32).astype(np.float64))  # noqa: E731 (fp32 values: no input rounding)
  return exact(z), exact(y), torch.from_numpy(keys)


def _reference(kind, p, z, y, keys, scale, dtype):
  """The reference's form, literally -> (loss, d loss / d z, d / d scale_w, d / d scale_b, number of sessions)"""
  z = z.to(dtype).clone().requires_grad_(True)
  w, b = (torch.tensor([v], dtype=dtype, requires_grad=True) for v in (scale or (1.0, 0.0)))
  y, T = y.to(dtype), p['temperature']
  if kind == LT.LISTWISE_DISTILL_LOSS:
    y = torch.log1p(torch.tensor(p['label_clip_max'], dtype=dtype)) - torch.log(torch.clamp(y, 1, p['label_clip_max']))
  a = (z * torch.abs(w) + b) if scale else z
  if T != 1.0:
    a = a / T
    y = y / T if p['label_is_logits'] else y
  sessions = torch.unique(keys)
  losses = []
  for x in sessions:
    m = keys == x
    t = y[m] / y[m].sum() if kind == LT.LISTWISE_DISTILL_LOSS else (torch.softmax(y[m], 0) if p['label_is_logits'] else y[m])
    losses.append(-(t * torch.log_softmax(a[m], 0)).sum())
  loss = torch.stack(losses).mean() * SCALE
  loss.backward()
  return loss.detach(), z.grad, w.grad, b.grad, len(sessions)


def _check(got, kind, p, z, y, keys, scale):
  """got: (loss, dz, dw, db) of the path under test, against fp64 at the module's bars"""
  want = _reference(kind, p, z, y, keys, scale, torch.float64)
  comp = None
  wabs = abs(scale[0]) if scale else 1.0  # g = dz / |w|
  bars = (max(abs(float(want[0])), 1e-30), max(float(want[1].abs().max()), 1e-30),
          float((want[1] * z).abs().sum()) / wabs + 1e-30, float(want[1].abs().sum()) / wabs + 1e-30)
  for i, tol in enumerate((1e-5, 1e-4, 1e-4, 1e-4)):
    if got[i] is None:
      continue
    err = float((got[i].double().cpu().reshape(-1) - want[i].reshape(-1)).abs().max()) / bars[i]
    print('  output %d: error %.2e of %.3e' % (i, err, bars[i]))
    if not err <= tol:  # the fp32 formula's own error decides
      comp = comp or _reference(kind, p, z, y, keys, scale, torch.float32)
      ref = float((comp[i].double().reshape(-1) - want[i].reshape(-1)).abs().max()) / bars[i]
      print('  output %d: fp32 composition %.2e' % (i, ref))
      assert np.isfinite(err) and err <= 4.0 * ref, (i, err, ref)
  return want


def _fused(kind, p, z, y, keys, scale, pitch=1):
  zd = torch.zeros(z.numel(), pitch, device=DEV)
  zd[:, 0] = z.to(DEV, torch.float32)
  zd.requires_grad_(True)
  w, b = (torch.tensor([v], device=DEV, requires_grad=True) for v in scale) if scale else (None, None)
  loss, n = lwl.fused(kind, y.to(DEV, torch.float32), zd[:, 0], keys.to(DEV), p, w, b, loss_scale=SCALE)
  (loss * 2.0).backward()  # (an upstream gradient that is not 1)
  return loss.detach(), zd.grad[:, 0] / 2.0, None if w is None else w.grad / 2.0, None if b is None else b.grad / 2.0, n


@pytest.mark.parametrize('B,pattern,config', CASES, ids=lambda v: str(v))
def test_kernel_against_fp64_autograd_of_the_reference_form(B, pattern, config):
  (kind, param), scale = CONFIGS[config]
  p = lwl.params_of(kind, param)
  z, y, keys = _inputs(B, pattern, kind)
  got = _fused(kind, p, z, y, keys, scale, pitch=3 if B % 2 else 1)
  again = _fused(kind, p, z, y, keys, scale, pitch=3 if B % 2 else 1)
  assert all(a is None or torch.equal(a, b) for a, b in zip(got, again))  # two runs: the same bits
  want = _check(got[:4], kind, p, z, y, keys, scale)
  assert int(got[4]) == want[4] == len(set(keys.tolist()))


def test_null_outputs_envelope_and_graph_replay():
  be = kernels.hip()
  assert be.listwise_grid(0) == 0 and be.listwise_grid(8193) == 0 and be.listwise_grid(1) == be.listwise_grid(8192) == 1
  assert int(be.lib.er_listwise_lds_bytes(8192)) == 96 << 10 and int(be.lib.er_listwise_lds_bytes(8193)) == 0
  z, y, keys = (t.to(DEV) for t in _inputs(8192, 'interleaved', LT.LISTWISE_RANK_LOSS))
  z, y = z.float(), y.float()
  w, b = torch.tensor([-1.5], device=DEV), torch.tensor([0.25], device=DEV)
  grads = [torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)]
  kw = dict(kind=kernels.LIST_RANK, flags=kernels.LIST_LABEL_IS_LOGITS, temperature=0.5, scale_w=w, scale_b=b)

  def run():
    o = be.listwise_loss(z, y, keys, grads=kernels.ThetaGradTable(grads), acc=False, **kw)
    return [o['loss_partials'], o['dlogits'], o['num_sessions']] + grads
  full = [t.clone() for t in run()]
  assert_runs_and_replay_bit_identical(run)
  # every optional output left out in turn: the others keep their bits
  assert torch.equal(be.listwise_loss(z, y, keys, want=('loss',), **kw)['loss_partials'], full[0])
  assert torch.equal(be.listwise_loss(z, y, keys, want=('dlogits',), **kw)['dlogits'], full[1])
  assert torch.equal(be.listwise_loss(z, y, keys, want=('num_sessions',), **kw)['num_sessions'], full[2])
  with pytest.raises(RuntimeError, match='er_listwise'):
    be.listwise_loss(z, y, keys, kind=kernels.LIST_RANK, temperature=0.0)


@pytest.mark.parametrize('B,device', [(8193, DEV), (65, 'cpu')])
def test_outside_the_envelope_and_on_the_cpu_the_composition_runs(B, device):
  for (kind, param), scale in (CONFIGS[1], CONFIGS[4]):
    z, y, keys = _inputs(B, 'interleaved', kind)
    sv = tuple(torch.tensor([v], device=device, requires_grad=True) for v in scale)
    loss, dz = loss_builder.build(kind, y.to(device, torch.float32), z.to(device, torch.float32), 1.0, loss_scale=SCALE,
                                  loss_param=param, session_ids=keys.to(device), scale_vars=sv)
    assert loss._er_extras is None  # (no launch)
    _check((loss, dz, sv[0].grad, sv[1].grad), kind, lwl.params_of(kind, param), z, y, keys, scale)


@pytest.mark.parametrize('kind', ['listwise_rank_loss', 'listwise_distill_loss'])
def test_the_step_with_the_kernel_replays_from_a_graph(kind):
  """configs/multi_tower_f1_pairwise_criteo_small.config with its pairwise loss replaced: three steps replayed from a
  captured hipGraph give the losses of three eager steps."""
  losses = {}
  for graph in (False, True):
    cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'multi_tower_f1_pairwise_criteo_small.config'))
    entry = cfg.model_config.losses[1]
    entry.loss_type = LT.Value(kind.upper())
    getattr(entry, kind).session_name = 'C1'
    getattr(entry, kind).scale_logits = True
    est = EasyRecEstimator(cfg, device=DEV, batch_size=192, seed=11).build()
    gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=192, seed=111)
    est.train_step(gen.next_batch())  # (one eager step before a capture: lazily created workspaces exist)
    if graph:
      est.capture(warmup=0)
    seen = []
    for _ in range(3):
      est.train_step(gen.next_batch())
      seen.append(est.loss_values())
    assert (est.graph is not None) == graph and kind in seen[0] and np.isfinite(seen[-1][kind])
    sd = est.state_dict()
    scope = lwl.SCOPES[entry.loss_type]
    assert float(sd[scope + '/scale_w'][0]) != 1.0  # (trained; scale_b's gradient is zero: softmax is shift invariant)
    losses[graph] = seen
  assert losses[True] == losses[False], (losses[True], losses[False])
