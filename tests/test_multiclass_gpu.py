"""The multi-logit head kernels (csrc/er_multiclass.hip) on the GPU, through the C ABI, against fp64 torch autograd
restatements written here: er_softmax_ce at every lane geometry (one lane per row up to 64 lanes per row, one and several
workgroups, a pitch wider than the row), with and without weights, with saturating logits, exact ties, labels outside the
row and forward-only launches; er_jrc against the reference's literal [B, B] form over every session layout; bit identity
(two runs, a hipGraph replay, the multi-head launch); the envelope's refusals; and estimator steps on the kernels against
the same steps on the torch compositions.

Bars: 1e-5 of the largest expected value on forward values, 1e-4 on gradients; where the fp32 formula itself misses
those (printed per case), four times the fp32 torch composition's own measured error on the same inputs."""
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.builders import multiclass_loss as mcl  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402

logging.disable(logging.WARNING)
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = 'EASYREC_AMD_FUSED_MULTICLASS'
PAD = 3  # columns of a wider tensor in front of and behind the logits: a pitch above C, a base off the 16-byte grid
SCALE = 0.75

SMC_SHAPES = [(B, C) for B in (1, 7, 64, 65, 257) for C in (2, 3, 5, 33, 64, 65, 130)] + [(7, 4096)]
WEIGHTS = ('none', 'zeros', 'all_zero')


def _rel(got, want):
  return float((got.double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _hold(got, want, base, comp, what):
  """max |got - want| <= max(base, 4 x the composition's error) * max |want|"""
  err = _rel(got, want)
  print('    %-10s kernel %.2e composition %.2e' % (what, err, comp))
  assert err <= max(base, 4.0 * comp), (what, err, comp)


def _weights(kind, B, rng):
  if kind == 'none':
    return None
  if kind == 'all_zero':
    return torch.zeros(B, dtype=torch.float64)
  w = torch.from_numpy(np.round(rng.random(B) * 2, 2) + 0.25)
  w[torch.from_numpy(rng.random(B) < 0.3)] = 0.0
  return w


# ----------------------------------------------------------------------------------- softmax cross entropy
def _smc_reference(z, y, w, dtype):
  """tf.losses.sparse_softmax_cross_entropy and the head's predictions, op by op with autograd -> (loss, dz, probs,
  logits_y, probs_y)"""
  z = z.to(dtype).clone().requires_grad_(True)
  lse = torch.logsumexp(z, dim=1)
  ce = lse - z.gather(1, y.reshape(-1, 1)).squeeze(1)
  if w is None:
    loss = SCALE * ce.sum() / z.shape[0]
  else:
    loss = SCALE * (w.to(dtype) * ce).sum() / max(float((w != 0).sum()), 1.0)
  dz, = torch.autograd.grad(loss, z)
  probs = torch.softmax(z.detach(), dim=1)
  return loss.detach().reshape(1), dz, probs, z.detach().max(dim=1).values, probs.max(dim=1).values


def _stable_order(z, y):
  """(first argmax, the label's place in the stable descending order) by numpy"""
  zn, yn = z.numpy(), y.numpy()
  order = np.argsort(-zn, axis=1, kind='stable')
  rank = np.array([int(np.nonzero(order[r] == yn[r])[0][0]) for r in range(zn.shape[0])])
  return order[:, 0], rank


def _launch_smc(z, y, w, want_grad=True, want_fwd=True, pad=PAD):
  """er_softmax_ce through the C ABI on a column slice of a wider tensor -> dict of outputs (loss = the partials' sum)"""
  be = kernels.hip()
  B, C = z.shape
  wide = torch.full((B, C + 2 * pad), 1e30, device=DEV)
  wide[:, pad:pad + C] = z.to(DEV, torch.float32)
  zs = wide[:, pad:pad + C]
  yd = None if y is None else y.to(DEV, torch.float32)
  wd = None if w is None else w.to(DEV, torch.float32)
  grid = be.softmax_ce_grid(B, C)
  assert grid >= 1
  f = lambda *s: torch.full(s, float('nan'), device=DEV)  # noqa: E731
  o = {'probs': f(B, C + pad) if want_fwd else None, 'y': torch.full((B,), -7, dtype=torch.int64, device=DEV) if want_fwd else None,
       'logits_y': f(B) if want_fwd else None, 'probs_y': f(B) if want_fwd else None,
       'dz': f(B, C + 1) if want_grad else None, 'rank': torch.full((B,), -7, dtype=torch.int32, device=DEV) if y is not None else None,
       'partials': f(grid) if want_grad else None}
  p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
  be.ck.er_softmax_ce(zs.data_ptr(), zs.stride(0), p(yd), p(wd), B, C, SCALE, p(o['probs']), C + pad, p(o['y']),
                      p(o['logits_y']), p(o['probs_y']), p(o['dz']), C + 1, p(o['rank']), p(o['partials']),
                      torch.cuda.current_stream().cuda_stream)
  torch.cuda.synchronize()
  if want_fwd:
    assert bool(torch.isnan(o['probs'][:, C:]).all())  # nothing written past the row
    o['probs'] = o['probs'][:, :C]
  if want_grad:
    assert bool(torch.isnan(o['dz'][:, C:]).all())
    o['dz'] = o['dz'][:, :C]
    o['loss'] = o['partials'].double().sum().reshape(1)
  return o


def _check_smc(z, y, w, label=''):
  want = _smc_reference(z, y, w, torch.float64)
  comp = [_rel(a, b) for a, b in zip(_smc_reference(z, y, w, torch.float32), want)]
  o = _launch_smc(z, y, w)
  print('  %s B %d C %d' % (label, z.shape[0], z.shape[1]))
  for t in (o['loss'], o['dz'], o['probs'], o['logits_y'], o['probs_y']):
    assert bool(torch.isfinite(t).all())
  _hold(o['loss'], want[0], 1e-5, comp[0], 'loss')
  _hold(o['dz'], want[1], 1e-4, comp[1], 'dlogits')
  _hold(o['probs'], want[2], 1e-5, comp[2], 'probs')
  _hold(o['logits_y'], want[3], 1e-5, comp[3], 'logits_y')
  _hold(o['probs_y'], want[4], 1e-5, comp[4], 'probs_y')
  first, rank = _stable_order(z, y)
  assert np.array_equal(o['y'].cpu().numpy(), first)
  assert np.array_equal(o['rank'].cpu().numpy(), rank)
  return o


def _smc_inputs(B, C, seed=0):
  rng = np.random.default_rng(1000 * B + C + seed)
  z = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32) * 2.0).double()
  y = torch.from_numpy(rng.integers(0, C, size=B))
  return z, y, rng


@pytest.mark.parametrize('B,C', SMC_SHAPES, ids=lambda v: str(v))
def test_softmax_ce_against_fp64(B, C):
  z, y, rng = _smc_inputs(B, C)
  for kind in WEIGHTS:
    w = _weights(kind, B, rng)
    o = _check_smc(z, y, w, kind)
    if kind == 'all_zero':  # loss 0 and a zero gradient, not 0 / 0
      assert float(o['loss']) == 0.0 and float(o['dz'].abs().max()) == 0.0


@pytest.mark.parametrize('B,C', [(7, 3), (65, 5), (7, 33), (65, 130)], ids=lambda v: str(v))
def test_softmax_ce_saturating_logits_and_ties(B, C):
  z, y, rng = _smc_inputs(B, C, seed=1)
  z[0, 0], z[0, C - 1] = 80.0, -80.0  # +-80 in one row
  z[B - 1, :] = -80.0
  z[B - 1, C // 2] = 80.0
  _check_smc(z, y, None, 'saturating')
  # exact ties: whole rows equal, the maximum held twice, the label's value held before and after it
  z, y, rng = _smc_inputs(B, C, seed=2)
  z[0, :] = 0.5
  z[B // 2, :] = torch.from_numpy(rng.integers(-1, 2, size=C).astype(np.float64))
  z[B - 1, 0] = z[B - 1, C - 1] = float(z[B - 1].max()) + 1.0
  for r in range(B):
    z[r, (int(y[r]) + 1) % C] = z[r, int(y[r])]
  _check_smc(z, y, _weights('zeros', B, rng), 'ties')


def test_softmax_ce_forward_only_and_labels_outside_the_row():
  B, C = 65, 5
  z, y, rng = _smc_inputs(B, C, seed=3)
  full = _launch_smc(z, y, None)
  fwd = _launch_smc(z, y, None, want_grad=False)  # evaluation: no dlogits, no loss
  for k in ('probs', 'y', 'logits_y', 'probs_y', 'rank'):
    assert torch.equal(full[k], fwd[k]), k
  pred = _launch_smc(z, None, None, want_grad=False)  # prediction: no labels at all
  for k in ('probs', 'y', 'logits_y', 'probs_y'):
    assert torch.equal(full[k], pred[k]), k
  grad = _launch_smc(z, y, None, want_fwd=False)  # training without the predictions
  assert torch.equal(full['dz'], grad['dz']) and torch.equal(full['partials'], grad['partials'])
  # labels outside [0, C), NaN included: the row adds nothing to the loss, zero dlogits, rank C; nz still counts it
  bad = y.double().clone()
  bad[0], bad[7], bad[B - 1] = -1.0, float(C), float('nan')
  keep = torch.ones(B, dtype=torch.float64)
  keep[[0, 7, B - 1]] = 0.0
  o = _launch_smc(z, bad, None)
  ce = torch.logsumexp(z, 1) - z.gather(1, y.reshape(-1, 1)).squeeze(1)
  want = SCALE * (keep * ce).sum() / B
  assert abs(float(o['loss']) - float(want)) <= 1e-5 * float(want)
  assert float(o['dz'][[0, 7, B - 1]].abs().max()) == 0.0
  assert o['rank'][[0, 7, B - 1]].tolist() == [C, C, C]
  assert bool(torch.isfinite(o['dz']).all()) and torch.equal(o['probs'], full['probs'])


def test_softmax_ce_refusals():
  be = kernels.hip()
  assert be.softmax_ce_grid(8, 1) == 0 and be.softmax_ce_grid(8, 4097) == 0 and be.softmax_ce_grid(0, 4) == 0
  assert be.jrc_grid(0) == 0 and be.jrc_grid(8193) == 0 and be.jrc_grid(8192) == 32
  z = torch.zeros(8, 4, device=DEV)
  y = torch.zeros(8, device=DEV)
  part = torch.zeros(4, device=DEV)
  s = torch.cuda.current_stream().cuda_stream
  call = be.lib.er_softmax_ce
  assert call(z.data_ptr(), 4, y.data_ptr(), None, 8, 1, 1.0, None, 0, None, None, None, None, 0, None, part.data_ptr(), s) == 2
  assert call(z.data_ptr(), 3, y.data_ptr(), None, 8, 4, 1.0, None, 0, None, None, None, None, 0, None, part.data_ptr(), s) == 2
  assert call(z.data_ptr(), 4, None, None, 8, 4, 1.0, None, 0, None, None, None, None, 0, None, part.data_ptr(), s) == 2
  keys = torch.zeros(8, dtype=torch.int64, device=DEV)
  assert be.lib.er_jrc(z.data_ptr(), 1, y.data_ptr(), keys.data_ptr(), None, 8, 0.5, 1.0, 1.0, part.data_ptr(), None, 0, None, s) == 2
  assert be.lib.er_jrc(z.data_ptr(), 4, y.data_ptr(), keys.data_ptr(), None, 8193, 0.5, 1.0, 1.0, part.data_ptr(), None, 0, None, s) == 2
  torch.cuda.synchronize()


def test_softmax_ce_bits():
  """two launches and a hipGraph replay give the same bits; the multi-head launch gives the single-head launch's"""
  be = kernels.hip()
  heads = []
  for B, C, weighted in ((257, 5, True), (65, 130, False), (64, 2, True)):
    z, y, rng = _smc_inputs(B, C, seed=4)
    w = _weights('zeros', B, rng) if weighted else None
    heads.append((z.to(DEV, torch.float32), y.to(DEV, torch.float32), None if w is None else w.to(DEV, torch.float32), SCALE))
  want = ('loss', 'dlogits', 'probs', 'y', 'logits_y', 'probs_y', 'label_rank')
  keys = ('loss_partials', 'dlogits', 'probs', 'y', 'logits_y', 'probs_y', 'label_rank')

  def run():
    return [be.softmax_ce(*heads[0], want=want)[k] for k in keys]
  assert_runs_and_replay_bit_identical(run)
  single = [be.softmax_ce(*h) for h in heads]
  multi = be.softmax_ce_multi(heads)
  torch.cuda.synchronize()
  for a, b in zip(single, multi):
    for k in ('loss_partials', 'dlogits', 'probs'):
      assert torch.equal(a[k], b[k]), k


# ----------------------------------------------------------------------------------------------------- JRC
def _jrc_reference(z, y, keys, w, alpha, dtype):
  """reference loss/jrc_loss.py with same_label_loss, literally: [B, B] masks, -1e9 on the masked logits"""
  z = z.to(dtype).clone().requires_grad_(True)
  B = z.shape[0]
  lse = torch.logsumexp(z, dim=1)
  ce = lse - z.gather(1, y.reshape(-1, 1)).squeeze(1)
  ce = ce.sum() / B if w is None else (w.to(dtype) * ce).sum() / max(float((w != 0).sum()), 1.0)
  onehot = torch.stack([1 - y, y], dim=1).to(dtype)
  mask = (keys.reshape(-1, 1) == keys.reshape(1, -1)).to(dtype)
  zz = z.unsqueeze(1).expand(B, B, 2) + (1 - mask.unsqueeze(2)) * -1e9
  yy = onehot.unsqueeze(1).expand(B, B, 2) * mask.unsqueeze(2)
  if w is not None:
    yy = yy * w.to(dtype).reshape(1, B, 1)
  loss_pos = -(yy[:, :, 1] * torch.log_softmax(zz[:, :, 1], dim=0)).sum(dim=0)
  loss_neg = -(yy[:, :, 0] * torch.log_softmax(zz[:, :, 0], dim=0)).sum(dim=0)
  ge = ((loss_pos + loss_neg) / mask.sum(dim=0)).mean()
  loss = SCALE * (alpha * ce + (1 - alpha) * ge)
  dz, = torch.autograd.grad(loss, z)
  return loss.detach().reshape(1), dz, torch.softmax(z.detach(), dim=1)[:, 1]


def _launch_jrc(z, y, keys, w, alpha, pad=PAD):
  be = kernels.hip()
  B = z.shape[0]
  wide = torch.full((B, 2 + 2 * pad), 1e30, device=DEV)
  wide[:, pad:pad + 2] = z.to(DEV, torch.float32)
  zs = wide[:, pad:pad + 2]
  grid = be.jrc_grid(B)
  part = torch.full((grid,), float('nan'), device=DEV)
  dz = torch.full((B, 3), float('nan'), device=DEV)
  probs = torch.full((B,), float('nan'), device=DEV)
  yd, kd = y.to(DEV, torch.float32), keys.to(DEV)
  wd = None if w is None else w.to(DEV, torch.float32)
  be.ck.er_jrc(zs.data_ptr(), zs.stride(0), yd.data_ptr(), kd.data_ptr(), None if wd is None else wd.data_ptr(), B, alpha,
               1.0, SCALE, part.data_ptr(), dz.data_ptr(), 3, probs.data_ptr(), torch.cuda.current_stream().cuda_stream)
  torch.cuda.synchronize()
  assert bool(torch.isnan(dz[:, 2]).all())
  return part.double().sum().reshape(1), dz[:, :2], probs


def _jrc_keys(layout, B, rng):
  if layout == 'distinct':
    return torch.from_numpy(rng.permutation(B).astype(np.int64))
  if layout == 'equal':
    return torch.full((B,), 42, dtype=torch.int64)
  if layout == 'high_bits':  # keys that differ only above bit 32, and negative keys
    k = torch.from_numpy(rng.integers(0, 3, size=B).astype(np.int64))
    return torch.where(k == 2, torch.full_like(k, -5), 7 + (k << 40))
  # mixed sizes; one session holds the first and the last example
  k = torch.from_numpy(rng.integers(1, max(B // 3, 2), size=B).astype(np.int64))
  k[0] = k[B - 1] = 0
  return k


JRC_CASES = [(B, layout) for B in (1, 2, 65, 257, 300) for layout in ('distinct', 'equal', 'mixed', 'high_bits')]


@pytest.mark.parametrize('B,layout', JRC_CASES, ids=lambda v: str(v))
def test_jrc_against_the_literal_form(B, layout):
  rng = np.random.default_rng(B * 31 + len(layout))
  keys = _jrc_keys(layout, B, rng)
  z = torch.from_numpy(rng.standard_normal((B, 2)).astype(np.float32) * 2.0).double()
  y = torch.from_numpy((rng.random(B) < 0.4).astype(np.int64))
  if layout == 'mixed' and B >= 65:
    y[keys == 1] = 1  # an all-positive session
    y[keys == 2] = 0  # an all-negative session
    members = torch.nonzero(keys == 3).reshape(-1)
    if len(members) >= 2:  # logits 100 apart inside one session
      z[members[0]] = torch.tensor([50.0, -50.0], dtype=torch.float64)
      z[members[1]] = torch.tensor([-50.0, 50.0], dtype=torch.float64)
  if layout == 'equal' and B >= 2:
    z[0, 1], z[B - 1, 1] = 60.0, -40.0
  for kind, alpha in (('none', 0.5), ('zeros', 0.3)):
    w = _weights(kind, B, rng)
    want = _jrc_reference(z, y, keys, w, alpha, torch.float64)
    comp = [_rel(a, b) for a, b in zip(_jrc_reference(z, y, keys, w, alpha, torch.float32), want)]
    loss, dz, probs = _launch_jrc(z, y, keys, w, alpha)
    print('  %s alpha %.1f B %d %s' % (kind, alpha, B, layout))
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dz).all())
    _hold(loss, want[0], 1e-5, comp[0], 'loss')
    _hold(dz, want[1], 1e-4, comp[1], 'dlogits')
    _hold(probs, want[2], 1e-5, comp[2], 'probs')


def test_jrc_bits():
  be = kernels.hip()
  rng = np.random.default_rng(5)
  B = 300
  z = torch.randn(B, 2, device=DEV)
  y = torch.from_numpy((rng.random(B) < 0.4).astype(np.float32)).to(DEV)
  keys = _jrc_keys('mixed', B, rng).to(DEV)
  w = _weights('zeros', B, rng).to(DEV, torch.float32)

  def run():
    o = be.jrc(z, y, keys, w, 0.3, ce_scale=1.0, loss_scale=SCALE)
    return [o['loss_partials'], o['dlogits'], o['probs']]
  assert_runs_and_replay_bit_identical(run)


def test_jrc_scalar_weight_is_applied_twice_to_the_cross_entropy():
  """loss_builder on the kernel against the composition with a python-scalar weight (jrc_loss.py:39-40, :126-127)"""
  rng = np.random.default_rng(6)
  B = 65
  z = torch.randn(B, 2, device=DEV)
  y = torch.from_numpy((rng.random(B) < 0.4).astype(np.int64)).to(DEV)
  keys = _jrc_keys('mixed', B, rng).to(DEV)
  loss, dz, extras = mcl.jrc(y, z, keys, 2.5, 0.8, 0.3, True)
  assert extras is not None
  total = extras['loss_partials'].double().sum()
  zr = z.double().clone().requires_grad_(True)
  want = mcl.jrc_compose(y, zr, keys, 0.3, 2.5, True) * 0.8
  gw, = torch.autograd.grad(want, zr)
  assert abs(float(total) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
  assert _rel(dz, gw.cpu()) <= 1e-4


# ------------------------------------------------------------------------------------------ estimator steps
def _two_steps(name, B, label_classes, fused):
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', name))
  for fc in list(cfg.feature_config.features) + list(cfg.feature_configs):
    if fc.hash_bucket_size > 1000:
      fc.hash_bucket_size = 1000
  before = os.environ.get(SWITCH)
  os.environ[SWITCH] = '1' if fused else '0'
  be, calls = kernels.hip(), []
  for fn in ('softmax_ce', 'softmax_ce_multi', 'jrc'):  # count the launches of the head kernels
    setattr(be, fn, (lambda inner, fn=fn: lambda *a, **k: (calls.append(fn), inner(*a, **k))[1])(getattr(be, fn)))
  try:
    est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=11).build()
    gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=111, label_classes=label_classes)
    losses = []
    for _ in range(2):
      est.train_step(gen.next_batch())
      losses.append(est.loss_values())
      if len(losses) == 1:
        first = {k: v for k, v in est.state_dict(slots=True).items() if k.endswith('/m')}
    return losses, first, calls
  finally:
    for fn in ('softmax_ce', 'softmax_ce_multi', 'jrc'):
      delattr(be, fn)  # (the instance attribute: the class's method shows again)
    if before is None:
      del os.environ[SWITCH]
    else:
      os.environ[SWITCH] = before


@pytest.mark.parametrize('name,B,label_classes', [('deepfm_multicls_criteo.config', 192, {'label': 5}),
                                                  ('dbmtl_jrc_small_taobao.config', 128, None)])
def test_estimator_on_the_kernels_against_the_compositions(name, B, label_classes):
  """two steps each way; tests/_oracle_steps.first_steps' bars: every loss 1e-5 (first step) / 1e-4 (second) of
  max(1e-3, |expected|), every variable's first moment after the first step 2e-4 of its own scale + 2e-6 of the largest"""
  got, got_m, launched = _two_steps(name, B, label_classes, True)
  want, want_m, composed = _two_steps(name, B, label_classes, False)
  assert len(launched) == 2 and not composed, (launched, composed)  # one head launch per step; none with the switch at 0
  for step, tol in ((0, 1e-5), (1, 1e-4)):
    assert set(got[step]) == set(want[step])
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
