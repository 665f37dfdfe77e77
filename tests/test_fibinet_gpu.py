"""FiBiNet's HIP field kernels (csrc/er_fibinet.hip) on the GPU: forward and every gradient against the fp64 torch
restatement (oracle/fibinet_ref.py) and the reference's own outputs (tests/golden/fibinet_vectors.npz), the max's tie
rule, the composed path outside the envelope, bit-identity (two runs, eager vs hipGraph replay), and the model against
the oracle."""
import logging
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.layers.keras import fibinet as fb  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from oracle import fibinet_ref as ref  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical, first_steps  # noqa: E402
from tests._oracle_steps import close as _close  # noqa: E402
from tests.test_fibinet_pins import GOLD, GOLD_CASES, fibinet_cfg, gold_case  # noqa: E402

logging.disable(logging.WARNING)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
PATTERN_TOL = 1e-5  # where the kernels' ReLU / arg-max pattern may differ from fp64's: within this of a tie


# ---------------------------------------------------------------------------------------- bilinear
# (B, F, D, kind, plus): the sample's geometry at B = 4096, B not a multiple of the 8 examples per workgroup round,
# odd F / odd D, `all` and `each`, plus and not
BILINEAR_CASES = [
    (4096, 17, 16, 'each', True),
    (301, 17, 16, 'each', False),
    (77, 17, 16, 'all', True),
    (13, 7, 5, 'each', True),
    (9, 5, 3, 'all', False),
    (5, 2, 8, 'each', True),
]


def _bilinear_product(x, ws, F, D, kind, plus):
  grads = [torch.zeros_like(w) for w in ws]
  return kernels.BiLinearFn.apply(x, F, D, kind == 'each', plus, grads, *ws), grads


def _check_bilinear(x64, p64, F, D, kind, plus, seed, run=_bilinear_product):
  names = ref.bilinear_names('b', kind, F)
  x = x64.to(DEV, torch.float32).requires_grad_(True)
  out, grads = run(x, [p64[n].to(DEV, torch.float32) for n in names], F, D, kind, plus)
  d64 = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
  out.backward(d64.to(DEV, torch.float32))
  torch.cuda.synchronize()
  xr = x64.clone().requires_grad_(True)
  pr = {n: v.clone().requires_grad_(True) for n, v in p64.items()}
  exp = ref.bilinear_pairs(ref.split(xr, F, D), kind, plus, pr, 'b')
  (exp * d64).sum().backward()
  _close(out, exp, 1e-5, 'forward')
  _close(x.grad, xr.grad, 1e-4, 'dx')
  for n, g in zip(names, grads):
    _close(g, pr[n].grad, 1e-4, n)


@pytest.mark.parametrize('case', BILINEAR_CASES, ids=lambda c: 'B%d_F%d_D%d_%s_plus%d' % c)
def test_bilinear_matches_the_fp64_restatement(case):
  B, F, D, kind, plus = case
  assert fb.bilinear_fits(F, D)
  x64, p64 = ref.random_bilinear(B, F, D, kind, seed=B + F)
  _check_bilinear(x64, p64, F, D, kind, plus, seed=3)


# ---------------------------------------------------------------------------------------- SENet
# (B, F, D, G, ratio, skip, ln): the sample's at B = 4096, B not a multiple of the 7 / 8 examples per round, odd
# widths, one group, every option off and on
SENET_CASES = [
    (4096, 17, 16, 2, 4, True, True),
    (303, 17, 16, 2, 4, True, False),
    (61, 17, 16, 1, 4, False, True),
    (13, 7, 6, 2, 4, False, False),
    (9, 5, 3, 3, 2, True, True),
    (5, 3, 5, 1, 8, True, True),
]


def _senet_product(x, ps, F, D, G, R, skip, ln):
  grads = [torch.zeros_like(p) for p in ps]
  return kernels.SENetFn.apply(x, F, D, G, R, skip, ln, grads, *ps), grads


def _licence(x64, p64, F, D, G, a1, x32):
  """The kernels' own ReLU pattern and arg-max choice, CHECKED against fp64's: where they differ, the fp64
  pre-activation lies within PATTERN_TOL of zero relative to the largest one (for the max: the two candidates within
  that distance of each other)."""
  pre = ref.senet_pre(ref.split(x64, F, D), G, p64, 's')
  mask = (a1.double().cpu() > 0).to(torch.float64)
  differ = mask != (pre > 0).to(torch.float64)
  lim = PATTERN_TOL * float(pre.abs().max())
  assert float(pre[differ].abs().max() if differ.any() else 0.0) <= lim, 'ReLU pattern differs away from zero'
  w32 = ref.max_weight_of(x32.double().cpu(), F, D, G)  # (exact comparisons of fp32 inputs: what the kernel does)
  w64 = ref.max_weight_of(x64, F, D, G)
  B = x64.shape[0]
  g64 = x64.reshape(B, F * G, D // G)
  gap = (g64.amax(dim=-1, keepdim=True) - g64).reshape(B, F * D)  # distance of each column from its group's maximum
  chosen = (w32 > 0) != (w64 > 0)
  assert float(gap[chosen].max() if chosen.any() else 0.0) <= PATTERN_TOL * float(x64.abs().max()), \
      'arg-max choice differs away from a tie'
  return mask, w32


def _check_senet(x64, p64, F, D, G, R, skip, ln, seed, run=_senet_product):
  names = ref.senet_names('s', ln)
  x = x64.to(DEV, torch.float32).requires_grad_(True)
  ps = [p64[n].to(DEV, torch.float32) for n in names]
  y, grads = run(x, ps, F, D, G, R, skip, ln)
  d64 = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
  y.backward(d64.to(DEV, torch.float32))
  be = kernels.hip()
  theta = torch.cat([p.reshape(-1) for p in ps])
  if fb.senet_fits(F, D, G, R):
    _, a1 = be.senet_fwd(x.detach(), theta, F, D, G, R, skip, ln, want_a1=True)
  else:  # the composed path: its own hidden layer
    a1 = torch.relu(ref.senet_pre(ref.split(x.detach(), F, D), G, dict(zip(names, ps)), 's'))
  torch.cuda.synchronize()
  mask, w32 = _licence(x64, p64, F, D, G, a1, x.detach())
  xr = x64.clone().requires_grad_(True)
  pr = {n: v.clone().requires_grad_(True) for n, v in p64.items()}
  exp = ref.senet(ref.split(x64, F, D), G, p64, 's', skip, ln)
  (ref.senet(ref.split(xr, F, D), G, pr, 's', skip, ln, relu_mask=mask, max_weight=w32) * d64).sum().backward()
  _close(y, exp, 1e-5, 'forward')
  _close(x.grad, xr.grad, 1e-4, 'dx')
  for n, g in zip(names, grads):
    _close(g, pr[n].grad, 1e-4, n)


@pytest.mark.parametrize('case', SENET_CASES, ids=lambda c: 'B%d_F%d_D%d_G%d_r%d_skip%d_ln%d' % c)
def test_senet_matches_the_fp64_restatement(case):
  B, F, D, G, ratio, skip, ln = case
  R = fb.senet_reduction(F, G, ratio)
  assert fb.senet_fits(F, D, G, R)
  x64, p64 = ref.random_senet(B, F, D, G, R, ln, seed=B + F + G)
  _check_senet(x64, p64, F, D, G, R, skip, ln, seed=5)


def test_senet_splits_the_gradient_of_a_tied_max_evenly():
  """TensorFlow's reduce_max: the gradient goes to every column that equals the maximum, divided by their count."""
  B, F, D, G, R = 3, 2, 4, 1, 2
  x64, p64 = ref.random_senet(B, F, D, G, R, False, seed=1)
  x64 = x64.float().double()
  x64[0, 0] = x64[0, 2] = x64[0, :4].max() + 1.0   # two tied maxima in example 0, field 0
  x64[1, 4:8] = 0.25                                # four in example 1, field 1
  x = x64.to(DEV, torch.float32).requires_grad_(True)
  names = ref.senet_names('s', False)
  ps = [p64[n].to(DEV, torch.float32) for n in names]
  y, _ = _senet_product(x, ps, F, D, G, R, False, False)
  d64 = torch.randn(B, F * D, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
  y.backward(d64.to(DEV, torch.float32))
  torch.cuda.synchronize()
  # hand-made expectation: d(loss)/d(max of the group) split over the ties, beside the other paths' share
  xr = x64.clone().requires_grad_(True)
  w = ref.max_weight_of(x64, F, D, G)
  assert w[0, 0] == 0.5 and w[0, 2] == 0.5 and w[0, 1] == 0.0 and bool((w[1, 4:8] == 0.25).all())
  pre = ref.senet_pre(ref.split(x64, F, D), G, p64, 's')
  mask = (pre > 0).to(torch.float64)
  (ref.senet(ref.split(xr, F, D), G, p64, 's', False, False, relu_mask=mask, max_weight=w) * d64).sum().backward()
  _close(x.grad, xr.grad, 1e-4, 'dx with ties')
  # and torch.amax, whose rule is the same, agrees without being told the choice
  xa = x64.clone().requires_grad_(True)
  (ref.senet(ref.split(xa, F, D), G, p64, 's', False, False) * d64).sum().backward()
  _close(x.grad, xa.grad, 1e-4, 'dx against amax')


# ---------------------------------------------------------------------------------------- the reference's own outputs
@pytest.mark.parametrize('tag', GOLD_CASES)
def test_kernels_match_the_reference_fixture(tag):
  pb, B, F, D, x64, var = gold_case(tag)
  se = pb.senet
  G, skip, ln = int(se.num_squeeze_group), bool(se.use_skip_connection), bool(se.use_output_layer_norm)
  R = fb.senet_reduction(F, G, int(se.reduction_ratio))
  p64 = {n.replace('fibinet/senet', 's'): v for n, v in var.items() if n.startswith('fibinet/senet/')}
  x = x64.to(DEV, torch.float32).requires_grad_(True)
  names = ref.senet_names('s', ln)
  y, grads = _senet_product(x, [p64[n].to(DEV, torch.float32) for n in names], F, D, G, R, skip, ln)
  _close(y, torch.from_numpy(GOLD['%s:senet' % tag]), 1e-5, (tag, 'senet'))
  _check_senet(x64, p64, F, D, G, R, skip, ln, seed=7)
  if pb.HasField('bilinear'):
    kind, plus = pb.bilinear.type, bool(pb.bilinear.use_plus)
    b64 = {n.replace('fibinet/bilinear', 'b'): v for n, v in var.items() if n.startswith('fibinet/bilinear/')}
    bn = ref.bilinear_names('b', kind, F)
    p, _ = _bilinear_product(x64.to(DEV, torch.float32), [b64[n].to(DEV, torch.float32) for n in bn], F, D, kind, plus)
    out = p.double().cpu() @ b64['b/output/kernel'] + b64['b/output/bias']
    _close(out, torch.from_numpy(GOLD['%s:bilinear' % tag]), 1e-5, (tag, 'bilinear'))
    _check_bilinear(x64, {n: b64[n] for n in bn}, F, D, kind, plus, seed=8)


# ---------------------------------------------------------------------------------------- outside the envelope
def test_geometry_outside_the_envelope_takes_the_composition():
  F, D, G, ratio = 40, 32, 2, 4
  R = fb.senet_reduction(F, G, ratio)
  assert not fb.senet_fits(F, D, G, R) and not fb.bilinear_fits(F, D)
  assert kernels.hip().senet_epb(F, D, G, R, True, True) == 0 and kernels.hip().bilinear_epb(F, D, True) == 0

  def senet_run(x, ps, F, D, G, R, skip, ln):
    for p in ps:
      p.requires_grad_(True)
    y = fb.senet_compose(ref.split(x, F, D), G, ps[0], ps[1], ps[2], ps[3], skip, *(ps[4:] if ln else ()))
    return y, _LazyGrads(ps)

  def bilinear_run(x, ws, F, D, kind, plus):
    for w in ws:
      w.requires_grad_(True)
    return fb.bilinear_compose(x, F, D, ws[0::2], ws[1::2], plus), _LazyGrads(ws)

  x64, p64 = ref.random_senet(33, F, D, G, R, True, seed=11)
  _check_senet(x64, p64, F, D, G, R, True, True, seed=12, run=senet_run)
  x64, p64 = ref.random_bilinear(33, F, D, 'each', seed=13)
  _check_bilinear(x64, p64, F, D, 'each', True, seed=14, run=bilinear_run)


class _LazyGrads(object):
  """The parameters' autograd gradients, read after backward."""

  def __init__(self, ps):
    self.ps = ps

  def __iter__(self):
    return iter([p.grad for p in self.ps])


def test_the_blocks_pick_the_path_by_the_envelope(monkeypatch):
  calls = []
  real_s, real_b = kernels.SENetFn.apply, kernels.BiLinearFn.apply
  monkeypatch.setattr(kernels.SENetFn, 'apply', lambda *a: calls.append('senet') or real_s(*a))
  monkeypatch.setattr(kernels.BiLinearFn, 'apply', lambda *a: calls.append('bilinear') or real_b(*a))
  B = 32
  cfg = fibinet_cfg(batch_size=B)
  est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=3).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=5)
  est.train_step(gen.next_batch())
  assert 'senet' in calls and 'bilinear' in calls


# ---------------------------------------------------------------------------------------- bit identity
def test_two_runs_and_graph_replay_are_bit_identical():
  B, F, D, G = 1001, 17, 16, 2
  R = fb.senet_reduction(F, G, 4)
  x64, s64 = ref.random_senet(B, F, D, G, R, True, seed=5)
  _, b64 = ref.random_bilinear(B, F, D, 'each', seed=6)
  x = x64.to(DEV, torch.float32)
  sp = [s64[n].to(DEV, torch.float32) for n in ref.senet_names('s', True)]
  bp = [b64[n].to(DEV, torch.float32) for n in ref.bilinear_names('b', 'each', F)]
  sg, bg = [torch.zeros_like(p) for p in sp], [torch.zeros_like(p) for p in bp]
  dy = torch.randn(B, F * D, device=DEV)
  dp = torch.randn(B, F * (F - 1) // 2, device=DEV)

  def run():
    for g in sg + bg:
      g.zero_()
    xi = x.detach().requires_grad_(True)
    y = kernels.SENetFn.apply(xi, F, D, G, R, True, True, sg, *sp)
    p = kernels.BiLinearFn.apply(xi, F, D, True, True, bg, *bp)
    torch.autograd.backward([y, p], [dy, dp])
    return [y.detach(), p.detach(), xi.grad] + [g.clone() for g in sg + bg]

  assert_runs_and_replay_bit_identical(run)


# ---------------------------------------------------------------------------------------- the model against the oracle
def _coverage(names, cfg):
  fbn = cfg.model_config.backbone.blocks[1].keras_layer.fibinet
  n_se = sum(k.startswith('fibinet/senet/') for k in names)
  n_bi = sum(k.startswith('fibinet/bilinear/') for k in names)
  n_bn = sum(k.startswith('batch_normalization_') for k in names)
  n_emb = sum('embedding_weights' in k for k in names)
  n_w = 0 if not fbn.HasField('bilinear') else (1 if fbn.bilinear.type == 'all' else 16)
  assert n_se == 6 and n_bi == (2 * n_w + 2 if n_w else 0) and n_bn == 2 * 17 and n_emb >= 2, \
      (len(names), n_se, n_bi, n_bn, n_emb)


def _first_steps(cfg, B, seed, **kw):
  return first_steps(cfg, B, seed, skip_bn_shadowed_bias=False, coverage=_coverage, **kw)


@pytest.mark.parametrize('kind', ['each', 'all', None])
def test_model_matches_the_oracle(kind):
  """B = 128, two steps, the sample's model section on small tables; with `each`, with `all`, without bilinear."""
  _first_steps(fibinet_cfg(bilinear_type=kind, batch_size=128), 128, 21)


def test_full_size_config_matches_the_oracle():
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'fibinet_taobao_10m.config'))
  _first_steps(cfg, 4096, 8, step0_tol=1e-4)


def test_evaluate_returns_an_auc():
  B = 128
  cfg = fibinet_cfg(batch_size=B)
  est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=3).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=103)
  for _ in range(3):
    est.train_step(gen.next_batch())
  res = est.evaluate([gen.next_batch() for _ in range(3)])
  assert 'auc' in res and 0.0 <= float(res['auc']) <= 1.0, res
