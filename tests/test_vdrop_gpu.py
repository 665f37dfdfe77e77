"""The variational dropout kernel (csrc/er_vdrop.hip) on the GPU: forward, penalty and every gradient against fp64
autograd of the restatement in tests/_vdrop_cases.py, fed the same noise; embedding-wise and feature-wise; training and
evaluation; without the input gradient; on a column slice of a wider tensor; with dlogit_p added into a given buffer and
returned; saturated probabilities; bit identity (two runs, eager vs hipGraph replay); the envelope's refusals; the layer
on the kernel against the torch composition; DeepFM and FM steps with the switch at 1 and at 0; the mask's mean."""
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.core import context  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.layers import variational_dropout_layer as vdl  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.protos import variational_dropout_pb2  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from tests import _vdrop_cases as vc  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402
from tests._oracle_steps import close as _close  # noqa: E402
from tests._uniter_cases import product_store  # noqa: E402

logging.disable(logging.WARNING)
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = 'EASYREC_AMD_FUSED_VDROP'
FILL = 0.25  # what a given dlogit_p buffer holds before the backward adds into it
PAD = 3      # columns in front of a slice: base and pitch off the 16-byte grid
CASES = [(B, dims, mode) for B, dims in vc.KERNEL_CASES for mode in vc.MODES]
CASE_IDS = lambda c: 'B%d_F%d_W%d_%s' % (c[0], len(c[1]), sum(c[1]), c[2])


def _dev(t):
  return t.to(DEV, torch.float32)


def _seg(dims, mode):
  return None if mode == 'embedding_wise' else kernels.VDropSeg(dims, DEV)


# ---------------------------------------------------------------------------------------- the kernel
_WANT = {}


def _rel(got, want):
  return float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _composition_error(x, logit_p, u, d, dims, ew, want):
  """The fp32 torch composition against fp64 on the same inputs, on the CPU (it is not the code under test): relative
  errors of (out, penalty, dx, dlogit_p with the penalty's part, dlogit_p of the penalty alone)"""
  xr, lr = x.float().requires_grad_(True), logit_p.float().requires_grad_(True)
  seg = None if ew else torch.from_numpy(vc.seg_of(dims))
  out, pen = vdl.vdrop_compose(xr, lr, None if u is None else u.float(), seg, vc.LAMBDA / x.shape[0])
  out.backward(d.float(), retain_graph=True)
  dx, dl = xr.grad.clone(), lr.grad.clone()
  lr.grad = None
  (pen * vc.DPENALTY).sum().backward()
  out64, pen64, dx64, dl64, dlp64 = want
  return (_rel(out.detach(), out64), _rel(pen.detach(), pen64.reshape(1)), _rel(dx, dx64), _rel(dl + lr.grad, dl64 + dlp64),
          _rel(lr.grad, dlp64))


def _want(case, train, inputs=None):
  """the case's inputs, the fp64 autograd of the restatement on them and the fp32 composition's errors; computed once"""
  key = case + (train,)
  if key not in _WANT:
    B, dims, mode = case[:3]
    ew = mode == 'embedding_wise'
    x, logit_p, u, d = inputs if inputs is not None else vc.kernel_inputs(B, dims, ew)
    want = vc.want(x, logit_p, u if train else None, d, dims, ew)
    _WANT[key] = (x, logit_p, u, d) + want + (_composition_error(x, logit_p, u if train else None, d, dims, ew, want),)
  return _WANT[key]


def _bar(base, composition_error):
  """The project's bar, or - where the fp32 composition itself misses it on these inputs: 1 - p is formed from the
  rounded p, so log(1 - p + EPS) loses up to 7e-4 at logit_p = 10, ten times that in the sigmoid's argument - four times
  the composition's measured error: rounding in another summation order, and no more."""
  return max(base, 4.0 * composition_error)


def _check(case, train=True, want_dx=True, sliced=False, inputs=None, reference=None):
  """reference: (out, penalty, dx, dlogit_p of out, dlogit_p of the penalty) to hold the kernel to instead of fp64"""
  B, dims, mode = case[:3]
  W = sum(dims)
  x64, l64, u64, d64, out64, pen64, dx64, dl64, dlp64, comp = _want(case, train, inputs)
  if reference is not None:
    out64, pen64, dx64, dl64, dlp64 = [t.double() for t in reference]
    comp = (0.0,) * 5
  print(CASE_IDS(case), 'train' if train else 'eval', 'composition errors (out, penalty, dx, dlogit_p, dlogit_p of the '
        'penalty): %.2e %.2e %.2e %.2e %.2e' % comp)
  u = _dev(u64) if train else None
  lam = vc.LAMBDA / B
  seg = _seg(dims, mode)
  d, dpen = _dev(d64), torch.tensor([vc.DPENALTY], device=DEV)
  for given in (False, True):
    if sliced:
      wide = torch.randn(B, W + 2 * PAD, device=DEV)
      wide[:, PAD:PAD + W] = _dev(x64)
      before = wide.clone()
      wide.requires_grad_(want_dx)
      x = wide[:, PAD:PAD + W]
      assert x.data_ptr() % 16 != 0 and x.stride(0) == W + 2 * PAD
    else:
      wide = x = _dev(x64).requires_grad_(want_dx)
    logit_p = _dev(l64).requires_grad_(True)
    grads = [torch.full_like(logit_p, FILL)] if given else None
    out, pen = kernels.VDropFn.apply(grads, x, logit_p, u, seg, lam)
    torch.autograd.backward([out, pen], [d, dpen])
    torch.cuda.synchronize()
    assert out.shape == (B, W) and pen.shape == (1,)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(pen).all())
    print('  given' if given else '  returned', 'out %.2e penalty %.2e' % (_rel(out.detach().cpu(), out64),
                                                                        _rel(pen.detach().cpu(), pen64.reshape(1))))
    _close(out, out64, _bar(1e-5, comp[0]), 'out')
    _close(pen, pen64.reshape(1), _bar(1e-5, comp[1]), 'penalty')
    if want_dx:
      cols = slice(PAD, PAD + W) if sliced else slice(None)
      assert bool(torch.isfinite(wide.grad).all())
      print('  dx %.2e' % _rel(wide.grad[:, cols].cpu(), dx64))
      _close(wide.grad[:, cols], dx64, _bar(1e-4, comp[2]), 'dx')
      if sliced:  # the neighbouring columns get exactly nothing
        assert float(wide.grad[:, :PAD].abs().max()) == 0.0 and float(wide.grad[:, PAD + W:].abs().max()) == 0.0
    else:
      assert wide.grad is None
    if sliced:  # the wider tensor itself is untouched
      assert torch.equal(wide.detach(), before)
    dl_all = dl64 + dlp64
    if given:
      assert logit_p.grad is None
      got = grads[0] - FILL
      # (added into a buffer holding FILL: the sum is rounded at the buffer's magnitude, which the floor allows for)
      assert bool(torch.isfinite(got).all())
      print('  dlogit_p, added %.2e' % _rel(got.cpu(), dl_all))
      _close(got, dl_all, _bar(1e-4, comp[3]), 'dlogit_p, added', scale=1e-3 * FILL)
    else:
      assert bool(torch.isfinite(logit_p.grad).all())
      print('  dlogit_p, returned %.2e' % _rel(logit_p.grad.cpu(), dl_all))
      _close(logit_p.grad, dl_all, _bar(1e-4, comp[3]), 'dlogit_p, returned')


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_vdrop_matches_fp64_autograd(case):
  assert vdl.vdrop_fits(sum(case[1]))
  _check(case)


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_vdrop_in_evaluation_mode(case):
  _check(case, train=False)


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_vdrop_without_the_input_gradient(case):
  _check(case, want_dx=False)


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_vdrop_reads_a_column_slice_of_a_wider_tensor(case):
  _check(case, sliced=True)


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_penalty_and_its_gradient_alone(case):
  """the penalty's value and its own gradient against fp64, with no gradient arriving for the output; lambda = 0 gives
  exactly 0"""
  B, dims, mode = case
  x64, l64, u64, d64, out64, pen64, dx64, dl64, dlp64, comp = _want(case, True)
  seg = _seg(dims, mode)
  logit_p = _dev(l64).requires_grad_(True)
  out, pen = kernels.VDropFn.apply(None, _dev(x64), logit_p, _dev(u64), seg, vc.LAMBDA / B)
  pen.backward(torch.tensor([vc.DPENALTY], device=DEV))
  print(CASE_IDS(case), 'penalty %.2e its gradient %.2e; the composition %.2e %.2e' % (
      _rel(pen.detach().cpu(), pen64.reshape(1)), _rel(logit_p.grad.cpu(), dlp64), comp[1], comp[4]))
  _close(pen, pen64.reshape(1), _bar(1e-5, comp[1]), 'penalty')
  _close(logit_p.grad, dlp64, _bar(1e-4, comp[4]), 'dlogit_p of the penalty')
  logit_p = _dev(l64).requires_grad_(True)
  out, pen = kernels.VDropFn.apply(None, _dev(x64), logit_p, _dev(u64), seg, 0.0)
  pen.backward(torch.tensor([vc.DPENALTY], device=DEV))
  assert float(pen.detach()) == 0.0 and float(logit_p.grad.abs().max()) == 0.0


@pytest.mark.parametrize('case', [(13, (1, 3, 4), m) for m in vc.MODES] + [(9, (16, 16, 16), m) for m in vc.MODES],
                         ids=CASE_IDS)
def test_saturated_probabilities_stay_finite_and_inside_the_bars(case):
  """logit_p = +-100 against u = 0 and the largest fp32 below 1: p rounds to 1 (or 1 - p to 1) in fp32 only, so fp64 is
  no reference here; every result is finite and within the bars of the fp32 composition evaluated on the CPU."""
  B, dims, mode = case
  ew = mode == 'embedding_wise'
  x64, l64, u64, d64 = vc.kernel_inputs(B, dims, ew)
  l64 = torch.where(torch.arange(l64.numel()) % 2 == 0, 100.0, -100.0).double()
  hi = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
  u64 = torch.where((torch.arange(u64.numel()).reshape(u64.shape) // 2) % 2 == 0, 0.0, hi).double()
  xr, lr = x64.float().requires_grad_(True), l64.float().requires_grad_(True)
  seg = None if ew else torch.from_numpy(vc.seg_of(dims))
  out, pen = vdl.vdrop_compose(xr, lr, u64.float(), seg, vc.LAMBDA / B)
  out.backward(d64.float(), retain_graph=True)
  dx, dl = xr.grad.clone(), lr.grad.clone()
  lr.grad = None
  (pen * vc.DPENALTY).sum().backward()
  ref = (out.detach(), pen.detach(), dx, dl, lr.grad.clone())
  assert all(bool(torch.isfinite(t).all()) for t in ref)
  _check(case + ('saturated',), inputs=(x64, l64, u64, d64), reference=ref)


def test_the_masks_mean_at_logit_zero():
  """at logit_p = 0 the mask is 1 - sigmoid(10 (log u - log(1 - u))) = (1 - u)^10 / (u^10 + (1 - u)^10): symmetric about
  1 / 2, so its mean is 1 / 2; a mean of n draws of a variable bounded in [0, 1] has a standard error of at most
  1 / (2 sqrt(n)); the margin is 6 of those"""
  B, W = 4096, 39
  gen = torch.Generator(device=DEV).manual_seed(11)
  u = torch.rand(B, W, device=DEV, generator=gen)
  out, _ = kernels.VDropFn.apply(None, torch.ones(B, W, device=DEV), torch.zeros(W, device=DEV), u, None, 0.0)
  n = B * W
  assert abs(float(out.double().mean()) - 0.5) <= 6 * 0.5 / np.sqrt(n)
  assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0


# ---------------------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize('case', [(301, (16,) * 17, m) for m in vc.MODES] + [(13, (1, 3, 4), m) for m in vc.MODES] +
                         [(77, (16, 8, 1, 4, 3), 'feature_wise')], ids=CASE_IDS)
def test_two_runs_and_graph_replay_are_bit_identical(case):
  B, dims, mode = case
  x64, l64, u64, d64 = vc.kernel_inputs(B, dims, mode == 'embedding_wise')
  x, logit_p, u, d = _dev(x64), _dev(l64), _dev(u64), _dev(d64)
  seg = _seg(dims, mode)
  grads = [torch.zeros_like(logit_p)]
  dpen = torch.tensor([vc.DPENALTY], device=DEV)

  def run():
    grads[0].zero_()
    xi = x.detach().requires_grad_(True)
    out, pen = kernels.VDropFn.apply(grads, xi, logit_p, u, seg, vc.LAMBDA / B)
    torch.autograd.backward([out, pen], [d, dpen])
    li = logit_p.detach().requires_grad_(True)
    plain, pen2 = kernels.VDropFn.apply(None, x, li, None, seg, vc.LAMBDA / B)
    torch.autograd.backward([plain, pen2], [d, dpen])
    return [out.detach(), pen.detach(), xi.grad, grads[0].clone(), plain.detach(), pen2.detach(), li.grad]

  assert_runs_and_replay_bit_identical(run)


# ---------------------------------------------------------------------------------------- outside the envelope
def test_launches_outside_the_envelope_return_an_error():
  import ctypes
  be = kernels.hip()
  t = torch.zeros(4, 8, device=DEV)
  out = torch.full((4, 8), -7.0, device=DEV)
  p = lambda x: x.data_ptr()

  def fwd(W, P, ld, seg_host=None, seg=None, ldu=8):
    be.ck.er_vdrop_fwd(p(t), ld, p(t), p(t), ldu, seg_host, seg, 4, W, P, 0.0, p(out), ld, p(out), None)

  def bwd(W, P, ld, seg_host=None, seg=None, ldu=8):
    be.ck.er_vdrop_bwd(p(t), ld, p(t), ld, p(t), p(t), ldu, seg_host, seg, 4, W, P, 0.0, None, p(out), ld, p(out), None)

  # W = 0, W = 4097, a pitch below W, P != W without a column map
  for W, P, ld in ((0, 0, 8), (4097, 4097, 4097), (8, 8, 7), (8, 4, 8)):
    assert be.vdrop_grid(4, W) == vc.grid_of(4, W) == (1 if W == 8 else 0)
    with pytest.raises(RuntimeError, match='er_vdrop_fwd'):
      fwd(W, P, ld)
    with pytest.raises(RuntimeError, match='er_vdrop_bwd'):
      bwd(W, P, ld)
  dev_seg = torch.zeros(8, dtype=torch.int32, device=DEV)
  # column maps that are not non-decreasing over 0 .. P - 1: descending, a gap, not from 0, not up to P - 1
  for P, seg in ((3, [0, 1, 1, 0, 2, 2, 2, 2]), (3, [0, 0, 0, 2, 2, 2, 2, 2]), (2, [1, 1, 1, 1, 1, 1, 1, 1]),
                 (3, [0, 0, 0, 0, 1, 1, 1, 1])):
    host = (ctypes.c_int32 * 8)(*seg)
    with pytest.raises(RuntimeError, match='column map'):
      fwd(8, P, 8, host, p(dev_seg))
    with pytest.raises(RuntimeError, match='column map'):
      bwd(8, P, 8, host, p(dev_seg))
  with pytest.raises(RuntimeError, match='pitch'):  # u's pitch below P
    fwd(8, 8, 8, ldu=7)
  assert be.vdrop_grid(0, 8) == vc.grid_of(0, 8) == 0
  torch.cuda.synchronize()
  assert bool((out == -7.0).all())  # nothing was launched


# ---------------------------------------------------------------------------------------- the layer
@pytest.mark.parametrize('embedding_wise', [True, False], ids=['embedding_wise', 'feature_wise'])
def test_layer_on_the_kernel_matches_the_composition(embedding_wise, monkeypatch):
  """Two groups at B = 67 through VariationalDropoutLayer on the kernel and with the switch at 0, fed the same noise:
  outputs and summed penalty within 1e-5, the input gradients and the variables' gradients within 1e-4; one forward and
  one backward launch per group on the kernel, none with the switch at 0."""
  B = 67
  groups = [('all', [('a', 16), ('b', 8), ('c', 1), ('d', 4), ('e', 3)]), ('wide', [('f%d' % i, 1) for i in range(9)])]
  cfg = variational_dropout_pb2.VariationalDropoutLayer(regularization_lambda=0.01,
                                                   embedding_wise_variational_dropout=embedding_wise)
  g = torch.Generator().manual_seed(5)
  xs = [torch.randn(B, sum(d for _, d in dims), generator=g).to(DEV) for _, dims in groups]
  dys = [torch.randn(x.shape, generator=g).to(DEV) for x in xs]
  layers = []

  def forward():
    if not layers:
      layers.extend(vdl.VariationalDropoutLayer(cfg, dims, True, name=name) for name, dims in groups)
    return [layer(x) for layer, x in zip(layers, xs)]

  vs, ctx = product_store(DEV, forward)
  assert sorted(vs.names()) == ['logit_p', 'logit_p_wide']
  P = [sum(d for _, d in dims) if embedding_wise else len(dims) for _, dims in groups]
  assert [tuple(layer.logit_p.shape) for layer in layers] == [(n,) for n in P]

  def run(fused):
    monkeypatch.setenv(SWITCH, '1' if fused else '0')
    vs.zero_grad()
    del ctx.vdrop_losses[:]
    torch.manual_seed(17)
    be = kernels.hip()
    be.op_log = []
    try:
      with context.use(ctx):
        xi = [x.detach().requires_grad_(True) for x in xs]
        ys = [layer(x) for layer, x in zip(layers, xi)]
        pens = list(ctx.vdrop_losses)
        torch.autograd.backward(ys + pens, dys + [torch.ones_like(p) for p in pens])
      names = [n for n, _ in be.op_log]
    finally:
      be.op_log = None
    torch.cuda.synchronize()
    return ([y.detach() for y in ys], sum(p.detach() for p in pens), [x.grad for x in xi],
            {n: torch.from_numpy(v) for n, v in vs.grad_dict().items()}, names)

  ys, pen, dxs, grads, names = run(True)
  count = lambda ns, k: sum(n == 'er::%s_kernel' % k for n in ns)
  assert count(names, 'vdrop_fwd') == count(names, 'vdrop_bwd') == 2, names
  ysc, penc, dxsc, gradsc, namesc = run(False)
  assert not any('vdrop' in n for n in namesc)
  for i in range(2):
    _close(ys[i], ysc[i], 1e-5, ('y', i))
    _close(dxs[i], dxsc[i], 1e-4, ('dx', i))
  _close(pen, penc, 1e-5, 'penalty')
  for n in ('logit_p', 'logit_p_wide'):
    assert float(gradsc[n].abs().max()) > 0
    _close(grads[n], gradsc[n], 1e-4, n)


# ---------------------------------------------------------------------------------------- the model
def _estimator(B, model, name='deepfm_vdrop_criteo.config', seed=3):
  """the new configs' shape with every table cut to 2000 rows; model 'FM': the same groups under the FM model"""
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', name))
  for f in cfg.feature_config.features:
    if f.HasField('hash_bucket_size') and f.hash_bucket_size > 0:
      f.hash_bucket_size = 2000
  if model == 'FM':
    cfg.model_config.model_class = 'FM'
    cfg.model_config.fm.SetInParent()
  torch.manual_seed(29)  # (the layer draws its noise on the device's generator: both switch settings see the same draws)
  return cfg, EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=seed).build()


@pytest.mark.parametrize('model,name', [('DeepFM', 'deepfm_vdrop_criteo.config'), ('FM', 'deepfm_vdrop_criteo.config'),
                                        ('DeepFM', 'deepfm_vdrop_criteo_feature_num.config')],
                         ids=['deepfm', 'fm', 'deepfm_feature_num'])
def test_model_steps_on_the_kernel_match_the_composition(model, name, monkeypatch):
  """Two training steps from the same state on the same batches and the same noise with the switch at 1 and at 0, at the
  bars of tests/_oracle_steps.first_steps: every loss within 1e-5 (first step) / 1e-4 (second) of max(1e-3, |loss|);
  after the first step every variable's gradient, read back as Adam's first moment, within 2e-4 of its own scale + 2e-6
  of the largest one (a dense bias under BatchNorm has a zero gradient and is not compared, as there)."""
  B = 67
  out = {}
  for flag in ('1', '0'):
    monkeypatch.setenv(SWITCH, flag)
    cfg, est = _estimator(B, model, name)
    gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=103)
    be = kernels.hip()
    be.op_log = []
    try:
      est.train_step(gen.next_batch())
      names = [n for n, _ in be.op_log]
    finally:
      be.op_log = None
    first, moments = est.loss_values(), est.state_dict(slots=True)
    est.train_step(gen.next_batch())
    out[flag] = (first, est.loss_values(), moments, names)
  count = lambda ns, k: sum(n == 'er::%s_kernel' % k for n in ns)
  assert count(out['1'][3], 'vdrop_fwd') == count(out['1'][3], 'vdrop_bwd') == 2  # (the deep and the wide group)
  assert not any('vdrop' in n for n in out['0'][3])
  for step, tol in ((0, 1e-5), (1, 1e-4)):
    got, ref = out['1'][step], out['0'][step]
    assert sorted(got) == sorted(ref) and 'variational_dropout_loss' in ref
    for k in ref:
      assert np.isfinite(got[k]) and abs(got[k] - ref[k]) <= tol * max(1e-3, abs(ref[k])), (step, k, got[k], ref[k])
  # the penalty is part of total_loss and not of regularization_loss
  first = out['1'][0]
  parts = sum(v for k, v in first.items() if k != 'total_loss')
  assert first['variational_dropout_loss'] > 0 and abs(first['total_loss'] - parts) <= 1e-5 * abs(parts)
  st1, st0 = out['1'][2], out['0'][2]
  moments = [k for k in st0 if k.endswith('/m')]
  gmax = max(float(np.abs(st0[k]).max()) for k in moments)
  compared = []
  for key in moments:
    k = key[:-len('/m')]
    if k.endswith('/bias') and (k[:-len('/bias')] + '/bn/gamma') in st0:
      continue
    err = float(np.abs(st1[key] - st0[key]).max())
    assert err <= 2e-4 * float(np.abs(st0[key]).max()) + 2e-6 * gmax, (k, err)
    compared.append(k)
  assert {'logit_p_deep', 'logit_p_wide'} <= set(compared)
  assert any('embedding_weights' in k for k in compared)
  assert float(np.abs(st0['logit_p_deep/m']).max()) > 0 and float(np.abs(st0['logit_p_wide/m']).max()) > 0


def test_eager_and_captured_steps_give_the_same_loss_bits(monkeypatch):
  monkeypatch.setenv(SWITCH, '1')
  B = 67
  losses = {}
  for graph in (False, True):
    cfg, est = _estimator(B, 'DeepFM')
    gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=104)
    est.train_step(gen.next_batch())  # (one eager step before a capture: lazily created workspaces exist)
    if graph:
      est.capture(warmup=0)
    seen = []
    for _ in range(3):
      est.train_step(gen.next_batch())
      seen.append(est.loss_values())
    assert (est.graph is not None) == graph
    losses[graph] = seen
  assert losses[True] == losses[False], (losses[True], losses[False])
