"""MaskNet's HIP kernels (csrc/er_masknet.hip) on the GPU: the mask multiply and the LayerNorm + ReLU, forward and every
gradient, against fp64 autograd over the restatement of tests/_masknet_cases.py; the parameter gradients added into
given buffers or returned; bit identity (two runs, eager vs hipGraph replay); the layers on the kernels against the
restatement and against the torch composition; the model with the switch at 1 and at 0; the envelope's refusals."""
import ctypes
import logging

import numpy as np
import pytest
import torch
from google.protobuf import text_format

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.core import context  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.layers.keras import mask_net as mn  # noqa: E402
from easyrec_amd.layers.utils import Parameter  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.protos import layer_pb2  # noqa: E402
from tests import _masknet_cases as mc  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402
from tests._oracle_steps import close as _close  # noqa: E402
from tests._uniter_cases import product_store  # noqa: E402
from tests.test_masknet_pins import masknet_cfg  # noqa: E402

logging.disable(logging.WARNING)
DEV = 'cuda:0'
PATTERN_TOL = 1e-5  # where the kernel's ReLU pattern may differ from fp64's: within this of zero (of the largest |pre|)
PATTERN_SHARE = 1e-4  # ... and on at most this share of a case's elements
CASE_IDS = lambda c: 'B%d_W%d_n%d' % c


def _dev(t):
  return t.to(DEV, torch.float32)


# ---------------------------------------------------------------------------------------- the mask multiply
def _check_mask_mul(case, want_dx=True, sliced=False):
  B, W, n = case
  x64, v64, d64, _, _ = mc.kernel_inputs(B, W, n)
  x = _dev(x64).requires_grad_(want_dx)
  if sliced:  # the masks as column slices of one wider tensor: pitch n * W + 3, bases off the 16-byte grid
    wide = torch.zeros(B, n * W + 3, device=DEV)
    for i, v in enumerate(v64):
      wide[:, 3 + i * W:3 + (i + 1) * W] = _dev(v)
    wide.requires_grad_(True)
    vs = [wide[:, 3 + i * W:3 + (i + 1) * W] for i in range(n)]
  else:
    vs = [_dev(v).requires_grad_(True) for v in v64]
  outs = kernels.MaskMulFn.apply(x, *vs)
  assert len(outs) == n
  torch.autograd.backward(list(outs), [_dev(d) for d in d64])
  torch.cuda.synchronize()
  xr = x64.clone().requires_grad_(True)
  vr = [v.clone().requires_grad_(True) for v in v64]
  torch.autograd.backward([xr * v for v in vr], d64)
  for i in range(n):
    _close(outs[i], x64 * v64[i], 1e-5, ('out', i))
    dv = wide.grad[:, 3 + i * W:3 + (i + 1) * W] if sliced else vs[i].grad
    _close(dv, vr[i].grad, 1e-4, ('dv', i))
  if sliced:
    assert float(wide.grad[:, :3].abs().max()) == 0.0
  if want_dx:
    _close(x.grad, xr.grad, 1e-4, 'dx')
  else:
    assert x.grad is None


@pytest.mark.parametrize('case', mc.KERNEL_CASES, ids=CASE_IDS)
def test_mask_mul_matches_fp64_autograd(case):
  assert mn.mask_mul_fits(case[1], case[2])
  _check_mask_mul(case)


@pytest.mark.parametrize('case', mc.KERNEL_CASES, ids=CASE_IDS)
def test_mask_mul_without_the_input_gradient(case):
  _check_mask_mul(case, want_dx=False)


@pytest.mark.parametrize('case', mc.KERNEL_CASES, ids=CASE_IDS)
def test_mask_mul_reads_column_slices_of_a_wider_tensor(case):
  _check_mask_mul(case, sliced=True)


# ---------------------------------------------------------------------------------------- LayerNorm + ReLU
def _licence(pre64, y):
  """The kernel's own ReLU pattern (y > 0), CHECKED against fp64's: where they differ the fp64 pre-activation lies
  within PATTERN_TOL of zero relative to the largest one, on at most PATTERN_SHARE of the elements."""
  mask = (y.detach().double().cpu() > 0).to(torch.float64)
  differ = mask != (pre64 > 0).to(torch.float64)
  lim = PATTERN_TOL * float(pre64.abs().max())
  assert float(pre64[differ].abs().max() if differ.any() else 0.0) <= lim, 'ReLU pattern differs away from zero'
  assert int(differ.sum()) <= PATTERN_SHARE * pre64.numel(), (int(differ.sum()), pre64.numel())
  return mask


def _ln_relu_reference(h64, ga64, be64, d64, mask):
  hr = [h.clone().requires_grad_(True) for h in h64]
  gr = [g.clone().requires_grad_(True) for g in ga64]
  br = [b.clone().requires_grad_(True) for b in be64]
  (mc.ln_relu_pre(hr, gr, br) * mask * torch.cat(d64, dim=1)).sum().backward()
  return [h.grad for h in hr], [g.grad for g in gr], [b.grad for b in br]


def _check_ln_relu(case, given_buffers, wide):
  B, O, n = case
  _, h64, d64, ga64, be64 = mc.kernel_inputs(B, O, n)
  hs = [_dev(h).requires_grad_(True) for h in h64]
  gb = [_dev(t).requires_grad_(True) for pair in zip(ga64, be64) for t in pair]
  fill = 0.25
  grads = [torch.full_like(t, fill) for t in gb] if given_buffers else None
  col0, pad = (4, 8) if wide else (0, 0)
  out = torch.full((B, n * O + pad), -7.0, device=DEV) if wide else None
  ret = kernels.LnReluFn.apply(mn.LN_EPSILON, grads, out, col0, *(hs + gb))
  if wide:  # written in place into the wider concatenation buffer; the other columns are untouched
    assert ret.data_ptr() == out.data_ptr() and ret.shape == out.shape
    assert bool((ret[:, :col0] == -7.0).all()) and bool((ret[:, col0 + n * O:] == -7.0).all())
  y = ret[:, col0:col0 + n * O]
  dret = torch.randn(ret.shape, device=DEV)  # (the gradient of the columns that are not the kernel's goes nowhere)
  dret[:, col0:col0 + n * O] = _dev(torch.cat(d64, dim=1))
  ret.backward(dret)
  torch.cuda.synchronize()
  pre64 = mc.ln_relu_pre(h64, ga64, be64)
  mask = _licence(pre64, y)
  dh64, dg64, db64 = _ln_relu_reference(h64, ga64, be64, d64, mask)
  _close(y, torch.relu(pre64), 1e-5, 'y')
  floor = 1e-30 if O > 1 else 1.0  # (O = 1: h - mean = 0, so dh = dgamma = 0 exactly in both)
  for i in range(n):
    _close(hs[i].grad, dh64[i], 1e-4, ('dh', i), scale=floor)
    dg, db = (grads[2 * i] - fill, grads[2 * i + 1] - fill) if given_buffers else (gb[2 * i].grad, gb[2 * i + 1].grad)
    if given_buffers:
      assert gb[2 * i].grad is None and gb[2 * i + 1].grad is None
    # (added into a buffer holding `fill`: the sum is rounded at the buffer's magnitude, which the floor allows for)
    _close(dg, dg64[i], 1e-4, ('dgamma', i), scale=max(floor, 1e-3 * fill if given_buffers else 0.0))
    _close(db, db64[i], 1e-4, ('dbeta', i), scale=1e-3 * fill if given_buffers else None)


@pytest.mark.parametrize('case', mc.KERNEL_CASES, ids=CASE_IDS)
def test_ln_relu_matches_fp64_autograd(case):
  """y written into a wider concatenation buffer; the parameter gradients returned to autograd."""
  assert mn.ln_relu_fits(case[1], case[2])
  _check_ln_relu(case, given_buffers=False, wide=True)


@pytest.mark.parametrize('case', [(301, 256, 3), (13, 7, 2), (64, 1027, 2)], ids=CASE_IDS)
def test_ln_relu_adds_the_parameter_gradients_into_given_buffers(case):
  _check_ln_relu(case, given_buffers=True, wide=False)


# ---------------------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize('case', [(301, 256, 3), (13, 7, 2)], ids=CASE_IDS)
def test_two_runs_and_graph_replay_are_bit_identical(case):
  B, W, n = case
  x64, t64, d64, ga64, be64 = mc.kernel_inputs(B, W, n)
  x, ts, ds = _dev(x64), [_dev(t) for t in t64], [_dev(d) for d in d64]
  gb = [_dev(t) for pair in zip(ga64, be64) for t in pair]
  grads = [torch.zeros_like(t) for t in gb]
  dy = torch.cat(ds, dim=1)

  def run():
    for g in grads:
      g.zero_()
    xi = x.detach().requires_grad_(True)
    vi = [t.detach().requires_grad_(True) for t in ts]
    outs = kernels.MaskMulFn.apply(xi, *vi)
    y = kernels.LnReluFn.apply(mn.LN_EPSILON, grads, None, 0, *(list(outs) + gb))
    y.backward(dy)
    return [o.detach() for o in outs] + [y.detach(), xi.grad] + [v.grad for v in vi] + [g.clone() for g in grads]

  assert_runs_and_replay_bit_identical(run)


# ---------------------------------------------------------------------------------------- the layers
W_L, A_L, O_L = 40, 24, 12
_BLOCK = 'mask_blocks { aggregation_size: %d output_size: %d } '
LAYER_CASES = {
    'parallel': ('masknet', (_BLOCK % (A_L, O_L)) * 3 + 'mlp { hidden_units: [16, 8] }'),
    'serial': ('masknet', 'use_parallel: false ' + _BLOCK % (A_L, W_L) + _BLOCK % (A_L, O_L)),
    'unequal': ('masknet', _BLOCK % (A_L, O_L) + _BLOCK % (A_L, O_L + 5) + _BLOCK % (A_L, O_L)),
    'block_ln': ('mask_block', 'aggregation_size: %d output_size: %d input_layer_norm: true' % (A_L, O_L)),
    'outside': ('masknet', _BLOCK % (A_L, 4100) + _BLOCK % (A_L, 4100)),
}
# the K8i launches a forward runs with the switch at 1: (mask multiplies, LayerNorm + ReLU launches)
LAYER_LAUNCHES = {'parallel': (1, 1), 'serial': (2, 2), 'unequal': (1, 3), 'block_ln': (1, 1), 'outside': (1, 0)}


def _layer_case(name, B):
  kind, text = LAYER_CASES[name]
  pb = (layer_pb2.MaskNet if kind == 'masknet' else layer_pb2.MaskBlock)()
  text_format.Merge(text, pb)
  g = torch.Generator().manual_seed(B + len(text))
  x64 = (torch.randn(B, W_L, generator=g, dtype=torch.float64) * 1.3 + 0.2).float().double()
  x = _dev(x64)
  made = []

  def forward():  # (the layers read the build context in their constructors too)
    if not made:
      made.append((mn.MaskNet if kind == 'masknet' else mn.MaskBlock)(Parameter(pb, False, l2_reg=1e-6), name=mc.NAMES[kind]))
    return made[0](x, training=True)

  vs, ctx = product_store(DEV, forward)
  layer = made[0]
  params = {}
  for n, v in vs.state_dict().items():
    v = torch.from_numpy(np.asarray(v)).double()
    if n.endswith('/gamma'):
      v = 1.0 + 0.2 * torch.randn(v.shape, generator=g, dtype=torch.float64)
    elif n.endswith('/beta') or n.endswith('/bias'):
      v = 0.2 * torch.randn(v.shape, generator=g, dtype=torch.float64)
    params[n] = v.float().double()
  vs, ctx = product_store(DEV, lambda: layer(x, training=True), params)
  return kind, pb, layer, x64, x, vs, ctx, params


@pytest.mark.parametrize('B', [67, 301])
@pytest.mark.parametrize('name', sorted(LAYER_CASES))
def test_layers_on_the_kernels_match_the_restatement_and_the_composition(name, B, monkeypatch):
  kind, pb, layer, x64, x, vs, ctx, params = _layer_case(name, B)
  trainable = [n for n in params if '/moving_' not in n]
  width = int(mc.restate(kind, pb, [x64], params).shape[1])
  dy64 = torch.randn(B, width, generator=torch.Generator().manual_seed(2), dtype=torch.float64)

  def run(fused):
    monkeypatch.setenv('EASYREC_AMD_FUSED_MASKNET', '1' if fused else '0')
    vs.zero_grad()
    ctx.grad_slots.clear()  # (what EasyRecModel.begin_step does: the dense layers' shared input-gradient buffers are per step)
    xi = x.detach().requires_grad_(True)
    be = kernels.hip()
    be.op_log = []
    try:
      with context.use(ctx):
        y = layer(xi, training=True)
        y.backward(_dev(dy64))
      names = [n for n, _ in be.op_log]
    finally:
      be.op_log = None
    torch.cuda.synchronize()
    return y.detach(), xi.grad, {n: torch.from_numpy(g) for n, g in vs.grad_dict().items()}, names

  y, dx, grads, names = run(True)
  count = lambda ns, k: sum(n == 'er::%s_kernel' % k for n in ns)
  n_mul, n_ln = LAYER_LAUNCHES[name]
  assert (count(names, 'mask_mul_fwd'), count(names, 'mask_mul_bwd')) == (n_mul, n_mul), names
  assert (count(names, 'ln_relu_fwd'), count(names, 'ln_relu_bwd')) == (n_ln, n_ln), names
  yc, dxc, gradsc, namesc = run(False)
  assert not any('mask_mul' in n or 'ln_relu' in n for n in namesc)
  xr = x64.clone().requires_grad_(True)
  pr = {n: p.clone().requires_grad_(n in trainable) for n, p in params.items()}
  want = mc.restate(kind, pb, [xr], pr)
  (want * dy64).sum().backward()
  for what, got_y, got_dx, got_g in (('kernels', y, dx, grads), ('composition', yc, dxc, gradsc)):
    _close(got_y, want, 1e-5, (what, 'y'))
    _close(got_dx, xr.grad, 1e-4, (what, 'dx'))
    for n in trainable:
      _close(got_g[n], pr[n].grad, 1e-4, (what, n), scale=1e-6 * float(max(p.grad.abs().max() for p in pr.values()
                                                                          if p.grad is not None)))
  # and the kernels against the composition directly, at the same bars
  _close(y, yc, 1e-5, 'y vs composition')
  _close(dx, dxc, 1e-4, 'dx vs composition')
  for n in trainable:
    _close(grads[n], gradsc[n], 1e-4, (n, 'vs composition'), scale=1e-6 * float(max(g.abs().max() for g in gradsc.values())))


# ---------------------------------------------------------------------------------------- the model
def _estimator(seed=3, B=64):
  cfg = masknet_cfg(batch_size=B)
  est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=seed).build()
  return cfg, est


def test_model_step_on_the_kernels_matches_the_composition(monkeypatch):
  """One training step from the same seed and batch with the switch at 1 and at 0: every loss within 1e-5 of
  max(1, |loss|), every dense variable's and embedding table's Adam first moment within 1e-4 of its largest element
  (the bars tests/_oracle_steps.first_steps applies at its first step)."""
  B = 64
  out = {}
  for flag in ('1', '0'):
    monkeypatch.setenv('EASYREC_AMD_FUSED_MASKNET', flag)
    cfg, est = _estimator(B=B)
    gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=103)
    be = kernels.hip()
    be.op_log = []
    try:
      est.train_step(gen.next_batch())
      names = [n for n, _ in be.op_log]
    finally:
      be.op_log = None
    out[flag] = (est.loss_values(), est.state_dict(slots=True), names)
  count = lambda ns, k: sum(n == 'er::%s_kernel' % k for n in ns)
  assert count(out['1'][2], 'mask_mul_fwd') == count(out['1'][2], 'mask_mul_bwd') == 1
  assert count(out['1'][2], 'ln_relu_fwd') == count(out['1'][2], 'ln_relu_bwd') == 1
  assert not any('mask_mul' in n or 'ln_relu' in n for n in out['0'][2])
  (loss1, st1, _), (loss0, st0, _) = out['1'], out['0']
  assert sorted(loss1) == sorted(loss0)
  for k in loss0:
    assert abs(loss1[k] - loss0[k]) <= 1e-5 * max(1.0, abs(loss0[k])), (k, loss1[k], loss0[k])
  moments = [k for k in st0 if k.endswith('/m')]
  assert any(k.startswith('mask_net/block_2/output_ln/') for k in moments) and any('embedding_weights' in k for k in moments)
  for k in moments:
    _close(st1[k], st0[k], 1e-4, k, scale=1e-6 * max(float(np.abs(st0[m]).max()) for m in moments))


def test_eager_and_captured_steps_give_the_same_loss_bits(monkeypatch):
  monkeypatch.setenv('EASYREC_AMD_FUSED_MASKNET', '1')
  B = 64
  losses = {}
  for graph in (False, True):
    cfg, est = _estimator(B=B)
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


# ---------------------------------------------------------------------------------------- outside the envelope
def test_launches_outside_the_envelope_return_an_error():
  """The return code only: the envelope is the first thing a launcher checks, before it reads an argument."""
  be = kernels.hip()
  lib = be.lib
  t = torch.zeros(4, 8, device=DEV)
  ptr = lambda ts: (ctypes.c_void_p * len(ts))(*[x.data_ptr() for x in ts])
  ld = lambda k, v: (ctypes.c_int64 * k)(*([v] * k))
  for W, n in ((4097, 1), (8, 9), (0, 1), (8, 0)):
    k = max(n, 1)
    assert lib.er_mask_mul_fwd(t.data_ptr(), max(W, 8), ptr([t] * k), ld(k, max(W, 8)), n, 4, W, ptr([t] * k),
                               ld(k, max(W, 8)), None) != 0, (W, n)
    assert b'outside the envelope' in lib.er_last_error()
    assert lib.er_mask_mul_bwd(t.data_ptr(), max(W, 8), ptr([t] * k), ld(k, max(W, 8)), ptr([t] * k), ld(k, max(W, 8)), n,
                               4, W, ptr([t] * k), ld(k, max(W, 8)), None, 0, None) != 0, (W, n)
    assert b'outside the envelope' in lib.er_last_error()
    assert be.ln_relu_grid(4, W, n) == 0
    assert lib.er_ln_relu_fwd(ptr([t] * k), ld(k, max(W, 8)), ptr([t] * k), ptr([t] * k), n, 4, W, 1e-3, t.data_ptr(),
                              max(W, 8) * k, t.data_ptr(), t.data_ptr(), None) != 0, (W, n)
    assert b'outside the envelope' in lib.er_last_error()
    assert lib.er_ln_relu_bwd(t.data_ptr(), max(W, 8) * k, t.data_ptr(), max(W, 8) * k, ptr([t] * k), ld(k, max(W, 8)),
                              ptr([t] * k), t.data_ptr(), t.data_ptr(), n, 4, W, ptr([t] * k), ld(k, max(W, 8)),
                              t.data_ptr(), None) != 0, (W, n)
    assert b'outside the envelope' in lib.er_last_error()
  torch.cuda.synchronize()
  assert float(t.abs().max()) == 0.0
