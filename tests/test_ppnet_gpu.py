"""PPNet's HIP gate kernel (csrc/er_ppnet.hip) on the GPU: forward and every gradient against fp64 autograd of
x * 2 * sigmoid(z + bias); without a bias, without the input gradient, on column slices of wider tensors, with the bias
gradient added into a given buffer or returned; saturated gates; bit identity (two runs, eager vs hipGraph replay); the
envelope's refusals; the layer on the kernel against the fp64 restatement of tests/_ppnet_cases.py and against the torch
composition; the model with the switch at 1 and at 0."""
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.core import context  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.layers.keras import ppnet as pn  # noqa: E402
from easyrec_amd.layers.utils import Parameter  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from tests import _ppnet_cases as pc  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402
from tests._oracle_steps import close as _close  # noqa: E402
from tests._uniter_cases import product_store  # noqa: E402
from tests.test_ppnet_pins import LAYER_CASES  # noqa: E402

logging.disable(logging.WARNING)
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = lambda c: 'B%d_W%d' % c
SWITCH = 'EASYREC_AMD_FUSED_PPNET'
FILL = 0.25  # what a given bias gradient buffer holds before the backward adds into it
PAD = 3      # columns in front of a slice: base and pitch off the 16-byte grid


def _dev(t):
  return t.to(DEV, torch.float32)


# ---------------------------------------------------------------------------------------- the kernel
_WANT = {}


def _want(case, inputs=None):
  """fp64 autograd of x * 2 * sigmoid(z + bias): (out, dx, dz, dbias) with the bias and without; computed once."""
  if case not in _WANT:
    x64, z64, d64, b64 = inputs if inputs is not None else pc.kernel_inputs(*case)
    res = {}
    for with_bias in (True, False):
      xr, zr = x64.clone().requires_grad_(True), z64.clone().requires_grad_(True)
      br = b64.clone().requires_grad_(True) if with_bias else None
      out = pc.gate_scale(xr, zr, br)
      out.backward(d64)
      res[with_bias] = (out.detach(), xr.grad, zr.grad, br.grad if with_bias else None)
    _WANT[case] = res
  return _WANT[case]


def _slice_of(t64, grad):
  wide = torch.zeros(t64.shape[0], t64.shape[1] + 2 * PAD, device=DEV)
  wide[:, PAD:PAD + t64.shape[1]] = _dev(t64)
  wide.requires_grad_(grad)
  return wide, wide[:, PAD:PAD + t64.shape[1]]


def _check_gate(case, with_bias=True, want_dx=True, sliced=False, given=False, inputs=None):
  B, W = case[:2]
  x64, z64, d64, b64 = inputs if inputs is not None else pc.kernel_inputs(B, W)
  out64, dx64, dz64, db64 = _want(case, inputs)[with_bias]
  if sliced:
    (xw, x), (zw, z), (_, d) = _slice_of(x64, want_dx), _slice_of(z64, True), _slice_of(d64, False)
    assert x.data_ptr() % 16 != 0 and x.stride(0) == W + 2 * PAD
  else:
    x, z, d = _dev(x64).requires_grad_(want_dx), _dev(z64).requires_grad_(True), _dev(d64)
    xw, zw = x, z
  bias = _dev(b64).requires_grad_(True) if with_bias else None
  grads = [torch.full_like(bias, FILL)] if (given and with_bias) else None
  out = kernels.GateScaleFn.apply(grads, x, z, bias)
  out.backward(d)
  torch.cuda.synchronize()
  cols = slice(PAD, PAD + W) if sliced else slice(None)
  assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(zw.grad).all())
  _close(out, out64, 1e-5, 'out')
  _close(zw.grad[:, cols], dz64, 1e-4, 'dz')
  if want_dx:
    assert bool(torch.isfinite(xw.grad).all())
    _close(xw.grad[:, cols], dx64, 1e-4, 'dx')
  else:
    assert xw.grad is None
  if sliced:  # the neighbouring columns get exactly nothing
    for wide in ([xw, zw] if want_dx else [zw]):
      assert float(wide.grad[:, :PAD].abs().max()) == 0.0 and float(wide.grad[:, PAD + W:].abs().max()) == 0.0
  if with_bias and given:
    assert bias.grad is None
    # (added into a buffer holding FILL: the sum is rounded at the buffer's magnitude, which the floor allows for)
    _close(grads[0] - FILL, db64, 1e-4, 'dbias', scale=1e-3 * FILL)
  elif with_bias:
    _close(bias.grad, db64, 1e-4, 'dbias')


@pytest.mark.parametrize('case', pc.KERNEL_CASES, ids=CASE_IDS)
def test_gate_scale_matches_fp64_autograd(case):
  assert pn.gate_scale_fits(case[1])
  _check_gate(case)


@pytest.mark.parametrize('case', pc.KERNEL_CASES, ids=CASE_IDS)
def test_gate_scale_without_a_bias(case):
  _check_gate(case, with_bias=False)


@pytest.mark.parametrize('case', pc.KERNEL_CASES, ids=CASE_IDS)
def test_gate_scale_without_the_input_gradient(case):
  _check_gate(case, want_dx=False)


@pytest.mark.parametrize('case', pc.KERNEL_CASES, ids=CASE_IDS)
def test_gate_scale_reads_column_slices_of_wider_tensors(case):
  _check_gate(case, sliced=True)


@pytest.mark.parametrize('case', pc.KERNEL_CASES, ids=CASE_IDS)
def test_gate_scale_adds_the_bias_gradient_into_a_given_buffer(case):
  _check_gate(case, given=True)


@pytest.mark.parametrize('case', [(13, 7), (10, 16)], ids=CASE_IDS)
def test_saturated_gates_stay_finite_and_inside_the_bars(case):
  """z + bias in {-100, -20, 0, 20, 100}, mixed: the gate is 0 at -100 and 2 at +100; nothing is NaN or infinite."""
  B, W = case
  x64, _, d64, _ = pc.kernel_inputs(B, W)
  levels = torch.tensor([-100.0, -20.0, 0.0, 20.0, 100.0], dtype=torch.float64)
  b64 = torch.tensor([0.5, -0.25, 0.0, 1.0], dtype=torch.float64)[torch.arange(W) % 4]
  z64 = levels[torch.arange(B * W).reshape(B, W) % 5] - b64  # (exact in fp32, and so is z + bias)
  assert set((z64 + b64).flatten().tolist()) == set(levels.tolist())
  key = case + ('saturated',)
  _check_gate(key, inputs=(x64, z64, d64, b64))
  out = kernels.GateScaleFn.apply(None, _dev(x64), _dev(z64), _dev(b64)).double().cpu()
  a = z64 + b64
  assert bool((out[a == -100.0] == 0.0).all()) and bool((out[a == 100.0] == 2.0 * x64.float().double()[a == 100.0]).all())


# ---------------------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize('case', [(301, 256), (13, 7), (77, 128)], ids=CASE_IDS)
def test_two_runs_and_graph_replay_are_bit_identical(case):
  x64, z64, d64, b64 = pc.kernel_inputs(*case)
  x, z, d, bias = _dev(x64), _dev(z64), _dev(d64), _dev(b64)
  grads = [torch.zeros_like(bias)]

  def run():
    grads[0].zero_()
    xi, zi = x.detach().requires_grad_(True), z.detach().requires_grad_(True)
    out = kernels.GateScaleFn.apply(grads, xi, zi, bias)
    out.backward(d)
    xn, zn = x.detach().requires_grad_(True), z.detach().requires_grad_(True)
    plain = kernels.GateScaleFn.apply(None, xn, zn, None)
    plain.backward(d)
    return [out.detach(), xi.grad, zi.grad, grads[0].clone(), plain.detach(), xn.grad, zn.grad]

  assert_runs_and_replay_bit_identical(run)


# ---------------------------------------------------------------------------------------- outside the envelope
def test_launches_outside_the_envelope_return_an_error():
  be = kernels.hip()
  t = torch.zeros(4, 8, device=DEV)
  out = torch.full((4, 8), -7.0, device=DEV)
  p = lambda x: x.data_ptr()
  # (W, pitch): W = 0, W = 4097, and a pitch below W
  for W, ld in ((0, 8), (4097, 4097), (8, 7)):
    assert be.gate_scale_grid(4, W) == (1 if W == 8 else 0)
    with pytest.raises(RuntimeError, match='er_gate_scale_fwd'):
      be.ck.er_gate_scale_fwd(p(t), ld, p(t), ld, p(t), 4, W, p(out), ld, None)
    with pytest.raises(RuntimeError, match='er_gate_scale_bwd'):
      be.ck.er_gate_scale_bwd(p(t), ld, p(t), ld, p(t), ld, p(t), 4, W, p(out), ld, p(out), ld, p(out), None)
  for which in range(3):  # each pitch of the forward on its own
    lds = [8, 8, 8]
    lds[which] = 7
    with pytest.raises(RuntimeError, match='pitch'):
      be.ck.er_gate_scale_fwd(p(t), lds[0], p(t), lds[1], p(t), 4, 8, p(out), lds[2], None)
  assert be.gate_scale_grid(0, 8) == 0
  torch.cuda.synchronize()
  assert bool((out == -7.0).all())  # nothing was launched


# ---------------------------------------------------------------------------------------- the layer
def _bn_shadowed(name, params):
  """a dense bias under BatchNormalization: its gradient is zero analytically"""
  return name.endswith('/dense/bias') and (name[:-len('/dense/bias')] + '/bn/gamma') in params


@pytest.mark.parametrize('tag,B', LAYER_CASES)
def test_layer_on_the_kernel_matches_the_restatement_and_the_composition(tag, B, monkeypatch):
  """1e-5 of the largest element forward, 1e-4 for the gradient of x, of gate_input and of every variable, for the
  layer on the kernel and for the torch composition against the fp64 restatement, and for the two against each other.
  Every element is compared: the cases keep their ReLU pre-activations away from zero (tests/test_ppnet_pins.py).  A
  gradient that is small beside the others is held to 1e-4 of 1e-6 of the largest gradient's magnitude at least.  A
  dense bias under BatchNormalization has the gradient zero analytically; in fp32 it is the rounding of a sum of B
  terms that cancel, and is held to 2^-20 (16 fp32 ulps) of the largest gradient's magnitude."""
  pb, x64, u64, params = pc.layer_case(tag, B)
  x, u = _dev(x64), _dev(u64)
  made = []

  def forward():  # (the layer reads the build context in its constructor too)
    if not made:
      made.append(pn.PPNet(Parameter(pb, False, l2_reg=1e-6), name=pc.NAME))
    return made[0]((x, u), training=True)

  vs, ctx = product_store(DEV, forward, params)
  layer = made[0]
  trainable = [n for n in params if '/moving_' not in n]
  xr, ur = x64.clone().requires_grad_(True), u64.clone().requires_grad_(True)
  pr = {n: p.clone().requires_grad_(n in trainable) for n, p in params.items()}
  want = pc.ppnet(pb, pr, pc.NAME, xr, ur)
  dy64 = torch.randn(want.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64).float().double()
  (want * dy64).sum().backward()
  largest = max(float(pr[n].grad.abs().max()) for n in trainable)

  def run(fused):
    monkeypatch.setenv(SWITCH, '1' if fused else '0')
    vs.zero_grad()
    ctx.grad_slots.clear()  # (what EasyRecModel.begin_step does: the dense layers' shared input-gradient buffers are per step)
    xi, ui = x.detach().requires_grad_(True), u.detach().requires_grad_(True)
    be = kernels.hip()
    be.op_log = []
    try:
      with context.use(ctx):
        y = layer((xi, ui), training=True)
        y.backward(_dev(dy64))
      names = [n for n, _ in be.op_log]
    finally:
      be.op_log = None
    torch.cuda.synchronize()
    return y.detach(), xi.grad, ui.grad, {n: torch.from_numpy(g) for n, g in vs.grad_dict().items()}, names

  y, dx, du, grads, names = run(True)
  count = lambda ns, k: sum(n == 'er::%s_kernel' % k for n in ns)
  assert count(names, 'gate_scale_fwd') == count(names, 'gate_scale_bwd') == len(layer.gates) >= 1, names
  yc, dxc, duc, gradsc, namesc = run(False)
  assert not any('gate_scale' in n for n in namesc)

  def compare(what, got, ref):
    gy, gdx, gdu, gg = got
    ry, rdx, rdu, rg = ref
    _close(gy, ry, 1e-5, (what, 'y'))
    _close(gdx, rdx, 1e-4, (what, 'dx'))
    _close(gdu, rdu, 1e-4, (what, 'dgate_input'))
    for n in trainable:
      if _bn_shadowed(n, params):
        assert float(gg[n].double().abs().max()) <= 2.0 ** -20 * largest, (what, n)
      else:
        _close(gg[n], rg[n], 1e-4, (what, n), scale=1e-6 * largest)

  ref = (want.detach(), xr.grad, ur.grad, {n: pr[n].grad for n in trainable})
  compare('kernel', (y, dx, du, grads), ref)
  compare('composition', (yc, dxc, duc, gradsc), ref)
  compare('kernel vs composition', (y, dx, du, grads), (yc, dxc, duc, gradsc))


# ---------------------------------------------------------------------------------------- the model
def _estimator(B, seed=3):
  """configs/ppnet_taobao_10m.config with the item table cut to a few thousand rows"""
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'ppnet_taobao_10m.config'))
  item = [f for f in cfg.feature_config.features if list(f.input_names) == ['adgroup_id']][0]
  assert item.hash_bucket_size == 10000000
  item.hash_bucket_size = 4000
  return cfg, EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=seed).build()


def test_model_steps_on_the_kernel_match_the_composition(monkeypatch):
  """Two training steps from the same state on the same batches with the switch at 1 and at 0, at the bars of
  tests/_oracle_steps.first_steps: every loss within 1e-5 (first step) / 1e-4 (second) of max(1e-3, |loss|); after the
  first step every variable's gradient, read back as Adam's first moment, within 2e-4 of its own scale + 2e-6 of the
  largest one (a dense bias under BatchNorm has a zero gradient and is not compared, as there)."""
  B = 67
  out = {}
  for flag in ('1', '0'):
    monkeypatch.setenv(SWITCH, flag)
    cfg, est = _estimator(B)
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
  assert count(out['1'][3], 'gate_scale_fwd') == count(out['1'][3], 'gate_scale_bwd') == 2
  assert not any('gate_scale' in n for n in out['0'][3])
  for step, tol in ((0, 1e-5), (1, 1e-4)):
    got, ref = out['1'][step], out['0'][step]
    assert sorted(got) == sorted(ref)
    for k in ref:
      assert np.isfinite(got[k]) and abs(got[k] - ref[k]) <= tol * max(1e-3, abs(ref[k])), (step, k, got[k], ref[k])
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
  assert {'ppnet/gate_1/weight/bias', 'ppnet/gate_2/weight/bias', 'ppnet/gate_1/dense/kernel',
          'ppnet/layer_0/dense/kernel'} <= set(compared)
  assert any('embedding_weights' in k for k in compared)
  assert float(np.abs(st0['ppnet/gate_1/weight/bias/m']).max()) > 0


def test_eager_and_captured_steps_give_the_same_loss_bits(monkeypatch):
  monkeypatch.setenv(SWITCH, '1')
  B = 67
  losses = {}
  for graph in (False, True):
    cfg, est = _estimator(B)
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
