"""The K8f kernels (csrc/er_mha.hip) on the GPU: the masked attention core and the residual add + LayerNorm, forward
and every gradient against the fp64 restatement (oracle/uniter_ref.py), both calling forms of the attention launch, a
constant LayerNorm row, bit-identity (two runs, eager vs hipGraph replay) of one encoder layer with gradients into the
variables' buffers, and the encoder layer on the fused path against the restatement and against the composition."""
import logging

import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.core import context  # noqa: E402
from easyrec_amd.layers import multihead_cross_attention as mca  # noqa: E402
from oracle import uniter_ref as ref  # noqa: E402
from tests import _uniter_cases as cases  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402
from tests._oracle_steps import close as _close  # noqa: E402

logging.disable(logging.WARNING)
DEV = 'cuda:0'
_encoder, _mask = cases.product_encoder, ref.mixed_mask

# (B, F, T, H, ds): the sample; more units than persistent workgroups; odd widths (4-byte staging); one query row and
# F != T; a cross shape; degenerate widths
ATTN_CASES = [
    (5, 33, 33, 4, 128),
    (301, 33, 33, 4, 128),
    (7, 9, 9, 3, 7),
    (3, 1, 17, 2, 8),
    (4, 16, 8, 2, 16),
    (6, 5, 1, 1, 1),
]


def _attn_reference(q64, k64, v64, mask, dctx64, B, F, T, H, ds):
  qr, kr, vr = (t.clone().requires_grad_(True) for t in (q64, k64, v64))
  want = ref.attention_core(qr, kr, vr, mask, B, F, T, H, ds)
  (want * dctx64).sum().backward()
  return want.detach(), qr.grad, kr.grad, vr.grad


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('case', ATTN_CASES, ids=lambda c: 'B%d_F%d_T%d_H%d_ds%d' % c)
def test_attention_kernels_match_the_restatement(case, masked):
  """er_mha_fwd / er_mha_bwd alone, called with separate Q and K | V buffers and, where F == T, with the packed
  [rows, 3 H ds] buffer too: ctx and dQ / dK / dV.  The mask: random keys, example 0 with a single open key, example 1
  with every key masked (the uniform-adder row)."""
  B, F, T, H, ds = case
  d = H * ds
  g = torch.Generator().manual_seed(B + F + ds)
  q64 = torch.randn(B * F, d, generator=g, dtype=torch.float64)
  k64 = torch.randn(B * T, d, generator=g, dtype=torch.float64)
  v64 = torch.randn(B * T, d, generator=g, dtype=torch.float64)
  dctx64 = torch.randn(B * F, d, generator=g, dtype=torch.float64)
  mask = _mask(B, T, B) if masked else None
  want, dq64, dk64, dv64 = _attn_reference(q64, k64, v64, mask, dctx64, B, F, T, H, ds)
  be = kernels.hip()
  to_mask = None if mask is None else mask.to(DEV)
  dctx = dctx64.to(DEV, torch.float32)
  # separate buffers: Q of its own, K | V side by side
  q = q64.to(DEV, torch.float32)
  kv = torch.cat([k64, v64], dim=1).to(DEV, torch.float32)
  ctx = be.mha_fwd(q, kv[:, :d], kv[:, d:], to_mask, B, F, T, H, ds)
  dq, dkv = torch.full_like(q, float('nan')), torch.full_like(kv, float('nan'))
  be.mha_bwd(q, kv[:, :d], kv[:, d:], to_mask, dctx, B, F, T, H, ds, dq, dkv[:, :d], dkv[:, d:])
  torch.cuda.synchronize()
  _close(ctx, want, 1e-5, 'ctx')
  _close(dq, dq64, 1e-4, 'dQ')
  _close(dkv[:, :d], dk64, 1e-4, 'dK')
  _close(dkv[:, d:], dv64, 1e-4, 'dV')
  if F != T:
    return
  # the packed self-attention buffer through the autograd function
  qkv = torch.cat([q64, k64, v64], dim=1).to(DEV, torch.float32).requires_grad_(True)
  out = kernels.MhaAttnFn.apply(qkv, None, to_mask, B, F, T, H, ds)
  out.backward(dctx)
  torch.cuda.synchronize()
  assert torch.equal(out.detach(), ctx)  # (the same launch on another pitch: the same bits)
  assert torch.equal(qkv.grad[:, :d], dq) and torch.equal(qkv.grad[:, d:], dkv)


def test_attention_function_with_separate_sources_and_the_projections():
  """MhaProjFn (n = 2 and 3) + MhaAttnFn in the cross form against the restatement, gradients into given buffers."""
  B, F, T, H, ds, din = 4, 16, 8, 2, 16, 24
  d = H * ds
  g = torch.Generator().manual_seed(9)
  xf64 = torch.randn(B * F, din, generator=g, dtype=torch.float64)
  xt64 = torch.randn(B * T, din, generator=g, dtype=torch.float64)
  p64 = {}
  for n in ('query', 'key', 'value'):
    p64['a/%s/kernel' % n] = torch.randn(din, d, generator=g, dtype=torch.float64) / din ** 0.5
    p64['a/%s/bias' % n] = torch.randn(d, generator=g, dtype=torch.float64)
  mask = _mask(B, T, 5)
  dy64 = torch.randn(B * F, d, generator=g, dtype=torch.float64)
  names = ['a/%s/%s' % (n, part) for part in ('kernel', 'bias') for n in ('query', 'key', 'value')]
  ps = [p64[n].to(DEV, torch.float32).requires_grad_(True) for n in names]
  grads = [torch.zeros_like(p) for p in ps]
  xf = xf64.to(DEV, torch.float32).requires_grad_(True)
  xt = xt64.to(DEV, torch.float32).requires_grad_(True)
  q = kernels.LinearFn.apply(xf, ps[0], ps[3], grads[0], grads[3], False, None, None)
  kv = kernels.MhaProjFn.apply(xt, [grads[1], grads[2], grads[4], grads[5]], 2, ps[1], ps[2], ps[4], ps[5])
  out = kernels.MhaAttnFn.apply(q, kv, mask.to(DEV), B, F, T, H, ds)
  out.backward(dy64.to(DEV, torch.float32))
  torch.cuda.synchronize()
  pr = {n: p.clone().requires_grad_(True) for n, p in p64.items()}
  xfr, xtr = xf64.clone().requires_grad_(True), xt64.clone().requires_grad_(True)
  want = ref.attention_layer(xfr, xtr, pr, 'a', mask, B, F, T, H, ds)
  (want * dy64).sum().backward()
  _close(out, want, 1e-5, 'out')
  _close(xf.grad, xfr.grad, 1e-4, 'dx_from')
  _close(xt.grad, xtr.grad, 1e-4, 'dx_to')
  for n, gr in zip(names, grads):
    # (the key bias shifts every score of a row alike: its gradient, the column sums of dK, is zero up to rounding and is
    # held at the scale of the key kernel's gradient, the same rows of dK weighted by x ~ N(0, 1))
    _close(gr, pr[n].grad, 1e-4, n, scale=float(pr['a/key/kernel'].grad.abs().max()) if n == 'a/key/bias' else None)
  # n = 3 on one source: the packed projection equals the three dense layers
  qkv = kernels.MhaProjFn.apply(xt.detach(), None, 3, *ps)
  for i, n in enumerate(('query', 'key', 'value')):
    _close(qkv[:, i * d:(i + 1) * d], ref.dense(xt64, p64, 'a/' + n), 1e-5, n)


# (rows, W): the sample's width (2 float4 per lane); one column; a narrow odd width over many rows; one float4 per
# lane with idle lanes; 4 float4 per lane with a ragged last one; the envelope's widest row (re-read form)
LN_CASES = [(165, 512), (7, 1), (1001, 7), (64, 64), (33, 1000), (5, 4096)]


def _ln_run(x64, res64, gamma64, beta64, dy64):
  be = kernels.hip()
  f32 = lambda t: None if t is None else t.to(DEV, torch.float32)  # noqa: E731
  x, res, gamma, beta, dy = f32(x64), f32(res64), f32(gamma64), f32(beta64), f32(dy64)
  y, mean, rstd = be.add_ln_fwd(x, res, gamma, beta, 1e-12)
  dgamma, dbeta = torch.full_like(gamma, float('nan')), torch.full_like(beta, float('nan'))
  dz = be.add_ln_bwd(dy, x, res, gamma, mean, rstd, kernels.ThetaGradTable([dgamma, dbeta]), False)
  torch.cuda.synchronize()
  return y, dz, dgamma, dbeta


def _ln_reference(x64, res64, gamma64, beta64, dy64):
  xr, gr, br = (t.clone().requires_grad_(True) for t in (x64, gamma64, beta64))
  z = xr if res64 is None else (xr.view(-1, res64.shape[0], xr.shape[1]) + res64).view(xr.shape)
  want = ref.add_layer_norm(z, None, gr, br)
  (want * dy64).sum().backward()
  return want.detach(), xr.grad, gr.grad, br.grad


# res: none, the full residual, and on the first case the per-position addend (res_rows = 33)
LN_RUNS = [(c, kind) for c in LN_CASES for kind in ('none', 'full')] + [(LN_CASES[0], 'broadcast')]


@pytest.mark.parametrize('case,res_kind', LN_RUNS, ids=lambda v: v if isinstance(v, str) else 'rows%d_W%d' % v)
def test_add_layer_norm_kernels_match_the_restatement(case, res_kind):
  rows, W = case
  g = torch.Generator().manual_seed(rows + W)
  x64 = torch.randn(rows, W, generator=g, dtype=torch.float64) * 2.0 + 0.5
  res_rows = {'none': 0, 'full': rows, 'broadcast': 33}[res_kind]
  res64 = torch.randn(res_rows, W, generator=g, dtype=torch.float64) if res_rows else None
  gamma64 = 1.0 + 0.3 * torch.randn(W, generator=g, dtype=torch.float64)
  beta64 = torch.randn(W, generator=g, dtype=torch.float64)
  dy64 = torch.randn(rows, W, generator=g, dtype=torch.float64)
  # (W = 1: z - mean = 0, y = beta, and dz = dgamma = 0 exactly in both: compared against a floor of 1)
  y, dz, dgamma, dbeta = _ln_run(x64, res64, gamma64, beta64, dy64)
  want, dz64, dgamma64, dbeta64 = _ln_reference(x64, res64, gamma64, beta64, dy64)
  _close(y, want, 1e-5, 'y')
  _close(dz, dz64, 1e-4, 'dz', scale=1e-30 if W > 1 else 1.0)
  _close(dgamma, dgamma64, 1e-4, 'dgamma', scale=1e-30 if W > 1 else 1.0)
  _close(dbeta, dbeta64, 1e-4, 'dbeta')


@pytest.mark.parametrize('W', [512, 36, 1030])
def test_a_constant_row_gives_beta_bit_for_bit(W):
  """Row 3 is constant: its mean is the constant exactly (taken about the row's first element), its variance 0, so
  y = beta to the bit and rstd = 1e6; dz is compared on that row alone, because its scale is 1e6 times the others'."""
  rows = 9
  g = torch.Generator().manual_seed(W)
  x64 = torch.randn(rows, W, generator=g, dtype=torch.float64).float().double()
  x64[3] = 0.1 * 7  # (not a dyadic value: a plain running sum of W copies does not stay exact)
  x64 = x64.float().double()
  gamma64 = 1.0 + 0.3 * torch.randn(W, generator=g, dtype=torch.float64)
  beta64 = torch.randn(W, generator=g, dtype=torch.float64).float().double()
  dy64 = torch.randn(rows, W, generator=g, dtype=torch.float64)
  y, dz, dgamma, dbeta = _ln_run(x64, None, gamma64, beta64, dy64)
  want, dz64, dgamma64, dbeta64 = _ln_reference(x64, None, gamma64, beta64, dy64)
  assert torch.equal(y[3].cpu(), beta64.float())
  others = [r for r in range(rows) if r != 3]
  _close(y[others], want[others], 1e-5, 'y')
  _close(dz[others], dz64[others], 1e-4, 'dz')
  _close(dz[3], dz64[3], 1e-4, 'dz of the constant row')
  assert float(dz64[3].abs().max()) > 1e4 * float(dz64[others].abs().max())
  _close(dgamma, dgamma64, 1e-4, 'dgamma')
  _close(dbeta, dbeta64, 1e-4, 'dbeta')


# ------------------------------------------------------------------------------------------------ the encoder layer
def _encoder_case(B, S, hidden, H, layers, inter, seed):
  params = ref.random_encoder_params('uniter', layers, hidden, inter, seed=seed)
  x64 = torch.randn(B, S, hidden, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)
  mask = _mask(B, S, seed + 2)
  x = x64.to(DEV, torch.float32)
  mask_d = mask.to(DEV)
  vs, ctx = cases.product_store(DEV, lambda: _encoder(x, mask_d, H, layers, inter), params)
  return params, x64, mask, x, mask_d, vs, ctx


def test_one_encoder_layer_two_runs_and_graph_replay_are_bit_identical():
  B, S, hidden, H = 257, 33, 64, 4
  params, x64, mask, x, mask_d, vs, ctx = _encoder_case(B, S, hidden, H, 1, 96, seed=3)
  dy = torch.randn(B, S, hidden, device=DEV)
  assert mca._fused(x) and mca.fits(S, S, hidden // H)

  def run():
    vs.zero_grad()
    xi = x.detach().requires_grad_(True)
    with context.use(ctx):
      y = _encoder(xi, mask_d, H, 1, 96)
      y.backward(dy)
    return [y.detach(), xi.grad, vs.flat_grad.clone()]

  assert not kernels.hip().wgrad_sink().active  # (the weight gradients are launched inside backward here)
  assert_runs_and_replay_bit_identical(run)


@pytest.mark.parametrize('shape', [(6, 9, 12, 3, 2, 10), (5, 33, 512, 4, 1, 512)], ids=['small', 'sample'])
def test_encoder_on_the_kernels_matches_the_restatement_and_the_composition(shape, monkeypatch):
  B, S, hidden, H, layers, inter = shape
  params, x64, mask, x, mask_d, vs, ctx = _encoder_case(B, S, hidden, H, layers, inter, seed=7)
  dy64 = torch.randn(B, S, hidden, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
  dy = dy64.to(DEV, torch.float32)

  def run(fused):
    monkeypatch.setenv('EASYREC_AMD_FUSED_MHA', '1' if fused else '0')
    vs.zero_grad()
    xi = x.detach().requires_grad_(True)
    be = kernels.hip()
    be.op_log = []
    try:
      with context.use(ctx):
        y = _encoder(xi, mask_d, H, layers, inter)
        y.backward(dy)
      names = [n for n, _ in be.op_log]
    finally:
      be.op_log = None
    torch.cuda.synchronize()
    return y.detach(), xi.grad, {n: torch.from_numpy(g) for n, g in vs.grad_dict().items()}, names

  y, dx, grads, names = run(True)
  # the fused path ran the new launches, once per layer (attention) and twice (add & LayerNorm)
  assert names.count('er::mha_fwd_kernel') == names.count('er::mha_bwd_kernel') == layers
  assert names.count('er::add_ln_fwd_kernel') == names.count('er::add_ln_bwd_kernel') == 2 * layers
  yc, dxc, gradsc, namesc = run(False)
  assert not any(n.startswith('er::mha_') or n.startswith('er::add_ln_') for n in namesc)
  xr = x64.clone().requires_grad_(True)
  pr = {n: p.clone().requires_grad_(True) for n, p in params.items()}
  want = ref.transformer_encoder(xr, mask, pr, 'uniter', layers, H)
  (want * dy64).sum().backward()
  for what, got_y, got_dx, got_g in (('kernels', y, dx, grads), ('composition', yc, dxc, gradsc)):
    _close(got_y, want, 1e-5, (what, 'y'))
    _close(got_dx, xr.grad, 1e-4, (what, 'dx'))
    ref_grads = {n: p.grad for n, p in pr.items()}
    for n, g in got_g.items():
      _close(g, ref_grads[n], 1e-4, (what, n), scale=ref.grad_floor(n, ref_grads))


def test_postprocessor_on_the_kernels_matches_the_restatement():
  """The per-position addend (token type + position rows, res_rows = S) and the per-token one, with their gradients."""
  B, S, W, V = 37, 16, 512, 5
  g = torch.Generator().manual_seed(8)
  x64 = torch.randn(B, S, W, generator=g, dtype=torch.float64)
  ids_b = torch.randint(0, V, (B, S), generator=g)

  def forward(x, ids):
    with mca.default_scopes():
      return mca.embedding_postprocessor(x, use_token_type=True, token_type_ids=ids, token_type_vocab_size=V,
                                         position_embedding_name='txt_position_embeddings_0', max_position_embeddings=20)

  x = x64.to(DEV, torch.float32)
  vs, ctx = cases.product_store(DEV, lambda: forward(x, 3))
  params = {n: torch.randn(v.shape, generator=g, dtype=torch.float64) for n, v in vs.state_dict().items()}
  vs, ctx = cases.product_store(DEV, lambda: forward(x, 3), params)
  dy64 = torch.randn(B, S, W, generator=g, dtype=torch.float64)
  for ids, ids64 in ((3, torch.full((S,), 3)), (ids_b, ids_b)):
    vs.zero_grad()
    xi = x.detach().requires_grad_(True)
    with context.use(ctx):
      y = forward(xi, ids)
      y.backward(dy64.to(DEV, torch.float32))
    torch.cuda.synchronize()
    xr = x64.clone().requires_grad_(True)
    pr = {n: p.clone().requires_grad_(True) for n, p in params.items()}
    want = ref.embedding_postprocessor(xr, pr, 'LayerNorm', ids64, 'token_type/token_type_embeddings',
                                       'position_embedding/txt_position_embeddings_0')
    (want * dy64).sum().backward()
    _close(y, want, 1e-5, 'y')
    _close(xi.grad, xr.grad, 1e-4, 'dx')
    for n, gr in vs.grad_dict().items():
      _close(gr, pr[n].grad, 1e-4, n)
