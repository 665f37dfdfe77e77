"""The streaming attention kernels (csrc/er_mha_stream.hip, include/easyrec_hip.h K8f-s) on the GPU: er_mha_stream_fwd /
_bwd through the C ABI against the fp64 composition (oracle/uniter_ref.attention_core) under autograd, on inputs that
are fp32 values cast to fp64.  Every output buffer goes to the library full of NaN: every owned element must come back
finite and the padding columns of a padded pitch must stay NaN.

Bars: tests/_oracle_steps.close with FWD_BAR = 1e-5 (ctx) and GRAD_BAR = 1e-4 (dQ, dK, dV).  Where the plain fp32 torch
composition (layers/multihead_cross_attention.attention_compose on the CPU) already sits above a third of such a bar
against the same fp64 values - the 4096-term rows, the saturated rows - the bar is 4 x that measured error (DESIGN.md
3.22); the measurement is printed beside every figure.  The fp64 reference and the fp32 composition are asserted finite
on every input.

A key tile is 64 keys up to ds = 64 and 32 above; a sub-tile (one rescale) is 32 keys; a wave owns 32 query rows."""
import logging

import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.layers import multihead_cross_attention as mca  # noqa: E402
from oracle import uniter_ref as ref  # noqa: E402
from tests import _attention_cases as ac  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402
from tests._oracle_steps import close as _close  # noqa: E402
from tests.test_attention_edges_gpu import _attention_layer_run  # noqa: E402  (the edges test's launch-name capture)

logging.disable(logging.WARNING)
DEV = 'cuda:0'
NAN = float('nan')
B = 4
# (F, T, ds, H)
CASES = [
    (35, 35, 128, 2),  # the first square outside the LDS envelope; a 3-row tail in the second row block
    (1, 65, 8, 1),     # one row; a one-key tail after a full tile
    (33, 64, 128, 1),  # a one-row tail; keys exactly two tiles; the largest head
    (70, 130, 20, 3),  # three key tiles; a head that is no multiple of the MFMA block
    (129, 1, 16, 2),   # ctx is V's row; dQ = dK = 0 exactly
    (2, 4096, 4, 1),   # 128 rescales per row; the top of the envelope
    (4096, 2, 4, 1),   # the top of the envelope on the query side
]


def _f32(t):
  return t.to(ac.F32).to(ac.F64)


def _mask(T, ds, seed):
  """Random keys; example 0: only the LAST key open; example 1: every key masked; example 2 (T beyond one tile): only
  the second tile's keys open, so that the running maximum climbs from the -10000 level to a real score."""
  m = ref.mixed_mask(B, T, seed)
  m[0] = 0
  m[0, T - 1] = 1
  tile = 64 if ds <= 64 else 32
  if T > tile:
    m[2] = 0
    m[2, tile:2 * tile] = 1
  return m


def _inputs(F, T, ds, H, masked, seed=0, top=None, ascending=False):
  g = torch.Generator().manual_seed(1000 * F + T + ds + H + seed)
  q, k, v, dctx = (_f32(torch.randn(B * n, H * ds, generator=g, dtype=ac.F64)) for n in (F, T, T, F))
  if ascending:  # the scores rise by ~20 / T per key along a common direction: every sub-tile raises the row maximum
    ramp = torch.arange(1, T + 1, dtype=ac.F64).repeat(B)[:, None] * (20.0 * 4.0 / T)
    q, k = _f32(0.1 * q + ds ** -0.5), _f32(0.1 * k + ramp * ds ** -0.5)
  if top is not None:  # saturated rows, as the _top80 cases of _attention_cases
    q = _f32(q * (top / float(ac.mha_scores(q, k, B, F, T, H, ds).max())))
  return dict(q=q, k=k, v=v, dctx=dctx, mask=_mask(T, ds, seed + 3) if masked else None, B=B)


def _eval(inp, dims, dt, fn):
  F, T, ds, H = dims
  q, k, v = (inp[n].to(dt).clone().requires_grad_(True) for n in ('q', 'k', 'v'))
  ctx = fn(q, k, v, inp['mask'], B, F, T, H, ds)
  dq, dk, dv = torch.autograd.grad(ctx, (q, k, v), inp['dctx'].to(dt))
  return dict(ctx=ctx.detach(), dq=dq, dk=dk, dv=dv)


def _nan(*shape):
  return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _run(inp, dims, packed=False, pad=0):
  """One forward and one backward call on a packed [rows, 3 H ds] buffer or on separate Q and K | V buffers, every row
  `pad` floats longer than its data.  -> dict(ctx, dq, dk, dv)."""
  F, T, ds, H = dims
  be, d = kernels.hip(), H * ds
  if packed:
    src, grad = _nan(B * F, 3 * d + pad), _nan(B * F, 3 * d + pad)
    cols, grads = [(src, i * d) for i in range(3)], [(grad, 3 * d)]
  else:
    qs, kvs, gq, gkv = _nan(B * F, d + pad), _nan(B * T, 2 * d + pad), _nan(B * F, d + pad), _nan(B * T, 2 * d + pad)
    cols, grads = [(qs, 0), (kvs, 0), (kvs, d)], [(gq, d), (gkv, 2 * d)]
  gbufs = [grad] * 3 if packed else [gq, gkv, gkv]
  ins, outs = [], []
  for (buf, c), gbuf, n in zip(cols, gbufs, 'qkv'):
    buf[:, c:c + d] = inp[n].to(DEV, torch.float32)
    ins.append(buf[:, c:c + d])
    outs.append(gbuf[:, c:c + d])
  mask = None if inp['mask'] is None else inp['mask'].to(DEV).contiguous()
  dctx = inp['dctx'].to(DEV, torch.float32).contiguous()
  ctx, lse, delta = _nan(B * F, d), _nan(B, H, F), _nan(B, H, F)
  ptrs = [x for t in ins for x in (t.data_ptr(), t.stride(0))] + [None if mask is None else mask.data_ptr()]
  stream = torch.cuda.current_stream().cuda_stream
  be.ck.er_mha_stream_fwd(*ptrs, B, F, T, H, ds, ctx.data_ptr(), lse.data_ptr(), stream)
  be.ck.er_mha_stream_bwd(*ptrs, dctx.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, F, T, H, ds, delta.data_ptr(),
                          *[x for t in outs for x in (t.data_ptr(), t.stride(0))], stream)
  torch.cuda.synchronize()
  got = dict(ctx=ctx, dq=outs[0], dk=outs[1], dv=outs[2])
  for n, t in list(got.items()) + [('lse', lse), ('delta', delta)]:
    assert bool(torch.isfinite(t).all()), (n, 'an element was not written or is not finite')
  for gbuf, used in grads:
    assert bool(torch.isnan(gbuf[:, used:]).all()), 'a padding column was written'
  return got


def _check(inp, dims, got, what):
  want, plain = _eval(inp, dims, ac.F64, ref.attention_core), _eval(inp, dims, ac.F32, mca.attention_compose)
  for n in ac.MHA_TENSORS:
    assert bool(torch.isfinite(want[n]).all()) and bool(torch.isfinite(plain[n]).all()), (what, n)
    if not want[n].any():
      assert not bool(got[n].any()), (what, n, 'exactly 0 in fp64')
      continue
    default, err32 = (ac.FWD_BAR if n == 'ctx' else ac.GRAD_BAR), ac.measure(plain[n], want[n])
    bar = 4.0 * err32 if err32 > default / 3.0 else default
    print('STREAM %s %s=%.3g bar=%.3g fp32-composition=%.3g' % (what, n, ac.measure(got[n], want[n]), bar, err32))
    _close(got[n], want[n], bar, (what, n))


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('dims', CASES, ids=lambda c: 'f%d_t%d_ds%d_h%d' % c)
def test_stream_kernels_match_fp64_autograd(dims, masked):
  F, T, ds, H = dims
  inp = _inputs(F, T, ds, H, masked)
  got = _run(inp, dims)
  _check(inp, dims, got, (dims, masked))
  if T == 1:  # softmax over one key: P = 1, ctx is V's row to the bit
    rows = inp['v'].view(B, 1, H * ds).expand(B, F, H * ds).reshape(B * F, H * ds)
    assert torch.equal(got['ctx'].cpu(), rows.to(torch.float32))


@pytest.mark.parametrize('what,dims,kw', [
    ('packed', (70, 70, 20, 3), dict(packed=True)),       # one [rows, 3 H ds] self-attention buffer
    ('padded', (37, 70, 21, 2), dict(pad=3)),             # pitch % 4 != 0 and an odd head: 4-byte accesses, ds + 1 zeroed
    ('padded16', (37, 70, 20, 2), dict(pad=4)),           # a padded pitch on the 16-byte path
    ('ascending', (40, 224, 16, 1), dict(ascending=True)),  # every sub-tile raises the row maximum: a rescale each
    ('top80', (70, 130, 8, 3), dict(top=80.0)),           # saturated rows
], ids=lambda v: v if isinstance(v, str) else None)
def test_stream_layouts_rescales_and_saturation(what, dims, kw):
  F, T, ds, H = dims
  run_kw = {k: v for k, v in kw.items() if k in ('packed', 'pad')}
  kw = {k: v for k, v in kw.items() if k not in run_kw}
  inp = _inputs(F, T, ds, H, masked=not kw, **kw)
  if 'ascending' in kw:
    s = ac.mha_scores(inp['q'], inp['k'], B, F, T, H, ds)
    tops = torch.stack([s[..., j:j + 32].max(dim=-1).values for j in range(0, T, 32)])
    assert bool((tops[1:] > tops[:-1] + 1.0).all())
  _check(inp, dims, _run(inp, dims, **run_kw), what)


def test_two_runs_and_a_graph_replay_are_bit_identical():
  """(70, 130, 20, 3) masked, 2049 units: more items than one walk of the 2048 persistent workgroups in every pass."""
  be = kernels.hip()
  F, T, ds, H, Bn = 70, 130, 20, 3, 683
  d = H * ds
  assert all(be.mha_stream_grid(Bn, F, T, H, ds, p) == 2048 < Bn * H for p in (0, 1, 2))
  q, kv, dctx = torch.randn(Bn * F, d, device=DEV), torch.randn(Bn * T, 2 * d, device=DEV), torch.randn(Bn * F, d, device=DEV)
  mask = ref.mixed_mask(Bn, T, 6).to(DEV)

  def run():
    ctx, lse = be.mha_stream_fwd(q, kv[:, :d], kv[:, d:], mask, Bn, F, T, H, ds)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    be.mha_stream_bwd(q, kv[:, :d], kv[:, d:], mask, dctx, ctx, lse, Bn, F, T, H, ds, dq, dkv[:, :d], dkv[:, d:])
    return [ctx, lse, dq, dkv]

  assert_runs_and_replay_bit_identical(run)
  assert all(bool(torch.isfinite(t).all()) for t in run())


@pytest.mark.parametrize('n,switch,expect', [
    (35, '1', ['er::attn_stream_bwd_dkv_kernel', 'er::attn_stream_bwd_dq_kernel', 'er::attn_stream_fwd_kernel']),
    (34, '1', ['er::mha_bwd_kernel', 'er::mha_fwd_kernel']),
    (35, '0', []),
])
def test_attention_layer_dispatch(n, switch, expect, monkeypatch):
  """(35, 35, 128) launches the stream kernels, (34, 34, 128) the LDS-resident ones only, and with
  EASYREC_AMD_MHA_STREAM=0 the outside shape launches neither; all hold the bars."""
  monkeypatch.setenv('EASYREC_AMD_MHA_STREAM', switch)
  assert mca.fits(n, n, 128) == (n == 34) and mca.stream_fits(n, n, 128)
  y, dx, want, dx64, names = _attention_layer_run(n, monkeypatch)
  assert sorted(k for k in names if k.startswith(('er::mha_', 'er::attn_stream_'))) == expect, names
  _close(y, want, ac.FWD_BAR, (n, switch, 'y'))
  _close(dx, dx64, ac.GRAD_BAR, (n, switch, 'dx'))


def test_shapes_outside_the_envelope_are_refused_and_not_launched():
  be = kernels.hip()
  x = torch.zeros(64, device=DEV)
  p, stream = x.data_ptr(), torch.cuda.current_stream().cuda_stream
  for F, T, ds in ((4, 4, 129), (4097, 4, 4), (4, 0, 4)):
    assert not mca.stream_fits(F, T, ds) and be.mha_stream_grid(1, F, T, 1, ds, 0) == 0
    assert be.lib.er_mha_stream_fwd(p, 129, p, 129, p, 129, None, 1, F, T, 1, ds, p, p, stream) != 0
    assert be.lib.er_mha_stream_bwd(p, 129, p, 129, p, 129, None, p, p, p, 1, F, T, 1, ds, p, p, 129, p, 129, p, 129,
                                    stream) != 0
  assert mca.stream_fits(4096, 4096, 128) and be.mha_stream_lds_bytes(128) == 33296 and be.mha_stream_lds_bytes(64) == 33808
  assert be.mha_stream_lds_bytes(129) == 0 and max(be.mha_stream_lds_bytes(ds) for ds in range(1, 129)) <= mca.LDS_BUDGET
  torch.cuda.synchronize()
  assert not bool(x.any())
