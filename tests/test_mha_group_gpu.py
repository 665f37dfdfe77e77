"""The grouped-unit attention launches and segment mean pooling (csrc/er_mha.hip, K8f) on the GPU.

er_mha_group_fwd / _bwd against er_mha_fwd / _bwd BIT FOR BIT (torch.equal on ctx, dQ, dK, dV): an output element is the
same one-thread chain over k and a softmax row the same wave butterfly, whichever threads own the unit; plus two runs
and a hipGraph replay with new inputs, one shape against the fp64 composition, and the refusal of a shape with room
for one unit only.  er_segment_mean_fwd / _bwd against fp64 within the derived bound of a sequential sum, its backward
exactly, rows past the length exactly 0, a zero length NaN in its own segment only, and a graph replay."""
import logging

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.layers import multihead_cross_attention as mca  # noqa: E402
from oracle import cmbf_ref as cref  # noqa: E402
from oracle import uniter_ref as ref  # noqa: E402
from tests._oracle_steps import close as _close  # noqa: E402

logging.disable(logging.WARNING)
DEV = 'cuda:0'

# (F, T, ds, H): a single element; CMBF's sample shapes (image -> text, text -> image, text self); small odd shapes,
# the last with an odd head size (4-byte staging)
SHAPES = [(1, 1, 1, 1), (1, 33, 16, 2), (33, 1, 16, 2), (33, 33, 16, 2), (5, 3, 4, 3), (9, 7, 3, 2)]


def _inputs(B, F, T, H, ds, seed, pad=0):
  """Separate Q and K | V buffers (row pitches d + pad and 2 d + pad) and dctx, fp32 on the device."""
  d = H * ds
  g = torch.Generator().manual_seed(seed)
  q = torch.randn(B * F, d + pad, generator=g).to(DEV)
  kv = torch.randn(B * T, 2 * d + pad, generator=g).to(DEV)
  dctx = torch.randn(B * F, d, generator=g).to(DEV)
  return q, kv, dctx


def _both(q, k, v, to_mask, dctx, B, F, T, H, ds, like_q, like_kv, d):
  """-> [(ctx, dq buffer, dkv buffer) of the one-unit launches, the same of the grouped launches]"""
  be = kernels.hip()
  out = []
  for fwd, bwd in ((be.mha_fwd, be.mha_bwd), (be.mha_group_fwd, be.mha_group_bwd)):
    ctx = fwd(q, k, v, to_mask, B, F, T, H, ds)
    dq, dkv = torch.full_like(like_q, float('nan')), torch.full_like(like_kv, float('nan'))
    if like_q is like_kv:  # the packed buffer: dQ | dK | dV side by side
      dkv = dq
      bwd(q, k, v, to_mask, dctx, B, F, T, H, ds, dq[:, :d], dq[:, d:2 * d], dq[:, 2 * d:3 * d])
    else:
      bwd(q, k, v, to_mask, dctx, B, F, T, H, ds, dq[:, :d], dkv[:, :d], dkv[:, d:2 * d])
    out.append((ctx, dq, dkv))
  torch.cuda.synchronize()
  return out


def _assert_same_bits(one, grouped, d, what):
  (c1, q1, kv1), (c2, q2, kv2) = one, grouped
  assert not torch.isnan(c1).any() and torch.equal(c1, c2), (what, 'ctx')
  # (the written columns; a padded pitch leaves its padding columns NaN in both)
  assert not torch.isnan(q1[:, :d]).any() and torch.equal(q1[:, :d], q2[:, :d]), (what, 'dQ')
  w = 3 * d if q1 is kv1 else 2 * d
  assert not torch.isnan(kv1[:, :w]).any() and torch.equal(kv1[:, :w], kv2[:, :w]), (what, 'dK | dV')


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'F%d_T%d_ds%d_H%d' % s)
def test_grouped_launches_give_the_one_unit_launches_bits(shape, masked):
  """Every shape with B * H in {1, G - 1, G, G + 1, 3 G + 1} units (a partial pass, a full one, several), separate
  buffers, and the packed Q | K | V buffer where F == T.  The mask: random keys, example 0 with a single open key, example 1 with every
  key masked."""
  F, T, ds, H = shape
  G = kernels.hip().mha_group_units(F, T, ds)
  assert G == mca.mha_group_units(F, T, ds) and G >= 2
  units = sorted({1, G - 1, G, G + 1, 3 * G + 1})
  # with the shape's own head count the batches whose B * H brackets each of those unit counts; with one head exactly them
  plans = [(H, sorted({max(1, u // H) for u in units} | {-(-u // H) for u in units}))] + ([(1, units)] if H > 1 else [])
  seen_units = set()
  for heads, batches in plans:
    d = heads * ds
    for B in batches:
      seen_units.add(B * heads)
      q, kv, dctx = _inputs(B, F, T, heads, ds, 10 * B + F)
      to_mask = ref.mixed_mask(B, T, B).to(DEV) if masked else None
      one, grouped = _both(q, kv[:, :d], kv[:, d:], to_mask, dctx, B, F, T, heads, ds, q, kv, d)
      _assert_same_bits(one, grouped, d, (shape, heads, B, 'separate'))
      if F == T:
        qkv = torch.cat([q, kv], dim=1).contiguous()
        one, grouped = _both(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], to_mask, dctx, B, F, T, heads, ds, qkv, qkv, d)
        _assert_same_bits(one, grouped, d, (shape, heads, B, 'packed'))
  assert seen_units >= set(units)


@pytest.mark.parametrize('shape', [(33, 33, 16, 2), (5, 3, 4, 3)], ids=lambda s: 'F%d_T%d_ds%d_H%d' % s)
def test_pitches_that_are_no_multiple_of_four(shape):
  """Row pitches d + 1 and 2 d + 3 floats: the staging takes 4-byte loads (and at ds = 16 differs from the aligned case
  in nothing else); the same bits as the one-unit launches, and as the aligned launch."""
  F, T, ds, H = shape
  B, d = 5, H * ds
  g = torch.Generator().manual_seed(77)
  qb = torch.randn(B * F, d + 1, generator=g).to(DEV)
  kvb = torch.randn(B * T, 2 * d + 3, generator=g).to(DEV)
  dctx = torch.randn(B * F, d, generator=g).to(DEV)
  to_mask = ref.mixed_mask(B, T, 3).to(DEV)
  q, k, v = qb[:, :d], kvb[:, :d], kvb[:, d:2 * d]
  assert q.stride(0) % 4 != 0 and k.stride(0) % 4 != 0
  one, grouped = _both(q, k, v, to_mask, dctx, B, F, T, H, ds, qb, kvb, d)
  _assert_same_bits(one, grouped, d, (shape, 'odd pitch'))
  aligned = kernels.hip().mha_group_fwd(q.contiguous(), k.contiguous(), v.contiguous(), to_mask, B, F, T, H, ds)
  torch.cuda.synchronize()
  assert torch.equal(aligned, grouped[0])


def test_more_units_than_one_walk_of_the_grid():
  """B = 4101, H = 2 at (1, 1, 1): 8202 units > G * 1024 = 8192, so the first workgroups walk twice and the last pass is
  partial."""
  B, F, T, H, ds = 4101, 1, 1, 2, 1
  assert kernels.hip().mha_group_units(F, T, ds) == 8 and B * H > 8 * 1024
  q, kv, dctx = _inputs(B, F, T, H, ds, 5)
  to_mask = ref.mixed_mask(B, T, 2).to(DEV)
  d = H * ds
  one, grouped = _both(q, kv[:, :d], kv[:, d:], to_mask, dctx, B, F, T, H, ds, q, kv, d)
  _assert_same_bits(one, grouped, d, 'two walks')
  assert torch.equal(grouped[0], kv[:, d:])  # (one key: P = 1, ctx = V)


def test_two_runs_and_a_graph_replay_with_new_inputs():
  B, F, T, H, ds = 37, 33, 33, 2, 16
  d = H * ds
  be = kernels.hip()
  to_mask = ref.mixed_mask(B, T, 4).to(DEV)
  def packed(seed):  # ([B F, 3 d]: the packed buffer, and dctx [B F, d])
    x, _, dy = _inputs(B, F, T, H, 3 * ds, seed)
    return x, dy[:, :d].contiguous()

  qkv, dctx = packed(1)
  assert qkv.shape == (B * F, 3 * d) and dctx.shape == (B * F, d)

  def run(x, dy):
    ctx = be.mha_group_fwd(x[:, :d], x[:, d:2 * d], x[:, 2 * d:], to_mask, B, F, T, H, ds)
    dx = torch.empty_like(x)
    be.mha_group_bwd(x[:, :d], x[:, d:2 * d], x[:, 2 * d:], to_mask, dy, B, F, T, H, ds, dx[:, :d], dx[:, d:2 * d], dx[:, 2 * d:])
    return ctx, dx

  first, second = run(qkv, dctx), run(qkv, dctx)
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(first, second))
  sx, sdy = qkv.clone(), dctx.clone()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    run(sx, sdy)  # (warm-up on the capture stream)
  torch.cuda.current_stream().wait_stream(s)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    static = run(sx, sdy)
  graph.replay()
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(first, static))
  qkv2, dctx2 = packed(2)
  sx.copy_(qkv2)
  sdy.copy_(dctx2)
  graph.replay()
  want = run(qkv2, dctx2)
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(want, static)) and not torch.equal(want[0], first[0])


def test_grouped_attention_against_the_fp64_composition():
  """(33, 33, 16) x 2 heads through MhaGroupAttnFn (the packed form) and (1, 33, 16) in the cross form: 1e-5 forward,
  1e-4 gradients."""
  for B, F, T, H, ds in ((9, 33, 33, 2, 16), (9, 1, 33, 2, 16)):
    d = H * ds
    g = torch.Generator().manual_seed(F)
    q64, k64, v64 = (torch.randn(B * n, d, generator=g, dtype=torch.float64) for n in (F, T, T))
    dctx64 = torch.randn(B * F, d, generator=g, dtype=torch.float64)
    mask = ref.mixed_mask(B, T, 8)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q64, k64, v64))
    want = ref.attention_core(qr, kr, vr, mask, B, F, T, H, ds)
    (want * dctx64).sum().backward()
    if F == T:
      src = torch.cat([q64, k64, v64], dim=1).to(DEV, torch.float32).requires_grad_(True)
      out = kernels.MhaGroupAttnFn.apply(src, None, mask.to(DEV), B, F, T, H, ds)
      out.backward(dctx64.to(DEV, torch.float32))
      dq, dk, dv = src.grad[:, :d], src.grad[:, d:2 * d], src.grad[:, 2 * d:]
    else:
      qs = q64.to(DEV, torch.float32).requires_grad_(True)
      kvs = torch.cat([k64, v64], dim=1).to(DEV, torch.float32).requires_grad_(True)
      out = kernels.MhaGroupAttnFn.apply(qs, kvs, mask.to(DEV), B, F, T, H, ds)
      out.backward(dctx64.to(DEV, torch.float32))
      dq, dk, dv = qs.grad, kvs.grad[:, :d], kvs.grad[:, d:]
    torch.cuda.synchronize()
    _close(out, want, 1e-5, 'ctx')
    _close(dq, qr.grad, 1e-4, 'dQ')
    _close(dk, kr.grad, 1e-4, 'dK')
    _close(dv, vr.grad, 1e-4, 'dV')


def test_a_shape_with_room_for_one_unit_is_refused_and_nothing_is_launched():
  B, F, T, H, ds = 2, 33, 33, 1, 128
  be = kernels.hip()
  assert be.mha_group_units(F, T, ds) == 1 and mca.mha_group_units(F, T, ds) == 1
  q, kv, dctx = _inputs(B, F, T, H, ds, 1)
  d = H * ds
  be.op_log = []
  try:
    with pytest.raises(RuntimeError, match='one unit per workgroup'):
      be.mha_group_fwd(q, kv[:, :d], kv[:, d:], None, B, F, T, H, ds)
    sentinel = torch.full_like(kv, 7.0)
    dq = torch.full_like(q, 7.0)
    with pytest.raises(RuntimeError, match='one unit per workgroup'):
      be.mha_group_bwd(q, kv[:, :d], kv[:, d:], None, dctx, B, F, T, H, ds, dq, sentinel[:, :d], sentinel[:, d:])
    torch.cuda.synchronize()
    assert be.op_log == [] and bool((sentinel == 7.0).all()) and bool((dq == 7.0).all())
  finally:
    be.op_log = None
  ctx = be.mha_fwd(q, kv[:, :d], kv[:, d:], None, B, F, T, H, ds)  # (the one-unit launch serves it)
  torch.cuda.synchronize()
  assert bool(torch.isfinite(ctx).all())


# ------------------------------------------------------------------------------------------------ segment mean
CMBF_SEG = list(range(10)) + [25, 33]  # nine general tokens, title 16, genres 8


def _seg_case(B, seg, W, with_lens, seed):
  g = torch.Generator().manual_seed(seed)
  S, n_seg = seg[-1], len(seg) - 1
  x = torch.randn(B, S, W, generator=g)
  lens = None
  if with_lens:
    widths = torch.tensor([b - a for a, b in zip(seg, seg[1:])])
    lens = (torch.rand(B, n_seg, generator=g) * widths).floor().to(torch.int32) + 1  # 1 .. width
    lens[0] = 1
    lens[1] = widths.to(torch.int32)
  dout = torch.randn(B, n_seg, W, generator=g)
  return x, lens, dout


def _seg_check(x, seg, lens, dout):
  be = kernels.hip()
  B, S, W = x.shape
  n_seg = len(seg) - 1
  sb = torch.tensor(seg, dtype=torch.int32, device=DEV)
  lens_d = None if lens is None else lens.to(DEV)
  out = be.segment_mean_fwd(x.to(DEV), sb, lens_d, n_seg)
  assert out.shape == (B, n_seg, W)
  torch.cuda.synchronize()
  widths = np.array([b - a for a, b in zip(seg, seg[1:])])
  L = np.broadcast_to(widths, (B, n_seg)) if lens is None else np.minimum(np.maximum(lens.numpy(), 0), widths)
  want = cref.segment_mean(x.double().numpy(), seg, None if lens is None else lens.tolist())
  # an L-term sequential fp32 sum, then one division: |err| <= (L + 1) * 2^-24 * sum |x| / len per element
  xa = np.abs(x.double().numpy())
  bound = np.zeros_like(want)
  for s in range(n_seg):
    for b in range(B):
      n = int(L[b, s])
      bound[b, s] = (n + 1) * 2.0 ** -24 * xa[b, seg[s]:seg[s] + n].sum(axis=0) / max(n, 1)
  err = np.abs(out.double().cpu().numpy() - want)
  assert (err <= bound).all(), (float((err - bound).max()), W, n_seg)
  # backward: exactly dout / len in fp32 on the first len rows, exactly 0 on the rest; every element written
  # (the kernel allocates its result; a sentinel-filled buffer is handed to the library call itself)
  dx = torch.full((B, S, W), float('nan'), device=DEV)
  d = dout.to(DEV)
  be.ck.er_segment_mean_bwd(d.data_ptr(), sb.data_ptr(), None if lens_d is None else lens_d.data_ptr(), B, S, W, n_seg,
                            dx.data_ptr(), None)
  torch.cuda.synchronize()
  want_dx = torch.zeros(B, S, W)
  Lt = torch.from_numpy(np.ascontiguousarray(L)).to(torch.float32)
  for s in range(n_seg):
    gq = dout[:, s, :] / Lt[:, s:s + 1]  # (one fp32 IEEE division)
    for b in range(B):
      want_dx[b, seg[s]:seg[s] + int(L[b, s])] = gq[b]
  assert torch.equal(dx.cpu(), want_dx)
  assert torch.equal(be.segment_mean_bwd(d, sb, lens_d, S).cpu(), want_dx)
  return out


@pytest.mark.parametrize('with_lens', [True, False], ids=['lens', 'full'])
@pytest.mark.parametrize('W', [1, 3, 32, 36])
def test_segment_mean_on_cmbf_s_layout(W, with_lens):
  """33 tokens in 11 segments (nine of width 1, then 16 and 8), lengths 1 .. width with an all-1 and an all-full example;
  W 1 and 3 (4-byte accesses), 32 and 36 (16-byte accesses, 36 with a ragged last group of lanes)."""
  x, lens, dout = _seg_case(7, CMBF_SEG, W, with_lens, 3 + W)
  _seg_check(x, CMBF_SEG, lens, dout)


@pytest.mark.parametrize('seg', [[0, 5], list(range(65))], ids=['one_segment', 'sixty_four_segments'])
def test_segment_mean_with_one_and_with_sixty_four_segments(seg):
  for W, with_lens in ((8, True), (3, False)):
    x, lens, dout = _seg_case(3, seg, W, with_lens, 9)
    _seg_check(x, seg, lens, dout)


def test_segment_mean_misaligned_base_takes_the_scalar_path():
  """W = 32 from a base 4 bytes off a 16-byte boundary: the same values as the aligned call."""
  x, lens, dout = _seg_case(4, CMBF_SEG, 32, True, 5)
  be = kernels.hip()
  sb = torch.tensor(CMBF_SEG, dtype=torch.int32, device=DEV)
  flat = torch.empty(x.numel() + 1, device=DEV)
  off = flat[1:].view(x.shape)
  off.copy_(x)
  assert off.data_ptr() % 16 == 4
  a = be.segment_mean_fwd(x.to(DEV), sb, lens.to(DEV), 11)
  b = be.segment_mean_fwd(off, sb, lens.to(DEV), 11)
  torch.cuda.synchronize()
  assert torch.equal(a, b)


def test_a_zero_length_is_nan_in_its_own_segment_only_and_its_gradient_is_zero():
  x, lens, dout = _seg_case(4, [0, 2, 6, 7], 4, True, 2)
  lens[2, 1] = 0
  be = kernels.hip()
  sb = torch.tensor([0, 2, 6, 7], dtype=torch.int32, device=DEV)
  out = be.segment_mean_fwd(x.to(DEV), sb, lens.to(DEV), 3)
  dx = be.segment_mean_bwd(dout.to(DEV), sb, lens.to(DEV), 7)
  torch.cuda.synchronize()
  nan = torch.isnan(out).all(dim=-1).cpu()
  want = torch.zeros(4, 3, dtype=torch.bool)
  want[2, 1] = True
  assert torch.equal(nan, want) and not torch.isnan(out[~want.to(DEV)]).any()
  assert bool((dx[2, 2:6] == 0).all()) and bool(torch.isfinite(dx).all())
  # the layer function and its autograd form
  xs = x.to(DEV).requires_grad_(True)
  y = mca.segment_mean(xs, [0, 2, 6, 7], lens.to(DEV))
  y[~want.to(DEV)].sum().backward()
  torch.cuda.synchronize()
  keep = ~want.to(DEV)  # (NaN is not equal to itself: the other segments bit for bit, the empty one NaN again)
  assert torch.equal(y.detach()[keep], out[keep]) and bool(torch.isnan(y.detach()[~keep]).all())
  assert bool(torch.isfinite(xs.grad).all())


def test_segment_mean_replays_in_a_graph_with_new_inputs():
  x, lens, dout = _seg_case(6, CMBF_SEG, 32, True, 1)
  be = kernels.hip()
  sb = torch.tensor(CMBF_SEG, dtype=torch.int32, device=DEV)
  sx, sl, sd = x.to(DEV), lens.to(DEV), dout.to(DEV)

  def run():
    return be.segment_mean_fwd(sx, sb, sl, 11), be.segment_mean_bwd(sd, sb, sl, 33)

  first = [t.clone() for t in run()]
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    run()
  torch.cuda.current_stream().wait_stream(s)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    static = run()
  graph.replay()
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(first, static))
  x2, lens2, dout2 = _seg_case(6, CMBF_SEG, 32, True, 2)
  sx.copy_(x2)
  sl.copy_(lens2)
  sd.copy_(dout2)
  graph.replay()
  torch.cuda.synchronize()
  got = [t.clone() for t in static]
  want = run()
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(want, got)) and not torch.equal(got[0], first[0])
