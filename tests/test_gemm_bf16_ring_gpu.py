"""-m gpu: the bf16 contractions at every edge of their k-tile ring and their epilogues (csrc/er_gemm_bf16.hip:
er_gemm_bf16_nt[_epi], er_cast_bf16; csrc/er_gemm.hip: er_gemm_bf16).

er_gemm_bf16_nt DMAs k-tiles of 64 into a ring of 4 XOR-swizzled LDS tile pairs, three tiles ahead, with hand-counted
waits, a barrier in the middle of each tile and zero-source tiles issued past the end; its epilogues store 16-byte pieces
under row predicates.  What such a kernel can get wrong is a k-chunk that is dropped, read twice, read before it landed or
after it was overwritten, a k-tail that is not masked, a store that is lost or lands outside the output.  tests/
_bf16_cases.py holds the cases (and the reasons for every shape), the operands and the expected values; this file launches
and compares:
  * exact integer operands: equality with the int64 product (+ bias + base), for fp32 and bf16 outputs,
  * random operands: the fp64 product of the rounded operands within the bounds the project holds these entry points to,
  * operand rows padded with NaN behind K: an unmasked k-tail chunk poisons the output,
  * every tensor a launch writes is a window inside a sentinel-filled buffer: guards in front, behind and between rows,
  * the same bits on a second launch.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.kernels import _p, _stream  # noqa: E402
from tests import _bf16_cases as bc  # noqa: E402
from tests._bf16_cases import Window, bits  # noqa: E402

DEV = 'cuda:0'
BF = torch.bfloat16


@pytest.fixture(scope='module')
def hip():
  assert torch.cuda.is_available(), 'gpu tests need an MI355X'
  be = kernels.hip()
  be._ck(be.lib.er_gemm_bf16_nt_prepare(), 'prepare')
  return be


def _epi(**kw):
  return kernels.GemmEpilogue(**{k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in kw.items()})


def _win(R, C, ld=None, dtype=torch.float32, base=None):
  return Window(R, C, ld, dtype=dtype, device=DEV, base=base)


# ---------------------------------------------------------------------------------------------- the ring, plain epilogue
@pytest.mark.parametrize('K', bc.KS)
def test_ring_exact_operands_over_every_edge(hip, K):
  """M x N of the module's lists, five output variants each: fp32 out; + bias with pitch N + 3; C += with bias, pitch
  round4(N) + 4 (twice: the same bits); bf16 out only; fp32 + bf16 out.  Every output equals the integer result."""
  e = bc.exact_for_k(K)
  a16, b16 = bc.poisoned_bf16(e.a, DEV), bc.poisoned_bf16(e.b, DEV)
  bias = e.bias.to(DEV)
  for M in bc.MS:
    for N in bc.NS:
      p0, p1, p2 = bc.pitches(N)
      base = e.base[:M, :N]
      plain = e.expected(M, N)
      runs = []
      w = _win(M, N, p0)
      hip.gemm_bf16_nt(a16, b16, M, N, K, out=w.out)
      runs.append(('fp32', w, plain))
      w = _win(M, N, p1)
      hip.gemm_bf16_nt(a16, b16, M, N, K, out=w.out, bias=bias)
      runs.append(('bias, pitch N + 3', w, e.expected(M, N, bias=True)))
      for again in (0, 1):
        w = _win(M, N, p2, base=base)
        hip.gemm_bf16_nt(a16, b16, M, N, K, out=w.out, bias=bias, accumulate=True)
        runs.append(('C += with bias, pitch round4(N) + 4, launch %d' % again, w, e.expected(M, N, bias=True, base=True)))
      w = _win(M, N, p0, dtype=BF)
      hip.gemm_bf16_nt(a16, b16, M, N, K, out_bf16=w.out)
      runs.append(('bf16 only', w, plain.to(BF)))
      w, wb = _win(M, N, p2), _win(M, N, p2 + 4, dtype=BF)
      hip.gemm_bf16_nt(a16, b16, M, N, K, out=w.out, out_bf16=wb.out)
      runs += [('fp32 beside bf16', w, plain), ('bf16 beside fp32', wb, plain.to(BF))]
      got = {}
      for name, w, exp in runs:
        what = (name, M, N, K)
        got[name] = w.read(what)
        assert torch.equal(got[name], exp), (what, int((got[name] != exp).sum()))
      assert torch.equal(bits(got[runs[2][0]]), bits(got[runs[3][0]]))


@pytest.mark.parametrize('K', bc.KS)
def test_ring_random_operands(hip, K):
  """randn rounded to bf16, fp32 + bf16 out: against the fp64 product of the rounded operands at test_gemm_bf16_nt's bound;
  finite; the same bits on a second launch and on one whose pitch forces scalar stores; guards intact"""
  r = bc.random_for_k(K)
  a16, b16 = bc.poisoned_bf16(r.a, DEV), bc.poisoned_bf16(r.b, DEV)
  for M, N in bc.RANDOM_MN:
    ref, bound = r.ref[:M, :N], r.bound(bc.NT_REL)[:M, :N]
    outs = []
    for ld in (bc.round4(N) + 4, bc.round4(N) + 4, N + 3):
      w, wb = _win(M, N, ld), _win(M, N, ld + 4, dtype=BF)
      hip.gemm_bf16_nt(a16, b16, M, N, K, out=w.out, out_bf16=wb.out)
      outs.append((w, wb))
    for i, (w, wb) in enumerate(outs):
      what = ('random', i, M, N, K)
      out, outb = w.read(what), wb.read(what)
      assert torch.isfinite(out).all(), what
      err = (out.double() - ref).abs()
      assert (err <= bound).all(), (what, float((err - bound).max()))
      assert torch.equal(outb, out.to(BF)), what
      if i:
        assert torch.equal(bits(out), first), (what, 'not the bits of the first launch')
      else:
        first = bits(out)


@pytest.mark.parametrize('K', bc.KS)
def test_ring_matches_the_staging_kernel_bit_for_bit(hip, K):
  """er_gemm_bf16 (NT; one k-split below K = 1024) stages the same bf16 values through registers, one k-tile at a time, and
  issues the same v_mfma_f32_32x32x16_bf16 over k ascending into one accumulator, the bias added after: measured on an
  MI355X the two kernels agree in every bit on this K grid (0 of 3.3 million outputs differed), with and without bias.
  The bf16 counterpart of tests/test_gemm_kloop_gpu.py: a ring slot read early, late or twice changes bits here even where
  it would stay inside the fp64 bound."""
  r = bc.random_for_k(K)
  a16, b16 = bc.poisoned_bf16(r.a, DEV), bc.poisoned_bf16(r.b, DEV)
  bias = torch.randn(bc.N_MAX, generator=torch.Generator().manual_seed(K)).to(DEV)
  for M, N in bc.RANDOM_MN:
    av, bv = bc.aligned_f32(r.a[:M], DEV), bc.aligned_f32(r.b[:N], DEV)  # (bf16 values: the staging kernel's rounding keeps them)
    for with_bias in (False, True):
      w, ws = _win(M, N, bc.round4(N) + 4), _win(M, N, N + 3)
      hip.gemm_bf16_nt(a16, b16, M, N, K, out=w.out, bias=bias if with_bias else None)
      hip.gemm(kernels.GEMM_NT, av, bv, out=ws.out, bias=bias if with_bias else None, bf16=True)
      what = ('ring against staging', M, N, K, with_bias)
      got, ref = w.read(what), ws.read(what)
      assert torch.isfinite(got).all(), what
      diff = bits(got) != bits(ref)
      assert not diff.any(), (what, int(diff.sum()))


# ---------------------------------------------------------------------------------------------- epilogues at edges
@pytest.mark.parametrize('N,K', bc.EPI_NK)
@pytest.mark.parametrize('bias', [True, False])
def test_stats_epilogue_at_edges(hip, N, K, bias):
  """ER_EPI_STATS: z (fp32 and bf16) exact; per 64-row tile the counts exactly, mean and M2 merged over the tiles against
  fp64 statistics of the stored z; nothing written around z, its bf16 copy or the statistics"""
  e = bc.Exact(max(bc.EPI_BS), N, K, 3000 + N + K)
  a16, b16 = bc.poisoned_bf16(e.a, DEV), bc.poisoned_bf16(e.b, DEV)
  bias_d = e.bias.to(DEV) if bias else None
  for B in bc.EPI_BS:
    tiles = hip.gemm_row_tiles(B)
    assert tiles == bc.row_tiles(B)
    z, zb, st = _win(B, N, N + 4), _win(B, N, N + 8, dtype=BF), _win(tiles, 3 * N)
    hip.gemm_bf16_nt(a16, b16, B, N, K, out=z.out, out_bf16=zb.out, bias=bias_d,
                     epi=_epi(kind=kernels.EPI_STATS, col_stats=st.out))
    what = ('stats', B, N, K, bias)
    exp = e.expected(B, N, bias=bias)
    got = z.read(what)
    assert torch.equal(got, exp), what
    assert torch.equal(zb.read(what), exp.to(BF)), what
    bc.check_col_stats(st.read(what), got, what)


@pytest.mark.parametrize('N,K', bc.EPI_NK)
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('use_bn', [True, False])
def test_batchnorm_backward_epilogue_at_edges(hip, N, K, relu, use_bn):
  """ER_EPI_BN_BWD over the column blocks (0, N), (4, 8) and one ending at N: dy exact and the bits of a plain launch; the
  partial sums of the block over the row tiles; nothing written around dy or the partials"""
  e = bc.Exact(max(bc.EPI_BS), N, K, 3000 + N + K)
  a16, b16 = bc.poisoned_bf16(e.a, DEV), bc.poisoned_bf16(e.b, DEV)
  act = kernels.ACT_RELU if relu else kernels.ACT_NONE
  for B in bc.EPI_BS:
    tiles = hip.gemm_row_tiles(B)
    exp = e.expected(B, N)
    plain = _win(B, N, N + 4)
    hip.gemm_bf16_nt(a16, b16, B, N, K, out=plain.out)
    plain = plain.read(('plain', B, N, K))
    for col0, n_src in bc.bn_blocks(N):
      src = bc.BnSource(B, n_src, use_bn, relu, B + N + K + col0)
      zd, yd = bc.padded_rows_f32(src.z, DEV), bc.padded_rows_f32(src.y, DEV)
      dev = lambda t: None if t is None else t.to(DEV)
      zbias, mean, invstd = dev(src.zbias), dev(src.mean) if use_bn else None, dev(src.invstd) if use_bn else None
      dy, part = _win(B, N, N + 4), _win(tiles, 2 * n_src)
      epi = _epi(kind=kernels.EPI_BN_BWD, bn_z=zd, bn_y=yd, bn_partial=part.out, bn_ld=zd.stride(0), bn_use_bn=int(use_bn),
                 bn_act=int(act), bn_col0=col0, bn_n_src=n_src)
      if use_bn:
        epi.bn_zbias, epi.bn_mean, epi.bn_invstd = zbias.data_ptr(), mean.data_ptr(), invstd.data_ptr()
      hip.gemm_bf16_nt(a16, b16, B, N, K, out=dy.out, epi=epi)
      what = ('bn_bwd', B, N, K, col0, n_src, relu, use_bn)
      got = dy.read(what)
      assert torch.equal(got, exp), what
      assert torch.equal(bits(got), bits(plain)), what
      src.check_partial(part.read(what).view(tiles, n_src, 2), got[:, col0:col0 + n_src], what)


@pytest.mark.parametrize('d', bc.CROSS_DS)
@pytest.mark.parametrize('diag', [0.0, 0.5])
def test_cross_forward_epilogue_at_edges(hip, d, diag):
  """ER_EPI_CROSS_FWD with u on and off, the bf16 copy on: u and the output against the fp64 formula at the bounds of
  test_cross_forward_in_the_bf16_contraction; without u the same output bits; guards of out, its bf16 copy and u intact"""
  for B in bc.EPI_BS:
    c = bc.CrossFwd(B, d, 3 * B + d)
    xb, wt = bc.poisoned_bf16(c.xr, DEV), bc.poisoned_bf16(c.wtr, DEV)
    x0, x, b = bc.padded_rows_f32(c.x0, DEV), bc.padded_rows_f32(c.x, DEV), c.b.to(DEV)
    res = {}
    for with_u in (True, False):
      out, outb, u = _win(B, d, d + 4), _win(B, d, d + 8, dtype=BF), _win(B, d, d + 8)
      epi = _epi(kind=kernels.EPI_CROSS_FWD, diag=diag, x0=x0, xl=x, ld_x0=x0.stride(0), ld_xl=x.stride(0))
      if with_u:
        epi.u, epi.ld_u = u.out.data_ptr(), u.ld
      hip.gemm_bf16_nt(xb, wt, B, d, d, out=out.out, out_bf16=outb.out, bias=b, epi=epi)
      what = ('cross_fwd', B, d, diag, with_u)
      res[with_u] = out.read(what), outb.read(what), u.read(what)
    out, outb, u = res[True]
    c.check(u, out, outb, diag, ('cross_fwd', B, d, diag))
    assert torch.equal(bits(res[False][0]), bits(out)) and torch.equal(bits(res[False][1]), bits(outb))
    assert (res[False][2] == bc.SENT[torch.float32]).all(), 'u was written although it was not asked for'


@pytest.mark.parametrize('d', bc.CROSS_DS)
@pytest.mark.parametrize('diag', [0.0, 0.3])
def test_cross_backward_epilogue_at_edges(hip, d, diag):
  """ER_EPI_CROSS_BWD, per launch: the top form (C = v and C += v) and the form with a lower cross layer (dx0 written and
  accumulated into; du_out, du_out_bf16, partial on, and once off) against the fp64 formulas; every written tensor guarded"""
  for B in bc.EPI_BS:
    c = bc.CrossBwd(B, d, 5 * B + d)
    tiles = hip.gemm_row_tiles(B)
    dub, wb = bc.poisoned_bf16(c.du, DEV), bc.poisoned_bf16(c.w, DEV)
    pr = lambda t: bc.padded_rows_f32(t, DEV)
    dout, du, x0, prev_u, xl = pr(c.dout), pr(c.du), pr(c.x0), pr(c.prev_u), pr(c.xl)
    prev_bias = c.prev_bias.to(DEV)

    def epilogue(**kw):
      epi = _epi(kind=kernels.EPI_CROSS_BWD, diag=diag, dout=dout, ld_dout=dout.stride(0), **kw)
      if diag:
        epi.du_in, epi.ld_du_in = du.data_ptr(), du.stride(0)
      return epi

    for acc in (False, True):
      out = _win(B, d, d + 4, base=c.base if acc else None)
      hip.gemm_bf16_nt(dub, wb, B, d, d, out=out.out, accumulate=acc, epi=epilogue())
      what = ('cross_bwd top', B, d, diag, acc)
      c.check_out(out.read(what), diag, acc, what)
    res = {}
    for acc0, side in ((False, True), (True, True), (False, False)):
      out, dx0 = _win(B, d, d + 4), _win(B, d, d + 8, base=c.dx0_old)
      du_out, du_out_b, part = _win(B, d, d + 4), _win(B, d, d + 8, dtype=BF), _win(tiles, d)
      kw = dict(x0=x0, ld_x0=x0.stride(0), prev_u=prev_u, ld_prev_u=prev_u.stride(0), prev_bias=prev_bias,
                dx0=dx0.out, ld_dx0=dx0.ld, accumulate_dx0=int(acc0))
      if diag:
        kw.update(xl=xl, ld_xl=xl.stride(0))
      if side:
        kw.update(du_out=du_out.out, ld_du_out=du_out.ld, du_out_bf16=du_out_b.out, ld_du_out_bf16=du_out_b.ld, partial=part.out)
      hip.gemm_bf16_nt(dub, wb, B, d, d, out=out.out, epi=epilogue(**kw))
      what = ('cross_bwd lower', B, d, diag, acc0, side)
      res[(acc0, side)] = r = [w.read(what) for w in (out, dx0, du_out, du_out_b, part)]
      c.check_out(r[0], diag, False, what)
      if side:
        c.check_lower(r[0], r[2], r[3], r[1], r[4], diag, acc0, what)
    on, off = res[(False, True)], res[(False, False)]
    assert torch.equal(bits(on[0]), bits(off[0])) and torch.equal(bits(on[1]), bits(off[1]))
    assert all((t.float() == bc.SENT[t.dtype]).all() for t in off[2:]), 'a side output was written although it was not asked for'


# ---------------------------------------------------------------------------------------------- er_gemm_bf16
_VARIANTS = [('plain', 0, False, False), ('bias, ldc > N', 3, True, False), ('C +=, ldc > N', 5, False, True),
             ('C += with bias', 0, True, True)]


@pytest.mark.parametrize('layout', [kernels.GEMM_NN, kernels.GEMM_NT, kernels.GEMM_TN])
def test_staging_kernel_exact_operands(hip, layout):
  """er_gemm_bf16 (fp32 operands rounded while staged) through HipBackend.gemm(bf16=True): the shapes and four variants of
  tests/test_gemm_epilogue_edges_gpu.py, + two shapes that take k-splits; operands through 16-byte aligned views with NaN
  in the pitch and through unaligned ones.  Equality with the integer result, guards intact."""
  for M, N, K in bc.GEMM_SHAPES:
    e, a, b = bc.exact_gemm(layout, M, N, K)
    bias = e.bias.to(DEV)
    for view in (bc.aligned_f32, bc.unaligned_f32):
      av, bv = view(a, DEV), view(b, DEV)
      runs = []
      for name, pad, with_bias, acc in _VARIANTS:
        w = _win(M, N, N + pad, base=e.base if acc else None)
        hip.gemm(layout, av, bv, out=w.out, bias=bias if with_bias else None, accumulate=acc, bf16=True)
        runs.append((name, w, e.expected(bias=with_bias, base=acc)))
      for name, w, exp in runs:
        what = (name, view.__name__, layout, M, N, K)
        got = w.read(what)
        assert torch.equal(got, exp), (what, int((got != exp).sum()))


@pytest.mark.parametrize('layout', [kernels.GEMM_NN, kernels.GEMM_NT, kernels.GEMM_TN])
def test_staging_kernel_random_operands(hip, layout):
  """randn operands (the kernel rounds them): the fp64 product of torch's bf16 rounding at test_gemm_bf16's bound"""
  for M, N, K in bc.GEMM_SHAPES:
    r, a, b = bc.random_gemm(layout, M, N, K)
    outs = []
    for view, pad in ((bc.aligned_f32, 0), (bc.unaligned_f32, 3)):
      w = _win(M, N, N + pad)
      hip.gemm(layout, view(a, DEV), view(b, DEV), out=w.out, bf16=True)
      outs.append((view.__name__, w))
    for name, w in outs:
      what = (name, layout, M, N, K)
      got = w.read(what)
      assert torch.isfinite(got).all(), what
      err = (got.double() - r.ref).abs()
      assert (err <= r.bound(bc.GEMM_REL)).all(), (what, float((err - r.bound(bc.GEMM_REL)).max()))


@pytest.mark.parametrize('M,N,K', bc.GEMM_STATS_SHAPES)
def test_staging_kernel_column_statistics(hip, M, N, K):
  """col_stats of er_gemm_bf16 (NN, bias, ldc > N): z exact, the statistics with the fp32 test's checks, guards intact"""
  e, a, b = bc.exact_gemm(kernels.GEMM_NN, M, N, K)
  tiles = hip.gemm_row_tiles(M)
  z, st = _win(M, N, N + 3), _win(tiles, 3 * N)
  hip.gemm(kernels.GEMM_NN, bc.aligned_f32(a, DEV), bc.aligned_f32(b, DEV), out=z.out, bias=e.bias.to(DEV), bf16=True,
           col_stats=st.out)
  what = ('col_stats', M, N, K)
  got = z.read(what)
  assert torch.equal(got, e.expected(bias=True)), what
  bc.check_col_stats(st.read(what), got, what)


# ---------------------------------------------------------------------------------------------- er_cast_bf16
@pytest.mark.parametrize('rows,cols', bc.CAST_SHAPES)
@pytest.mark.parametrize('aligned', [True, False])
def test_cast_zeroes_the_padding_up_to_the_leading_dimension(hip, rows, cols, aligned):
  """plain and transposed from a column block of a wider fp32 buffer (16-byte aligned rows: the vector read path; one float
  off: the scalar one) into sentinel-filled destinations with ld_dst = pad8, pad8 + 8, pad8 + 40: the values are torch's
  round-to-nearest-even cast, EVERY padding column up to ld_dst is zero (include/easyrec_hip.h: they are read as the
  k-tail), nothing around the destination is touched."""
  src, x = bc.cast_source(rows, cols, aligned, DEV)
  want = x.to(BF)
  for ld_p, ld_t in zip(bc.cast_lds(cols), bc.cast_lds(rows)):
    plain, tr = _win(rows, ld_p, dtype=BF), _win(cols, ld_t, dtype=BF)
    hip.cast_bf16([(src, plain.out, False), (src, tr.out, True)])
    what = ('cast', rows, cols, aligned, ld_p, ld_t)
    p, t = plain.read(what), tr.read(what)
    assert torch.equal(p[:, :cols], want), what
    assert torch.equal(t[:, :rows], want.t()), what
    assert (p[:, cols:] == 0).all(), (what, 'plain: padding columns not zeroed', (p[:, cols:] != 0).nonzero()[:4].tolist())
    assert (t[:, rows:] == 0).all(), (what, 'transposed: padding columns not zeroed', (t[:, rows:] != 0).nonzero()[:4].tolist())


# ---------------------------------------------------------------------------------------------- refusals
def test_entry_point_refuses_what_the_kernel_cannot_take(hip):
  """host-side checks of er_gemm_bf16_nt[_epi], called directly where the wrapper would pad: each raises with the library's
  message, nothing is launched, and the device is fine afterwards"""
  a = torch.zeros(16, 64, dtype=BF, device=DEV)
  b = torch.zeros(16, 64, dtype=BF, device=DEV)
  c = torch.zeros(16, 64, device=DEV)
  cb = torch.zeros(16, 64, dtype=BF, device=DEV)
  stats = torch.zeros(16 * 3, device=DEV)

  def nt(M=16, N=16, K=32, A=a.data_ptr(), lda=64, Bt=b.data_ptr(), ldb=64, C=c.data_ptr(), ldc=64, Cb=None, ldcb=0,
         accumulate=0):
    hip._ck(hip.lib.er_gemm_bf16_nt(M, N, K, A, lda, Bt, ldb, C, ldc, Cb, ldcb, None, accumulate, _stream()), 'er_gemm_bf16_nt')

  nt()  # (the arguments the refusals below vary are fine)
  with pytest.raises(RuntimeError, match='multiples of 8'):
    nt(K=36)
  with pytest.raises(RuntimeError, match='multiples of 8'):
    nt(lda=60)
  with pytest.raises(RuntimeError, match='multiples of 8'):
    nt(ldb=68)
  with pytest.raises(RuntimeError, match='16-byte aligned'):
    nt(A=a.data_ptr() + 8)
  with pytest.raises(RuntimeError, match='16-byte aligned'):
    nt(Bt=b.data_ptr() + 8)
  with pytest.raises(RuntimeError, match='leading dimension of C too small'):
    nt(ldc=15)
  with pytest.raises(RuntimeError, match='leading dimension of C too small'):
    nt(Cb=cb.data_ptr(), ldcb=12)
  with pytest.raises(RuntimeError, match='accumulate needs the fp32 output'):
    nt(C=None, ldc=0, Cb=cb.data_ptr(), ldcb=64, accumulate=1)
  epi = _epi(kind=kernels.EPI_STATS, col_stats=stats)
  with pytest.raises(RuntimeError, match='an epilogue needs N'):
    hip._ck(hip.lib.er_gemm_bf16_nt_epi(16, 14, 32, _p(a), 64, _p(b), 64, _p(c), 64, None, 0, None, 0, ctypes.byref(epi),
                                        _stream()), 'er_gemm_bf16_nt_epi')
  torch.cuda.synchronize()
  assert torch.equal(c, torch.zeros_like(c)) and torch.equal(cb, torch.zeros_like(cb))
