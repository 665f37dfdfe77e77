"""-m gpu: the two reducing epilogues of the fp32 GEMM block (er_gemm_core.h: tile_col_stats, tile_bn_bwd_partial) against
a CPU replica of their documented fixed order, bit for bit.

Both reductions synchronise the workgroup in front of the block's plain stores, so a lane whose column lies outside N, and
a row tile with missing rows, must walk through both barriers and skip only their stores.  A full row tile takes the
reductions without row predicates and with the constant count 16, the last one with them; the epilogue's operands (y, z)
are requested behind the first two k-tiles' loads.  What such code can get wrong is a store outside the output, a sum that
takes a row that does not exist or drops one that does, an epilogue operand used before it arrived - each changes bits or
a sentinel - or a skipped barrier, which hangs.

Reference: numpy float32, one correctly rounded operation at a time (the library is built with -ffp-contract=off and its
divisions are IEEE divisions), in the order the code documents.
  column statistics of a 64-row tile (value = the stored z = acc + bias), per column:
    a lane's 16 rows in register order, row = 64 t + 32 wm + 4 khalf + (r & 3) + 8 (r >> 2), r = 0 .. 15: n counts the rows
    < M, s their sum, mean = s / n (0 if none), m2 = sum (z - mean)^2 in the same order; chan_merge of the lane pair (khalf
    0 first); chan_merge of the two waves (wm 0 first).  The count is the tile's row count exactly.
  BatchNorm-backward partials (sum g, sum g * xhat) of a 64-row tile, per source column:
    the same 16 rows in register order, g = dy, set to 0 where the activation is ReLU and not y > 0, sg = sg + g,
    sgx = sgx + g * (((z + zbias) - mean) * invstd) (0 without BatchNorm); the lane pair summed, khalf 0 first; then
    wm 0 + wm 1.  dy itself must equal hip.gemm's output bit for bit.
Every output and partial buffer lies inside sentinels (in front, behind, and between the rows where it has a pitch), and a
second launch must give the same bits.

Shapes: M in {1, 31, 33, 64, 65, 129} x N in {1, 63, 64, 65, 84, 128} x K in {32, 97} - lanes with col >= N, tiles with
missing rows, full tiles, more than one tile either way, one and four k-tiles; at most 3 x 2 workgroups, the kernels with
the pinned k loop.  One shape of 18 x 16 = 288 workgroups (more than kPinnedMaxWorkgroups = 256) takes the instantiations
that leave the loop to the compiler through the same epilogue.  The column block (col0 > 0, n_src < N) needs N >= 3.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.kernels import _p, _stream  # noqa: E402

DEV = 'cuda:0'
SENT = -12345.5  # (exact in fp32; far from anything the seeded operands produce)
GUARD = 96
F = np.float32

_MS = [1, 31, 33, 64, 65, 129]
_NS = [1, 63, 64, 65, 84, 128]
_KS = [32, 97]
_BIG = (64 * 17 + 1, 64 * 15 + 20, 32)  # 18 x 16 tiles


@pytest.fixture(scope='module')
def hip():
  assert torch.cuda.is_available(), 'gpu tests need an MI355X'
  return kernels.hip()


class Window:
  """[R, C] with row pitch ld inside a sentinel-filled buffer: sentinels in front, behind and between the rows."""

  def __init__(self, R, C, ld):
    self.R, self.C, self.ld = R, C, ld
    self.buf = torch.full((GUARD + R * ld + GUARD,), SENT, dtype=torch.float32, device=DEV)
    self.view = torch.as_strided(self.buf, (R, C), (ld, 1), GUARD)

  def read(self, what):
    torch.cuda.synchronize()
    buf = self.buf.cpu()
    guard = torch.ones(buf.numel(), dtype=torch.bool)
    torch.as_strided(guard, (self.R, self.C), (self.ld, 1), GUARD).fill_(False)
    assert torch.equal(buf[guard], torch.full((int(guard.sum()),), SENT)), (what, 'a store landed outside the buffer')
    return torch.as_strided(buf, (self.R, self.C), (self.ld, 1), GUARD).clone().numpy()


def _padded(x, pad=4):
  """x [R, C] (CPU) on the device with an aligned base, pitch = C rounded up to 4, + pad; the padding is NaN"""
  R, C = x.shape
  ld = (C + 3) // 4 * 4 + pad
  buf = torch.full((R, ld), float('nan'), dtype=torch.float32, device=DEV)
  buf[:, :C] = x.to(DEV)
  return buf[:, :C]


def _bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _lane_rows(t, wm, khalf):
  return [64 * t + 32 * wm + 4 * khalf + (r & 3) + 8 * (r >> 2) for r in range(16)]


def _chan_merge(a, b):
  """chan_merge(n, mean, m2; nb, mb, m2b) of er_gemm_core.h, elementwise over the columns"""
  (n, mean, m2), (nb, mb, m2b) = a, b
  with np.errstate(invalid='ignore', divide='ignore'):
    tot = n + nb
    delta = mb - mean
    mean_m = mean + delta * (nb / tot)
    m2_m = (m2 + m2b) + (delta * delta) * ((n * nb) / tot)
  keep, take = nb == 0, n == 0  # (b empty: a as it is; else a empty: b)
  pick = lambda x, y, z: np.where(keep, x, np.where(take, y, z)).astype(F)  # noqa: E731
  return pick(n, nb, tot), pick(mean, mb, mean_m), pick(m2, m2b, m2_m)


def _replica_col_stats(z, tiles):
  """z [M, N] float32 -> [tiles, N, 3]"""
  M, N = z.shape
  out = np.zeros((tiles, N, 3), F)
  for t in range(tiles):
    waves = []
    for wm in (0, 1):
      halves = []
      for khalf in (0, 1):
        rows = [r for r in _lane_rows(t, wm, khalf) if r < M]
        n, s = np.zeros(N, F), np.zeros(N, F)
        for r in rows:
          n, s = n + F(1), s + z[r]
        with np.errstate(invalid='ignore', divide='ignore'):
          mean = np.where(n > 0, s / n, F(0)).astype(F)
        m2 = np.zeros(N, F)
        for r in rows:
          d = z[r] - mean
          m2 = m2 + d * d
        halves.append((n, mean, m2))
      waves.append(_chan_merge(halves[0], halves[1]))
    n, mean, m2 = _chan_merge(waves[0], waves[1])
    out[t, :, 0], out[t, :, 1], out[t, :, 2] = n, mean, m2
  return out


def _replica_bn_partial(dy, y, z, zbias, mean, invstd, relu, tiles):
  """dy / y / z [M, n_src] float32 (the source columns) -> [tiles, n_src, 2]"""
  M, n = dy.shape
  use_bn = mean is not None
  bv = zbias if zbias is not None else np.zeros(n, F)
  out = np.zeros((tiles, n, 2), F)
  for t in range(tiles):
    waves = []
    for wm in (0, 1):
      halves = []
      for khalf in (0, 1):
        sg, sgx = np.zeros(n, F), np.zeros(n, F)
        for r in _lane_rows(t, wm, khalf):
          if r >= M:
            continue
          g = dy[r]
          if relu:
            g = np.where(y[r] > 0, g, F(0)).astype(F)
          sg = sg + g
          if use_bn:
            sgx = sgx + g * (((z[r] + bv) - mean) * invstd)
        halves.append((sg, sgx))
      waves.append((halves[0][0] + halves[1][0], halves[0][1] + halves[1][1]))
    out[t, :, 0] = waves[0][0] + waves[1][0]
    out[t, :, 1] = waves[0][1] + waves[1][1]
  return out


# ---------------------------------------------------------------------------------------------------------------------
# forward: hip.gemm(GEMM_NN, ..., bias, col_stats), ldc > N
# ---------------------------------------------------------------------------------------------------------------------
def _col_stats_case(hip, M, N, K):
  g = torch.Generator().manual_seed(M * 131 + N * 17 + K * 7)
  a, b, bias = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), torch.randn(N, generator=g)
  av, bv, bias_d = _padded(a, 0), _padded(b, 0), bias.to(DEV)
  tiles = hip.gemm_row_tiles(M)
  assert tiles == (M + 63) // 64
  got = []
  for run in (0, 1):
    what = ('col_stats', M, N, K, run)
    w = Window(M, N, N + 3)
    st = Window(1, tiles * N * 3, tiles * N * 3)
    hip.gemm(kernels.GEMM_NN, av, bv, out=w.view, bias=bias_d, col_stats=st.view.view(-1))
    z, s = w.read(what), st.read(what).reshape(tiles, N, 3)
    assert np.isfinite(z).all() and np.isfinite(s).all(), what
    got.append((z, s))
  z, s = got[0]
  assert np.array_equal(_bits(z), _bits(got[1][0])) and np.array_equal(_bits(s), _bits(got[1][1])), ('not deterministic', M, N, K)
  # the k loop has its own test (tests/test_gemm_kloop_gpu.py); here only that z is the contraction at all
  ref = a.double() @ b.double() + bias.double()
  assert np.abs(z - ref.numpy()).max() <= 1e-4 * max(1.0, float(ref.abs().max())), (M, N, K)
  rows = np.array([min(64, M - 64 * t) for t in range(tiles)], F)
  assert np.array_equal(s[..., 0], np.broadcast_to(rows[:, None], (tiles, N))), ('counts', M, N, K)
  exp = _replica_col_stats(z, tiles)
  diff = _bits(s) != _bits(exp)
  assert not diff.any(), ('column statistics differ from the replica', M, N, K, int(diff.sum()), s[diff][:4], exp[diff][:4])


@pytest.mark.parametrize('K', _KS)
def test_column_statistics_match_the_replica_bit_for_bit(hip, K):
  for M in _MS:
    for N in _NS:
      _col_stats_case(hip, M, N, K)


def test_column_statistics_in_the_compiler_ordered_kernels(hip):
  _col_stats_case(hip, *_BIG)


# ---------------------------------------------------------------------------------------------------------------------
# backward: hip.gemm_bn_bwd(GEMM_NT, ...) - dy = dz_next . W_next^T with the producing layer's BatchNorm-backward sums
# ---------------------------------------------------------------------------------------------------------------------
def _bn_bwd_case(hip, M, N, K, relu, use_bn, block):
  """block: the producing layer made the columns [col0, col0 + n_src) of dy only (col0 > 0, n_src < N)"""
  col0, n_src = (max(1, N // 4), N - max(1, N // 4) - 1) if block else (0, N)
  g = torch.Generator().manual_seed(M * 131 + N * 17 + K * 7 + 3 * relu + 5 * use_bn + 11 * block)
  a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
  z = torch.randn(M, n_src, generator=g)
  y = torch.randn(M, n_src, generator=g)  # (its sign decides the ReLU mask; about half of them are not > 0)
  y[torch.rand(M, n_src, generator=g) < 0.1] = 0.0
  zbias = torch.randn(n_src, generator=g)
  mean = torch.randn(n_src, generator=g) if use_bn else None
  invstd = (torch.rand(n_src, generator=g) + 0.5) if use_bn else None
  av, wv = _padded(a, 0), _padded(w, 0)
  zy = torch.full((2, M, (n_src + 3) // 4 * 4 + 4), float('nan'), dtype=torch.float32, device=DEV)  # (one pitch for both)
  zv, yv = zy[0, :, :n_src], zy[1, :, :n_src]
  zv.copy_(z.to(DEV))
  yv.copy_(y.to(DEV))
  dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
  src = kernels.BnSource(zv, dev(zbias), yv, dev(mean), dev(invstd), kernels.ACT_RELU if relu else kernels.ACT_NONE)
  tiles = hip.gemm_row_tiles(M)
  plain = hip.gemm(kernels.GEMM_NT, av, wv).cpu().numpy()
  got = []
  for run in (0, 1):
    what = ('bn_bwd', M, N, K, relu, use_bn, block, run)
    part = Window(1, tiles * n_src * 2, tiles * n_src * 2)
    dy = hip.gemm_bn_bwd(kernels.GEMM_NT, av, wv, src, part.view.view(-1), col0=col0 if block else None)
    p = part.read(what).reshape(tiles, n_src, 2)
    dy = dy.cpu().numpy()
    # the same C entry point with dy inside sentinels (ldc > N): gemm_bn_bwd allocates a dense dy itself
    part2, win = Window(1, tiles * n_src * 2, tiles * n_src * 2), Window(M, N, N + 5)
    args = (kernels.GEMM_NT, M, N, K, _p(av), av.stride(0), _p(wv), wv.stride(0), _p(win.view), win.view.stride(0), _p(src.z),
            _p(src.zbias), _p(src.y), _p(src.mean), _p(src.invstd), src.y.stride(0), int(use_bn), int(src.act), _p(part2.view))
    if block:
      hip.ck.er_gemm_f32_bn_bwd_cols(*args, int(col0), int(n_src), _stream())
    else:
      hip.ck.er_gemm_f32_bn_bwd(*args, _stream())
    dy2, p2 = win.read(what), part2.read(what).reshape(tiles, n_src, 2)
    assert np.array_equal(_bits(dy), _bits(dy2)) and np.array_equal(_bits(p), _bits(p2)), (what, 'ldc changes the result')
    got.append((dy, p))
  dy, p = got[0]
  assert np.array_equal(_bits(dy), _bits(got[1][0])) and np.array_equal(_bits(p), _bits(got[1][1])), ('not deterministic', what)
  assert np.isfinite(dy).all() and np.isfinite(p).all(), what
  diff = _bits(dy) != _bits(plain)
  assert not diff.any(), ('dy differs from hip.gemm', what, int(diff.sum()))
  np_ = lambda t: None if t is None else t.numpy()  # noqa: E731
  exp = _replica_bn_partial(np.ascontiguousarray(dy[:, col0:col0 + n_src]), y.numpy(), z.numpy(), np_(zbias), np_(mean),
                            np_(invstd), relu, tiles)
  diff = _bits(p) != _bits(exp)
  assert not diff.any(), ('BatchNorm-backward partials differ from the replica', what, int(diff.sum()), p[diff][:4], exp[diff][:4])


@pytest.mark.parametrize('K', _KS)
@pytest.mark.parametrize('use_bn', [True, False])
@pytest.mark.parametrize('relu', [True, False])
def test_bn_backward_partials_match_the_replica_bit_for_bit(hip, relu, use_bn, K):
  for M in _MS:
    for N in _NS:
      _bn_bwd_case(hip, M, N, K, relu, use_bn, False)
      if N >= 3:
        _bn_bwd_case(hip, M, N, K, relu, use_bn, True)


@pytest.mark.parametrize('block', [False, True])
def test_bn_backward_partials_in_the_compiler_ordered_kernels(hip, block):
  _bn_bwd_case(hip, *_BIG, True, True, block)
