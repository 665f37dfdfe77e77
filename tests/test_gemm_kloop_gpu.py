"""-m gpu: the pipelined k loop of the fp32 GEMM block (er_gemm_core.h, the aligned path of gemm_f32_block) against the
block's own unaligned path, bit for bit.

The unaligned path - the `else` branch that loads with fetch_tile_generic, one k-tile at a time, no register sets, no
double-buffered LDS, two barriers per tile - contracts the same k order with the same MFMA into one accumulator.  It is
the bit reference for the pipelined loop, whose issue order is pinned by scheduling fences: what such a loop can get
wrong is a fragment read that overtakes the staging write of its tile, a staging write that overtakes the reads of the
tile before, a register set staged before its loads have arrived, or an edge tile whose masks were lost - each of them
changes bits.  Every case therefore calls HipBackend.gemm twice on the SAME values:
  * aligned: both operands with a 16-byte aligned base and a row pitch that is the row length rounded up to 4 floats (the
    padding holds NaN: a k-tile or row edge that is not masked poisons the output),
  * unaligned: the same values seen through views that start one float into their buffer and have a row pitch that is
    no multiple of 4 - which sends the launch down the generic path,
and requires the two outputs to be equal as bit patterns, each of them equal to itself on a second launch, each within
the bound the other fp32 GEMM tests hold against an fp64 matmul (tests/test_kernels_gpu.py::test_gemm_f32,
tests/test_gemm_epilogue_edges_gpu.py: 1e-6 * sum |a||b| + 1e-6 - an f32 fma chain; + 1e-5 with bias / accumulate - that
bound lives in those tests, tests/_bars.py holds only the trajectory bars), and every sentinel around the output intact.
The two paths agree bit for bit on the library this loop replaced as well (checked through EASYREC_AMD_LIB): the zero
k-tile with which the pipelined loop rounds an odd tile count up could only change an exact -0 sum, which seeded normal
operands do not produce.

Shapes, the smallest at which the pipeline can go wrong: K in {1, 31, 32, 33, 64, 65, 96, 97, 160} (one to five k-tiles:
prologue only, one loop trip with a zero tile, full pairs, ragged last tiles in the masked loop behind interior ones),
M in {1, 63, 64, 65, 129}, N in {1, 63, 64, 65, 84} (edge tiles, full tiles, more than one tile either way), NN / NT / TN,
plain, with bias, C +=, with column statistics (NN: the partial statistics compared too), and two k-splits over an odd
tile count per split (K = 1087 over 14 x 13 tiles: 17 k-tiles each, the second ragged).  The M x N x K grid launches at
most 6 workgroups and so takes the kernels with the pinned loop (er_gemm_core.h kPinnedMaxWorkgroups = 256: launch_gemm
chooses by tiles x splits), as does a split-K case of 6 tiles x 7 splits; the two-split case (364 workgroups) and a launch of
29 x 20 tiles take the kernels that leave the order to the compiler and are held to the same reference.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402

DEV = 'cuda:0'
SENT = -12345.5  # (exact in fp32; far from anything the seeded operands produce)
GUARD = 96       # sentinel floats in front of and behind the output window

_KS = [1, 31, 32, 33, 64, 65, 96, 97, 160]
_MS = [1, 63, 64, 65, 129]
_NS = [1, 63, 64, 65, 84]
_LAYOUTS = [kernels.GEMM_NN, kernels.GEMM_NT, kernels.GEMM_TN]


@pytest.fixture(scope='module')
def hip():
  assert torch.cuda.is_available(), 'gpu tests need an MI355X'
  return kernels.hip()


def _aligned(x):
  """x [R, C] (CPU) on the device with pitch = C rounded up to 4 and a 16-byte aligned base; the padding is NaN"""
  R, C = x.shape
  ld = (C + 3) // 4 * 4
  buf = torch.full((R, ld), float('nan'), dtype=torch.float32, device=DEV)
  buf[:, :C] = x.to(DEV)
  v = buf[:, :C]
  assert v.data_ptr() % 16 == 0 and v.stride(0) % 4 == 0
  return v


def _unaligned(x):
  """the same values one float into their buffer, pitch = C rounded up to 4, + 1: neither base nor pitch is aligned"""
  R, C = x.shape
  ld = (C + 3) // 4 * 4 + 1
  buf = torch.full((1 + R * ld,), float('nan'), dtype=torch.float32, device=DEV)
  v = torch.as_strided(buf, (R, C), (ld, 1), 1)
  v.copy_(x.to(DEV))
  assert v.data_ptr() % 16 != 0 and v.stride(0) % 4 != 0
  return v


class Window:
  """An [M, N] output with row stride ldc inside a sentinel-filled buffer."""

  def __init__(self, M, N, ldc, base=None):
    self.M, self.N, self.ldc = M, N, ldc
    self.buf = torch.full((GUARD + M * ldc + GUARD,), SENT, dtype=torch.float32, device=DEV)
    self.out = torch.as_strided(self.buf, (M, N), (ldc, 1), GUARD)
    if base is not None:
      self.out.copy_(base.to(DEV))

  def read(self, what):
    """-> the window's [M, N] on the CPU, after checking that every guard element still holds the sentinel"""
    torch.cuda.synchronize()
    buf = self.buf.cpu()
    guard = torch.ones(buf.numel(), dtype=torch.bool)
    torch.as_strided(guard, (self.M, self.N), (self.ldc, 1), GUARD).fill_(False)
    assert torch.equal(buf[guard], torch.full((int(guard.sum()),), SENT)), (what, 'a store landed outside the output')
    return torch.as_strided(buf, (self.M, self.N), (self.ldc, 1), GUARD).clone()


def _bits(t):
  return t.contiguous().view(torch.int32)


def _operands(layout, M, N, K, seed):
  g = torch.Generator().manual_seed(seed)
  a = torch.randn((K, M) if layout == kernels.GEMM_TN else (M, K), generator=g)
  b = torch.randn((N, K) if layout == kernels.GEMM_NT else (K, N), generator=g)
  bias, base = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
  A = (a.t() if layout == kernels.GEMM_TN else a).double()
  Bm = (b.t() if layout == kernels.GEMM_NT else b).double()
  return a, b, bias, base, A @ Bm, (A.abs() @ Bm.abs()) * 1e-6


def _both_paths(hip, layout, M, N, K, variants):
  """every variant on the aligned and on the unaligned views, twice each; variants: (name, ldc pad, bias?, accumulate?, stats?)"""
  a, b, bias, base, ref, bound = _operands(layout, M, N, K, M * 131 + N * 17 + K * 7 + layout)
  views = {'aligned': (_aligned(a), _aligned(b)), 'unaligned': (_unaligned(a), _unaligned(b))}
  bias_d = bias.to(DEV)
  tiles = hip.gemm_row_tiles(M)
  for name, pad, with_bias, acc, with_stats in variants:
    exp = ref + (bias.double() if with_bias else 0) + (base.double() if acc else 0)
    tol = bound + (1e-5 if (with_bias or acc) else 1e-6)
    got = {}
    for path, (av, bv) in views.items():
      for run in (0, 1):
        w = Window(M, N, N + pad, base=base if acc else None)
        stats = torch.full((tiles * N * 3 + GUARD,), SENT, dtype=torch.float32, device=DEV) if with_stats else None
        hip.gemm(layout, av, bv, out=w.out, bias=bias_d if with_bias else None, accumulate=acc, col_stats=stats)
        what = (name, path, run, layout, M, N, K)
        out = w.read(what)
        assert torch.isfinite(out).all(), what
        err = (out.double() - exp).abs()
        assert (err <= tol).all(), (what, float((err - tol).max()))
        res = [out]
        if with_stats:
          st = stats.cpu()
          assert torch.equal(st[tiles * N * 3:], torch.full((GUARD,), SENT)), what
          st = st[:tiles * N * 3].view(tiles, N, 3)
          rows = torch.tensor([min(64, M - 64 * t) for t in range(tiles)], dtype=torch.float32)
          assert torch.equal(st[..., 0], rows[:, None].expand(tiles, N)), what
          res.append(st)
        got[(path, run)] = res
    for i in range(len(got[('aligned', 0)])):
      first = _bits(got[('aligned', 0)][i])
      assert torch.equal(first, _bits(got[('aligned', 1)][i])), (name, 'the aligned path is not deterministic', layout, M, N, K, i)
      assert torch.equal(_bits(got[('unaligned', 0)][i]), _bits(got[('unaligned', 1)][i])), (name, 'the unaligned path is not deterministic', layout, M, N, K, i)
      diff = first != _bits(got[('unaligned', 0)][i])
      assert not diff.any(), (name, 'pipelined and generic k loop differ', layout, M, N, K, i, int(diff.sum()))


_PLAIN = [('plain', 0, False, False, False), ('bias, ldc > N', 3, True, False, False), ('C +=, ldc > N', 5, False, True, False),
          ('C += with bias', 0, True, True, False)]


@pytest.mark.parametrize('layout', _LAYOUTS)
@pytest.mark.parametrize('K', _KS)
def test_pipelined_k_loop_matches_the_generic_one_bit_for_bit(hip, layout, K):
  """plain / bias / C += / C += with bias over every M x N of the module's list"""
  for M in _MS:
    for N in _NS:
      _both_paths(hip, layout, M, N, K, _PLAIN)


@pytest.mark.parametrize('K', _KS)
def test_column_statistics_match_bit_for_bit(hip, K):
  """col_stats (NN, bias, ldc > N): the stored z and the per-row-tile Welford triples of both paths, bit for bit; the counts
  are the tiles' row counts exactly"""
  for M in _MS:
    for N in _NS:
      _both_paths(hip, kernels.GEMM_NN, M, N, K, [('col_stats', 3, True, False, True)])


@pytest.mark.parametrize('layout', _LAYOUTS)
def test_two_k_splits_over_an_odd_tile_count(hip, layout):
  """M x N = 895 x 831 is 14 x 13 = 182 tiles: er_gemm_f32's choose_splits takes 512 / 182 = 2 splits for K >= 1024, and
  K = 1087 gives each 544 = 17 x 32 (the second 543: ragged) - an odd k-tile count per split, through the split-K
  workspace and its reduce (plain and C += with bias).  2 x 182 workgroups: the compiler-ordered loop."""
  hip.gemm_reserve(2 * 895 * 831)
  _both_paths(hip, layout, 895, 831, 1087, [_PLAIN[0], _PLAIN[3]])


@pytest.mark.parametrize('layout', _LAYOUTS)
def test_large_launches_keep_the_compiler_ordered_loop(hip, layout):
  """M x N = 1793 x 1217 is 29 x 20 = 580 tiles, more than kPinnedMaxWorkgroups = 256: launch_gemm takes the kernels whose k
  loop the compiler orders; K = 97 is four k-tiles with a ragged last one (plain and C += with bias)."""
  _both_paths(hip, layout, 1793, 1217, 97, [_PLAIN[0], _PLAIN[3]])


@pytest.mark.parametrize('layout', _LAYOUTS)
def test_k_splits_in_the_pinned_loop(hip, layout):
  """M x N = 129 x 84 is 6 tiles: choose_splits is bounded by K / 128 = 8 for K = 1087, k_per_split = 160 = 5 k-tiles (odd),
  7 splits, the last of 127 columns (4 tiles, ragged): 42 workgroups, the pinned loop, through the split-K workspace and
  its reduce (plain and C += with bias)."""
  hip.gemm_reserve(8 * 129 * 84)
  _both_paths(hip, layout, 129, 84, 1087, [_PLAIN[0], _PLAIN[3]])
