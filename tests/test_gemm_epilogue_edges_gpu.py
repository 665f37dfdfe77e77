"""-m gpu: the store side of the fp32 GEMM block's epilogues (er_gemm_core.h) at tile edges.

The epilogues form a lane's 16 values first and then issue its stores back to back - without row predicates where the
workgroup's 64 rows all exist, under them in the last row tile.  What that can break is a store that is lost or that lands
outside [0, M) x [0, N).  Every case therefore writes into a window of a larger buffer that is filled with a sentinel -
in front of the output, behind it and, with ldc > N, between its rows - and checks that
  * every element of the window matches an fp64 matmul within the bound tests/test_kernels_gpu.py::test_gemm_f32 uses
    for the same entry point (1e-6 * sum |a||b| + 1e-6: an f32 fma chain; + 1e-5 with bias / accumulate, as there),
  * every guard element still holds the sentinel, exactly.
Shapes: M in {1, 63, 64, 65, 130}, N in {1, 31, 33, 64, 65, 96}, K in {1, 32, 40} (K = 1024 where a path needs k-splits):
pairs with an edge in M only, in N only, in both and in neither; more than one tile in either direction.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.kernels import _p, _stream  # noqa: E402

DEV = 'cuda:0'
SENT = -12345.5  # (exact in fp32; far from anything the seeded operands produce)
GUARD = 96       # sentinel floats in front of and behind the window

_NEITHER = [(64, 64, 32), (64, 64, 40)]
_M_ONLY = [(1, 64, 1), (63, 64, 32), (65, 64, 40), (130, 64, 32)]
_N_ONLY = [(64, 1, 32), (64, 31, 40), (64, 33, 1), (64, 65, 32), (64, 96, 40)]
_BOTH = [(1, 1, 1), (63, 31, 40), (65, 33, 32), (130, 65, 40), (130, 96, 1), (65, 96, 32)]
_SHAPES = _NEITHER + _M_ONLY + _N_ONLY + _BOTH
_LAYOUTS = [kernels.GEMM_NN, kernels.GEMM_NT, kernels.GEMM_TN]


@pytest.fixture(scope='module')
def hip():
  assert torch.cuda.is_available(), 'gpu tests need an MI355X'
  return kernels.hip()


class Window:
  """An [M, N] output with row stride ldc inside a sentinel-filled buffer."""

  def __init__(self, M, N, ldc, base=None):
    self.M, self.N, self.ldc = M, N, ldc
    self.buf = torch.full((GUARD + M * ldc + GUARD,), SENT, dtype=torch.float32, device=DEV)
    self.out = torch.as_strided(self.buf, (M, N), (ldc, 1), GUARD)
    if base is not None:
      self.out.copy_(base.to(DEV))

  def check(self, exp, bound, what):
    """exp, bound: fp64 [M, N] on the CPU"""
    torch.cuda.synchronize()
    buf = self.buf.cpu()
    got = torch.as_strided(buf, (self.M, self.N), (self.ldc, 1), GUARD)
    assert torch.isfinite(got).all(), what
    err = (got.double() - exp).abs()
    assert (err <= bound).all(), (what, float((err - bound).max()))
    guard = torch.ones(buf.numel(), dtype=torch.bool)
    torch.as_strided(guard, (self.M, self.N), (self.ldc, 1), GUARD).fill_(False)
    assert torch.equal(buf[guard], torch.full((int(guard.sum()),), SENT)), (what, 'a store landed outside the output')


def _operands(layout, M, N, K, seed):
  g = torch.Generator().manual_seed(seed)
  a = torch.randn((K, M) if layout == kernels.GEMM_TN else (M, K), generator=g)
  b = torch.randn((N, K) if layout == kernels.GEMM_NT else (K, N), generator=g)
  bias, base = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
  A = (a.t() if layout == kernels.GEMM_TN else a).double()
  Bm = (b.t() if layout == kernels.GEMM_NT else b).double()
  return a, b, bias, base, A @ Bm, (A.abs() @ Bm.abs()) * 1e-6


def _all_paths(hip, layout, M, N, K):
  """plain, + bias into ldc > N, accumulate (+ bias) into ldc > N: one entry point, the reference computed once"""
  a, b, bias, base, ref, bound = _operands(layout, M, N, K, M * 131 + N * 17 + K + layout)
  ad, bd = a.to(DEV), b.to(DEV)
  w = Window(M, N, N)
  hip.gemm(layout, ad, bd, out=w.out)
  w.check(ref, bound + 1e-6, 'plain')
  w = Window(M, N, N + 3)
  hip.gemm(layout, ad, bd, out=w.out, bias=bias.to(DEV))
  w.check(ref + bias.double(), bound + 1e-6 + 1e-6 * bias.double().abs(), 'bias, ldc > N')  # (one more rounding, of the sum)
  w = Window(M, N, N + 5, base=base)
  hip.gemm(layout, ad, bd, out=w.out, accumulate=True)
  w.check(base.double() + ref, bound + 1e-5, 'accumulate, ldc > N')
  w = Window(M, N, N, base=base)
  hip.gemm(layout, ad, bd, out=w.out, bias=bias.to(DEV), accumulate=True)
  w.check(base.double() + ref + bias.double(), bound + 1e-5, 'accumulate + bias')


@pytest.mark.parametrize('layout', _LAYOUTS)
@pytest.mark.parametrize('M,N,K', _SHAPES)
def test_stores_stay_inside_the_output(hip, layout, M, N, K):
  _all_paths(hip, layout, M, N, K)


@pytest.mark.parametrize('layout', _LAYOUTS)
@pytest.mark.parametrize('M,N', [(64, 64), (65, 64), (64, 33), (130, 96), (63, 31), (1, 1)])
def test_split_k_workspace_and_reduce_stay_inside_the_output(hip, layout, M, N):
  """K = 1024: er_gemm_f32 takes 8 k-splits for these outputs (choose_splits: <= 6 tiles, K >= 1024) - the block stores to
  the [splits][M][N] workspace, the reduce adds bias / the old values into the window."""
  _all_paths(hip, layout, M, N, 1024)


@pytest.mark.parametrize('M,N,K', [(64, 64, 32), (63, 64, 32), (64, 33, 1), (65, 33, 32), (130, 65, 40), (130, 96, 1), (1, 1, 1)])
def test_column_statistics_are_those_of_the_stored_output(hip, M, N, K):
  """col_stats: per row tile and column the Welford triple (count, mean, M2) of what the launch stored.  Merged over the
  row tiles in fp64 they are the column statistics of the stored z: counts exactly; mean within 1e-5 max|z| and M2 within
  1e-4 (M2 + max|z|^2) - sequential fp32 sums of <= 64 terms per tile (64 eps = 4e-6 relative to the largest term)."""
  a, b, bias, _, ref, bound = _operands(kernels.GEMM_NN, M, N, K, M + N + K)
  tiles = hip.gemm_row_tiles(M)
  assert tiles == (M + 63) // 64
  stats = torch.full((tiles * N * 3 + GUARD,), SENT, dtype=torch.float32, device=DEV)
  w = Window(M, N, N + 3)
  hip.gemm(kernels.GEMM_NN, a.to(DEV), b.to(DEV), out=w.out, bias=bias.to(DEV), col_stats=stats)
  w.check(ref + bias.double(), bound + 1e-5, 'col_stats')
  st = stats.cpu()
  assert torch.equal(st[tiles * N * 3:], torch.full((GUARD,), SENT))
  st = st[:tiles * N * 3].double().view(tiles, N, 3)
  z = w.out.cpu().double()
  n, mean_t, m2_t = st[..., 0], st[..., 1], st[..., 2]
  rows = torch.tensor([min(64, M - 64 * t) for t in range(tiles)], dtype=torch.float64)
  assert torch.equal(n, rows[:, None].expand(tiles, N))
  mean = (n * mean_t).sum(0) / M
  m2 = m2_t.sum(0) + (n * (mean_t - mean)**2).sum(0)
  zmax = float(z.abs().max())
  assert ((mean - z.mean(0)).abs() <= 1e-5 * zmax + 1e-7).all()
  m2_ref = ((z - z.mean(0))**2).sum(0)
  assert ((m2 - m2_ref).abs() <= 1e-4 * (m2_ref + zmax * zmax) + 1e-7).all()


def _bn_bwd_cols(hip, layout, a, b, out, src, partial, col0, n_src):
  """er_gemm_f32_bn_bwd_cols into a caller-owned output (HipBackend.gemm_bn_bwd allocates its own)"""
  (M, K), (N, _) = a.shape, b.shape
  hip._ck(hip.lib.er_gemm_f32_bn_bwd_cols(layout, M, N, K, _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0),
                                          _p(src.z), _p(src.zbias), _p(src.y), _p(src.mean), _p(src.invstd), src.y.stride(0),
                                          int(src.mean is not None), int(src.act), _p(partial), int(col0), n_src, _stream()),
          'er_gemm_f32_bn_bwd_cols')


@pytest.mark.parametrize('B,N,K,col0,n_src', [(65, 96, 32, 17, 64), (130, 65, 40, 33, 31), (64, 64, 32, 1, 33),
                                              (1, 33, 1, 3, 1), (63, 96, 40, 60, 36)])
@pytest.mark.parametrize('act', [kernels.ACT_RELU, kernels.ACT_NONE])
def test_batchnorm_backward_epilogue_with_a_column_block(hip, B, N, K, col0, n_src, act):
  """dy = dz_next . W^T (NT) with the BatchNorm-backward sums of the columns [col0, col0 + n_src): dy is the fp64 product
  within the GEMM bound with no store outside it (ldc > N); the partials, summed over the row tiles, are sum g and
  sum g * xhat of the block (g = dy masked by the activation) within 2e-5 * sum |terms| - fp32 sums of B <= 130 terms,
  130 eps = 8e-6 - and nothing is written behind them."""
  g = torch.Generator().manual_seed(B + N + K + col0 + act)
  z = torch.randn(B, n_src, generator=g).to(DEV)
  gamma, beta = (torch.rand(n_src, generator=g) + 0.5).to(DEV), (torch.randn(n_src, generator=g) * 0.1).to(DEV)
  mm, mv = torch.zeros(n_src, device=DEV), torch.ones(n_src, device=DEV)
  y, mean, invstd = hip.bn_act_fwd(z, None, gamma, beta, 1, 1e-3, 0.99, mm, mv, act)
  dz_next, wt = torch.randn(B, K, generator=g) * 0.1, torch.randn(N, K, generator=g)
  src = kernels.BnSource(z, None, y, mean, invstd, act)
  tiles = hip.gemm_row_tiles(B)
  partial = torch.full((tiles * n_src * 2 + GUARD,), SENT, dtype=torch.float32, device=DEV)
  w = Window(B, N, N + 3)
  _bn_bwd_cols(hip, kernels.GEMM_NT, dz_next.to(DEV), wt.to(DEV), w.out, src, partial, col0, n_src)
  ref = dz_next.double() @ wt.double().t()
  w.check(ref, (dz_next.double().abs() @ wt.double().abs().t()) * 1e-6 + 1e-6, 'bn_bwd dy')
  assert torch.equal(w.out, hip.gemm(kernels.GEMM_NT, dz_next.to(DEV), wt.to(DEV)))
  p = partial.cpu()
  assert torch.equal(p[tiles * n_src * 2:], torch.full((GUARD,), SENT))
  p = p[:tiles * n_src * 2].double().view(tiles, n_src, 2).sum(0)
  gm = w.out.cpu().double()[:, col0:col0 + n_src]
  if act == kernels.ACT_RELU:
    gm = gm * (y.cpu() > 0).double()
  xhat = (z.cpu().double() - mean.cpu().double()) * invstd.cpu().double()
  assert ((p[:, 0] - gm.sum(0)).abs() <= 2e-5 * gm.abs().sum(0) + 1e-7).all()
  assert ((p[:, 1] - (gm * xhat).sum(0)).abs() <= 2e-5 * (gm * xhat).abs().sum(0) + 1e-7).all()


@pytest.mark.parametrize('layout', [kernels.GEMM_TN, kernels.GEMM_NN])
def test_grouped_launch_mixing_full_and_edge_tiles(hip, layout):
  """One grouped launch whose problems are a single full tile, edge tiles in both directions, a multi-tile output and (TN)
  a k-split one: every window against fp64, every guard intact."""
  hip.gemm_reserve(1 << 22)
  shapes = [(64, 64, 40), (65, 33, 32), (130, 96, 40), (1, 1, 1), (63, 64, 32), (64, 31, 1)]
  if layout == kernels.GEMM_TN:
    shapes += [(65, 33, 4096), (64, 64, 4096)]
  probs, wins, exps = [], [], []
  for i, (M, N, K) in enumerate(shapes):
    a, b, bias, base, ref, bound = _operands(layout, M, N, K, 1000 + i)
    acc = i % 2 == 1
    w = Window(M, N, N + (i % 3), base=base if acc else None)
    probs.append((a.to(DEV), b.to(DEV), w.out, bias.to(DEV), acc))
    wins.append(w)
    exps.append(((base.double() if acc else 0) + ref + bias.double(), bound + 1e-5))
  hip.gemm_grouped(layout, probs)
  for i, (w, (exp, bound)) in enumerate(zip(wins, exps)):
    w.check(exp, bound, 'problem %d %r' % (i, shapes[i]))


def test_small_fused_tail_changes_no_bit():
  """The step's tail in two launches (the weight gradients through the block's split-K workspace path next to the embedding
  row update; the dense optimizer finishing them behind the cross-tile fix) against the four separate launches, on a small
  step: B = 192 (the weight gradients contract six k-tiles; no embedding tile is full), one table with a single row (the
  column-reduced path) next to tables of 40 rows (long runs of equal keys).  Four steps: every loss, table,
  slot and dense variable bit for bit, the way tests/test_deepfm_gpu.py::test_fused_step_variants_change_no_bit compares
  the full-size variants."""
  import os
  import numpy as np
  from easyrec_amd.input.criteo_synthetic import SyntheticCriteo
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  from easyrec_amd.utils import config_util
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(root, 'configs', 'deepfm_criteo_small.config'))
  hashed = [f for f in cfg.feature_config.features if f.HasField('hash_bucket_size') and f.hash_bucket_size > 0]
  for i, f in enumerate(hashed):
    f.hash_bucket_size = 1 if i == 0 else 40
  B = 192
  gen = SyntheticCriteo(cfg.data_config, list(cfg.feature_config.features), batch_size=B, seed=13)
  batches = [gen.next_batch() for _ in range(4)]
  be = kernels.hip()

  def run(tail, riders):
    be.defer_catch_up, be.prologue_tables, be.fused_tail, be.tail_riders = True, True, tail, riders
    be.tail_wgrad_blocks = 0  # (the stand-alone launch's k-splits: the same summation order over the batch in both)
    be.tail_launches = 0
    try:
      est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=4).build()
      losses = []
      for b in batches:
        est.train_step(b)
        losses.append(est.loss_values())
      assert est.engine._fused is True
      assert be.tail_launches == (len(batches) if tail else 0)
      return losses, est.state_dict(slots=True)
    finally:
      del be.defer_catch_up, be.prologue_tables, be.fused_tail, be.tail_wgrad_blocks, be.tail_riders

  base_l, base_s = run(False, False)
  for tail, riders in ((True, False), (True, True)):
    l, s = run(tail, riders)
    assert l == base_l, (tail, riders)
    assert set(s) == set(base_s)
    for k in s:
      assert np.array_equal(s[k], base_s[k]), (tail, riders, k)
