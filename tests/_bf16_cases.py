"""Cases, operands and expected values for the bf16 contractions (csrc/er_gemm_bf16.hip: er_gemm_bf16_nt[_epi] and
er_cast_bf16; csrc/er_gemm.hip: er_gemm_bf16).  No backend is imported here: tests/test_bf16_cases.py (CPU) checks what this
module claims about its own cases, tests/test_gemm_bf16_ring_gpu.py launches the kernels and compares.

Exact operands.  A and B are integers drawn uniformly from [-8, 8], bias and base integers from [-64, 64].  Every such value
is a bfloat16 (8 significant bits hold |v| <= 256), every product an integer of magnitude <= 64, and with K <= 1088 every
partial sum of products, in any order and under any split of k, plus bias and base stays below 64 * 1088 + 128 < 2**24: it
is an integer that float32 holds exactly, so no summation order, k-split or epilogue order can round.  The expected output
is the int64 matmul (+ bias + base) and the comparison is equality: a dropped, duplicated, stale or mis-swizzled 16-byte
k-chunk moves the result by whole integers.

Random operands.  randn rounded to bfloat16 (torch's round-to-nearest-even cast); the reference is the float64 product of
the rounded operands, whose products float32 holds exactly, so a kernel differs from it by its float32 summation only.
The bounds are the ones the project already holds these entry points to:
  er_gemm_bf16_nt: 2e-5 * sum |a||b| + 1e-6   (tests/test_kernels_gpu.py::test_gemm_bf16_nt)
  er_gemm_bf16:    2e-6 * sum |a||b| + 1e-6   (tests/test_kernels_gpu.py::test_gemm_bf16)

Poisoned padding.  bf16 operands live in buffers whose row pitch is K + 72 (a multiple of 8 as K is; 72 > one k-tile, so
a k-tile that is read whole stays inside the row's own allocation); the columns [K, pitch) hold NaN.  A k-tail chunk that
the kernel does not mask makes the output NaN.  fp32 operands (er_gemm_bf16) use aligned / unaligned views with NaN in
the pitch, as tests/test_gemm_kloop_gpu.py does.

Windows.  Every tensor a launch writes is an [R, C] window with row pitch ld inside a buffer filled with a sentinel: GUARD
elements in front, GUARD behind, ld - C between the rows.  -12345.5 for float32 and -12288 for bfloat16 (= -1.5 * 2**13,
exact in bfloat16).  Only guard elements are compared with the sentinel, so an output that happens to equal it is fine.

Shapes (k-tile 64, ring of 4 tile pairs, three tiles issued by the prologue; T = ceil(K / 64)):
  K: 8, 56 (one ragged tile: tiles 1..3 all zero-source), 64 (one full tile), 72, 128, 136, 192, 200 (tile counts at and
     below the prologue's three issues, with and without the narrowest ragged tail the entry point admits, + 8), 256 (ring
     exactly full, the first in-loop issue a zero tile), 264 (the first real tile DMA'd over a buffer that was read), 320,
     328, 384, 448 (the wrap continues: five, six and seven tiles), 512, 520, 584 (two turns of the ring).
  M: 1, 64, 65, 128, 129, 257 (row clamp to M - 1, a half-empty wave row block, exact tiles, three row tiles).
  N: 1, 4, 63, 64, 68, 128, 129, 132 (N % 4 != 0: scalar stores; N % 4 == 0: 16-byte stores; 4 clamps the cross pre-load
     column; 129, 132: two column tiles with a narrow last one).
  Output pitch: N, N + 3 (scalar stores even when N % 4 == 0), round4(N) + 4 (16-byte stores with gaps between rows).
"""
import torch

U = 2.0 ** -24

KS = [8, 56, 64, 72, 128, 136, 192, 200, 256, 264, 320, 328, 384, 448, 512, 520, 584]
MS = [1, 64, 65, 128, 129, 257]
NS = [1, 4, 63, 64, 68, 128, 129, 132]
RANDOM_MN = [(1, 1), (65, 68), (129, 129), (257, 132)]
M_MAX, N_MAX = max(MS), max(NS)
K_EXACT_MAX = 1088  # 64 * 1088 + 128 < 2**24

EPI_BS = [1, 63, 65, 129]
CROSS_DS = [8, 72, 136, 264]        # square d = N = K of the cross epilogues
EPI_NK = [(4, 8), (64, 72), (68, 264), (132, 136)]  # STATS and BN_BWD

# er_gemm_bf16 (fp32 operands rounded while staged): tests/test_gemm_epilogue_edges_gpu.py's _SHAPES, + two that take k-splits
GEMM_SHAPES = [(64, 64, 32), (64, 64, 40),
               (1, 64, 1), (63, 64, 32), (65, 64, 40), (130, 64, 32),
               (64, 1, 32), (64, 31, 40), (64, 33, 1), (64, 65, 32), (64, 96, 40),
               (1, 1, 1), (63, 31, 40), (65, 33, 32), (130, 65, 40), (130, 96, 1), (65, 96, 32),
               (65, 33, 1088), (130, 96, 1088)]
GEMM_STATS_SHAPES = [(63, 64, 32), (65, 33, 32), (130, 65, 40)]
GEMM_NN, GEMM_NT, GEMM_TN = 0, 1, 2  # (include/easyrec_hip.h; tests/test_bf16_cases.py compares them with kernels')

CAST_SHAPES = [(1, 1), (7, 3), (33, 65), (130, 70)]
CAST_LD_EXTRA = [0, 8, 40]  # ld_dst = pad8(width) + one of these

NT_REL, GEMM_REL, ABS = 2e-5, 2e-6, 1e-6

PAD = 72
GUARD = 96
SENT = {torch.float32: -12345.5, torch.bfloat16: -12288.0}


def round4(n):
  return (n + 3) // 4 * 4


def pad8(n):
  return (n + 7) // 8 * 8


def pitches(N):
  """the three output pitches of the module's list"""
  return N, N + 3, round4(N) + 4


def bn_blocks(N):
  """column blocks (col0, n_src) of the BatchNorm-backward epilogue: all columns, (4, 8), one that ends at N"""
  blocks = [(0, N)]
  if N >= 16:
    blocks += [(4, 8), (N - 8, 8)]
  return blocks


# ---------------------------------------------------------------------------------------------- exact operands
class Exact(object):
  """integer operands a [M, K], b [N, K] (fp32 tensors), bias [N], base [M, N] and the int64 results"""

  def __init__(self, M, N, K, seed):
    assert K <= K_EXACT_MAX
    g = torch.Generator().manual_seed(seed)
    self.M, self.N, self.K = M, N, K
    self.a_int = torch.randint(-8, 9, (M, K), generator=g, dtype=torch.int64)
    self.b_int = torch.randint(-8, 9, (N, K), generator=g, dtype=torch.int64)
    self.bias_int = torch.randint(-64, 65, (N,), generator=g, dtype=torch.int64)
    self.base_int = torch.randint(-64, 65, (M, N), generator=g, dtype=torch.int64)
    self.prod_int = self.a_int @ self.b_int.t()
    self.a, self.b = self.a_int.float(), self.b_int.float()
    self.bias, self.base = self.bias_int.float(), self.base_int.float()

  def magnitude(self):
    """max over the outputs of sum |a||b| + |bias| + |base|: what must stay below 2**24"""
    return int((self.a_int.abs() @ self.b_int.abs().t() + self.bias_int.abs() + self.base_int.abs()).max())

  def expected(self, M=None, N=None, bias=False, base=False):
    """fp32 [M, N] (the leading rows of a and b): a . b^T (+ bias) (+ base), exact"""
    M, N = M or self.M, N or self.N
    e = self.prod_int[:M, :N]
    if bias:
      e = e + self.bias_int[:N]
    if base:
      e = e + self.base_int[:M, :N]
    assert int(e.abs().max()) < 2 ** 24
    return e.float()


def exact_for_k(K):
  """one operand set per K: every (M, N) of the lists takes its leading rows"""
  return Exact(M_MAX, N_MAX, K, 1000 + K)


def exact_gemm(layout, M, N, K):
  """-> (Exact, a, b): a, b fp32 in the layout er_gemm_bf16 takes (NN: a[M,K] b[K,N]; NT: a[M,K] b[N,K]; TN: a[K,M] b[K,N])"""
  e = Exact(M, N, K, M * 131 + N * 17 + K + layout)
  a = e.a.t().contiguous() if layout == GEMM_TN else e.a
  b = e.b if layout == GEMM_NT else e.b.t().contiguous()
  return e, a, b


# ---------------------------------------------------------------------------------------------- random operands
class Random(object):
  """randn operands rounded to bfloat16 (held as fp32), the fp64 product of the rounded operands and sum |a||b|"""

  def __init__(self, M, N, K, seed, scale_b=1.0):
    g = torch.Generator().manual_seed(seed)
    self.M, self.N, self.K = M, N, K
    self.a_raw = torch.randn(M, K, generator=g)
    self.b_raw = torch.randn(N, K, generator=g) * scale_b
    self.a = self.a_raw.to(torch.bfloat16).float()
    self.b = self.b_raw.to(torch.bfloat16).float()
    self.ref = self.a.double() @ self.b.double().t()
    self.scale = self.a.double().abs() @ self.b.double().abs().t()

  def bound(self, rel):
    return rel * self.scale + ABS


def random_for_k(K):
  return Random(M_MAX, N_MAX, K, 2000 + K)


def random_gemm(layout, M, N, K):
  """-> (Random, a, b): the UNROUNDED fp32 operands in er_gemm_bf16's layout (the kernel rounds them while staging)"""
  r = Random(M, N, K, M * 131 + N * 17 + K * 7 + layout)
  a = r.a_raw.t().contiguous() if layout == GEMM_TN else r.a_raw
  b = r.b_raw if layout == GEMM_NT else r.b_raw.t().contiguous()
  return r, a, b


# ---------------------------------------------------------------------------------------------- operand buffers
def poisoned_bf16(x, device='cpu'):
  """x [R, K] fp32 holding bfloat16 values -> a bf16 tensor [R, K + PAD] whose columns [K, K + PAD) are NaN; rows are
  16-byte aligned (K % 8 == 0).  The kernels take it with K and its row pitch."""
  R, K = x.shape
  assert K % 8 == 0
  xb = x.to(torch.bfloat16)
  assert torch.equal(xb.float(), x), 'the operand is not a bfloat16 value'
  buf = torch.full((R, K + PAD), float('nan'), dtype=torch.bfloat16, device=device)
  buf[:, :K] = xb.to(device)
  assert buf.data_ptr() % 16 == 0 and buf.stride(0) % 8 == 0
  return buf


def aligned_f32(x, device='cpu'):
  """x [R, C] with pitch = C rounded up to 4 and a 16-byte aligned base; the padding is NaN"""
  R, C = x.shape
  buf = torch.full((R, round4(C)), float('nan'), dtype=torch.float32, device=device)
  buf[:, :C] = x.to(device)
  v = buf[:, :C]
  assert v.data_ptr() % 16 == 0 and v.stride(0) % 4 == 0
  return v


def unaligned_f32(x, device='cpu'):
  """the same values one float into their buffer, pitch = C rounded up to 4, + 1: neither base nor pitch is aligned"""
  R, C = x.shape
  ld = round4(C) + 1
  buf = torch.full((1 + R * ld,), float('nan'), dtype=torch.float32, device=device)
  v = torch.as_strided(buf, (R, C), (ld, 1), 1)
  v.copy_(x.to(device))
  assert v.data_ptr() % 16 != 0 and v.stride(0) % 4 != 0
  return v


def padded_rows_f32(x, device='cpu'):
  """x [R, C] (C % 4 == 0) as an epilogue input: 16-byte aligned rows with pitch C + 4, the padding NaN"""
  R, C = x.shape
  assert C % 4 == 0
  buf = torch.full((R, C + 4), float('nan'), dtype=torch.float32, device=device)
  buf[:, :C] = x.to(device)
  return buf[:, :C]


class Window(object):
  """An [R, C] output with row pitch ld inside a sentinel-filled buffer (GUARD elements in front and behind)."""

  def __init__(self, R, C, ld=None, dtype=torch.float32, device='cpu', base=None):
    ld = C if ld is None else ld
    assert ld >= C
    self.R, self.C, self.ld, self.dtype = R, C, ld, dtype
    self.sent = SENT[dtype]
    self.buf = torch.full((GUARD + R * ld + GUARD,), self.sent, dtype=dtype, device=device)
    self.out = torch.as_strided(self.buf, (R, C), (ld, 1), GUARD)
    if base is not None:
      self.out.copy_(base.to(device))

  def guard_mask(self):
    g = torch.ones(self.buf.numel(), dtype=torch.bool)
    torch.as_strided(g, (self.R, self.C), (self.ld, 1), GUARD).fill_(False)
    return g

  def read(self, what):
    """-> the window's [R, C] on the CPU, after checking that every guard element still holds the sentinel (the caller
    synchronizes: .cpu() on the launch's stream does)"""
    buf = self.buf.cpu()
    g = self.guard_mask()
    assert torch.equal(buf[g], torch.full((int(g.sum()),), self.sent, dtype=self.dtype)), (what, 'a store landed outside the output')
    return torch.as_strided(buf, (self.R, self.C), (self.ld, 1), GUARD).clone()


def bits(t):
  return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------- epilogue references
def row_tiles(M):
  return (M + 63) // 64


def check_col_stats(st, z, what):
  """st [tiles, N, 3] (count, mean, M2 per 64-row tile and column) against the stored z [M, N]: counts exactly; merged over
  the tiles in fp64, mean within 1e-5 max|z| + 1e-7 and M2 within 1e-4 (M2 + max|z|^2) + 1e-7 - the bounds of
  tests/test_gemm_epilogue_edges_gpu.py::test_column_statistics_are_those_of_the_stored_output"""
  M, N = z.shape
  tiles = row_tiles(M)
  st, z = st.double().view(tiles, N, 3), z.double()
  n, mean_t, m2_t = st[..., 0], st[..., 1], st[..., 2]
  rows = torch.tensor([min(64, M - 64 * t) for t in range(tiles)], dtype=torch.float64)
  assert torch.equal(n, rows[:, None].expand(tiles, N)), what
  mean = (n * mean_t).sum(0) / M
  m2 = m2_t.sum(0) + (n * (mean_t - mean) ** 2).sum(0)
  zmax = float(z.abs().max())
  assert ((mean - z.mean(0)).abs() <= 1e-5 * zmax + 1e-7).all(), what
  m2_ref = ((z - z.mean(0)) ** 2).sum(0)
  assert ((m2 - m2_ref).abs() <= 1e-4 * (m2_ref + zmax * zmax) + 1e-7).all(), what


class BnSource(object):
  """the layer below a BatchNorm-backward epilogue: z [B, n] (+ zbias), batch statistics, y = act(xhat gamma + beta) in
  float32 - inputs of the epilogue (it reads y for the ReLU mask, mean / invstd as data)"""

  def __init__(self, B, n, use_bn, relu, seed):
    g = torch.Generator().manual_seed(seed)
    self.z = torch.randn(B, n, generator=g)
    self.zbias = torch.randn(n, generator=g) * 0.1 if use_bn else None
    gamma, beta = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.1
    zz = self.z + self.zbias if use_bn else self.z
    self.mean = zz.mean(0)
    self.invstd = 1.0 / torch.sqrt(zz.var(0, unbiased=False) + 1e-3)
    pre = (zz - self.mean) * self.invstd * gamma + beta if use_bn else zz
    self.y = torch.relu(pre) if relu else pre
    self.use_bn, self.relu = use_bn, relu

  def check_partial(self, partial, dy_block, what):
    """partial [tiles, n, 2] summed over the tiles = (sum g, sum g xhat), g = dy masked by the activation, within
    2e-5 * sum |terms| + 1e-7 (tests/test_gemm_epilogue_edges_gpu.py::test_batchnorm_backward_epilogue_with_a_column_block:
    fp32 sums of B <= 130 terms, 130 eps = 8e-6)"""
    p = partial.double().sum(0)
    gm = dy_block.double()
    if self.relu:
      gm = gm * (self.y > 0).double()
    assert ((p[:, 0] - gm.sum(0)).abs() <= 2e-5 * gm.abs().sum(0) + 1e-7).all(), what
    if self.use_bn:
      # (z + zbias is one float32 addition, correctly rounded in torch and in the kernel alike: the reference starts from
      # that float32 sum - with a single row z + zbias - mean is then exactly 0 on both sides, not the addition's rounding)
      xhat = ((self.z + self.zbias).double() - self.mean.double()) * self.invstd.double()
      assert ((p[:, 1] - (gm * xhat).sum(0)).abs() <= 2e-5 * (gm * xhat).abs().sum(0) + 1e-7).all(), what
    else:
      assert torch.equal(p[:, 1], torch.zeros_like(p[:, 1])), what


class CrossFwd(object):
  """x_{l+1} = x0 * (x . w + b + diag * x) + x with x and w^T as bf16 operands (tests/test_fused_epilogues_gpu.py::
  test_cross_forward_in_the_bf16_contraction): u against the fp64 product of the rounded operands at the NT bound; the
  output against the epilogue's own arithmetic in fp64 from the kernel's u, within 2e-6 max|ref|."""

  def __init__(self, B, d, seed):
    g = torch.Generator().manual_seed(seed)
    self.x0, self.x = torch.randn(B, d, generator=g), torch.randn(B, d, generator=g)
    self.w = torch.randn(d, d, generator=g) * 0.05
    self.b = torch.randn(d, generator=g)
    self.xr = self.x.to(torch.bfloat16).float()
    self.wtr = self.w.t().contiguous().to(torch.bfloat16).float()  # Bt [N, K]
    self.u_ref = self.xr.double() @ self.wtr.double().t()
    self.scale = self.xr.double().abs() @ self.wtr.double().abs().t()

  def check(self, u, out, outb, diag, what):
    assert torch.isfinite(u).all() and torch.isfinite(out).all(), what
    assert ((u.double() - self.u_ref).abs() <= NT_REL * self.scale + ABS).all(), what
    ref = self.x0.double() * (u.double() + self.b.double() + diag * self.x.double()) + self.x.double()
    assert float((out.double() - ref).abs().max()) <= 2e-6 * float(ref.abs().max()), what
    assert torch.equal(outb, out.to(torch.bfloat16)), what


class CrossBwd(object):
  """One input-gradient launch of the cross stack's backward: v = du . w^T + dout + diag * du is the whole gradient of
  x_{l-1}, C (+)= v; with a lower cross layer du_out = v * x0, dx0 (+)= v * (prev_u + prev_bias + diag * xl), partial =
  per-64-row-tile column sums of du_out (the fp64 expressions tests/test_fused_epilogues_gpu.py::
  test_cross_stack_backward_through_the_fused_chain differentiates), du and w as bf16 operands."""
  TOL = 2e-2  # of each tensor's largest reference value: that test's bound for bf16 operands

  def __init__(self, B, d, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    self.B, self.d = B, d
    self.du = (r(B, d) * 0.1).to(torch.bfloat16).float()  # (du_in is the fp32 tensor whose bf16 copy is the operand)
    self.w = (r(d, d) * (0.5 / d ** 0.5)).to(torch.bfloat16).float()  # Bt [N = d_in, K = d_out]
    self.dout, self.base = r(B, d) * 0.1, r(B, d)
    self.x0, self.prev_u, self.xl, self.dx0_old = r(B, d), r(B, d), r(B, d), r(B, d)
    self.prev_bias = r(d) * 0.1
    self.acc = self.du.double() @ self.w.double().t()
    self.scale = self.du.double().abs() @ self.w.double().abs().t()

  def close(self, got, ref, what):
    assert torch.isfinite(got).all(), what
    err = float((got.double() - ref).abs().max())
    assert err <= self.TOL * (float(ref.abs().max()) + 1e-12), (what, err)

  def check_out(self, out, diag, accumulate, what):
    """C against fp64 at the issue's bound and at the derived one: the contraction at the NT bound, then the product with
    diag and up to three additions in fp32, each within U of the magnitudes it adds (4 U M, M the formula in absolute
    values)"""
    v = self.acc + self.dout.double() + diag * self.du.double()
    ref = v + (self.base.double() if accumulate else 0)
    self.close(out, ref, what)
    mag = self.acc.abs() + self.dout.double().abs() + abs(diag) * self.du.double().abs() + (self.base.double().abs() if accumulate else 0)
    assert ((out.double() - ref).abs() <= NT_REL * self.scale + ABS + 4 * U * mag).all(), what

  def check_lower(self, v, du_out, du_out_b, dx0, partial, diag, accumulate_dx0, what):
    """the lower layer's part.  At the issue's bound against fp64 from the reference v; and, from the v the launch stored
    (C = v without accumulate), the elementwise results within the roundings of their own fp32 operations: du_out one
    product (2 U), dx0 two additions, two products and the accumulation (6 U M), the partial sums sequential fp32 sums of
    <= 64 terms (2e-5 sum |terms| + 1e-7, as the BatchNorm partials); the bf16 copy is the rounding of du_out."""
    vr = self.acc + self.dout.double() + diag * self.du.double()
    t = self.prev_u.double() + self.prev_bias.double() + diag * self.xl.double()
    old = self.dx0_old.double() if accumulate_dx0 else 0
    self.close(du_out, vr * self.x0.double(), (what, 'du_out'))
    self.close(dx0, old + vr * t, (what, 'dx0'))
    tiles = row_tiles(self.B)
    tile_sum = lambda x: torch.stack([x[i * 64:(i + 1) * 64].sum(0) for i in range(tiles)])
    self.close(partial, tile_sum(vr * self.x0.double()), (what, 'partial'))
    vd = v.double()
    ref = vd * self.x0.double()
    assert ((du_out.double() - ref).abs() <= 2 * U * ref.abs()).all(), (what, 'du_out from the stored v')
    assert torch.equal(du_out_b, du_out.to(torch.bfloat16)), (what, 'du_out_bf16')
    tm = self.prev_u.double().abs() + self.prev_bias.double().abs() + abs(diag) * self.xl.double().abs()
    mag = (self.dx0_old.double().abs() if accumulate_dx0 else 0) + vd.abs() * tm
    assert ((dx0.double() - (old + vd * t)).abs() <= 6 * U * mag).all(), (what, 'dx0 from the stored v')
    d64 = du_out.double()
    assert ((partial.double() - tile_sum(d64)).abs() <= 2e-5 * tile_sum(d64.abs()) + 1e-7).all(), (what, 'partial from the stored du_out')


# ---------------------------------------------------------------------------------------------- er_cast_bf16
def cast_source(rows, cols, aligned, device='cpu'):
  """-> (src, wide): src [rows, cols] a column block of a wider fp32 buffer; aligned: every row starts on 16 bytes (the
  vector read path), else the block starts one float into the buffer with an odd pitch (the scalar read path).  Holds an
  infinity and a tie (1.00390625 = 1 + 2**-8 rounds to even: 1.0)."""
  g = torch.Generator().manual_seed(rows * 7 + cols)
  x = torch.randn(rows, cols, generator=g) * 3
  x[rows - 1, cols - 1] = 1.00390625
  x[0, 0] = float('inf')
  ld, off = (round4(cols) + 8, 4) if aligned else (round4(cols) + 9, 1)
  wide = torch.full((rows, ld), float('nan'), dtype=torch.float32, device=device)
  src = wide[:, off:off + cols]
  src.copy_(x.to(device))
  assert (src.data_ptr() % 16 == 0 and ld % 4 == 0) if aligned else (src.data_ptr() % 16 != 0 and ld % 4 != 0)
  return src, x


def cast_lds(width):
  return [pad8(width) + e for e in CAST_LD_EXTRA]
