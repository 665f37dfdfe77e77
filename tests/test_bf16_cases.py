"""The bf16 contraction cases (tests/_bf16_cases.py) without a GPU: what the module claims about its own operands,
expected values, bounds, poisoned padding and sentinels, so that tests/test_gemm_bf16_ring_gpu.py cannot pass for the
wrong reason."""
import pytest
import torch

from tests import _bf16_cases as bc


def _exact_cases():
  for K in bc.KS:
    yield 'K=%d' % K, bc.exact_for_k(K)
  for layout in (bc.GEMM_NN, bc.GEMM_NT, bc.GEMM_TN):
    for M, N, K in bc.GEMM_SHAPES:
      yield 'gemm %d %r' % (layout, (M, N, K)), bc.exact_gemm(layout, M, N, K)[0]
  for N, K in bc.EPI_NK:
    yield 'epi %r' % ((N, K),), bc.Exact(max(bc.EPI_BS), N, K, 3000 + N + K)


_EXACT = list(_exact_cases())


def test_layout_constants_are_the_librarys():
  from easyrec_amd import kernels
  assert (bc.GEMM_NN, bc.GEMM_NT, bc.GEMM_TN) == (kernels.GEMM_NN, kernels.GEMM_NT, kernels.GEMM_TN)
  assert [bc.pad8(n) for n in (1, 8, 9, 130)] == [kernels.Bf16Shadows.pad8(n) for n in (1, 8, 9, 130)]


def test_shape_lists_are_the_ones_the_ring_needs():
  """every K is one the entry point admits (a multiple of 8); the k-tile counts 1 .. 10 all occur, ragged and full"""
  assert all(K % 8 == 0 and K <= bc.K_EXACT_MAX for K in bc.KS)
  assert {(K + 63) // 64 for K in bc.KS} == set(range(1, 11))
  assert {K for K in bc.KS if K % 64 == 0} >= {64, 128, 192, 256, 320, 384, 512}
  assert all(M in bc.MS and N in bc.NS for M, N in bc.RANDOM_MN)
  assert bc.PAD % 8 == 0 and bc.PAD >= 64
  for N in bc.NS:
    p = bc.pitches(N)
    assert p[0] == N and p[1] % 4 != N % 4 and p[2] % 4 == 0 and p[2] > N


@pytest.mark.parametrize('name,e', _EXACT, ids=[n for n, _ in _EXACT])
def test_exact_operands_are_bfloat16_and_sums_stay_exact(name, e):
  for t in (e.a, e.b, e.bias, e.base):
    assert torch.equal(t.to(torch.bfloat16).float(), t)
    assert torch.equal(t, t.round())
  assert e.magnitude() < 2 ** 24
  exp = e.expected(bias=True, base=True)
  assert torch.equal(exp.double(), (e.prod_int + e.bias_int + e.base_int).double())


@pytest.mark.parametrize('name,e', _EXACT, ids=[n for n, _ in _EXACT])
def test_float32_in_a_shuffled_k_order_gives_the_integer_result(name, e):
  """chunk by chunk (8 k = one 16-byte chunk of the kernel) in a shuffled order, accumulating in float32; and the same in
  two independent halves that are then added (a k-split)"""
  g = torch.Generator().manual_seed(e.K)
  chunks = [torch.arange(k, min(k + 8, e.K)) for k in range(0, e.K, 8)]
  order = torch.randperm(len(chunks), generator=g).tolist()
  acc = torch.zeros(e.M, e.N)
  halves = [torch.zeros(e.M, e.N), torch.zeros(e.M, e.N)]
  for i, c in enumerate(order):
    part = e.a[:, chunks[c]] @ e.b[:, chunks[c]].t()
    acc = acc + part
    halves[i % 2] = halves[i % 2] + part
  assert acc.dtype == torch.float32
  assert torch.equal(acc, e.expected())
  assert torch.equal(halves[0] + halves[1], e.expected())
  assert torch.equal(acc + e.bias + e.base, e.expected(bias=True, base=True))


def test_leading_rows_of_the_per_k_operands_give_the_sliced_result():
  e = bc.exact_for_k(72)
  for M, N in ((1, 1), (65, 63), (257, 132)):
    assert torch.equal(e.expected(M, N, bias=True).double(), (e.a_int[:M] @ e.b_int[:N].t() + e.bias_int[:N]).double())


@pytest.mark.parametrize('K', bc.KS)
def test_a_plain_float32_product_meets_the_nt_bound(K):
  """the random-operand reference, re-evaluated as a float32 `@` of the rounded operands, sits inside the stated bound: a
  correct fp32-accumulate kernel can meet it"""
  r = bc.random_for_k(K)
  assert torch.equal(r.a.to(torch.bfloat16).float(), r.a) and torch.equal(r.b.to(torch.bfloat16).float(), r.b)
  got = r.a @ r.b.t()
  assert ((got.double() - r.ref).abs() <= r.bound(bc.NT_REL)).all()


@pytest.mark.parametrize('layout', [bc.GEMM_NN, bc.GEMM_NT, bc.GEMM_TN])
def test_a_plain_float32_product_meets_the_staging_kernels_bound(layout):
  for M, N, K in bc.GEMM_SHAPES:
    r, a, b = bc.random_gemm(layout, M, N, K)
    A = a.t() if layout == bc.GEMM_TN else a
    Bm = b.t() if layout == bc.GEMM_NT else b
    assert A.shape == (M, K) and Bm.shape == (K, N)
    got = A.to(torch.bfloat16).float() @ Bm.to(torch.bfloat16).float()
    assert ((got.double() - r.ref).abs() <= r.bound(bc.GEMM_REL)).all(), (layout, M, N, K)
    e, a, b = bc.exact_gemm(layout, M, N, K)
    A = a.t() if layout == bc.GEMM_TN else a
    Bm = b.t() if layout == bc.GEMM_NT else b
    assert torch.equal(A @ Bm, e.expected())


def test_poisoned_padding_is_where_the_builder_says():
  e = bc.exact_for_k(56)
  buf = bc.poisoned_bf16(e.a)
  assert buf.dtype == torch.bfloat16 and buf.shape == (bc.M_MAX, 56 + bc.PAD) and buf.stride(0) % 8 == 0
  assert torch.equal(buf[:, :56].float(), e.a)
  assert torch.isnan(buf[:, 56:]).all()
  with pytest.raises(AssertionError):
    bc.poisoned_bf16(torch.full((2, 8), 1.00390625))  # (not a bfloat16 value)
  x = torch.arange(15, dtype=torch.float32).view(3, 5)
  for view in (bc.aligned_f32(x), bc.unaligned_f32(x)):
    assert torch.equal(view, x)
  v = bc.aligned_f32(x)
  assert torch.isnan(torch.as_strided(v, (3, 8), (8, 1))[:, 5:]).all()
  v = bc.unaligned_f32(x)
  whole = torch.as_strided(v, (1 + 3 * 9,), (1,), 0)
  assert int(torch.isnan(whole).sum()) == 1 + 3 * 9 - 15
  v = bc.padded_rows_f32(torch.ones(3, 8))
  assert v.stride(0) == 12 and torch.isnan(torch.as_strided(v, (3, 12), (12, 1))[:, 8:]).all()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_window_sentinels_and_guard_check(dtype):
  sent = bc.SENT[dtype]
  assert float(torch.tensor(sent, dtype=dtype)) == sent  # exact in the window's type
  w = bc.Window(3, 5, 8, dtype=dtype)
  assert w.buf.numel() == 2 * bc.GUARD + 3 * 8 and w.out.data_ptr() % 16 == 0
  assert int(w.guard_mask().sum()) == w.buf.numel() - 15
  assert (w.buf == sent).all()
  w.out.fill_(1.0)
  assert torch.equal(w.read('ok'), torch.ones(3, 5, dtype=dtype))
  for at in (bc.GUARD - 1, bc.GUARD + 5, bc.GUARD + 2 * 8 + 5, bc.GUARD + 3 * 8):  # in front, between rows, behind the last row
    w = bc.Window(3, 5, 8, dtype=dtype)
    w.buf[at] = 0.0
    with pytest.raises(AssertionError):
      w.read('a store outside')
  w = bc.Window(2, 2, base=torch.tensor([[1.0, 2.0], [3.0, 4.0]]), dtype=dtype)
  assert torch.equal(w.read('base').float(), torch.tensor([[1.0, 2.0], [3.0, 4.0]]))


def test_reference_checkers_accept_float32_and_reject_a_wrong_tile():
  """the epilogue checkers on float32 evaluations of their own formulas; each must reject a result that is off by one row"""
  e = bc.Exact(129, 68, 264, 5)
  z = e.expected(bias=True)
  tiles = bc.row_tiles(129)
  st = torch.zeros(tiles, 68, 3)
  for t in range(tiles):
    rows = z[t * 64:(t + 1) * 64]
    st[t, :, 0], st[t, :, 1] = rows.shape[0], rows.mean(0)
    st[t, :, 2] = ((rows - rows.mean(0)) ** 2).sum(0)
  bc.check_col_stats(st, z, 'f32')
  bad = st.clone()
  bad[2, :, 1] = z[127]  # (the last tile holds row 128 only)
  with pytest.raises(AssertionError):
    bc.check_col_stats(bad, z, 'wrong row')
  for use_bn in (True, False):
    src = bc.BnSource(129, 8, use_bn, True, 9)
    dy = z[:, 4:12]
    gm = dy * (src.y > 0).float()
    xhat = ((src.z + src.zbias - src.mean) * src.invstd) if use_bn else torch.zeros_like(src.z)
    p = torch.stack([torch.stack([gm[t * 64:(t + 1) * 64].sum(0), (gm * xhat)[t * 64:(t + 1) * 64].sum(0)], 1) for t in range(tiles)])
    src.check_partial(p, dy, 'f32')
    with pytest.raises(AssertionError):
      src.check_partial(p, z[:, 5:13], 'wrong block')


@pytest.mark.parametrize('diag', [0.0, 0.5])
def test_cross_checkers_accept_a_float32_evaluation(diag):
  c = bc.CrossFwd(65, 72, 7)
  u = c.xr @ c.wtr.t()
  out = c.x0 * (u + c.b + diag * c.x) + c.x
  c.check(u, out, out.to(torch.bfloat16), diag, 'f32')
  with pytest.raises(AssertionError):
    c.check(u, out + c.x0 * 1e-3, out.to(torch.bfloat16), diag, 'off')
  b = bc.CrossBwd(129, 72, 8)
  v = b.du @ b.w.t() + b.dout
  v = v + diag * b.du if diag else v
  b.check_out(v, diag, False, 'f32')
  b.check_out(v + b.base, diag, True, 'f32 +=')
  du_out = v * b.x0
  t = b.prev_u + b.prev_bias
  t = t + diag * b.xl if diag else t
  tiles = bc.row_tiles(129)
  partial = torch.stack([du_out[i * 64:(i + 1) * 64].sum(0) for i in range(tiles)])
  for acc0 in (False, True):
    dx0 = b.dx0_old + v * t if acc0 else v * t
    b.check_lower(v, du_out, du_out.to(torch.bfloat16), dx0, partial, diag, acc0, 'f32')
  with pytest.raises(AssertionError):
    b.check_lower(v, du_out, du_out.to(torch.bfloat16), v * t, partial.roll(1, 0), diag, False, 'tiles swapped')


def test_cast_sources_take_both_read_paths():
  for rows, cols in bc.CAST_SHAPES:
    for aligned in (True, False):
      src, x = bc.cast_source(rows, cols, aligned)
      assert torch.equal(src, x) and src.stride(1) == 1
      assert all((src.data_ptr() + 4 * r * src.stride(0)) % 16 == 0 for r in range(rows)) == aligned or rows * cols == 1
      assert torch.isinf(x[0, 0]) and (rows * cols == 1 or float(x[-1, -1].to(torch.bfloat16)) == 1.0)
    assert bc.cast_lds(rows) == [bc.pad8(rows), bc.pad8(rows) + 8, bc.pad8(rows) + 40]
  # the transposed kernel works in 32 x 32 tiles: the lists hold destinations wider than the last tile's edge
  assert any(ld > (rows + 31) // 32 * 32 for rows, _ in bc.CAST_SHAPES for ld in bc.cast_lds(rows))
