"""-m gpu: bias + BatchNorm + activation, Dice and every fused form of them in libeasyrec_hip.so (through
easyrec_amd.kernels.HipBackend) against fp64 autograd of the formulas, on the cases and within the derived per-element
bounds of tests/_dense_cases.py (tests/test_dense_restatement.py holds a plain float32 evaluation and the CPU oracle to
the same ones).  A fused form is compared with the ONE fp64 formula, never with another launch: what its contraction
wrote (z, dy) is taken as data, so the contraction's own rounding - bounded by the gemm tests - stays out.

Each case also asserts the path it is meant to take where host arithmetic or the op log can tell, and that a second
launch returns the same bits.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from tests import _dense_cases as dc  # noqa: E402
from tests._interaction_cases import check  # noqa: E402

DEV = 'cuda:0'
RELU, LIN = kernels.ACT_RELU, kernels.ACT_NONE


@pytest.fixture(scope='module')
def hip():
  assert torch.cuda.is_available(), 'gpu tests need an MI355X'
  assert (kernels.BN_NONE, kernels.BN_BATCH, kernels.BN_FROZEN) == (dc.BN_NONE, dc.BN_BATCH, dc.BN_FROZEN)
  assert (kernels.ACT_NONE, kernels.ACT_RELU) == (dc.ACT_NONE, dc.ACT_RELU)
  be = kernels.hip()
  be._ck(be.lib.er_gemm_bf16_nt_prepare(), 'prepare')
  return be


def _same_bits(a, b, what):
  for k in a:
    assert torch.equal(a[k], b[k]), '%s: %s differs between two launches' % (what, k)


class _Copies(object):
  """Stands where a Bf16Shadows stands in bn_act_bwd / bn_apply_from_stats: hands out the bf16 copy's buffer, every element 7."""

  def new_copy(self, t):
    self.last = torch.full((t.shape[0], kernels.Bf16Shadows.pad8(t.shape[1])), 7.0, dtype=torch.bfloat16, device=t.device)
    return self.last


# ------------------------------------------------------------------------------------------------------------------
# the stand-alone kernels: er_bn_act_fwd / er_bn_act_bwd_ld, er_dice_fwd / er_dice_bwd
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', [c['id'] for c in dc.BN_CASES])
def test_bn_act(hip, cid):
  c, t = dc.bn_case(cid), dc.bn_inputs(cid)
  # the path this case is meant to take, from the library's own host arithmetic
  assert hip.lib.er_bn_row_chunks(c['B'], c['N']) == dc.choose_chunks(c['B'], c['N'])
  assert hip.lib.er_bn_apply_row_tiles(c['B']) == dc.apply_tiles_per_block(c['B'])
  assert hip.lib.er_gemm_row_tiles(c['B']) == dc.gemm_row_tiles(c['B'])
  got = dc.run_bn(hip, t, c['mode'], c['act'], DEV)
  want, bound = dc.bn_reference(cid, got['y'])
  check('hip', 'bn', c, got, want, bound)
  assert dc.sign_mismatches(got['y'], t, c['mode'], c['act'], dc.bn_forward_reference(cid)[1]['pre']) == 0
  if c['mode'] == dc.BN_FROZEN:  # the moving statistics come back bit-identical
    assert torch.equal(got['mm'].cpu(), t['mm']) and torch.equal(got['mv'].cpu(), t['mv'])
  if c['dy_wide']:
    assert dc.dy_of(t, DEV).stride(0) > c['N']
  _same_bits(got, dc.run_bn(hip, t, c['mode'], c['act'], DEV), cid)


@pytest.mark.parametrize('cid', ['bn-33x65-train-relu-randn', 'bn-8192x8-train-relu-randn', 'bn-8192x5-train-relu-randn-dyld'])
def test_bn_act_bf16_copies(hip, cid):
  """dxb (er_bn_act_bwd_ld_b16) and yb (er_bn_apply_from_stats_b16): the fp32 bound plus one bfloat16 rounding."""
  c, t = dc.bn_case(cid), dc.bn_inputs(cid)
  B, N = c['B'], c['N']
  x, b, gamma, beta = (t[k].to(DEV) for k in ('x', 'bias', 'gamma', 'beta'))
  z = x + b
  stats = torch.empty(dc.gemm_row_tiles(B) * N * 3, device=DEV)
  # (the statistics of z from a contraction with the identity: what the epilogue emits for exactly these values)
  z2 = hip.gemm(kernels.GEMM_NN, z, torch.eye(N, device=DEV), col_stats=stats)
  assert torch.equal(z2, z)

  def run():
    yc, dc_ = _Copies(), _Copies()
    mm, mv = t['mm'].to(DEV).clone(), t['mv'].to(DEV).clone()
    y, mean, invstd = hip.bn_apply_from_stats(z, None, stats, dc.gemm_row_tiles(B), gamma, beta, dc.EPS, dc.MOM, mm, mv, c['act'],
                                              bf16_state=yc)
    dx, _, _, _ = hip.bn_act_bwd(z, None, gamma, y, mean, invstd, dc.dy_of(t, DEV), 1, c['act'], False, True, bf16_state=dc_)
    return y, dx, yc, dc_

  y, dx, yc, dc_ = run()
  tz = dict(t, x=z.cpu(), bias=None)
  want, bound, _ = dc.bn_reference_of(tz, dc.BN_BATCH, c['act'], y)
  got = dict(y=y, dx=dx, yb=yc.last[:, :N].float(), dxb=dc_.last[:, :N].float())
  wantd = dict(y=want['y'], dx=want['dx'], yb=want['y'], dxb=want['dx'])
  bd = dict(y=bound['y'], dx=bound['dx'], yb=dc.bf16_bound(bound['y'], want['y']), dxb=dc.bf16_bound(bound['dx'], want['dx']))
  check('hip', 'bn_bf16_copies', c, got, wantd, bd)
  assert torch.equal(yc.last[:, :N], y.to(torch.bfloat16)) and torch.equal(dc_.last[:, :N], dx.to(torch.bfloat16))
  # the pad columns beside the copies (handed out holding 7) must not move
  assert bool((yc.last[:, N:] == 7).all()) and bool((dc_.last[:, N:] == 7).all())
  assert (yc.last.shape[1] > N) == (N % 8 != 0)
  y2, dx2, yc2, dc2 = run()
  _same_bits(dict(y=y, dx=dx, yb=yc.last, dxb=dc_.last), dict(y=y2, dx=dx2, yb=yc2.last, dxb=dc2.last), cid)


@pytest.mark.parametrize('cid', [c['id'] for c in dc.DICE_CASES])
def test_dice(hip, cid):
  t, want, bound = dc.dice_reference(cid)
  got = dc.run_dice(hip, t, DEV)
  check('hip', 'dice', dc.dice_case(cid), got, want, bound)
  _same_bits(got, dc.run_dice(hip, t, DEV), cid)


# ------------------------------------------------------------------------------------------------------------------
# statistics from a contraction's epilogue, then er_bn_apply_from_stats
# ------------------------------------------------------------------------------------------------------------------
def _form_tensors(name, z, N, act):
  """The case tensors of a fused form: x is the z its contraction wrote, taken as data (no bias: the GEMM added it)."""
  t = dc.bn_tensors(name, z.shape[0], N, bias=False)
  t['x'] = z.detach().cpu().clone()
  return t


def _check_form(hip, name, t, act, fwd, stats=None, T=None):
  """fwd = (y, mean, invstd, mm, mv) as the form left them; the backward is er_bn_act_bwd chained from it."""
  B, N = t['x'].shape
  got = dc.run_bn(hip, t, dc.BN_BATCH, act, DEV, fwd=fwd)
  want, bound, pre = dc.bn_reference_of(t, dc.BN_BATCH, act, got['y'])
  case = dict(id=name)
  check('hip', 'bn_form', case, got, want, bound)
  assert dc.sign_mismatches(got['y'], t, dc.BN_BATCH, act, pre) == 0
  if stats is not None:  # the emitted (count, mean, M2) records themselves, pooled exactly
    n, mean, var = dc.pooled_stats(stats, T, N)
    assert bool((n == B).all()), 'the emitted counts do not sum to B'
    sref, sbound = dc.stats_reference(t['x'])
    check('hip', 'emitted_stats', case, dict(mean=mean, var=var), sref, sbound)
  return got


@pytest.mark.parametrize('M,K,N,kind,bf16', dc.STATS_FORM_CASES)
def test_contraction_emits_statistics_then_apply(hip, M, K, N, kind, bf16):
  """gemm(col_stats=) in f32 (tile_col_stats in er_gemm_f32), in bf16 with the operands rounded while staged (er_gemm_bf16:
  'staged') and gemm_bf16_nt(epi=EPI_STATS) (True), then er_bn_apply_from_stats."""
  name = 'stats-%dx%dx%d-%s-%s' % (M, K, N, kind, dc.STATS_FLAVOUR[bf16])
  a, w, bias = (v.to(DEV) for v in dc.stats_form_operands(M, K, N, kind))
  T = hip.gemm_row_tiles(M)
  assert T == dc.gemm_row_tiles(M)

  def run():
    stats = torch.full((T * N * 3,), float('nan'), device=DEV)
    if bf16 == 'staged':
      hip.op_log = []
      try:
        z = hip.gemm(kernels.GEMM_NN, a, w, bias=bias, bf16=True, col_stats=stats)
        assert [k for k, _ in hip.op_log] == ['er::gemm_bf16_kernel<true, false>'], hip.op_log
      finally:
        hip.op_log = None
    elif bf16:
      pad = kernels.Bf16Shadows.pad8
      ab = torch.empty(M, pad(K), dtype=torch.bfloat16, device=DEV)
      wt = torch.empty(N, pad(K), dtype=torch.bfloat16, device=DEV)
      hip.cast_bf16([(a, ab, False), (w.t().contiguous(), wt, False)])
      z = torch.empty(M, N, device=DEV)
      hip.gemm_bf16_nt(ab, wt, M, N, K, out=z, bias=bias,
                       epi=kernels.GemmEpilogue(kind=kernels.EPI_STATS, col_stats=stats.data_ptr()))
    else:
      z = hip.gemm(kernels.GEMM_NN, a, w, bias=bias, col_stats=stats)
    t = _form_tensors(name, z, N, RELU)
    mm, mv = t['mm'].to(DEV).clone(), t['mv'].to(DEV).clone()
    y, mean, invstd = hip.bn_apply_from_stats(z, None, stats, T, t['gamma'].to(DEV), t['beta'].to(DEV), dc.EPS, dc.MOM, mm, mv, RELU)
    return t, z, stats, (y, mean, invstd, mm, mv)

  t, z, stats, fwd = run()
  got = _check_form(hip, name, t, RELU, fwd, stats, T)
  t2, z2, stats2, fwd2 = run()
  assert torch.equal(z, z2) and torch.equal(stats, stats2)
  _same_bits(dict(y=fwd[0], mean=fwd[1], invstd=fwd[2], mm=fwd[3], mv=fwd[4]),
             dict(y=fwd2[0], mean=fwd2[1], invstd=fwd2[2], mm=fwd2[3], mv=fwd2[4]), name)
  assert (T > dc.K_INLINE_CHUNKS) == (M > 16384)  # the merge launch runs from 257 row tiles on


# ------------------------------------------------------------------------------------------------------------------
# finalize alone + the apply inside the next contraction's staging (er_gemm_f32_bn_a / er_gemv_f32_bn_a)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,K,N,kind,chain', [(16385, 8, 3, 'mean1000', False), (16385, 8, 8, 'head0', True), (777, 32, 20, 'drift', True),
                                              (4096, 64, 4, 'mean1000', False), (130, 12, 5, 'randn', True)])
def test_apply_in_the_next_contractions_staging(hip, M, K, N, kind, chain):
  name = 'bn_a-%dx%dx%d-%s' % (M, K, N, kind)
  a, w0 = (v.to(DEV) for v in dc.gemm_operands(kind, M, 8, K, M + K))
  g = torch.Generator().manual_seed(M + N)
  w1 = (torch.randn(K, N, generator=g) * 0.2).to(DEV)
  b1 = torch.randn(N, generator=g).to(DEV)
  T = hip.gemm_row_tiles(M)
  stats = torch.empty(T * K * 3, device=DEV)
  z = hip.gemm(kernels.GEMM_NN, a, w0, col_stats=stats)
  t = _form_tensors(name, z, K, RELU)

  def run():
    pend = dict(z=z, stats=stats, chunks=T, gamma=t['gamma'].to(DEV), beta=t['beta'].to(DEV), eps=dc.EPS, momentum=dc.MOM,
                moving_mean=t['mm'].to(DEV).clone(), moving_var=t['mv'].to(DEV).clone(), act=RELU, y=torch.full_like(z, float('nan')),
                mean=torch.empty(K, device=DEV), invstd=torch.empty(K, device=DEV))
    assert hip.bn_a_ok(pend, w1)
    s2 = torch.full((T * N * 3,), float('nan'), device=DEV) if chain else None
    hip.op_log = []
    try:
      out = hip.gemm_bn_a(pend, w1, b1, col_stats=s2)
      log = [k for k, _ in hip.op_log]
    finally:
      hip.op_log = None
    return pend, out, s2, log

  pend, out, s2, log = run()
  gemv = (not chain) and N <= 4 and M >= hip.BN_IN_STAGING_MIN_ROWS
  assert hip.gemv_ok(z, M, N, K) == (N <= 4 and M >= hip.BN_IN_STAGING_MIN_ROWS)
  assert log == ['er::gemv_bna_kernel<%d>' % N] if gemv else log == ['er::gemm_f32_bna_kernel'], log
  fwd = (pend['y'], pend['mean'], pend['invstd'], pend['moving_mean'], pend['moving_var'])
  _check_form(hip, name, t, RELU, fwd, stats, T)
  # the contraction on the activations it left behind (taken as data)
  ref, bound = dc.gemm_bound(pend['y'], w1, b1)
  check('hip', 'bn_a_out', dict(id=name), dict(out=out), dict(out=ref), dict(out=bound))
  if chain:  # ... and its own column statistics feed the next layer's apply
    t2 = _form_tensors(name + '-next', out, N, LIN)
    mm, mv = t2['mm'].to(DEV).clone(), t2['mv'].to(DEV).clone()
    y, mean, invstd = hip.bn_apply_from_stats(out, None, s2, T, t2['gamma'].to(DEV), t2['beta'].to(DEV), dc.EPS, dc.MOM, mm, mv, LIN)
    _check_form(hip, name + '-next', t2, LIN, (y, mean, invstd, mm, mv), s2, T)
  pend2, out2, s22, _ = run()
  assert torch.equal(out, out2) and torch.equal(pend['y'], pend2['y']) and torch.equal(pend['invstd'], pend2['invstd'])
  assert s2 is None or torch.equal(s2, s22)


# ------------------------------------------------------------------------------------------------------------------
# the apply fused with the wide / FM concat (er_bn_apply_wide_fm)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,K,N,n_w,F,D,kind', [(4096, 16, 64, 39, 39, 16, 'head0'), (8192, 8, 128, 5, 7, 8, 'mean1000'),
                                                (100, 8, 20, 5, 7, 3, 'drift')])
def test_bn_apply_wide_fm(hip, B, K, N, n_w, F, D, kind):
  name = 'wide_fm-%dx%d-%s' % (B, N, kind)
  a, w = (v.to(DEV) for v in dc.gemm_operands(kind, B, K, N, B + N))
  g = torch.Generator().manual_seed(B)
  wide_full = torch.randn(B, n_w + 3, generator=g).to(DEV)
  x_full = torch.randn(B, F * D + (4 if D % 4 == 0 else 1), generator=g).to(DEV)
  wide, fx = wide_full[:, :n_w], x_full[:, :F * D]
  T = hip.gemm_row_tiles(B)
  stats = torch.empty(T * N * 3, device=DEV)
  z = hip.gemm(kernels.GEMM_NN, a, w, col_stats=stats)
  t = _form_tensors(name, z, N, RELU)

  def run():
    pend = dict(z=z, stats=stats, chunks=T, gamma=t['gamma'].to(DEV), beta=t['beta'].to(DEV), eps=dc.EPS, momentum=dc.MOM,
                moving_mean=t['mm'].to(DEV).clone(), moving_var=t['mv'].to(DEV).clone(), act=RELU, y=torch.full_like(z, float('nan')),
                mean=torch.empty(N, device=DEV), invstd=torch.empty(N, device=DEV))
    res = hip.bn_apply_wide_fm(pend, wide, fx, F, D)
    assert res is not None
    return pend, res[0], res[1]

  pend, out, S = run()
  _check_form(hip, name, t, RELU, (pend['y'], pend['mean'], pend['invstd'], pend['moving_mean'], pend['moving_var']), stats, T)
  assert torch.equal(out[:, 1 + D:], pend['y'])  # the concat's column block is the same activation
  fm, S1 = hip.fm_fwd(fx, F, D)
  assert torch.equal(out[:, 1:1 + D], fm) and torch.equal(S, S1) and torch.equal(out[:, :1], hip.rowsum_fwd(wide, n_w))
  pend2, out2, S2 = run()
  assert torch.equal(out, out2) and torch.equal(S, S2) and torch.equal(pend['mean'], pend2['mean'])


# ------------------------------------------------------------------------------------------------------------------
# backward column sums from the input-gradient contraction (er_gemm_f32_bn_bwd, _cols) + er_bn_act_bwd_from_partials
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,K,col0,n_src,data,act,use_bn', [
    (4096, 64, 16, None, 0, 'mean1000', RELU, 1), (300, 72, 8, 8, 32, 'randn', RELU, 1), (130, 65, 8, None, 0, 'drift', LIN, 1),
    (33, 5, 4, 1, 3, 'bigbias', RELU, 1), (16385, 8, 4, None, 0, 'randn', RELU, 1), (130, 20, 8, None, 0, 'randn', RELU, 0)])
def test_input_gradient_contraction_emits_the_backward_sums(hip, B, N, K, col0, n_src, data, act, use_bn):
  ns = n_src or N
  name = 'bn_bwd-%dx%dx%d-%s-c%s' % (B, N, K, data, col0)
  t = dc.bn_tensors(name, B, ns, data=data, head=64)
  x, b, gamma, beta = (t[k].to(DEV) for k in ('x', 'bias', 'gamma', 'beta'))
  mode = dc.BN_BATCH if use_bn else dc.BN_NONE
  if not use_bn:
    t['gamma'] = t['beta'] = gamma = beta = None
  y, mean, invstd = hip.bn_act_fwd(x, b, gamma, beta, mode, dc.EPS, dc.MOM, None, None, act)
  g = torch.Generator().manual_seed(B + N)
  dzn = (torch.randn(B, K, generator=g) * 0.1).to(DEV)
  w = torch.randn(N, K, generator=g).to(DEV)
  src = kernels.BnSource(x, b, y, mean, invstd, act, gamma)
  T = hip.gemm_row_tiles(B)

  def run():
    partial = torch.full((T * ns * 2,), float('nan'), device=DEV)
    hip.op_log = []
    try:
      dy = hip.gemm_bn_bwd(kernels.GEMM_NT, dzn, w, src, partial, col0=col0)
      log = [k for k, _ in hip.op_log]
    finally:
      hip.op_log = None
    assert log == ['er::gemm_f32_bn_bwd_kernel<true, true>'], log
    blk = dy if col0 is None else dy[:, col0:col0 + ns]
    res = hip.bn_act_bwd(x, b, gamma, y, mean, invstd, blk, mode, act, True, use_bn == 1, partial=partial)
    return dy, blk, partial, res

  dy, blk, partial, res = run()
  assert col0 is None or blk.stride(0) > ns
  # the sums: sum g and sum g xhat of the dy the contraction wrote and the y / mean / invstd handed to it
  ref, bd = dc.colsum_reference(blk, x, b, y, mean, invstd, act)
  p = partial.view(T, ns, 2).double().sum(dim=0).cpu()
  got = dict(sg=p[:, 0], sgx=p[:, 1]) if use_bn else dict(sg=p[:, 0])
  check('hip', 'bwd_sums', dict(id=name), got, ref, bd)
  # the backward that consumes them, against autograd on that dy
  t['dyw'] = torch.zeros(B, ns + dc.DY_PAD)
  t['dyw'][:, 2:2 + ns] = blk.cpu()
  want, bound, _ = dc.bn_reference_of(t, mode, act, y)
  names = ('dx', 'dbias', 'dgamma', 'dbeta')
  gotb = {k: v for k, v in zip(names, res) if v is not None}
  check('hip', 'bwd_from_partials', dict(id=name), gotb, {k: want[k] for k in gotb}, {k: bound[k] for k in gotb})
  dy2, _, partial2, res2 = run()
  assert torch.equal(dy, dy2) and torch.equal(partial, partial2)
  _same_bits(gotb, {k: v for k, v in zip(names, res2) if v is not None}, name)


@pytest.mark.parametrize('B,K,with_bn', [(4096, 64, True), (130, 8, True), (300, 64, False), (1000, 256, True)])
def test_head_sigmoid_ce_emits_the_backward_sums(hip, B, K, with_bn):
  """er_head_sigmoid_ce with its BatchNorm sums on: per 64-row tile (sum g, sum g xhat) of the producing layer, g the dx it
  wrote masked by the layer's activation output."""
  name = 'head-%dx%d-%d' % (B, K, with_bn)
  t = dc.bn_tensors(name, B, K, data='mean1000' if with_bn else 'randn', bias=False)
  z, gamma, beta = (t[k].to(DEV) for k in ('x', 'gamma', 'beta'))
  if with_bn:
    yc, mean, invstd = hip.bn_act_fwd(z, None, gamma, beta, 1, dc.EPS, dc.MOM, None, None, RELU)
  else:
    yc, mean, invstd = hip.bn_act_fwd(z, None, None, None, 0, dc.EPS, dc.MOM, None, None, RELU)
  xbuf = torch.zeros(B, K + 8, device=DEV)
  xbuf[:, :K] = yc
  x = xbuf[:, :K]  # (a row stride wider than K: the head reads a column block in place)
  g = torch.Generator().manual_seed(B + K)
  w = (torch.randn(K, 1, generator=g) * 0.3).to(DEV)
  b = torch.randn(1, generator=g).to(DEV)
  labels = (torch.rand(B, generator=g) < 0.3).float().to(DEV)
  src = kernels.BnSource(z, None, x, mean, invstd, RELU)
  out = hip.head_sigmoid_ce(x, w, b, labels, 0.7, src=src)
  ref, bd = dc.colsum_reference(out['dx'], z, None, x, mean, invstd, RELU)
  p = out['bn_partials'].double().sum(dim=0).cpu()
  assert out['bn_partials'].shape == (dc.gemm_row_tiles(B), K, 2)
  got = dict(sg=p[:, 0], sgx=p[:, 1]) if with_bn else dict(sg=p[:, 0])
  check('hip', 'head_sums', dict(id=name), got, ref, bd)
  if not with_bn:
    assert not bool(p[:, 1].abs().sum())  # no BatchNorm: the second sum is zero
  out2 = hip.head_sigmoid_ce(x, w, b, labels, 0.7, src=src)
  assert torch.equal(out['bn_partials'], out2['bn_partials']) and torch.equal(out['dx'], out2['dx'])


# ------------------------------------------------------------------------------------------------------------------
# several layers in one launch (er_bn_fwd_multi / er_bn_bwd_multi), layers of unequal shape and mode
# ------------------------------------------------------------------------------------------------------------------
def test_bn_multi_layers_of_unequal_shape(hip):
  specs = [('multi-batch', 300, 72, dc.BN_BATCH, 'mean1000'), ('multi-frozen', 130, 20, dc.BN_FROZEN, 'bigbias'),
           ('multi-none', 64, 5, dc.BN_NONE, 'randn'), ('multi-batch2', 4096, 64, dc.BN_BATCH, 'head0')]
  L = []
  for name, B, N, mode, data in specs:
    if mode == dc.BN_BATCH:  # batch statistics come from a contraction's epilogue: z is its output, no bias of the layer's own
      a, w = (v.to(DEV) for v in dc.gemm_operands(data, B, 8, N, B + N))
      stats = torch.empty(hip.gemm_row_tiles(B) * N * 3, device=DEV)
      z = hip.gemm(kernels.GEMM_NN, a, w, col_stats=stats)
      t = _form_tensors(name, z, N, RELU)
    else:
      t = dc.bn_tensors(name, B, N, data=data, mode=mode, affine=mode != dc.BN_NONE)
      stats = None
    L.append(dict(name=name, t=t, mode=mode, stats=stats))

  def run():
    fl = []
    for l in L:
      t = l['t']
      dev = lambda k: None if t[k] is None else t[k].to(DEV)  # noqa: E731
      fl.append(dict(x=dev('x'), bias=dev('bias'), gamma=dev('gamma'), beta=dev('beta'),
                     moving_mean=t['mm'].to(DEV).clone() if l['mode'] else None, moving_var=t['mv'].to(DEV).clone() if l['mode'] else None,
                     col_stats=l['stats'], use_bn=l['mode'], act=RELU, eps=dc.EPS, momentum=dc.MOM))
    outs = hip.bn_fwd_multi(fl)
    bl = [dict(x=f['x'], bias=f['bias'], gamma=f['gamma'], beta=f['beta'], y=o[0], mean=o[1], invstd=o[2], dy=dc.dy_of(l['t'], DEV),
               use_bn=l['mode'], act=RELU, partial=None, into=None) for f, o, l in zip(fl, outs, L)]
    return fl, outs, hip.bn_bwd_multi(bl)

  fl, outs, grads = run()
  fl2, outs2, grads2 = run()
  for l, f, f2, o, gr, o2, gr2 in zip(L, fl, fl2, outs, grads, outs2, grads2):
    if l['mode']:
      assert torch.equal(f['moving_mean'], f2['moving_mean']) and torch.equal(f['moving_var'], f2['moving_var']), l['name']
    got = dict(y=o[0], dx=gr[0])
    if l['mode']:
      got.update(save_mean=o[1], save_invstd=o[2], mm=f['moving_mean'], mv=f['moving_var'])
    for k, v in zip(('dbias', 'dgamma', 'dbeta'), gr[1:]):
      if v is not None:
        got[k] = v
    want, bound, pre = dc.bn_reference_of(l['t'], l['mode'], RELU, o[0])
    check('hip', 'bn_multi', dict(id=l['name']), got, {k: want[k] for k in got}, {k: bound[k] for k in got})
    assert dc.sign_mismatches(o[0], l['t'], l['mode'], RELU, pre) == 0
    if l['mode'] == dc.BN_FROZEN:
      assert torch.equal(f['moving_mean'].cpu(), l['t']['mm']) and torch.equal(f['moving_var'].cpu(), l['t']['mv'])
    assert all(a is None or torch.equal(a, b) for a, b in zip(o, o2)), l['name']    # y, mean, invstd
    assert all(a is None or torch.equal(a, b) for a, b in zip(gr, gr2)), l['name']  # dx, dbias, dgamma, dbeta


# ------------------------------------------------------------------------------------------------------------------
# frozen statistics inside the grouped contractions: the forward epilogue (fz_*) and bn_dz_out
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,K,Ns,data', [(4096, 16, (64, 20), 'bigbias'), (100, 12, (37, 64), 'bigbias')])
def test_grouped_contraction_frozen_epilogues(hip, M, K, Ns, data):
  g = torch.Generator().manual_seed(M + K)
  xin = torch.randn(M, K, generator=g).to(DEV)
  L = []
  for i, n in enumerate(Ns):
    name = 'grouped-frozen-%dx%d-%s' % (M, n, data)
    w = (torch.randn(K, n, generator=g) * 0.1).to(DEV)
    z = hip.gemm(kernels.GEMM_NN, xin, w)  # (the values the grouped launch will write, for the case's moving statistics)
    t = dc.bn_tensors(name, M, n, data=data, mode=dc.BN_FROZEN)
    zz = z.cpu().double() + t['bias'].double()
    t['mm'] = (zz.mean(0) * 1.01).float()
    t['mv'] = (zz.var(0, unbiased=False) * 0.9 + 0.01).float()
    L.append(dict(name=name, t=t, w=w, n=n, wT=torch.randn(n, K, generator=g).to(DEV), dzn=(torch.randn(M, K, generator=g) * 0.1).to(DEV)))

  def run():
    zs = [torch.full((M, l['n']), float('nan'), device=DEV) for l in L]
    fz = [dict(bias=l['t']['bias'].to(DEV), gamma=l['t']['gamma'].to(DEV), beta=l['t']['beta'].to(DEV),
               moving_mean=l['t']['mm'].to(DEV).clone(), moving_var=l['t']['mv'].to(DEV).clone(), eps=dc.EPS, act=RELU,
               y=torch.full((M, l['n']), float('nan'), device=DEV), save=torch.empty(2, l['n'], device=DEV)) for l in L]
    hip.gemm_grouped(kernels.GEMM_NN, [(xin, l['w'], zs[i], None, False, None, None, fz[i]) for i, l in enumerate(L)])
    # the input-gradient contraction of the layer above, leaving dz = gamma * invstd * masked dy and the column sums
    dz = [torch.full((M, l['n']), float('nan'), device=DEV) for l in L]
    parts = [torch.empty(hip.gemm_row_tiles(M) * l['n'] * 2, device=DEV) for l in L]
    srcs = []
    for i, l in enumerate(L):
      s = kernels.BnSource(zs[i], fz[i]['bias'], fz[i]['y'], fz[i]['save'][0], fz[i]['save'][1], RELU, fz[i]['gamma'], None,
                           beta=fz[i]['beta'], fused=True)
      s.frozen = True
      srcs.append(s)
    hip.gemm_grouped(kernels.GEMM_NT, [(l['dzn'], l['wT'], dz[i], None, False, None, (srcs[i], parts[i], True)) for i, l in enumerate(L)])
    gr = hip.bn_bwd_multi([dict(x=zs[i], bias=fz[i]['bias'], gamma=fz[i]['gamma'], beta=fz[i]['beta'], y=fz[i]['y'], mean=fz[i]['save'][0],
                                invstd=fz[i]['save'][1], dy=dz[i], use_bn=kernels.BN_FROZEN, act=RELU, partial=parts[i], into=None,
                                dx_done=True) for i, l in enumerate(L)])
    return zs, fz, dz, gr

  zs, fz, dz, gr = run()
  # the plain contraction's dy, as data for the reference backward
  dys = [torch.empty(M, l['n'], device=DEV) for l in L]
  hip.gemm_grouped(kernels.GEMM_NT, [(l['dzn'], l['wT'], dys[i], None, False) for i, l in enumerate(L)])
  zs2, fz2, dz2, gr2 = run()
  for i, l in enumerate(L):
    t = dict(l['t'], x=zs[i].cpu())
    t['dyw'] = torch.zeros(M, l['n'] + dc.DY_PAD)
    t['dyw'][:, 2:2 + l['n']] = dys[i].cpu()
    got = dict(y=fz[i]['y'], save_mean=fz[i]['save'][0], save_invstd=fz[i]['save'][1], mm=fz[i]['moving_mean'], mv=fz[i]['moving_var'],
               dx=dz[i], dbias=gr[i][1], dgamma=gr[i][2], dbeta=gr[i][3])
    want, bound, pre = dc.bn_reference_of(t, dc.BN_FROZEN, RELU, fz[i]['y'])
    check('hip', 'grouped_frozen', dict(id=l['name']), got, {k: want[k] for k in got}, {k: bound[k] for k in got})
    assert dc.sign_mismatches(fz[i]['y'], t, dc.BN_FROZEN, RELU, pre) == 0
    assert torch.equal(fz[i]['moving_mean'].cpu(), l['t']['mm']) and torch.equal(fz[i]['moving_var'].cpu(), l['t']['mv'])
    assert gr[i][0].data_ptr() == dz[i].data_ptr()
    assert torch.equal(zs[i], zs2[i]) and torch.equal(fz[i]['y'], fz2[i]['y']) and torch.equal(dz[i], dz2[i])
    assert all(torch.equal(a, b) for a, b in zip(gr[i][1:], gr2[i][1:]))
