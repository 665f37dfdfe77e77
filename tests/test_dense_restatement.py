"""The dense-layer cases (tests/_dense_cases.py) without a GPU:

  * the formulas evaluated in plain float32 (two-pass variance, float32 autograd) fit HALF of every derived bound;
  * oracle.kernel_ref.RefBackend fits every bound, forward and backward, fresh buffers and accumulate-into;
  * a RefBackend carrying one deliberate mistake fails the case meant to catch it - in particular the float32
    E[z^2] - mean^2 variance fails the large-mean case;
  * the host arithmetic the case comments rely on (row chunks, the empty last chunk, the pre-merge threshold, row tiles
    per workgroup) is what the built library answers through er_bn_row_chunks / er_bn_apply_row_tiles /
    er_gemm_row_tiles (host-side entry points: no device is touched);
  * the emitted-statistics cases tell a per-tile float32 E[z^2] - mean^2 from a two-pass evaluation, for every flavour
    of contraction.

tests/test_dense_gpu.py runs the same cases through the HIP kernels and their fused forms.
"""
import pytest
import torch

from oracle import kernel_ref
from oracle.kernel_ref import RefBackend
from tests import _dense_cases as dc
from tests._interaction_cases import F32, check, ratios

_BN_IDS = [c['id'] for c in dc.BN_CASES]
_DICE_IDS = [c['id'] for c in dc.DICE_CASES]


@pytest.fixture(scope='module')
def ref():
  return RefBackend()


def test_constants_are_the_oracles():
  assert (dc.BN_FROZEN, dc.ACT_RELU) == (kernel_ref.BN_FROZEN, kernel_ref.ACT_RELU)


# ------------------------------------------------------------------------------------------------------------------
# plain float32 within half the bound; RefBackend within the bound
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', _BN_IDS)
def test_bn_plain_float32_fits_half_the_bound(cid):
  c, t = dc.bn_case(cid), dc.bn_inputs(cid)
  got = dc.bn_plain(t, c['mode'], c['act'], F32)
  want, bound = dc.bn_reference(cid, got['y'])
  check('f32', 'bn', c, got, want, bound, frac=0.5)
  assert dc.sign_mismatches(got['y'], t, c['mode'], c['act'], dc.bn_forward_reference(cid)[1]['pre']) == 0


@pytest.mark.parametrize('cid', _BN_IDS)
def test_bn_ref_backend_fits_the_bound(cid, ref):
  c, t = dc.bn_case(cid), dc.bn_inputs(cid)
  got = dc.run_bn(ref, t, c['mode'], c['act'])
  want, bound = dc.bn_reference(cid, got['y'])
  check('ref', 'bn', c, got, want, bound)
  assert dc.sign_mismatches(got['y'], t, c['mode'], c['act'], dc.bn_forward_reference(cid)[1]['pre']) == 0
  if c['mode'] == dc.BN_FROZEN:
    assert torch.equal(got['mm'], t['mm']) and torch.equal(got['mv'], t['mv'])


@pytest.mark.parametrize('cid', _DICE_IDS)
def test_dice_plain_float32_fits_half_the_bound(cid):
  t, want, bound = dc.dice_reference(cid)
  check('f32', 'dice', dc.dice_case(cid), dc.dice_plain(t, F32), want, bound, frac=0.5)


@pytest.mark.parametrize('cid', _DICE_IDS)
def test_dice_ref_backend_fits_the_bound(cid, ref):
  t, want, bound = dc.dice_reference(cid)
  check('ref', 'dice', dc.dice_case(cid), dc.run_dice(ref, t), want, bound)


def test_autograd_leaves_only_noise_in_the_bias_gradient_under_batch_statistics():
  """The reference keeps autograd's value for dbias; it is zero up to fp64 rounding, far inside the bound."""
  cid = 'bn-33x65-train-relu-randn'
  want, bound = dc.bn_reference(cid, dc.bn_forward_reference(cid)[0]['y'])
  assert float(want['dbias'].abs().max()) < 1e-12 and bool((want['dbias'].abs() <= bound['dbias']).all())
  assert torch.equal(want['acc_dbias'], dc.bn_inputs(cid)['old']['dbias'].double())


def test_case_lists_cover_what_they_claim():
  ids = set(_BN_IDS)
  assert len(ids) == len(_BN_IDS)
  for B in (1, 2, 15, 16, 17, 33):
    for N in (1, 3, 63, 64, 65, 130):
      assert any(c['B'] == B and c['N'] == N and c['mode'] == dc.BN_BATCH for c in dc.BN_CASES)
  assert dc.LARGE_MEAN_CASE in ids
  # er_dense.hip's host arithmetic, as the case comments state it
  assert dc.choose_chunks(3969, 1000) * dc.rows_per_chunk(3969, 1000) - dc.rows_per_chunk(3969, 1000) >= 3969  # empty last chunk
  assert dc.choose_chunks(8225, 5) > dc.K_INLINE_CHUNKS >= dc.choose_chunks(8192, 5)
  assert {dc.apply_tiles_per_block(c['B']) for c in dc.BN_CASES} == {1, 4, 16}
  for tpb in (4, 16):  # the 16-byte lanes (N % 4 == 0) and the scalar ones under several row tiles per workgroup
    ns = {c['N'] % 4 == 0 for c in dc.BN_CASES if dc.apply_tiles_per_block(c['B']) == tpb}
    assert ns == {True, False}, tpb
  t = dc.bn_inputs('bn-2048x64-train-relu-head0')
  assert abs(float(t['x'][:32].mean())) < 1.0 and float(t['x'][32:].min()) >= 999.0
  t = dc.bn_inputs('bn-33x5-train-relu-const')
  assert float(t['x'][:, 0].std()) == 0.0
  t = dc.bn_inputs('bn-33x65-train-relu-randn')
  assert float(t['gamma'][0]) == 0.0 and float(t['gamma'][1]) < 0
  y = dc.bn_forward_reference('bn-33x65-train-relu-randn')[0]['y']
  assert float(y[:, 2].max()) == 0.0  # every dy of column 2 is masked
  assert any(c['dy_wide'] for c in dc.BN_CASES) and dc.bn_inputs('bn-8192x5-train-relu-randn-dyld')['dy_wide']


def test_restated_host_arithmetic_is_the_librarys(built_lib):
  """choose_chunks / apply_tiles_per_block / gemm_row_tiles of _dense_cases.py against the library's own answers, on every
  case's shape and around every threshold (an ER_BN_TILES_MID setting or a changed constant shows here)."""
  from easyrec_amd import kernels
  lib = kernels.load_library(built_lib)
  shapes = {(c['B'], c['N']) for c in dc.BN_CASES} | {(c['B'], c['N']) for c in dc.DICE_CASES}
  shapes |= {(M, N) for M, _, N, _, _ in dc.STATS_FORM_CASES}
  shapes |= {(B, N) for B in (1, 31, 32, 33, 2048, 8191, 8192, 8193, 8224, 8225, 32768, 32769, 204800) for N in (1, 64, 65, 192, 193, 1000, 4096)}
  for B, N in sorted(shapes):
    assert lib.er_bn_row_chunks(B, N) == dc.choose_chunks(B, N), (B, N)
    assert lib.er_bn_apply_row_tiles(B) == dc.apply_tiles_per_block(B), B
    assert lib.er_gemm_row_tiles(B) == dc.gemm_row_tiles(B), B
  assert lib.er_bn_row_chunks(3969, 1000) == 64 and lib.er_bn_row_chunks(8225, 5) == 258


def test_emitted_statistics_cases_catch_a_naive_tile_variance():
  """Per 64-row tile records computed in float32 on the CPU and pooled exactly, as the GPU test pools the emitted ones: a
  two-pass M2 fits stats_reference's bound on every case; n (E[z^2] - mean^2) exceeds it on the small-M large-mean case
  of EVERY flavour (f32, staged bf16, bf16-NT) - and only there: with B in the thousands the bound's 2 d_mu mean(dev)
  term has grown past what the naive form loses."""
  caught = set()
  for M, K, N, kind, flavour in dc.STATS_FORM_CASES:
    a, w, bias = dc.stats_form_operands(M, K, N, kind)
    z = a @ w + bias
    ref, bound = dc.stats_reference(z)
    T = dc.gemm_row_tiles(M)
    case = dict(id='stats-%dx%dx%d-%s-%s' % (M, K, N, kind, dc.STATS_FLAVOUR[flavour]))
    n, mean, var = dc.pooled_stats(dc.naive_tile_stats(z, False), T, N)
    assert bool((n == M).all())
    check('f32', 'emitted_stats', case, dict(mean=mean, var=var), ref, bound, frac=0.5)
    _, mean, var = dc.pooled_stats(dc.naive_tile_stats(z, True), T, N)
    r = ratios(dict(mean=mean, var=var), ref, bound)
    print('RATIO who=naive op=emitted_stats case=%s tensor=var ratio=%.4g' % (case['id'], r['var']))
    if r['var'] > 1.0:
      caught.add((kind, flavour, M))
  for flavour in (False, 'staged', True):
    assert any(k == 'mean1000' and f == flavour and M <= 130 for k, f, M in caught), (flavour, sorted(map(str, caught)))
  assert not any(M >= 4096 for _, _, M in caught)  # (what the case list's comment says about the tall cases)


# ------------------------------------------------------------------------------------------------------------------
# planted mistakes: each backend below is wrong in one way, and its named case must fail
# ------------------------------------------------------------------------------------------------------------------
class _Fwd(RefBackend):
  """RefBackend's training forward with the pieces a mistake replaces."""

  def _var(self, z, mean):
    return ((z - mean)**2).mean(dim=0)

  def _invstd(self, var, eps):
    return 1.0 / torch.sqrt(var + eps)

  def _stats_input(self, x, z):
    return z

  def _moving(self, v, value, momentum):
    v.sub_((v - value) * (1.0 - momentum))

  def bn_act_fwd(self, x, bias, gamma, beta, use_bn, eps, momentum, moving_mean, moving_var, act):
    if use_bn != dc.BN_BATCH:
      return RefBackend.bn_act_fwd(self, x, bias, gamma, beta, use_bn, eps, momentum, moving_mean, moving_var, act)
    z = x if bias is None else x + bias
    s = self._stats_input(x, z)
    mean = s.mean(dim=0)
    var = self._var(s, mean)
    invstd = self._invstd(var, eps)
    y = (z - mean) * invstd
    y = y * (gamma if gamma is not None else 1.0) + (beta if beta is not None else 0.0)
    if moving_mean is not None:
      self._moving(moving_mean, mean, momentum)
      self._moving(moving_var, var, momentum)
    return (torch.relu(y) if act == dc.ACT_RELU else y), mean, invstd


@pytest.mark.parametrize('cid', [i for i in _BN_IDS if '-train-' in i])
def test_the_scaffold_of_the_planted_mistakes_is_sound(cid):
  """_Fwd without a mistake fits every bound on every batch-statistics case: a planted failure comes from the mistake."""
  assert not _bn_failing(_Fwd(), cid)


class _NaiveVariance(_Fwd):  # E[z^2] - mean^2 in float32
  def _var(self, z, mean):
    return (z * z).mean(dim=0) - mean * mean


class _UnbiasedVariance(_Fwd):
  def _var(self, z, mean):
    return ((z - mean)**2).sum(dim=0) / max(z.shape[0] - 1, 1)


class _EpsOutsideTheRoot(_Fwd):
  def _invstd(self, var, eps):
    return 1.0 / (torch.sqrt(var) + eps)


class _BiasLeftOutOfTheStatistics(_Fwd):
  def _stats_input(self, x, z):
    return x


class _MomentumSwapped(_Fwd):
  def _moving(self, v, value, momentum):
    v.sub_((v - value) * momentum)


class _MaskIncludesZero(RefBackend):
  def _bn_act_bwd(self, x, bias, gamma, y, mean, invstd, dy, use_bn, act, need_bias, need_affine):
    y2 = torch.where(y >= 0, torch.ones_like(y), -torch.ones_like(y)) if act == dc.ACT_RELU else y
    return RefBackend._bn_act_bwd(self, x, bias, gamma, y2, mean, invstd, dy, use_bn, act, need_bias, need_affine)


class _DxWithoutTheXhatTerm(RefBackend):
  def _bn_act_bwd(self, x, bias, gamma, y, mean, invstd, dy, use_bn, act, need_bias, need_affine):
    dx, dbias, dgamma, dbeta = RefBackend._bn_act_bwd(self, x, bias, gamma, y, mean, invstd, dy, use_bn, act, need_bias, need_affine)
    if use_bn == dc.BN_BATCH:
      g = dy * (y > 0).to(dy.dtype) if act == dc.ACT_RELU else dy
      dx = (gamma if gamma is not None else 1.0) * invstd * (g - g.sum(dim=0) / x.shape[0])
    return dx, dbias, dgamma, dbeta


class _DgammaTimesSigma(RefBackend):  # sum g (z - mean): the invstd factor of xhat is missing
  def _bn_act_bwd(self, x, bias, gamma, y, mean, invstd, dy, use_bn, act, need_bias, need_affine):
    dx, dbias, dgamma, dbeta = RefBackend._bn_act_bwd(self, x, bias, gamma, y, mean, invstd, dy, use_bn, act, need_bias, need_affine)
    return dx, dbias, (None if dgamma is None else dgamma / invstd), dbeta


class _FrozenUsesBatchStatistics(RefBackend):
  def bn_act_fwd(self, x, bias, gamma, beta, use_bn, eps, momentum, moving_mean, moving_var, act):
    if use_bn == dc.BN_FROZEN:
      return RefBackend.bn_act_fwd(self, x, bias, gamma, beta, dc.BN_BATCH, eps, momentum, None, None, act)
    return RefBackend.bn_act_fwd(self, x, bias, gamma, beta, use_bn, eps, momentum, moving_mean, moving_var, act)


class _DiceWithoutStatisticsGradient(RefBackend):
  def dice_bwd(self, x, alpha, mean, invstd, dy):
    xh = (x - mean) * invstd
    p = torch.sigmoid(xh)
    q = dy * x * (1.0 - alpha) * p * (1.0 - p)
    return dy * (alpha + (1.0 - alpha) * p) + invstd * q, (dy * (1.0 - p) * x).sum(dim=0)


class _DiceDalphaWithP(RefBackend):
  def dice_bwd(self, x, alpha, mean, invstd, dy):
    dx, _ = RefBackend.dice_bwd(self, x, alpha, mean, invstd, dy)
    p = torch.sigmoid((x - mean) * invstd)
    return dx, (dy * p * x).sum(dim=0)


def _bn_failing(be, cid):
  c, t = dc.bn_case(cid), dc.bn_inputs(cid)
  got = dc.run_bn(be, t, c['mode'], c['act'])
  want, bound = dc.bn_reference(cid, got['y'])
  return {k for k, v in ratios(got, want, bound).items() if not v <= 1.0}


def _dice_failing(be, cid):
  t, want, bound = dc.dice_reference(cid)
  return {k for k, v in ratios(dc.run_dice(be, t), want, bound).items() if not v <= 1.0}


def test_catches_float32_naive_variance_on_the_large_mean_case():
  assert dc.LARGE_MEAN_CASE == 'bn-33x5-train-relu-mean1000'
  assert {'save_invstd', 'mv'} <= _bn_failing(_NaiveVariance(), dc.LARGE_MEAN_CASE)
  assert 'save_invstd' in _bn_failing(_NaiveVariance(), 'bn-33x5-train-relu-bigbias')
  assert 'save_invstd' in _bn_failing(_NaiveVariance(), 'bn-2048x64-train-relu-mean1000')
  # ... and it is that case that tells: on ordinary data the naive form is as good as any
  assert not _bn_failing(_NaiveVariance(), 'bn-33x65-train-relu-randn')


def test_catches_variance_over_b_minus_one():
  assert {'save_invstd', 'mv', 'y'} <= _bn_failing(_UnbiasedVariance(), 'bn-33x65-train-relu-randn')


def test_catches_eps_outside_the_square_root():
  assert {'save_invstd', 'y'} <= _bn_failing(_EpsOutsideTheRoot(), 'bn-33x65-train-relu-randn')
  assert 'save_invstd' in _bn_failing(_EpsOutsideTheRoot(), 'bn-1x3-train-relu-randn-dyld')  # variance 0: r = 1 / sqrt(eps)


def test_catches_bias_left_out_of_the_statistics():
  assert {'save_mean', 'mm', 'y'} <= _bn_failing(_BiasLeftOutOfTheStatistics(), 'bn-33x5-train-relu-bigbias')


def test_catches_momentum_swapped():
  assert {'mm', 'mv'} <= _bn_failing(_MomentumSwapped(), 'bn-17x65-train-relu-randn')


def test_catches_mask_that_includes_zero():
  # column 2 is all zeros after the ReLU: y >= 0 lets its whole gradient through
  assert {'dx', 'dgamma', 'dbeta'} <= _bn_failing(_MaskIncludesZero(), 'bn-33x65-train-relu-randn')
  assert 'dbias' in _bn_failing(_MaskIncludesZero(), 'bn-33x130-none-relu-randn')


def test_catches_dx_without_the_xhat_term():
  assert 'dx' in _bn_failing(_DxWithoutTheXhatTerm(), 'bn-33x65-train-relu-randn')


def test_catches_dgamma_without_invstd():
  assert {'dgamma', 'acc_dgamma'} <= _bn_failing(_DgammaTimesSigma(), 'bn-33x65-train-relu-randn')


def test_catches_frozen_mode_normalising_by_batch_statistics():
  assert {'y', 'save_mean', 'save_invstd'} <= _bn_failing(_FrozenUsesBatchStatistics(), 'bn-17x65-frozen-relu-randn-dyld')


def test_catches_dice_without_its_gradient_through_the_statistics():
  assert 'dx' in _dice_failing(_DiceWithoutStatisticsGradient(), 'dice-17x65-randn')


def test_catches_dice_dalpha_with_p_for_one_minus_p():
  assert 'dalpha' in _dice_failing(_DiceDalphaWithP(), 'dice-17x65-randn')
