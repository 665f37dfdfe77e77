"""The interaction kernels' cases (tests/_interaction_cases.py) without a GPU:

  * a plain float32 torch evaluation of each formula, with float32 autograd, fits HALF of every derived bound: the
    bounds are attainable by an honest float32 implementation;
  * oracle.kernel_ref.RefBackend, the oracle every model-level test is measured against, fits every bound, forward
    and backward: its hand-derived backward passes are pinned to fp64 autograd of the formulas;
  * a RefBackend carrying one deliberate mistake fails the case meant to catch it: the cases have teeth.

tests/test_interaction_gpu.py runs the same cases through the HIP kernels.
"""
import pytest
import torch

from tests import _interaction_cases as ic
from oracle.kernel_ref import RefBackend

_IDS = ['%s' % c['id'] for _, c in ic.ALL_CASES]


@pytest.fixture(scope='module')
def ref():
  return RefBackend()


# ------------------------------------------------------------------------------------------------------------------
# plain float32 within half the bound; RefBackend within the bound
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('op,case', ic.ALL_CASES, ids=_IDS)
def test_plain_float32_fits_half_the_bound(op, case):
  _, want, bound = ic.reference(op, case['id'])
  ic.check('f32', op, case, ic.plain_f32(op, case['id']), want, bound, frac=0.5)


@pytest.mark.parametrize('op,case', ic.ALL_CASES, ids=_IDS)
def test_ref_backend_fits_the_bound(op, case, ref):
  _, want, bound = ic.reference(op, case['id'])
  ic.check('ref', op, case, ic.run(op, ref, case['id']), want, bound)


def _cross_v2_all(who, be, case, frac, dev='cpu'):
  inp = ic.cross_v2_inputs_of(case['id'])
  worst = {}
  for variant in ic.cross_v2_variants():
    want, bound = ic.cross_v2_reference(case['id'], variant)
    if be is None:
      got = ic.cross_v2_formula(case, inp, ic.F32, variant)
    else:
      got = ic.run_cross_v2(be, case, inp, dev, variant)
    tag = dict(case, id='%s-diag%g-bias%d-dx%d-acc0%d-accx%d' % ((case['id'],) + variant))
    for k, v in ic.check(who, 'cross_v2', tag, got, want, bound, frac).items():
      worst[k] = max(worst.get(k, 0.0), v)
  for diag in ic.CROSS_V2_DIAGS:
    for has_bias in (True, False):
      want, bound = ic.cross_v2_plain_reference(case['id'], diag, has_bias)
      if be is None:
        got = ic.cross_v2_plain_formula(case, inp, ic.F32, diag, has_bias)
      else:
        got = ic.run_cross_v2_plain(be, case, inp, dev, diag, has_bias)
      ic.check(who, 'cross_v2', dict(case, id='%s-plain-diag%g-bias%d' % (case['id'], diag, has_bias)), got, want, bound, frac)
  return worst


@pytest.mark.parametrize('case', ic.CROSS_V2_CASES, ids=[c['id'] for c in ic.CROSS_V2_CASES])
def test_cross_v2_plain_float32_fits_half_the_bound(case):
  _cross_v2_all('f32', None, case, 0.5)


@pytest.mark.parametrize('case', ic.CROSS_V2_CASES, ids=[c['id'] for c in ic.CROSS_V2_CASES])
def test_cross_v2_ref_backend_fits_the_bound(case, ref):
  _cross_v2_all('ref', ref, case, 1.0)


def test_case_lists_cover_what_they_claim():
  """The properties the case comments rely on, as host arithmetic."""
  for c in ic.DIN_CASES:
    assert ic.din_fast_expected(c) == (c['path'] == 'fast'), c['id']
    sl = ic.reference('din', c['id'])[0]['seq_len'].tolist()
    assert {0, 1, c['L']} <= set(sl), c['id']
  assert any(c['E'] // 4 == 64 for c in ic.DIN_CASES) and any(c['E'] > 64 and c['path'] == 'general' for c in ic.DIN_CASES)
  assert {(c['B'], c['d'], c['L']) for c in ic.CROSS_V1_CASES} >= {(1100, 70, 2), (3, 1024, 2), (3, 1024, 9), (2, 1024, 20),
                                                                   (5, 17, 1)}
  assert 2 * 9 * 1024 * 4 > 64 * 1024 and 2 * 20 * 1024 * 4 == 160 * 1024 and 2 * 20481 * 4 > 160 * 1024
  assert any(ic.fm_vec_expected(c) and c['layout'] == 'wide' for c in ic.FM_CASES)
  assert any(ic.cross_v2_vec_expected(c) for c in ic.CROSS_V2_CASES)
  z = ic.reference('ce', 'ce-300-w')[0]['z'].tolist()
  assert all(any(abs(v - s) < 1e-7 * max(1.0, abs(s)) for v in z) for s in ic.CE_SPECIAL)
  _cin_claims()
  _dot_claims()


def _cin_claims():
  cases = ic.CIN_CASES
  K = [c['H'] * c['H0'] for c in cases]
  blk = ic.CIN_BLOCK
  assert any(k < blk for k in K) and blk in K and any(blk < k < 2 * blk and k % blk for k in K)
  assert any(c['H'] > blk for c in cases) and any(c['H0'] > blk for c in cases)
  assert any(c['D'] == 1 for c in cases) and any(c['H0'] == 1 for c in cases) and any(c['N'] == 1 for c in cases)
  assert all(c['B'] <= 7 for c in cases)
  # both forms; the later one written and added to, at every shape; the first one aliased and adding, H == H0
  later = {(c['B'], c['H'], c['H0'], c['D'], c['N']): set() for c in cases if c['form'] == 'later'}
  for c in cases:
    if c['form'] == 'later':
      later[(c['B'], c['H'], c['H0'], c['D'], c['N'])].add(c['add_xi'])
      assert ic.cin_strides(c) == (c['D'] * c['H'], 1, c['H'])
    else:
      assert c['add_xi'] == 1 and c['H'] == c['H0'] and ic.cin_strides(c) == (c['H0'] * c['D'], c['D'], 1)
  assert later and all(v == {0, 1} for v in later.values())
  assert {(c['H'], c['H0']) for c in cases if c['form'] == 'first'} >= {(16, 16)}
  assert {(c['H'], c['H0']) for c in cases if c['form'] == 'later'} >= {(3, 2), (16, 16), (17, 16), (300, 2), (2, 300), (122, 123)}
  # the two act_pool kernels: below a block, straddling one; every dnext form; strided pooled / dpooled with neighbours
  assert any(c['B'] * c['D'] * c['N'] < blk for c in cases)
  assert any(c['B'] * c['N'] > blk and (c['B'] * c['N']) % blk for c in cases)
  assert {c['dnext'] for c in cases} == {'none', 'present', 'alias'}
  assert any(c['col0'] > 0 and c['ld'] > c['col0'] + c['N'] for c in cases) and any(c['ld'] == c['N'] for c in cases)
  # LDS: an admitted case within 1 KiB of the budget, with B * D = 2
  big = [c for c in cases if ic.CIN_LDS_BUDGET - 1024 < ic.cin_outer_bwd_lds(c['H'], c['H0'])]
  assert big and all(ic.cin_outer_bwd_lds(c['H'], c['H0']) <= ic.CIN_LDS_BUDGET for c in cases)
  assert all(c['B'] * c['D'] == 2 for c in big)
  # the planted ties: c == -bias exactly and one float32 above, both under a non-zero incoming gradient
  for c in cases:
    inp, want, _ = ic.reference('cin', c['id'])
    (r0, n0), (r1, n1) = ic.cin_ties(c)
    assert inp['c'][r0, n0] == -inp['bias'][n0] and want['fm'][r0, n0] == 0 and want['dc'][r0, n0] == 0
    assert inp['c'][r1, n1] > -inp['bias'][n1] and want['fm'][r1, n1] > 0
    assert inp['c'][r1, n1] == torch.nextafter(-inp['bias'][n1], torch.tensor(float('inf')))
    for r, n in ((r0, n0), (r1, n1)):
      g = inp['dpooled'][r // c['D'], c['col0'] + n] + (0 if c['dnext'] == 'none' else inp['dnext'][r, n])
      assert g != 0
    assert want['dc'][r1, n1] != 0
    assert torch.equal(inp['fm32'].to(ic.F64) > 0, want['fm'] > 0)  # the mask: the same in float32 and float64
  # refused: truly over the limit, by the arithmetic of the ER_REQUIRE lines
  lds, alias, cols = ic.CIN_REFUSED
  assert ic.cin_outer_bwd_lds(lds['H'], lds['H0']) > ic.CIN_LDS_BUDGET >= ic.cin_outer_bwd_lds(lds['H'] - 1, lds['H0'])
  assert alias['form'] == 'first' and not alias['add_xi'] and ic.cin_outer_bwd_lds(alias['H'], alias['H0']) <= ic.CIN_LDS_BUDGET
  assert cols['H'] * cols['H0'] >= 1 << 24 and cols['B'] * cols['D'] < 0x7FFFFFFF


def _dot_claims():
  cases, ref = ic.DOT_CASES, RefBackend()
  blk = ic.CIN_BLOCK
  full = [c for c in cases if not c['fwd_only']]
  assert {(c['B'], c['F'], c['D']) for c in full} == set(ic.DOT_SHAPES) >= {(5, 2, 3), (3, 9, 1), (4, 27, 16), (1, 40, 8)}
  for shape in ic.DOT_SHAPES:
    assert {(c['si'], c['layout']) for c in full if (c['B'], c['F'], c['D']) == shape} == \
        {(si, lay) for si in (False, True) for lay in ('contig', 'wide')}
  assert any(ic.dot_pairs(c['F'], c['si']) > blk and c['F'] * c['D'] > blk for c in full)
  assert all(ic.dot_bwd_lds(c['F'], c['D'], c['si']) <= ic.DOT_LDS_BUDGET for c in full)
  for c in full:  # the wide layouts: every base off a 16-byte boundary, no row stride a multiple of 4 floats
    seen = {}
    ic.run('dot', ref, c['id'], 'cpu', seen)
    n, P = c['F'] * c['D'], ic.dot_pairs(c['F'], c['si'])
    if c['layout'] == 'wide':
      assert all(p % 16 for p in seen['ptrs']) and all(s % 4 for s in seen['strides']), c['id']
      assert all(s > w + ic.DOT_OFF for s, w in zip(seen['strides'], (n, P, P, n))), c['id']  # neighbours on both sides
    else:
      assert seen['strides'] == [n, P, P, n] or c['B'] == 1, c['id']
  # the forward runs where the backward is refused: F = 128, D = 64
  only, = [c for c in cases if c['fwd_only']]
  assert (only['B'], only['F'], only['D'], only['si']) == (1, 128, 64, False)
  assert ic.dot_fwd_lds(128, 64) <= ic.DOT_LDS_BUDGET < ic.dot_bwd_lds(128, 64, False)
  # refused: truly over the limit, by the arithmetic of the ER_REQUIRE lines
  by = {c['what']: c for c in ic.DOT_REFUSED}
  assert set(by) == {'fwd_lds', 'bwd_lds', 'out_stride', 'g_stride'}
  assert ic.dot_fwd_lds(by['fwd_lds']['F'], by['fwd_lds']['D']) > ic.DOT_LDS_BUDGET
  c = by['bwd_lds']
  assert ic.dot_bwd_lds(c['F'], c['D'], c['si']) > ic.DOT_LDS_BUDGET >= ic.dot_fwd_lds(c['F'], c['D'])
  for k in ('out_stride', 'g_stride'):  # everything but the stride is admissible
    c = by[k]
    assert c['F'] > 1 and ic.dot_pairs(c['F'], c['si']) > 1 and ic.dot_bwd_lds(c['F'], c['D'], c['si']) <= ic.DOT_LDS_BUDGET


# ------------------------------------------------------------------------------------------------------------------
# planted mistakes: each RefBackend subclass below is wrong in one way, and its case must fail
# ------------------------------------------------------------------------------------------------------------------
def _mask(L, seq_len):
  return torch.arange(L)[None, :] < seq_len[:, None].to(torch.int64)


class _ScaleDroppedFromDscores(RefBackend):
  def din_pool_bwd(self, probs, hist, seq_len, dout, scale=1.0, dhist=None, acc_h=False):
    return RefBackend.din_pool_bwd(self, probs, hist, seq_len, dout, 1.0, dhist, acc_h)


class _MaskNotAppliedToDscores(RefBackend):
  def din_pool_bwd(self, probs, hist, seq_len, dout, scale=1.0, dhist=None, acc_h=False):
    full = torch.full_like(seq_len, hist.shape[1])
    return RefBackend.din_pool_bwd(self, probs, hist, full, dout, scale, dhist, acc_h)


class _PadIsMinusInfinity(RefBackend):
  def din_pool_fwd(self, scores, hist, seq_len, scale=1.0):
    s = torch.where(_mask(hist.shape[1], seq_len), scores * scale, torch.full_like(scores, float('-inf')))
    p = torch.softmax(s, dim=1)
    return torch.bmm(p[:, None, :], hist)[:, 0, :], p


class _ConcatSignFlipped(RefBackend):
  def din_concat_bwd(self, q, h, dout, dh=None, acc_h=False):
    E = h.shape[2]
    flipped = dout.clone()
    flipped[..., E:2 * E], flipped[..., 2 * E:3 * E] = dout[..., 2 * E:3 * E], dout[..., E:2 * E]  # g2 - g1
    dq, _ = RefBackend.din_concat_bwd(self, q, h, dout)
    _, r = RefBackend.din_concat_bwd(self, q, h, flipped, dh, acc_h)
    return dq, r


class _AccumulateIgnored(RefBackend):
  @staticmethod
  def _into(val, into, accumulate):
    return RefBackend._into(val, into, False)


class _AccHIgnored(RefBackend):
  def din_concat_bwd(self, q, h, dout, dh=None, acc_h=False):
    return RefBackend.din_concat_bwd(self, q, h, dout, dh, False)

  def din_pool_bwd(self, probs, hist, seq_len, dout, scale=1.0, dhist=None, acc_h=False):
    return RefBackend.din_pool_bwd(self, probs, hist, seq_len, dout, scale, dhist, False)


class _DiagTermDroppedFromDx(RefBackend):
  def cross_v2_bwd(self, x0, x, u, bias, diag_scale, dout):
    g0, _, du = RefBackend.cross_v2_bwd(self, x0, x, u, bias, diag_scale, dout)
    return g0, dout.clone(), du


class _DxNotJoinedIntoDx0(RefBackend):
  def cross_v2_bwd_acc(self, x0, x, u, bias, diag_scale, dout, dx0, acc0, dx, accx):
    if dx is None:
      dx = torch.empty_like(x0)
    return RefBackend.cross_v2_bwd_acc(self, x0, x, u, bias, diag_scale, dout, dx0, acc0, dx, 0)


class _XStrideTakenAsFD(RefBackend):
  @staticmethod
  def _packed(x, n):  # rows read n apart from the view's first element, whatever the row pitch
    return x.as_strided((x.shape[0], n), (n, 1), x.storage_offset())

  def fm_fwd(self, x, F, D):
    return RefBackend.fm_fwd(self, self._packed(x, F * D), F, D)

  def rowsum_fwd(self, x, n):
    return RefBackend.rowsum_fwd(self, self._packed(x, n), n)

  def dot_interaction_fwd(self, x, F, D, self_interaction, out=None):
    return RefBackend.dot_interaction_fwd(self, self._packed(x, F * D), F, D, self_interaction, out)

  def dot_interaction_bwd(self, x, g, F, D, self_interaction, into=None, accumulate=False):
    return RefBackend.dot_interaction_bwd(self, self._packed(x, F * D), g, F, D, self_interaction, into, accumulate)


class _CinColumnIndexSwapped(RefBackend):
  def cin_outer_fwd(self, xi, strides, H, x0, z):  # column m * H + h
    B, H0, D = x0.shape
    RefBackend.cin_outer_fwd(self, xi, strides, H, x0, z)
    z.copy_(z.reshape(B * D, H, H0).transpose(1, 2).reshape(B * D, H0 * H))


class _CinCol0Ignored(RefBackend):
  def cin_act_pool_fwd(self, c, bias, B, D, pooled, col0):
    RefBackend.cin_act_pool_fwd(self, c, bias, B, D, pooled, 0)


class _CinDnextDropped(RefBackend):
  def cin_act_pool_bwd(self, fm, dpooled, col0, dnext, B, D, dc):
    RefBackend.cin_act_pool_bwd(self, fm, dpooled, col0, None, B, D, dc)


class _CinAddXiIgnored(RefBackend):
  def cin_outer_bwd(self, dz, xi, strides, H, x0, dxi, add_xi, dx0):
    RefBackend.cin_outer_bwd(self, dz, xi, strides, H, x0, dxi, False, dx0)


class _CinLaterStridesAsFirst(RefBackend):
  @staticmethod
  def _cin_view(x, strides, B, H, D):
    return torch.as_strided(x, (B, H, D), (H * D, D, 1))


class _CinMaskIncludesZero(RefBackend):
  def cin_act_pool_bwd(self, fm, dpooled, col0, dnext, B, D, dc):  # fm >= 0 in place of fm > 0
    N = fm.shape[1]
    g = dpooled[:, col0:col0 + N][:, None, :].expand(B, D, N).reshape(B * D, N)
    g = g if dnext is None else g + dnext
    dc.copy_(torch.where(fm >= 0, g, torch.zeros_like(g)))


class _CinAliasedDx0TermDropped(RefBackend):
  def cin_outer_bwd(self, dz, xi, strides, H, x0, dxi, add_xi, dx0):
    if dxi is not dx0:
      return RefBackend.cin_outer_bwd(self, dz, xi, strides, H, x0, dxi, add_xi, dx0)
    RefBackend.cin_outer_bwd(self, dz, xi, strides, H, x0, dxi, add_xi, torch.zeros_like(dx0))  # the dx0 term goes nowhere


class _DotPairsByColumn(RefBackend):
  @staticmethod
  def _dot_pairs(F, self_interaction):
    return sorted(RefBackend._dot_pairs(F, self_interaction), key=lambda p: (p[1], p[0]))


class _DotSelfTermOnce(RefBackend):
  def dot_interaction_bwd(self, x, g, F, D, self_interaction, into=None, accumulate=False):
    e = x[:, :F * D].reshape(x.shape[0], F, D)
    de = torch.zeros_like(e)
    for p, (i, j) in enumerate(self._dot_pairs(F, self_interaction)):
      de[:, i] += g[:, p:p + 1] * e[:, j]
      if i != j:
        de[:, j] += g[:, p:p + 1] * e[:, i]
    return self._into(de.reshape(x.shape[0], F * D), into, accumulate)


class _GateLeftOutOfDotg(RefBackend):
  def mmoe_mix_bwd(self, experts, gates, dout):
    dexperts, _ = RefBackend.mmoe_mix_bwd(self, experts, gates, dout)
    dg = torch.einsum('tbh,ebh->tbe', dout, experts)
    dotg = (gates[..., 1:] * dg[..., 1:]).sum(dim=-1, keepdim=True)  # gate 0 is missing from the sum
    return dexperts, gates * (dg - dotg)


class _OneOperandInBf16(RefBackend):
  def fm_fwd(self, x, F, D):
    e = x[:, :F * D].reshape(x.shape[0], F, D)
    S = e.sum(dim=1)
    q = (e.to(torch.bfloat16).to(torch.float32) * e).sum(dim=1)  # one operand of e * e rounded to bfloat16
    return 0.5 * (S * S - q), S


def _failing(op, be, cid):
  """The tensors of a case on which `be` exceeds the bound."""
  _, want, bound = ic.reference(op, cid)
  return {k for k, v in ic.ratios(ic.run(op, be, cid), want, bound).items() if not v <= 1.0}


def _cross_v2_failing(be, cid, variant):
  case, inp = ic.case_by_id('cross_v2', cid), ic.cross_v2_inputs_of(cid)
  want, bound = ic.cross_v2_reference(cid, variant)
  return {k for k, v in ic.ratios(ic.run_cross_v2(be, case, inp, 'cpu', variant), want, bound).items() if not v <= 1.0}


def test_catches_scale_dropped_from_dscores():
  assert 'dscores' in _failing('din', _ScaleDroppedFromDscores(), 'din-33x50x32-fast-sE')


def test_catches_mask_not_applied_to_dscores():
  # only the seq_len == 0 row can show it: elsewhere the masked probabilities are exactly zero
  assert 'dscores' in _failing('din', _MaskNotAppliedToDscores(), 'din-33x50x32-fast-s1')


def test_catches_minus_infinity_pad_in_an_empty_history():
  assert {'probs', 'out'} <= _failing('din', _PadIsMinusInfinity(), 'din-5x13x12-general-s1')


def test_catches_sign_flip_in_concat_backward():
  assert {'dh', 'dh_fresh', 'dh_acc'} <= _failing('din', _ConcatSignFlipped(), 'din-4x70x8-general-s1')


def test_catches_accumulate_ignored():
  assert {'acc_fm', 'acc_rs'} <= _failing('fm', _AccumulateIgnored(), 'fm-7x3x5-wide')


def test_catches_acc_h_ignored():
  assert {'dh_acc', 'dhist_acc'} <= _failing('din', _AccHIgnored(), 'din-9x1x16-fast-s1')


def test_catches_diag_term_dropped_from_cross_v2_dx():
  v = (ic.CROSS_V2_DIAGS[1], True, True, 0, 0)
  assert 'dx' in _cross_v2_failing(_DiagTermDroppedFromDx(), 'v2-9x3-contig', v)
  assert 'dx0' in _cross_v2_failing(_DiagTermDroppedFromDx(), 'v2-9x3-contig', (v[0], True, False, 0, 0))


def test_catches_dx_not_joined_into_dx0():
  assert 'dx0' in _cross_v2_failing(_DxNotJoinedIntoDx0(), 'v2-77x130-ld4', (0.0, True, False, 1, 0))


def test_catches_x_stride_taken_as_fd():
  assert {'fm', 'S', 'rowsum'} <= _failing('fm', _XStrideTakenAsFD(), 'fm-513x39x16-wide')


def test_catches_gate_left_out_of_dotg():
  assert 'dlogits' in _failing('mmoe', _GateLeftOutOfDotg(), 'mmoe-2x4x65x33')


def test_catches_one_operand_rounded_to_bfloat16():
  # the bounds resolve float32-level error: a bfloat16 operand (2**-9 relative) in ONE of the products is 2**15 U
  assert 'fm' in _failing('fm', _OneOperandInBf16(), 'fm-513x39x16-contig')
  assert 'fm' in _failing('fm', _OneOperandInBf16(), 'fm-64x8x64-contig-offset100')


_CIN_SMALL = 'cin-later-3x3x2x4x5-col2of10-present-add%d'


def test_catches_cin_column_index_swapped():
  assert 'z' in _failing('cin', _CinColumnIndexSwapped(), 'cin-later-2x17x16x2x3-col1of6-alias-add0')
  assert 'z' in _failing('cin', _CinColumnIndexSwapped(), 'cin-later-2x16x16x3x7-col0of7-none-add0')  # H == H0: a permutation
  # xi IS x0 in the first form: z is symmetric in (h, m), and only the later form can tell
  assert not _failing('cin', _CinColumnIndexSwapped(), 'cin-first-2x16x16x3x2-col1of4-present-add1')


def test_catches_cin_col0_ignored():
  assert 'pooled' in _failing('cin', _CinCol0Ignored(), _CIN_SMALL % 0)


def test_catches_cin_dnext_dropped():
  assert 'dc' in _failing('cin', _CinDnextDropped(), _CIN_SMALL % 0)
  assert 'dc' in _failing('cin', _CinDnextDropped(), 'cin-later-2x17x16x2x3-col1of6-alias-add0')


def test_catches_cin_add_xi_ignored():
  assert 'dxi' in _failing('cin', _CinAddXiIgnored(), _CIN_SMALL % 1)
  assert not _failing('cin', _CinAddXiIgnored(), _CIN_SMALL % 0)  # which is why both values are cases


def test_catches_cin_later_strides_taken_as_first():
  assert {'z', 'dxi', 'dx0'} <= _failing('cin', _CinLaterStridesAsFirst(), _CIN_SMALL % 0)


def test_catches_cin_mask_that_includes_zero():
  # on a ReLU output fm >= 0 is everything: the masked elements fail, and among them the planted tie itself
  cid = 'cin-later-2x16x16x3x7-col0of7-none-add0'
  assert 'dc' in _failing('cin', _CinMaskIncludesZero(), cid)
  (r0, n0), (r1, n1) = ic.cin_ties(ic.case_by_id('cin', cid))
  got, want = ic.run('cin', _CinMaskIncludesZero(), cid)['dc'], ic.reference('cin', cid)[1]['dc']
  assert got[r0, n0] != 0 and want[r0, n0] == 0 and got[r1, n1] == want[r1, n1] != 0


def test_catches_cin_aliased_dx0_term_dropped():
  assert 'dx0' in _failing('cin', _CinAliasedDx0TermDropped(), 'cin-first-3x3x3x2x4-col0of4-alias-add1')
  assert not _failing('cin', _CinAliasedDx0TermDropped(), _CIN_SMALL % 1)


def test_catches_dot_pairs_walked_by_column():
  assert {'out', 'dx'} <= _failing('dot', _DotPairsByColumn(), 'dot-3x9x1-si0-contig')
  assert not _failing('dot', _DotPairsByColumn(), 'dot-5x2x3-si0-contig')  # one pair: F = 2 cannot show it


def test_catches_dot_self_term_counted_once():
  assert _failing('dot', _DotSelfTermOnce(), 'dot-3x9x1-si1-contig') == {'dx', 'dx_acc'}
  assert not _failing('dot', _DotSelfTermOnce(), 'dot-3x9x1-si0-contig')


def test_catches_dot_accumulate_ignored():
  assert _failing('dot', _AccumulateIgnored(), 'dot-5x2x3-si0-wide') == {'dx_acc'}


def test_catches_dot_x_stride_taken_as_fd():
  assert {'out', 'dx', 'dx_acc'} <= _failing('dot', _XStrideTakenAsFD(), 'dot-4x27x16-si0-wide')
  assert not _failing('dot', _XStrideTakenAsFD(), 'dot-4x27x16-si0-contig')
