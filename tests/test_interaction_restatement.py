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
