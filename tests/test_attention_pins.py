"""The bars and preconditions of tests/test_attention_edges_gpu.py, held without a GPU (cases: tests/_attention_cases.py).

Every case is evaluated in plain fp32 torch on the CPU - the product's composition attention_compose for er_mha_*, the
AutoInt oracle at torch.float32 - and compared with the fp64 reference by close's measure (max error over max value);
each figure is printed.  A (case, tensor) without a record in MHA_BARS / AI_BARS must measure at or below one third of
its default bar (1e-5 forward, 1e-4 gradients); a recorded bar must be 4 x its recorded measurement, and today's
measurement must lie within a factor 2 of the record.  Also here: the saturated cases' largest score and the gap
between the two best scores of every row, "P = 1 exactly" where a case relies on it, and the Python envelope
predicates against the closed forms of include/easyrec_hip.h (K8f, K8c) with the figures the case tables quote."""
import pytest
import torch

from easyrec_amd.layers import multihead_attention as mha
from easyrec_amd.layers import multihead_cross_attention as mca
from tests import _attention_cases as ac


def _held(tag, tensor, err, default, record):
  """-> None, or what is wrong with the bar of (tag, tensor) given its plain fp32 error `err`."""
  if record is None:
    return None if err <= default / 3 else '%s %s: fp32 error %.3g above a third of %g and no bar of its own' % (tag, tensor, err, default)
  measured, bar = record
  if abs(bar - 4 * measured) > 1e-12 * bar:
    return '%s %s: the bar %g is not 4 x the recorded %g' % (tag, tensor, bar, measured)
  if measured <= default / 3:
    return '%s %s: the recorded %g needs no bar of its own' % (tag, tensor, measured)
  if not measured / 2 <= err <= 2 * measured:
    return '%s %s: measured %.3g, recorded %g' % (tag, tensor, err, measured)
  return None


@pytest.mark.parametrize('tag,masked', ac.MHA_RUNS, ids=ac.mha_run_id)
def test_mha_plain_fp32_sits_within_a_third_of_each_bar_or_the_bar_is_recorded(tag, masked):
  want = ac.mha_reference(tag, masked)
  got = ac.mha_eval(tag, masked, ac.F32, mca.attention_compose)
  bad = []
  for t in ac.MHA_TENSORS:
    exact_zero = float(want[t].abs().max()) == 0.0
    err = ac.measure(got[t], want[t], floor=1.0 if exact_zero else 1e-30)
    default = ac.FWD_BAR if t == 'ctx' else ac.GRAD_BAR
    print('PIN op=mha case=%s masked=%d tensor=%s fp32_vs_fp64=%.3g bar=%g' % (tag, masked, t, err, ac.mha_bar(tag, masked, t)))
    bad.append(_held(tag, t, err, default, ac.MHA_BARS.get((tag, masked, t))))
  assert not [b for b in bad if b], bad


@pytest.mark.parametrize('tag', sorted(ac.AI_CASES))
def test_autoint_plain_fp32_sits_within_a_third_of_each_bar_or_the_bar_is_recorded(tag):
  worst = dict.fromkeys(ac.AI_TENSORS, 0.0)
  for B in ac.ai_batches(tag):
    y32 = ac.ai_eval(tag, B, ac.F32)['y']
    pattern = (y32 > 0).to(ac.F64)  # (the gradient through the fp32 evaluation's own ReLU pattern, as on the GPU)
    got, want = ac.ai_eval(tag, B, ac.F32, pattern), ac.ai_eval(tag, B, ac.F64, pattern)
    for t in ac.AI_TENSORS:
      exact_zero = float(want[t].abs().max()) == 0.0
      worst[t] = max(worst[t], ac.measure(got[t], want[t], floor=1.0 if exact_zero else 1e-30))
  bad = []
  for t in ac.AI_TENSORS:
    print('PIN op=autoint case=%s tensor=%s fp32_vs_fp64=%.3g bar=%g' % (tag, t, worst[t], ac.ai_bar(tag, t)))
    bad.append(_held(tag, t, worst[t], ac.FWD_BAR if t == 'y' else ac.GRAD_BAR, ac.AI_BARS.get((tag, t))))
  assert not [b for b in bad if b], bad


def test_no_bar_is_recorded_for_a_case_that_does_not_exist():
  assert all(tag in ac.MHA_ALL and t in ac.MHA_TENSORS for tag, _, t in ac.MHA_BARS)
  assert all(tag in ac.AI_CASES and t in ac.AI_TENSORS for tag, t in ac.AI_BARS)


# ------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize('tag', sorted(ac.MHA_SAT_CASES))
def test_mha_saturated_rows_reach_their_score_and_have_no_near_tie(tag):
  top, gap = ac.mha_top_gap(tag)
  print('PIN op=mha case=%s top=%.6g min_gap=%.3g' % (tag, top, gap))
  assert abs(top - ac.MHA_SAT_CASES[tag]['top']) <= 1e-4 * top and gap > ac.SAT_MIN_GAP
  p = torch.softmax(ac.mha_scores(*[ac.mha_inputs(tag, False)[n] for n in ('q', 'k')], ac.mha_inputs(tag, False)['B'],
                                  *[ac.MHA_SAT_CASES[tag][n] for n in ('F', 'T', 'H', 'ds')]), dim=-1)
  assert float(p.max()) > 0.9999  # (nearly one-hot rows are among them)


def test_autoint_saturated_rows_reach_their_score_and_have_no_near_tie():
  for B in ac.ai_batches('d128_top80'):
    top, gap = ac.ai_top_gap('d128_top80', B)
    print('PIN op=autoint case=d128_top80 B=%d top=%.6g min_gap=%.3g' % (B, top, gap))
    assert abs(top - 80.0) <= 1e-4 * top and gap > ac.SAT_MIN_GAP
  for tag in ('d128', 'mid', 'f60', 'f89'):  # (the others stay O(1) .. O(10): nothing saturates by accident)
    assert ac.ai_top_gap(tag, 3)[0] < 20.0, tag


def test_one_key_gives_p_equal_one_exactly():
  """f4096_t1, masked or not (T = 1: the only key is the row's largest adder whatever its mask): ctx is V's row and
  dQ = dK = 0 in fp64 and in plain fp32 alike.  AutoInt f1: dQ = dK = 0 and y = relu(V + R)."""
  c = ac.MHA_CASES['f4096_t1']
  assert c['T'] == 1
  for masked in (False, True):
    inp = ac.mha_inputs('f4096_t1', masked)
    rows = inp['v'].view(inp['B'], 1, -1).expand(inp['B'], c['F'], c['H'] * c['ds']).reshape(inp['B'] * c['F'], -1)
    for res, dt in ((ac.mha_reference('f4096_t1', masked), ac.F64),
                    (ac.mha_eval('f4096_t1', masked, ac.F32, mca.attention_compose), ac.F32)):
      assert torch.equal(res['ctx'], rows.to(dt)) and not res['dq'].any() and not res['dk'].any()
  a = ac.AI_CASES['f1']
  d = a['H'] * a['ds']
  for B in ac.ai_batches('f1'):
    g = ac.ai_inputs('f1', B)['g']
    for dt in (ac.F64, ac.F32):
      y = ac.ai_eval('f1', B, dt)['y']
      res = ac.ai_eval('f1', B, dt, (y > 0).to(dt))
      assert torch.equal(y, torch.relu(g[:, 2 * d:3 * d].to(dt) + g[:, 3 * d:].to(dt)))
      assert not res['dq'].any() and not res['dk'].any()


def test_the_masks_special_examples():
  """A masked run with more than one round of keys: example 0 one open key, 1 none, 2 only the last key, 3 only j = 64."""
  for tag, c in ac.MHA_CASES.items():
    m = ac.mha_inputs(tag, True)['mask']
    assert m.dtype == torch.int32 and m.shape == (ac.mha_batch(tag, True), c['T'])
    assert int(m[0].sum()) == 1 and int(m[1].sum()) == 0
    if c['T'] > ac.WAVE:
      assert m.shape[0] >= 4 and m[2].nonzero().flatten().tolist() == [c['T'] - 1]
      assert m[3].nonzero().flatten().tolist() == [ac.WAVE]
  assert {t for t, c in ac.MHA_CASES.items() if c['T'] > ac.WAVE} == {'t200_f1', 't70_f70', 't4095_f1'}


# ------------------------------------------------------------------------------------------------ envelopes
def test_mha_predicates_match_the_headers_closed_forms():
  for F, T, ds in ac.MHA_GRID_SHAPES:
    for bwd in (True, False):
      assert mca.lds_bytes(F, T, ds, bwd) == ac.mha_bytes(F, T, ds, bwd), (F, T, ds, bwd)
    assert mca.fits(F, T, ds) == ac.mha_inside(F, T, ds), (F, T, ds)
    assert mca.mha_group_units(F, T, ds) == ac.mha_units(F, T, ds), (F, T, ds)
  assert (mca.LDS_BUDGET, mca.MAX_SEQ_LEN, mca.MAX_HEAD_SIZE) == (ac.MHA_BUDGET, ac.MHA_MAX_LEN, ac.MHA_MAX_DS)
  # both sides of every edge
  for inside, outside in (((34, 34, 128), (35, 35, 128)), ((1, 4095, 1), (1, 4096, 1)), ((4096, 1, 1), (4097, 1, 1)),
                          ((1, 1, 128), (1, 1, 129)), ((4096, 1, 1), (4096, 1, 2))):
    assert mca.fits(*inside) and not mca.fits(*outside), (inside, outside)
  assert mca.lds_bytes(4097, 1, 1) <= mca.LDS_BUDGET  # (the length bound decides there, not the bytes)
  assert mca.lds_bytes(35, 35, 128) == ac.MHA_OUTSIDE['bytes'] > mca.LDS_BUDGET


def test_mha_cases_quote_their_bytes_and_units():
  for tag, c in ac.MHA_CASES.items():
    assert mca.lds_bytes(c['F'], c['T'], c['ds']) == c['bytes'], tag
    assert mca.mha_group_units(c['F'], c['T'], c['ds']) == c['G'], tag
  for c in ac.MHA_SAT_CASES.values():
    assert mca.fits(c['F'], c['T'], c['ds'])
  assert {c['G'] for c in ac.MHA_CASES.values()} == {1, 2, 4, 8}
  c = ac.MHA_CASES
  # what each tag is named for
  assert c['t200_f1']['T'] % ac.WAVE != 0 and c['t200_f1']['T'] > 3 * ac.WAVE
  assert c['f130_t3']['F'] > ac.WAVE and c['f130_t3']['G'] == 8           # one wave per unit: the row loop strides by 1
  assert c['f4096_t1']['F'] > 8 * ac.WAVE                                 # eight waves: more than 64 rows each
  assert -(-c['t4095_f1']['T'] // ac.WAVE) == 64 and not mca.fits(1, c['t4095_f1']['T'] + 1, 1)
  assert not mca.fits(35, 35, 128) and c['edge_ds128']['ds'] == mca.MAX_HEAD_SIZE
  assert (c['m_rem2']['F'] % 4, c['m_rem2']['T'] % 4, c['m_rem3']['F'] % 4, c['m_rem3']['T'] % 4) == (2, 3, 3, 2)
  assert all(c[t][n] > 4 for t in ('m_rem2', 'm_rem3') for n in ('F', 'T'))


def test_autoint_predicates_match_the_headers_closed_form_and_the_cases_their_epb():
  for F, H, ds in ac.AI_GRID_SHAPES:
    assert mha.lds_bytes(F, H, ds) == ac.ai_bytes(F, H, ds), (F, H, ds)
    if ac.ai_bytes(F, H, ds) > ac.AI_BUDGET:
      with pytest.raises(ValueError, match='envelope'):
        mha.check_envelope(F, H, ds)
    else:
      mha.check_envelope(F, H, ds)
  assert mha.LDS_BUDGET == ac.AI_BUDGET
  assert mha.lds_bytes(89, 1, 1) == 64792 and mha.lds_bytes(90, 1, 1) > mha.LDS_BUDGET
  assert any(ac.ai_bytes(*s) > ac.AI_BUDGET for s in ac.AI_GRID_SHAPES if s[:2] == (18, 2))
  for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
    with pytest.raises(ValueError, match='at least 1'):
      mha.check_envelope(*bad)
  for tag, c in ac.AI_CASES.items():
    assert min(8, mha.LDS_BUDGET // mha.lds_bytes(c['F'], c['H'], c['ds'])) == c['epb_bwd'] == ac.ai_epb(c['F'], c['H'], c['ds'], True), tag
    assert ac.ai_epb(c['F'], c['H'], c['ds'], False) == c['epb_fwd'], tag
  assert ac.AI_CASES['mid']['epb_bwd'] in (3, 5) and 1 < ac.AI_CASES['mid']['epb_fwd'] < 8
  assert ac.ai_batches('mid') == [1, 4, 5, 6, 11] and ac.ai_batches('f89') == [1, 2, 3, 5] and ac.ai_batches('d128') == [1, 2, 3, 5]
