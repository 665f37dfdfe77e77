"""-m gpu: the FM / row sum, cross v1, cross v2 epilogue, DIN, MMoE and sigmoid cross-entropy kernels of
libeasyrec_hip.so (through easyrec_amd.kernels.HipBackend) against fp64 autograd of their formulas, on the cases and
within the derived per-element bounds of tests/_interaction_cases.py (tests/test_interaction_restatement.py holds a
plain float32 evaluation and the CPU oracle to the same ones).

Each case also asserts the dispatch it is meant to take where that is plain host arithmetic on shape, stride and
address, that a second launch returns the same bits, and - for the shapes the library must refuse - that it raises.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from tests import _interaction_cases as ic  # noqa: E402

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def hip():
  assert torch.cuda.is_available(), 'gpu tests need an MI355X'
  return kernels.hip()


def _same_bits(a, b, what):
  for k in a:
    assert torch.equal(a[k], b[k]), '%s: %s differs between two launches' % (what, k)


def _aligned(ptrs):
  return all(p % 16 == 0 for p in ptrs)


def _run_case(hip, op, case):
  _, want, bound = ic.reference(op, case['id'])
  seen = {}
  got = ic.run(op, hip, case['id'], DEV, seen)
  ic.check('hip', op, case, got, want, bound)
  _same_bits(got, ic.run(op, hip, case['id'], DEV), case['id'])
  return seen


@pytest.mark.parametrize('case', ic.FM_CASES, ids=[c['id'] for c in ic.FM_CASES])
def test_fm_and_rowsum(hip, case):
  seen = _run_case(hip, 'fm', case)
  # er_fm_fwd's rule, from what the call was given: the 'wide' layouts must stay on fm_fwd_kernel<4> with
  # x_stride > F*D, the 'off1' ones must fall back to <1>
  vec = case['D'] % 4 == 0 and seen['x_stride'] % 4 == 0 and seen['x_ptr'] % 16 == 0
  assert vec == ic.fm_vec_expected(case)
  assert (seen['x_stride'] > case['F'] * case['D']) == (case['layout'] != 'contig')


@pytest.mark.parametrize('case', ic.CROSS_V1_CASES, ids=[c['id'] for c in ic.CROSS_V1_CASES])
def test_cross_v1(hip, case):
  _run_case(hip, 'cross_v1', case)
  assert hip.lib.er_cross_v1_bwd_partials(case['B']) == min(case['B'], 512)  # rows beyond 512 stride over the grid


@pytest.mark.parametrize('case', ic.CROSS_V1_REFUSED, ids=[c['id'] for c in ic.CROSS_V1_REFUSED])
def test_cross_v1_refuses(hip, case):
  inp = {k: v.to(DEV) for k, v in ic.cross_v1_inputs(case).items()}
  dots = torch.zeros(case['B'], case['L'], device=DEV)
  if case['d'] > 1024:
    with pytest.raises(RuntimeError, match='exceeds'):
      hip.cross_v1_fwd(inp['x0'], inp['w'], inp['b'])
  with pytest.raises(RuntimeError, match='er_cross_v1_bwd'):
    hip.cross_v1_bwd(inp['x0'], inp['w'], inp['b'], dots, inp['dout'])
  torch.cuda.synchronize()  # nothing was launched: nothing to fail here


@pytest.mark.parametrize('case', ic.CROSS_V2_CASES, ids=[c['id'] for c in ic.CROSS_V2_CASES])
def test_cross_v2_epilogue(hip, case):
  inp = ic.cross_v2_inputs_of(case['id'])
  for variant in ic.cross_v2_variants():
    want, bound = ic.cross_v2_reference(case['id'], variant)
    seen = {}
    got = ic.run_cross_v2(hip, case, inp, DEV, variant, seen)
    tag = dict(case, id='%s-diag%g-bias%d-dx%d-acc0%d-accx%d' % ((case['id'],) + variant))
    ic.check('hip', 'cross_v2', tag, got, want, bound)
    _same_bits(got, ic.run_cross_v2(hip, case, inp, DEV, variant), tag['id'])
    # er_cross_v2_epilogue_bwd_acc's rule: <4> needs d % 4 == 0, every leading dimension % 4 == 0, every base aligned
    vec = case['d'] % 4 == 0 and all(ld % 4 == 0 for ld in seen['lds']) and _aligned(seen['ptrs'])
    assert vec == ic.cross_v2_vec_expected(case), tag['id']
  for diag in ic.CROSS_V2_DIAGS:
    for has_bias in (True, False):
      want, bound = ic.cross_v2_plain_reference(case['id'], diag, has_bias)
      got = ic.run_cross_v2_plain(hip, case, inp, DEV, diag, has_bias)
      ic.check('hip', 'cross_v2', dict(case, id='%s-plain-diag%g-bias%d' % (case['id'], diag, has_bias)), got, want, bound)
      _same_bits(got, ic.run_cross_v2_plain(hip, case, inp, DEV, diag, has_bias), case['id'])


@pytest.mark.parametrize('case', ic.DIN_CASES, ids=[c['id'] for c in ic.DIN_CASES])
def test_din_concat_and_pool(hip, case):
  seen = _run_case(hip, 'din', case)
  # din_fast_ok: the shape rule and 16-byte alignment of every tensor the five entry points test
  fast = ic.din_fast_expected(case) and _aligned(seen['ptrs'])
  assert fast == (case['path'] == 'fast')
  assert _aligned(seen['ptrs'])  # so the general-path cases are general by SHAPE, not by a stray address


@pytest.mark.parametrize('case', ic.MMOE_CASES, ids=[c['id'] for c in ic.MMOE_CASES])
def test_mmoe_mix(hip, case):
  _run_case(hip, 'mmoe', case)


def test_mmoe_refuses_more_than_32_experts(hip):
  case = ic.MMOE_REFUSED
  inp = {k: v.to(DEV) for k, v in ic.mmoe_inputs(case).items()}
  with pytest.raises(RuntimeError, match='at most 32 experts'):
    hip.mmoe_mix_fwd(inp['experts'], inp['logits'])
  with pytest.raises(RuntimeError, match='at most 32 experts'):
    hip.mmoe_mix_bwd(inp['experts'], torch.softmax(inp['logits'], dim=-1), inp['dout'])
  torch.cuda.synchronize()


@pytest.mark.parametrize('case', ic.CE_CASES, ids=[c['id'] for c in ic.CE_CASES])
def test_sigmoid_ce(hip, case):
  _run_case(hip, 'ce', case)
