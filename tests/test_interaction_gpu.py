"""-m gpu: the FM / row sum, cross v1, cross v2 epilogue, DIN, MMoE, sigmoid cross-entropy, CIN (each of its four
kernels on its own) and DLRM dot-interaction kernels of libeasyrec_hip.so (through easyrec_amd.kernels.HipBackend) against fp64 autograd of their formulas, on the cases and
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


@pytest.mark.parametrize('case', ic.CIN_CASES, ids=[c['id'] for c in ic.CIN_CASES])
def test_cin(hip, case):
  _run_case(hip, 'cin', case)


def _sentinel(*shape):
  return torch.full(shape, -7.5, dtype=torch.float32, device=DEV)


def _untouched(*tensors):
  torch.cuda.synchronize()  # nothing was launched: nothing to fail here, and nothing was written
  for t in tensors:
    assert bool((t == -7.5).all())


@pytest.mark.parametrize('case', ic.CIN_REFUSED, ids=[c['id'] for c in ic.CIN_REFUSED])
def test_cin_refuses(hip, case):
  B, H, H0, D = case['B'], case['H'], case['H0'], case['D']
  strides = ic.cin_strides(case)
  if case['kernel'] == 'outer_fwd':
    # the column check precedes any access: a few floats stand for the operands, so the ABI is called directly
    xi, x0, z = torch.ones(8, device=DEV), torch.ones(8, device=DEV), _sentinel(8)
    with pytest.raises(RuntimeError, match=case['match']):
      hip.ck.er_cin_outer_fwd(xi.data_ptr(), strides[0], strides[1], strides[2], H, x0.data_ptr(), H0, D, B, z.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    _untouched(z)
    return
  assert case['form'] == 'first'  # dxi IS dx0
  x0, dz, dx0 = torch.ones(B, H0, D, device=DEV), torch.ones(B * D, H * H0, device=DEV), _sentinel(B, H0, D)
  with pytest.raises(RuntimeError, match=case['match']):
    hip.cin_outer_bwd(dz, x0, strides, H, x0, dx0, bool(case['add_xi']), dx0)
  _untouched(dx0)


@pytest.mark.parametrize('case', ic.DOT_CASES, ids=[c['id'] for c in ic.DOT_CASES])
def test_dot_interaction(hip, case):
  seen = _run_case(hip, 'dot', case)
  if case['fwd_only']:  # F = 128, D = 64: the forward's LDS fits, the backward's (with the P gradients) does not
    inp = ic.reference('dot', case['id'])[0]
    dx = _sentinel(case['B'], case['F'] * case['D'])
    with pytest.raises(RuntimeError, match='er_dot_interaction_bwd.*exceed the LDS budget'):
      hip.dot_interaction_bwd(inp['xw'].to(DEV), inp['gw'].to(DEV), case['F'], case['D'], case['si'], into=dx)
    _untouched(dx)
  elif case['layout'] == 'wide':  # x, out, g, dx: every base off a 16-byte boundary, no row stride a multiple of 4
    assert all(p % 16 for p in seen['ptrs']) and all(s % 4 for s in seen['strides'])


@pytest.mark.parametrize('case', ic.DOT_REFUSED, ids=[c['id'] for c in ic.DOT_REFUSED])
def test_dot_refuses(hip, case):
  B, F, D, si, what = case['B'], case['F'], case['D'], case['si'], case['what']
  n, P = F * D, ic.dot_pairs(F, si)
  x, g = torch.ones(B, n, device=DEV), torch.ones(B, P, device=DEV)
  out, dx = _sentinel(B, P), _sentinel(B, n)
  short = lambda t: torch.as_strided(t, (B, P), (P - 1, 1))  # rows P - 1 apart: they overlap
  if what in ('fwd_lds', 'out_stride'):
    with pytest.raises(RuntimeError, match='er_dot_interaction_fwd.*' + case['match']):
      hip.dot_interaction_fwd(x, F, D, si, out=short(out) if what == 'out_stride' else out)
  if what != 'out_stride':
    with pytest.raises(RuntimeError, match='er_dot_interaction_bwd.*' + case['match']):
      hip.dot_interaction_bwd(x, short(g) if what == 'g_stride' else g, F, D, si, into=dx)
  _untouched(out, dx)


def test_cin_four_kernels_replay_from_a_graph(hip):
  """The four launches of one later-layer case, captured once: a replay, and a replay after new inputs were copied
  into the static buffers, return the bits of eager launches."""
  case = ic.case_by_id('cin', 'cin-later-2x17x16x2x3-col1of6-alias-add1')
  inputs = [ic.reference('cin', case['id'])[0], ic.cin_inputs(case, seed=1017)]
  eager = [{k: v.clone() for k, v in ic.run_cin(hip, case, inp, DEV).items()} for inp in inputs]
  assert not torch.equal(eager[0]['z'], eager[1]['z'])
  static = ic.cin_buffers(case, inputs[0], DEV)

  def refill(inp):  # the launches work in place (c -> fm, dx0 +=, dc over dnext): every buffer gets its start value
    for k, v in ic.cin_buffers(case, inp, DEV).items():
      if v is not None:
        static[k].copy_(v)

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    ic.cin_launch(hip, case, static)  # (warm-up on the capture stream)
  torch.cuda.current_stream().wait_stream(s)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    ic.cin_launch(hip, case, static)
  for inp, want in zip(inputs, eager):
    refill(inp)
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(want, ic.cin_results(static), case['id'])
