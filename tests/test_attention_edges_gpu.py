"""The attention cores at the edges of their envelopes on the GPU: er_mha_fwd / _bwd / er_mha_group_* (csrc/er_mha.hip)
and er_autoint_attn_fwd / _bwd (csrc/er_autoint.hip) against the fp64 oracle under autograd.  Cases, inputs, references
and bars: tests/_attention_cases.py; the bars' justification on the CPU: tests/test_attention_pins.py.  Every output
buffer is handed to the library filled with NaN and every element it owns must come back finite.

Which case enters which loop:
  the key stride `j = lane; j < T; j += 64` of mha_softmax / mha_ds / mha_stage_adder with a ragged last round:
      t200_f1 (4 rounds, the last of 8), t70_f70 (2, 6), t4095_f1 (64, 63); their masks open only the last key of
      example 2 and only j = 64 of example 3
  the row stride `i = wave; i < F; i += waves` on one wave: f130_t3 grouped (G = 8: 130 rows on one wave);
      F > 8 x 64 on eight waves: f4096_t1; F > 64 on eight: t70_f70
  mha_group_units 8 / 4 / 2 / 1: f130_t3, m_rem2, m_rem3 / t200_f1 / g2 / the rest
  mha_mm's rows past M, M % 4 = 2 and 3, with F and with T as M: m_rem2, m_rem3 (t70_f70 and g2's F = T: 2 and 0)
  both sides of each envelope: edge_ds128 | (35, 35, 128) through attention_layer, t4095_f1 | (1, 4096, 1),
      f4096_t1 | F = 4097, ds 128 | 129 and AutoInt f89 | F = 90 in the two boundary tests (predicates only outside)
  er_autoint's examples per workgroup: backward 1 / forward 2: d128, f89; 1 / 3: f60; a middle one, 3 / 5: mid; 8 / 8: f1;
      B = epb - 1, epb, epb + 1, 2 epb + 1 for each
  F = 1 (AutoInt f1: dQ = dK = 0, y = relu(V + R)) and T = 1 (f4096_t1: ctx is V's row, dQ = dK = 0), to the bit
  saturated rows: t70_f70_top30 / _top80, sample_top30 / _top80, AutoInt d128_top80
"""
import logging

import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.core import context  # noqa: E402
from easyrec_amd.layers import multihead_attention as mha  # noqa: E402
from easyrec_amd.layers import multihead_cross_attention as mca  # noqa: E402
from oracle import uniter_ref as ref  # noqa: E402
from tests import _attention_cases as ac  # noqa: E402
from tests import _uniter_cases as ucases  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402
from tests._oracle_steps import close as _close  # noqa: E402

logging.disable(logging.WARNING)
DEV = 'cuda:0'
NAN = float('nan')


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
  return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _mha_run(inp, F, T, H, ds, group=False):
  """One forward and one backward launch on separate Q and K | V buffers; ctx, dQ and dK | dV go to the library full of
  NaN.  -> dict(ctx, dq, dk, dv), every element finite."""
  be = kernels.hip()
  B, d = inp['B'], H * ds
  q = inp['q'].to(DEV, torch.float32)
  kv = torch.cat([inp['k'], inp['v']], dim=1).to(DEV, torch.float32)
  dctx = inp['dctx'].to(DEV, torch.float32).contiguous()
  mask = None if inp['mask'] is None else inp['mask'].to(DEV).contiguous()
  assert q.shape == (B * F, d) and kv.shape == (B * T, 2 * d) and (mask is None or mask.dtype == torch.int32)
  k, v = kv[:, :d], kv[:, d:]
  ctx, dq, dkv = _nan(B * F, d), _nan(B * F, d), _nan(B * T, 2 * d)
  dk, dv = dkv[:, :d], dkv[:, d:]
  fwd, bwd = (be.ck.er_mha_group_fwd, be.ck.er_mha_group_bwd) if group else (be.ck.er_mha_fwd, be.ck.er_mha_bwd)
  mp = None if mask is None else mask.data_ptr()
  fwd(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), mp, B, F, T, H, ds, ctx.data_ptr(),
      _stream())
  bwd(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), mp, dctx.data_ptr(), B, F, T, H, ds,
      dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0), dv.data_ptr(), dv.stride(0), _stream())
  torch.cuda.synchronize()
  out = dict(ctx=ctx, dq=dq, dk=dk, dv=dv)
  for n, t in out.items():
    assert bool(torch.isfinite(t).all()), (n, 'an element was not written or is not finite')
  return out


def _same_bits(one, grouped, what):
  for n in ac.MHA_TENSORS:
    assert torch.equal(one[n], grouped[n]), (what, n)


@pytest.mark.parametrize('tag,masked', ac.MHA_RUNS, ids=ac.mha_run_id)
def test_mha_edge_cases_match_fp64_autograd(tag, masked):
  """ctx within its bar (1e-5 unless recorded), dQ / dK / dV within theirs (1e-4); a gradient that is exactly 0 in fp64
  (one key: P = 1) is exactly 0; where two or more units fit a workgroup the grouped launches give the same bits."""
  c, inp = ac.MHA_ALL[tag], ac.mha_inputs(tag, masked)
  F, T, H, ds = c['F'], c['T'], c['H'], c['ds']
  be = kernels.hip()
  G = be.mha_group_units(F, T, ds)
  if tag in ac.MHA_CASES:
    assert be.mha_lds_bytes(F, T, ds) == c['bytes'] <= be.MHA_LDS_BUDGET, (tag, be.mha_lds_bytes(F, T, ds))
    assert G == c['G'], (tag, G)
  got, want = _mha_run(inp, F, T, H, ds), ac.mha_reference(tag, masked)
  figures = {n: ac.measure(got[n], want[n], floor=1e-30 if want[n].any() else 1.0) for n in ac.MHA_TENSORS}
  print('EDGE op=mha case=%s masked=%d ' % (tag, masked) + ' '.join('%s=%.3g/%g' % (n, figures[n], ac.mha_bar(tag, masked, n))
                                                                     for n in ac.MHA_TENSORS))
  for n in ac.MHA_TENSORS:
    if want[n].any():
      _close(got[n], want[n], ac.mha_bar(tag, masked, n), (tag, masked, n))
    else:
      assert not bool(got[n].any()), (tag, masked, n, 'exactly 0 in fp64')
  if T == 1:  # softmax over one key: P = 1, ctx is V's row to the bit
    assert tag == 'f4096_t1' and not want['dq'].any() and not want['dk'].any()
    rows = inp['v'].view(inp['B'], 1, H * ds).expand(inp['B'], F, H * ds).reshape(inp['B'] * F, H * ds)
    assert torch.equal(got['ctx'].cpu(), rows.to(torch.float32))
  if G >= 2:
    _same_bits(got, _mha_run(inp, F, T, H, ds, group=True), (tag, masked))


def _random_inputs(B, F, T, H, ds, seed, masked):
  g = torch.Generator().manual_seed(seed)
  q, k, v, dctx = (torch.randn(B * n, H * ds, generator=g) for n in (F, T, T, F))
  return dict(q=q, k=k, v=v, dctx=dctx, mask=ac.mha_mask(B, T, seed) if masked else None, B=B)


GROUPED = [tag for tag, c in ac.MHA_CASES.items() if c['G'] >= 2]


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('tag', GROUPED)
def test_grouped_launches_at_the_new_shapes_give_the_one_unit_launches_bits(tag, masked):
  """B * H in {G - 1, G, G + 1}: a partial pass, a full one, a full and a partial one; with the shape's own head count
  where it divides the unit count, else with one head."""
  assert set(GROUPED) == {'t200_f1', 'f130_t3', 'g2', 'm_rem2', 'm_rem3'}
  c = ac.MHA_CASES[tag]
  F, T, ds = c['F'], c['T'], c['ds']
  G = kernels.hip().mha_group_units(F, T, ds)
  assert G == c['G'] == mca.mha_group_units(F, T, ds) and {'g2': 2, 't200_f1': 4}.get(tag, 8) == G
  seen = set()
  for units in (G - 1, G, G + 1):
    H = c['H'] if units % c['H'] == 0 else 1
    B = units // H
    seen.add(B * H)
    inp = _random_inputs(B, F, T, H, ds, 10 * units + F, masked)
    _same_bits(_mha_run(inp, F, T, H, ds), _mha_run(inp, F, T, H, ds, group=True), (tag, masked, B, H))
  assert seen == {G - 1, G, G + 1}


# ------------------------------------------------------------------------------------------------ the envelope's boundary
def test_python_predicates_agree_with_the_library_across_the_boundary():
  """lds_bytes (both kernels), mha_group_units and fits against er_mha_lds_bytes / er_mha_group_units on both
  neighbours of every edge case, the bounds and empty arguments.  Whether er_mha_fwd would accept a shape is decided
  from the library's own figures (its byte count within the budget, the bounds of mha_shape_ok; er_mha_group_units is
  0 exactly outside): no refused shape is launched."""
  be = kernels.hip()
  inside = 0
  for F, T, ds in ac.MHA_GRID_SHAPES:
    for bwd in (True, False):
      assert mca.lds_bytes(F, T, ds, bwd) == be.mha_lds_bytes(F, T, ds, bwd), (F, T, ds, bwd)
    G = be.mha_group_units(F, T, ds)
    assert mca.mha_group_units(F, T, ds) == G, (F, T, ds)
    accepted = (1 <= F <= ac.MHA_MAX_LEN and 1 <= T <= ac.MHA_MAX_LEN and 1 <= ds <= be.MHA_MAX_DS and
                0 < be.mha_lds_bytes(F, T, ds, True) <= be.MHA_LDS_BUDGET)
    assert mca.fits(F, T, ds) == accepted == (G >= 1), (F, T, ds, accepted, G)
    inside += accepted
  assert 0 < inside < len(ac.MHA_GRID_SHAPES)
  for shape in ((35, 35, 128), (1, 4096, 1), (4097, 1, 1), (1, 1, 129), (0, 5, 4)):
    assert shape in ac.MHA_GRID_SHAPES and be.mha_group_units(*shape) == 0 and not mca.fits(*shape)
  for shape in ((34, 34, 128), (1, 4095, 1), (4096, 1, 1), (1, 1, 128)):
    assert shape in ac.MHA_GRID_SHAPES and be.mha_group_units(*shape) >= 1 and mca.fits(*shape)


def _attention_layer_run(F, monkeypatch):
  """attention_layer (self-attention, one head of 128, a to-mask) on F tokens with the fused path on -> (y, dx and their
  fp64 values, the names of the launches)."""
  monkeypatch.setenv('EASYREC_AMD_FUSED_MHA', '1')
  B, H, ds, W = ac.MHA_OUTSIDE['B'], ac.MHA_OUTSIDE['H'], ac.MHA_OUTSIDE['ds'], 24
  g = torch.Generator().manual_seed(F)
  x64 = torch.randn(B, F, W, generator=g, dtype=torch.float64).float().double()
  dy64 = torch.randn(B * F, H * ds, generator=g, dtype=torch.float64).float().double()
  mask = ref.mixed_mask(B, F, 3)
  x, mask_d = x64.to(DEV, torch.float32), mask.to(DEV)

  def forward(xi):
    with context.varstore().scope('a'):
      return mca.attention_layer(xi, xi, ds, H, mca.create_attention_mask_from_input_mask(xi, mask_d),
                                 do_return_2d_tensor=True)

  vs, _ = ucases.product_store(DEV, lambda: forward(x))
  params = {n: (torch.randn(v.shape, generator=g, dtype=torch.float64) * (W ** -0.5 if n.endswith('kernel') else 1.0)).float().double()
            for n, v in vs.state_dict().items()}
  assert sorted(params) == sorted('a/%s/%s' % (n, p) for n in ('query', 'key', 'value') for p in ('kernel', 'bias'))
  vs, ctx = ucases.product_store(DEV, lambda: forward(x), params)
  assert mca._fused(x)
  be = kernels.hip()
  xi = x.detach().requires_grad_(True)
  be.op_log = []
  try:
    with context.use(ctx):
      y = forward(xi)
      y.backward(dy64.to(DEV, torch.float32))
    names = [n for n, _ in be.op_log]
  finally:
    be.op_log = None
  torch.cuda.synchronize()
  xr = x64.clone().requires_grad_(True)
  x2 = xr.reshape(B * F, W)
  want = ref.attention_layer(x2, x2, params, 'a', mask, B, F, F, H, ds)
  (want * dy64).sum().backward()
  return y.detach(), xi.grad, want.detach(), xr.grad, names


def test_the_first_shape_outside_takes_the_composition_and_the_last_inside_the_kernels(monkeypatch):
  """(35, 35, 128) needs 82180 bytes: attention_layer launches no er::mha_ kernel and its result holds the same bars;
  (34, 34, 128), through the same code, launches them."""
  F = ac.MHA_OUTSIDE['F']
  be = kernels.hip()
  assert be.mha_lds_bytes(F, F, 128) == ac.MHA_OUTSIDE['bytes'] > be.MHA_LDS_BUDGET and not mca.fits(F, F, 128)
  for n, launched in ((F, False), (F - 1, True)):
    y, dx, want, dx64, names = _attention_layer_run(n, monkeypatch)
    mha_names = [k for k in names if k.startswith('er::mha_')]
    assert (sorted(mha_names) == ['er::mha_bwd_kernel', 'er::mha_fwd_kernel']) if launched else not mha_names, (n, names)
    _close(y, want, ac.FWD_BAR, (n, 'y'))
    _close(dx, dx64, ac.GRAD_BAR, (n, 'dx'))


# ------------------------------------------------------------------------------------------------ AutoInt
def _autoint_run(g64, dy64, B, F, H, ds):
  """-> (y [B F, d], dg [B F, 4d]) from NaN-filled buffers, every element finite."""
  be = kernels.hip()
  d = H * ds
  g, dy = g64.to(DEV, torch.float32).contiguous(), dy64.to(DEV, torch.float32).contiguous()
  assert g.shape == (B * F, 4 * d) and dy.shape == (B * F, d)
  y, dg = _nan(B * F, d), _nan(B * F, 4 * d)
  be.ck.er_autoint_attn_fwd(g.data_ptr(), B, F, H, ds, y.data_ptr(), _stream())
  be.ck.er_autoint_attn_bwd(g.data_ptr(), y.data_ptr(), dy.data_ptr(), B, F, H, ds, dg.data_ptr(), _stream())
  torch.cuda.synchronize()
  assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dg).all())
  return y, dg


@pytest.mark.parametrize('tag', list(ac.AI_CASES))
def test_autoint_edge_cases_match_fp64_autograd(tag):
  """y within its bar, dQ | dK | dV | dR (through the kernels' own ReLU pattern) within theirs, at every B around the
  larger of the two kernels' examples per workgroup."""
  c = ac.AI_CASES[tag]
  F, H, ds = c['F'], c['H'], c['ds']
  d = H * ds
  be = kernels.hip()
  assert be.autoint_lds_bytes(F, H, ds) == mha.lds_bytes(F, H, ds) == ac.ai_bytes(F, H, ds) <= be.AUTOINT_LDS_BUDGET
  assert (be.autoint_epb(F, H, ds, 1), be.autoint_epb(F, H, ds, 0)) == (c['epb_bwd'], c['epb_fwd']), tag
  if tag == 'mid':
    assert c['epb_bwd'] == min(8, mha.LDS_BUDGET // mha.lds_bytes(F, H, ds)) == 3
  for B in ac.ai_batches(tag):
    inp = ac.ai_inputs(tag, B)
    y, dg = _autoint_run(inp['g'], inp['dy'], B, F, H, ds)
    got = dict(y=y, dq=dg[:, :d], dk=dg[:, d:2 * d], dv=dg[:, 2 * d:3 * d], dr=dg[:, 3 * d:])
    want = ac.ai_eval(tag, B, ac.F64, (y.double().cpu() > 0).to(ac.F64))
    figures = {n: ac.measure(got[n], want[n], floor=1e-30 if want[n].any() else 1.0) for n in ac.AI_TENSORS}
    print('EDGE op=autoint case=%s B=%d ' % (tag, B) + ' '.join('%s=%.3g/%g' % (n, figures[n], ac.ai_bar(tag, n))
                                                                for n in ac.AI_TENSORS))
    for n in ac.AI_TENSORS:
      if want[n].any():
        _close(got[n], want[n], ac.ai_bar(tag, n), (tag, B, n))
      else:
        assert not bool(got[n].any()), (tag, B, n, 'exactly 0 in fp64')
    if F == 1:  # softmax over one field: P = 1, dS = 0
      assert tag == 'f1' and not want['dq'].any() and not want['dk'].any()
      g32 = inp['g'].to(torch.float32)
      assert torch.equal(y.cpu(), torch.relu(g32[:, 2 * d:3 * d] + g32[:, 3 * d:]))


def test_autoint_predicates_agree_with_the_library_across_the_boundary():
  """lds_bytes against er_autoint_lds_bytes around (89 | 90, 1, 1) and (18, 2, 64 .. 106); check_envelope raises exactly
  where the library's budget is exceeded, which is where er_autoint_epb gives 0."""
  be = kernels.hip()
  raised = 0
  for F, H, ds in ac.AI_GRID_SHAPES:
    assert mha.lds_bytes(F, H, ds) == be.autoint_lds_bytes(F, H, ds), (F, H, ds)
    outside = be.autoint_lds_bytes(F, H, ds) > be.AUTOINT_LDS_BUDGET
    assert outside == (be.autoint_epb(F, H, ds, 1) == 0) == (be.autoint_epb(F, H, ds, 0) == 0), (F, H, ds)
    if outside:
      raised += 1
      with pytest.raises(ValueError, match='envelope'):
        mha.check_envelope(F, H, ds)
    else:
      mha.check_envelope(F, H, ds)
  assert 0 < raised < len(ac.AI_GRID_SHAPES)
  assert be.autoint_epb(89, 1, 1, 1) == 1 and be.autoint_epb(90, 1, 1, 1) == 0
  assert be.autoint_epb(18, 2, 104, 1) == 1 and be.autoint_epb(18, 2, 105, 1) == 0


# ------------------------------------------------------------------------------------------------ bit identity
def test_two_runs_and_a_graph_replay_are_bit_identical_at_the_multi_round_shapes():
  """t200_f1 through the grouped launches and t70_f70 through the one-unit launches, each with more units than one
  walk of the persistent grid (1024 workgroups x G), and AutoInt d128."""
  be = kernels.hip()
  jobs = []
  for tag, B, group in (('t200_f1', 2049, True), ('t70_f70', 1025, False)):
    c = ac.MHA_CASES[tag]
    F, T, H, ds = c['F'], c['T'], c['H'], c['ds']
    assert B * H > ac.MHA_GRID * (c['G'] if group else 1) and (c['G'] >= 2) == group
    d = H * ds
    q, kv, dctx = torch.randn(B * F, d, device=DEV), torch.randn(B * T, 2 * d, device=DEV), torch.randn(B * F, d, device=DEV)
    jobs.append((group, q, kv, ac.mha_mask(B, T, 6).to(DEV), dctx, B, F, T, H, ds))
  a = ac.AI_CASES['d128']
  aB, aF, aH, ads = 257, a['F'], a['H'], a['ds']
  g = torch.randn(aB * aF, 4 * aH * ads, device=DEV)
  g[:, :2 * aH * ads] *= ads ** -0.5
  dy = torch.randn(aB * aF, aH * ads, device=DEV)

  def mha(group, q, kv, mask, dctx, B, F, T, H, ds):
    d = H * ds
    fwd, bwd = (be.mha_group_fwd, be.mha_group_bwd) if group else (be.mha_fwd, be.mha_bwd)
    ctx = fwd(q, kv[:, :d], kv[:, d:], mask, B, F, T, H, ds)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    bwd(q, kv[:, :d], kv[:, d:], mask, dctx, B, F, T, H, ds, dq, dkv[:, :d], dkv[:, d:])
    return [ctx, dq, dkv]

  def run():
    out = []
    for job in jobs:
      out += mha(*job)
    y = be.autoint_attn_fwd(g, aF, aH, ads)
    return out + [y, be.autoint_attn_bwd(g, y, dy, aF, aH, ads)]

  assert_runs_and_replay_bit_identical(run)
  first = run()
  torch.cuda.synchronize()
  assert all(bool(torch.isfinite(t).all()) for t in first)
  one_unit = mha(False, *jobs[0][1:])  # (the grouped walk of 4098 units against the one-unit launches)
  torch.cuda.synchronize()
  assert all(torch.equal(x, y) for x, y in zip(first[:3], one_unit))
