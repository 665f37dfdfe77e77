"""The cross-attention blocks, the CMBF layer and segment mean pooling on the CPU: the fp64 restatement
(oracle/cmbf_ref.py) against the REFERENCE'S OWN run (tests/golden/cmbf_vectors.npz, made by
tests/golden/make_cmbf_vectors.py from the reference's layers/cmbf.py, layers/multihead_cross_attention.py and
model/cmbf.py over the numpy stand-in) at 1e-9; the product on the stand-in backend with the reference's variable names
and order, its layer output and logits at 1e-5 and every gradient against the restatement at 1e-4; the Python mirror of
er_mha_group_units against the library; the segment mean composition against a plain loop."""
import numpy as np
import pytest
import torch

from easyrec_amd.core import context
from easyrec_amd.layers import multihead_cross_attention as mca
from oracle import cmbf_ref as cref
from oracle import uniter_ref as ref
from tests import _cmbf_cases as ccases
from tests import _uniter_cases as cases
from tests._oracle_steps import close

GOLD = ccases.fixture()
CASES = sorted({k.split(':')[0] for k in GOLD.files})
TAPS = ('image_tower', 'text_tower', 'image_cross', 'text_cross')


def test_fixture_covers_the_cases():
  assert CASES == sorted(['all', 'img0', 'patches', 'multi_image', 'image_only', 'text_only', 'general_only',
                          'no_token_type_no_pos', 'other_plain', 'eval'])
  cfg, groups, training, inputs, var = ccases.fixture_case(GOLD, 'all')
  c = cfg.model_config.cmbf.config
  assert (c.multi_head_num, c.text_head_size, c.image_head_size, c.image_cross_head_size, c.text_cross_head_size) == \
      (2, 4, 3, 3, 4)
  assert c.hidden_dropout_prob == 0 and c.attention_probs_dropout_prob == 0 and c.text_seq_emb_dropout_prob == 0
  assert c.image_self_attention_layer_num == 2 and 'img_map_matrix' in var and 'img_projection/kernel' in var
  assert any(n.startswith('other_dnn/') for n in var)
  lens = [n.tolist() for _, n in inputs['text']]
  assert all(n.count(1) >= 2 and 0 not in n for n in lens) and 5 in lens[0] and 3 in lens[1] and len(lens[0]) == 6
  c0 = ccases.fixture_case(GOLD, 'img0')
  assert c0[0].model_config.cmbf.config.image_self_attention_layer_num == 0 and GOLD['img0:image_tower'].shape == (6, 1, 6)
  assert 'img_projection/kernel' in c0[4] and 'img_map_matrix' not in c0[4]
  assert ccases.fixture_case(GOLD, 'patches')[0].model_config.cmbf.config.image_feature_patch_num == 3
  assert GOLD['patches:image_tower'].shape == (6, 3, 6) and GOLD['multi_image:image_tower'].shape == (6, 2, 6)
  assert ccases.fixture_case(GOLD, 'image_only')[1] == ['image'] and ccases.fixture_case(GOLD, 'text_only')[1] == ['general', 'text']
  assert ccases.fixture_case(GOLD, 'general_only')[1] == ['image', 'general'] and GOLD['general_only:hidden'].shape == (6, 6 + 3 * 8)
  nt = ccases.fixture_case(GOLD, 'no_token_type_no_pos')
  assert not any(n.startswith('token_type/') or n.startswith('position_embedding/') for n in nt[4])
  assert 'token_type/token_type_embeddings' in var and 'position_embedding/position_embeddings_1' in var
  assert not any(n.startswith('other_dnn/') for n in ccases.fixture_case(GOLD, 'other_plain')[4])
  assert not ccases.fixture_case(GOLD, 'eval')[2]


@pytest.mark.parametrize('tag', CASES)
def test_restatement_matches_the_reference(tag):
  """Every tensor of the fixture - both towers, both cross outputs, the layer output, logits and probs - at 1e-9."""
  cfg, groups, training, inputs, var = ccases.fixture_case(GOLD, tag)
  towers, hidden, logits = cref.cmbf_model(var, cfg, inputs, training)
  seen = 0
  for k in TAPS:
    if '%s:%s' % (tag, k) in GOLD.files:
      close(towers[k], GOLD['%s:%s' % (tag, k)], 1e-9, (tag, k))
      seen += 1
  assert seen == {'image_only': 1, 'text_only': 1}.get(tag, 4)
  close(hidden, GOLD['%s:hidden' % tag], 1e-9, (tag, 'hidden'))
  close(logits, GOLD['%s:logits' % tag], 1e-9, (tag, 'logits'))
  close(torch.sigmoid(logits), GOLD['%s:probs' % tag], 1e-9, (tag, 'probs'))


@pytest.mark.parametrize('tag', CASES)
def test_product_names_forward_and_gradients_match_the_reference(ref_backend, tag):
  """The variables the product creates are the reference's (BatchNorm's moving statistics aside: the stand-in creates
  them only where it reads them, in eval mode), in the reference's creation order; towers, cross outputs, layer output
  and logits match the reference's at 1e-5 (fp32 against fp64); in the training cases the gradient of every variable
  the layer output depends on matches the fp64 restatement's at 1e-4 (cmbf_ref.grad_floor: a key bias as for Uniter,
  and a cross block's query / key projections at their value kernel's scale - the block collapses a side's tokens and
  those gradients are zero up to rounding)."""
  cfg, groups, training, inputs, var = ccases.fixture_case(GOLD, tag)
  vs, ctx, run = ccases.product_fixture_forward('cpu', cfg, training, inputs, var)
  got = [n for n in vs.names() if '/moving_' not in n]
  assert got == [n for n in var if '/moving_' not in n]
  assert all(tuple(vs.state_dict()[n].shape) == tuple(var[n].shape) for n in var)
  W = GOLD['%s:hidden' % tag].shape[1]
  dy64 = torch.randn(6, W, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
  vs.zero_grad()
  with context.use(ctx):
    layer, hidden, logits = run()
    if training:
      (hidden * dy64.float()).sum().backward()
  for k in TAPS:
    if '%s:%s' % (tag, k) in GOLD.files:
      close(layer.taps[k], GOLD['%s:%s' % (tag, k)], 1e-5, (tag, k))
  close(hidden, GOLD['%s:hidden' % tag], 1e-5, (tag, 'hidden'))
  close(logits, GOLD['%s:logits' % tag], 1e-5, (tag, 'logits'))
  close(torch.sigmoid(logits), GOLD['%s:probs' % tag], 1e-5, (tag, 'probs'))
  if not training:
    return
  pr = {n: v.clone().requires_grad_(True) for n, v in var.items()}
  _, want, _ = cref.cmbf_model(pr, cfg, inputs, training)
  (want * dy64).sum().backward()
  ref_grads = {n: p.grad for n, p in pr.items() if p.grad is not None}
  got = vs.grad_dict()
  assert len(ref_grads) > 30
  for n, g in ref_grads.items():
    if n.endswith('/bias') and (n[:-len('/bias')] + '/bn/gamma') in var:
      continue  # d(loss)/d(bias) == 0 under BatchNorm: rounding noise in fp64, exactly 0 in the product
    close(got[n], g, 1e-4, (tag, n), scale=cref.grad_floor(n, ref_grads))


def test_cross_tower_names_order_and_the_refused_left_mask(ref_backend):
  """<name>{left_to_right,right_to_left}_cross_layer_<i>/... in the reference's creation order; a left_input_mask raises
  (the reference hands None to create_attention_mask_from_input_mask there and fails itself)."""
  left, right = torch.randn(3, 2, 6), torch.randn(3, 5, 8)

  def tower(**kw):
    return mca.cross_attention_tower(left, right, num_hidden_layers=2, num_attention_heads=2, left_size_per_head=3,
                                     right_size_per_head=4, **kw)

  vs, ctx = cases.product_store('cpu', lambda: tower(right_input_mask=torch.ones(3, 5, dtype=torch.int32)))
  assert vs.names() == cref.cross_tower_variable_names(2)
  st = vs.state_dict()
  # a block's projections read the OTHER side's width for key / value; intermediate <= 0 means H * size_per_head
  assert st['left_to_right_cross_layer_0/attention/cross/key/kernel'].shape == (8, 6)
  assert st['right_to_left_cross_layer_0/attention/cross/key/kernel'].shape == (6, 8)
  assert st['left_to_right_cross_layer_1/attention/cross/key/kernel'].shape == (8, 6)
  assert st['left_to_right_cross_layer_0/intermediate/dense/kernel'].shape == (6, 6)
  assert all(vs.l2_of(n) == 0.0 for n in vs.names())
  with context.use(ctx), torch.no_grad():
    a, b = tower(right_input_mask=torch.ones(3, 5, dtype=torch.int32))
    assert tuple(a.shape) == (3, 2, 6) and tuple(b.shape) == (3, 5, 8)
    with pytest.raises(ValueError, match='left_input_mask'):
      tower(left_input_mask=torch.ones(3, 2, dtype=torch.int32))


def test_cross_tower_on_the_stand_in_matches_the_restatement(ref_backend):
  """Both blocks of a layer read the PREVIOUS layer's outputs; a right mask with an all-masked and a single-key example;
  forward at 1e-5, the inputs' and every variable's gradient at 1e-4."""
  B, L, R, H, lds, rds = 4, 3, 7, 2, 3, 4
  g = torch.Generator().manual_seed(8)
  l64, r64 = torch.randn(B, L, 5, generator=g, dtype=torch.float64), torch.randn(B, R, 9, generator=g, dtype=torch.float64)
  mask = ref.mixed_mask(B, R, 6)

  def tower(a, b):
    return mca.cross_attention_tower(a, b, num_hidden_layers=2, num_attention_heads=H, left_size_per_head=lds,
                                     right_size_per_head=rds, left_intermediate_size=7, right_intermediate_size=0,
                                     right_input_mask=mask, initializer_range=0.5)

  vs, ctx = cases.product_store('cpu', lambda: tower(l64.float(), r64.float()))
  params = {n: torch.randn(v.shape, generator=g, dtype=torch.float64) * 0.4 for n, v in vs.state_dict().items()}
  vs, ctx = cases.product_store('cpu', lambda: tower(l64.float(), r64.float()), params)
  a, b = l64.float().requires_grad_(True), r64.float().requires_grad_(True)
  da, db = torch.randn(B, L, H * lds, generator=g, dtype=torch.float64), torch.randn(B, R, H * rds, generator=g, dtype=torch.float64)
  with context.use(ctx):
    ya, yb = tower(a, b)
    ((ya * da.float()).sum() + (yb * db.float()).sum()).backward()
  pr = {n: p.clone().requires_grad_(True) for n, p in params.items()}
  ar, br = l64.clone().requires_grad_(True), r64.clone().requires_grad_(True)
  wa, wb = cref.cross_attention_tower(ar, br, pr, 2, H, lds, rds, mask)
  ((wa * da).sum() + (wb * db).sum()).backward()
  close(ya, wa, 1e-5, 'left')
  close(yb, wb, 1e-5, 'right')
  close(a.grad, ar.grad, 1e-4, 'd left')
  close(b.grad, br.grad, 1e-4, 'd right')
  ref_grads = {n: p.grad for n, p in pr.items()}
  for n, gr in vs.grad_dict().items():
    close(gr, ref_grads[n], 1e-4, n, scale=cref.grad_floor(n, ref_grads))


def test_group_units_default_leaves_every_launch_as_it_was(ref_backend):
  import inspect
  assert inspect.signature(mca.attention_layer).parameters['group_units'].default is False
  assert inspect.signature(mca.transformer_encoder).parameters['group_units'].default is False


def test_group_units_formula_is_the_library_s(built_lib, monkeypatch):
  """8 / 4 / 2 / 1 / 0 on both sides of every edge: G * er_mha_lds_bytes(F, T, ds, 1) <= 81920."""
  from easyrec_amd import kernels
  be = kernels.HipBackend()
  grid = [(F, T, ds) for F in (1, 2, 5, 9, 17, 33, 40, 64, 100) for T in (1, 3, 8, 33, 64, 200) for ds in (1, 3, 4, 16, 24, 64, 128)]
  grid += [(0, 3, 4), (3, 0, 4), (3, 3, 0), (3, 3, 129), (4097, 1, 1), (1, 4097, 1), (4096, 1, 1)]
  for F, T, ds in grid:
    assert be.mha_group_units(F, T, ds) == mca.mha_group_units(F, T, ds), (F, T, ds)
  seen = set()
  for ds in (16, 128):
    prev = 8
    for n in range(1, 140):
      g, unit = mca.mha_group_units(n, n, ds), mca.lds_bytes(n, n, ds)
      assert g == be.mha_group_units(n, n, ds)
      want = 0 if unit > mca.LDS_BUDGET else next((k for k in (8, 4, 2) if k * unit <= mca.LDS_BUDGET), 1)
      assert g == want and g <= prev, (n, ds, g)
      if g != prev:  # an edge: n - 1 had `prev`, n has g
        seen.add((prev, g))
      prev = g
  assert seen >= {(8, 4), (4, 2), (2, 1), (1, 0)}
  # CMBF's sample shapes: every one of them groups
  assert [mca.mha_group_units(*s) for s in ((1, 33, 16), (33, 1, 16), (33, 33, 16), (1, 1, 16), (64, 64, 24))] == [8, 8, 4, 8, 1]
  assert mca.mha_group_units(33, 33, 128) == 1 and mca.mha_group_units(64, 64, 128) == 0
  import ctypes
  host = ctypes.addressof(ctypes.create_string_buffer(16))  # (non-null; the shape is refused before anything reads it)
  with pytest.raises(RuntimeError, match='one unit per workgroup'):
    be.ck.er_mha_group_fwd(host, 128, host, 128, host, 128, None, 1, 33, 33, 1, 128, host, None)
  with pytest.raises(RuntimeError, match='outside the envelope'):
    be.ck.er_mha_group_fwd(host, 128, host, 128, host, 128, None, 1, 64, 64, 1, 128, host, None)
  monkeypatch.setenv('EASYREC_AMD_MHA_GROUP_UNITS', '0')
  assert not mca.group_units_enabled()
  monkeypatch.setenv('EASYREC_AMD_MHA_GROUP_UNITS', '1')
  assert mca.group_units_enabled()
  monkeypatch.delenv('EASYREC_AMD_MHA_GROUP_UNITS')
  assert mca.group_units_enabled() == (mca.GROUP_UNITS_DEFAULT != '0')


def test_segment_mean_composition_against_a_loop():
  """W in {1, 3, 32}; 33 tokens in 11 segments (nine of width 1, then 16 and 8) with lengths including 1 and full;
  without lengths; one segment; a gradient: dout / len on the first len rows, exactly 0 on the rest."""
  g = torch.Generator().manual_seed(3)
  seg = list(range(10)) + [25, 33]
  for W in (1, 3, 32):
    x = torch.randn(5, 33, W, generator=g, dtype=torch.float64)
    lens = torch.ones(5, 11, dtype=torch.int64)
    lens[:, 9] = torch.tensor([1, 16, 7, 2, 16])
    lens[:, 10] = torch.tensor([8, 1, 1, 5, 40])  # (40: clamped to the width 8)
    close(mca.segment_mean_compose(x, seg, lens), cref.segment_mean(x, seg, lens.tolist()), 1e-12, ('lens', W))
    close(mca.segment_mean_compose(x, seg, None), cref.segment_mean(x, seg, None), 1e-12, ('full', W))
    close(mca.segment_mean_compose(x, [0, 33], None), x.mean(dim=1, keepdim=True), 1e-12, ('one', W))
    close(mca.segment_mean(x, seg, lens), cref.segment_mean(x, seg, lens.tolist()), 1e-12, ('public', W))
  x = torch.randn(2, 6, 3, generator=g, dtype=torch.float64, requires_grad=True)
  dout = torch.randn(2, 2, 3, generator=g, dtype=torch.float64)
  (mca.segment_mean(x, [0, 2, 6], torch.tensor([[2, 3], [1, 4]])) * dout).sum().backward()
  want = torch.zeros(2, 6, 3, dtype=torch.float64)
  want[0, 0:2], want[0, 2:5], want[1, 0:1], want[1, 2:6] = dout[0, 0] / 2, dout[0, 1] / 3, dout[1, 0] / 1, dout[1, 1] / 4
  close(x.grad, want, 1e-12, 'gradient')
  assert torch.all(x.grad[0, 5] == 0) and torch.all(x.grad[1, 1] == 0)
  for bad in ([0, 3], [1, 6], [0, 4, 4, 6], [0, 5, 3, 6]):
    with pytest.raises(ValueError, match='tile'):
      mca.segment_mean(x, bad)


def test_a_length_of_zero_is_nan_in_its_own_segment_only():
  """0 / 0, the reference's emb_sum / count (layers/cmbf.py:311-316)."""
  x = torch.randn(3, 6, 4, generator=torch.Generator().manual_seed(1))
  lens = torch.tensor([[2, 4], [0, 4], [2, 0]])
  y = mca.segment_mean(x, [0, 2, 6], lens)
  nan = torch.isnan(y).all(dim=-1)
  assert nan.tolist() == [[False, False], [True, False], [False, True]]
  assert np.isnan(cref.segment_mean(x, [0, 2, 6], lens.tolist())[1, 0]).all()
