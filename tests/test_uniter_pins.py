"""The BERT-style encoder layer (easyrec_amd/layers/multihead_cross_attention.py) on the CPU: the torch composition on
the stand-in backend against the fp64 restatement (oracle/uniter_ref.py), the reference's variable names, the mask and
the 1 / sqrt(ds) scaling, and the Python mirror of the K8f kernels' envelope against the library."""
import math

import numpy as np
import pytest
import torch

from easyrec_amd.core import context
from easyrec_amd.layers import multihead_cross_attention as mca
from oracle import uniter_ref as ref
from tests import _uniter_cases as cases
from tests._oracle_steps import close


_mask = ref.mixed_mask
_encoder = cases.product_encoder


def test_envelope_formula_is_the_library_s(built_lib):
  from easyrec_amd import kernels
  be = kernels.HipBackend()
  for F, T, ds in [(33, 33, 128), (9, 9, 7), (1, 17, 8), (16, 8, 16), (5, 1, 1), (64, 64, 128), (40, 33, 128), (33, 200, 16)]:
    for bwd in (False, True):
      assert be.mha_lds_bytes(F, T, ds, bwd) == mca.lds_bytes(F, T, ds, bwd), (F, T, ds, bwd)
  assert be.mha_lds_bytes(0, 3, 4) == 0 == mca.lds_bytes(0, 3, 4)
  assert mca.lds_bytes(33, 33, 128) == 76956 and mca.LDS_BUDGET == be.MHA_LDS_BUDGET
  assert mca.fits(33, 33, 128) and mca.fits(1, 1, 1) and mca.fits(16, 8, 16)
  assert not mca.fits(64, 64, 128) and not mca.fits(4, 4, 129) and not mca.fits(0, 4, 8)
  # a length past 4096 is outside the envelope although its LDS figure is inside: the library refuses it (a host check,
  # before any launch), and the layer takes the composition
  assert mca.lds_bytes(4097, 1, 1) <= mca.LDS_BUDGET and mca.lds_bytes(5000, 1, 1) <= mca.LDS_BUDGET
  assert mca.fits(4096, 1, 1) and not mca.fits(4097, 1, 1) and not mca.fits(1, 4097, 1)
  import ctypes
  host = ctypes.addressof(ctypes.create_string_buffer(16))  # (non-null; the shape is refused before anything reads it)
  for F, T in ((4097, 1), (1, 4097)):
    with pytest.raises(RuntimeError, match='outside the envelope'):
      be.ck.er_mha_fwd(host, 1, host, 1, host, 1, None, 1, F, T, 1, 1, host, None)
  assert be.add_ln_grid(5, 4096) == 2 and be.add_ln_grid(10 ** 6, 512) == 1024 and be.add_ln_grid(1, 1) == 1
  assert be.add_ln_grid(8, 4097) == 0 and be.add_ln_grid(0, 8) == 0
  assert mca.LN_MAX_WIDTH == be.ADD_LN_MAX_W == 4096 and mca.MAX_HEAD_SIZE == be.MHA_MAX_DS


def test_scores_are_multiplied_by_the_inverse_root_of_the_head_size():
  """S = Q K^T * (1 / sqrt(ds)) (:191-193), the counterpart of AutoInt's S = Q K^T * sqrt(ds): with one-hot values the
  output shows the softmax of q . k / 2 at ds = 4, in the restatement and in the product's composition."""
  ds = 4
  q = torch.tensor([[3.0, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.float64)
  k = torch.tensor([[1.0, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.float64)
  v = torch.tensor([[1.0, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.float64)
  s = 3.0 / 2.0
  want = math.exp(s) / (math.exp(s) + 1.0)
  assert abs(float(ref.attention_core(q, k, v, None, 1, 2, 2, 1, ds)[0, 0]) - want) < 1e-12
  with context.use(context.ModelContext(None, None, is_training=False)):
    got = mca.attention_compose(q, k, v, None, 1, 2, 2, 1, ds)
  assert abs(float(got[0, 0]) - want) < 1e-12


def test_the_mask_adds_minus_ten_thousand_and_an_all_masked_row_is_the_unmasked_softmax():
  """(1 - mask) * -10000 is a finite adder: a masked key gets probability exp(-10000 + ..) = 0 beside an open one, and a
  row whose keys are ALL masked is the softmax of its scores.  The fp32 composition must hold the fp64 restatement's
  bar (1e-5) on exactly that input: it applies the adder relative to the row's largest adder."""
  B, F, T, H, ds = 3, 5, 6, 2, 8
  g = torch.Generator().manual_seed(11)
  q, k, v = (torch.randn(B * n, H * ds, generator=g, dtype=torch.float64) for n in (F, T, T))
  mask = _mask(B, T, 2)
  assert int(mask[1].sum()) == 0 and int(mask[0].sum()) == 1
  want = ref.attention_core(q, k, v, mask, B, F, T, H, ds)
  free = ref.attention_core(q, k, v, None, B, F, T, H, ds)
  close(want.reshape(B, F, -1)[1], free.reshape(B, F, -1)[1], 1e-9, 'all masked = unmasked')
  v1 = v.reshape(B, T, H * ds)[0, T // 2]
  close(want.reshape(B, F, -1)[0], v1.expand(F, -1), 1e-12, 'a single open key')
  with context.use(context.ModelContext(None, None, is_training=False)):
    got = mca.attention_compose(q.float(), k.float(), v.float(), mask, B, F, T, H, ds)
    got3 = mca.attention_compose(q.float(), k.float(), v.float(), mca.create_attention_mask_from_input_mask(
        torch.zeros(B, F, 1), mask).contiguous(), B, F, T, H, ds)
  close(got, want, 1e-5, 'composition, [B, T] mask')
  close(got3, want, 1e-5, 'composition, [B, F, T] mask')
  m3 = mca.create_attention_mask_from_input_mask(torch.zeros(B, F, 1), mask)
  assert tuple(m3.shape) == (B, F, T) and m3.dtype == mask.dtype and m3.stride(1) == 0
  assert torch.equal(mca._row_mask(m3, B, F, T), mask)
  assert mca._row_mask(m3.contiguous(), B, F, T) is None  # (a mask of its own per query row: the composition)


@pytest.mark.parametrize('act', ['gelu', 'tanh', 'swish', 'relu'])
def test_encoder_on_the_stand_in_matches_the_restatement(ref_backend, act):
  """Variable names and shapes are the reference's; the forward and every gradient match the fp64 restatement."""
  B, S, hidden, H, layers, inter = 6, 9, 12, 3, 2, 10
  params = ref.random_encoder_params('uniter', layers, hidden, inter, seed=5)
  x64 = torch.randn(B, S, hidden, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
  mask = _mask(B, S, 3)
  x = x64.float().requires_grad_(True)
  vs, ctx = cases.product_store('cpu', lambda: _encoder(x.detach(), mask, H, layers, inter, act), params)
  assert vs.names() == ref.encoder_variable_names('uniter', layers)
  assert all(vs.l2_of(n) == 0.0 for n in vs.names())  # (the encoder's dense layers carry no regulariser)
  dy = torch.randn(B, S, hidden, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
  with context.use(ctx):
    y = _encoder(x, mask, H, layers, inter, act)
    y.backward(dy.float())
  xr = x64.clone().requires_grad_(True)
  pr = {n: p.clone().requires_grad_(True) for n, p in params.items()}
  want = ref.transformer_encoder(xr, mask, pr, 'uniter', layers, H, act)
  (want * dy).sum().backward()
  close(y, want, 1e-5, 'encoder output')
  close(x.grad, xr.grad, 1e-4, 'dx')
  ref_grads = {n: p.grad for n, p in pr.items()}
  for n, g in vs.grad_dict().items():
    close(g, ref_grads[n], 1e-4, n, scale=ref.grad_floor(n, ref_grads))


def test_initializers_are_the_reference_s(ref_backend):
  """Kernels: truncated normal with stddev initializer_range (nothing beyond 2 sigma); biases and beta zeros, gamma ones."""
  x = torch.randn(2, 5, 64)
  vs, _ = cases.product_store('cpu', lambda: mca.transformer_encoder(
      x, None, hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256, initializer_range=0.03))
  st = vs.state_dict()
  for n, v in st.items():
    if n.endswith('/kernel'):
      assert np.abs(v).max() <= 2 * 0.03 + 1e-7 and 0.02 < v.std() < 0.03, n
    elif n.endswith('/gamma'):
      assert np.all(v == 1.0)
    else:
      assert np.all(v == 0.0), n


def test_postprocessor_names_numbering_and_values(ref_backend):
  """token_type/<name> and position_embedding/<name>; unnamed layer norms are LayerNorm, LayerNorm_1, .. in call order
  inside default_scopes(); token-type ids as an int, per position and per token give the restatement's values and
  gradients."""
  B, S, W, V = 4, 5, 8, 3
  g = torch.Generator().manual_seed(4)
  xa, xb = (torch.randn(B, S, W, generator=g, dtype=torch.float64) for _ in range(2))
  ids_b = torch.randint(0, V, (B, S), generator=g)

  def forward(a, b):
    with mca.default_scopes():
      ya = mca.embedding_postprocessor(a, use_token_type=True, token_type_ids=2, token_type_vocab_size=V,
                                       use_position_embeddings=False)
      yb = mca.embedding_postprocessor(b, use_token_type=True, token_type_ids=ids_b, token_type_vocab_size=V,
                                       use_position_embeddings=True, position_embedding_name='txt_position_embeddings_0',
                                       max_position_embeddings=7)
    return ya, yb

  vs, ctx = cases.product_store('cpu', lambda: forward(xa.float(), xb.float()))
  assert vs.names() == ['token_type/token_type_embeddings', 'LayerNorm/beta', 'LayerNorm/gamma',
                        'position_embedding/txt_position_embeddings_0', 'LayerNorm_1/beta', 'LayerNorm_1/gamma']
  assert vs.state_dict()['position_embedding/txt_position_embeddings_0'].shape == (7, W)
  params = {n: torch.randn(v.shape, generator=g, dtype=torch.float64) for n, v in vs.state_dict().items()}
  vs, ctx = cases.product_store('cpu', lambda: forward(xa.float(), xb.float()), params)
  a, b = xa.float().requires_grad_(True), xb.float().requires_grad_(True)
  with context.use(ctx):
    ya, yb = forward(a, b)
    ((ya * ya).sum() + (yb * yb).sum()).backward()
  pr = {n: p.clone().requires_grad_(True) for n, p in params.items()}
  ar, br = xa.clone().requires_grad_(True), xb.clone().requires_grad_(True)
  wa = ref.embedding_postprocessor(ar, pr, 'LayerNorm', torch.full((S,), 2), 'token_type/token_type_embeddings')
  wb = ref.embedding_postprocessor(br, pr, 'LayerNorm_1', ids_b, 'token_type/token_type_embeddings',
                                   'position_embedding/txt_position_embeddings_0')
  ((wa * wa).sum() + (wb * wb).sum()).backward()
  close(ya, wa, 1e-5, 'ya')
  close(yb, wb, 1e-5, 'yb')
  close(b.grad, br.grad, 1e-4, 'dxb')
  for n, gr in vs.grad_dict().items():
    close(gr, pr[n].grad, 1e-4, n)
  with pytest.raises(ValueError, match='max_position_embeddings'):
    with context.use(ctx):
      mca.embedding_postprocessor(b, use_position_embeddings=True, max_position_embeddings=S - 1)


def test_dropout_runs_only_while_training(ref_backend):
  """Hidden and attention dropout change the output of a training pass; outside training two passes are bit-equal and
  equal the pass without dropout."""
  x = torch.randn(4, 6, 8, generator=torch.Generator().manual_seed(3))

  def enc(hidden_p, att_p):
    return mca.transformer_encoder(x, None, hidden_size=8, num_hidden_layers=1, num_attention_heads=2,
                                   intermediate_size=8, hidden_dropout_prob=hidden_p,
                                   attention_probs_dropout_prob=att_p, initializer_range=0.5)

  vs, ctx = cases.product_store('cpu', lambda: enc(0.0, 0.0))
  with context.use(ctx), torch.no_grad():
    plain = enc(0.0, 0.0)
    torch.manual_seed(1)
    assert not torch.equal(enc(0.5, 0.0), plain) and not torch.equal(enc(0.0, 0.5), plain)
    ctx.is_training = False
    assert torch.equal(enc(0.5, 0.5), plain) and torch.equal(enc(0.5, 0.5), plain)


def test_the_switch_and_the_stand_in_take_the_composition(ref_backend, monkeypatch):
  x = torch.zeros(2, 3, 8)
  assert not mca._fused(x)  # (a CPU tensor on the stand-in backend)
  monkeypatch.setenv('EASYREC_AMD_FUSED_MHA', '0')
  assert not mca.fused_enabled()
  monkeypatch.setenv('EASYREC_AMD_FUSED_MHA', '1')
  assert mca.fused_enabled()
  with pytest.raises(ValueError, match='multiple'):
    mca.transformer_encoder(x, hidden_size=8, num_attention_heads=3)
  with pytest.raises(ValueError, match='hidden size'):
    mca.transformer_encoder(x, hidden_size=16, num_attention_heads=4)
