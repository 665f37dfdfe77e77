"""The sequence-combiner HIP kernels (csrc/er_seq_combine.hip) on the GPU: forward and every gradient against the fp64
torch restatement (oracle/seq_combiner_ref.py) with the column read at a pitch from inside a wider buffer, the max's
tie rule, the composed path (outside the envelope, switch off, another activation, no padding), path selection,
bit-identity (two runs, eager vs hipGraph replay), the models against the test-side oracle, and evaluate()."""
import logging
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.layers.keras import text_cnn as tc  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from oracle import seq_combiner_ref as sref  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402
from tests._oracle_steps import close as _close  # noqa: E402
from tests.test_seq_combiner_pins import (GOLD, GOLD_CNN, NEAR_TIE_CAP, PATTERN_TOL, POOL_CASES,  # noqa: E402
                                          TEXT_CNN_CASES, case_id, gold_cnn, gold_conv_params, gold_mlp, random_pool,
                                          random_text_cnn, steps_against_the_oracle)

logging.disable(logging.WARNING)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
PAD_LEFT, PAD_RIGHT = 3, 2  # columns beside the sequence column in the wider buffer
SENTINEL = 7.5


def _wide(x64):
  """x [B, L, D] as a column view at offset PAD_LEFT of a [B, L, PAD_LEFT + D + PAD_RIGHT] buffer."""
  B, L, D = x64.shape
  buf = torch.full((B, L, PAD_LEFT + D + PAD_RIGHT), SENTINEL, dtype=torch.float32, device=DEV)
  buf[:, :, PAD_LEFT:PAD_LEFT + D] = x64.to(DEV, torch.float32)
  return buf, buf[:, :, PAD_LEFT:PAD_LEFT + D]


def _neighbours_untouched(dbuf, D):
  assert bool((dbuf[:, :, :PAD_LEFT] == SENTINEL).all()) and bool((dbuf[:, :, PAD_LEFT + D:] == SENTINEL).all()), \
      'the backward wrote outside its column'


# ---------------------------------------------------------------------------------------- TextCNN
def _check_text_cnn(case, x64, ks64, bs64, seed=3, min_near=0, cap=NEAR_TIE_CAP):
  B, L, P, D, sizes, filters, act = case
  be = kernels.hip()
  assert tc.text_cnn_fits(P, D, sizes, filters) and be.text_cnn_epb(P, D, sizes, filters) > 0
  SF = sum(filters)
  params = [t.to(DEV, torch.float32) for pair in zip(ks64, bs64) for t in pair]
  theta = torch.cat([p.reshape(-1) for p in params])
  _, x = _wide(x64)
  # forward into a wider output buffer, with the selection the backward will use
  ybuf = torch.full((B, SF + 3), SENTINEL, dtype=torch.float32, device=DEV)
  y, sel = be.text_cnn_fwd(x, theta, P, sizes, filters, act == 'relu', out=ybuf[:, 1:1 + SF], want_sel=True)
  d64 = torch.randn(B, SF, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
  grads = [torch.zeros_like(p) for p in params]
  dbuf, dx = _wide(torch.full_like(x64, SENTINEL))  # (every position of the column must be written)
  be.text_cnn_bwd(x, theta, d64.to(DEV, torch.float32), P, sizes, filters, act == 'relu', kernels.ThetaGradTable(grads),
                  acc=True, dx=dx)
  torch.cuda.synchronize()
  assert bool((ybuf[:, 0] == SENTINEL).all()) and bool((ybuf[:, 1 + SF:] == SENTINEL).all())
  _neighbours_untouched(dbuf, D)
  # the oracle: fp64's own arg-max, except where its top two candidates (or the maximum and 0 under relu) lie within
  # PATTERN_TOL: there, under the kernel's own selection
  near = sref.near_ties(x64, P, ks64, bs64, act, PATTERN_TOL)
  share = float(near.double().mean())
  print('text_cnn %s: %d of %d outputs near a tie (%.3f %%)' % (case_id(case), int(near.sum()), near.numel(), 100 * share))
  assert share <= cap and int(near.sum()) >= min_near
  bits = sel.cpu()
  n_max = P - min(sizes) + 1
  weight = ((bits[:, :, None] >> torch.arange(n_max)[None, None, :]) & 1).double()
  assert bool((weight.sum(dim=-1) >= 1).all())
  weight = weight / weight.sum(dim=-1, keepdim=True)
  active = (y.cpu() > 0) if act == 'relu' else torch.ones(B, SF, dtype=torch.bool)
  xr = x64.clone().requires_grad_(True)
  kr = [k.clone().requires_grad_(True) for k in ks64]
  br = [b.clone().requires_grad_(True) for b in bs64]
  exp = sref.text_cnn_ref(x64, P, ks64, bs64, act)
  (sref.text_cnn_ref(xr, P, kr, br, act, select=(near, weight, active)) * d64).sum().backward()
  _close(y, exp, 1e-5, 'forward')
  _close(dx, xr.grad, 1e-4, 'dx')
  for i, (gk, gb) in enumerate(zip(grads[0::2], grads[1::2])):
    _close(gk, kr[i].grad, 1e-4, 'dkernel_%d' % i)
    _close(gb, br[i].grad, 1e-4, 'dbias_%d' % i)
  return y


@pytest.mark.parametrize('case', TEXT_CNN_CASES, ids=case_id)
def test_text_cnn_matches_the_fp64_restatement(case):
  x64, ks64, bs64 = random_text_cnn(case)
  _check_text_cnn(case, x64, ks64, bs64)


def test_text_cnn_shares_the_gradient_of_a_tied_max_evenly():
  """Two identical windows and an all-padding tail: each tied position takes dy / ties (TensorFlow's reduce_max); the
  bias takes the whole dy.  Example 0: windows 0 and 2 hold the same values and win filter 0; example 1 is all zeros
  (every window of every filter is the bias: P - k + 1 ties); filter 1's bias wins everywhere over the padding tail."""
  case = (2, 4, 6, 3, [2], [2], 'linear')
  x64 = torch.randn(2, 4, 3, generator=torch.Generator().manual_seed(5)).float().double()
  x64[0, 2:] = x64[0, :2]
  x64[1] = 0.0
  w = torch.zeros(2, 3, 2, dtype=torch.float64)
  w[:, :, 0] = x64[0, :2]
  w[:, :, 1] = -x64[0, :2] * 0.01
  b = torch.tensor([0.5, 100.0], dtype=torch.float64)
  be = kernels.hip()
  x = x64.to(DEV, torch.float32)
  params = [w.to(DEV, torch.float32), b.to(DEV, torch.float32)]
  theta = torch.cat([p.reshape(-1) for p in params])
  y, sel = be.text_cnn_fwd(x, theta, 6, [2], [2], False, want_sel=True)
  dy = torch.tensor([[2.0, 4.0], [1.0, 0.0]], dtype=torch.float64)
  grads = [torch.zeros_like(p) for p in params]
  dx = be.text_cnn_bwd(x, theta, dy.to(DEV, torch.float32), 6, [2], [2], False, kernels.ThetaGradTable(grads))
  torch.cuda.synchronize()
  assert int(sel[0, 0]) == 0b00101 and int(sel[1, 0]) == 0b11111  # (example 0: windows 0 and 2; example 1: all five)
  xr, wr, br = (t.clone().requires_grad_(True) for t in (x64, w, b))
  (sref.text_cnn_ref(xr, 6, [wr], [br], 'linear') * dy).sum().backward()  # (torch.amax: the same rule)
  _close(dx, xr.grad, 1e-5, 'dx with ties')
  _close(grads[0], wr.grad, 1e-5, 'dkernel with ties')
  assert torch.allclose(grads[1].cpu().double(), dy.sum(dim=0))  # (the bias gradient is the full dy)


@pytest.mark.parametrize('tag', GOLD_CNN)
def test_kernels_match_the_reference_fixture(tag):
  pb, x64, lens, var, want = gold_cnn(tag)
  ks64, bs64 = gold_conv_params(pb, var)
  B, L, D = x64.shape
  case = (B, L, int(pb.pad_sequence_length), D, [int(k) for k in pb.filter_sizes], [int(f) for f in pb.num_filters],
          pb.activation)
  # (six examples with zero rows from their length on: windows that lie wholly in the padding are EXACT ties, in fp64
  #  and in fp32 alike, and a single one of them is 2.4 % of a case's 42 outputs: the seeded cases' cap does not apply)
  y = _check_text_cnn(case, x64, ks64, bs64, seed=7, cap=1.0)
  if pb.HasField('mlp'):  # (the kernel's pooled output through the fixture's own mlp)
    y = gold_mlp(pb, var, y.double().cpu())
  _close(y, want, 1e-5, tag)


def test_attention_kernel_matches_the_reference_fixture():
  be = kernels.hip()
  x64, lens = torch.from_numpy(GOLD['input_layer:x:hist']), torch.from_numpy(GOLD['input_layer:len:hist'])
  w64 = torch.from_numpy(GOLD['input_layer:var:hist_embedding/attention/kernel'])
  y = be.seq_attn_pool_fwd(x64.to(DEV, torch.float32), lens.to(DEV, torch.int32), w64.reshape(-1).to(DEV, torch.float32))
  _close(y, GOLD['input_layer:out'][:, :4], 1e-5, 'attention')


# ---------------------------------------------------------------------------------------- attention pooling
@pytest.mark.parametrize('case', POOL_CASES, ids=lambda c: 'B%d_L%d_D%d' % c)
def test_attention_pooling_matches_the_fp64_restatement(case):
  B, L, D = case
  be = kernels.hip()
  assert tc.seq_attn_pool_fits(L, D) and be.seq_attn_pool_epb(L, D) > 0
  x64, lens, w64 = random_pool(case)
  _, x = _wide(x64)
  lens32 = lens.to(DEV, torch.int32)
  w = w64.to(DEV, torch.float32)
  y = be.seq_attn_pool_fwd(x, lens32, w)
  d64 = torch.randn(B, D, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
  gw = [torch.zeros_like(w)]
  dbuf, dx = _wide(torch.full_like(x64, SENTINEL))  # (every position of the column must be written)
  be.seq_attn_pool_bwd(x, lens32, w, d64.to(DEV, torch.float32), kernels.ThetaGradTable(gw), acc=True, dx=dx)
  torch.cuda.synchronize()
  _neighbours_untouched(dbuf, D)
  xr, wr = x64.clone().requires_grad_(True), w64.clone().requires_grad_(True)
  exp = sref.seq_attn_pool_ref(xr, lens, wr)
  (exp * d64).sum().backward()
  _close(y, exp, 1e-5, 'forward')
  assert float(y[lens32 == 0].abs().max() if bool((lens == 0).any()) else 0.0) == 0.0  # (a row of length 0 pools to 0)
  _close(dx, xr.grad, 1e-4, 'dx')
  _close(gw[0], wr.grad, 1e-4, 'dw')


# ---------------------------------------------------------------------------------------- path selection
# what takes the composition: another activation, no padding, a geometry outside the envelope (P = 70; the switch off
# runs the same function)
COMPOSED_CASES = [
    (13, 5, 7, 5, [2, 3], [3, 2], 'tanh'),
    (13, 9, 0, 5, [2, 3], [3, 2], 'relu'),
    (13, 20, 70, 5, [2, 3], [3, 2], 'relu'),
]


@pytest.mark.parametrize('case', COMPOSED_CASES, ids=case_id)
def test_the_composition_passes_the_same_checks_on_the_gpu(case):
  B, L, P, D, sizes, filters, act = case
  assert act == 'tanh' or P <= 0 or not tc.text_cnn_fits(P, D, sizes, filters)
  x64, ks64, bs64 = random_text_cnn(case)
  _, x = _wide(x64)
  x.requires_grad_(True)
  ps = [t.to(DEV, torch.float32).requires_grad_(True) for t in ks64 + bs64]
  out = tc.text_cnn_compose(x, P, ps[:len(ks64)], ps[len(ks64):], act)
  d64 = torch.randn(out.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
  gs = torch.autograd.grad(out, [x] + ps, d64.to(DEV, torch.float32))
  xr = [t.clone().requires_grad_(True) for t in [x64] + ks64 + bs64]
  exp = sref.text_cnn_ref(xr[0], P, xr[1:1 + len(ks64)], xr[1 + len(ks64):], act)
  (exp * d64).sum().backward()
  _close(out, exp, 1e-5, 'forward')
  for g, r, what in zip(gs, xr, ['dx'] + ['dkernel'] * len(ks64) + ['dbias'] * len(bs64)):
    _close(g, r.grad, 1e-4, what)


def _kernel_calls_of_one_step(cfg, monkeypatch):
  calls = []
  for fn, tag in ((kernels.TextCnnFn, 'text_cnn'), (kernels.SeqAttnPoolFn, 'attention')):
    monkeypatch.setattr(fn, 'apply', (lambda real, tag: lambda *a: calls.append(tag) or real(*a))(fn.apply, tag))
  B = 32
  est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=3).build()
  del calls[:]  # (the build pass)
  est.train_step(SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=5).next_batch())
  return calls


def test_the_layers_pick_the_path_by_the_envelope(monkeypatch):
  from tests.test_seq_combiner_pins import _feature, model_cfg
  monkeypatch.setenv('EASYREC_AMD_FUSED_SEQ_COMBINE', '1')
  assert _kernel_calls_of_one_step(model_cfg('deepfm_textcnn', 32), monkeypatch) == ['text_cnn']
  assert _kernel_calls_of_one_step(model_cfg('deepfm_attention', 32), monkeypatch) == ['attention', 'attention']
  assert _kernel_calls_of_one_step(model_cfg('backbone_textcnn', 32), monkeypatch) == ['text_cnn']
  assert _kernel_calls_of_one_step(model_cfg('deepfm_no_pad', 32), monkeypatch) == []       # no padding
  cfg = model_cfg('deepfm_textcnn', 32)
  _feature(cfg, 'title').sequence_combiner.text_cnn.activation = 'tanh'
  assert _kernel_calls_of_one_step(cfg, monkeypatch) == []                                  # another activation
  cfg = model_cfg('deepfm_textcnn', 32)
  _feature(cfg, 'title').sequence_combiner.text_cnn.pad_sequence_length = 70
  assert _kernel_calls_of_one_step(cfg, monkeypatch) == []                                  # outside the envelope
  monkeypatch.setenv('EASYREC_AMD_FUSED_SEQ_COMBINE', '0')
  assert _kernel_calls_of_one_step(model_cfg('deepfm_textcnn', 32), monkeypatch) == []      # the switch
  assert _kernel_calls_of_one_step(model_cfg('deepfm_attention', 32), monkeypatch) == []


def test_two_runs_and_graph_replay_are_bit_identical():
  be = kernels.hip()
  case = (1001, 14, 14, 16, [2, 3, 4], [8, 4, 4], 'relu')
  x64, ks64, bs64 = random_text_cnn(case)
  x = x64.to(DEV, torch.float32)
  params = [t.to(DEV, torch.float32) for pair in zip(ks64, bs64) for t in pair]
  theta = torch.cat([p.reshape(-1) for p in params])
  dy = torch.randn(1001, 16, device=DEV)
  px64, lens, w64 = random_pool((1001, 50, 16))
  px, plens, pw = px64.to(DEV, torch.float32), lens.to(DEV, torch.int32), w64.to(DEV, torch.float32)
  table = kernels.ThetaGradTable([torch.zeros_like(p) for p in params])
  ptable = kernels.ThetaGradTable([torch.zeros_like(pw)])

  def run():
    y = be.text_cnn_fwd(x, theta, 14, case[4], case[5], True)
    dx = be.text_cnn_bwd(x, theta, dy, 14, case[4], case[5], True, table, acc=False)
    py = be.seq_attn_pool_fwd(px, plens, pw)
    pdx = be.seq_attn_pool_bwd(px, plens, pw, dy, ptable, acc=False)
    return [y, dx, py, pdx] + [g.clone() for g in table.grads + ptable.grads]
  assert_runs_and_replay_bit_identical(run)


# ---------------------------------------------------------------------------------------- the models
@pytest.mark.parametrize('kind', ['deepfm_textcnn', 'deepfm_attention', 'backbone_mlp', 'backbone_textcnn',
                                  'backbone_textcnn_bn'])
def test_model_matches_the_oracle(kind, monkeypatch):
  """B = 128, small tables, at first_steps' bars against the test-side fp64 oracle: every loss key, the logits, the
  first moment of every variable - the convolution kernels, `attention` and the sequence tables among them (coverage)."""
  monkeypatch.setenv('EASYREC_AMD_FUSED_SEQ_COMBINE', '1')
  calls = []
  for fn in (kernels.TextCnnFn, kernels.SeqAttnPoolFn):
    real = fn.apply
    monkeypatch.setattr(fn, 'apply', (lambda real: lambda *a: calls.append(1) or real(*a))(real))
  steps_against_the_oracle(kind, 128, 4, DEV)
  assert calls, 'the model did not run the sequence-combiner kernels'


def test_evaluate_returns_an_auc():
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'deepfm_textcnn_movielens.config'))
  B = 256
  est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=3).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=5)
  for _ in range(2):
    est.train_step(gen.next_batch())
  res = est.evaluate([gen.next_batch() for _ in range(2)])
  assert 'auc' in res and 0.0 <= float(res['auc']) <= 1.0, res
