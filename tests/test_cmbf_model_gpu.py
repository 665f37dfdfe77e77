"""CMBF on the GPU: the cases of the reference's own run (tests/golden/cmbf_vectors.npz) with their gradients, training
steps at the sample's model section (hidden 32, 33 text tokens, 3 cross layers) against the fp64 oracle
(oracle/model_oracle.py) at first_steps' bars, steps on the grouped attention launches against steps on the one-unit
launches bit for bit, the launches a step runs, a step with the sample's sequence dropout, and evaluate()."""
import logging

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from oracle import cmbf_ref as cref  # noqa: E402
from tests import _cmbf_cases as ccases  # noqa: E402

logging.disable(logging.WARNING)
DEV = 'cuda:0'
GOLD = ccases.fixture()


@pytest.mark.parametrize('tag', sorted({k.split(':')[0] for k in GOLD.files}))
def test_fixture_cases_on_the_gpu(tag, monkeypatch):
  """Every case of tests/golden/cmbf_vectors.npz (the reference's own run) through the product on the GPU, on the
  grouped launches: towers, cross outputs, the layer output and the logits against the npz at 1e-5, and (the
  training-mode cases) the gradient of every variable the layer output depends on against the fp64 restatement's at
  1e-4, with tests/test_cmbf_pins.py's floors (cmbf_ref.grad_floor; a bias under BatchNorm is skipped)."""
  from easyrec_amd.core import context
  from tests._oracle_steps import close
  monkeypatch.setenv('EASYREC_AMD_MHA_GROUP_UNITS', '1')
  cfg, groups, training, inputs, var = ccases.fixture_case(GOLD, tag)
  vs, ctx, run = ccases.product_fixture_forward(DEV, cfg, training, inputs, var)
  W = GOLD['%s:hidden' % tag].shape[1]
  dy64 = torch.randn(6, W, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
  vs.zero_grad()
  be = kernels.hip()
  be.op_log = []
  try:
    with context.use(ctx):
      layer, hidden, logits = run()
      if training:
        (hidden * dy64.to(DEV, torch.float32)).sum().backward()
    torch.cuda.synchronize()
    names = [n for n, _ in be.op_log]
  finally:
    be.op_log = None
  # (every attention shape of the fixture leaves room for several units: all of them take the grouped launch)
  assert names.count('er::mha_group_fwd_kernel') > 0 and names.count('er::mha_fwd_kernel') == 0
  for k in ('image_tower', 'text_tower', 'image_cross', 'text_cross'):
    if '%s:%s' % (tag, k) in GOLD.files:
      close(layer.taps[k], GOLD['%s:%s' % (tag, k)], 1e-5, (tag, k))
  close(hidden, GOLD['%s:hidden' % tag], 1e-5, (tag, 'hidden'))
  close(logits, GOLD['%s:logits' % tag], 1e-5, (tag, 'logits'))
  if not training:
    return
  pr = {n: v.clone().requires_grad_(True) for n, v in var.items()}
  _, want, _ = cref.cmbf_model(pr, cfg, inputs, training)
  close(want, GOLD['%s:hidden' % tag], 1e-9, (tag, 'restated hidden'))
  (want * dy64).sum().backward()
  ref_grads = {n: p.grad for n, p in pr.items() if p.grad is not None}
  got = vs.grad_dict()
  assert len(ref_grads) > 30
  for n, g in ref_grads.items():
    if n.endswith('/bias') and (n[:-len('/bias')] + '/bn/gamma') in var:
      continue
    close(got[n], g, 1e-4, (tag, n), scale=cref.grad_floor(n, ref_grads))


# ------------------------------------------------------------------------------------------------ against the fp64 oracle
def _figures(cfg, B, seed, fused, monkeypatch):
  """tests/_oracle_steps.step_figures against the fp64 oracle: every comparison of first_steps in units of ITS bar
  (<= 1 holds it), the largest of each kind."""
  from tests._oracle_steps import step_figures, worst
  monkeypatch.setenv('EASYREC_AMD_FUSED_MHA', '1' if fused else '0')
  monkeypatch.setenv('EASYREC_AMD_MHA_GROUP_UNITS', '1')
  _, fig, compared = step_figures(cfg, B, seed, device=DEV, oracle_dtype=torch.float64)
  assert len(compared) > 40
  return worst(fig)


@pytest.mark.parametrize('kind', ['all', 'image', 'text'])
def test_first_steps_against_the_fp64_oracle(kind, monkeypatch):
  """The sample's model section (hidden 32, 33 text tokens, 3 cross layers; image only: the only_image sample's 64
  tokens through img_map_matrix), B = 64, dropouts 0, on the kernels (grouped launches) against the fp64 oracle, at
  first_steps' OWN bars (every figure <= 1 in units of its bar).  The fp32 torch composition
  (EASYREC_AMD_FUSED_MHA=0) is measured against the same oracle on the same batches and printed beside it for the
  record; it sets no bar.  Measured on one MI355X, kernels / composition, in units of the bar:
    all groups  loss 0.013 / 0.021, logits 0.26 / 0.11, gradients 0.015 / 0.016, second step's loss 0.001 / 0.001
    image only  loss 0.053 / 0.053, logits 0.96 / 0.96, gradients 0.67 / 0.68, second step's loss 0.001 / 0.003
    text only   loss 0.010 / 0.010, logits 0.08 / 0.13, gradients 0.007 / 0.012, second step's loss 0.001 / 0.001
  (Image only: 64 tokens of hidden 48 at initializer_range 0.02 pool to rows that are nearly equal across the batch, and
  final_dnn's BatchNorm divides by their spread; kernels and composition sit at the same distance from fp64.)"""
  B = 64
  cfg = ccases.cmbf_cfg(kind, batch_size=B)
  fused = _figures(cfg, B, 21, True, monkeypatch)
  comp = _figures(cfg, B, 21, False, monkeypatch)
  print('cmbf first steps vs fp64 oracle, in units of the first_steps bar:', kind, 'kernels', fused, 'composition', comp)
  for k in fused:
    assert fused[k] <= 1.0, (k, fused[k], comp[k])


# ------------------------------------------------------------------------------------------------ grouped against one-unit
def _run(cfg, B, seed, grouped, monkeypatch, steps=2):
  """`steps` training steps -> (losses per step, the first step's logits, every variable's Adam first moment after the
  first step)."""
  monkeypatch.setenv('EASYREC_AMD_FUSED_MHA', '1')
  monkeypatch.setenv('EASYREC_AMD_MHA_GROUP_UNITS', '1' if grouped else '0')
  est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=seed).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=seed + 100)
  losses, logits, slots = [], None, None
  for step in range(steps):
    est.train_step(gen.next_batch())
    losses.append(est.loss_values())
    if step == 0:
      logits = {k: v.detach().cpu().numpy().copy() for k, v in est.model._prediction_dict.items()
                if k.startswith('logits') and torch.is_tensor(v)}
      slots = {k: v for k, v in est.state_dict(slots=True).items() if k.endswith('/m')}
  return losses, logits, slots


@pytest.mark.parametrize('kind', ['all', 'text'])
def test_steps_on_the_grouped_launches_equal_steps_on_the_one_unit_launches_bit_for_bit(kind, monkeypatch):
  """EASYREC_AMD_MHA_GROUP_UNITS=1 against =0: the grouped kernels give the one-unit kernels' bits, so two training
  steps give the same losses, logits and first moments of every variable, bit for bit."""
  B = 64
  cfg = ccases.cmbf_cfg(kind, batch_size=B)
  got, got_logits, got_m = _run(cfg, B, 21, True, monkeypatch)
  exp, exp_logits, exp_m = _run(cfg, B, 21, False, monkeypatch)
  assert got == exp, (got, exp)
  assert got_logits and sorted(got_logits) == sorted(exp_logits)
  assert all(np.array_equal(got_logits[k], exp_logits[k]) for k in exp_logits)
  assert len(exp_m) > 40 and sorted(got_m) == sorted(exp_m)
  for k, want in exp_m.items():
    assert np.array_equal(got_m[k], want), k
  assert any('cross_layer_2/attention/self/key/kernel' in k or 'text_self_attention_layer_1' in k for k in exp_m)


@pytest.mark.parametrize('grouped', [True, False], ids=['grouped', 'one_unit'])
def test_the_step_runs_the_new_launches(grouped, monkeypatch):
  """One training step of cmbf_movielens' section at B = 32.  Attention launches each way: 2 text encoder layers + 3
  cross layers x 2 blocks x 2 attentions (cross, self) = 14, every shape of them with room for several units
  ((33, 33, 16): 4; (1, 33, 16), (33, 1, 16), (1, 1, 16): 8), so all 14 are grouped launches when the switch is on and
  one-unit launches when it is off.  Add & LayerNorm each way: 2 postprocessors (title, genres) + 2 x 2 in the text
  encoder + 6 blocks x 2 = 18.  Segment mean each way: 1, merge_text_embedding (the single image token's mean is a
  reshape)."""
  monkeypatch.setenv('EASYREC_AMD_FUSED_MHA', '1')
  monkeypatch.setenv('EASYREC_AMD_MHA_GROUP_UNITS', '1' if grouped else '0')
  cfg = ccases.cmbf_cfg('all', batch_size=32, seq_dropout=0.1)
  est = EasyRecEstimator(cfg, device=DEV, batch_size=32, seed=3).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=32, seed=9)
  be = kernels.hip()
  be.op_log = []
  try:
    est.train_step(gen.next_batch())
    names = [n for n, _ in be.op_log]
  finally:
    be.op_log = None
  on, off = ('er::mha_group_%s_kernel', 'er::mha_%s_kernel') if grouped else ('er::mha_%s_kernel', 'er::mha_group_%s_kernel')
  for way in ('fwd', 'bwd'):
    assert names.count(on % way) == 14 and names.count(off % way) == 0, (way, names.count(on % way), names.count(off % way))
    assert names.count('er::add_ln_%s_kernel' % way) == 18
    assert names.count('er::segment_mean_%s_kernel' % way) == 1


def test_a_step_with_sequence_dropout_and_evaluation_without():
  """text_seq_emb_dropout_prob 0.1 (the sample's): finite losses over three steps; two evaluation-mode predictions of
  one batch (`_predict_eval`, what evaluate() runs) are bit-equal; evaluate() returns an AUC."""
  B = 64
  cfg = ccases.cmbf_cfg('all', batch_size=B, seq_dropout=0.1)
  est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=5).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=105)
  for _ in range(3):
    est.train_step(gen.next_batch())
    assert all(np.isfinite(v) for v in est.loss_values().values()), est.loss_values()
  b = gen.next_batch()
  outs = [{k: v.detach().clone() for k, v in pred.items() if torch.is_tensor(v)} for _, pred in est._predict_eval([b, b])]
  assert outs[0] and all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])
  res = est.evaluate([gen.next_batch() for _ in range(3)])
  assert 'auc' in res and 0.0 <= float(res['auc']) <= 1.0, res
