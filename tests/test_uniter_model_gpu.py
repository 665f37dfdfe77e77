"""Uniter and DBMTL.bottom_uniter on the GPU: training steps at the sample's model section (hidden 512, 33 tokens)
against the fp64 oracle (oracle/model_oracle.py) at first_steps' bars, the cases of the reference's own run
(tests/golden/uniter_vectors.npz) with their gradients, the kernels against the torch composition
(EASYREC_AMD_FUSED_MHA=0) at the same bars, the launches a step runs, a step with hidden dropout, and evaluate()."""
import logging

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from oracle import uniter_ref as ref  # noqa: E402
from tests import _uniter_cases as cases  # noqa: E402

logging.disable(logging.WARNING)
DEV = 'cuda:0'


def _run(cfg, B, seed, fused, monkeypatch, steps=2):
  """`steps` training steps -> (losses per step, the first step's logits, every variable's Adam first moment after the
  first step, the names of the launches logged during the first step)."""
  monkeypatch.setenv('EASYREC_AMD_FUSED_MHA', '1' if fused else '0')
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


@pytest.mark.parametrize('kind,dbmtl', [('all', False), ('text', False), ('all', True)], ids=['all', 'text', 'dbmtl'])
def test_steps_on_the_kernels_match_the_composition(kind, dbmtl, monkeypatch):
  """first_steps' bars between the two paths: losses 1e-5 (first step) / 1e-4 (second), logits rtol 1e-4 / atol 1e-5,
  every variable's gradient (Adam's first moment) within 2e-4 of its scale + 2e-6 of the largest."""
  B = 128
  cfg = cases.uniter_cfg(kind, batch_size=B, hidden=512, heads=4, layers=2, hidden_dropout=0.0, dbmtl=dbmtl)
  got, got_logits, got_m = _run(cfg, B, 21, True, monkeypatch)
  exp, exp_logits, exp_m = _run(cfg, B, 21, False, monkeypatch)
  for step in range(2):
    assert sorted(got[step]) == sorted(exp[step])
    for k in exp[step]:
      assert abs(got[step][k] - exp[step][k]) <= (1e-5 if step == 0 else 1e-4) * max(1e-3, abs(exp[step][k])), \
          (step, k, got[step][k], exp[step][k])
  assert got_logits and sorted(got_logits) == sorted(exp_logits)
  for k in exp_logits:
    assert np.allclose(got_logits[k], exp_logits[k], rtol=1e-4, atol=1e-5), k
  gmax = max(float(np.abs(v).max()) for v in exp_m.values())
  compared = 0
  for k, want in exp_m.items():
    d, scale = float(np.abs(got_m[k] - want).max()), float(np.abs(want).max())
    assert d <= 2e-4 * scale + 2e-6 * gmax, (k, d, scale)
    compared += 1
  assert compared > 40 and any('uniter_layer_1/attention/self/key/kernel' in k for k in exp_m)
  assert any(k.startswith('input_layer/') for k in exp_m)


def test_the_step_runs_the_new_launches():
  cfg = cases.uniter_cfg('all', batch_size=32, hidden=64, heads=4, layers=2)
  est = EasyRecEstimator(cfg, device=DEV, batch_size=32, seed=3).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=32, seed=9)
  be = kernels.hip()
  be.op_log = []
  try:
    est.train_step(gen.next_batch())
    names = [n for n, _ in be.op_log]
  finally:
    be.op_log = None
  # two layers: an attention launch each way per layer; four postprocessor and four encoder add & LayerNorm launches
  assert names.count('er::mha_fwd_kernel') == 2 and names.count('er::mha_bwd_kernel') == 2
  assert names.count('er::add_ln_fwd_kernel') == 8 and names.count('er::add_ln_bwd_kernel') == 8


def test_a_step_with_hidden_dropout_and_evaluation_without():
  """hidden_dropout_prob 0.1 (the sample's): finite losses over three steps; two evaluation-mode predictions of one batch
  are bit-equal (no dropout outside training); evaluate() returns an AUC.  The predictions go through `_predict_eval`
  (is_training False, what evaluate() runs) and not through two plain predict() calls: predict() on an estimator built
  for training keeps the training flags, for every model of this project."""
  B = 128
  cfg = cases.uniter_cfg('all', batch_size=B, hidden=512, heads=4, layers=2, hidden_dropout=0.1)
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


# ------------------------------------------------------------------------------------------------ against the fp64 oracle
def _figures(cfg, B, seed, fused, monkeypatch):
  """tests/_oracle_steps.step_figures against the fp64 oracle: every comparison of first_steps in units of ITS bar
  (<= 1 holds it), the largest of each kind."""
  from tests._oracle_steps import step_figures, worst
  monkeypatch.setenv('EASYREC_AMD_FUSED_MHA', '1' if fused else '0')
  _, fig, compared = step_figures(cfg, B, seed, device=DEV, oracle_dtype=torch.float64)
  assert len(compared) > 40
  return worst(fig)


@pytest.mark.parametrize('kind,dbmtl', [('all', False), ('text', False), ('all', True)], ids=['all', 'text', 'dbmtl'])
def test_first_steps_against_the_fp64_oracle(kind, dbmtl, monkeypatch):
  """The sample's model section (hidden 512, 33 / 25 tokens, initializer_range 0.02), B = 128, dropouts 0, on the
  kernels against the fp64 oracle, at first_steps' OWN bars (every figure <= 1 in units of its bar).  The fp32 torch
  composition (EASYREC_AMD_FUSED_MHA=0) is measured against the same oracle on the same batches and printed beside it
  for the record; it sets no bar.  Measured on one MI355X, kernels / composition, in units of the bar:
    all groups  loss 0.005 / 0.005, logits 0.36 / 0.19, gradients 0.015 / 0.017, second step's loss 0.002 / 0.001
    text only   loss 0.025 / 0.036, logits 0.49 / 0.69, gradients 0.047 / 0.036, second step's loss 0.010 / 0.003
    DBMTL       loss 0.099 / 0.176, logits 0.79 / 0.74, gradients 0.054 / 0.049, second step's loss 0.007 / 0.027"""
  B = 128
  cfg = cases.uniter_cfg(kind, batch_size=B, hidden=512, heads=4, layers=2, hidden_dropout=0.0, dbmtl=dbmtl)
  fused = _figures(cfg, B, 21, True, monkeypatch)
  comp = _figures(cfg, B, 21, False, monkeypatch)
  print('uniter first steps vs fp64 oracle, in units of the first_steps bar:', kind, dbmtl, 'kernels', fused,
        'composition', comp)
  for k in fused:
    assert fused[k] <= 1.0, (k, fused[k], comp[k])


# ------------------------------------------------------------------------------------------------ the reference's fixture
GOLD = cases.fixture()


@pytest.mark.parametrize('tag', sorted({k.split(':')[0] for k in GOLD.files}))
def test_fixture_cases_on_the_gpu(tag):
  """Every case of tests/golden/uniter_vectors.npz (the reference's own run) through the product on the GPU: the layer
  output and the logits against the npz at 1e-5, and the gradient of every variable the [CLS] feature depends on
  against the fp64 restatement's at 1e-4 (the training-mode cases: in evaluation mode the dense layers run without
  autograd and there is no gradient to compare)."""
  from easyrec_amd.core import context
  from tests._oracle_steps import close
  cfg, groups, training, inputs, var = cases.fixture_case(GOLD, tag)
  vs, ctx, run = cases.product_fixture_forward(DEV, cfg, training, inputs, var)
  H = cfg.model_config.uniter.config.hidden_size
  dy64 = torch.randn(6, H, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
  vs.zero_grad()
  with context.use(ctx):
    hidden, logits = run()
    if training:
      (hidden[:, :H] * dy64.to(DEV, torch.float32)).sum().backward()
  torch.cuda.synchronize()
  close(hidden, GOLD['%s:hidden' % tag], 1e-5, (tag, 'hidden'))
  close(logits, GOLD['%s:logits' % tag], 1e-5, (tag, 'logits'))
  if not training:
    return
  pr = {n: v.clone().requires_grad_(True) for n, v in var.items()}
  img = inputs['image'].reshape(6, 1, -1) if 'image' in inputs else None
  gen = inputs['general'].reshape(6, 3, -1) if 'general' in inputs else None
  cls = ref.uniter_cls(pr, cfg.model_config.uniter.config, img, gen, inputs.get('text', []))
  close(cls, GOLD['%s:cls' % tag], 1e-9, (tag, 'restated cls'))
  (cls * dy64).sum().backward()
  ref_grads = {n: p.grad for n, p in pr.items() if p.grad is not None}
  got = vs.grad_dict()
  assert len(ref_grads) > 30 and 'cls_emb' in ref_grads
  for n, g in ref_grads.items():
    close(got[n], g, 1e-4, (tag, n), scale=ref.grad_floor(n, ref_grads))
