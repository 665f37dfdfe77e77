"""AutoInt's HIP attention core (csrc/er_autoint.hip) on the GPU: forward and every gradient against the fp64 torch
restatement (oracle/autoint_ref.py) and the reference's own outputs (tests/golden/autoint_vectors.npz), bit-identity
(two runs, eager vs hipGraph replay), and the model against the oracle."""
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from oracle import autoint_ref as ref  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical, first_steps  # noqa: E402
from tests._oracle_steps import close as _close  # noqa: E402
from tests.test_autoint_pins import autoint_cfg  # noqa: E402

logging.disable(logging.WARNING)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

# (B, F, d_in, H, ds): the samples' layers (d_in 16 then 64), odd widths, one head, B not a multiple of the examples
# per workgroup (2 or 3 at F = 18 / 20, d = 64)
CASES = [
    (7, 18, 16, 2, 32),
    (301, 18, 64, 2, 32),
    (5, 20, 16, 2, 32),
    (9, 5, 8, 3, 7),
    (11, 6, 12, 1, 12),
    (4096, 18, 64, 2, 32),
]


def _layer(x, ws, H, ds):
  """One layer through the product's functions: x [B, F, d_in] -> [B, F, d]; gradients into fresh buffers."""
  B, F, d_in = x.shape
  grads = [torch.zeros_like(w) for w in ws]
  qkvr = kernels.AutoIntProjFn.apply(x.reshape(B * F, d_in), grads, *ws)
  y = kernels.AutoIntAttnFn.apply(qkvr, F, H, ds)
  return y.view(B, F, H * ds), grads


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'B%d_F%d_din%d_H%d_ds%d' % c)
def test_layer_matches_the_fp64_restatement(case):
  B, F, d_in, H, ds = case
  x64, ws64 = ref.random_case(B, F, d_in, H, ds, seed=B + F + ds)
  dy64 = torch.randn(B, F, H * ds, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
  x = x64.to(DEV, torch.float32).requires_grad_(True)
  y, grads = _layer(x, [w.to(DEV, torch.float32) for w in ws64], H, ds)
  y.backward(dy64.to(DEV, torch.float32))
  torch.cuda.synchronize()

  xr = x64.clone().requires_grad_(True)
  wr = [w.clone().requires_grad_(True) for w in ws64]
  params = dict(zip(ref.names('l'), wr))
  exp = ref.mha_layer(xr, H, ds, params, 'l')
  # (the gradient through the kernels' ReLU pattern: at B = 4096 a few of the 4.7 M pre-activations lie within fp32
  # rounding of 0, and a flipped mask entry moves its row's dx by a whole term)
  mask = (y.detach().double().cpu() > 0).to(torch.float64)
  (ref.mha_layer(xr, H, ds, params, 'l', mask=mask) * dy64).sum().backward()
  _close(y, exp, 1e-5, 'forward')
  _close(x.grad, xr.grad, 1e-4, 'dx')
  for n, g, w in zip(ref.names('l'), grads, wr):
    _close(g, w.grad, 1e-4, n)


@pytest.mark.parametrize('case', CASES[:5], ids=lambda c: 'B%d_F%d_din%d_H%d_ds%d' % c)
def test_attention_kernels_match_the_restatement(case):
  """The attention launches alone: y and dQ | dK | dV | dR from a random [B * F, 4d] block."""
  B, F, _, H, ds = case
  d = H * ds
  g64 = torch.randn(B * F, 4 * d, generator=torch.Generator().manual_seed(B), dtype=torch.float64)
  dy64 = torch.randn(B * F, d, generator=torch.Generator().manual_seed(B + 1), dtype=torch.float64)
  be = kernels.hip()
  g = g64.to(DEV, torch.float32)
  y = be.autoint_attn_fwd(g, F, H, ds)
  dg = be.autoint_attn_bwd(g, y, dy64.to(DEV, torch.float32), F, H, ds)
  torch.cuda.synchronize()
  gr = g64.clone().requires_grad_(True)
  gv = gr.view(B, F, 4 * d)
  q, k, v, r = gv[..., :d], gv[..., d:2 * d], gv[..., 2 * d:3 * d], gv[..., 3 * d:]
  exp = ref.attention_core(q, k, v, r, H, ds).reshape(B * F, d)
  # (the backward's ReLU pattern is y > 0 on the kernels' own y: the restatement's gradient goes through that pattern)
  mask = (y.double().cpu() > 0).to(torch.float64).view(B, F, d)
  (ref.attention_core(q, k, v, r, H, ds, mask=mask).reshape(B * F, d) * dy64).sum().backward()
  _close(y, exp, 1e-5, 'y')
  for k, what in enumerate(('dQ', 'dK', 'dV', 'dR')):
    _close(dg[:, k * d:(k + 1) * d], gr.grad[:, k * d:(k + 1) * d], 1e-4, what)


GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'autoint_vectors.npz'))
GOLD_CASES = sorted({k.split(':')[0] for k in GOLD.files})


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_layers_match_the_reference_fixture(tag):
  B, fnum, knum, D, H, ds, layers = [int(v) for v in GOLD['%s:cfg' % tag]]
  F = fnum + knum
  var = {k.split(':var:')[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith(tag + ':var:')}
  x64 = torch.from_numpy(GOLD['%s:x' % tag]).reshape(B, F, D)
  x = x64.to(DEV, torch.float32).requires_grad_(True)
  fea, fea64 = x, x64.clone().requires_grad_(True)
  h64 = fea64
  all_grads = []
  for i in range(layers):
    name = ref.layer_name(i)
    ws = [var[n].to(DEV, torch.float32) for n in ref.names(name)]
    fea, grads = _layer(fea, ws, H, ds)
    all_grads.append(grads)
    _close(fea, torch.from_numpy(GOLD['%s:layer%d' % (tag, i)]), 1e-5, (tag, i))
  params64 = {n: v.clone().requires_grad_(True) for n, v in var.items()}
  logits64 = ref.autoint_logits(h64.reshape(B, -1), F, D, H, ds, layers, params64)
  _close(logits64, torch.from_numpy(GOLD['%s:logits' % tag]), 1e-9, (tag, 'logits'))
  # every gradient through the stack against the restatement's
  w_out = var['output/kernel'].to(DEV, torch.float32)
  logits = fea.reshape(B, -1) @ w_out
  logits.sum().backward()
  logits64.sum().backward()
  torch.cuda.synchronize()
  _close(x.grad, h64.grad, 1e-4, (tag, 'dx'))
  for i, grads in enumerate(all_grads):
    for n, g in zip(ref.names(ref.layer_name(i)), grads):
      _close(g, params64[n].grad, 1e-4, (tag, n))


def test_two_runs_and_graph_replay_are_bit_identical():
  B, F, d_in, H, ds = 1001, 18, 64, 2, 32
  x64, ws64 = ref.random_case(B, F, d_in, H, ds, seed=5)
  x = x64.to(DEV, torch.float32).reshape(B * F, d_in)
  ws = [w.to(DEV, torch.float32) for w in ws64]
  grads = [torch.zeros_like(w) for w in ws]
  dy = torch.randn(B * F, H * ds, device=DEV)
  be = kernels.hip()

  def run():
    for g in grads:
      g.zero_()
    xi = x.detach().requires_grad_(True)
    qkvr = kernels.AutoIntProjFn.apply(xi, grads, *ws)
    y = kernels.AutoIntAttnFn.apply(qkvr, F, H, ds)
    y.backward(dy)
    return [y.detach(), xi.grad] + [g.clone() for g in grads]

  assert not be.wgrad_sink().active  # (the weight gradients are launched inside backward here)
  assert_runs_and_replay_bit_identical(run)


# ---------------------------------------------------------------------------------------- the model against the oracle
def _coverage(names, cfg):
  n_att = sum(k.startswith('multi_head_self_attention_layer_') for k in names)
  n_emb = sum('embedding_weights' in k for k in names)
  assert n_att == 4 * cfg.model_config.autoint.interacting_layer_num and n_emb >= 2, (len(names), n_att, n_emb)


def _first_steps(cfg, B, seed, **kw):
  return first_steps(cfg, B, seed, skip_bn_shadowed_bias=False, coverage=_coverage, **kw)


@pytest.mark.parametrize('sequence', [False, True])
def test_model_matches_the_oracle(sequence):
  """B = 128, two steps, the samples' model section (2 heads x 32, 3 layers) on small tables."""
  _first_steps(autoint_cfg(sequence=sequence, layers=3, heads=2, head_size=32, batch_size=128), 128, 21 + sequence)


def test_model_without_interacting_layers_matches_the_oracle():
  _first_steps(autoint_cfg(layers=0, batch_size=128), 128, 9)


def test_full_size_config_matches_the_oracle():
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'autoint_taobao_10m.config'))
  _first_steps(cfg, 4096, 8, step0_tol=1e-4)


def test_evaluate_returns_an_auc():
  B = 128
  cfg = autoint_cfg(layers=3, heads=2, head_size=32, batch_size=B)
  est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=3).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=103)
  for _ in range(3):
    est.train_step(gen.next_batch())
  res = est.evaluate([gen.next_batch() for _ in range(3)])
  assert 'auc' in res and 0.0 <= float(res['auc']) <= 1.0, res
