"""AutoInt on the CPU: the model class resolves, the layer's variables follow the reference's names and shapes
(layers/multihead_attention.py, model/autoint.py), the restatement reproduces the reference's own outputs, unsupported
setups raise at build time, and the model trains on a stand-in backend exactly as the oracle does."""
import os

import numpy as np
import pytest
import torch

from easyrec_amd.core.variables import VarStore
from easyrec_amd.layers import multihead_attention as mha
from easyrec_amd.utils import load_class
from oracle.kernel_ref import RefBackend
from oracle import autoint_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'autoint_vectors.npz'))
GOLD_CASES = sorted({k.split(':')[0] for k in GOLD.files})


def _gold(tag):
  B, fnum, knum, D, H, ds, layers = [int(v) for v in GOLD['%s:cfg' % tag]]
  var = {k.split(':var:')[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith(tag + ':var:')}
  return B, fnum + knum, D, H, ds, layers, torch.from_numpy(GOLD['%s:x' % tag]), var


def test_model_class_is_registered():
  load_class.import_all_models()
  from easyrec_amd.model.easy_rec_model import _EASY_REC_MODEL_CLASS_MAP
  assert 'AutoInt' in _EASY_REC_MODEL_CLASS_MAP


def test_fixture_covers_the_cases():
  cfgs = {t: [int(v) for v in GOLD['%s:cfg' % t]] for t in GOLD_CASES}
  assert any(c[1] + c[2] == 18 and c[3:] == [16, 2, 32, 3] for c in cfgs.values())
  assert any(c[1] + c[2] == 20 and c[2] > 0 for c in cfgs.values())
  assert any(c[4] == 1 and c[5] == c[3] for c in cfgs.values())  # one head of size D
  assert any(c[6] == 0 for c in cfgs.values())
  assert any(c[5] % 2 == 1 and c[4] == 3 for c in cfgs.values())


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_restatement_matches_the_reference(tag):
  B, F, D, H, ds, layers, x, var = _gold(tag)
  fea = x.reshape(B, F, D)
  for i in range(layers):
    fea = ref.mha_layer(fea, H, ds, var, ref.layer_name(i))
    want = GOLD['%s:layer%d' % (tag, i)]
    assert np.abs(fea.numpy() - want).max() <= 1e-9 * np.abs(want).max(), (tag, i)
  got = ref.autoint_logits(x, F, D, H, ds, layers, var)
  want = GOLD['%s:logits' % tag]
  assert np.abs(got.numpy() - want).max() <= 1e-9 * np.abs(want).max(), tag


def test_scores_are_multiplied_by_sqrt_head_size():
  """S = Q K^T / ds ** -0.5: with V = I-like columns the output shows the softmax of sqrt(ds) * q . k."""
  ds = 4
  q = torch.tensor([[[1.0, 0, 0, 0], [0, 0, 0, 0]]], dtype=torch.float64)
  k = torch.tensor([[[0.5, 0, 0, 0], [0, 0, 0, 0]]], dtype=torch.float64)
  v = torch.tensor([[[1.0, 0, 0, 0], [0, 0, 0, 0]]], dtype=torch.float64)
  y = ref.attention_core(q, k, v, torch.zeros_like(q), 1, ds)
  s = 0.5 * 2.0  # q0 . k0 * sqrt(4)
  assert abs(float(y[0, 0, 0]) - np.exp(s) / (np.exp(s) + 1.0)) < 1e-12
  # the kernels' factor as the geometry gives it (csrc/er_autoint.hip AiGeom.scale) is the same
  be = RefBackend()
  g = torch.cat([q, k, v, torch.zeros_like(q)], dim=2).reshape(2, 16).float()
  assert abs(float(be.autoint_attn_fwd(g, 2, 1, ds)[0, 0]) - np.exp(s) / (np.exp(s) + 1.0)) < 1e-6


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_product_variable_names_are_the_reference_names(tag):
  B, F, D, H, ds, layers, x, var = _gold(tag)
  vs = VarStore('cpu')
  d_in = D
  for i in range(layers):
    ws = mha.MultiHeadAttention(H, ds, 1e-6, use_res=True, name=ref.layer_name(i)).variables(d_in, vs)
    assert [tuple(w.shape) for w in ws] == [tuple(var[n].shape) for n in ref.names(ref.layer_name(i))]
    d_in = H * ds
  vs.get_variable('output/kernel', (F * d_in, 1))
  vs.get_variable('output/bias', (1,), 'zeros')
  assert sorted(vs.names()) == sorted(var)
  assert all(vs.l2_of(n) == (0.0 if n.startswith('output/') else 1e-6) for n in vs.names())


def test_envelope():
  assert mha.lds_bytes(18, 2, 32) <= mha.LDS_BUDGET and mha.lds_bytes(20, 2, 32) <= mha.LDS_BUDGET
  mha.check_envelope(20, 2, 32)
  mha.check_envelope(5, 3, 7)
  for F, H, ds in [(64, 2, 32), (20, 8, 32), (0, 2, 32), (18, 0, 32)]:
    with pytest.raises(ValueError):
      mha.check_envelope(F, H, ds)


def test_envelope_formula_is_the_library_s(built_lib):
  from easyrec_amd import kernels
  be = kernels.HipBackend()
  for F, H, ds in [(18, 2, 32), (20, 2, 32), (5, 3, 7), (6, 1, 12), (64, 2, 32)]:
    assert be.autoint_lds_bytes(F, H, ds) == mha.lds_bytes(F, H, ds)
    assert (be.autoint_epb(F, H, ds, True) > 0) == (mha.lds_bytes(F, H, ds) <= mha.LDS_BUDGET)


def test_use_res_false_is_not_implemented():
  with pytest.raises(NotImplementedError):
    mha.MultiHeadAttention(2, 32, None, use_res=False)


# ---------------------------------------------------------------------------------------- configs and the model
def autoint_cfg(sequence=False, layers=2, heads=2, head_size=8, batch_size=16):
  """A small AutoInt config (the sample's model section on the scaled-down taobao tables)."""
  import sys
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  cfg = make_configs.autoint_taobao(sequence=sequence, batch_size=batch_size, scale=0.01, seq_len=12)
  ai = cfg.model_config.autoint
  ai.interacting_layer_num, ai.multi_head_num, ai.multi_head_size = layers, heads, head_size
  return cfg


def _check(cfg, dense_dtype='f32', engine=None):
  from easyrec_amd.model.autoint import AutoInt
  fnum, knum = AutoInt.field_counts(cfg.model_config)
  return AutoInt.check_supported(cfg.model_config.autoint, list(cfg.feature_config.features), fnum, knum,
                                 dense_dtype, engine)


def test_field_counts_of_the_two_samples():
  from easyrec_amd.model.autoint import AutoInt
  assert AutoInt.field_counts(autoint_cfg().model_config) == (18, 0)
  assert AutoInt.field_counts(autoint_cfg(sequence=True).model_config) == (18, 2)
  assert _check(autoint_cfg()) == 16 and _check(autoint_cfg(sequence=True)) == 16


def test_rejected_combinations():
  from easyrec_amd.layers.sharded_embedding import ShardedEmbeddingEngine
  cfg = autoint_cfg()
  with pytest.raises(ValueError, match='bf16'):
    _check(cfg, 'bf16')
  with pytest.raises(ValueError, match='embedding-parallel'):
    _check(cfg, 'f32', object.__new__(ShardedEmbeddingEngine))
  uneven = autoint_cfg()
  uneven.feature_config.features[0].embedding_dim = 8
  with pytest.raises(ValueError, match='consistent'):
    _check(uneven)
  missing = autoint_cfg()
  del missing.model_config.feature_groups[0].feature_names[-1]
  with pytest.raises(ValueError, match='consistent'):
    _check(missing)
  wide = autoint_cfg(heads=8, head_size=32)
  with pytest.raises(ValueError, match='envelope'):
    _check(wide)
  _check(autoint_cfg(layers=0, heads=8, head_size=32))  # no attention layer: nothing to fit


def test_committed_config_is_the_sample_model():
  from easyrec_amd.utils import config_util
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'autoint_taobao_10m.config'))
  mc = cfg.model_config
  assert mc.model_class == 'AutoInt' and len(mc.feature_groups[0].feature_names) == 18
  ai = mc.autoint
  assert (ai.multi_head_num, ai.multi_head_size, ai.interacting_layer_num) == (2, 32, 3)
  assert abs(ai.l2_regularization - 1e-6) < 1e-12 and abs(mc.embedding_regularization - 1e-6) < 1e-12
  assert cfg.data_config.batch_size == 4096
  assert {f.embedding_dim for f in cfg.feature_config.features} == {16}
  assert max(f.hash_bucket_size for f in cfg.feature_config.features) == 10000000
  assert _check(cfg) == 16


@pytest.mark.parametrize('sequence', [False, True])
def test_model_builds_and_steps_on_the_stand_in(ref_backend, built_lib, sequence):
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  from oracle.model_oracle import OracleTrainer
  B = 16
  cfg = autoint_cfg(sequence=sequence, layers=2, heads=2, head_size=8, batch_size=B)
  est = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4).build()
  st = est.state_dict()
  assert 'multi_head_self_attention_layer_1/dnn/kernel' in st and st['output/kernel'].shape == ((20 if sequence else 18) * 16, 1)
  orc = OracleTrainer(cfg, st, batch_size=B)
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=44)
  for _ in range(2):
    b = gen.next_batch()
    est.train_step(b)
    got, exp = est.loss_values(), orc.train_step(b)
    for k in exp:
      assert abs(got[k] - exp[k]) <= 1e-4 * max(1e-3, abs(exp[k])), (k, got[k], exp[k])
