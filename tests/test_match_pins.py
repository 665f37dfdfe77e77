"""The two-tower models on the CPU: the classes resolve, DSSM's variables follow the reference's names
(model/dssm.py), the composed head equals the fp64 restatement, both configs train on the stand-in backend with the
restatement's losses, unsupported setups raise at build time, the LDS formula is the library's, and the rank counts
reproduce a sort-based top-k under ties."""
import os
import sys

import numpy as np
import pytest
import torch

from _oracle_steps import covers, first_steps
from easyrec_amd.layers import match_head
from oracle import match_ref as ref
from easyrec_amd.utils import load_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make_configs():
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  return make_configs


def dssm_cfg(in_batch=False, batch_size=16):
  return _make_configs().dssm_taobao(in_batch=in_batch, batch_size=batch_size, scale=0.01)


def test_model_classes_are_registered():
  load_class.import_all_models()
  from easyrec_amd.model.easy_rec_model import _EASY_REC_MODEL_CLASS_MAP
  assert 'DSSM' in _EASY_REC_MODEL_CLASS_MAP and 'MatchModel' in _EASY_REC_MODEL_CLASS_MAP


@pytest.mark.parametrize('name,in_batch', [('dssm_taobao_10m.config', False), ('dssm_inbatch_taobao_10m.config', True)])
def test_committed_configs_are_the_generated_ones(name, in_batch):
  from easyrec_amd.protos.loss_pb2 import LossType
  from easyrec_amd.protos.simi_pb2 import Similarity
  from easyrec_amd.utils import config_util
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', name))
  assert cfg == _make_configs().dssm_taobao(in_batch=in_batch, item_rows=10000000)
  mc = cfg.model_config
  assert mc.model_class == 'DSSM' and [g.group_name for g in mc.feature_groups] == ['user', 'item']
  assert list(mc.dssm.user_tower.dnn.hidden_units) == [256, 128, 64, 32] == list(mc.dssm.item_tower.dnn.hidden_units)
  assert cfg.data_config.batch_size == 4096 and cfg.data_config.WhichOneof('sampler') is None
  if in_batch:
    assert mc.loss_type == LossType.SOFTMAX_CROSS_ENTROPY and mc.dssm.simi_func == Similarity.INNER_PRODUCT
    assert mc.dssm.scale_simi and mc.dssm.item_id == 'adgroup_id'
  else:
    assert mc.loss_type == LossType.CLASSIFICATION and mc.dssm.simi_func == Similarity.COSINE and mc.dssm.scale_simi


def _operands(B, extra, D, seed):
  g = torch.Generator().manual_seed(seed)
  return (torch.randn(B, D, generator=g, dtype=torch.float64).float(),
          torch.randn(B + extra, D, generator=g, dtype=torch.float64).float())


@pytest.mark.parametrize('opt', ['plain', 'scale', 'ids', 'ignore', 'weights'])
def test_composed_head_equals_the_restatement(opt):
  U, I = _operands(6, 3, 5, seed=3)
  sw, sb = (torch.tensor([-1.5]), torch.tensor([0.2])) if opt == 'scale' else (None, None)
  ids = torch.tensor([3, 1, 3, 2, 1, 3, 3, 1, 0]) if opt == 'ids' else None
  w = torch.tensor([1.0, 0.0, 2.0, 0.5, 1.0, 0.0]) if opt == 'weights' else None
  d = lambda t: None if t is None else t.double()
  got = match_head.match_head(U, I, 2.0, sw, sb, ids, opt == 'ignore', w)  # (a CPU tensor: the composition)
  want = ref.list_wise_losses(U.double(), I.double(), 2.0, d(sw), d(sb), ids, opt == 'ignore', d(w))
  for g, e in zip(got, want):
    assert abs(float(g) - float(e)) <= 1e-5 * max(1e-3, abs(float(e)))
  z = ref.logits(U.double(), I.double(), 2.0, d(sw), d(sb), ids, opt == 'ignore')
  if opt in ('ids', 'ignore'):
    assert float(z.min()) == -1e32 and float(torch.softmax(z, 1).min()) == 0.0  # a masked entry adds exactly 0
  x = torch.cat([U, torch.zeros(1, 5)])
  assert torch.allclose(match_head.normalize(x).double(), ref.l2_normalize(x.double()), atol=1e-6)
  assert torch.isfinite(match_head.normalize(x)).all()


def test_rank_counts_follow_top_k_s_tie_rule():
  g = torch.Generator().manual_seed(7)
  U = torch.randint(-1, 2, (9, 3), generator=g).float()
  I = torch.randint(-1, 2, (14, 3), generator=g).float()
  I[4] = I[0]
  z = ref.logits(U.double(), I.double())
  assert any(len(np.unique(r)) < len(r) for r in z.numpy())
  want_in, want_neg = ref.rank_counts(z.numpy())
  c_in, c_neg = match_head.rank_counts(U, I)
  assert np.array_equal(c_in.numpy(), want_in) and np.array_equal(c_neg.numpy(), want_neg)
  for k in (1, 2, 5):
    assert match_head.recall_at_k(c_in, c_neg, k) == pytest.approx(ref.recall_at_k(z.numpy(), k), abs=1e-12)
  # hand-made ties: the positive equals an earlier and a later in-batch column and an extra negative
  z = np.array([[1.0, 1.0, 0.0, 1.0], [2.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 3.0]])
  assert [list(v) for v in ref.rank_counts(z)] == [[0, 1, 2], [0, 0, 1]]
  assert ref.recall_at_k(z, 1) == {'recall@1': 1 / 3, 'recall_neg_sam@1': 2 / 3, 'recall_in_batch@1': 1 / 3}


def test_lds_formula_is_the_library_s(built_lib):
  from easyrec_amd import kernels
  be = kernels.HipBackend()
  for D in range(0, 131):
    assert be.match_lds_bytes(D) == match_head.lds_bytes(D), D
  assert match_head.lds_bytes(128) == 4 * (96 * 129 + 32 * 65 + 256) + 768 <= 65536
  assert match_head.lds_bytes(0) == 0 == match_head.lds_bytes(129)


def dssm_coverage(names, cfg):
  covers(names, cfg, {'sim_w', 'sim_b', 'user_dnn/dnn_3/kernel', 'item_dnn/dnn_0/kernel', 'user_dnn/dnn_1/bn/gamma'})


def backbone_coverage(names, cfg):
  covers(names, cfg, {'user_tower/layer_1/dense/kernel', 'item_tower/layer_0/dense/kernel', 'user_tower/layer_0/bn/gamma'})


@pytest.mark.parametrize('in_batch', [False, True])
def test_model_builds_and_steps_on_the_stand_in(ref_backend, built_lib, in_batch):
  """Two steps against the fp64 model oracle from the batch on (tests/_oracle_steps.first_steps)."""
  from easyrec_amd.input.synthetic import SyntheticBatches
  B = 16
  cfg = dssm_cfg(in_batch, B)

  def initial_values(est, orc, step, batch):
    if step == 0:  # (the oracle still holds the state the estimator was built with)
      assert float(orc.state['sim_w'][0]) == 1.0 and float(orc.state['sim_b'][0]) == 0.0
  est = first_steps(cfg, B, seed=4, device='cpu', oracle_dtype=torch.float64, coverage=dssm_coverage, after_step=initial_values)
  st = est.state_dict()
  for tower in ('user_dnn', 'item_dnn'):
    assert st[tower + '/dnn_3/kernel'].shape == (64, 32) and tower + '/dnn_3/bn/gamma' not in st
    assert tower + '/dnn_2/bn/gamma' in st and est.varstore.l2_of(tower + '/dnn_3/kernel') == pytest.approx(1e-6)
  assert est.varstore.l2_of('sim_w') == 0.0
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=44)
  # evaluation: the list-wise metrics from the rank counts, the point-wise auc
  est.model._is_training = est.ctx.is_training = False
  pred = est.predict(gen.next_batch())
  assert pred['user_tower_emb'].shape == (B, 32) and ('logits' in pred)
  metrics = est.model.build_metric_graph(cfg.eval_config)
  assert set(metrics) == ({'recall@10', 'recall_neg_sam@10', 'recall_in_batch@10'} if in_batch else {'auc'})
  if in_batch:
    assert metrics == pytest.approx(ref.recall_at_k(pred['logits'].double().numpy(), 10))
  out = est.model.build_output_dict()
  assert len(out['user_emb']) == B and out['user_emb'][0].count(',') == 31


@pytest.mark.parametrize('sampler', ['negative_sampler', 'negative_sampler_v2', 'hard_negative_sampler',
                                     'hard_negative_sampler_v2'])
def test_samplers_are_refused(ref_backend, sampler):
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  cfg = dssm_cfg(True)
  getattr(cfg.data_config, sampler).SetInParent()
  with pytest.raises(NotImplementedError, match=sampler + ':'):
    EasyRecEstimator(cfg, device='cpu', batch_size=16, seed=4)


def test_other_refusals(ref_backend):
  from easyrec_amd.layers.sharded_embedding import ShardedEmbeddingEngine
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  from easyrec_amd.model.match_model import MatchModel
  from easyrec_amd.protos.loss_pb2 import LossType
  with pytest.raises(ValueError, match='bf16'):
    EasyRecEstimator(dssm_cfg(True), device='cpu', batch_size=16, seed=4, dense_dtype='bf16')
  with pytest.raises(ValueError, match='embedding-parallel'):
    MatchModel.check_supported(LossType.SOFTMAX_CROSS_ENTROPY, 'f32', object.__new__(ShardedEmbeddingEngine), 'DSSM')
  from easyrec_amd.model.embedding_parallel import EmbeddingParallelEstimator
  for in_batch in (False, True):
    with pytest.raises(ValueError, match='DSSM: embedding-parallel'):
      EmbeddingParallelEstimator(dssm_cfg(in_batch), device='cpu', batch_size=16, seed=4, rank=0, world=1)
  with pytest.raises(ValueError, match='invalid loss type'):
    MatchModel.check_supported(LossType.PAIR_WISE_LOSS, 'f32', None)
  # a batch that carries hard negatives
  cfg = dssm_cfg(True)
  f = cfg.data_config.input_fields.add()
  f.input_name = 'hard_neg_indices'
  fc = cfg.feature_config.features.add()
  fc.input_names.append('hard_neg_indices')
  fc.feature_type = fc.RawFeature
  with pytest.raises(NotImplementedError, match='hard_neg_indices'):
    EasyRecEstimator(cfg, device='cpu', batch_size=16, seed=4)


# ---------------------------------------------------------------------------------------- the reference's own outputs
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'match_vectors.npz'))
GOLD_CASES = sorted({k.split(':')[0] for k in GOLD.files})


def gold_case(tag):
  """(options, head, loss type, {name: fp64 tensor} of the case's arrays, {name: variable})"""
  import json
  import types
  from easyrec_amd.protos.loss_pb2 import LossType
  from easyrec_amd.protos.simi_pb2 import Similarity
  o = json.loads(str(GOLD[tag + ':opts']))
  head = types.SimpleNamespace(simi_func=getattr(Similarity, o['simi']), temperature=o.get('temperature', 1.0),
                               scale_simi=o['scale'])
  arr = {k.split(':', 1)[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files
         if k.startswith(tag + ':') and ':var:' not in k and GOLD[k].dtype == np.float64}
  var = {k.split(':var:')[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith(tag + ':var:')}
  return o, head, getattr(LossType, o['loss']), arr, var


def gold_towers(o, arr, var):
  """the two tower outputs in front of the similarity: the DSSM towers, or the backbone's outputs (indices 1 / 0)"""
  if o.get('backbone'):
    return arr['user'], arr['item']
  return ref.tower(arr['user'], var, 'user_dnn'), ref.tower(arr['item'], var, 'item_dnn')


def gold_head_args(o, arr):
  ids = torch.tensor(o['ids']) if 'ids' in o else None
  w = torch.tensor(o['weight'], dtype=torch.float64) if 'weight' in o else None
  return ids, w, bool(o.get('ignore'))


def test_fixture_covers_the_cases():
  opts = {t: gold_case(t)[0] for t in GOLD_CASES}
  assert all(o['B'] <= 6 for o in opts.values())
  assert any(o['simi'] == 'COSINE' and o.get('temperature') == 0.5 and o.get('sim_w') == -1.5 for o in opts.values())
  assert any(o['simi'] == 'INNER_PRODUCT' and not o['scale'] and o['loss'] == 'SOFTMAX_CROSS_ENTROPY' for o in opts.values())
  assert any('ids' in o and len(set(o['ids'][:o['B']])) < o['B'] for o in opts.values())
  assert any(o.get('ignore') for o in opts.values()) and any(0.0 in o.get('weight', []) for o in opts.values())
  assert any(o.get('extra') == 3 for o in opts.values()) and any(o.get('backbone') for o in opts.values())
  assert {'CLASSIFICATION', 'L2_LOSS', 'SOFTMAX_CROSS_ENTROPY'} == {o['loss'] for o in opts.values()}
  assert float(GOLD['cos_scale:var:sim_w'][0]) == -1.5
  var = gold_case('ip')[4]
  assert sorted(n for n in var if n.startswith('user_dnn')) == sorted(
      ['user_dnn/dnn_%d/%s' % (i, v) for i in range(3) for v in ('kernel', 'bias')] +
      ['user_dnn/dnn_%d/bn/%s' % (i, v) for i in range(2) for v in ('gamma', 'beta')])
  assert float(GOLD['ids:logits'].min()) == -1e32 and float(GOLD['ids:probs'].min()) == 0.0
  assert str(GOLD['ip:user_emb'][0]) == ','.join('%f' % v for v in GOLD['ip:user_tower_emb'][0])


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_restatement_matches_the_reference(tag):
  o, head, loss_type, arr, var = gold_case(tag)
  ids, w, ignore = gold_head_args(o, arr)
  u, i = gold_towers(o, arr, var)
  losses, pred = ref.head_losses(head, loss_type, u, i, var, arr['label'], ids, w, ignore)
  want_losses = {k.split('loss:')[1]: v for k, v in arr.items() if k.startswith('loss:')}
  assert set(losses) == set(want_losses)
  checked = 0
  for k, v in list(pred.items()) + list(losses.items()):
    want = want_losses[k] if k in want_losses and k not in pred else arr[k]
    unmasked = want.abs() < 1e31
    assert v.shape == want.shape and torch.equal(v.abs() < 1e31, unmasked), (tag, k)
    assert float((v - want)[unmasked].abs().max()) <= 1e-9 * float(want[unmasked].abs().max()), (tag, k)
    assert torch.equal(v[~unmasked], want[~unmasked])  # the masked logits are -1e32 exactly
    checked += 1
  assert checked >= 4


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_product_host_path_matches_the_reference(tag):
  """The package's own CPU functions (normalisation, masked logits, composed losses, point-wise heads through the
  loss builder's restated formulas) on the fixture's tower outputs, fp32, at the stand-in's bars."""
  from easyrec_amd.protos.loss_pb2 import LossType
  from easyrec_amd.protos.simi_pb2 import Similarity
  o, head, loss_type, arr, var = gold_case(tag)
  ids, w, ignore = gold_head_args(o, arr)
  u, i = [t.float() for t in gold_towers(o, arr, var)]
  inv_t = 1.0
  if head.simi_func == Similarity.COSINE:
    u, i, inv_t = match_head.normalize(u), match_head.normalize(i), 1.0 / head.temperature
  sw, sb = (var['sim_w'].float(), var['sim_b'].float()) if head.scale_simi else (None, None)
  near = lambda got, want, tol: float((got.double() - want).abs().max()) <= tol * max(1e-3, float(want.abs().max()))
  assert near(u, arr['user_tower_emb'], 1e-5) and near(i, arr['item_tower_emb'], 1e-5)
  if loss_type == LossType.SOFTMAX_CROSS_ENTROPY:
    z = match_head.masked_logits(u, i, inv_t, sw, sb, ids, ignore)
    keep = arr['logits'].abs() < 1e31
    assert torch.equal(z.double().abs() < 1e31, keep) and near(z.double()[keep], arr['logits'][keep], 1e-5)
    ce, reg = match_head.match_head(u, i, inv_t, sw, sb, ids, ignore, None if w is None else w.float())
    assert near(ce, arr['loss:cross_entropy_loss'], 1e-5) and near(reg, arr['loss:reg_pos_loss'], 1e-5)
    c_in, c_neg = match_head.rank_counts(u, i, inv_t, sw, sb, ids, ignore)
    want_in, want_neg = ref.rank_counts(arr['logits'].numpy())
    assert np.array_equal(c_in.numpy(), want_in) and np.array_equal(c_neg.numpy(), want_neg)


def backbone_cfg(B=16):
  return _make_configs().dssm_backbone_taobao(batch_size=B, scale=0.01)


def l2_cfg(B=16):
  from easyrec_amd.protos.loss_pb2 import LossType
  cfg = dssm_cfg(False, B)
  cfg.model_config.loss_type = LossType.L2_LOSS
  del cfg.eval_config.metrics_set[:]
  cfg.eval_config.metrics_set.add().mean_absolute_error.SetInParent()
  return cfg


def test_backbone_form_builds_and_steps(ref_backend, built_lib):
  """MatchModel over a backbone (model_params): the reference's dssm_on_taobao_backbone model section, no sampler."""
  cfg = backbone_cfg()
  est = first_steps(cfg, 16, seed=4, device='cpu', oracle_dtype=torch.float64, coverage=backbone_coverage)
  st = est.state_dict()
  assert 'user_tower/layer_1/dense/kernel' in st and 'sim_w' not in st and st['item_tower/layer_1/dense/kernel'].shape == (128, 32)
  est.model._is_training = est.ctx.is_training = False
  pred = est.predict()
  assert pred['logits'].shape == (16, 16) and est.model.get_outputs()[:2] == ['logits', 'probs']
  metrics = est.model.build_metric_graph(cfg.eval_config)
  assert metrics == pytest.approx(ref.recall_at_k(pred['logits'].double().numpy(), 10))


def test_l2_loss_head_builds_and_steps(ref_backend, built_lib):
  cfg = l2_cfg()
  est = first_steps(cfg, 16, seed=4, device='cpu', oracle_dtype=torch.float64, coverage=dssm_coverage)
  est.model._is_training = est.ctx.is_training = False
  pred = est.predict()
  assert pred['y'].shape == (16,) and est.model.get_outputs()[0] == 'y'
  mae = est.model.build_metric_graph(cfg.eval_config)['mean_absolute_error']
  assert mae == pytest.approx(float((est.features.label('clk').double() - pred['y'].double()).abs().mean()), rel=1e-6)
