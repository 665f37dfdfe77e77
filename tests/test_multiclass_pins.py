"""The multi-class softmax and JRC heads on the host side: the torch compositions and RankModel's head table against
values and names the reference's own code produced (tests/golden/make_multiclass_vectors.py) at 1e-9 in fp64, the
gradient that seeds the backward against central differences of the reference's forward, the metrics against direct numpy
counts (ties in the logits included), every build-time refusal, and estimators of both new configs' shapes stepping on a
stand-in backend."""
import logging
import os
import types

import numpy as np
import pytest
import torch

from easyrec_amd import kernels
from easyrec_amd.builders import loss_builder
from easyrec_amd.builders import multiclass_loss as mcl
from easyrec_amd.core import context, metrics
from easyrec_amd.input.synthetic import SyntheticBatches
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
from easyrec_amd.model.rank_model import RankModel
from easyrec_amd.protos import loss_pb2
from easyrec_amd.protos.loss_pb2 import LossType
from easyrec_amd.utils import config_util
from oracle.kernel_ref import RefBackend

logging.disable(logging.WARNING)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'multiclass_vectors.npz'))
REFERENCE = '/root/reference'


def _t(name):
  return torch.from_numpy(G[name])


def _near(got, want, tol=1e-9):
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  assert got.shape == want.shape
  assert float(np.abs(got - want).max()) <= tol * max(1.0, float(np.abs(want).max())), float(np.abs(got - want).max())


def _grad_near(dz, want):
  """central differences (h = 1e-6) of an O(1) loss carry about 1e-10 of rounding and 1e-12 of truncation per entry:
  tests/test_loss_pins.py's bar for the same kind of fixture"""
  assert float(np.abs(dz.numpy() - want).max()) <= 2e-5 * float(np.abs(want).max()) + 1e-7


@pytest.fixture
def cpu(monkeypatch):
  monkeypatch.setattr(kernels, '_BACKEND', RefBackend())


# ------------------------------------------------------------------------------------------------ the compositions
@pytest.mark.parametrize('C', [3, 5])
@pytest.mark.parametrize('tag', ['', '_w'])
def test_softmax_ce_composition_and_loss_builder_against_the_reference(cpu, C, tag):
  z, y = _t('smc_c%d_logits' % C), _t('smc_c%d_labels' % C)
  weights = _t('weights') if tag else 1.0
  _near(mcl.softmax_ce_compose(y, z, weights), G['smc_c%d%s_loss' % (C, tag)])
  loss, dz = loss_builder.build(LossType.CLASSIFICATION, y, z, weights, C)
  _near(loss, G['smc_c%d%s_loss' % (C, tag)].reshape(1))
  _grad_near(dz, G['smc_c%d%s_grad' % (C, tag)])
  scaled, dzs = loss_builder.build(LossType.CLASSIFICATION, y, z, weights, C, loss_scale=0.25)
  _near(scaled, 0.25 * G['smc_c%d%s_loss' % (C, tag)].reshape(1))
  _near(dzs, 0.25 * dz.numpy())


@pytest.mark.parametrize('wtag', ['', '_w', '_s2'])
@pytest.mark.parametrize('alpha', [0.5, 0.3])
@pytest.mark.parametrize('same', [True, False])
def test_jrc_composition_and_loss_builder_against_the_reference(cpu, wtag, alpha, same):
  z, y, keys = _t('jrc_logits'), _t('jrc_labels'), _t('jrc_sessions')
  weights = {'': 1.0, '_w': _t('weights'), '_s2': 2.0}[wtag]
  tag = 'jrc%s_a%d_%s' % (wtag, round(alpha * 10), 'same' if same else 'diff')
  param = loss_pb2.JRCLoss(session_name='user_id', alpha=alpha, same_label_loss=same)
  _near(mcl.jrc_compose(y, z, keys, param.alpha, weights, same), G[tag + '_loss'])  # (alpha is a float32 field)
  loss, dz = loss_builder.build(LossType.JRC_LOSS, y, z, weights, 2, loss_param=param, session_ids=keys)
  _near(loss, G[tag + '_loss'].reshape(1))
  _grad_near(dz, G[tag + '_grad'])


def test_jrc_session_algebra_is_the_masked_form():
  """what er_jrc evaluates (include/easyrec_hip.h K8l) - per-session log-sum-exps, each session's sum shared out over
  its members - is the reference's [B, B] form"""
  z, y, keys, w = _t('jrc_logits'), _t('jrc_labels').double(), _t('jrc_sessions'), _t('weights')
  B = len(y)
  ge = 0.0
  for i in range(B):
    S = torch.nonzero(keys == keys[i]).reshape(-1)
    lse1, lse0 = torch.logsumexp(z[S, 1], 0), torch.logsumexp(z[S, 0], 0)
    ge += (w[S].sum() / len(S)) * -(y[i] * (z[i, 1] - lse1) + (1 - y[i]) * (z[i, 0] - lse0))
  ce = mcl.softmax_ce_compose(y, z, w)
  alpha = loss_pb2.JRCLoss(alpha=0.3).alpha  # (a float32 field)
  _near(alpha * ce + (1 - alpha) * ge / B, G['jrc_w_a3_same_loss'])


# ------------------------------------------------------------------------------------------------ the head table
class _Features(dict):
  def batch_ids_of(self, name):
    return self[name]


def _bare_model(labels, features=None, training=False):
  m = RankModel.__new__(RankModel)
  m._prediction_dict, m._loss_dict, m._backward_seeds, m._losses = {}, {}, [], []
  m._labels, m._feature_dict, m._is_training = labels, _Features(features or {}), training
  return m


@pytest.mark.parametrize('suffix', ['', '_cvr'])
def test_multiclass_head_keys_and_values(cpu, suffix):
  z = _t('multiclass_logits')
  m = _bare_model({'lbl': _t('smc_c5_labels')})
  with context.use(context.ModelContext(None, None, is_training=False)):
    pred = m._output_to_prediction_impl(z, LossType.CLASSIFICATION, num_class=5, suffix=suffix)
    assert set(pred) == set(G['names_multiclass_pred' + suffix])
    for k in pred:
      _near(pred[k], G['multiclass%s/%s' % (suffix, k)])
    assert pred['y' + suffix][3] == 1 and z[3, 1] == z[3, 4]  # the tie: the first index
    m._prediction_dict.update(pred)
    for given in ('', 'my_loss'):
      got = m._build_loss_impl(LossType.CLASSIFICATION, 'lbl', 1.0, 5, suffix, given)
      assert list(got) == list(G['names_multiclass_loss%s_%s' % (suffix, given or 'default')])
    assert m._get_outputs_impl(LossType.CLASSIFICATION, 5, suffix) == list(G['names_multiclass_outputs' + suffix])
    assert m._get_outputs_impl(LossType.CLASSIFICATION, 1, suffix) == ['probs' + suffix, 'logits' + suffix]


@pytest.mark.parametrize('suffix', ['', '_cvr'])
def test_jrc_head_keys_and_values(cpu, suffix):
  z = _t('jrc_logits')
  m = _bare_model({'clk': _t('jrc_labels')}, {'user_id': _t('jrc_sessions')})
  param = loss_pb2.JRCLoss(session_name='user_id', alpha=0.5)
  with context.use(context.ModelContext(None, None, is_training=False)):
    pred = m._output_to_prediction_impl(z, LossType.JRC_LOSS, num_class=2, suffix=suffix)
    assert set(pred) == set(G['names_jrc_pred' + suffix])
    for k in pred:
      _near(pred[k], G['jrc%s/%s' % (suffix, k)])
    m._prediction_dict.update(pred)
    for given in ('', 'my_loss'):
      got = m._build_loss_impl(LossType.JRC_LOSS, 'clk', 1.0, 2, suffix, given, param)
      assert list(got) == list(G['names_jrc_loss%s_%s' % (suffix, given or 'default')])
      _near(list(got.values())[0], G['jrc_model_loss' + suffix].reshape(1))
    assert m._get_outputs_impl(LossType.JRC_LOSS, 2, suffix) == list(G['names_jrc_outputs' + suffix])
    with pytest.raises(AssertionError, match='num_class must be 2'):
      m._output_to_prediction_impl(torch.zeros(4, 3), LossType.JRC_LOSS, num_class=3)


def test_training_probabilities_come_from_the_loss(cpu):
  z = _t('multiclass_logits')
  m = _bare_model({'lbl': _t('smc_c5_labels')}, training=True)
  with context.use(context.ModelContext(None, None, is_training=True)):
    m._prediction_dict.update(m._output_to_prediction_impl(z, LossType.CLASSIFICATION, num_class=5))
    assert m._prediction_dict['probs'] is None and m._prediction_dict['logits'] is z
    m._build_loss_impl(LossType.CLASSIFICATION, 'lbl', 1.0, 5)
  _near(m._prediction_dict['probs'], G['multiclass/probs'])
  _near(m._prediction_dict['probs_1'], G['multiclass/probs_1'])


# ------------------------------------------------------------------------------------------------ the metrics
def _tied_logits(rng, B, C):
  z = rng.integers(-2, 3, size=(B, C)).astype(np.float32)  # small integers: ties in most rows
  z[0, :] = 1.0
  return z


def test_label_rank_and_first_argmax_against_numpy_with_ties():
  rng = np.random.default_rng(3)
  for C in (2, 3, 7):
    z = _tied_logits(rng, 200, C)
    y = rng.integers(0, C, size=200)
    order = np.argsort(-z, axis=1, kind='stable')
    want = np.array([int(np.nonzero(order[r] == y[r])[0][0]) for r in range(200)])
    got = mcl.label_rank(torch.from_numpy(z), torch.from_numpy(y.astype(np.float32)))
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(mcl.first_argmax(torch.from_numpy(z)).numpy(), order[:, 0])
    for k in (1, 2):
      m = metrics.TopKHits(k, 'cpu')
      m.update(got[:120])
      m.update(got[120:])
      assert m.result() == float((want < k).sum()) / 200


def _small(name, shrink=1000):
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', name))
  for fc in list(cfg.feature_config.features) + list(cfg.feature_configs):
    if fc.hash_bucket_size > shrink:
      fc.hash_bucket_size = shrink
  return cfg


def _estimator(cfg, B=32, label_classes=None, **kw):
  est = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=5, **kw).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=6, label_classes=label_classes)
  return est, gen


def test_multiclass_estimator_steps_and_streams_accuracy_and_recall(cpu):
  est, gen = _estimator(_small('deepfm_multicls_criteo.config'), label_classes={'label': 5})
  batches = [gen.next_batch() for _ in range(3)]
  losses = []
  for _ in range(2):
    est.train_step(batches[0])
    losses.append(est.loss_values())
  assert set(losses[0]) == {'cross_entropy_loss', 'regularization_loss', 'total_loss'}
  assert all(np.isfinite(v) for step in losses for v in step.values())
  assert losses[1]['cross_entropy_loss'] < losses[0]['cross_entropy_loss']
  assert est.model.get_outputs() == ['y', 'probs', 'logits', 'probs_y', 'logits_y', 'probs_1', 'logits_1']
  got = est.evaluate(batches)
  hits = {1: 0, 2: 0}
  for batch, pred in est._predict_eval(batches):
    z, y = pred['logits'].numpy(), batch['labels'][0].astype(np.int64)
    assert pred['probs'].shape == (32, 5) and np.array_equal(pred['y'].numpy(), np.argmax(z, axis=1))
    order = np.argsort(-z, axis=1, kind='stable')
    for k in hits:
      hits[k] += int((order[:, :k] == y[:, None]).any(axis=1).sum())
  assert got == {'accuracy': hits[1] / 96.0, 'recall_at_topk': hits[2] / 96.0}
  # the four binary metrics refuse five classes as the reference does; error metrics refuse a multi-class head
  ec = type(est.pipeline_config.eval_config)()
  for kind in ('auc', 'gauc', 'session_auc', 'max_f1'):
    one = type(ec)()
    getattr(one.metrics_set.add(), kind).SetInParent()
    with pytest.raises(ValueError, match='Wrong class number'):
      est.evaluate(batches[:1], one)
  one = type(ec)()
  one.metrics_set.add().mean_absolute_error.SetInParent()
  with pytest.raises(ValueError, match='mean_absolute_error is not supported'):
    est.evaluate(batches[:1], one)


def test_two_class_softmax_head_feeds_the_binary_metrics_with_its_positive_column(cpu):
  cfg = _small('deepfm_multicls_criteo.config')
  cfg.model_config.num_class = 2
  est, gen = _estimator(cfg)
  batch = gen.next_batch()
  est.train_step(batch)
  ec = type(cfg.eval_config)()
  ec.metrics_set.add().auc.SetInParent()
  ec.metrics_set.add().max_f1.SetInParent()
  got = est.evaluate([batch], ec)
  (_, pred), = list(est._predict_eval([batch]))
  label = torch.from_numpy(batch['labels'][0])
  auc = metrics.AUC(200, 'cpu')
  auc.update(label, pred['probs'][:, 1], None)
  f1 = metrics.DeviceMaxF1(200, 'cpu')
  f1.update(label, pred['logits'][:, 1])
  assert got == {'auc': auc.result(), 'max_f1': f1.result()}


def test_jrc_estimator_steps_and_feeds_auc_with_its_probs(cpu):
  est, gen = _estimator(_small('dbmtl_jrc_small_taobao.config'))
  batch = gen.next_batch()
  losses = []
  for _ in range(2):
    est.train_step(batch)
    losses.append(est.loss_values())
  assert set(losses[0]) == {'cross_entropy_loss_ctr', 'jrc_loss_cvr', 'regularization_loss', 'total_loss'}
  assert all(np.isfinite(v) for step in losses for v in step.values())
  assert losses[1]['jrc_loss_cvr'] < losses[0]['jrc_loss_cvr']
  assert est.model.get_outputs() == ['probs_ctr', 'logits_ctr', 'probs_cvr', 'pos_logits_cvr']
  got = est.evaluate([batch])
  (_, pred), = list(est._predict_eval([batch]))
  assert pred['logits_cvr'].shape == (32, 2) and pred['probs_cvr'].shape == (32,)
  _near(pred['probs_cvr'], torch.softmax(pred['logits_cvr'], dim=1)[:, 1], 1e-6)
  auc = metrics.AUC(200, 'cpu')
  auc.update(torch.from_numpy(batch['labels'][1]), pred['probs_cvr'], None)
  assert got['auc_cvr'] == auc.result()
  # the session keys are the id column the embedding sees
  assert torch.equal(est.features.batch_ids_of('user_id'), est.model._session_ids(
      LossType.JRC_LOSS, loss_pb2.JRCLoss(session_name='user_id')))


# ------------------------------------------------------------------------------------------------ the refusals
def test_loss_builder_refusals(cpu):
  z, y, keys = _t('jrc_logits'), _t('jrc_labels'), _t('jrc_sessions')
  with pytest.raises(AssertionError, match='label.dtype must in'):
    loss_builder.build(LossType.CLASSIFICATION, y.double(), _t('smc_c3_logits'), 1.0, 3)
  marked = y.float()
  marked._er_integral = True  # (the device label row of an INT64 field)
  loss_builder.build(LossType.CLASSIFICATION, marked, z, 1.0, 2)
  with pytest.raises(ValueError, match='session_name'):
    loss_builder.build(LossType.JRC_LOSS, y, z, 1.0, 2, loss_param=None, session_ids=keys)
  for strategy in ('random_uniform', 'random_normal', 'random_bernoulli', 'uncertainty'):
    with pytest.raises(NotImplementedError, match=strategy):
      loss_builder.build(LossType.JRC_LOSS, y, z, 1.0, 2, session_ids=keys,
                         loss_param=loss_pb2.JRCLoss(session_name='user_id', loss_weight_strategy=strategy))
  with pytest.raises(ValueError, match='Unsupported loss weight strategy'):
    loss_builder.build(LossType.JRC_LOSS, y, z, 1.0, 2, session_ids=keys,
                       loss_param=loss_pb2.JRCLoss(session_name='user_id', loss_weight_strategy='sometimes'))
  with pytest.raises(AssertionError, match='num_class must be 2'):
    loss_builder.build(LossType.JRC_LOSS, y, z, 1.0, 3, session_ids=keys, loss_param=loss_pb2.JRCLoss(session_name='u'))
  with pytest.raises(NotImplementedError, match='ZILN_LOSS'):
    loss_builder.build(LossType.ZILN_LOSS, y, _t('smc_c3_logits'), 1.0, 3)
  with pytest.raises(AssertionError, match='num_class must be 1'):
    loss_builder.build(LossType.BINARY_CROSS_ENTROPY_LOSS, y, z, 1.0, 2)


def _jrc_tower(cfg):
  return cfg.model_config.dbmtl.task_towers[1]


def test_build_time_refusals(cpu):
  def build(cfg, **kw):
    return EasyRecEstimator(cfg, device='cpu', batch_size=16, seed=1, **kw).build()
  cfg = _small('dbmtl_jrc_small_taobao.config')
  _jrc_tower(cfg).losses[0].jrc_loss.ClearField('session_name')
  with pytest.raises(ValueError, match='session_name'):
    build(cfg)
  cfg = _small('dbmtl_jrc_small_taobao.config')
  _jrc_tower(cfg).losses[0].jrc_loss.session_name = 'no_such_feature'
  with pytest.raises(ValueError, match='no_such_feature'):
    build(cfg)
  for strategy in ('random_uniform', 'uncertainty'):
    cfg = _small('dbmtl_jrc_small_taobao.config')
    _jrc_tower(cfg).losses[0].jrc_loss.loss_weight_strategy = strategy
    with pytest.raises(NotImplementedError, match=strategy):
      build(cfg)
  cfg = _small('dbmtl_jrc_small_taobao.config')
  _jrc_tower(cfg).num_class = 3
  with pytest.raises(AssertionError, match='num_class must be 2'):
    build(cfg)
  cfg = _small('dbmtl_jrc_small_taobao.config')
  _jrc_tower(cfg).losses[0].loss_type = LossType.ZILN_LOSS
  with pytest.raises(NotImplementedError, match='ZILN_LOSS'):
    build(cfg)
  for name in ('deepfm_multicls_criteo.config', 'dbmtl_jrc_small_taobao.config'):
    with pytest.raises(ValueError, match='bf16'):
      build(_small(name), dense_dtype='bf16')
  cfg = _small('deepfm_multicls_criteo.config')
  kd = cfg.model_config.kd.add()
  kd.soft_label_name, kd.pred_name = 'label', 'logits'
  with pytest.raises(NotImplementedError, match='kd'):
    build(cfg)
  # a FLOAT label field under a multi-class head: the reference's dtype assertion, at the first step
  cfg = _small('deepfm_multicls_criteo.config')
  cfg.data_config.input_fields[0].input_type = cfg.data_config.FLOAT
  est, gen = _estimator(cfg)
  with pytest.raises(AssertionError, match='label.dtype must in'):
    est.train_step(gen.next_batch())


def test_embedding_parallel_engine_is_refused():
  from easyrec_amd.layers.sharded_embedding import ShardedEmbeddingEngine
  m = _bare_model({})
  m._base_model_config = types.SimpleNamespace(kd=[])
  ctx = context.ModelContext(None, ShardedEmbeddingEngine.__new__(ShardedEmbeddingEngine), is_training=True)
  with context.use(ctx):
    m._check_head(LossType.CLASSIFICATION, 1)  # a binary head passes
    with pytest.raises(ValueError, match='embedding-parallel'):
      m._check_head(LossType.CLASSIFICATION, 5)
    with pytest.raises(ValueError, match='embedding-parallel'):
      m._check_head(LossType.JRC_LOSS, 2, loss_pb2.JRCLoss(session_name='user_id'))


def test_switch_and_envelopes(monkeypatch):
  assert mcl.fused_enabled() == (os.environ.get('EASYREC_AMD_FUSED_MULTICLASS', mcl.FUSED_DEFAULT) != '0')
  monkeypatch.setenv('EASYREC_AMD_FUSED_MULTICLASS', '0')
  assert not mcl.fused_enabled()
  monkeypatch.setenv('EASYREC_AMD_FUSED_MULTICLASS', '1')
  assert mcl.fused_enabled() and not mcl._on_kernels(torch.zeros(4, 3))  # a CPU tensor never goes to the kernels
  assert mcl.softmax_ce_fits(1, 2) and mcl.softmax_ce_fits(10, 4096) and not mcl.softmax_ce_fits(10, 4097)
  assert not mcl.softmax_ce_fits(10, 1) and mcl.jrc_fits(8192) and not mcl.jrc_fits(8193) and not mcl.jrc_fits(0)


def test_synthetic_label_classes_keyword_leaves_the_default_stream_alone():
  cfg = _small('dbmtl_jrc_small_taobao.config')
  fcs = config_util.get_compatible_feature_configs(cfg)
  plain = SyntheticBatches(cfg.data_config, fcs, batch_size=64, seed=9).next_batch()
  again = SyntheticBatches(cfg.data_config, fcs, batch_size=64, seed=9, label_classes=None).next_batch()
  assert all(np.array_equal(plain[k], again[k]) for k in plain)
  assert set(np.unique(plain['labels'])) <= {0.0, 1.0}
  drawn = SyntheticBatches(cfg.data_config, fcs, batch_size=4096, seed=9, label_classes={'buy': 7}).next_batch()
  assert set(np.unique(drawn['labels'][1])) == set(float(c) for c in range(7))
  assert set(np.unique(drawn['labels'][0])) <= {0.0, 1.0}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='the reference checkout is not on this machine')
def test_reference_config_count():
  """159 of 224: the four multi-class / JRC configs of the reference now build and step; deepfm_multi_cls_small stays out
  for its `kd` section (knowledge distillation is not built), which it says itself."""
  import subprocess
  import sys
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'count_reference_configs.py'), REFERENCE, '-v'],
                       capture_output=True, text=True, check=True).stdout
  assert out.splitlines()[0] == '159 of 224 build and step', out.splitlines()[0]
  failed = {line.split(' -> ')[0]: line for line in out.splitlines() if ' -> ' in line}
  for name in ('deepfm_multi_cls_on_avazu_ctr.config', 'deepfm_distribute_eval_multi_cls_on_avazu_ctr.config',
               'wide_and_deep_no_final_on_avazau_ctr.config', 'dbmtl_on_taobao_with_multi_loss.config'):
    assert name not in failed, failed[name]
  assert 'kd' in failed['deepfm_multi_cls_small.config']
