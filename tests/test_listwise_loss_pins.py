"""The listwise ranking losses' torch compositions (easyrec_amd/builders/listwise_loss.py), through loss_builder.build on
the CPU in fp64, against values and central-difference gradients of the reference's own loss/listwise_loss.py
(tests/golden/listwise_loss_vectors.npz, written by tests/golden/make_listwise_loss_vectors.py); the build-time refusals,
the scale variables' names and two estimator steps on the stand-in backend."""
import logging
import os
import types

import numpy as np
import pytest
import torch

from easyrec_amd import kernels
from easyrec_amd.builders import listwise_loss as lwl
from easyrec_amd.builders import loss_builder
from easyrec_amd.core import context
from easyrec_amd.input.synthetic import SyntheticBatches
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
from easyrec_amd.model.rank_model import RankModel
from easyrec_amd.protos import loss_pb2
from easyrec_amd.utils import config_util
from oracle.kernel_ref import RefBackend

LT = loss_pb2.LossType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = np.load(os.path.join(ROOT, 'tests', 'golden', 'listwise_loss_vectors.npz'))
RANK, DISTILL = loss_pb2.ListwiseRankLoss, loss_pb2.ListwiseDistillLoss

# fixture entry -> (loss type, loss_param, the labels' array, the sample weight)
CASES = {
    'rank': (LT.LISTWISE_RANK_LOSS, RANK(session_name='u'), 'labels', 1.0),
    'rank_logits_t': (LT.LISTWISE_RANK_LOSS, RANK(session_name='u', label_is_logits=True, temperature=0.5), 'labels', 1.0),
    'rank_scale_t': (LT.LISTWISE_RANK_LOSS, RANK(session_name='u', scale_logits=True, temperature=2.0), 'labels', 1.0),
    'rank_logits_fn_w': (LT.LISTWISE_RANK_LOSS, RANK(session_name='u', label_is_logits=True, temperature=2.0,
                                                     transform_fn='lambda x: x * 2.0 + 1.0'), 'labels', 0.5),
    'distill': (LT.LISTWISE_DISTILL_LOSS, DISTILL(session_name='u'), 'positions', 1.0),
    'distill_clip_scale_t': (LT.LISTWISE_DISTILL_LOSS, DISTILL(session_name='u', label_clip_max_value=64.0, scale_logits=True,
                                                               temperature=0.5), 'positions', 1.0),
    'distill_fn': (LT.LISTWISE_DISTILL_LOSS, DISTILL(session_name='u', transform_fn='lambda x: 1.0 / x'), 'positions', 2.0),
    'rank_tensor_weights': (LT.LISTWISE_RANK_LOSS, RANK(session_name='u'), 'labels', torch.full((40,), 3.0)),  # ignored
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_composition_matches_the_reference(name):
  loss_type, param, labels, weight = CASES[name]
  scale = None
  if param.scale_logits:
    scale = tuple(torch.tensor([v], dtype=torch.float64, requires_grad=True) for v in VEC[name + '_scale'])
  loss, dz = loss_builder.build(loss_type, torch.from_numpy(VEC[labels]), torch.from_numpy(VEC['logits']), weight,
                                loss_param=param, session_ids=torch.from_numpy(VEC['sessions']), scale_vars=scale)
  assert abs(float(loss) - float(VEC[name])) <= 1e-12 * max(1.0, abs(float(VEC[name])))
  # (central differences at h = 1e-6 of an fp64 forward: ~1e-9 absolute)
  assert float(np.abs(dz.numpy() - VEC[name + '_grad']).max()) <= 1e-7
  if scale:
    assert float(np.abs(np.array([float(v.grad) for v in scale]) - VEC[name + '_scale_grad']).max()) <= 1e-7


def _config(kind='listwise_rank_loss', **fields):
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'multi_tower_f1_pairwise_criteo_small.config'))
  entry = cfg.model_config.losses[1]
  entry.loss_type = LT.Value(kind.upper())
  getattr(entry, kind).temperature = 1.0  # (selects the oneof)
  for k, v in fields.items():
    setattr(getattr(entry, kind), k, v)
  return cfg


def test_build_time_refusals(monkeypatch):
  monkeypatch.setattr(kernels, '_BACKEND', RefBackend())
  build = lambda cfg, **kw: EasyRecEstimator(cfg, device='cpu', batch_size=16, seed=1, **kw).build()  # noqa: E731
  for kind in ('listwise_rank_loss', 'listwise_distill_loss'):
    with pytest.raises(ValueError, match='session_name'):
      build(_config(kind))
    with pytest.raises(ValueError, match='F1'):  # a raw feature is no id feature
      build(_config(kind, session_name='F1'))
    with pytest.raises(ValueError, match='bf16'):
      build(_config(kind, session_name='C1'), dense_dtype='bf16')
    with pytest.raises(ValueError, match='no_such_module.no_fn'):
      build(_config(kind, session_name='C1', transform_fn='no_such_module.no_fn'))
  from easyrec_amd.layers.sharded_embedding import ShardedEmbeddingEngine
  m = RankModel.__new__(RankModel)
  m._feature_dict = types.SimpleNamespace()
  with context.use(context.ModelContext(None, ShardedEmbeddingEngine.__new__(ShardedEmbeddingEngine), is_training=True)):
    with pytest.raises(ValueError, match='embedding-parallel'):
      m._check_head(LT.LISTWISE_RANK_LOSS, 1, RANK(session_name='C1'))


@pytest.mark.parametrize('kind,scope', [('listwise_rank_loss', 'listwise_loss'), ('listwise_distill_loss', 'listwise_distill_loss')])
def test_two_steps_on_the_stand_in_against_the_composition(monkeypatch, kind, scope):
  """The pairwise config with its second loss replaced: the loss key is the reference's, the scale variables carry its
  names and train, and each step's value is the composition's on the same logits, labels, keys and scale values."""
  monkeypatch.setattr(kernels, '_BACKEND', RefBackend())
  monkeypatch.setattr(logging.root.manager, 'disable', logging.ERROR)
  seen, inner = [], lwl.build

  def spy(loss_type, label, pred, loss_weight, loss_scale, loss_param, session_ids, scale_vars=None):
    out = inner(loss_type, label, pred, loss_weight, loss_scale, loss_param, session_ids, scale_vars)
    sw, sb = lwl.scale_variables(lwl.params_of(loss_type, loss_param))
    want = lwl.compose(loss_type, label.double(), pred.detach().double(), session_ids, lwl.params_of(loss_type, loss_param),
                       sw.detach().double(), sb.detach().double()) * loss_scale
    seen.append((float(out[0]), float(want), len(torch.unique(session_ids))))
    return out
  monkeypatch.setattr(lwl, 'build', spy)
  cfg = _config(kind, session_name='C1', scale_logits=True, temperature=2.0)
  est = EasyRecEstimator(cfg, device='cpu', batch_size=64, seed=11).build()
  before = est.state_dict()
  assert float(before[scope + '/scale_w'][0]) == 1.0 and float(before[scope + '/scale_b'][0]) == 0.0
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=64, seed=111)
  for step in range(2):
    est.train_step(gen.next_batch())
    got, want, sessions = seen[step]
    assert 1 < sessions < 64 and est.loss_values()[kind] == pytest.approx(got, rel=1e-6)
    assert abs(got - want) <= 1e-5 * max(1e-3, abs(want)), (step, got, want)
  assert float(est.state_dict()[scope + '/scale_w'][0]) != 1.0  # (scale_b's gradient is zero: softmax is shift invariant)
