"""MIND on the CPU: the class resolves, the restatement (oracle/mind_ref.py) and the product's composed capsule layer,
attention and interest similarity hold the reference's own outputs (tests/golden/mind_vectors.npz, written by
tests/golden/make_mind_vectors.py) to 1e-6 of their scale in fp64, the evaluation routing table is the seeded numpy draw,
the capsule count is int(log(float32(len))) for every length, both committed configs train on the stand-in backend with
the restatement's losses, and a sampler is refused."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from _oracle_steps import covers, first_steps
from easyrec_amd.layers import capsule_layer
from oracle import mind_ref as ref
from easyrec_amd.utils import load_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'mind_vectors.npz'))
GOLD_CASES = sorted({k.split(':')[0] for k in GOLD.files})


def _make_configs():
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  return make_configs


def mind_cfg(list_wise=False, batch_size=16):
  return _make_configs().mind_taobao(list_wise=list_wise, batch_size=batch_size, scale=0.01)


def gold_case(tag):
  """(options, the `mind` message, loss type, {name: fp64 tensor} of the case's arrays, {name: variable}, the sequences in
  group order)"""
  from google.protobuf import text_format
  from easyrec_amd.protos import mind_pb2
  from easyrec_amd.protos.loss_pb2 import LossType
  o = json.loads(str(GOLD[tag + ':opts']))
  msg = text_format.Merge(o['config'], mind_pb2.MIND())
  arr = {k.split(':', 1)[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files
         if k.startswith(tag + ':') and ':var:' not in k and ':seq:' not in k and GOLD[k].dtype.kind in 'fi'}
  var = {k.split(':var:')[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith(tag + ':var:')}
  seqs = {k.split(':seq:')[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith(tag + ':seq:')}
  return o, msg, getattr(LossType, o['loss']), arr, var, seqs


def gold_logits0(o, msg, arr):
  """the routing logits the case ran with: the stored draw, or the evaluation table"""
  if o['training']:
    return arr['routing_logits']
  c = msg.capsule_config
  return torch.from_numpy(capsule_layer.eval_routing_logits(c.max_seq_len, c.max_k, c.routing_logits_stddev)).double()


def hold(got, want, what):
  """1e-6 of the array's scale"""
  got, want = got.detach().double(), want.double()
  scale = max(float(want.abs().max()), 1e-3)
  assert float((got - want).abs().max()) <= 1e-6 * scale, (what, float((got - want).abs().max()), scale)


def test_model_class_is_registered():
  load_class.import_all_models()
  from easyrec_amd.model.easy_rec_model import _EASY_REC_MODEL_CLASS_MAP
  assert 'MIND' in _EASY_REC_MODEL_CLASS_MAP


def test_fixture_covers_the_cases():
  assert GOLD_CASES == sorted(['train', 'eval', 'scale0', 'const', 'squash', 'short', 'concat', 'time', 'pow100', 'list',
                               'simi_reg'])
  o, msg, _, arr, _, seqs = gold_case('train')
  assert arr['lens'].tolist() == [0, 1, 8, 21, 30, 13] and msg.capsule_config.max_seq_len == 24
  assert seqs['cate_seq'].shape[1] == 30 and gold_case('short')[5]['cate_seq'].shape[1] == 10  # L > S and L < S
  assert arr['num_high_capsules'].tolist() == [1, 1, 2, 3, 3, 2]
  assert gold_case('const')[3]['num_high_capsules'].tolist() == [4] * 6


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_restatement_holds_the_fixture(tag):
  o, msg, loss_type, arr, var, seqs = gold_case(tag)
  hist = ref.combine_hist(msg, seqs, arr['lens'])
  ids = torch.tensor(o['ids']) if 'ids' in o else None
  losses, pred = ref.mind_forward(msg, loss_type, hist, arr['lens'], arr['user'], arr['item'], var,
                                  gold_logits0(o, msg, arr), arr['label'], ids, training=o['training'])
  assert pred['user_emb_num'].tolist() == arr['num_high_capsules'].tolist()
  for k in ('high_capsules', 'user_interests', 'user_tower_emb', 'item_tower_emb', 'logits', 'probs', 'interests_simi'):
    hold(pred[k], arr[k], k)
  want = {k.split('loss:')[1]: v for k, v in arr.items() if k.startswith('loss:')}
  assert set(losses) == set(want)
  for k, v in want.items():
    hold(losses[k], v, k)


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_composed_layer_holds_the_fixture(tag):
  """the product's own composition (layers/capsule_layer.py, model/mind.py interest_similarity) in fp64, between the
  restatement's towers"""
  from easyrec_amd.model.mind import interest_similarity
  from easyrec_amd.protos.simi_pb2 import Similarity
  o, msg, loss_type, arr, var, seqs = gold_case(tag)
  c = msg.capsule_config
  hist = ref.combine_hist(msg, seqs, arr['lens'])
  high, ncaps = capsule_layer.capsule_compose(hist, arr['lens'], var['capsule/S'], gold_logits0(o, msg, arr), c.max_seq_len,
                                              c.max_k, c.num_iters, c.routing_logits_scale, c.squash_pow, c.scale_ratio,
                                              c.const_caps_num)
  assert ncaps.dtype == torch.int32 and ncaps.tolist() == arr['num_high_capsules'].tolist()
  hold(high, arr['high_capsules'], 'high_capsules')
  B, K, _ = high.shape
  t = o['training']
  u = ref.dnn(ref.batch_norm(arr['user'], var, 'user_fea_bn', t), var, 'user_dnn', training=t)
  ui = torch.cat([high, u[:, None, :].expand(B, K, u.shape[1])], dim=2).reshape(B * K, -1)
  ui = ref.dnn(ui, var, 'concat_dnn', last_plain=True, training=t).reshape(B, K, -1)
  it = arr['item_tower_emb']
  if msg.simi_func == Similarity.COSINE:
    ui = capsule_layer.normalize_compose(ui)
  emb, ui = capsule_layer.attention_compose(ui, it, ncaps, msg.simi_pow)
  hold(emb, arr['user_tower_emb'], 'user_tower_emb')
  hold(ui, arr['user_interests'], 'user_interests')
  hold(interest_similarity(ui, high, ncaps)[0], arr['interests_simi'], 'interests_simi')


def test_eval_routing_table_is_the_seeded_draw():
  state = np.random.get_state()
  for S, K, std in [(64, 5, 1.0), (24, 4, 0.5), (1, 1, 2.0)]:
    got = capsule_layer.eval_routing_logits(S, K, std)
    np.random.seed(28)
    want = np.random.uniform(high=std, size=[S, K]).astype(np.float32)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
  np.random.set_state(state)
  # the layer hands the same table to every batch outside training, and does not disturb numpy's generator
  import types
  cfg = types.SimpleNamespace(max_seq_len=24, max_k=4, high_dim=5, num_iters=3, routing_logits_scale=20.0,
                              routing_logits_stddev=1.0, squash_pow=1.0, scale_ratio=1.0, const_caps_num=False)
  np.random.seed(5)
  first = np.random.random()
  np.random.seed(5)
  table = capsule_layer.CapsuleLayer(cfg, False).routing_logits(3, 'cpu')
  assert np.random.random() == first and table.shape == (24, 4)
  assert table.numpy().tobytes() == capsule_layer.eval_routing_logits(24, 4, 1.0).tobytes()
  noise = capsule_layer.CapsuleLayer(cfg, True).routing_logits(3, 'cpu')
  assert noise.shape == (3, 24, 4) and float(noise.abs().max()) <= 2.0


def test_capsule_count_is_int_log_float32_of_the_length():
  lens = np.arange(0, 3001)
  for K in (1, 5, 8):
    with np.errstate(divide='ignore'):
      logs = np.log(lens.astype(np.float32))
    want = np.array([max(1, min(K, int(v))) if np.isfinite(v) else 1 for v in logs])
    got = capsule_layer.num_capsules(torch.from_numpy(lens), 3000, K, False)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    assert np.array_equal(ref.num_capsules(lens, 3000, K, False).numpy(), want)
  # the thresholds are where the count steps, and clipping to max_seq_len comes first
  assert [int(np.log(np.float32(t))) for t in capsule_layer.CAPS_THRESHOLDS] == [2, 3, 4, 5, 6, 7, 8]
  assert [int(np.log(np.float32(t - 1))) for t in capsule_layer.CAPS_THRESHOLDS] == [1, 2, 3, 4, 5, 6, 7]
  assert capsule_layer.num_capsules(torch.tensor([100, 7, -3]), 20, 8, False).tolist() == [2, 1, 1]
  assert capsule_layer.num_capsules(torch.tensor([100, 7, 0]), 20, 6, True).tolist() == [6, 6, 6]


def test_fp32_composition_leaves_the_gpu_bars_a_factor_of_four():
  """What tests/test_mind_gpu.py's capsule cases rest their default bars on: the same ops in fp32 torch on the CPU sit
  within a quarter of 1e-5 (forward) / 1e-4 (gradients) of fp64 on every case."""
  import test_mind_gpu as gpu

  def compose(hist, lens, Smat, l0, *cfg):
    return capsule_layer.capsule_compose(hist, lens, Smat, l0, *cfg)

  for tag in sorted(gpu.CAPSULE_CASES):
    c = gpu.capsule_case(**gpu.CAPSULE_CASES[tag])
    want = gpu.capsule_reference(c)
    got = gpu.capsule_reference(c, fn=compose, dtype=torch.float32)
    assert got[1].tolist() == want[1].tolist()
    for i, bar in ((0, 1e-5), (2, 1e-4), (3, 1e-4)):
      err = float((got[i].double() - want[i]).abs().max() / want[i].abs().max())
      assert 4 * err <= bar, (tag, i, err)


def test_lds_formula():
  assert capsule_layer.lds_bytes(64, 16, 64, 5) == 4 * (64 * 17 + 64 * 65 + 64 * 5 + 2 * 5 * 65 + 64) == 25128
  assert capsule_layer.lds_bytes(128, 128, 128, 8) == 144960
  for bad in [(129, 16, 64, 5), (64, 129, 64, 5), (64, 16, 129, 5), (64, 16, 64, 9), (0, 16, 64, 5)]:
    assert capsule_layer.lds_bytes(*bad) == 0


@pytest.mark.parametrize('name,list_wise', [('mind_taobao_10m.config', False), ('mind_inbatch_taobao_10m.config', True)])
def test_committed_configs_are_the_generated_ones(name, list_wise):
  from easyrec_amd.protos.loss_pb2 import LossType
  from easyrec_amd.utils import config_util
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', name))
  assert cfg == _make_configs().mind_taobao(list_wise=list_wise, item_rows=10000000)
  mc = cfg.model_config
  assert mc.model_class == 'MIND' and [g.group_name for g in mc.feature_groups] == ['hist', 'user', 'item']
  assert list(mc.mind.user_dnn.hidden_units) == [256, 128, 64, 32] == list(mc.mind.item_dnn.hidden_units)
  assert list(mc.mind.concat_dnn.hidden_units) == [64, 32]
  c = mc.mind.capsule_config
  assert (c.max_k, c.max_seq_len, c.high_dim, c.num_iters) == (5, 64, 64, 3)
  assert cfg.data_config.batch_size == 4096 and cfg.data_config.WhichOneof('sampler') is None
  assert mc.loss_type == (LossType.SOFTMAX_CROSS_ENTROPY if list_wise else LossType.CLASSIFICATION)


def mind_coverage(names, cfg):
  covers(names, cfg, {'capsule/S', 'concat_dnn/dnn_0/kernel', 'user_dnn/dnn_0/kernel', 'item_dnn/dnn_0/kernel', 'sim_w'},
         groups=('hist', 'user', 'item'))


def hand_over_routing_logits(seen=None):
  """first_steps' after_step for MIND: the oracle runs the step on the routing logits the product drew (kept in `seen`)"""
  def after_step(est, orc, step, batch):
    orc.routing_logits = est.model._capsule_layer.last_routing_logits.detach().cpu().numpy()
    if seen is not None:
      seen.append(orc.routing_logits.copy())
  return after_step


@pytest.mark.parametrize('list_wise', [False, True])
def test_model_builds_and_steps_on_the_stand_in(ref_backend, built_lib, list_wise):
  """Two steps against the fp64 model oracle from the batch on, run on the routing logits each step drew
  (tests/_oracle_steps.first_steps)."""
  from easyrec_amd.input.synthetic import SyntheticBatches
  B = 16
  cfg = mind_cfg(list_wise, B)
  noise = []
  est = first_steps(cfg, B, seed=4, device='cpu', oracle_dtype=torch.float64, coverage=mind_coverage,
                    after_step=hand_over_routing_logits(noise))
  st = est.state_dict()
  assert st['capsule/S'].shape == (16, 64) and est.varstore.l2_of('capsule/S') == 0.0
  assert st['concat_dnn/dnn_0/kernel'].shape == (96, 64) and st['concat_dnn/dnn_1/kernel'].shape == (64, 32)
  assert 'concat_dnn/dnn_1/bn/gamma' not in st and 'item_dnn/dnn_3/bn/gamma' not in st and 'user_dnn/dnn_3/bn/gamma' in st
  assert 'user_fea_bn/gamma' in st and 'sim_w' in st
  assert noise[0].shape == (B, 64, 5) and not np.array_equal(noise[0], noise[1])
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=44)
  # evaluation: the shared table, the interest metrics beside MatchModel's
  est.model._is_training = est.ctx.is_training = False
  pred = est.predict(gen.next_batch())
  assert est.model._capsule_layer.last_routing_logits.shape == (64, 5)
  assert pred['user_interests'].shape == (B, 5, 32) and pred['high_capsules'].shape == (B, 5, 64)
  assert pred['user_emb_num'].dtype == torch.int32 and 'logits' in pred
  metrics = est.model.build_metric_graph(cfg.eval_config)
  extra = {'recall@10', 'recall_neg_sam@10', 'recall_in_batch@10', 'interests_recall@10',
           'interests_neg_sam_recall@10'} if list_wise else {'auc'}
  assert set(metrics) == {'interest_similarity', 'capsule_similarity'} | extra
  out = est.model.build_output_dict()
  assert set(out) == {'logits', 'probs', 'user_emb', 'item_emb', 'user_emb_num', 'user_interests', 'item_tower_emb'}
  assert len(out['user_emb']) == B and out['user_emb'][0].count('|') == 4 and out['user_emb'][0].count(',') == 5 * 31


def test_interest_similarity_loss_joins_the_losses(ref_backend, built_lib):
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  cfg = mind_cfg(False)
  cfg.model_config.mind.max_interests_simi = 0.5
  est = EasyRecEstimator(cfg, device='cpu', batch_size=16, seed=4).build()
  est.train_step(SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=16, seed=44).next_batch())
  got = est.loss_values()
  assert got['reg_interest_simi'] == pytest.approx(max(0.0, float(est.model._prediction_dict['interests_simi'].detach()) - 0.5),
                                                   abs=1e-6)


@pytest.mark.parametrize('sampler', ['negative_sampler', 'negative_sampler_v2', 'hard_negative_sampler',
                                     'hard_negative_sampler_v2'])
def test_samplers_are_refused(ref_backend, sampler):
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  cfg = mind_cfg(True)
  getattr(cfg.data_config, sampler).SetInParent()
  with pytest.raises(NotImplementedError, match=sampler + ':'):
    EasyRecEstimator(cfg, device='cpu', batch_size=16, seed=4)


def test_other_refusals(ref_backend):
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  from easyrec_amd.model.embedding_parallel import EmbeddingParallelEstimator
  with pytest.raises(ValueError, match='MIND: dense_dtype bf16'):
    EasyRecEstimator(mind_cfg(), device='cpu', batch_size=16, seed=4, dense_dtype='bf16')
  with pytest.raises(ValueError, match='MIND: embedding-parallel'):
    EmbeddingParallelEstimator(mind_cfg(), device='cpu', batch_size=16, seed=4, rank=0, world=1)
