"""Variational dropout on the CPU: the fp64 restatement and the product's torch composition reproduce the reference's
own outputs (tests/golden/vdrop_vectors.npz) under the reference's variable names and shapes; the three things the
reference leaves un-dropped; the penalty as a loss of its own; what is rejected at build time; the Python envelope
helper is the library's; the committed configs are the generated ones; the feature ranking; the checkpoint tool; and
the reference's six variational-dropout configs build and step on a stand-in backend."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from easyrec_amd.core.variables import VarStore
from easyrec_amd.protos import variational_dropout_pb2
from oracle.kernel_ref import RefBackend
from tests import _vdrop_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = '/root/reference'
GOLD = vc.gold()
TAGS = ['ew_train', 'fw_train', 'ew_eval', 'fw_eval', 'seq', 'two_deep', 'two_wide']
SIX = ['dbmtl_variational_dropout', 'dbmtl_variational_dropout_feature_num',
       'dbmtl_variational_dropout_on_sequence_feature_taobao', 'deepfm_combo_variational_dropout_on_avazu_ctr',
       'din_varitional_dropout_on_taobao', 'fm_variational_dropout_on_taobao']


def gold_case(tag):
  """-> dict: x (the concatenation before dropout), dims (feature -> width, in its order), logit_p, u (None outside
  training), out, penalty, and the flags; fp64"""
  g = lambda k: GOLD['%s:%s' % (tag, k)]
  names, widths = [str(n) for n in g('plain_names')], [int(d) for d in g('plain_dims')]
  parts = [GOLD['%s:x:%s' % (tag, n)] for n in names]
  group, dims = json.loads(str(g('collection')))
  c = {'group': str(g('group')), 'embedding_wise': bool(g('embedding_wise')), 'training': bool(g('training')),
       'lambda': float(g('lambda')), 'plain': OrderedDict(zip(names, parts)), 'dims': OrderedDict(dims),
       'logit_p': torch.from_numpy(g('logit_p')), 'var_name': str(g('var_name')),
       'u': torch.from_numpy(g('u')) if bool(g('training')) else None, 'out': torch.from_numpy(g('out')),
       'penalty': float(g('penalty')), 'feats': [GOLD['%s:feat:%d' % (tag, i)] for i in range(int(g('n_feats')))]}
  assert group == c['group'] and list(c['dims'].items())[:len(names)] == list(zip(names, widths))
  return c


def seq_pooled(tag):
  """the attention-pooled sequence column of the `seq` case, from the fixture's inputs (layers/input_layer.py:323-338)"""
  x, lens = torch.from_numpy(GOLD[tag + ':seq_x']), torch.from_numpy(GOLD[tag + ':seq_len'])
  w = torch.from_numpy(GOLD[tag + ':var:hist_embedding/attention/kernel'])
  logits = (x @ w).squeeze(-1)
  mask = torch.arange(x.shape[1])[None, :] < lens[:, None]
  score = torch.softmax(torch.where(mask, logits, torch.full_like(logits, -2.0 ** 32 + 1)), dim=-1)
  return (score[:, :, None] * x).sum(dim=1)


def before_dropout(tag, c):
  parts = [torch.from_numpy(p) for p in c['plain'].values()]
  if tag == 'seq':
    parts.append(seq_pooled(tag))
  return torch.cat(parts, dim=1)


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_covers_the_cases():
  cases = {t: gold_case(t) for t in TAGS}
  assert all(c['out'].shape[0] <= 6 and c['out'].shape[1] <= 12 for c in cases.values())
  assert list(cases['ew_train']['dims'].values()) == [1, 3, 4] == list(cases['fw_train']['dims'].values())
  assert cases['ew_train']['embedding_wise'] and cases['ew_train']['training'] and cases['ew_train']['logit_p'].shape == (8,)
  assert not cases['fw_train']['embedding_wise'] and cases['fw_train']['logit_p'].shape == (3,)
  assert not cases['ew_eval']['training'] and not cases['fw_eval']['training'] and cases['ew_eval']['u'] is None
  # the group `all` against a named group
  assert cases['ew_train']['group'] == 'all' and cases['ew_train']['var_name'] == 'logit_p'
  assert cases['fw_train']['group'] == 'g' and cases['fw_train']['var_name'] == 'logit_p_g'
  # the sequence column comes after the plain ones
  assert list(cases['seq']['dims'].items()) == [('age', 2), ('city', 3), ('hist', 4)]
  assert cases['seq']['var_name'] == 'logit_p_user' and cases['seq']['logit_p'].shape == (3,)
  # two groups with row counts of their own
  assert cases['two_deep']['out'].shape[0] == 6 and cases['two_wide']['out'].shape[0] == 5
  assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'vdrop_vectors.npz')) < 100000


@pytest.mark.parametrize('tag', TAGS)
def test_restatement_matches_the_reference(tag):
  c = gold_case(tag)
  x = before_dropout(tag, c)
  out, pen = vc.vdrop(x, c['logit_p'], c['u'], list(c['dims'].values()), c['embedding_wise'], c['lambda'])
  assert out.shape == c['out'].shape
  assert float((out - c['out']).abs().max()) <= 1e-12 * float(c['out'].abs().max())
  assert abs(float(pen) - c['penalty']) <= 1e-12 * abs(c['penalty'])


def test_the_summed_penalty_is_the_loss():
  loss = float(GOLD['two:loss'])
  assert abs(loss - (gold_case('two_deep')['penalty'] + gold_case('two_wide')['penalty'])) <= 1e-15
  # (each group divides by its own row count)
  for tag in ('two_deep', 'two_wide'):
    c = gold_case(tag)
    p = torch.sigmoid(c['logit_p'])
    assert abs(c['lambda'] / c['out'].shape[0] * float((1 - p).sum()) - c['penalty']) <= 1e-12 * c['penalty']


def test_what_the_reference_leaves_undropped():
  """the fixture shows each quirk: the dict handed to the target attention and the embedding L2's weights hold the
  tensors BEFORE dropout; the returned feature list is the split of the tensor AFTER it"""
  c = gold_case('seq')
  x = before_dropout('seq', c)
  pooled = seq_pooled('seq')
  for name, part in c['plain'].items():
    assert np.array_equal(GOLD['seq:dict:' + name], part)
  assert not any(k.startswith('seq:dict:hist') for k in GOLD.files)  # (only feature_column.input_layer fills the dict)
  # weights_list: the sequence column's embeddings over time, then every column's output, all before dropout
  reg = [GOLD['seq:reg:%d' % i] for i in range(4)]
  assert 'seq:reg:4' not in GOLD.files
  assert np.array_equal(reg[0], GOLD['seq:seq_x'])
  for got, want in zip(reg[1:], list(c['plain'].values()) + [pooled.numpy()]):
    assert np.abs(got - want).max() <= 1e-12
  # the feature list: the split of the dropped tensor, in the concatenation's order
  widths = list(c['dims'].values())
  assert [f.shape[1] for f in c['feats']] == widths
  assert np.array_equal(np.concatenate(c['feats'], axis=1), c['out'].numpy())
  assert float((c['out'] - x).abs().max()) > 1e-3  # (the dropout did act)


# ------------------------------------------------------------------------------------------------ the product's layer
class _Ctx(object):
  """The piece of the build context the layer reads."""

  def __init__(self, vs, dense_dtype='f32'):
    self.varstore, self.dense_dtype = vs, dense_dtype
    self.is_training, self.building, self.engine = True, True, None
    self.vdrop_losses = []


@pytest.fixture
def cpu_context(monkeypatch):
  from easyrec_amd import kernels
  from easyrec_amd.core import context
  monkeypatch.setattr(kernels, '_BACKEND', RefBackend())

  def make(dense_dtype='f32'):
    ctx = _Ctx(VarStore('cpu'), dense_dtype)
    monkeypatch.setattr(context, 'current', lambda: ctx)
    monkeypatch.setattr(context, 'varstore', lambda: ctx.varstore)
    return ctx
  return make


def _config(c):
  return variational_dropout_pb2.VariationalDropoutLayer(regularization_lambda=c['lambda'],
                                                         embedding_wise_variational_dropout=c['embedding_wise'])


@pytest.mark.parametrize('tag', TAGS)
def test_product_variables_and_outputs_are_the_reference_s(tag, cpu_context):
  """The variable's name and shape, no L2, the collection entry; and from the fixture's variable and noise the
  composition's output and penalty at 1e-5, rounded to the product's fp32."""
  from easyrec_amd.layers.variational_dropout_layer import VariationalDropoutLayer
  c = gold_case(tag)
  ctx = cpu_context()
  layer = VariationalDropoutLayer(_config(c), c['dims'], c['training'], name=c['group'])
  vs = ctx.varstore
  assert vs.names() == [c['var_name']] and tuple(layer.logit_p.shape) == tuple(c['logit_p'].shape)
  assert vs.l2_of(c['var_name']) == 0.0 and layer.logit_p.requires_grad
  assert json.loads(layer.collection_entry) == json.loads(str(GOLD[tag + ':collection']))
  # tf.get_variable's default initializer: glorot uniform with fan_in = fan_out = P
  P = layer.logit_p.numel()
  assert float(layer.logit_p.detach().abs().max()) <= np.sqrt(6.0 / (2 * P)) + 1e-6
  vs.load_state_dict({c['var_name']: c['logit_p'].numpy()}, strict=False)
  x = before_dropout(tag, c).float()
  u = None if c['u'] is None else c['u'].float()
  out, pen = layer.apply(x, u)
  assert out.dtype == torch.float32 and pen.shape == (1,)
  assert float((out.detach().double() - c['out']).abs().max()) <= 1e-5 * float(c['out'].abs().max())
  assert abs(float(pen.detach()) - c['penalty']) <= 1e-5 * abs(c['penalty'])
  # __call__ draws its own noise in training and collects the penalty
  again = layer(x)
  assert len(ctx.vdrop_losses) == 1 and again.shape == out.shape
  assert torch.equal(again, out) != c['training']


def test_noise_is_uniform_and_shaped_like_the_probabilities(cpu_context):
  from easyrec_amd.layers.variational_dropout_layer import VariationalDropoutLayer
  cpu_context()
  cfg = variational_dropout_pb2.VariationalDropoutLayer(regularization_lambda=0.01, embedding_wise_variational_dropout=False)
  layer = VariationalDropoutLayer(cfg, OrderedDict([('a', 2), ('b', 3)]), True, name='all')
  torch.manual_seed(3)
  u = layer.sample_noise(4096, torch.device('cpu'))
  assert u.shape == (4096, 2) and u.dtype == torch.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
  assert abs(float(u.double().mean()) - 0.5) <= 6 * np.sqrt(1.0 / 12 / u.numel())
  assert VariationalDropoutLayer(cfg, OrderedDict([('a', 2)]), False, name='e').sample_noise(4, torch.device('cpu')) is None


# ------------------------------------------------------------------------------------------------ the models
def _make_configs():
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  return make_configs


def test_committed_configs_are_the_generated_ones():
  from easyrec_amd.utils import config_util
  mk = _make_configs()
  for name, ew in (('deepfm_vdrop_criteo.config', True), ('deepfm_vdrop_criteo_feature_num.config', False)):
    cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', name))
    assert cfg == mk.deepfm_vdrop_criteo(embedding_wise=ew)
    vd = cfg.model_config.variational_dropout
    assert abs(vd.regularization_lambda - 0.01) < 1e-9 and vd.embedding_wise_variational_dropout == ew
    cfg.model_config.ClearField('variational_dropout')
    assert cfg == mk.deepfm_criteo()  # (deepfm_criteo.config plus the one section)


def _shrunk(cfg):
  """as tools/count_reference_configs.py shrinks a config's tables"""
  for fc in list(cfg.feature_config.features) + list(cfg.feature_configs):
    if fc.hash_bucket_size > 2000:
      fc.hash_bucket_size = 2000
    if fc.num_buckets > 2000:
      fc.num_buckets = 2000
  return cfg


def _small(embedding_wise=True, **kw):
  return _make_configs().deepfm_vdrop_criteo(embedding_wise=embedding_wise, hash_bucket_size=1000, batch_size=16, **kw)


def _estimator(cfg, B=16, seed=4, **kw):
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  return EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=seed, **kw).build()


def _batch(cfg, est, B=16, seed=44):
  from easyrec_amd.input.synthetic import SyntheticBatches
  return SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=seed).next_batch()


@pytest.mark.parametrize('embedding_wise', [True, False], ids=['embedding_wise', 'feature_wise'])
def test_model_steps_and_the_penalty_is_a_loss_of_its_own(embedding_wise, ref_backend, built_lib):
  cfg = _small(embedding_wise)
  est = _estimator(cfg)
  st = est.state_dict()
  assert st['logit_p_deep'].shape == ((39 * 16,) if embedding_wise else (39,))
  assert st['logit_p_wide'].shape == ((39,) if embedding_wise else (39,))
  batch = _batch(cfg, est)
  before = {k: st[k].copy() for k in ('logit_p_deep', 'logit_p_wide')}
  est.train_step(batch)
  losses = est.loss_values()
  assert all(np.isfinite(v) for v in losses.values()), losses
  # the penalty: lambda / rows * sum(1 - p) over the two groups, from the variables the step started from
  want = sum(0.01 / 16 * float((1 - 1 / (1 + np.exp(-before[k].astype(np.float64)))).sum()) for k in before)
  assert abs(losses['variational_dropout_loss'] - want) <= 1e-5 * want
  # part of total_loss, not of regularization_loss
  parts = sum(v for k, v in losses.items() if k != 'total_loss')
  assert abs(losses['total_loss'] - parts) <= 1e-5 * abs(parts)
  plain = _make_configs().deepfm_criteo(hash_bucket_size=1000, batch_size=16)
  ref = _estimator(plain)
  ref.train_step(batch)
  # the embedding-output L2 is taken before the dropout: the same value as without it (same seed, same tables)
  assert abs(losses['regularization_loss'] - ref.loss_values()['regularization_loss']) <= \
      1e-6 * ref.loss_values()['regularization_loss']
  # the variables moved: the gradient reached them
  after = est.state_dict()
  assert all(float(np.abs(after[k] - before[k]).max()) > 0 for k in before)


def test_input_layer_keeps_the_dict_undropped_and_splits_the_dropped_tensor(ref_backend, built_lib):
  from easyrec_amd.core import context
  cfg = _small(False)
  est = _estimator(cfg)
  est.features.load(_batch(cfg, est))
  est.features.transform()
  layer = est.model._input_layer
  with context.use(est.ctx):
    est.model.begin_step()
    out, flist, names = layer(est.features, 'deep', is_dict=True)
    assert len(est.ctx.vdrop_losses) == 1
  raw = est.engine.groups['group:deep']['out']
  assert out.shape == raw.shape and float((out - raw).abs().max()) > 0
  assert flist.base is out and flist.dims == [16] * 39 and getattr(out, '_er_sink', None) is None
  assert torch.equal(torch.cat(list(flist), dim=1), out)
  assert torch.equal(torch.cat([names[n] for n in names], dim=1), raw) and len(names) == 39
  # feature-wise: one mask value per (row, feature)
  o3, r3 = out.detach().double().reshape(16, 39, 16), raw.double().reshape(16, 39, 16)
  assert float((o3 * r3[:, :, :1] - o3[:, :, :1] * r3).abs().max()) <= 1e-6 * float(r3.abs().max()) ** 2
  with pytest.raises(ValueError, match='variational dropout is not supported in not combined mode now.'):
    layer(est.features, 'deep', is_combine=False)


def test_a_training_estimator_evaluates_without_noise(ref_backend, built_lib):
  """evaluate() clears the context's is_training: the group output is x * (1 - p), the same on every call"""
  from easyrec_amd.core import context
  cfg = _small(False)
  est = _estimator(cfg)
  est.features.load(_batch(cfg, est))
  est.features.transform()
  layer = est.model._input_layer
  est.ctx.is_training = False
  with context.use(est.ctx), torch.no_grad():
    est.model.begin_step()
    first = layer(est.features, 'wide')[0].clone()
    second = layer(est.features, 'wide')[0]
  raw = est.engine.groups['group:wide']['out']
  p = torch.sigmoid(torch.from_numpy(est.state_dict()['logit_p_wide']))
  assert torch.equal(first, second)
  assert float((first - raw * (1 - p)).abs().max()) <= 1e-6 * float(raw.abs().max())
  est.ctx.is_training = True
  with context.use(est.ctx), torch.no_grad():
    assert not torch.equal(layer(est.features, 'wide')[0], first)


def test_a_group_that_combines_sequence_columns_is_refused(ref_backend, built_lib):
  """configs/deepfm_textcnn_movielens.config's shape (tests/test_seq_combiner_pins.model_cfg) under variational dropout:
  NotImplementedError at build time, naming variational dropout - dropout over sequence_combiner columns is not built"""
  from tests.test_seq_combiner_pins import model_cfg
  cfg = model_cfg('deepfm_textcnn')
  cfg.model_config.variational_dropout.regularization_lambda = 0.01
  with pytest.raises(NotImplementedError, match='variational dropout over combined sequence columns'):
    _estimator(cfg, B=8, seed=1)


def test_rejected_setups(ref_backend, built_lib):
  from easyrec_amd.layers.input_layer import InputLayer
  from easyrec_amd.layers.sharded_embedding import ShardedEmbeddingEngine
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  with pytest.raises(ValueError, match='variational dropout.*bf16'):
    EasyRecEstimator(_small(), device='cpu', batch_size=16, seed=4, dense_dtype='bf16').build()

  from easyrec_amd.core import context

  class Fake(object):
    _engine = ShardedEmbeddingEngine.__new__(ShardedEmbeddingEngine)
  with context.use(_Ctx(None)):
    with pytest.raises(ValueError, match='variational dropout.*embedding-parallel'):
      InputLayer._check_variational_dropout(Fake(), 'deep', [])
    Fake._engine = None
    with pytest.raises(ValueError, match='variational dropout.*negative sampler'):
      InputLayer._check_variational_dropout(Fake(), 'item', ['item_id'])
    InputLayer._check_variational_dropout(Fake(), 'deep', [])


def test_envelope_helper_is_the_library_s(built_lib):
  from easyrec_amd import kernels
  from easyrec_amd.layers import variational_dropout_layer as vdl
  be = kernels.HipBackend()
  for W in range(-1, 4098):
    assert (be.vdrop_grid(1, W) > 0) == vdl.vdrop_fits(W), W
    assert be.vdrop_grid(77, W) == vc.grid_of(77, W), W
  for B in (-3, 0, 1, 5, 8, 9, 4096, 8192, 8193, 100000):
    assert be.vdrop_grid(B, 16) == vc.grid_of(B, 16), B
  for B, dims in vc.KERNEL_CASES:
    assert be.vdrop_grid(B, sum(dims)) == vc.grid_of(B, sum(dims)) > 0
  # outside the envelope the launches are errors before anything else is looked at (nothing is launched: no device)
  for W in (0, 4097):
    assert be.lib.er_vdrop_fwd(None, W, None, None, W, None, None, 4, W, W, 0.0, None, W, None, None) == 2
    assert b'outside the envelope' in be.lib.er_last_error()
    assert be.lib.er_vdrop_bwd(None, W, None, W, None, None, W, None, None, 4, W, W, 0.0, None, None, W, None, None) == 2
    assert b'outside the envelope' in be.lib.er_last_error()


def test_feature_importance_sorts_as_the_reference_s_tool():
  """reference tools/feature_selection.py:116-151 on a hand-made logit_p"""
  from easyrec_amd.layers.variational_dropout_layer import feature_importance
  dims = OrderedDict([('a', 2), ('b', 1), ('c', 3)])
  sig = lambda v: 1 / (1 + np.exp(-np.asarray(v, dtype=np.float64)))
  got = feature_importance(np.array([2.0, -1.0, 0.5], dtype=np.float32), dims, False)
  assert list(got) == ['b', 'c', 'a'] and np.allclose(list(got.values()), sig([-1.0, 0.5, 2.0]))
  logit = np.array([3.0, -3.0, 1.0, -2.0, -2.0, -1.0], dtype=np.float32)
  got = feature_importance(logit, dims, True)
  want = {'a': sig(logit[:2]).mean(), 'b': sig(logit[2:3]).mean(), 'c': sig(logit[3:]).mean()}
  assert list(got) == sorted(want, key=want.get) == ['c', 'a', 'b']
  assert all(abs(got[k] - want[k]) <= 1e-12 for k in want)


def test_estimator_ranking_and_the_checkpoint_tool(ref_backend, built_lib, tmp_path, capsys):
  from easyrec_amd.tools import feature_selection
  from easyrec_amd.utils import checkpoint
  from google.protobuf import text_format
  cfg = _small(True)
  est = _estimator(cfg)
  est.train_step(_batch(cfg, est))
  ranking = est.feature_importance()
  assert list(ranking) == ['wide', 'deep'] and all(len(r) == 39 for r in ranking.values())
  for r in ranking.values():
    assert list(r.values()) == sorted(r.values())
  p = 1 / (1 + np.exp(-est.state_dict()['logit_p_deep'].astype(np.float64)))
  assert abs(ranking['deep']['C3'] - p[(13 + 2) * 16:(13 + 3) * 16].mean()) <= 1e-12
  path = str(tmp_path / 'model.ckpt-1')
  checkpoint.save(est, path)
  config_path = str(tmp_path / 'pipeline.config')
  with open(config_path, 'w') as f:
    f.write(text_format.MessageToString(cfg))
  got, excluded = feature_selection.main(['--config', config_path, '--checkpoint', path, '--topk', '30'])
  # the groups in the config's order; the same numbers, the same order
  assert {g: list(r.items()) for g, r in got.items()} == {g: list(r.items()) for g, r in ranking.items()}
  want = set(list(ranking['deep'])[30:]) | set(list(ranking['wide'])[30:])
  assert excluded == sorted(want) and 'excluded: ' in capsys.readouterr().out
  feature_selection.main(['--config', config_path, '--checkpoint', path, '--topk', '30', '--output_dir', str(tmp_path / 'o')])
  rows = open(str(tmp_path / 'o' / 'feature_dropout_ratio_deep.csv')).read().splitlines()
  assert rows[0] == 'feature_name,mean_drop_p' and [r.split(',')[0] for r in rows[1:]] == list(ranking['deep'])
  assert open(str(tmp_path / 'o' / 'excluded_features.txt')).read().split() == excluded


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='no checkout of the reference')
@pytest.mark.parametrize('name', SIX)
def test_reference_configs_build_and_step_on_the_stand_in(name, ref_backend, built_lib):
  """the six shipped configs that stopped at `variational dropout is outside the hot-path scope`"""
  from easyrec_amd.utils import config_util
  cfg = _shrunk(config_util.get_configs_from_pipeline_file(os.path.join(REFERENCE, 'samples', 'model_config', name + '.config')))
  assert cfg.model_config.HasField('variational_dropout')
  est = _estimator(cfg, B=8, seed=1)
  est.train_step(_batch(cfg, est, B=8, seed=2))
  losses = est.loss_values()
  assert all(np.isfinite(v) for v in losses.values()) and losses['variational_dropout_loss'] > 0
  assert any(k == 'logit_p' or k.startswith('logit_p_') for k in est.state_dict())
