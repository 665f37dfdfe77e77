"""FiBiNet on the CPU: the blocks resolve, their variables follow the reference's names and shapes
(layers/keras/fibinet.py, layers/common_layers.py), the restatement reproduces the reference's own outputs, unsupported
setups raise at build time, the Python envelope formulas are the library's, and the model trains on a stand-in backend
exactly as the oracle does."""
import os

import numpy as np
import pytest
import torch
from google.protobuf import text_format

from easyrec_amd.core.variables import VarStore
from easyrec_amd.protos import layer_pb2
from easyrec_amd.utils import load_class
from oracle.kernel_ref import RefBackend
from oracle import fibinet_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'fibinet_vectors.npz'))
GOLD_CASES = sorted({k.split(':')[0] for k in GOLD.files if k.endswith(':pb')})


def gold_case(tag):
  """(FiBiNet message, B, F, D, x [B, F * D], {name: variable}) of a fixture case, fp64."""
  pb = layer_pb2.FiBiNet()
  text_format.Merge(str(GOLD['%s:pb' % tag]), pb)
  B, F, D = [int(v) for v in GOLD['%s:cfg' % tag]]
  var = {k.split(':var:')[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith(tag + ':var:')}
  return pb, B, F, D, torch.from_numpy(GOLD['%s:x' % tag]), var


def test_blocks_are_registered():
  for name in ('FiBiNet', 'BiLinear', 'SENet'):
    cls, customize = load_class.load_keras_layer(name)
    assert cls is not None and customize, name


def test_fixture_covers_the_cases():
  cases = {t: gold_case(t) for t in GOLD_CASES}
  bl = lambda pb: (pb.bilinear.type, pb.bilinear.use_plus) if pb.HasField('bilinear') else None
  assert any(c[2:4] == (17, 16) and bl(c[0]) == ('each', True) for c in cases.values())
  assert {('all', True), ('each', False), ('all', False)} <= {bl(c[0]) for c in cases.values()}
  assert any(not c[0].HasField('bilinear') for c in cases.values())
  assert any(not c[0].HasField('mlp') for c in cases.values())
  assert any(c[0].senet.num_squeeze_group == 1 and not c[0].senet.use_skip_connection and
             not c[0].senet.use_output_layer_norm for c in cases.values())
  assert any(c[2] % 2 == 1 and c[3] % 4 != 0 for c in cases.values())
  assert list(GOLD['interaction:error']) == ['IndexError', 'list index out of range']


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_restatement_matches_the_reference(tag):
  pb, B, F, D, x, var = gold_case(tag)
  fields = ref.split(x, F, D)
  se = pb.senet
  got = {'senet': ref.senet(fields, int(se.num_squeeze_group), var, 'fibinet/senet', se.use_skip_connection,
                            se.use_output_layer_norm),
         'out': ref.fibinet(fields, pb, var)}
  if pb.HasField('bilinear'):
    got['bilinear'] = ref.bilinear(fields, pb.bilinear.type, pb.bilinear.use_plus, var, 'fibinet/bilinear')
  for k, v in got.items():
    want = GOLD['%s:%s' % (tag, k)]
    assert v.shape == want.shape and np.abs(v.numpy() - want).max() <= 1e-9 * np.abs(want).max(), (tag, k)


def test_restatement_matches_the_reference_input_batch_norm():
  dims = [int(d) for d in GOLD['input_bn:dims']]
  x = torch.from_numpy(GOLD['input_bn:x'])
  var = {k.split(':var:')[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith('input_bn:var:')}
  cols = np.cumsum([0] + dims)
  got = ref.input_batch_norm([x[:, cols[i]:cols[i + 1]] for i in range(len(dims))], var)
  for i, v in enumerate(got):
    want = GOLD['input_bn:out_%d' % i]
    assert np.abs(v.numpy() - want).max() <= 1e-9 * np.abs(want).max(), i


class _Ctx(object):
  """The piece of the build context the blocks read."""

  def __init__(self, vs, dense_dtype='f32'):
    self.varstore, self.dense_dtype = vs, dense_dtype
    self.is_training, self.building, self.engine = True, True, None


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


def _block(pb, l2=1e-6):
  from easyrec_amd.layers.keras import FiBiNet
  from easyrec_amd.layers.utils import Parameter
  return FiBiNet(Parameter(pb, False, l2_reg=l2), name='fibinet')


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_product_variables_and_outputs_are_the_reference_s(tag, cpu_context):
  """Names, shapes and L2 flags; and with the fixture's values loaded, the composed path's output."""
  pb, B, F, D, x, var = gold_case(tag)
  ctx = cpu_context()
  layer = _block(pb)
  fields = ref.split(x.float(), F, D)
  layer(fields, training=True)
  vs = ctx.varstore
  own = [n for n in vs.names() if '/moving_' not in n]
  assert sorted(own) == sorted(var)
  assert all(tuple(vs._vars[n]['tensor'].shape) == tuple(var[n].shape) for n in own)
  assert all(vs.l2_of(n) == (1e-6 if n.startswith('fibinet/mlp/') and n.endswith('/kernel') else 0.0) for n in own)
  vs.load_state_dict({n: v.numpy() for n, v in var.items()}, strict=False)
  got = layer(fields, training=True).detach().double().numpy()
  want = GOLD['%s:out' % tag]
  assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()


def test_input_layer_batch_norm_names_are_the_reference_s(cpu_context):
  from easyrec_amd.layers import backbone
  dims = [int(d) for d in GOLD['input_bn:dims']]
  x = torch.from_numpy(GOLD['input_bn:x']).float()
  var = {k.split(':var:')[1]: GOLD[k] for k in GOLD.files if k.startswith('input_bn:var:')}
  ctx = cpu_context()
  cols = np.cumsum([0] + dims)
  feats = [x[:, cols[i]:cols[i + 1]] for i in range(len(dims))]
  whole, flist = backbone._input_batch_norm(x, feats, True, True)
  vs = ctx.varstore
  assert whole is None and sorted(vs.names()) == sorted(var)
  assert all(tuple(vs._vars[n]['tensor'].shape) == var[n].shape for n in var)
  vs.load_state_dict(var)
  _, flist = backbone._input_batch_norm(x, feats, True, True)
  for i, f in enumerate(flist):
    want = GOLD['input_bn:out_%d' % i]
    assert np.abs(f.detach().double().numpy() - want).max() <= 1e-4 * np.abs(want).max(), i
  # the per-feature moving statistics are views of the whole-tensor ones
  ctx.building = False
  backbone._input_batch_norm(x, feats, True, True)
  st = vs.state_dict()
  assert np.abs(st['batch_normalization/moving_mean']).max() > 0
  for stat in ('moving_mean', 'moving_variance'):
    cat = np.concatenate([st['batch_normalization_%d/%s' % (k + 1, stat)] for k in range(len(dims))])
    assert np.array_equal(cat, st['batch_normalization/' + stat])
  # a second normalising block goes on counting; both outputs with the 2-D tensor
  whole, flist = backbone._input_batch_norm(x, feats, True, False, first=4)
  assert whole.shape == x.shape and len(flist) == 3 and 'batch_normalization_7/gamma' in vs.names()


def test_rejected_setups(cpu_context):
  from easyrec_amd.layers.keras import BiLinear
  from easyrec_amd.layers.utils import Parameter
  cpu_context()
  pb = layer_pb2.Bilinear()
  text_format.Merge("type: 'interaction' num_output_units: 4", pb)
  with pytest.raises(NotImplementedError, match='out of range'):
    BiLinear(Parameter.make_from_pb(pb), name='b')
  text_format.Merge("type: 'each'", pb)
  layer = BiLinear(Parameter.make_from_pb(pb), name='b')
  with pytest.raises(ValueError, match='embedding dimensions must be same'):
    layer([torch.zeros(2, 4), torch.zeros(2, 8)])
  with pytest.raises(TypeError):
    layer(torch.zeros(2, 8))
  cpu_context('bf16')
  with pytest.raises(ValueError, match='bf16'):
    BiLinear(Parameter.make_from_pb(pb), name='b')
  with pytest.raises(ValueError, match='bf16'):
    _block(gold_case('sample')[0])


@pytest.mark.parametrize('option', ['do_layer_norm: true', 'dropout_rate: 0.5', 'feature_dropout_rate: 0.5',
                                    'only_output_3d_tensor: true'])
def test_other_input_layer_options_still_raise(option):
  from easyrec_amd.layers.backbone import Package
  from easyrec_amd.protos import backbone_pb2
  cfg = backbone_pb2.InputLayer()
  text_format.Merge(option, cfg)
  pkg = object.__new__(Package)
  pkg._features, pkg._input_layer = None, lambda features, group: (torch.zeros(2, 4), [torch.zeros(2, 4)])
  with pytest.raises(AssertionError, match='outside the hot-path scope'):
    pkg._input_layer_output('all', cfg)


def test_envelope():
  from easyrec_amd.layers.keras import fibinet as fb
  assert fb.bilinear_fits(17, 16) and fb.senet_fits(17, 16, 2, 17)
  assert fb.bilinear_lds_bytes(17, 16) == 4 * (16 * (16 * 17 + 16) + 136 + 272 + 512)
  assert fb.senet_lds_bytes(17, 16, 2, 17) == 4 * (6613 + 4 * 272 + 136 + 34 + 2)
  assert not fb.bilinear_fits(40, 32) and not fb.senet_fits(40, 32, 2, 40)
  assert not fb.bilinear_fits(65, 2) and not fb.bilinear_fits(1, 8) and not fb.senet_fits(4, 6, 4, 2)


def test_envelope_formula_is_the_library_s(built_lib):
  from easyrec_amd import kernels
  from easyrec_amd.layers.keras import fibinet as fb
  be = kernels.HipBackend()
  for F, D in [(17, 16), (7, 5), (2, 8), (40, 32), (64, 8), (65, 2), (30, 64), (1, 8)]:
    assert be.bilinear_lds_bytes(F, D) == fb.bilinear_lds_bytes(F, D), (F, D)
    for each in (True, False):
      assert (be.bilinear_epb(F, D, each) > 0) == fb.bilinear_fits(F, D), (F, D)
  assert be.bilinear_epb(17, 16, True) == 8
  for F, D, G, R in [(17, 16, 2, 17), (7, 6, 2, 7), (5, 3, 3, 15), (40, 32, 2, 40), (64, 64, 1, 2), (4, 6, 4, 2),
                     (17, 16, 2, 69)]:
    assert be.senet_lds_bytes(F, D, G, R) == fb.senet_lds_bytes(F, D, G, R), (F, D, G, R)
    for ln in (True, False):
      assert (be.senet_epb(F, D, G, R, ln, True) > 0) == fb.senet_fits(F, D, G, R), (F, D, G, R)
  assert be.senet_epb(17, 16, 2, 17, True, True) == 7 and be.senet_epb(17, 16, 2, 17, True, False) == 8


# ---------------------------------------------------------------------------------------- configs and the model
def fibinet_cfg(bilinear_type='each', use_plus=True, batch_size=16):
  """A small FiBiNet config (the sample's model section on the scaled-down taobao tables); bilinear_type None: no
  bilinear."""
  import sys
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  cfg = make_configs.fibinet_taobao(bilinear_type=bilinear_type or 'each', use_plus=use_plus, batch_size=batch_size,
                                    scale=0.01)
  if bilinear_type is None:
    cfg.model_config.backbone.blocks[1].keras_layer.fibinet.ClearField('bilinear')
  return cfg


def test_committed_config_is_the_generated_sample_model():
  import sys
  from easyrec_amd.utils import config_util
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'fibinet_taobao_10m.config'))
  assert cfg == make_configs.fibinet_taobao(item_rows=10000000)
  mc = cfg.model_config
  fbn = mc.backbone.blocks[1].keras_layer.fibinet
  assert mc.model_class == 'RankModel' and len(mc.feature_groups[0].feature_names) == 17
  assert mc.backbone.blocks[0].input_layer.do_batch_norm and mc.backbone.blocks[0].input_layer.only_output_feature_list
  assert (fbn.bilinear.type, fbn.bilinear.num_output_units, fbn.senet.reduction_ratio) == ('each', 512, 4)
  assert list(fbn.mlp.hidden_units) == [512, 256] and cfg.data_config.batch_size == 4096
  assert {f.embedding_dim for f in cfg.feature_config.features} == {16}


@pytest.mark.parametrize('kind,plus', [('each', True), ('all', False), (None, True)])
def test_model_builds_and_steps_on_the_stand_in(ref_backend, built_lib, kind, plus):
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  from oracle.model_oracle import OracleTrainer
  B = 16
  cfg = fibinet_cfg(bilinear_type=kind, use_plus=plus, batch_size=B)
  est = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4).build()
  st = est.state_dict()
  assert 'fibinet/senet/W2/kernel' in st and 'batch_normalization_17/gamma' in st and st['output/kernel'].shape == (256, 1)
  assert ('fibinet/bilinear/each_15/kernel' in st) == (kind == 'each')
  orc = OracleTrainer(cfg, st, batch_size=B)
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=44)
  for _ in range(2):
    b = gen.next_batch()
    est.train_step(b)
    got, exp = est.loss_values(), orc.train_step(b)
    for k in exp:
      assert abs(got[k] - exp[k]) <= 1e-4 * max(1e-3, abs(exp[k])), (k, got[k], exp[k])
