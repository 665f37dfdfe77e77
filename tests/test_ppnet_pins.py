"""PPNet on the CPU: the layer resolves, its variables follow the reference's names and shapes (layers/keras/ppnet.py;
the two names the reference leaves to keras' numbering are this project's), the composed path and the fp64 restatement
reproduce the reference's own outputs (tests/golden/ppnet_vectors.npz), L2 lands on the MLP kernels only, no gradient
reaches x through the gates' input, dropout acts while training only, unsupported setups raise, the Python envelope
helper is the library's, the seeded layer cases of the GPU tests keep their ReLUs away from zero, and the models build
and step on a stand-in backend."""
import os
import sys

import numpy as np
import pytest
import torch
from google.protobuf import text_format

from easyrec_amd.core.variables import VarStore
from easyrec_amd.protos import layer_pb2
from easyrec_amd.utils import load_class
from oracle.kernel_ref import RefBackend
from tests import _ppnet_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = '/root/reference'
L2 = 1e-6


def test_layer_is_registered():
  cls, customize = load_class.load_keras_layer('PPNet')
  assert cls is not None and customize
  from easyrec_amd.layers.keras import ppnet
  assert cls is ppnet.PPNet


def test_fixture_covers_the_cases():
  cases = {t: pc.gold_case(t) for t in pc.GOLD_CASES}
  pbs = [c[0] for c in cases.values()]
  assert all(c[1][0].shape[0] == 6 and max(x.shape[1] for x in c[1]) <= 12 for c in cases.values())
  gp = lambda p: p.gate_params
  assert any(p.mode == 'lazy' and p.full_gate_input and not p.HasField('gate_params') for p in pbs)
  assert any(not p.HasField('mode') and p.mode == 'eager' and gp(p).output_dim == 7 for p in pbs)
  assert any(not p.full_gate_input for p in pbs)
  assert any(gp(p).use_bn for p in pbs)
  assert any(gp(p).HasField('hidden_dim') and gp(p).hidden_dim not in list(p.mlp.hidden_units) for p in pbs)
  assert any(gp(p).activation not in ('relu', '') for p in pbs)
  assert any(p.mlp.use_bias and p.mlp.use_final_bias for p in pbs)
  assert any(not p.mlp.use_bn for p in pbs)
  assert any(len(p.mlp.hidden_units) == 1 for p in pbs)
  assert all(len(p.mlp.dropout_ratio) == 0 and gp(p).dropout_rate == 0 for p in pbs)
  # the variables the fixture holds are the ones the message implies (tests/_ppnet_cases.variable_shapes)
  for tag, (pb, xs, var, _) in cases.items():
    assert {n: tuple(v.shape) for n, v in var.items()} == pc.variable_shapes(pb, xs[0].shape[1], xs[1].shape[1]), tag


@pytest.mark.parametrize('tag', pc.GOLD_CASES)
def test_restatement_matches_the_reference(tag):
  pb, xs, var, want = pc.gold_case(tag)
  got = pc.ppnet(pb, var, pc.NAME, xs[0], xs[1])
  assert got.shape == want.shape
  assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), tag


class _Ctx(object):
  """The piece of the build context the layers read."""

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


def _layer(pb, l2=L2):
  from easyrec_amd.layers.keras import PPNet
  from easyrec_amd.layers.utils import Parameter
  return PPNet(Parameter(pb, False, l2_reg=l2), name=pc.NAME)


def _message(text):
  pb = layer_pb2.PPNet()
  text_format.Merge(text, pb)
  return pb


@pytest.mark.parametrize('tag', pc.GOLD_CASES)
def test_product_variables_and_outputs_are_the_reference_s(tag, cpu_context):
  """Names, shapes and L2 flags (the MLP's kernels only: the reference puts no regulariser on a gate's Dense layers);
  and from the fixture's variables the composed path's output at the project's 1e-5 of the largest element, with
  everything rounded to the product's fp32 and with the variables as the fixture holds them."""
  pb, xs, var, want = pc.gold_case(tag)
  ctx = cpu_context()
  layer = _layer(pb)
  layer([x.float() for x in xs], training=True)
  vs = ctx.varstore
  assert sorted(vs.names()) == sorted(var)
  assert all(tuple(vs._vars[n]['tensor'].shape) == tuple(var[n].shape) for n in var)
  carries = lambda n: n.endswith('/dense/kernel') and '/layer_' in n
  assert all(vs.l2_of(n) == (L2 if carries(n) else 0.0) for n in var), [(n, vs.l2_of(n)) for n in var]
  vs.load_state_dict({n: v.numpy() for n, v in var.items()}, strict=False)
  got = layer([x.float() for x in xs], training=True).detach().double()
  assert got.shape == want.shape
  assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), tag
  for n, v in var.items():
    vs._vars[n]['tensor'] = v.clone()
  got = layer(xs, training=True)
  assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), tag


@pytest.mark.parametrize('tag', ['lazy', 'eager'])
def test_no_gradient_reaches_x_through_the_gates_input(tag, cpu_context):
  """stop_gradient(x) in gate_input: a loss taken through a gate only leaves x without a gradient, while the rest of
  gate_input gets one; the restatement (whose full gradient the GPU tests compare) agrees."""
  pb, xs, var, _ = pc.gold_case(tag)
  ctx = cpu_context()
  layer = _layer(pb)
  layer([x.float() for x in xs], training=True)
  for n, v in var.items():
    ctx.varstore._vars[n]['tensor'] = v.clone()
  x, u = xs[0].clone().requires_grad_(True), xs[1].clone().requires_grad_(True)
  gi = layer.gate_input(x, u)
  assert gi.shape[1] == x.shape[1] + u.shape[1] and torch.equal(gi[:, :x.shape[1]], x.detach())
  for i, gate in sorted(layer.gates.items()):
    gate.scale(torch.ones(x.shape[0], gate.output_dim, dtype=torch.float64), gi, training=True).sum().backward()
  assert x.grad is None and float(u.grad.abs().max()) > 0
  # the restatement: through each gate alone, x gets what the MLP path hands it and nothing via gate_input
  for i in sorted(layer.gates):
    xr, ur = xs[0].clone().requires_grad_(True), xs[1].clone().requires_grad_(True)
    const = torch.ones(x.shape[0], layer.gates[i].output_dim, dtype=torch.float64)
    gate_in = torch.cat([xr.detach(), ur], dim=-1)
    (const * pc.gate_nn(pb.gate_params, var, '%s/gate_%d' % (pc.NAME, i), gate_in)).sum().backward()
    assert xr.grad is None and float(ur.grad.abs().max()) > 0


def test_dropout_changes_training_and_leaves_evaluation_alone(cpu_context):
  pb, xs, var, _ = pc.gold_case('lazy')
  ctx = cpu_context()
  plain = _layer(pb)
  dropped = _layer(_message('mlp { hidden_units: [8, 5] dropout_ratio: [0.5, 0.5] } mode: "lazy" '
                            'gate_params { dropout_rate: 0.5 }'))
  xs = [x.float() for x in xs]
  plain(xs, training=True)  # (one store: the two layers share the variables under one name)
  ctx.varstore.load_state_dict({n: v.numpy() for n, v in var.items()}, strict=False)
  torch.manual_seed(5)
  assert not torch.equal(dropped(xs, training=True), plain(xs, training=True))
  torch.manual_seed(5)
  gate_only = _layer(_message('mlp { hidden_units: [8, 5] } mode: "lazy" gate_params { dropout_rate: 0.5 }'))
  assert not torch.equal(gate_only(xs, training=True), plain(xs, training=True))
  ctx.is_training = False
  with torch.no_grad():
    assert torch.equal(dropped(xs, training=False), plain(xs, training=False))


def test_rejected_setups(cpu_context):
  cpu_context()
  with pytest.raises(ValueError, match='invalid dropout_ratio'):
    _layer(_message('mlp { hidden_units: [8, 5] dropout_ratio: [0.0, 1.0] } mode: "lazy"'))
  with pytest.raises(ValueError, match='invalid dropout_ratio'):
    _layer(_message('mlp { hidden_units: [8, 5] } mode: "lazy" gate_params { dropout_rate: 1.5 }'))
  x, u = torch.zeros(3, 7), torch.zeros(3, 4)
  for text in ('mlp { hidden_units: [8, 5] }', 'mlp { hidden_units: [8, 5] } mode: "eager" gate_params { output_dim: 8 }'):
    with pytest.raises(ValueError, match='gate_params.output_dim = 7'):
      _layer(_message(text))([x, u], training=True)
  _layer(_message('mlp { hidden_units: [8, 5] } gate_params { output_dim: 7 }'))([x, u], training=True)
  cpu_context('bf16')
  with pytest.raises(ValueError, match='bf16'):
    _layer(pc.gold_case('lazy')[0])


def test_envelope_helper_is_the_library_s(built_lib):
  from easyrec_amd import kernels
  from easyrec_amd.layers.keras import ppnet
  be = kernels.HipBackend()
  for W in (-1, 0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 272, 512, 1023, 1024, 1027, 4095, 4096, 4097, 8192, 65536):
    for B in (1, 5, 8, 9, 4096, 100000):
      assert (be.gate_scale_grid(B, W) > 0) == ppnet.gate_scale_fits(W), (B, W)
    assert be.gate_scale_grid(0, W) == 0 and be.gate_scale_grid(-3, W) == 0
  grid = lambda B: min(-(-B // pc.ROWS_PER_WG), pc.GRID_CAP)
  for B, W in pc.KERNEL_CASES:
    assert be.gate_scale_grid(B, W) == grid(B), (B, W)
  assert be.gate_scale_grid(4096, 512) == 512 and be.gate_scale_grid(301, 256) == 38 and be.gate_scale_grid(1, 16) == 1
  big = [c for c in pc.KERNEL_CASES if c[0] > pc.ROWS_PER_WG * pc.GRID_CAP]
  assert big and all(be.gate_scale_grid(*c) == pc.GRID_CAP for c in big)
  # outside the envelope the launches are errors before anything else is looked at (nothing is launched: no device)
  for W in (0, 4097):
    assert be.lib.er_gate_scale_fwd(None, W, None, W, None, 4, W, None, W, None) != 0
    assert b'outside the envelope' in be.lib.er_last_error()
    assert be.lib.er_gate_scale_bwd(None, W, None, W, None, W, None, 4, W, None, W, None, W, None, None) != 0
    assert b'outside the envelope' in be.lib.er_last_error()


LAYER_CASES = [(t, 6) for t in pc.GOLD_CASES] + [('sample', 64), ('sample', 1024)]


@pytest.mark.parametrize('tag,B', LAYER_CASES)
def test_layer_cases_keep_their_relus_away_from_zero(tag, B):
  """What licenses the GPU tests to compare every element: in the fp64 restatement no ReLU pre-activation lies within
  1e-5 (of the largest one's magnitude) of zero."""
  pb, x, u, var = pc.layer_case(tag, B)
  assert {n: tuple(v.shape) for n, v in var.items()} == pc.variable_shapes(pb, x.shape[1], u.shape[1])
  assert all(torch.equal(t, t.float().double()) for t in [x, u] + list(var.values()))
  pres = []
  y = pc.ppnet(pb, var, pc.NAME, x, u, pres)
  assert bool(torch.isfinite(y).all()) and len(pres) >= 2
  assert pc.relu_margin(pres) > pc.RELU_MARGIN, (tag, B, pc.relu_margin(pres))


# ---------------------------------------------------------------------------------------- configs and the models
def _make_configs():
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  return make_configs


def ppnet_cfg(batch_size=16, **kw):
  """The sample's model section on the scaled-down taobao tables."""
  return _make_configs().ppnet_taobao(batch_size=batch_size, scale=0.01, **kw)


def test_committed_config_is_the_generated_sample_model():
  from easyrec_amd.utils import config_util
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'ppnet_taobao_10m.config'))
  assert cfg == _make_configs().ppnet_taobao(item_rows=10000000)
  m = cfg.model_config
  block = m.backbone.blocks[0]
  net = block.keras_layer.ppnet
  assert m.model_class == 'RankModel' and [g.group_name for g in m.feature_groups] == ['memorize', 'general']
  assert [len(g.feature_names) for g in m.feature_groups] == [3, 14]
  assert [i.feature_group_name for i in block.inputs] == ['general', 'memorize'] and block.merge_inputs_into_list
  assert list(net.mlp.hidden_units) == [512, 256] and net.mode == 'lazy' and net.full_gate_input
  assert list(m.backbone.top_mlp.hidden_units) == [128, 64] and cfg.data_config.batch_size == 4096
  assert abs(m.embedding_regularization - 1e-5) < 1e-12 and abs(m.model_params.l2_regularization - 1e-6) < 1e-12
  assert {f.embedding_dim for f in cfg.feature_config.features} == {16}


def _shrunk(cfg):
  """as tools/count_reference_configs.py shrinks a config's tables"""
  for fc in list(cfg.feature_config.features) + list(cfg.feature_configs):
    if fc.hash_bucket_size > 2000:
      fc.hash_bucket_size = 2000
    if fc.num_buckets > 2000:
      fc.num_buckets = 2000
  return cfg


def _two_steps(cfg, B, seed=4):
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  est = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=seed).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=seed + 40)
  batch = gen.next_batch()
  seen = []
  for _ in range(2):  # (the same batch twice: the second loss is the first one after one update)
    est.train_step(batch)
    losses = est.loss_values()
    assert all(np.isfinite(v) for v in losses.values()), losses
    seen.append(losses)
  # decreasing, or at least of the same order: one Adam step on one small batch may overshoot, never by a decade
  assert all(seen[1][k] <= 10.0 * max(seen[0][k], 1e-3) for k in seen[0]), seen
  return est


def _check_state(est):
  st = est.state_dict()
  assert st['ppnet/layer_0/dense/kernel'].shape == (224, 512) and st['ppnet/layer_1/bn/gamma'].shape == (256,)
  assert st['ppnet/gate_1/dense/kernel'].shape == (272, 512) and st['ppnet/gate_1/weight/bias'].shape == (512,)
  assert st['ppnet/gate_2/weight/kernel'].shape == (256, 256) and 'ppnet/gate_0/weight/kernel' not in st
  assert st['backbone_top_mlp/layer_0/dense/kernel'].shape == (256, 128)


def test_committed_config_builds_and_steps_on_the_stand_in(ref_backend, built_lib):
  from easyrec_amd.utils import config_util
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'ppnet_taobao_10m.config'))
  _check_state(_two_steps(_shrunk(cfg), 16))


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='no checkout of the reference')
def test_reference_config_builds_and_steps_on_the_stand_in(ref_backend, built_lib):
  from easyrec_amd.utils import config_util
  path = os.path.join(REFERENCE, 'samples', 'model_config', 'ppnet_on_taobao.config')
  _check_state(_two_steps(_shrunk(config_util.get_configs_from_pipeline_file(path)), 16, seed=1))
