"""MaskNet on the CPU: the layers resolve, their variables follow the reference's names and shapes
(layers/keras/mask_net.py, layers/keras/blocks.py Gate), the composed path and the fp64 restatement reproduce the
reference's own outputs (tests/golden/masknet_vectors.npz), L2 lands where the reference puts it, unsupported setups
raise, the Python envelope helpers are the library's, and the models build and step on a stand-in backend."""
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
from tests import _masknet_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = '/root/reference'
L2 = 1e-6


def test_layers_are_registered():
  for name in ('MaskNet', 'MaskBlock', 'Gate'):
    cls, customize = load_class.load_keras_layer(name)
    assert cls is not None and customize, name


def test_fixture_covers_the_cases():
  cases = {t: mc.gold_case(t) for t in mc.GOLD_CASES}
  nets = [c[1] for c in cases.values() if c[0] == 'masknet']
  blocks = [c for c in cases.values() if c[0] == 'mask_block']
  gates = [c[1] for c in cases.values() if c[0] == 'gate']
  assert all(c[2][0].shape[0] == 6 and max(x.shape[1] for x in c[2]) <= 12 for c in cases.values())
  assert any(p.use_parallel and p.input_layer_norm and len(p.mask_blocks) == 3 for p in nets)
  assert any(p.use_parallel and not p.input_layer_norm for p in nets)
  assert any(not p.use_parallel and len(p.mask_blocks) == 2 for p in nets)
  assert any(b.HasField('reduction_factor') for p in nets for b in p.mask_blocks)
  assert any(b.HasField('projection_dim') for p in nets for b in p.mask_blocks)
  assert any(b.input_layer_norm for p in nets for b in p.mask_blocks)
  assert any(not b.HasField('output_size') for p in nets for b in p.mask_blocks)
  assert any(len({b.output_size for b in p.mask_blocks}) > 1 and p.use_parallel for p in nets)
  assert any(not p.HasField('mlp') for p in nets)
  assert any(len(c[2]) == 1 for c in blocks) and any(len(c[2]) == 2 for c in blocks)
  assert {0, 1} <= {int(p.weight_index) for p in gates}


@pytest.mark.parametrize('tag', mc.GOLD_CASES)
def test_restatement_matches_the_reference(tag):
  kind, pb, xs, var, want = mc.gold_case(tag)
  got = mc.restate(kind, pb, xs, var)
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


def _layer(kind, pb, l2=L2):
  from easyrec_amd.layers import keras as layers
  from easyrec_amd.layers.utils import Parameter
  cls = {'masknet': layers.MaskNet, 'mask_block': layers.MaskBlock, 'gate': layers.Gate}[kind]
  return cls(Parameter(pb, False, l2_reg=l2), name=mc.NAMES[kind])


def _carries_l2(name):
  """aggregation, project and the MLP kernels only (reference mask_net.py:52-65, :123; blocks.py:188)"""
  return name.endswith('/kernel') and ('/aggregation/' in name or '/project/' in name or '/mlp/' in name or
                                      '/top_mlp/' in name)


@pytest.mark.parametrize('tag', mc.GOLD_CASES)
def test_product_variables_and_outputs_are_the_reference_s(tag, cpu_context):
  """Names, shapes and L2 flags; and from the fixture's variables the composed path's output: 1e-6 of the largest
  element with the variables as the fixture holds them (fp64; the composition is dtype-agnostic torch), and 1e-4, the
  bar of the other families' pins, with everything rounded to the product's fp32 (measured there: at most 1.1e-6, the
  serial case - two blocks and two batch-normalised layers over 6 rows)."""
  kind, pb, xs, var, want = mc.gold_case(tag)
  ctx = cpu_context()
  layer = _layer(kind, pb)
  one = lambda ts: ts[0] if len(ts) == 1 else ts
  layer(one([x.float() for x in xs]), training=True)
  vs = ctx.varstore
  assert sorted(vs.names()) == sorted(var)
  assert all(tuple(vs._vars[n]['tensor'].shape) == tuple(var[n].shape) for n in var)
  assert all(vs.l2_of(n) == (L2 if _carries_l2(n) else 0.0) for n in var), [(n, vs.l2_of(n)) for n in var]
  vs.load_state_dict({n: v.numpy() for n, v in var.items()}, strict=False)
  got = layer(one([x.float() for x in xs]), training=True).detach().double()
  assert got.shape == want.shape
  assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()), tag
  for n, v in var.items():
    vs._vars[n]['tensor'] = v.clone()
  got = layer(one(xs), training=True)
  assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-6 * float(want.abs().max()), tag


def test_rejected_setups(cpu_context):
  from easyrec_amd.layers.keras import Gate, MaskBlock, MaskNet
  from easyrec_amd.layers.utils import Parameter
  cpu_context()
  pb = layer_pb2.MaskBlock()
  text_format.Merge('output_size: 4', pb)
  with pytest.raises(ValueError, match='reduction factor or aggregation size'):
    MaskBlock(Parameter.make_from_pb(pb), name='b')
  text_format.Merge('aggregation_size: 0', pb)
  with pytest.raises(ValueError, match='reduction factor or aggregation size'):
    MaskBlock(Parameter.make_from_pb(pb), name='b')
  pb = layer_pb2.MaskBlock()
  text_format.Merge('reduction_factor: 0.01 output_size: 4', pb)  # (int(8 * 0.01) == 0)
  with pytest.raises(ValueError, match='aggregation size 0'):
    MaskBlock(Parameter.make_from_pb(pb), name='b')(torch.zeros(2, 8))
  gate = Gate(Parameter.make_from_pb(mc.gate_message()), name='g')
  with pytest.raises(AssertionError, match='at least 2'):
    gate([torch.zeros(2, 3)])
  cpu_context('bf16')
  text_format.Merge('aggregation_size: 4', pb)
  with pytest.raises(ValueError, match='bf16'):
    MaskBlock(Parameter.make_from_pb(pb), name='b')
  with pytest.raises(ValueError, match='bf16'):
    MaskNet(Parameter.make_from_pb(mc.gold_case('parallel_ln')[1]), name='m')


def test_envelope_helpers_are_the_library_s(built_lib):
  from easyrec_amd import kernels
  from easyrec_amd.layers.keras import mask_net as mn
  be = kernels.HipBackend()
  widths, counts = (0, 1, 5, 272, 1024, 1028, 4095, 4096, 4097), (0, 1, 2, 3, 7, 8, 9)
  for O in widths:
    for n in counts:
      for B in (1, 5, 4096, 100000):
        assert (be.ln_relu_grid(B, O, n) > 0) == mn.ln_relu_fits(O, n), (B, O, n)
      assert be.ln_relu_grid(0, O, n) == 0
  assert be.ln_relu_grid(4096, 256, 3) == 1024 and be.ln_relu_grid(301, 256, 3) == 76 and be.ln_relu_grid(3, 7, 1) == 1
  assert mn.ln_relu_fits(4096, 7) and not mn.ln_relu_fits(4096, 8) and mn.ln_relu_fits(4095, 8)
  # the mask multiply has no grid function: its envelope is what the launch checks before anything else (a null x makes
  # every call an error, so nothing is launched; the text tells which check refused)
  for W in widths:
    for n in counts:
      rc = be.lib.er_mask_mul_fwd(None, W, None, None, n, 4, W, None, None, None)
      assert rc != 0
      outside = b'outside the envelope' in be.lib.er_last_error()
      assert outside == (not mn.mask_mul_fits(W, n)), (W, n)


# ---------------------------------------------------------------------------------------- configs and the models
def _make_configs():
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  return make_configs


def masknet_cfg(batch_size=16, **kw):
  """The sample's model section on the scaled-down taobao tables."""
  return _make_configs().masknet_taobao(batch_size=batch_size, scale=0.01, **kw)


def test_committed_config_is_the_generated_sample_model():
  from easyrec_amd.utils import config_util
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'masknet_taobao_10m.config'))
  assert cfg == _make_configs().masknet_taobao(item_rows=10000000)
  m = cfg.model_config
  net = m.backbone.blocks[0].keras_layer.masknet
  assert m.model_class == 'RankModel' and len(m.feature_groups[0].feature_names) == 17
  assert net.use_parallel and net.input_layer_norm and len(net.mask_blocks) == 3
  assert all((b.aggregation_size, b.output_size) == (512, 256) for b in net.mask_blocks)
  assert list(net.mlp.hidden_units) == [512, 256] and cfg.data_config.batch_size == 4096
  assert {f.embedding_dim for f in cfg.feature_config.features} == {16}


def _step(cfg, B, seed=4):
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  est = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=seed).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=seed + 40)
  est.train_step(gen.next_batch())
  losses = est.loss_values()
  assert all(np.isfinite(v) for v in losses.values()), losses
  return est


def test_model_builds_and_steps_on_the_stand_in(ref_backend, built_lib):
  est = _step(masknet_cfg(batch_size=16), 16)
  st = est.state_dict()
  assert st['mask_net/block_2/weights/kernel'].shape == (512, 272) and st['mask_net/input_ln/gamma'].shape == (272,)
  assert st['mask_net/block_0/output_ln/beta'].shape == (256,) and st['mask_net/mlp/layer_1/dense/kernel'].shape == (512, 256)


def _reference_config(name):
  """loaded and shrunk as tools/count_reference_configs.py does"""
  from easyrec_amd.utils import config_util
  path = [p for d in ('samples/model_config', 'examples/configs')
          for p in [os.path.join(REFERENCE, d, name + '.config')] if os.path.exists(p)][0]
  cfg = config_util.get_configs_from_pipeline_file(path)
  for fc in list(cfg.feature_config.features) + list(cfg.feature_configs):
    if fc.hash_bucket_size > 2000:
      fc.hash_bucket_size = 2000
    if fc.num_buckets > 2000:
      fc.num_buckets = 2000
  return cfg


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='no checkout of the reference')
@pytest.mark.parametrize('name', ['masknet_on_taobao', 'masknet_on_movielens', 'dbmtl_backbone_on_taobao'])
def test_reference_configs_build_and_step_on_the_stand_in(ref_backend, built_lib, name):
  _step(_reference_config(name), 16, seed=1)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='no checkout of the reference')
def test_cdn_config_gets_past_mask_block_and_gate(ref_backend, built_lib):
  """cdn_on_taobao names MaskBlock (under `repeat`) and Gate; both resolve and build.  What still stops the config is its
  gate_weight MLP's `final_activation: "softmax"`, which is neither: with that one activation made
  linear the model builds and steps, and the repeated blocks carry the reference's names."""
  cfg = _reference_config('cdn_on_taobao')
  with pytest.raises(ValueError, match='unsupported activation: softmax'):
    _step(cfg, 16, seed=1)
  gate_weight = [b for b in cfg.model_config.backbone.blocks if b.name == 'gate_weight'][0]
  assert gate_weight.keras_layer.mlp.final_activation == 'softmax'
  gate_weight.keras_layer.mlp.final_activation = 'linear'
  st = _step(cfg, 16, seed=1).state_dict()
  assert st['gen_experts_2/weights/kernel'].shape[0] == 1024 and st['gen_experts_0/output_ln/gamma'].shape == (256,)


def test_ln_relu_fn_leaves_no_reference_cycle(monkeypatch):
  """The Function keeps its own output for the backward's ReLU pattern.  Kept as the returned tensor itself, the output
  would own the node and the node the output: the graph - and the AccumulateGrad nodes of the leaves behind it - would
  stay alive until a garbage collection, into the next step's stream capture.  The node dies with its output."""
  import gc
  import weakref
  from easyrec_amd import kernels

  class _Torch(object):  # (the two calls of the backend the Function makes, in torch)

    def ln_relu_fwd(self, hs, gammas, betas, eps, y=None):
      pre = mc.ln_relu_pre(hs, gammas, betas, eps)
      stats = torch.zeros(len(hs), hs[0].shape[0])
      if y is None:
        return torch.relu(pre), stats, stats
      y.copy_(torch.relu(pre))
      return y, stats, stats

    def ln_relu_bwd(self, dy, y, hs, gammas, mean, rstd, grads, acc):
      return [torch.zeros_like(h) for h in hs]

  monkeypatch.setattr(kernels, '_BACKEND', _Torch())
  monkeypatch.setattr(kernels, 'ThetaGradTable', lambda grads: grads)
  gc.disable()
  try:
    for wide in (False, True):
      h = torch.randn(5, 8, requires_grad=True)
      out = torch.zeros(5, 12) if wide else None
      y = kernels.LnReluFn.apply(1e-3, None, out, 4, h, torch.ones(8, requires_grad=True), torch.zeros(8, requires_grad=True))
      y.sum().backward()
      node = weakref.ref(y.grad_fn)
      del y, out
      assert node() is None, wide
  finally:
    gc.enable()
