"""What the Uniter and CMBF tests share beside the restatement (oracle/uniter_ref.py): the PRODUCT's layers outside an
estimator, the test configs, and the cases of the reference's own run (tests/golden/uniter_vectors.npz)."""
import torch


def product_store(device, forward, params=None, training=True, seed=1):
  """A VarStore + ModelContext for running the PRODUCT's layer functions outside an estimator: forward() (called inside
  the context, without gradients) creates the variables, `params` (name -> fp64 tensor / array) overwrites them, then
  the store is packed (every variable's .grad is its slice of the flat gradient buffer).  -> (varstore, context)."""
  from easyrec_amd.core import context
  from easyrec_amd.core.variables import VarStore
  vs = VarStore(device, seed=seed)
  ctx = context.ModelContext(vs, None, is_training=training)
  with context.use(ctx), torch.no_grad():
    forward()
  if params is not None:
    assert sorted(params) == sorted(vs.names()), (sorted(set(params) ^ set(vs.names())))
    vs.load_state_dict({k: torch.as_tensor(v).detach().cpu().numpy() for k, v in params.items()})
  vs.pack()
  ctx.building = False
  return vs, ctx


def product_encoder(x, mask, H, layers, intermediate, act='gelu', name='uniter'):
  """The PRODUCT's transformer_encoder (inside a ModelContext) on x [B, S, hidden] with the to-mask [B, S] or None."""
  from easyrec_amd.layers import multihead_cross_attention as mca
  from easyrec_amd.utils.activation import get_activation
  att_mask = None if mask is None else mca.create_attention_mask_from_input_mask(x, mask)
  return mca.transformer_encoder(x, att_mask, hidden_size=x.shape[-1], num_hidden_layers=layers, num_attention_heads=H,
                                 intermediate_size=intermediate, intermediate_act_fn=get_activation(act), name=name)


def uniter_cfg(kind='all', batch_size=16, hidden=512, heads=4, layers=2, hidden_dropout=0.0, dbmtl=False,
               initializer_range=None):
  """tools/make_configs.uniter_movielens (the sample's sections) with the groups of `kind`: 'all' (image, general,
  text, other), 'image' (the only_image sample) or 'text' (general + text, the only_text sample); dbmtl: the model of
  samples/model_config/dbmtl_uniter_on_movielens.config (towers classify / rating over bottom_uniter).
  initializer_range: the encoder's (the sample leaves the default 0.02, at which the [CLS] rows of a small batch are
  nearly equal and final_dnn's BatchNorm divides fp32 rounding noise by their tiny spread)."""
  import os
  import sys
  from google.protobuf import text_format
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  cfg = make_configs.uniter_movielens(batch_size=batch_size)
  mc = cfg.model_config
  keep = {'all': ('image', 'general', 'text', 'other'), 'image': ('image',), 'text': ('general', 'text')}[kind]
  groups = [g for g in mc.feature_groups if g.group_name in keep]
  del mc.feature_groups[:]
  mc.feature_groups.extend(groups)
  uc = mc.uniter.config
  uc.hidden_size, uc.num_attention_heads, uc.num_hidden_layers = hidden, heads, layers
  uc.intermediate_size, uc.hidden_dropout_prob = hidden, hidden_dropout
  if initializer_range is not None:
    uc.initializer_range = initializer_range
  if kind != 'all':
    uc.ClearField('other_feature_dnn')
  if dbmtl:
    tower = uc.__class__()
    tower.CopyFrom(uc)
    mc.ClearField('uniter')
    mc.model_class = 'DBMTL'
    text_format.Merge('''
      task_towers { tower_name: "classify" label_name: "label" loss_type: CLASSIFICATION metrics_set { auc {} }
                    dnn { hidden_units: [256, 128, 64] } relation_dnn { hidden_units: [32] } weight: 1.0 }
      task_towers { tower_name: "rating" label_name: "rating" loss_type: L2_LOSS metrics_set { mean_squared_error {} }
                    dnn { hidden_units: [256, 128, 64] } relation_tower_names: ["classify"]
                    relation_dnn { hidden_units: [32] } weight: 1.0 }
      l2_regularization: 1e-6''', mc.dbmtl)
    mc.dbmtl.bottom_uniter.CopyFrom(tower)
    cfg.data_config.label_fields.append('rating')
  return cfg


# ------------------------------------------------------------------------------------------------ the reference's fixture
def fixture():
  import os
  import numpy as np
  return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'uniter_vectors.npz'))


def fixture_case(gold, tag):
  """-> (cfg (EasyRecConfig of the case), groups, training, inputs {group: fp64 tensor; 'text': [(emb, len)]},
  variables {TF name: fp64 tensor} in creation order)"""
  import json
  from google.protobuf import text_format
  from easyrec_amd.protos import pipeline_pb2
  meta = json.loads(str(gold['%s:cfg' % tag]))
  cfg = text_format.Parse(meta['config'], pipeline_pb2.EasyRecConfig())
  inputs = {}
  for g in meta['groups']:
    if g == 'text':
      inputs['text'] = [(torch.from_numpy(gold['%s:in:text%d' % (tag, i)]), torch.from_numpy(gold['%s:in:len%d' % (tag, i)]))
                        for i in range(2)]
    else:
      inputs[g] = torch.from_numpy(gold['%s:in:%s' % (tag, g)])
  names = json.loads(str(gold['%s:names' % tag]))
  var = {n: torch.from_numpy(gold['%s:var:%s' % (tag, n)]) for n in names}
  return cfg, meta['groups'], meta['training'], inputs, var


class StubInputLayer(object):
  """The input layer's protocol over ready-made group tensors (the fixture's inputs)."""

  def __init__(self, inputs, device, dtype):
    self.inputs, self.device, self.dtype = inputs, device, dtype

  def has_group(self, name):
    return name in self.inputs

  def __call__(self, features, name, is_combine=True):
    if name == 'text':
      assert not is_combine
      return [(e.to(self.device, self.dtype), n.to(self.device)) for e, n in self.inputs['text']], None, []
    return self.inputs[name].to(self.device, self.dtype), []


def product_fixture_forward(device, cfg, training, inputs, var):
  """The PRODUCT's layers/uniter.Uniter, final_dnn and dense `output` (model/uniter.py's three lines) over the fixture's
  inputs and variables -> (varstore, context, run) with run() -> (layer output, logits)."""
  from easyrec_amd.layers import dnn
  from easyrec_amd.layers import uniter as uniter_layer
  mc = cfg.model_config
  il = StubInputLayer(inputs, device, torch.float32)

  def run():
    layer = uniter_layer.Uniter(mc, list(cfg.feature_config.features), None, mc.uniter.config, il)
    hidden = layer(training, l2_reg=None)
    x = dnn.DNN(mc.uniter.final_dnn, None, 'final_dnn', training)(hidden)
    return hidden, dnn.dense(x, 1, 'output').squeeze(1)

  vs, ctx = product_store(device, run, training=training)
  vs.load_state_dict({k: v.numpy() for k, v in var.items()}, strict=False)
  return vs, ctx, run
