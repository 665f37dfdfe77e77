"""What the CMBF tests share beside the restatement (oracle/cmbf_ref.py): the cases of the reference's own run
(tests/golden/cmbf_vectors.npz), the PRODUCT's layer over them, and the test configs."""
import json
import os

import numpy as np
import torch

from tests import _uniter_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture():
  return np.load(os.path.join(ROOT, 'tests', 'golden', 'cmbf_vectors.npz'))


def fixture_case(gold, tag):
  """-> (cfg, groups, training, inputs {group: fp64 tensor; 'text': [(emb, len)]}, variables {TF name: fp64 tensor} in
  creation order)"""
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
  flat, var, o = gold['%s:vars' % tag], {}, 0
  for name, shape in json.loads(str(gold['%s:names' % tag])):
    n = int(np.prod(shape, dtype=np.int64))
    var[name] = torch.from_numpy(flat[o:o + n].reshape(shape).copy())
    o += n
  assert o == flat.size
  return cfg, meta['groups'], meta['training'], inputs, var


def product_fixture_forward(device, cfg, training, inputs, var):
  """The PRODUCT's layers/cmbf.CMBF, final_dnn and dense `output` (model/cmbf.py's three lines) over the fixture's
  inputs and variables -> (varstore, context, run) with run() -> (layer, layer output, logits)."""
  from easyrec_amd.layers import cmbf as cmbf_layer
  from easyrec_amd.layers import dnn
  mc = cfg.model_config
  il = cases.StubInputLayer(inputs, device, torch.float32)

  def run():
    layer = cmbf_layer.CMBF(mc, list(cfg.feature_config.features), None, mc.cmbf.config, il)
    hidden = layer(training, l2_reg=None)
    x = dnn.DNN(mc.cmbf.final_dnn, None, 'final_dnn', training)(hidden)
    return layer, hidden, dnn.dense(x, 1, 'output').squeeze(1)

  vs, ctx = cases.product_store(device, run, training=training)
  vs.load_state_dict({k: v.numpy() for k, v in var.items()}, strict=False)
  return vs, ctx, run


def cmbf_cfg(kind='all', batch_size=16, seq_dropout=0.0, image_layers=None):
  """tools/make_configs.cmbf_movielens (the sample's sections: hidden 32, 33 text tokens, 3 cross layers) with the groups
  of `kind`: 'all' (image, general, text), 'image' (the only_image sample's group) or 'text' (general + text, the
  only_text sample's); text_seq_emb_dropout_prob set to seq_dropout (the sample leaves the default 0.1).  image_layers:
  image_self_attention_layer_num (default: the sample's 0, and 2 for 'image' as in the only_image sample: 64 tokens
  through img_map_matrix)."""
  import sys
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  cfg = make_configs.cmbf_movielens(batch_size=batch_size)
  mc = cfg.model_config
  keep = {'all': ('image', 'general', 'text'), 'image': ('image',), 'text': ('general', 'text')}[kind]
  groups = [g for g in mc.feature_groups if g.group_name in keep]
  del mc.feature_groups[:]
  mc.feature_groups.extend(groups)
  mc.cmbf.config.text_seq_emb_dropout_prob = seq_dropout
  if image_layers is None and kind == 'image':
    image_layers = 2
  if image_layers is not None:
    mc.cmbf.config.image_self_attention_layer_num = image_layers
  return cfg
