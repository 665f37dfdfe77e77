#!/usr/bin/env python
"""Golden vectors from the REFERENCE'S OWN FiBiNet blocks (layers/keras/fibinet.py: SENet, BiLinear, FiBiNet.call) and
input-layer block (layers/common_layers.py: EnhancedInputLayer.call with do_batch_norm), run where a checkout of the
reference is available.

It reuses the numpy `tensorflow` stand-in of make_reference_layer_vectors.py (make_tf(), load_reference(), the nested
keras naming) and adds what these files call on top of it: tf.layers.batch_normalization with TF's default layer names
in creation order (batch_normalization, batch_normalization_1, ...) and a tf.reshape to [-1, ...].  The seeded inputs,
every variable under its reference name and the blocks' outputs go to tests/golden/fibinet_vectors.npz (fp64).

Cases (tag: B, F, D, then the FiBiNet message in text format):
  sample        the sample's geometry: 17 fields of 16, SENet ratio 4, bilinear `each` with use_plus, an MLP
  all_plus      bilinear `all`, use_plus
  each_mul      bilinear `each`, use_plus false
  all_mul       bilinear `all`, use_plus false
  no_bilinear   SENet -> MLP
  no_mlp        SENet | bilinear, no MLP
  se_bare       one squeeze group, no skip connection, no layer norm
  odd           7 fields of 6 (odd F, D not a multiple of 4)
  interaction   bilinear `interaction`: the exception BiLinear.call raises (its type and message), nothing else
  input_bn      EnhancedInputLayer.call, do_batch_norm + only_output_feature_list, training: the per-feature outputs

usage: python tests/golden/make_fibinet_vectors.py [<reference checkout>]   (default: make_reference_layer_vectors.REF)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_reference_layer_vectors as mrl  # noqa: E402

MLP = 'mlp { hidden_units: [12, 6] }'
# (tag, B, F, D, FiBiNet message)
CASES = [
    ('sample', 8, 17, 16, "senet { reduction_ratio: 4 } bilinear { type: 'each' num_output_units: 24 } " + MLP),
    ('all_plus', 8, 6, 8, "senet { reduction_ratio: 3 } bilinear { type: 'all' num_output_units: 10 } " + MLP),
    ('each_mul', 8, 5, 4, "senet { reduction_ratio: 2 } bilinear { type: 'each' use_plus: false num_output_units: 9 } " + MLP),
    ('all_mul', 8, 4, 8, "senet { reduction_ratio: 4 } bilinear { type: 'all' use_plus: false num_output_units: 7 } " + MLP),
    ('no_bilinear', 8, 6, 8, 'senet { reduction_ratio: 4 } ' + MLP),
    ('no_mlp', 8, 6, 8, "senet { reduction_ratio: 4 } bilinear { type: 'each' num_output_units: 10 }"),
    ('se_bare', 8, 5, 8, 'senet { reduction_ratio: 2 num_squeeze_group: 1 use_skip_connection: false '
     "use_output_layer_norm: false } bilinear { type: 'each' num_output_units: 6 } " + MLP),
    ('odd', 8, 7, 6, "senet { reduction_ratio: 4 } bilinear { type: 'each' num_output_units: 11 } " + MLP),
]
BN_COUNT = [0]


def _extend(tf):
  A = mrl._arr

  def batch_normalization(inputs, training=False, name=None, reuse=None, **kw):
    if name is None:  # tf.layers' default: the layer class's snake name, numbered per graph in creation order
      name = 'batch_normalization' if BN_COUNT[0] == 0 else 'batch_normalization_%d' % BN_COUNT[0]
      BN_COUNT[0] += 1
    return mrl._tensor(mrl._layers_batch_normalization(inputs, training=training, name=name, **kw))

  tf.layers.batch_normalization = batch_normalization
  tf.reshape = lambda x, shape: mrl._tensor(np.reshape(A(x), [int(s) for s in shape]))
  tf.GraphKeys = types.SimpleNamespace(UPDATE_OPS='update_ops')
  tf.keras.layers.BatchNormalization = mrl.BatchNormalization
  tf.keras.layers.LayerNormalization = mrl.LayerNormalization


def load_reference_blocks():
  """(fibinet module, common_layers module, Parameter) of the reference over the stand-in."""
  tf = mrl.make_tf()
  _extend(tf)
  sys.modules['tensorflow'] = tf
  relu = tf.nn.relu
  stubs = [('easy_rec', {}), ('easy_rec.python', {}), ('easy_rec.python.utils', {}), ('easy_rec.python.layers', {}),
           ('easy_rec.python.layers.keras', {}), ('easy_rec.python.compat', {}), ('easy_rec.python.protos', {}),
           ('easy_rec.python.compat.layers', {'layer_norm': None}),
           ('easy_rec.python.utils.activation',
            {'get_activation': lambda name, **kw: relu if name in ('relu', 'tf.nn.relu', 'nn.relu') else None}),
           ('tensorflow.python', {}), ('tensorflow.python.keras', {}),
           ('tensorflow.python.keras.initializers', {'Constant': mrl._Initializer}),
           ('tensorflow.python.keras.layers', {'Dense': mrl.Dense, 'Dropout': mrl.Dropout, 'Lambda': mrl._Layer,
                                               'Layer': mrl._Layer}),
           ('easy_rec.python.layers.keras.activation',
            {'activation_layer': lambda a, name=None: mrl._Activation(a, name)}),
           ('easy_rec.python.layers.keras.layer_norm', {'LayerNormalization': mrl.LayerNormalization}),
           ('easy_rec.python.layers.utils', {'Parameter': object}),
           ('easy_rec.python.utils.shape_utils', {'pad_or_truncate_sequence': None}),
           ('easy_rec.python.utils.tf_utils', {'add_elements_to_collection': lambda *a, **k: None})]
  for name, attrs in stubs:
    m = types.ModuleType(name)
    for k, v in attrs.items():
      setattr(m, k, v)
    sys.modules[name] = m
  blocks = mrl.load_reference('easy_rec/python/layers/keras/blocks.py', 'ref_keras_blocks')
  sys.modules['easy_rec.python.layers.keras.blocks'] = blocks
  utils_ref = mrl.load_reference_parameter()
  fib = mrl.load_reference('easy_rec/python/layers/keras/fibinet.py', 'ref_keras_fibinet')
  common = mrl.load_reference('easy_rec/python/layers/common_layers.py', 'ref_common_layers')
  return fib, common, utils_ref.Parameter


def _spy(cls, seen, key):
  real = cls.call

  def call(self, inputs, **kw):
    y = real(self, inputs, **kw)
    seen[key] = np.asarray(y, dtype=np.float64)
    return y

  cls.call = call


def main():
  mrl.REF = sys.argv[1] if len(sys.argv) > 1 else mrl.REF
  from google.protobuf import text_format
  from easyrec_amd.protos import backbone_pb2, layer_pb2
  fib, common, Parameter = load_reference_blocks()
  seen = {}
  _spy(fib.SENet, seen, 'senet')
  _spy(fib.BiLinear, seen, 'bilinear')
  rng = np.random.default_rng(2026)
  out = {}
  mrl.NEST[0] = True
  for tag, B, F, D, text in CASES:
    mrl.VARS.clear()
    seen.clear()
    pb = layer_pb2.FiBiNet()
    text_format.Merge(text, pb)
    x = rng.standard_normal((B, F * D))
    fields = [mrl._tensor(x[:, i * D:(i + 1) * D]) for i in range(F)]
    layer = fib.FiBiNet(Parameter.make_from_pb(pb), name='fibinet')
    y = layer.call(fields, training=True)  # (the block's own call: its sub-layers carry the block's name themselves)
    out['%s:cfg' % tag] = np.asarray([B, F, D], dtype=np.int64)
    out['%s:pb' % tag] = np.asarray(text)
    out['%s:x' % tag] = x
    out['%s:out' % tag] = np.asarray(y, dtype=np.float64)
    for k, v in seen.items():
      out['%s:%s' % (tag, k)] = v
    for name, v in mrl.VARS.items():
      out['%s:var:%s' % (tag, name)] = np.asarray(v, dtype=np.float64)

  # `interaction`: the reference's own call fails for every F >= 2
  mrl.VARS.clear()
  pb = layer_pb2.Bilinear()
  text_format.Merge("type: 'interaction' num_output_units: 4", pb)
  layer = fib.BiLinear(Parameter.make_from_pb(pb), name='bilinear')
  fields = [mrl._tensor(rng.standard_normal((4, 8))) for _ in range(3)]
  try:
    layer(fields)
    raise SystemExit('BiLinear(type=interaction) ran: the recorded defect is gone, revisit layers/keras/fibinet.py')
  except IndexError as e:
    out['interaction:error'] = np.asarray([type(e).__name__, str(e)])
  mrl.NEST[0] = False

  # the input-layer block: do_batch_norm + only_output_feature_list, training
  mrl.VARS.clear()
  BN_COUNT[0] = 0
  B, dims = 8, [4, 4, 6]
  feats = [rng.standard_normal((B, d)) * (1.0 + i) + 0.5 * i for i, d in enumerate(dims)]
  cfg = backbone_pb2.InputLayer()
  text_format.Merge('do_batch_norm: true only_output_feature_list: true', cfg)
  group = lambda feature_dict, name, is_combine=True: (mrl._tensor(np.concatenate(feats, axis=1)),
                                                       [mrl._tensor(f) for f in feats])
  got = common.EnhancedInputLayer(group, {}, 'all')(cfg, True)
  out['input_bn:dims'] = np.asarray(dims, dtype=np.int64)
  out['input_bn:x'] = np.concatenate(feats, axis=1)
  for i, f in enumerate(got):
    out['input_bn:out_%d' % i] = np.asarray(f, dtype=np.float64)
  # (training mode reads no moving statistics; TF creates them beside gamma / beta: zeros / ones)
  for name, v in list(mrl.VARS.items()):
    out['input_bn:var:%s' % name] = np.asarray(v, dtype=np.float64)
    if name.endswith('/gamma'):
      out['input_bn:var:%s' % name.replace('/gamma', '/moving_mean')] = np.zeros_like(v)
      out['input_bn:var:%s' % name.replace('/gamma', '/moving_variance')] = np.ones_like(v)

  path = os.path.join(HERE, 'fibinet_vectors.npz')
  np.savez_compressed(path, **out)
  print('wrote %s (%d arrays, %d bytes)' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
  main()
