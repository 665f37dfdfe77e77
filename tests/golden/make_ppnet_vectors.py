#!/usr/bin/env python
"""Golden vectors from the REFERENCE'S OWN PPNet and GateNN (layers/keras/ppnet.py), run where a checkout of the
reference is available.

It reuses the numpy `tensorflow` stand-in of make_reference_layer_vectors.py (make_tf(), load_reference(), the nested
keras naming) and the module stubs of make_fibinet_vectors.py, and supplies what ppnet.py needs beyond them:
  - tf.stop_gradient (the identity: only forward values are recorded);
  - a name for the two layers GateNN leaves unnamed: keras numbers unnamed layers per graph, so the reference has no
    stable name for them; here `dense` and `batch_normalization` under the gate's own name (this project's choice,
    easyrec_amd/layers/keras/ppnet.py);
  - `training` on the gates' calls: PPNet.call calls its gates without the argument, and keras hands a nested layer the
    enclosing call's value (base_layer's call context), so a gate's BatchNormalization normalises with the batch
    statistics while training;
  - an activation layer that knows tanh besides relu.
The seeded inputs, every variable under its name and the layer's output go to tests/golden/ppnet_vectors.npz (fp64):
data only.

Cases (tag: widths of x and gate_input, then the message in text format), all at B = 6, widths <= 12, dropout 0:
  lazy          mode lazy, everything else the sample's defaults
  eager         mode unset (the proto's default, eager) with gate_params.output_dim = the width of x
  no_full       full_gate_input: false
  gate_bn       gates with use_bn
  gate_hidden   gates with hidden_dim != the output width
  gate_tanh     gates with activation tanh
  mlp_bias      MLP use_bias / use_final_bias
  no_bn         MLP use_bn: false
  single        a single-layer MLP
  eager_single  a single-layer MLP in eager mode: gate_0 only

usage: python tests/golden/make_ppnet_vectors.py [<reference checkout>]   (default: make_reference_layer_vectors.REF)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_fibinet_vectors as mfv  # noqa: E402
import make_reference_layer_vectors as mrl  # noqa: E402

B = 6
WX, WG = 7, 4
MLP = 'mlp { hidden_units: [8, 5] } '
# (tag, message)
CASES = [
    ('lazy', MLP + 'mode: "lazy"'),
    ('eager', MLP + 'gate_params { output_dim: %d }' % WX),
    ('no_full', MLP + 'mode: "lazy" full_gate_input: false'),
    ('gate_bn', MLP + 'mode: "lazy" gate_params { use_bn: true }'),
    ('gate_hidden', MLP + 'mode: "lazy" gate_params { hidden_dim: 6 }'),
    ('gate_tanh', MLP + 'mode: "lazy" gate_params { activation: "tanh" }'),
    ('mlp_bias', 'mlp { hidden_units: [8, 5] use_bias: true use_final_bias: true } mode: "lazy"'),
    ('no_bn', 'mlp { hidden_units: [8, 5] use_bn: false } mode: "lazy"'),
    ('single', 'mlp { hidden_units: [6] } mode: "lazy"'),
    ('eager_single', 'mlp { hidden_units: [6] } mode: "eager" gate_params { output_dim: %d hidden_dim: 5 }' % WX),
]
TRAINING = [None]  # the enclosing PPNet call's `training`


class _Activation(mrl._Layer):

  def __init__(self, kind, name=None):
    super(_Activation, self).__init__(name=name)
    self.kind = kind

  def call(self, x, **kwargs):
    x = mrl._arr(x)
    if self.kind in (None, 'linear'):
      return x
    assert self.kind in ('relu', 'tanh'), self.kind
    return np.maximum(x, 0.0) if self.kind == 'relu' else np.tanh(x)


def load_reference_ppnet():
  """(ppnet module, Parameter) of the reference over the stand-in."""
  _, _, Parameter = mfv.load_reference_blocks()
  tf = sys.modules['tensorflow']
  tf.stop_gradient = lambda x: x
  tf.keras.layers.Dense = lambda units, name=None, **kw: mrl.Dense(units, name=name or 'dense', **kw)
  tf.keras.layers.BatchNormalization = lambda name=None, **kw: mrl.BatchNormalization(name=name or 'batch_normalization', **kw)
  tf.keras.layers.Dropout = mrl.Dropout
  sys.modules['easy_rec.python.layers.keras.activation'].activation_layer = lambda a, name=None: _Activation(a, name)
  ppnet = mrl.load_reference('easy_rec/python/layers/keras/ppnet.py', 'ref_keras_ppnet')
  gate_call = ppnet.GateNN.call

  def call(self, x, training=None, **kwargs):
    return gate_call(self, x, training=TRAINING[0] if training is None else training, **kwargs)

  ppnet.GateNN.call = call
  return ppnet, Parameter


def main():
  mrl.REF = sys.argv[1] if len(sys.argv) > 1 else mrl.REF
  from google.protobuf import text_format
  from easyrec_amd.protos import layer_pb2
  ppnet, Parameter = load_reference_ppnet()
  rng = np.random.default_rng(2028)
  out = {}
  mrl.NEST[0] = True
  for tag, text in CASES:
    mrl.VARS.clear()
    pb = layer_pb2.PPNet()
    text_format.Merge(text, pb)
    x = rng.standard_normal((B, WX)) * 1.3 + 0.2
    u = rng.standard_normal((B, WG)) * 1.3 + 0.2
    layer = ppnet.PPNet(Parameter.make_from_pb(pb), name='ppnet')
    TRAINING[0] = True
    # (PPNet.call multiplies in place: in eager mode that is its input, so it gets copies)
    y = layer((mrl._tensor(x.copy()), mrl._tensor(u.copy())), training=True)
    TRAINING[0] = None
    out['%s:pb' % tag] = np.asarray(text)
    out['%s:x0' % tag] = x
    out['%s:x1' % tag] = u
    out['%s:out' % tag] = np.asarray(y, dtype=np.float64)
    for vname, v in mrl.VARS.items():
      out['%s:var:%s' % (tag, vname)] = np.asarray(v, dtype=np.float64)
      # (training mode reads no moving statistics; keras creates them beside gamma / beta: zeros / ones)
      if vname.endswith('/gamma'):
        out['%s:var:%s' % (tag, vname.replace('/gamma', '/moving_mean'))] = np.zeros_like(v)
        out['%s:var:%s' % (tag, vname.replace('/gamma', '/moving_variance'))] = np.ones_like(v)
  mrl.NEST[0] = False
  path = os.path.join(HERE, 'ppnet_vectors.npz')
  np.savez_compressed(path, **out)
  print('wrote %s (%d arrays, %d bytes)' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
  main()
