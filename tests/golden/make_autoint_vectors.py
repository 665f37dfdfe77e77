#!/usr/bin/env python
"""Golden vectors from the REFERENCE'S OWN AutoInt (model/autoint.py:50-80) and MultiHeadAttention
(layers/multihead_attention.py:9-161), run where a checkout of the reference is available.

It reuses the numpy `tensorflow` stand-in of make_reference_layer_vectors.py (make_tf(), load_reference()) and adds
the ops these two files call on top of it: tf.layers.dense on 3-D input (use_bias, kernel_regularizer ignored: the L2
term is not part of the forward), tf.linalg.matmul(a, b, transpose_b) and a reshape to [-1, ...].  The reference's
build_predict_graph then runs unmodified on a bare instance; the seeded inputs, every variable under its TF name, each
interacting layer's output and the logits go to tests/golden/autoint_vectors.npz (fp64).

Cases (tag: B, fields from feature_names + hist_seq, key fields, D, heads, head size, layers):
  f18   the plain sample: 18 fields, D 16, 2 heads x 32, 3 layers
  odd   5 fields, D 8, 3 heads x 7, 2 layers (d = 21: odd widths everywhere)
  h1    one head of size D
  f20   the sequence sample's 20 fields (18 + 2 keys)
  l0    no interacting layer: the embeddings flattened straight into the output layer

usage: python tests/golden/make_autoint_vectors.py [<reference checkout>]   (default: make_reference_layer_vectors.REF)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_layer_vectors as mrl  # noqa: E402

# (tag, B, feature_num, seq_key_num, D, H, ds, layers)
CASES = [
    ('f18', 5, 18, 0, 16, 2, 32, 3),
    ('odd', 4, 5, 0, 8, 3, 7, 2),
    ('h1', 3, 6, 0, 12, 1, 12, 2),
    ('f20', 3, 18, 2, 16, 2, 32, 2),
    ('l0', 4, 7, 0, 8, 2, 4, 0),
]


def _extend(tf):
  A = mrl._arr

  def layers_dense(inputs, units, use_bias=True, kernel_regularizer=None, activation=None, name=None, **kw):
    x = A(inputs)
    lim = np.sqrt(6.0 / (x.shape[-1] + units))  # glorot_uniform, as the reference's default
    k = mrl.VARS.setdefault(name + '/kernel', mrl._VAR_RNG.uniform(-lim, lim, (x.shape[-1], units)))
    y = x @ k
    if use_bias:
      y = y + mrl.VARS.setdefault(name + '/bias', mrl._VAR_RNG.standard_normal(units) * 0.1)
    return mrl._tensor(activation(y) if activation is not None else y)

  tf.layers.dense = layers_dense
  tf.linalg.matmul = lambda a, b, transpose_a=False, transpose_b=False: mrl._tensor(
      (np.swapaxes(A(a), -1, -2) if transpose_a else A(a)) @ (np.swapaxes(A(b), -1, -2) if transpose_b else A(b)))
  tf.reshape = lambda x, shape: mrl._tensor(np.reshape(A(x), [int(s) for s in shape]))
  tf.transpose = lambda x, perm: mrl._tensor(np.transpose(A(x), perm))
  tf.nn.softmax = lambda x, axis=-1, name=None: mrl._tensor(mrl._softmax(A(x), axis))
  tf.nn.relu = lambda x, name=None: mrl._tensor(np.maximum(A(x), 0.0))


def load_autoint():
  tf = mrl.make_tf()
  _extend(tf)
  sys.modules['tensorflow'] = tf
  for pkg in ('easy_rec', 'easy_rec.python', 'easy_rec.python.layers', 'easy_rec.python.model',
              'easy_rec.python.protos'):
    sys.modules[pkg] = types.ModuleType(pkg)
  stubs = {'easy_rec.python.model.rank_model': {'RankModel': object},
           'easy_rec.python.protos.autoint_pb2': {'AutoInt': object}}
  for name, attrs in stubs.items():
    m = types.ModuleType(name)
    for k, v in attrs.items():
      setattr(m, k, v)
    sys.modules[name] = m
    parent, child = name.rsplit('.', 1)
    setattr(sys.modules[parent], child, m)
  mha = mrl.load_reference('easy_rec/python/layers/multihead_attention.py', 'easy_rec.python.layers.multihead_attention')
  sys.modules['easy_rec.python.layers.multihead_attention'] = mha
  sys.modules['easy_rec.python.layers'].multihead_attention = mha
  return mha, mrl.load_reference('easy_rec/python/model/autoint.py', 'ref_autoint').AutoInt


def main():
  mrl.REF = sys.argv[1] if len(sys.argv) > 1 else mrl.REF
  mha, AutoInt = load_autoint()
  seen = []
  real_call = mha.MultiHeadAttention.__call__

  def spy(self, x):
    y = real_call(self, x)
    seen.append(np.asarray(y, dtype=np.float64))
    return y

  mha.MultiHeadAttention.__call__ = spy
  rng = np.random.default_rng(2025)
  out = {}
  for tag, B, feature_num, seq_key_num, D, H, ds, layers in CASES:
    mrl.VARS.clear()
    del seen[:]
    F = feature_num + seq_key_num
    x = rng.standard_normal((B, F * D))
    model = AutoInt.__new__(AutoInt)  # bare instance: build_predict_graph reads only these attributes
    model._features = mrl._tensor(x)
    model._feature_num, model._seq_key_num, model._d_model = feature_num, seq_key_num, D
    model._head_num, model._head_size, model._l2_reg, model._num_class = H, ds, None, 1
    model._model_config = types.SimpleNamespace(interacting_layer_num=layers)
    model._prediction_dict = {}
    model._add_to_prediction_dict = lambda logits, m=model: m._prediction_dict.update(logits=np.asarray(logits))
    model.build_predict_graph()
    out['%s:cfg' % tag] = np.asarray([B, feature_num, seq_key_num, D, H, ds, layers], dtype=np.int64)
    out['%s:x' % tag] = x
    for i, y in enumerate(seen):
      out['%s:layer%d' % (tag, i)] = y
    out['%s:logits' % tag] = np.asarray(model._prediction_dict['logits'], dtype=np.float64)
    for name, v in mrl.VARS.items():
      out['%s:var:%s' % (tag, name)] = np.asarray(v, dtype=np.float64)
  path = os.path.join(HERE, 'autoint_vectors.npz')
  np.savez_compressed(path, **out)
  print('wrote %s (%d arrays, %d bytes)' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
  main()
