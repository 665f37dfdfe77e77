#!/usr/bin/env python
"""Golden vectors from the REFERENCE'S OWN MultiTowerBST.bst() (model/multi_tower_bst.py:62-151) and its
LayerNormalization (layers/layer_norm.py:9-40), run where a checkout of the reference is available.

It reuses the numpy `tensorflow` stand-in of make_reference_layer_vectors.py (make_tf(), load_reference()) and adds the
ops bst() calls on top of it: slice, cond, pad(mode), ones, rsqrt, reduce_mean over an axis list, tf.layers.dense under
the enclosing variable scopes (AUTO_REUSE: a name seen before is the same variable), a tf.layers.Layer whose unnamed
instances get keras' per-graph unique names (layer_normalization, layer_normalization_1, ...) and keras Ones / Zeros
initializers.  The reference's bst() then runs unmodified on a bare instance; the seeded inputs, every variable under
its TF name and the outputs go to tests/golden/bst_vectors.npz (fp64).

Cases: E = 32 / H = 4, E = 20 / H = 3 (heads 7, 7, 6), E = 9 / H = 6 (5 heads); lengths 0, 1, full and longer than
T - 1; the batch's longest sequence L below T - 1, equal to it and above T; two towers (shared dense variables, their own
LayerNorms).

usage: python tests/golden/make_bst_vectors.py [<reference checkout>]   (default: make_reference_layer_vectors.REF)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_layer_vectors as mrl  # noqa: E402

# (tag, B, L = batch max, T, E, H, lengths, towers)
CASES = [
    ('e32h4_short', 4, 6, 8, 32, 4, [0, 1, 6, 3], 1),       # L < T - 1: padded
    ('e32h4_equal', 4, 7, 8, 32, 4, [7, 0, 1, 5], 1),       # L == T - 1
    ('e32h4_long', 5, 11, 8, 32, 4, [11, 9, 0, 1, 7], 1),   # L > T: sliced; lengths > T - 1
    ('e20h3', 4, 12, 10, 20, 3, [12, 9, 1, 0], 1),          # heads 7, 7, 6
    ('e9h6', 4, 5, 6, 9, 6, [5, 2, 0, 1], 1),               # 5 heads: 2, 2, 2, 2, 1
    ('two_towers', 3, 9, 8, 16, 4, [9, 0, 4], 2),           # shared dense variables, separate LayerNorms
]


class _LayersLayer(object):
  """tf.layers.Layer: an unnamed instance is named after its class in snake case, made unique per graph (keras
  backend.unique_object_name); build() runs once, under a variable scope of that name, on the first call."""
  counts = {}

  def __init__(self, name=None, **kw):
    if name is None:
      base = ''.join('_' + c.lower() if c.isupper() else c for c in self.__class__.__name__).lstrip('_')
      n = _LayersLayer.counts.get(base, 0)
      _LayersLayer.counts[base] = n + 1
      name = base if n == 0 else '%s_%d' % (base, n)
    self.name = name
    self.built = False

  def __call__(self, x, *a, **k):
    tf = sys.modules['tensorflow']
    if not self.built:
      with tf.variable_scope(self.name):
        self.build(np.shape(x))
      self.built = True
    return self.call(x, *a, **k)


def _extend(tf):
  A = mrl._arr

  def layers_dense(inputs, units, activation=None, name=None, **kw):
    full = ''.join(v + '/' for v in mrl.VAR_SCOPES) + name
    x = A(inputs)
    k = mrl.VARS.setdefault(full + '/kernel', mrl._VAR_RNG.standard_normal((x.shape[-1], units)) * 0.4)
    b = mrl.VARS.setdefault(full + '/bias', mrl._VAR_RNG.standard_normal(units) * 0.1)
    y = x @ k + b
    return mrl._tensor(activation(y) if activation is not None else y)

  def tf_slice(x, begin, size):
    x = A(x)
    idx = tuple(slice(b, None if s == -1 else b + s) for b, s in zip(begin, size))
    return mrl._tensor(x[idx])

  tf.layers.dense = layers_dense
  tf.layers.Layer = _LayersLayer
  tf.slice = tf_slice
  tf.cond = lambda pred, true_fn, false_fn: true_fn() if bool(np.asarray(pred)) else false_fn()
  tf.pad = lambda x, paddings, mode='CONSTANT': mrl._tensor(np.pad(A(x), [tuple(int(v) for v in p) for p in paddings]))
  tf.ones = lambda shape, dtype=None: np.ones([int(s) for s in np.asarray(shape)], dtype=dtype or np.float64)
  tf.rsqrt = lambda x: mrl._tensor(1.0 / np.sqrt(A(x)))
  tf.reduce_mean = lambda x, axis=None, keepdims=False: mrl._tensor(
      np.mean(A(x), axis=tuple(axis) if isinstance(axis, (list, tuple)) else axis, keepdims=keepdims))
  tf.float16 = np.float16
  tf.keras.initializers.Ones = mrl._Initializer
  tf.keras.initializers.Zeros = mrl._Initializer

  def get_variable(name=None, shape=None, dtype=None, initializer=None, **kw):
    shape = (shape,) if isinstance(shape, (int, np.integer)) else tuple(int(d) for d in shape)
    full = ''.join(v + '/' for v in mrl.VAR_SCOPES) + name
    if name == 'layer_norm_scale':  # off its ones initial value, so that the consumers must read it
      return mrl.VARS.setdefault(full, 1.0 + 0.2 * mrl._VAR_RNG.standard_normal(shape))
    return mrl.VARS.setdefault(full, 0.1 * mrl._VAR_RNG.standard_normal(shape))

  tf.get_variable = get_variable
  scope = tf.variable_scope
  tf.variable_scope = lambda name=None, name_or_scope=None, **kw: scope(name_or_scope if name is None else name)


def load_bst():
  tf = mrl.make_tf()
  _extend(tf)
  sys.modules['tensorflow'] = tf
  for pkg in ('easy_rec', 'easy_rec.python', 'easy_rec.python.compat', 'easy_rec.python.layers', 'easy_rec.python.model',
              'easy_rec.python.protos'):
    sys.modules[pkg] = types.ModuleType(pkg)
  stubs = {'easy_rec.python.compat.regularizers': {}, 'easy_rec.python.layers.dnn': {},
           'easy_rec.python.layers.seq_input_layer': {}, 'easy_rec.python.model.rank_model': {'RankModel': object},
           'easy_rec.python.protos.multi_tower_pb2': {'MultiTower': object}}
  for name, attrs in stubs.items():
    m = types.ModuleType(name)
    for k, v in attrs.items():
      setattr(m, k, v)
    sys.modules[name] = m
    parent, child = name.rsplit('.', 1)
    setattr(sys.modules[parent], child, m)
  ln = mrl.load_reference('easy_rec/python/layers/layer_norm.py', 'easy_rec.python.layers.layer_norm')
  sys.modules['easy_rec.python.layers.layer_norm'] = ln
  sys.modules['easy_rec.python.layers'].layer_norm = ln
  return mrl.load_reference('easy_rec/python/model/multi_tower_bst.py', 'ref_multi_tower_bst').MultiTowerBST


def main():
  mrl.REF = sys.argv[1] if len(sys.argv) > 1 else mrl.REF
  MultiTowerBST = load_bst()
  rng = np.random.default_rng(2024)
  out = {}
  for tag, B, L, T, E, H, lens, towers in CASES:
    mrl.VARS.clear()
    _LayersLayer.counts.clear()
    model = MultiTowerBST.__new__(MultiTowerBST)  # bare instance: bst() reads nothing from self but its methods
    lens = np.asarray(lens, dtype=np.int64)
    out['%s:cfg' % tag] = np.asarray([B, L, T, E, H, towers], dtype=np.int64)
    out['%s:len' % tag] = lens
    for i in range(towers):
      hist = rng.standard_normal((B, L, E)) * (np.arange(L)[None, :, None] < lens[:, None, None])  # zero padding
      key = rng.standard_normal((B, E))
      res = model.bst({'key': mrl._tensor(key), 'hist_seq_emb': mrl._tensor(hist), 'hist_seq_len': lens}, seq_size=T,
                      head_count=H, name='tower_%d' % i)
      out['%s:key%d' % (tag, i)] = key
      out['%s:hist%d' % (tag, i)] = hist
      out['%s:out%d' % (tag, i)] = np.asarray(res, dtype=np.float64)
    for name, v in mrl.VARS.items():
      out['%s:var:%s' % (tag, name)] = np.asarray(v, dtype=np.float64)
  path = os.path.join(HERE, 'bst_vectors.npz')
  np.savez_compressed(path, **out)
  print('wrote %s (%d arrays, %d bytes)' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
  main()
