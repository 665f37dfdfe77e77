#!/usr/bin/env python
"""Golden vectors from the REFERENCE'S OWN variational dropout, run where a checkout of the reference is available:
  easy_rec/python/layers/variational_dropout_layer.py   VariationalDropoutLayer, whole
  easy_rec/python/layers/input_layer.py                 InputLayer.single_call_input_layer, the variational-dropout
                                                        branch (:348-362) with what surrounds it (:302-376)
over the numpy `tensorflow` stand-in of make_reference_layer_vectors.py and the input-layer stand-ins of
make_seq_combiner_vectors.py (columns, builder, variable scopes hold seeded tensors: the feature columns themselves are
pinned by other fixtures).  The stand-in gains what the layer needs beyond them: tf.random_uniform (seeded, the draw
recorded), tf.log, tf.range, tf.tile / tf.concat / tf.reshape / tf.expand_dims that keep integer indices, tf.gather_nd,
tf.get_variable with `initializer` (seeded values; name and shape recorded) and the collections.  Everything goes to
tests/golden/vdrop_vectors.npz (fp64): data only.

Cases, B = 6 (`two` 5 and 6), widths <= 12; every case runs single_call_input_layer on one group:
  ew_train   group `all`, embedding-wise, training, plain columns of widths [1, 3, 4]        -> variable `logit_p`
  fw_train   group `g`, feature-wise, training, the same widths                              -> variable `logit_p_g`
  ew_eval, fw_eval   both modes with is_training False (no noise)
  seq        group `user`: plain columns [2, 3] and a sequence column `hist` (attention combiner, width 4) after them;
             an embedding regulariser (its weights_list recorded: the tensors BEFORE dropout) and the
             feature_name_to_output_tensors dict (BEFORE dropout); the returned feature list (the split AFTER dropout)
  two        groups `deep` (6 rows) and `wide` (5 rows) in one graph: the `variational_dropout_loss` collection holds one
             penalty per group, each with its own row count; their sum is the loss

usage: python tests/golden/make_vdrop_vectors.py [<reference checkout>]   (default: make_reference_layer_vectors.REF)
"""
import contextlib
import os
import sys
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_reference_layer_vectors as base  # noqa: E402
import make_seq_combiner_vectors as msc  # noqa: E402

RNG = np.random.default_rng(20261021)
COLLECTIONS = {}
DRAWS = []     # the uniform draws of the current case, in order
CREATED = []   # (variable name, value) of the current case, in creation order
REG = []       # weights_list of every apply_regularization call of the current case


def extend_tf(tf):
  msc.extend_tf(tf)
  keep = lambda x: x if isinstance(x, np.ndarray) else np.asarray(x)
  tf.float32 = np.float64
  tf.log = lambda x: np.log(base._arr(x))
  tf.range = lambda n: np.arange(int(n))
  tf.tile = lambda x, multiples: np.tile(keep(x), [int(m) for m in multiples])
  tf.concat = lambda xs, axis=-1: np.concatenate([keep(x) for x in xs], axis=axis)
  tf.expand_dims = lambda x, axis: np.expand_dims(keep(x), axis)
  tf.reshape = lambda x, shape: np.reshape(keep(x), [int(s) for s in shape])
  tf.shape = lambda x: np.asarray(np.shape(x))
  tf.gather_nd = lambda params, indices: keep(params)[tuple(np.asarray(indices).astype(np.int64).T)]
  tf.split = lambda x, sizes, axis=-1: np.split(keep(x), np.cumsum(sizes)[:-1], axis=axis)
  tf.add_to_collection = lambda name, value: COLLECTIONS.setdefault(name, []).append(value)
  tf.get_collection = lambda name: list(COLLECTIONS.get(name, []))

  def random_uniform(shape, dtype=None, seed=None, name=None):
    u = RNG.random([int(s) for s in shape]).astype(np.float32).astype(np.float64)  # (values an fp32 run can be fed)
    DRAWS.append(u)
    return u
  tf.random_uniform = random_uniform

  def get_variable(name=None, shape=None, dtype=None, initializer=None, **kw):
    assert initializer is None and dtype is np.float64
    full = ''.join(s + '/' for s in msc.SCOPES) + name
    value = RNG.uniform(-2.5, 2.5, [int(s) for s in shape])
    CREATED.append((full, value))
    return value
  tf.get_variable = get_variable


def load_reference_modules():
  """(variational_dropout_layer, input_layer) of the reference over the stand-in."""
  base.sys.modules['tensorflow'] = tf = base.make_tf()
  extend_tf(tf)
  for pkg in ('easy_rec', 'easy_rec.python', 'easy_rec.python.utils', 'easy_rec.python.layers', 'easy_rec.python.compat',
              'easy_rec.python.compat.feature_column', 'easy_rec.python.feature_column', 'easy_rec.python.protos',
              'easy_rec.python.layers.keras'):
    sys.modules.setdefault(pkg, types.ModuleType(pkg))
  from easyrec_amd import protos

  @contextlib.contextmanager
  def variable_scope(name, default_name=None, **kw):
    msc.SCOPES.append(name if name is not None else default_name)
    try:
      yield
    finally:
      msc.SCOPES.pop()

  def input_layer(features, columns, cols_to_output_tensors=None, feature_name_to_output_tensors=None, **kw):
    # (feature_column.input_layer: the plain columns' outputs, concatenated in the columns' order)
    for c in columns:
      cols_to_output_tensors[c] = c.tensor
      if feature_name_to_output_tensors is not None:
        feature_name_to_output_tensors[c.raw_name] = c.tensor
    width0 = np.zeros((features['rows'], 0))
    return base._tensor(np.concatenate([width0] + [np.asarray(c.tensor) for c in columns], axis=1))

  fc_mod = types.ModuleType('easy_rec.python.compat.feature_column.feature_column')
  fc_mod.input_layer = input_layer
  fc_mod._LazyBuilder = lambda features: None
  fc_mod._SharedEmbeddingColumn = object
  mods = {
      'tensorflow.python': {}, 'tensorflow.python.framework': {}, 'tensorflow.python.framework.ops': {},
      'tensorflow.python.ops': {},
      'tensorflow.python.ops.array_ops': {'concat': lambda xs, axis=-1: np.concatenate([np.asarray(x) for x in xs], axis=axis)},
      'tensorflow.python.ops.variable_scope': {'variable_scope': variable_scope},
      'easy_rec.python.compat.regularizers': {
          'apply_regularization': lambda reg, weights_list=None: REG.append([np.asarray(w) for w in weights_list])},
      'easy_rec.python.compat.feature_column.feature_column_v2': {'is_embedding_column': lambda c: True,
                                                                  'EmbeddingColumn': object},
      'easy_rec.python.feature_column.feature_column': {'FeatureColumnParser': object},
      'easy_rec.python.feature_column.feature_group': {'FeatureGroup': object},
      'easy_rec.python.layers.sequence_feature_layer': {},
      'easy_rec.python.layers.utils': {'Parameter': object},
      'easy_rec.python.protos.feature_config_pb2': {'WideOrDeep': protos.feature_config_pb2.WideOrDeep},
      'easy_rec.python.utils.conditional': {}, 'easy_rec.python.utils.shape_utils': {},
  }
  for name, attrs in mods.items():
    m = types.ModuleType(name)
    for k, v in attrs.items():
      setattr(m, k, v)
    sys.modules[name] = m
  sys.modules['easy_rec.python.compat.feature_column.feature_column'] = fc_mod
  sys.modules['easy_rec.python.compat.feature_column'].feature_column = fc_mod
  sys.modules['easy_rec.python.compat'].regularizers = sys.modules['easy_rec.python.compat.regularizers']
  sys.modules['tensorflow.python.ops'].array_ops = sys.modules['tensorflow.python.ops.array_ops']
  sys.modules['tensorflow.python.ops'].variable_scope = sys.modules['tensorflow.python.ops.variable_scope']
  sys.modules['tensorflow.python.framework'].ops = sys.modules['tensorflow.python.framework.ops']
  sys.modules['easy_rec.python.layers.keras'].TextCNN = object
  sys.modules['easy_rec.python.utils'].conditional = sys.modules['easy_rec.python.utils.conditional']
  sys.modules['easy_rec.python.utils'].shape_utils = sys.modules['easy_rec.python.utils.shape_utils']
  vd_mod = base.load_reference('easy_rec/python/layers/variational_dropout_layer.py',
                               'easy_rec.python.layers.variational_dropout_layer')
  sys.modules['easy_rec.python.layers.variational_dropout_layer'] = vd_mod
  layers_pkg = sys.modules['easy_rec.python.layers']
  layers_pkg.sequence_feature_layer = sys.modules['easy_rec.python.layers.sequence_feature_layer']
  layers_pkg.variational_dropout_layer = vd_mod
  il_mod = base.load_reference('easy_rec/python/layers/input_layer.py', 'ref_layers_input_layer')
  return vd_mod, il_mod, protos


class Column(object):
  """a plain column holding its seeded output"""

  def __init__(self, raw, tensor):
    self.raw_name, self.name, self._var_scope_name = raw, raw + '_embedding', raw + '_embedding'
    self.tensor = base._tensor(tensor)


def run_group(il_mod, protos, out, tag, group_name, rows, dims, embedding_wise, training, lam, seq=None, reg=None):
  """one single_call_input_layer call; records everything under `<tag>:`"""
  from google.protobuf import text_format
  del DRAWS[:], CREATED[:], REG[:]
  plain = [Column(name, RNG.standard_normal((rows, d)) * 1.3 + 0.2) for name, d in dims]
  seq_cols = []
  if seq is not None:
    name, D, L = seq
    pb = protos.feature_config_pb2.SequenceCombiner()
    text_format.Merge('attention { }', pb)
    lens = np.array([L, 1, 3, 0, 2, L][:rows], dtype=np.int64)
    emb = RNG.standard_normal((rows, L, D)) * (np.arange(L)[None, :] < lens[:, None])[:, :, None]
    col = Column(name, np.zeros((rows, 0)))
    col.sequence_combiner = pb
    col._get_sequence_dense_tensor = lambda builder: (base._tensor(emb), lens)
    seq_cols.append(col)
    out['%s:seq_x' % tag], out['%s:seq_len' % tag] = emb, lens
  msc.CASE[0] = tag
  cfg = types.SimpleNamespace(regularization_lambda=lam, embedding_wise_variational_dropout=embedding_wise)
  group = types.SimpleNamespace(select_columns=lambda parser: (plain, seq_cols))
  fake = types.SimpleNamespace(_feature_groups={group_name: group}, _fc_parser=None, _is_training=training,
                               _kernel_regularizer=None, _variational_dropout_config=cfg, _embedding_regularizer=reg)
  names = {}
  base.NEST[0] = True
  try:
    concat, feats = il_mod.InputLayer.single_call_input_layer(fake, {'rows': rows}, group_name, names)
  finally:
    base.NEST[0] = False
  assert len(CREATED) == 1 and len(DRAWS) == (1 if training else 0)
  out['%s:group' % tag] = np.array(group_name)
  out['%s:embedding_wise' % tag], out['%s:training' % tag] = np.array(embedding_wise), np.array(training)
  out['%s:lambda' % tag] = np.array(lam)
  out['%s:plain_names' % tag] = np.array([n for n, _ in dims])
  out['%s:plain_dims' % tag] = np.array([d for _, d in dims])
  for c in plain:
    out['%s:x:%s' % (tag, c.raw_name)] = np.asarray(c.tensor)
  out['%s:var_name' % tag], out['%s:logit_p' % tag] = np.array(CREATED[0][0]), CREATED[0][1]
  if training:
    out['%s:u' % tag] = DRAWS[0]
  out['%s:out' % tag] = np.asarray(concat)
  out['%s:n_feats' % tag] = np.array(len(feats))
  for i, f in enumerate(feats):
    out['%s:feat:%d' % (tag, i)] = np.asarray(f)
  for k, v in names.items():
    out['%s:dict:%s' % (tag, k)] = np.asarray(v)
  for i, w in enumerate(REG[0] if REG else []):
    out['%s:reg:%d' % (tag, i)] = w
  for k, v in base.VARS.items():  # (the attention kernel of a sequence column)
    if k.startswith(tag + ':var:'):
      out[k] = np.asarray(v)


def main():
  base.REF = msc.REF = sys.argv[1] if len(sys.argv) > 1 else base.REF
  vd_mod, il_mod, protos = load_reference_modules()
  out = OrderedDict()
  dims = [('a', 1), ('b', 3), ('c', 4)]
  for tag, group, ew, training in (('ew_train', 'all', True, True), ('fw_train', 'g', False, True),
                                   ('ew_eval', 'all', True, False), ('fw_eval', 'g', False, False)):
    COLLECTIONS.clear()
    run_group(il_mod, protos, out, tag, group, 6, dims, ew, training, 0.01)
    out['%s:penalty' % tag] = np.asarray(COLLECTIONS['variational_dropout_loss'][0])
    out['%s:collection' % tag] = np.array(COLLECTIONS['variational_dropout'][0])
  COLLECTIONS.clear()
  run_group(il_mod, protos, out, 'seq', 'user', 6, [('age', 2), ('city', 3)], False, True, 0.02, seq=('hist', 4, 5), reg=1e-4)
  out['seq:penalty'] = np.asarray(COLLECTIONS['variational_dropout_loss'][0])
  out['seq:collection'] = np.array(COLLECTIONS['variational_dropout'][0])
  COLLECTIONS.clear()
  run_group(il_mod, protos, out, 'two_deep', 'deep', 6, [('a', 4), ('b', 4)], True, True, 0.05)
  run_group(il_mod, protos, out, 'two_wide', 'wide', 5, [('a', 1), ('b', 1)], True, True, 0.05)
  pens = COLLECTIONS['variational_dropout_loss']
  assert len(pens) == 2
  out['two_deep:penalty'], out['two_wide:penalty'] = np.asarray(pens[0]), np.asarray(pens[1])
  out['two_deep:collection'], out['two_wide:collection'] = [np.array(c) for c in COLLECTIONS['variational_dropout']]
  tf = sys.modules['tensorflow']
  out['two:loss'] = np.asarray(tf.add_n(tf.get_collection('variational_dropout_loss')))  # (easy_rec_estimator.py:177-181)
  path = os.path.join(HERE, 'vdrop_vectors.npz')
  np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
  print('wrote %s (%d arrays, %d bytes)' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
  main()
