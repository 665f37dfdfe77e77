#!/usr/bin/env python
"""Golden vectors from the REFERENCE'S OWN Uniter: layers/uniter.py, layers/multihead_cross_attention.py and
model/uniter.py run unmodified, where a checkout of the reference is available, over the numpy `tensorflow` stand-in of
make_reference_layer_vectors.py (make_tf(), load_reference()).

New stand-in pieces: tf.layers.dense with bias, default name `dense` and `reuse` under the variable scopes;
tf.variable_scope with AUTO_REUSE (variables are found again by name); tf.map_fn, tf.one_hot, tf.slice, tf.ones /
tf.zeros, tf.to_int32; tf.assert_less_equal / tf.control_dependencies as no-ops; tf.truncated_normal_initializer
(ignored: the variables are seeded here).  `easy_rec.python.compat.layers.layer_norm` is TensorFlow's contrib code, not
the reference's own: it is RESTATED here like the other TF arithmetic (normalise over the last axis with the mean and
the mean of squared differences, epsilon 1e-12, `beta` / `gamma` under the scope, default scope `LayerNorm` made unique
per enclosing variable scope in call order).  `utils.activation.get_activation` / `gelu` and `shape_utils.get_shape_list`
are small stand-ins too, and `dnn.DNN` is make_match_vectors' dense -> BatchNorm -> relu stack.  The input layer is a
stub that hands out the seeded group tensors; RankModel is a bare base whose _add_to_prediction_dict squeezes the
logits and takes their sigmoid (num_class 1).

Cases, each with hidden 12, 3 heads, 2 layers, intermediate 10, B = 6 (text lengths 0, 1 and max_seq_len among them),
both dropouts 0: all (the four groups), image (image only), text_tanh (text only, hidden_act tanh), nopos
(use_position_embeddings false), general_hidden (general width = hidden: no txt_projection), other_plain (`other`
without other_feature_dnn), eval (is_training False).  Inputs, every variable under its TF name in creation order, the
encoder output, the [CLS] feature, the layer output, logits and probs go to tests/golden/uniter_vectors.npz (fp64).

usage: python tests/golden/make_uniter_vectors.py [<reference checkout>]   (default: make_reference_layer_vectors.REF)
"""
import contextlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_match_vectors as mm  # noqa: E402
import make_reference_layer_vectors as mrl  # noqa: E402

B, HIDDEN, HEADS, LAYERS, INTER = 6, 12, 3, 2, 10
IMG_DIM, GEN_N, GEN_DIM, TXT_DIM, TXT_LENS, OTHER_W = 9, 3, 5, 4, (5, 3), 6
# tag -> (groups, overrides)
CASES = [
    ('all', ('image', 'general', 'text', 'other'), {}),
    ('image', ('image',), {}),
    ('text_tanh', ('text',), {'hidden_act': 'tanh'}),
    ('nopos', ('image', 'general', 'text', 'other'), {'use_position_embeddings': False}),
    ('general_hidden', ('image', 'general', 'text'), {'general_dim': HIDDEN}),
    ('other_plain', ('general', 'text', 'other'), {'other_dnn': False}),
    ('eval', ('image', 'general', 'text', 'other'), {'training': False}),
]
LN_COUNTS = {}


def _scope():
  return mrl.MODEL_SCOPE[0] + ''.join(v + '/' for v in mrl.VAR_SCOPES)


def _extend(tf):
  A, T = mrl._arr, mrl._tensor

  def dense(inputs, units, activation=None, name=None, kernel_initializer=None, reuse=None, **kw):
    x = A(inputs)
    full = _scope() + (name or 'dense')
    k = mrl.VARS.setdefault(full + '/kernel', mrl._VAR_RNG.standard_normal((x.shape[-1], units)) * 0.4)
    b = mrl.VARS.setdefault(full + '/bias', mrl._VAR_RNG.standard_normal(units) * 0.1)
    y = x @ k + b
    return T(activation(y) if activation is not None else y)

  tf.layers.dense = dense
  tf.truncated_normal_initializer = lambda stddev=1.0: None
  tf.ones = lambda shape, dtype=None: T(np.ones([int(s) for s in np.asarray(shape).reshape(-1)], dtype=dtype or np.float64))
  tf.zeros = lambda shape, dtype=None: T(np.zeros([int(s) for s in np.asarray(shape).reshape(-1)], dtype=dtype or np.float64))
  tf.to_int32 = lambda x: np.asarray(x).astype(np.int64)
  tf.map_fn = lambda fn, elems: T(np.stack([np.asarray(fn(int(t))) for t in np.asarray(elems)]))
  tf.one_hot = lambda ids, depth: T(np.eye(int(depth))[np.asarray(ids).astype(np.int64)])
  tf.slice = lambda x, begin, size: T(A(x)[tuple(slice(b, None if s == -1 else b + int(s)) for b, s in zip(begin, size))])
  tf.assert_less_equal = lambda a, b: None
  tf.control_dependencies = lambda deps: contextlib.nullcontext()
  tf.concat = lambda xs, axis=-1: T(np.concatenate([np.asarray(x) for x in xs], axis=axis))
  tf.stack = lambda xs, axis=0: np.stack([np.asarray(x) for x in xs], axis=axis)
  tf.tanh = lambda x: T(np.tanh(A(x)))
  tf.matmul = lambda a, b, transpose_b=False: T(A(a) @ (np.swapaxes(A(b), -1, -2) if transpose_b else A(b)))
  tf.nn.relu = lambda x, name=None: T(np.maximum(A(x), 0.0))


def layer_norm(inputs, begin_norm_axis=-1, begin_params_axis=-1, scope=None):
  """compat/layers.py layer_norm (TF contrib), restated: see the module docstring."""
  assert begin_norm_axis == -1 and begin_params_axis == -1
  x = mrl._arr(inputs)
  if scope is None:
    n = LN_COUNTS[_scope()] = LN_COUNTS.get(_scope(), -1) + 1
    scope = 'LayerNorm' if n == 0 else 'LayerNorm_%d' % n
  full = _scope() + scope
  beta = mrl.VARS.setdefault(full + '/beta', mrl._VAR_RNG.standard_normal(x.shape[-1]) * 0.2)
  gamma = mrl.VARS.setdefault(full + '/gamma', mrl._VAR_RNG.random(x.shape[-1]) + 0.5)
  mean = x.mean(axis=-1, keepdims=True)
  var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
  return mrl._tensor((x - mean) / np.sqrt(var + 1e-12) * gamma + beta)


def _gelu(x):
  x = mrl._arr(x)
  return mrl._tensor(x * 0.5 * (1.0 + np.tanh(np.sqrt(2 / np.pi) * (x + 0.044715 * np.power(x, 3)))))


def _get_activation(name, **kw):
  x_ = mrl._arr
  return {'gelu': _gelu, 'tanh': lambda x: mrl._tensor(np.tanh(x_(x))), 'relu': lambda x: mrl._tensor(np.maximum(x_(x), 0.0)),
          'swish': lambda x: mrl._tensor(x_(x) / (1.0 + np.exp(-x_(x))))}[name.lower()]


def load_uniter():
  tf = mrl.make_tf()
  mm._extend(tf)
  _extend(tf)
  sys.modules['tensorflow'] = tf
  for pkg in ('easy_rec', 'easy_rec.python', 'easy_rec.python.layers', 'easy_rec.python.model', 'easy_rec.python.protos',
              'easy_rec.python.compat', 'easy_rec.python.utils'):
    sys.modules[pkg] = types.ModuleType(pkg)

  def module(name, **attrs):
    m = sys.modules[name] = types.ModuleType(name)
    for k, v in attrs.items():
      setattr(m, k, v)
    setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], m)
    return m

  module('easy_rec.python.compat.layers', layer_norm=layer_norm)
  module('easy_rec.python.utils.activation', gelu=_gelu, get_activation=_get_activation)
  module('easy_rec.python.utils.shape_utils',
         get_shape_list=lambda t, expected_rank=None, name=None: [int(s) for s in np.asarray(t).shape])
  module('easy_rec.python.layers.dnn', DNN=mm._DNN)

  class RankModel(object):

    def _add_to_prediction_dict(self, output):
      z = np.squeeze(mrl._arr(output), axis=1)
      self._prediction_dict['logits'] = z
      self._prediction_dict['probs'] = 1.0 / (1.0 + np.exp(-z))

  module('easy_rec.python.model.rank_model', RankModel=RankModel)
  module('easy_rec.python.protos.uniter_pb2', Uniter=object)
  mca = mrl.load_reference('easy_rec/python/layers/multihead_cross_attention.py',
                           'easy_rec.python.layers.multihead_cross_attention')
  sys.modules['easy_rec.python.layers.multihead_cross_attention'] = mca
  sys.modules['easy_rec.python.layers'].multihead_cross_attention = mca
  layer = mrl.load_reference('easy_rec/python/layers/uniter.py', 'easy_rec.python.layers.uniter')
  sys.modules['easy_rec.python.layers.uniter'] = layer
  sys.modules['easy_rec.python.layers'].uniter = layer
  model = mrl.load_reference('easy_rec/python/model/uniter.py', 'easy_rec.python.model.uniter')
  return mca, layer, model


def case_config(groups, opts):
  """(model_config, feature_configs) of a case as this repository's protos (the reference reads the same fields)."""
  from google.protobuf import text_format
  from easyrec_amd.protos import pipeline_pb2
  gen_dim = opts.get('general_dim', GEN_DIM)
  feats = ["features { input_names: 'img' feature_type: RawFeature raw_input_dim: %d }" % IMG_DIM]
  feats += ["features { input_names: 'g%d' feature_type: IdFeature embedding_dim: %d num_buckets: 10 }" % (i, gen_dim)
            for i in range(GEN_N)]
  feats += ["features { input_names: 't%d' feature_type: SequenceFeature embedding_dim: %d max_seq_len: %d "
            "hash_bucket_size: 50 }" % (i, TXT_DIM, L) for i, L in enumerate(TXT_LENS)]
  feats += ["features { input_names: 'o0' feature_type: RawFeature raw_input_dim: %d }" % OTHER_W]
  names = {'image': ['img'], 'general': ['g%d' % i for i in range(GEN_N)], 'text': ['t0', 't1'], 'other': ['o0']}
  fg = ' '.join("feature_groups { group_name: '%s' %s wide_deep: DEEP }" %
                (g, ' '.join("feature_names: '%s'" % n for n in names[g])) for g in groups)
  other = 'other_feature_dnn { hidden_units: 7 }' if ('other' in groups and opts.get('other_dnn', True)) else ''
  text = '''feature_config { %s }
    model_config { model_class: 'Uniter' %s
      uniter { config { hidden_size: %d num_attention_heads: %d num_hidden_layers: %d intermediate_size: %d
                        hidden_act: '%s' max_position_embeddings: 6 hidden_dropout_prob: 0 attention_probs_dropout_prob: 0
                        use_position_embeddings: %s %s }
               final_dnn { hidden_units: 8 hidden_units: 5 } } }''' % (
      ' '.join(feats), fg, HIDDEN, HEADS, LAYERS, INTER, opts.get('hidden_act', 'gelu'),
      'true' if opts.get('use_position_embeddings', True) else 'false', other)
  cfg = text_format.Parse(text, pipeline_pb2.EasyRecConfig())
  return cfg, text


class StubInputLayer(object):

  def __init__(self, groups, tensors):
    self.groups, self.tensors = groups, tensors

  def has_group(self, name):
    return name in self.groups

  def __call__(self, features, name, is_combine=True):
    if name == 'text':
      return [(mrl._tensor(np.array(e)), np.array(n)) for e, n in self.tensors['text']], None, None
    # (copies: the reference's `output += ..` is an in-place add on a numpy array, a new tensor in TensorFlow)
    return mrl._tensor(np.array(self.tensors[name])), None


def main():
  mca, layer_mod, model_mod = load_uniter()
  rng = np.random.default_rng(2024)
  out = {}
  for tag, groups, opts in CASES:
    mrl.MODEL_SCOPE[0] = tag + '::'
    LN_COUNTS.clear()
    cfg, text = case_config(groups, opts)
    gen_dim = opts.get('general_dim', GEN_DIM)
    lens = [np.array([0, 1, L, 2, L, 1][:B]) for L in TXT_LENS]
    tensors = {'image': rng.standard_normal((B, IMG_DIM)), 'general': rng.standard_normal((B, GEN_N * gen_dim)),
               'other': rng.standard_normal((B, OTHER_W)), 'text': []}
    for L, n in zip(TXT_LENS, lens):
      e = rng.standard_normal((B, L, TXT_DIM))
      e[np.arange(L)[None, :] >= n[:, None]] = 0.0  # (padding rows of a sequence embedding are zero)
      tensors['text'].append((e, n))
    training = opts.get('training', True)
    seen = {}
    real = mca.transformer_encoder

    def spy(*a, **k):
      seen['encoder'] = real(*a, **k)
      return seen['encoder']

    mca.transformer_encoder = spy
    try:
      mc = cfg.model_config
      ulayer = layer_mod.Uniter(mc, list(cfg.feature_config.features), None, mc.uniter.config,
                                StubInputLayer(groups, tensors))
      model = object.__new__(model_mod.Uniter)
      model._uniter_layer, model._is_training, model._l2_reg = ulayer, training, 0.0
      model._model_config, model._num_class, model._prediction_dict = mc.uniter, 1, {}
      real_call = ulayer.__class__.__call__

      def call(self, *a, **k):
        seen['hidden'] = real_call(self, *a, **k)
        return seen['hidden']

      ulayer.__class__.__call__ = call
      try:
        pred = model.build_predict_graph()
      finally:
        ulayer.__class__.__call__ = real_call
    finally:
      mca.transformer_encoder = real
    out['%s:cfg' % tag] = np.array(json.dumps({'groups': list(groups), 'training': training, 'config': text}))
    for g in groups:
      if g == 'text':
        for i, (e, n) in enumerate(tensors['text']):
          out['%s:in:text%d' % (tag, i)], out['%s:in:len%d' % (tag, i)] = e, n
      else:
        out['%s:in:%s' % (tag, g)] = tensors[g]
    names = [k for k in mrl.VARS if k.startswith(tag + '::')]
    out['%s:names' % tag] = np.array(json.dumps([k.split('::', 1)[1] for k in names]))
    for k in names:
      out['%s:var:%s' % (tag, k.split('::', 1)[1])] = np.asarray(mrl.VARS[k], dtype=np.float64)
    out['%s:encoder' % tag] = np.asarray(seen['encoder'], dtype=np.float64)
    out['%s:cls' % tag] = np.asarray(seen['encoder'], dtype=np.float64)[:, 0, :]
    out['%s:hidden' % tag] = np.asarray(seen['hidden'], dtype=np.float64)
    out['%s:logits' % tag] = np.asarray(pred['logits'], dtype=np.float64)
    out['%s:probs' % tag] = np.asarray(pred['probs'], dtype=np.float64)
    print(tag, 'encoder', out['%s:encoder' % tag].shape, 'variables', len(names))
  path = os.path.join(HERE, 'uniter_vectors.npz')
  np.savez_compressed(path, **out)
  print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
