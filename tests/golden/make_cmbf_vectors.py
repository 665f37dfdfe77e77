#!/usr/bin/env python
"""Golden vectors from the REFERENCE'S OWN CMBF: layers/cmbf.py, layers/multihead_cross_attention.py and model/cmbf.py
run unmodified, where a checkout of the reference is available, over the numpy `tensorflow` stand-in of
make_reference_layer_vectors.py as make_uniter_vectors.py extends it (its loader, `_extend`, layer_norm restatement,
stub input layer and bare RankModel are imported, not copied).

New stand-in pieces: tf.to_float; a tower's output compares by identity, as a TensorFlow tensor does.
tf.get_variable('img_map_matrix') is the stand-in's seeded normal.

Cases, each with B = 6, multi_head_num 2, text head size 4 x 2 heads, image head size 3 x 2 heads, cross head sizes 3
(image) and 4 (text), 2 text layers, 2 cross layers, all three dropouts 0, text lengths 1, 1 and max among the examples:
  all                   image (one embedding, image_self_attention_layer_num 2, image_feature_dim 5: img_projection and
                        img_map_matrix), general, text, other with its DNN; token types and positions
  img0                  image_self_attention_layer_num 0 with img_projection: one image token
  patches               image_feature_patch_num 3
  multi_image           two image features
  image_only, text_only one tower
  general_only          image + general, no sequences: the reshape branch of merge_text_embedding, no mask
  no_token_type_no_pos  use_token_type false, use_position_embeddings false
  other_plain           `other` without other_feature_dnn
  eval                  is_training False
Inputs, every variable under its TF name in creation order (`<tag>:names`: [name, shape] pairs; `<tag>:vars`: the
values end to end), both tower outputs, both cross outputs, the layer output,
logits and probs go to tests/golden/cmbf_vectors.npz (fp64).

usage: python tests/golden/make_cmbf_vectors.py [<reference checkout>]   (default: make_reference_layer_vectors.REF)
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_reference_layer_vectors as mrl  # noqa: E402
import make_uniter_vectors as mu  # noqa: E402

B, HEADS = 6, 2
IMG_DIM, GEN_N, GEN_DIM, TXT_DIM, TXT_LENS, OTHER_W = 9, 3, 5, 4, (5, 3), 6
ALL = ('image', 'general', 'text', 'other')
# tag -> (groups, overrides)
CASES = [
    ('all', ALL, {}),
    ('img0', ALL, {'image_layers': 0}),
    ('patches', ALL, {'patches': 3}),
    ('multi_image', ALL, {'n_image': 2}),
    ('image_only', ('image',), {}),
    ('text_only', ('general', 'text'), {}),
    ('general_only', ('image', 'general'), {}),
    ('no_token_type_no_pos', ALL, {'use_token_type': False, 'use_position_embeddings': False}),
    ('other_plain', ('image', 'general', 'text', 'other'), {'other_dnn': False}),
    ('eval', ALL, {'training': False}),
]


class _Identity(mrl._Tensor):
  """A tower's output: `None not in [image, text]` (layers/cmbf.py:342) compares TensorFlow tensors by identity, where
  numpy would compare element by element."""

  def __eq__(self, other):
    return self is other

  def __ne__(self, other):
    return self is not other

  __hash__ = object.__hash__


def load_cmbf():
  mca, _, _ = mu.load_uniter()
  tf = sys.modules['tensorflow']
  tf.to_float = lambda x: mrl._tensor(np.asarray(x).astype(np.float64))
  m = sys.modules['easy_rec.python.protos.cmbf_pb2'] = types.ModuleType('easy_rec.python.protos.cmbf_pb2')
  m.CMBF = object
  sys.modules['easy_rec.python.protos'].cmbf_pb2 = m
  layer = mrl.load_reference('easy_rec/python/layers/cmbf.py', 'easy_rec.python.layers.cmbf')
  sys.modules['easy_rec.python.layers.cmbf'] = layer
  sys.modules['easy_rec.python.layers'].cmbf = layer
  model = mrl.load_reference('easy_rec/python/model/cmbf.py', 'easy_rec.python.model.cmbf')
  return mca, layer, model


def case_config(groups, opts):
  """(EasyRecConfig, its text) of a case as this repository's protos (the reference reads the same fields)."""
  from google.protobuf import text_format
  from easyrec_amd.protos import pipeline_pb2
  n_image = opts.get('n_image', 1)
  feats = ["features { input_names: 'img%d' feature_type: RawFeature raw_input_dim: %d }" % (i, IMG_DIM)
           for i in range(n_image)]
  feats += ["features { input_names: 'g%d' feature_type: IdFeature embedding_dim: %d num_buckets: 10 }" % (i, GEN_DIM)
            for i in range(GEN_N)]
  feats += ["features { input_names: 't%d' feature_type: SequenceFeature embedding_dim: %d max_seq_len: %d "
            "hash_bucket_size: 50 }" % (i, TXT_DIM, L) for i, L in enumerate(TXT_LENS)]
  feats += ["features { input_names: 'o0' feature_type: RawFeature raw_input_dim: %d }" % OTHER_W]
  names = {'image': ['img%d' % i for i in range(n_image)], 'general': ['g%d' % i for i in range(GEN_N)],
           'text': ['t0', 't1'], 'other': ['o0']}
  fg = ' '.join("feature_groups { group_name: '%s' %s wide_deep: DEEP }" %
                (g, ' '.join("feature_names: '%s'" % n for n in names[g])) for g in groups)
  other = 'other_feature_dnn { hidden_units: 7 }' if ('other' in groups and opts.get('other_dnn', True)) else ''
  text = '''feature_config { %s }
    model_config { model_class: 'CMBF' %s
      cmbf { config { multi_head_num: %d image_multi_head_num: 2 text_multi_head_num: 2 text_head_size: 4
                      image_head_size: 3 image_feature_patch_num: %d image_feature_dim: 5
                      image_self_attention_layer_num: %d text_self_attention_layer_num: 2 cross_modal_layer_num: 2
                      image_cross_head_size: 3 text_cross_head_size: 4 hidden_dropout_prob: 0
                      attention_probs_dropout_prob: 0 use_token_type: %s use_position_embeddings: %s
                      max_position_embeddings: 6 text_seq_emb_dropout_prob: 0 %s }
             final_dnn { hidden_units: 8 hidden_units: 5 } } }''' % (
      ' '.join(feats), fg, HEADS, opts.get('patches', 1), opts.get('image_layers', 2),
      'true' if opts.get('use_token_type', True) else 'false',
      'true' if opts.get('use_position_embeddings', True) else 'false', other)
  return text_format.Parse(text, pipeline_pb2.EasyRecConfig()), text


def main():
  mca, layer_mod, model_mod = load_cmbf()
  rng = np.random.default_rng(2025)
  out = {}
  for tag, groups, opts in CASES:
    mrl.MODEL_SCOPE[0] = tag + '::'
    mu.LN_COUNTS.clear()
    cfg, text = case_config(groups, opts)
    lens = [np.array([1, 1, L, 2, L, 1][:B]) for L in TXT_LENS]
    tensors = {'image': rng.standard_normal((B, IMG_DIM * opts.get('n_image', 1))),
               'general': rng.standard_normal((B, GEN_N * GEN_DIM)), 'other': rng.standard_normal((B, OTHER_W)),
               'text': []}
    for L, n in zip(TXT_LENS, lens):
      e = rng.standard_normal((B, L, TXT_DIM))
      e[np.arange(L)[None, :] >= n[:, None]] = 0.0  # (padding rows of a sequence embedding are zero)
      tensors['text'].append((e, n))
    training = opts.get('training', True)
    seen = {}
    real_encoder, real_cross = mca.transformer_encoder, mca.cross_attention_tower

    def encoder(*a, **k):
      y = np.asarray(real_encoder(*a, **k)).view(_Identity)
      seen[{'image_self_attention': 'image_tower', 'text_self_attention': 'text_tower'}[k['name']]] = y
      return y

    def cross(*a, **k):
      seen['image_cross'], seen['text_cross'] = real_cross(*a, **k)
      return seen['image_cross'], seen['text_cross']

    mca.transformer_encoder, mca.cross_attention_tower = encoder, cross
    real_tower = layer_mod.CMBF.image_self_attention_tower

    def image_tower(self):
      y = real_tower(self)
      if y is not None:
        y = seen['image_tower'] = np.asarray(y).view(_Identity)  # (also the form without an encoder)
      return y

    real_call = layer_mod.CMBF.__call__

    def call(self, *a, **k):
      seen['hidden'] = real_call(self, *a, **k)
      return seen['hidden']

    layer_mod.CMBF.image_self_attention_tower, layer_mod.CMBF.__call__ = image_tower, call
    try:
      mc = cfg.model_config
      layer = layer_mod.CMBF(mc, list(cfg.feature_config.features), None, mc.cmbf.config,
                             mu.StubInputLayer(groups, tensors))
      model = object.__new__(model_mod.CMBF)
      model._cmbf_layer, model._is_training, model._l2_reg = layer, training, 0.0
      model._model_config, model._num_class, model._prediction_dict = mc.cmbf, 1, {}
      pred = model.build_predict_graph()
    finally:
      mca.transformer_encoder, mca.cross_attention_tower = real_encoder, real_cross
      layer_mod.CMBF.image_self_attention_tower, layer_mod.CMBF.__call__ = real_tower, real_call
    out['%s:cfg' % tag] = np.array(json.dumps({'groups': list(groups), 'training': training, 'config': text}))
    for g in groups:
      if g == 'text':
        for i, (e, n) in enumerate(tensors['text']):
          out['%s:in:text%d' % (tag, i)], out['%s:in:len%d' % (tag, i)] = e, n
      else:
        out['%s:in:%s' % (tag, g)] = tensors[g]
    names = [k for k in mrl.VARS if k.startswith(tag + '::')]
    # (one flat array per case: an npz entry per variable would cost more in zip headers than in values)
    out['%s:names' % tag] = np.array(json.dumps([[k.split('::', 1)[1], list(np.shape(mrl.VARS[k]))] for k in names]))
    out['%s:vars' % tag] = np.concatenate([np.asarray(mrl.VARS[k], dtype=np.float64).reshape(-1) for k in names])
    for k in ('image_tower', 'text_tower', 'image_cross', 'text_cross', 'hidden'):
      if k in seen:
        out['%s:%s' % (tag, k)] = np.asarray(seen[k], dtype=np.float64)
    out['%s:logits' % tag] = np.asarray(pred['logits'], dtype=np.float64)
    out['%s:probs' % tag] = np.asarray(pred['probs'], dtype=np.float64)
    print(tag, 'hidden', out['%s:hidden' % tag].shape, 'variables', len(names), sorted(seen))
  path = os.path.join(HERE, 'cmbf_vectors.npz')
  np.savez_compressed(path, **out)
  print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
