"""UNITER's multi-modal layer (reference easy_rec/python/layers/uniter.py:14-301).

Feature groups: `image` (raw features of raw_input_dim, one token each, through `img_projection` when the width is not
hidden_size), `general` (embedded features, one token each, through `txt_projection`), `text` (sequence features read
with is_combine=False, a token per position, through `txt_seq_projection_<i>`) and `other` (through
`other_feature_dnn`, beside the encoder).  The tokens [CLS | image | general | text_0 | text_1 ..] each pass
embedding_postprocessor (token-type rows when there is more than one tower or feature, position rows for image and
text) and then the transformer encoder `uniter`; the [CLS] row, concatenated with the `other` features, is the output.
Token-type ids (:66-72, :168, :235): image 0, general 1 (0 without an image group), then a consecutive id per text
feature; the table holds one row per text feature plus one each for an image and a general group.  The to-mask is ones
for [CLS], image and general tokens and position < length for each text feature.

The reference's assertions are ValueError at build time here, as are bf16 dense and the embedding-parallel engine (the
encoder's kernels are fp32, layers/multihead_cross_attention.py).
"""
import torch

from easyrec_amd.core import context
from easyrec_amd.layers import dnn
from easyrec_amd.layers import multihead_cross_attention as mca
from easyrec_amd.layers.sharded_embedding import ShardedEmbeddingEngine
from easyrec_amd.utils.activation import get_activation

GROUPS = ('image', 'general', 'text')


def _feature_name(feature_config):
  return feature_config.feature_name if feature_config.HasField('feature_name') else feature_config.input_names[0]


class Uniter(object):

  def __init__(self, model_config, feature_configs, features, uniter_config, input_layer):
    self._model_config = uniter_config
    self._features = features
    self._input_layer = input_layer
    ctx = context.current()
    if getattr(ctx, 'dense_dtype', 'f32') == 'bf16':
      raise ValueError('Uniter: dense_dtype bf16 is not supported (the encoder kernels are fp32)')
    if isinstance(ctx.engine, ShardedEmbeddingEngine):
      raise ValueError('Uniter: embedding-parallel training of a Uniter model is not supported')
    self._has = {g: input_layer.has_group(g) for g in GROUPS + ('other',)}
    tower_num = sum(self._has.values())
    if tower_num == 0:
      raise ValueError('there must be one of the feature groups: [image, text, general, other]')
    names = {g: [] for g in GROUPS}
    for fea_group in model_config.feature_groups:
      if fea_group.group_name in names:
        names[fea_group.group_name] = list(fea_group.feature_names)
        if len(set(fea_group.feature_names)) != len(fea_group.feature_names):
          raise ValueError('there are duplicate features in `%s` feature group' % fea_group.group_name)
    self._img_feature_num = len(names['image'])
    self._general_feature_num = len(names['general'])
    self._txt_feature_num = len(names['text'])
    self._use_token_type = sum(self._has[g] for g in GROUPS) > 1 or self._txt_feature_num > 1 or self._img_feature_num > 1
    self._token_type_vocab_size = self._txt_feature_num + (self._img_feature_num > 0) + (self._general_feature_num > 0)
    dims = {g: [] for g in GROUPS}
    max_seq_len = 0
    for fc in feature_configs:
      name = _feature_name(fc)
      if name in names['image']:
        dims['image'].append(fc.raw_input_dim)
      if name in names['general']:
        dims['general'].append(fc.embedding_dim)
      if name in names['text']:
        dims['text'].append(fc.embedding_dim)
        if fc.HasField('max_seq_len'):
          if fc.max_seq_len <= 0:
            raise ValueError('feature config `max_seq_len` must be greater than 0 for feature: ' + name)
          max_seq_len = max(max_seq_len, fc.max_seq_len)
    for g in GROUPS:
      if len(set(dims[g])) > 1 or len(dims[g]) != len(names[g]):
        raise ValueError('Uniter requires that all `%s` feature dimensions must be consistent.' % g)
    if self._txt_feature_num > 0 and uniter_config.use_position_embeddings:
      if uniter_config.max_position_embeddings <= 0:
        raise ValueError('model config `max_position_embeddings` must be greater than 0.')
      if uniter_config.max_position_embeddings < max_seq_len:
        raise ValueError('model config `max_position_embeddings` must be greater than or equal to the maximum of all '
                         'feature config `max_seq_len`, which is %d' % max_seq_len)
    self._img_emb_size = dims['image'][0] if dims['image'] else 0
    self._general_emb_size = dims['general'][0] if dims['general'] else 0
    if self._has['image'] and self._img_emb_size <= 0:
      raise ValueError('`image` feature dimensions must be greater than 0, set by `raw_input_dim`')

  def token_type_ids(self):
    """{'image': id, 'general': id, 'text': [id per text feature]} as the reference numbers them."""
    start = 1 if self._img_feature_num > 0 else 0
    text0 = start + (1 if self._has['general'] else 0)
    return {'image': 0, 'general': start, 'text': [text0 + i for i in range(self._txt_feature_num)]}

  def _post(self, x, token_type_id, hidden_dropout, use_position, position_name='position_embeddings'):
    c = self._model_config
    return mca.embedding_postprocessor(
        x, use_token_type=self._use_token_type, token_type_ids=token_type_id,
        token_type_vocab_size=self._token_type_vocab_size, use_position_embeddings=use_position,
        max_position_embeddings=c.max_position_embeddings, position_embedding_name=position_name,
        dropout_prob=hidden_dropout)

  def __call__(self, is_training, *args, **kwargs):
    c = self._model_config
    hidden_dropout = c.hidden_dropout_prob if is_training else 0.0
    att_dropout = c.attention_probs_dropout_prob if is_training else 0.0
    hidden = c.hidden_size
    ids = self.token_type_ids()
    il, features = self._input_layer, self._features
    sub_modules = []
    with mca.default_scopes():
      tokens, masks = [], []
      if self._has['image']:
        img = il(features, 'image')[0]
        if self._img_emb_size != hidden:
          img = dnn.dense(img.reshape(-1, self._img_emb_size), hidden, 'img_projection')
        img = img.reshape(-1, self._img_feature_num, hidden)
        tokens.append(self._post(img, ids['image'], hidden_dropout, c.use_position_embeddings, 'img_position_embeddings'))
        masks.append(torch.ones(img.shape[0], self._img_feature_num, dtype=torch.int32, device=img.device))
      if self._has['general']:
        gen = il(features, 'general')[0]
        if self._general_emb_size != hidden:
          gen = dnn.dense(gen.reshape(-1, self._general_emb_size), hidden, 'txt_projection')
        gen = gen.reshape(-1, self._general_feature_num, hidden)
        tokens.append(self._post(gen, ids['general'], hidden_dropout, False))
        masks.append(torch.ones(gen.shape[0], self._general_feature_num, dtype=torch.int32, device=gen.device))
      if self._has['text']:
        seq_features = il(features, 'text', is_combine=False)[0]
        for i, (seq_fea, seq_len) in enumerate(seq_features):
          B, L, emb = seq_fea.shape
          if emb != hidden:
            seq_fea = dnn.dense(seq_fea.reshape(-1, emb), hidden, 'txt_seq_projection_%d' % i).reshape(B, L, hidden)
          tokens.append(self._post(seq_fea, ids['text'][i], hidden_dropout, c.use_position_embeddings,
                                   'txt_position_embeddings_%d' % i))
          pos = torch.arange(L, device=seq_fea.device, dtype=torch.int32)
          masks.append((pos[None, :] < seq_len.to(torch.int32)[:, None]).to(torch.int32))
      if tokens:
        B = tokens[0].shape[0]
        cls_emb = context.varstore().get_variable('cls_emb', (1, 1, hidden), 'glorot_uniform')
        all_fea = torch.cat([cls_emb.expand(B, 1, hidden)] + tokens, dim=1)
        input_mask = torch.cat([torch.ones(B, 1, dtype=torch.int32, device=all_fea.device)] + masks, dim=1)
        attention_mask = mca.create_attention_mask_from_input_mask(all_fea, input_mask)
        attention_fea = mca.transformer_encoder(
            all_fea, attention_mask, hidden_size=hidden, num_hidden_layers=c.num_hidden_layers,
            num_attention_heads=c.num_attention_heads, intermediate_size=c.intermediate_size,
            intermediate_act_fn=get_activation(c.hidden_act), hidden_dropout_prob=hidden_dropout,
            attention_probs_dropout_prob=att_dropout, initializer_range=c.initializer_range, name='uniter')
        sub_modules.append(attention_fea[:, 0, :])  # the [CLS] feature
      if self._has['other']:
        other = il(features, 'other')[0]
        if c.HasField('other_feature_dnn'):
          other = dnn.DNN(c.other_feature_dnn, kwargs.get('l2_reg', 0), 'other_dnn', is_training)(other)
        sub_modules.append(other)
    return sub_modules[0] if len(sub_modules) == 1 else torch.cat(sub_modules, dim=-1)
