"""fp64 torch restatement of the reference's BERT-style encoder (easy_rec/python/layers/multihead_cross_attention.py:
attention_layer, transformer_encoder, embedding_postprocessor, layer_norm) and of Uniter's forward up to the [CLS]
feature (layers/uniter.py), formula by formula, for the tests of easyrec_amd/layers/multihead_cross_attention.py,
layers/uniter.py and the K8f kernels, and for the model oracle (oracle/model_oracle.py).  The helpers those tests share
that build the product (configs, the reference fixture's cases) are tests/_uniter_cases.py.  `params` maps the
reference's variable names to fp64 tensors; everything is differentiable by autograd."""
import math

import torch

LN_EPSILON = 1e-12


def attention_core(q, k, v, to_mask, B, F, T, H, ds):
  """:179-243: q [B * F, H ds], k, v [B * T, H ds], to_mask [B, T] (1 attend) or [B, F, T] or None -> [B * F, H ds]."""
  q4 = q.reshape(B, F, H, ds).permute(0, 2, 1, 3)
  k4 = k.reshape(B, T, H, ds).permute(0, 2, 1, 3)
  v4 = v.reshape(B, T, H, ds).permute(0, 2, 1, 3)
  scores = torch.matmul(q4, k4.transpose(-1, -2)) * (1.0 / math.sqrt(float(ds)))
  if to_mask is not None:
    m = to_mask.to(scores.dtype)
    m = m[:, None, None, :] if m.dim() == 2 else m[:, None, :, :]
    scores = scores + (1.0 - m) * -10000.0
  probs = torch.softmax(scores, dim=-1)
  return torch.matmul(probs, v4).permute(0, 2, 1, 3).reshape(B * F, H * ds)


def add_layer_norm(x, res, gamma, beta, eps=LN_EPSILON):
  """compat/layers.py layer_norm over the last axis of x + res (res broadcasts from the left)."""
  z = x if res is None else x + res
  mean = z.mean(dim=-1, keepdim=True)
  var = ((z - mean) ** 2).mean(dim=-1, keepdim=True)
  return (z - mean) * torch.rsqrt(var + eps) * gamma + beta


def dense(x, params, name, act=None):
  y = x @ params[name + '/kernel'] + params[name + '/bias']
  return y if act is None else act(y)


def gelu(x):
  return x * 0.5 * (1.0 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * torch.pow(x, 3))))


ACTIVATIONS = {'gelu': gelu, 'tanh': torch.tanh, 'relu': torch.relu, 'swish': lambda x: x * torch.sigmoid(x)}


def attention_layer(from_2d, to_2d, params, scope, to_mask, B, F, T, H, ds):
  q = dense(from_2d, params, scope + '/query')
  k = dense(to_2d, params, scope + '/key')
  v = dense(to_2d, params, scope + '/value')
  return attention_core(q, k, v, to_mask, B, F, T, H, ds)


def encoder_variable_names(name, layers):
  out = []
  for i in range(layers):
    p = '%s_layer_%d' % (name, i)
    for dn in ('attention/self/query', 'attention/self/key', 'attention/self/value', 'attention/output/dense'):
      out += ['%s/%s/kernel' % (p, dn), '%s/%s/bias' % (p, dn)]
    out += ['%s/attention/output/LayerNorm/beta' % p, '%s/attention/output/LayerNorm/gamma' % p]
    out += ['%s/intermediate/dense/kernel' % p, '%s/intermediate/dense/bias' % p]
    out += ['%s/output/dense/kernel' % p, '%s/output/dense/bias' % p]
    out += ['%s/output/LayerNorm/beta' % p, '%s/output/LayerNorm/gamma' % p]
  return out


def transformer_encoder(x, to_mask, params, name, layers, H, act='gelu', scope=''):
  """:246-369: x [B, S, hidden] -> [B, S, hidden]; to_mask [B, S] or None."""
  B, S, hidden = x.shape
  ds = hidden // H
  prev = x.reshape(B * S, hidden)
  for i in range(layers):
    p = '%s%s_layer_%d' % (scope, name, i)
    att = attention_layer(prev, prev, params, p + '/attention/self', to_mask, B, S, S, H, ds)
    att = dense(att, params, p + '/attention/output/dense')
    att = add_layer_norm(att, prev, params[p + '/attention/output/LayerNorm/gamma'],
                         params[p + '/attention/output/LayerNorm/beta'])
    mid = dense(att, params, p + '/intermediate/dense', ACTIVATIONS[act] if isinstance(act, str) else act)
    out = dense(mid, params, p + '/output/dense')
    prev = add_layer_norm(out, att, params[p + '/output/LayerNorm/gamma'], params[p + '/output/LayerNorm/beta'])
  return prev.reshape(B, S, hidden)


def embedding_postprocessor(x, params, ln_name, token_type_ids=None, token_type_table=None, position_table=None):
  """:665-769: x [B, S, W]; token_type_ids [S] or [B, S] int64 with the table's name; position_table: its name."""
  B, S, W = x.shape
  out = x
  if token_type_ids is not None:
    out = out + params[token_type_table][token_type_ids]
  if position_table is not None:
    out = out + params[position_table][:S]
  return add_layer_norm(out, None, params[ln_name + '/gamma'], params[ln_name + '/beta'])


def random_encoder_params(name, layers, hidden, intermediate, seed, scale=0.3):
  """Variables of transformer_encoder with non-trivial biases, gammas and betas."""
  g = torch.Generator().manual_seed(seed)
  params = {}
  for n in encoder_variable_names(name, layers):
    if n.endswith('/kernel'):
      din = intermediate if '/output/dense/kernel' in n and '/attention/' not in n else hidden
      dout = intermediate if '/intermediate/' in n else hidden
      params[n] = torch.randn(din, dout, generator=g, dtype=torch.float64) * scale / math.sqrt(din)
    elif n.endswith('/gamma'):
      params[n] = 1.0 + 0.2 * torch.randn(hidden, generator=g, dtype=torch.float64)
    else:
      width = intermediate if '/intermediate/' in n else hidden
      params[n] = 0.1 * torch.randn(width, generator=g, dtype=torch.float64)
  return params


def mixed_mask(B, T, seed):
  """A to-mask [B, T] int32: random keys, example 0 with a single open key, example 1 with every key masked."""
  m = (torch.rand(B, T, generator=torch.Generator().manual_seed(seed)) < 0.7).to(torch.int32)
  m[:, 0] = 1
  m[0] = 0
  m[0, T // 2] = 1
  if B > 1:
    m[1] = 0
  return m


def grad_floor(name, ref_grads):
  """The floor of a gradient's scale in a comparison: None, except for a key bias.  A key bias shifts every score of a
  row alike, so its gradient (the column sums of dK) is zero up to rounding; it is held at the scale of its key
  kernel's gradient, the same rows of dK weighted by the layer's input."""
  if name.endswith('/key/bias'):
    return float(ref_grads[name[:-len('bias')] + 'kernel'].abs().max())
  return None


def uniter_token_types(has_image, has_general, n_text):
  """layers/uniter.py:66-72, :168, :235 -> (use_token_type, vocabulary size, image id, general id, [text ids]); n_image
  and the number of towers beyond these three do not change the numbering (one image feature assumed)."""
  start = 1 if has_image else 0
  text0 = start + (1 if has_general else 0)
  use = (int(has_image) + int(has_general) + int(n_text > 0)) > 1 or n_text > 1
  return use, n_text + int(has_image) + int(has_general), 0, start, [text0 + i for i in range(n_text)]


def uniter_cls(params, c, img, general, seqs):
  """layers/uniter.py:128-286 up to the [CLS] feature, in the dtype of the inputs.  c: the uniter tower config; img
  [B, n_img, raw_dim] or None; general [B, n_general, dim] or None; seqs: [(embedding [B, L, dim], lengths [B])] per
  text feature.  Tokens [CLS | image | general | text ..]; embedding_postprocessor per tower with LayerNorm,
  LayerNorm_1, .. in call order; the to-mask ones except position >= length of a text feature.  -> [B, hidden]"""
  hidden = c.hidden_size
  use_tt, _, img_id, gen_id, txt_ids = uniter_token_types(img is not None, general is not None, len(seqs))
  tt = 'token_type/token_type_embeddings'
  ln = iter(['LayerNorm'] + ['LayerNorm_%d' % i for i in range(1, 8)])
  tokens, masks = [], []

  def post(x, type_id, position_table):
    S = x.shape[1]
    ids = torch.full((S,), type_id, dtype=torch.int64) if use_tt else None
    return embedding_postprocessor(x, params, next(ln), ids, tt if use_tt else None,
                                   position_table if c.use_position_embeddings else None)

  if img is not None:
    B = img.shape[0]
    if img.shape[-1] != hidden:
      img = dense(img.reshape(-1, img.shape[-1]), params, 'img_projection').reshape(B, -1, hidden)
    tokens.append(post(img, img_id, 'position_embedding/img_position_embeddings'))
    masks.append(torch.ones(B, img.shape[1], dtype=torch.int64))
  if general is not None:
    B = general.shape[0]
    if general.shape[-1] != hidden:
      general = dense(general.reshape(-1, general.shape[-1]), params, 'txt_projection').reshape(B, -1, hidden)
    S = general.shape[1]
    ids = torch.full((S,), gen_id, dtype=torch.int64) if use_tt else None
    tokens.append(embedding_postprocessor(general, params, next(ln), ids, tt if use_tt else None, None))
    masks.append(torch.ones(B, S, dtype=torch.int64))
  for i, (e, lens) in enumerate(seqs):
    B, L, emb = e.shape
    if emb != hidden:
      e = dense(e.reshape(-1, emb), params, 'txt_seq_projection_%d' % i).reshape(B, L, hidden)
    tokens.append(post(e, txt_ids[i], 'position_embedding/txt_position_embeddings_%d' % i))
    masks.append((torch.arange(L)[None, :] < torch.as_tensor(lens).reshape(-1, 1)).to(torch.int64))
  B = tokens[0].shape[0]
  cls = params['cls_emb'].expand(B, 1, hidden)
  x = torch.cat([cls] + tokens, dim=1)
  mask = torch.cat([torch.ones(B, 1, dtype=torch.int64)] + masks, dim=1)
  out = transformer_encoder(x, mask, params, 'uniter', c.num_hidden_layers, c.num_attention_heads, c.hidden_act)
  return out[:, 0, :]
