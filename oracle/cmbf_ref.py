"""fp64 torch restatement of the reference's cross-attention blocks (easy_rec/python/layers/multihead_cross_attention.py
:372-595) and of CMBF's forward (layers/cmbf.py), formula by formula on oracle/uniter_ref.py's pieces, for the tests of
easyrec_amd/layers/cmbf.py, model/cmbf.py and the grouped attention / segment mean kernels, and for the model oracle
(oracle/model_oracle.py).  The helpers those tests share that build the product (configs, the reference fixture's cases)
are tests/_cmbf_cases.py.  `params` maps the reference's variable names to fp64 tensors; everything is differentiable
by autograd."""
import numpy as np
import torch

from oracle import uniter_ref as ref


def _ln(x, res, params, scope):
  return ref.add_layer_norm(x, res, params[scope + '/LayerNorm/gamma'], params[scope + '/LayerNorm/beta'])


def cross_attention_block(from_tensor, to_tensor, params, prefix, cross_mask, self_mask, H, ds):
  """:372-485.  from_tensor [B, F, .], to_tensor [B, T, .]; cross_mask [B, T], self_mask [B, F] or None;
  prefix '<name>cross_layer_<i>' -> [B, F, H ds]."""
  B, F, T = from_tensor.shape[0], from_tensor.shape[1], to_tensor.shape[1]
  f2, t2 = from_tensor.reshape(B * F, -1), to_tensor.reshape(B * T, -1)
  cross = ref.attention_layer(f2, t2, params, prefix + '/attention/cross', cross_mask, B, F, T, H, ds)
  own = ref.attention_layer(cross, cross, params, prefix + '/attention/self', self_mask, B, F, F, H, ds)
  att = _ln(own, cross, params, prefix + '/attention/output')
  mid = ref.dense(att, params, prefix + '/intermediate/dense', torch.relu)
  out = ref.dense(mid, params, prefix + '/output/dense')
  return _ln(out, att, params, prefix + '/output').reshape(B, F, H * ds)


def cross_attention_tower(left, right, params, layers, H, left_ds, right_ds, right_mask, name=''):
  """:488-595 with left_input_mask None: both blocks of a layer read the previous layer's outputs."""
  for i in range(layers):
    new_left = cross_attention_block(left, right, params, '%sleft_to_right_cross_layer_%d' % (name, i), right_mask, None, H,
                                     left_ds)
    right = cross_attention_block(right, left, params, '%sright_to_left_cross_layer_%d' % (name, i), None, right_mask, H,
                                  right_ds)
    left = new_left
  return left, right


def cross_block_variable_names(prefix):
  out = []
  for att in ('cross', 'self'):
    for dn in ('query', 'key', 'value'):
      out += ['%s/attention/%s/%s/kernel' % (prefix, att, dn), '%s/attention/%s/%s/bias' % (prefix, att, dn)]
  out += ['%s/attention/output/LayerNorm/beta' % prefix, '%s/attention/output/LayerNorm/gamma' % prefix]
  out += ['%s/intermediate/dense/kernel' % prefix, '%s/intermediate/dense/bias' % prefix]
  out += ['%s/output/dense/kernel' % prefix, '%s/output/dense/bias' % prefix]
  out += ['%s/output/LayerNorm/beta' % prefix, '%s/output/LayerNorm/gamma' % prefix]
  return out


def cross_tower_variable_names(layers, name=''):
  out = []
  for i in range(layers):
    out += cross_block_variable_names('%sleft_to_right_cross_layer_%d' % (name, i))
    out += cross_block_variable_names('%sright_to_left_cross_layer_%d' % (name, i))
  return out


def grad_floor(name, ref_grads):
  """The floor of a gradient's scale in a comparison: uniter_ref.grad_floor (a key bias), and for the query and key
  projections of a cross_attention_block the scale of the same attention's VALUE kernel gradient.

  Why: the block has no residual from its input.  Its cross attention replaces every from-token by a convex mixture of
  the other side's value rows, so after a layer the tokens of a side nearly coincide (in the fixture's `all` case their
  spread is 3e-5 of their size; with ONE image token, T = 1, they coincide exactly).  With coinciding key and value
  rows the probabilities are uniform over the keys and dP = dctx V^T is constant along a row, so
  dS = P o (dP - rowsum(dP o P)) vanishes: the query and key gradients are zero up to the rounding of dP, whose size is
  |dctx| |V| - the quantities whose product with the layer's input IS the value kernel's gradient.  fp32 rounding of dP
  (2^-24 relative) therefore shows in dW_query and dW_key at about 1e-7 of dW_value's scale, whatever their own size
  (4e-9 of it in the `all` case).  A gradient held at 1e-4 of dW_value's scale is still held three orders of magnitude
  above that rounding."""
  floor = ref.grad_floor(name, ref_grads)
  parts = name.split('/')
  if 'cross_layer_' in name and len(parts) >= 4 and parts[-2] in ('query', 'key') and parts[-4] == 'attention':
    value = float(ref_grads['/'.join(parts[:-2] + ['value', 'kernel'])].abs().max())
    floor = max(floor or 0.0, value)
  return floor


def segment_mean(x, seg_begin, lens):
  """The pooling of merge_text_embedding / reduce_mean as a plain loop (numpy fp64): x [B, S, W], seg_begin n_seg + 1 ints,
  lens [B, n_seg] or None -> [B, n_seg, W]; len == 0 gives NaN (0 / 0)."""
  x = np.asarray(x, dtype=np.float64)
  B, S, W = x.shape
  n_seg = len(seg_begin) - 1
  out = np.zeros((B, n_seg, W))
  for b in range(B):
    for s in range(n_seg):
      width = seg_begin[s + 1] - seg_begin[s]
      n = width if lens is None else min(max(int(lens[b][s]), 0), width)
      acc = np.zeros(W)
      for t in range(n):
        acc = acc + x[b, seg_begin[s] + t]
      with np.errstate(invalid='ignore', divide='ignore'):
        out[b, s] = acc / np.float64(n)
  return out


def cmbf_towers(params, c, img, n_img, general, seqs):
  """layers/cmbf.py:133-378 in the dtype of the inputs.  c: the CMBF tower config; img [B, n_img * raw_dim] or None;
  general [B, n_general, dim] or None; seqs [(embedding [B, L, dim], lengths [B])] -> dict with image_tower, text_tower,
  image_cross, text_cross (where they exist) and `fused`, the pooled features side by side (without `other`)."""
  H = c.multi_head_num
  out = {}
  img_fea = None
  if img is not None:
    B = img.shape[0]
    raw = img.shape[1] // n_img
    if c.image_self_attention_layer_num <= 0:
      hidden = H * c.image_cross_head_size
      x = img.reshape(-1, raw)
      if raw != hidden:
        x = ref.dense(x, params, 'img_projection')
      img_fea = x.reshape(B, n_img, hidden)
    else:
      hidden = c.image_head_size * c.image_multi_head_num
      if n_img > 1:
        x = img.reshape(-1, raw)
        if raw != hidden:
          x = ref.dense(x, params, 'img_projection')
        x = x.reshape(B, n_img, hidden)
      elif c.image_feature_patch_num > 1:
        emb = raw // c.image_feature_patch_num
        x = img.reshape(-1, emb)
        if emb != hidden:
          x = ref.dense(x, params, 'img_projection')
        x = x.reshape(B, c.image_feature_patch_num, hidden)
      else:
        x = img
        if c.image_feature_dim != raw:
          x = ref.dense(x, params, 'img_projection')
        x = x.unsqueeze(-1) * params['img_map_matrix']
      img_fea = ref.transformer_encoder(x, None, params, 'image_self_attention', c.image_self_attention_layer_num, H)
    out['image_tower'] = img_fea
  hidden = c.text_head_size * c.text_multi_head_num
  tokens, masks = [], []
  if general is not None:
    B, n_gen = general.shape[0], general.shape[1]
    g = general
    if g.shape[-1] != hidden:
      g = ref.dense(g.reshape(-1, g.shape[-1]), params, 'txt_projection').reshape(B, n_gen, hidden)
    tokens.append(g)
    masks.append(torch.ones(B, n_gen, dtype=torch.int64))
  ln = iter(['LayerNorm'] + ['LayerNorm_%d' % i for i in range(1, 8)])
  for i, (e, lens) in enumerate(seqs):
    B, L, emb = e.shape
    if emb != hidden:
      e = ref.dense(e.reshape(-1, emb), params, 'txt_seq_projection_%d' % i).reshape(B, L, hidden)
    ids = torch.full((L,), i, dtype=torch.int64) if c.use_token_type else None
    tokens.append(ref.embedding_postprocessor(
        e, params, next(ln), ids, 'token_type/token_type_embeddings' if c.use_token_type else None,
        'position_embedding/position_embeddings_%d' % i if c.use_position_embeddings else None))
    masks.append((torch.arange(L)[None, :] < torch.as_tensor(lens).reshape(-1, 1)).to(torch.int64))
  txt_fea = mask = None
  if tokens:
    x = torch.cat(tokens, dim=1)
    mask = torch.cat(masks, dim=1) if seqs else None
    txt_fea = ref.transformer_encoder(x, mask, params, 'text_self_attention', c.text_self_attention_layer_num, H)
    out['text_tower'] = txt_fea

  def merge(t):
    B, S, W = t.shape
    if not seqs:
      return t.reshape(B, S * W)
    n_gen = 0 if general is None else general.shape[1]
    parts = [t[:, :n_gen, :]] if n_gen else []
    begin = n_gen
    for e, lens in seqs:
      L = e.shape[1]
      m = (torch.arange(L)[None, :] < torch.as_tensor(lens).reshape(-1, 1)).to(t.dtype).unsqueeze(-1)
      parts.append((t[:, begin:begin + L, :] * m).sum(dim=1, keepdim=True) / m.sum(dim=1, keepdim=True))
      begin += L
    return torch.cat(parts, dim=1).reshape(B, -1)

  if img_fea is not None and txt_fea is not None:
    left, right = cross_attention_tower(img_fea, txt_fea, params, c.cross_modal_layer_num, H, c.image_cross_head_size,
                                        c.text_cross_head_size, mask)
    out['image_cross'], out['text_cross'] = left, right
    out['fused'] = torch.cat([left.mean(dim=1), merge(right)], dim=-1)
  elif img_fea is not None:
    out['fused'] = img_fea.mean(dim=1)
  elif txt_fea is not None:
    out['fused'] = merge(txt_fea)
  return out


def dnn(x, params, name, units, training, eps=1e-3):
  """layers/dnn.py: per layer dense -> BatchNorm (the batch's statistics in training, the moving ones outside) -> relu."""
  for i in range(len(units)):
    scope = '%s/dnn_%d' % (name, i)
    x = ref.dense(x, params, scope)
    if training:
      mean, var = x.mean(dim=0), x.var(dim=0, unbiased=False)
    else:
      mean, var = params[scope + '/bn/moving_mean'], params[scope + '/bn/moving_variance']
    x = torch.relu((x - mean) / torch.sqrt(var + eps) * params[scope + '/bn/gamma'] + params[scope + '/bn/beta'])
  return x


def cmbf_model(params, cfg, inputs, training):
  """model/cmbf.py:39-47 over a fixture case's inputs -> (towers dict, layer output, logits)."""
  mc = cfg.model_config
  c = mc.cmbf.config
  towers = fixture_towers(cfg, inputs, params)
  parts = [towers['fused']] if 'fused' in towers else []
  if 'other' in inputs:
    other = inputs['other']
    if c.HasField('other_feature_dnn'):
      other = dnn(other, params, 'other_dnn', c.other_feature_dnn.hidden_units, training)
    parts.append(other)
  hidden = torch.cat(parts, dim=-1)
  x = dnn(hidden, params, 'final_dnn', mc.cmbf.final_dnn.hidden_units, training)
  return towers, hidden, ref.dense(x, params, 'output').squeeze(1)


def fixture_towers(cfg, inputs, var):
  """cmbf_towers over a fixture case's inputs."""
  mc = cfg.model_config
  n_img = len([g for g in mc.feature_groups if g.group_name == 'image'][0].feature_names) if 'image' in inputs else 0
  gen = inputs['general'].reshape(inputs['general'].shape[0], 3, -1) if 'general' in inputs else None
  return cmbf_towers(var, mc.cmbf.config, inputs.get('image'), n_img, gen, inputs.get('text', []))
