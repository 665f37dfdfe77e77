"""The BERT-style transformer encoder of the reference's multi-modal models (reference
easy_rec/python/layers/multihead_cross_attention.py): `attention_layer` (:42-243), `transformer_encoder` (:246-369),
`embedding_postprocessor` (:665-769), `create_attention_mask_from_input_mask` (:631-662) and `layer_norm` (:598-601);
`cross_attention_block` (:372-485) and `cross_attention_tower` (:488-595) of CMBF, and `segment_mean`, the pooling CMBF
ends with (layers/cmbf.py:292-326, :364).

Variables, as the reference's TF1 graph names them under the caller's scope (tf.layers.dense with bias, kernels
truncated normal with stddev `initializer_range`, biases zeros; compat/layers.py layer_norm: beta zeros, gamma ones,
epsilon 1e-12):
  <name>_layer_<i>/attention/self/{query,key,value}/{kernel,bias}
  <name>_layer_<i>/attention/output/dense/{kernel,bias}, <name>_layer_<i>/attention/output/LayerNorm/{beta,gamma}
  <name>_layer_<i>/intermediate/dense/{kernel,bias}
  <name>_layer_<i>/output/dense/{kernel,bias}, <name>_layer_<i>/output/LayerNorm/{beta,gamma}
  token_type/<token_type_embedding_name>, position_embedding/<position_embedding_name>
  <name>{left_to_right,right_to_left}_cross_layer_<i>/attention/{cross,self}/{query,key,value}/{kernel,bias},
  .../attention/output/LayerNorm/{beta,gamma}, .../intermediate/dense, .../output/dense, .../output/LayerNorm
  LayerNorm, LayerNorm_1, .. for a layer_norm without a name, in call order within `default_scopes()`.

Which path runs is decided by what the code can see.  On the HIP backend, with fp32 tensors on the GPU and a shape
inside the kernels' envelope (fits / LN_MAX_WIDTH below, the formulas of include/easyrec_hip.h K8f), the attention
between the projections and the output dense is one launch each way (kernels.MhaAttnFn), the projections that share an
input are one contraction on a packed operand (kernels.MhaProjFn), and every add & LayerNorm is one launch each way
(kernels.AddLayerNormFn).  A caller that passes group_units=True (CMBF's towers and blocks) gets the grouped-unit attention
launch (kernels.MhaGroupAttnFn: several (example, head) units per workgroup, the same result bits) wherever
mha_group_units(F, T, ds) >= 2, unless EASYREC_AMD_MHA_GROUP_UNITS=0.  Anywhere else - a stand-in backend on the CPU, a shape outside the envelope, a mask that
differs between query rows or is floating point (the kernels take int32 0 / 1 masks), projection activations,
attention dropout while training, EASYREC_AMD_FUSED_MHA=0 - the same function is composed of torch ops between the
same dense layers.

Both paths apply the mask's adder (1 - mask) * -10000 relative to the row's largest adder.  Softmax ignores a shift of
the whole row, so with any open key this is the reference's formula; with every key masked the row is the softmax of
the scores themselves, where s - 10000 in fp32 would round them to multiples of 2^-10 first.

Dropout is torch.nn.functional.dropout (as layers/dnn.py): parity with TensorFlow holds in distribution only.
"""
import contextlib
import math
import os
import threading

import torch

from easyrec_amd import kernels
from easyrec_amd.core import context
from easyrec_amd.core.variables import truncated_normal
from easyrec_amd.layers import dnn
from easyrec_amd.utils.activation import gelu

LN_EPSILON = 1e-12     # compat/layers.py:144
LDS_BUDGET = 81920     # bytes per workgroup of the attention kernels (csrc/er_mha.hip)
MAX_HEAD_SIZE = 128
MAX_SEQ_LEN = 4096     # from- and to-length bound of the attention kernels (mha_shape_ok)
LN_MAX_WIDTH = 4096
MASK_ADDER = -10000.0
GROUP_UNITS_DEFAULT = '1'  # (the grouped launches measured faster at every CMBF shape: DESIGN.md 3.17)
SEGMENT_MEAN_MAX = 4096  # W and S bound of er_segment_mean; at most 64 segments


# ------------------------------------------------------------------------------------------------ the kernels' envelope
def lds_bytes(from_len, to_len, head_size, bwd=True):
  """er_mha_lds_bytes: Q (and dctx) rows, K and V rows at the odd pitch odd(ds); P (and dS) at odd(T); the keys' adders."""
  if from_len < 1 or to_len < 1 or head_size < 1:
    return 0
  ld, ldp = head_size | 1, to_len | 1
  if bwd:
    return 4 * ((2 * from_len + 2 * to_len) * ld + 2 * from_len * ldp + to_len)
  return 4 * ((from_len + 2 * to_len) * ld + from_len * ldp + to_len)


def fits(from_len, to_len, head_size):
  return (1 <= from_len <= MAX_SEQ_LEN and 1 <= to_len <= MAX_SEQ_LEN and 1 <= head_size <= MAX_HEAD_SIZE and
          lds_bytes(from_len, to_len, head_size) <= LDS_BUDGET)


def mha_group_units(from_len, to_len, head_size):
  """er_mha_group_units: (example, head) units per workgroup of the grouped attention launches: the largest of 8, 4, 2
  whose backward LDS regions fit the budget side by side; 1 when only one fits; 0 outside the envelope."""
  if not fits(from_len, to_len, head_size):
    return 0
  unit = lds_bytes(from_len, to_len, head_size)
  for g in (8, 4, 2):
    if g * unit <= LDS_BUDGET:
      return g
  return 1


def group_units_enabled():
  """EASYREC_AMD_MHA_GROUP_UNITS=0: callers that ask for the grouped launches get the one-unit launches (the same
  result bits either way; the A/B switch of er_mha_group_*)."""
  return os.environ.get('EASYREC_AMD_MHA_GROUP_UNITS', GROUP_UNITS_DEFAULT) != '0'


def fused_enabled():
  """EASYREC_AMD_FUSED_MHA=0: the torch composition everywhere (the A/B switch of the K8f kernels)."""
  return os.environ.get('EASYREC_AMD_FUSED_MHA', '1') != '0'


def _fused(x):
  return fused_enabled() and x.is_cuda and x.dtype == torch.float32 and isinstance(kernels.hip(), kernels.HipBackend)


def _grads_of(params):
  # (the variables' slices of the flat gradient buffer; None in the build pass, before VarStore.pack)
  return [p.grad for p in params] if all(p.grad is not None for p in params) else None


def create_initializer(initializer_range=0.02):
  return lambda shape, rng: truncated_normal(shape, rng, 0.0, initializer_range)


def dropout(input_tensor, dropout_prob):
  """dropout_prob: the probability of DROPPING a value; only while training."""
  if dropout_prob is None or dropout_prob == 0.0 or not context.current().is_training:
    return input_tensor
  return torch.nn.functional.dropout(input_tensor, p=dropout_prob, training=True)


# ------------------------------------------------------------------------------------------------ default-scoped names
_TLS = threading.local()


@contextlib.contextmanager
def default_scopes():
  """One forward pass of a model: layer_norm calls without a name are numbered LayerNorm, LayerNorm_1, .. per enclosing
  variable scope in call order, as tf.variable_scope(None, default_name='LayerNorm') does while the graph is built."""
  prev = getattr(_TLS, 'counts', None)
  _TLS.counts = {}
  try:
    yield
  finally:
    _TLS.counts = prev


def _default_name(vs, base):
  counts = getattr(_TLS, 'counts', None)
  if counts is None:
    return base
  key = vs.full_name(base)
  n = counts.get(key, 0)
  counts[key] = n + 1
  return base if n == 0 else '%s_%d' % (base, n)


# ------------------------------------------------------------------------------------------------ add & LayerNorm
def add_layer_norm_compose(x, res, gamma, beta):
  """LN(x + res) op by op: the variance as the mean of squared differences (tf.nn.moments)."""
  z = x if res is None else x + res
  mean = z.mean(dim=-1, keepdim=True)
  diff = z - mean
  var = (diff * diff).mean(dim=-1, keepdim=True)
  return diff * torch.rsqrt(var + LN_EPSILON) * gamma + beta


def layer_norm(input_tensor, name=None, residual=None):
  """Layer normalisation over the last dimension of input_tensor (+ residual).  residual: the same shape, or [S, W]
  against an input [B, S, W] (a per-position addend)."""
  vs = context.varstore()
  name = name or _default_name(vs, 'LayerNorm')
  W = int(input_tensor.shape[-1])
  beta = vs.get_variable(name + '/beta', (W,), 'zeros')
  gamma = vs.get_variable(name + '/gamma', (W,), 'ones')
  if _fused(input_tensor) and 1 <= W <= LN_MAX_WIDTH and input_tensor.numel() > 0:
    shape = input_tensor.shape
    res = None if residual is None else residual.reshape(-1, W)
    y = kernels.AddLayerNormFn.apply(input_tensor.reshape(-1, W), res, gamma, beta, LN_EPSILON, _grads_of([gamma, beta]))
    return y.reshape(shape)
  if residual is not None and residual.numel() == input_tensor.numel():
    residual = residual.reshape(input_tensor.shape)
  return add_layer_norm_compose(input_tensor, residual, gamma, beta)


def layer_norm_and_dropout(input_tensor, dropout_prob, name=None, residual=None):
  return dropout(layer_norm(input_tensor, name, residual=residual), dropout_prob)


# ------------------------------------------------------------------------------------------------ attention
def create_attention_mask_from_input_mask(from_tensor, to_mask):
  """to_mask [B, T] (1 attend, 0 masked) -> [B, F, T]: every query row of an example sees the same keys.  The result
  is a broadcast VIEW (stride 0 over F) that keeps to_mask's dtype (the reference casts to float; the consumers here
  cast where they add).  attention_layer recognises the view and hands an INTEGER mask to the kernels as [B, T]."""
  B, F = int(from_tensor.shape[0]), int(from_tensor.shape[1])
  assert to_mask.dim() == 2 and to_mask.shape[0] == B
  return to_mask.unsqueeze(1).expand(B, F, to_mask.shape[1])


def _row_mask(attention_mask, B, F, T):
  """The [B, T] mask behind a [B, F, T] mask that is the same for every query row (a broadcast view), else None."""
  if attention_mask.dim() == 2 and tuple(attention_mask.shape) == (B, T):
    return attention_mask
  if tuple(attention_mask.shape) == (B, F, T) and (F == 1 or attention_mask.stride(1) == 0):
    return attention_mask[:, 0, :]
  return None


def attention_compose(q, k, v, mask, B, F, T, H, ds, dropout_prob=0.0):
  """The attention between the projections and the output dense, op by op: q [B * F, H ds], k, v [B * T, H ds], mask
  None, [B, T] or [B, F, T] -> [B * F, H ds]."""
  q4 = q.reshape(B, F, H, ds).permute(0, 2, 1, 3)
  k4 = k.reshape(B, T, H, ds).permute(0, 2, 1, 3)
  v4 = v.reshape(B, T, H, ds).permute(0, 2, 1, 3)
  scores = torch.matmul(q4, k4.transpose(-1, -2)) * (1.0 / math.sqrt(float(ds)))
  if mask is not None:
    m3 = mask.unsqueeze(1) if mask.dim() == 2 else mask  # [B, 1 or F, T]
    adder = (1.0 - m3.to(scores.dtype)) * MASK_ADDER
    adder = adder - adder.max(dim=-1, keepdim=True).values
    scores = scores + adder.unsqueeze(1)
  probs = dropout(torch.softmax(scores, dim=-1), dropout_prob)
  return torch.matmul(probs, v4).permute(0, 2, 1, 3).reshape(B * F, H * ds)


def attention_layer(from_tensor, to_tensor, size_per_head, num_attention_heads=1, attention_mask=None, query_act=None,
                    key_act=None, value_act=None, attention_probs_dropout_prob=0.0, initializer_range=0.02,
                    do_return_2d_tensor=False, batch_size=None, from_seq_length=None, to_seq_length=None, reuse=None,
                    group_units=False):
  """Multi-headed attention from from_tensor to to_tensor ([B, F, W] / [B, T, W], or 2-D with batch_size and the two
  lengths given); the same tensor object for both is self-attention.  attention_mask: [B, F, T] (or [B, T]), 1 attend.
  group_units: on the fused path, take the grouped-unit launch where two or more units fit a workgroup."""
  if from_tensor.dim() != to_tensor.dim():
    raise ValueError('The rank of `from_tensor` must match the rank of `to_tensor`.')
  if from_tensor.dim() == 3:
    batch_size, from_seq_length, to_seq_length = from_tensor.shape[0], from_tensor.shape[1], to_tensor.shape[1]
  elif batch_size is None or from_seq_length is None or to_seq_length is None:
    raise ValueError('When passing in rank 2 tensors to attention_layer, the values for `batch_size`, '
                     '`from_seq_length`, and `to_seq_length` must all be specified.')
  B, F, T, H, ds = int(batch_size), int(from_seq_length), int(to_seq_length), int(num_attention_heads), int(size_per_head)
  d = H * ds
  self_attention = from_tensor is to_tensor
  from_2d = from_tensor.reshape(-1, from_tensor.shape[-1])
  to_2d = from_2d if self_attention else to_tensor.reshape(-1, to_tensor.shape[-1])
  vs = context.varstore()
  init = create_initializer(initializer_range)
  ws, bs = [], []
  for name, src in (('query', from_2d), ('key', to_2d), ('value', to_2d)):
    ws.append(vs.get_variable(name + '/kernel', (int(src.shape[-1]), d), init))
    bs.append(vs.get_variable(name + '/bias', (d,), 'zeros'))
  ctx = context.current()
  drop = attention_probs_dropout_prob if ctx.is_training else 0.0
  row_mask = None if attention_mask is None else _row_mask(attention_mask, B, F, T)
  fused = (_fused(from_2d) and fits(F, T, ds) and not drop and query_act is None and key_act is None and
           value_act is None and B * F > 0 and
           # (the kernels read an int32 0 / 1 mask: a floating mask may hold other weights and stays with the composition)
           (attention_mask is None or (row_mask is not None and not row_mask.is_floating_point())))
  if fused:
    to_mask = None if row_mask is None else row_mask.to(torch.int32).contiguous()
    grouped = group_units and group_units_enabled() and mha_group_units(F, T, ds) >= 2
    attn = kernels.MhaGroupAttnFn if grouped else kernels.MhaAttnFn
    if self_attention:
      qkv = kernels.MhaProjFn.apply(from_2d, _grads_of(ws + bs), 3, *(ws + bs))
      out = attn.apply(qkv, None, to_mask, B, F, T, H, ds)
    else:
      q = dnn.dense(from_2d, d, 'query', kernel_initializer=init)
      kv_params = ws[1:] + bs[1:]
      kv = kernels.MhaProjFn.apply(to_2d, _grads_of(kv_params), 2, *kv_params)
      out = attn.apply(q, kv, to_mask, B, F, T, H, ds)
  else:
    q = dnn.dense(from_2d, d, 'query', kernel_initializer=init)
    k = dnn.dense(to_2d, d, 'key', kernel_initializer=init)
    v = dnn.dense(to_2d, d, 'value', kernel_initializer=init)
    q = q if query_act is None else query_act(q)
    k = k if key_act is None else key_act(k)
    v = v if value_act is None else value_act(v)
    mask = attention_mask if row_mask is None else row_mask
    out = attention_compose(q, k, v, mask, B, F, T, H, ds, drop)
  return out if do_return_2d_tensor else out.reshape(B, F, d)


def transformer_encoder(input_tensor, attention_mask=None, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                        intermediate_size=3072, intermediate_act_fn=gelu, hidden_dropout_prob=0.0,
                        attention_probs_dropout_prob=0.0, initializer_range=0.02, reuse=None, name='transformer',
                        group_units=False):
  """input_tensor [B, S, hidden_size] -> the last layer's [B, S, hidden_size].  group_units: see attention_layer."""
  if hidden_size % num_attention_heads != 0:
    raise ValueError('The hidden size (%d) is not a multiple of the number of attention heads (%d)' %
                     (hidden_size, num_attention_heads))
  head_size = hidden_size // num_attention_heads
  if input_tensor.dim() != 3:
    raise ValueError('transformer_encoder: a rank 3 input is expected, got rank %d' % input_tensor.dim())
  B, S, width = (int(n) for n in input_tensor.shape)
  if width != hidden_size:
    raise ValueError('The width of the input tensor (%d) != hidden size (%d)' % (width, hidden_size))
  vs = context.varstore()
  init = create_initializer(initializer_range)
  prev = input_tensor.reshape(B * S, width)
  for layer_idx in range(num_hidden_layers):
    with vs.scope('%s_layer_%d' % (name, layer_idx)):
      layer_input = prev
      with vs.scope('attention'):
        with vs.scope('self'):
          att = attention_layer(layer_input, layer_input, head_size, num_attention_heads, attention_mask,
                                attention_probs_dropout_prob=attention_probs_dropout_prob,
                                initializer_range=initializer_range, do_return_2d_tensor=True, batch_size=B,
                                from_seq_length=S, to_seq_length=S, reuse=reuse, group_units=group_units)
        with vs.scope('output'):
          att = dropout(dnn.dense(att, hidden_size, 'dense', kernel_initializer=init), hidden_dropout_prob)
          att = layer_norm(att, 'LayerNorm', residual=layer_input)
      with vs.scope('intermediate'):
        mid = dnn.dense(att, intermediate_size, 'dense', kernel_initializer=init)
        if intermediate_act_fn is not None:
          mid = intermediate_act_fn(mid)
      with vs.scope('output'):
        out = dropout(dnn.dense(mid, hidden_size, 'dense', kernel_initializer=init), hidden_dropout_prob)
        prev = layer_norm(out, 'LayerNorm', residual=att)
  return prev.reshape(B, S, width)


def cross_attention_block(from_tensor, to_tensor, layer_idx, size_per_head, cross_attention_mask=None,
                          self_attention_mask=None, num_attention_heads=1, intermediate_size=512, hidden_dropout_prob=0.0,
                          attention_probs_dropout_prob=0.0, initializer_range=0.02, name=''):
  """reference :372-485.  from_tensor [B, F, Wf] attends to to_tensor [B, T, Wt] (`cross`), the result attends to
  itself (`self`: one Q | K | V contraction), LN(self + cross), a ReLU intermediate dense, an output dense and
  LN(output + attention output) -> [B, F, num_attention_heads * size_per_head]."""
  if from_tensor.dim() != 3 or to_tensor.dim() != 3:
    raise ValueError('cross_attention_block: rank 3 inputs are expected')
  B, F, T = int(from_tensor.shape[0]), int(from_tensor.shape[1]), int(to_tensor.shape[1])
  hidden = num_attention_heads * size_per_head
  vs = context.varstore()
  init = create_initializer(initializer_range)
  with vs.scope('%scross_layer_%d' % (name, layer_idx)):
    with vs.scope('attention'):
      with vs.scope('cross'):
        cross = attention_layer(from_tensor, to_tensor, size_per_head, num_attention_heads, cross_attention_mask,
                                attention_probs_dropout_prob=attention_probs_dropout_prob,
                                initializer_range=initializer_range, do_return_2d_tensor=True, batch_size=B,
                                from_seq_length=F, to_seq_length=T, group_units=True)
      with vs.scope('self'):
        own = attention_layer(cross, cross, size_per_head, num_attention_heads, self_attention_mask,
                              attention_probs_dropout_prob=attention_probs_dropout_prob,
                              initializer_range=initializer_range, do_return_2d_tensor=True, batch_size=B,
                              from_seq_length=F, to_seq_length=F, group_units=True)
      with vs.scope('output'):
        att = layer_norm(dropout(own, hidden_dropout_prob), 'LayerNorm', residual=cross)
    with vs.scope('intermediate'):
      mid = torch.relu(dnn.dense(att, intermediate_size, 'dense', kernel_initializer=init))
    with vs.scope('output'):
      out = dropout(dnn.dense(mid, hidden, 'dense', kernel_initializer=init), hidden_dropout_prob)
      out = layer_norm(out, 'LayerNorm', residual=att)
  return out.reshape(B, F, hidden)


def cross_attention_tower(left_tensor, right_tensor, num_hidden_layers=1, num_attention_heads=12, left_size_per_head=64,
                          right_size_per_head=64, left_intermediate_size=0, right_intermediate_size=0,
                          left_input_mask=None, right_input_mask=None, hidden_dropout_prob=0.0,
                          attention_probs_dropout_prob=0.0, initializer_range=0.02, name=''):
  """reference :488-595: num_hidden_layers times a `left_to_right_` and a `right_to_left_` cross_attention_block, both
  reading the previous layer's outputs -> ([B, L, H * left_size_per_head], [B, R, H * right_size_per_head]).
  right_input_mask [B, R] masks the right tokens as keys (of the left block's cross attention and the right block's self
  attention).  The reference cannot take a left_input_mask (it hands None to create_attention_mask_from_input_mask)."""
  if left_input_mask is not None:
    raise ValueError('cross_attention_tower: `left_input_mask` is not supported (the reference fails on it itself)')
  if left_intermediate_size <= 0:
    left_intermediate_size = num_attention_heads * left_size_per_head
  if right_intermediate_size <= 0:
    right_intermediate_size = num_attention_heads * right_size_per_head
  left_2_right_mask = right_mask = None
  if right_input_mask is not None:
    left_2_right_mask = create_attention_mask_from_input_mask(left_tensor, right_input_mask)
    right_mask = create_attention_mask_from_input_mask(right_tensor, right_input_mask)
  prev_left, prev_right = left_tensor, right_tensor
  for layer_idx in range(num_hidden_layers):
    left = cross_attention_block(prev_left, prev_right, layer_idx, left_size_per_head, left_2_right_mask, None,
                                 num_attention_heads, left_intermediate_size, hidden_dropout_prob,
                                 attention_probs_dropout_prob, initializer_range, '%sleft_to_right_' % name)
    right = cross_attention_block(prev_right, prev_left, layer_idx, right_size_per_head, None, right_mask,
                                  num_attention_heads, right_intermediate_size, hidden_dropout_prob,
                                  attention_probs_dropout_prob, initializer_range, '%sright_to_left_' % name)
    prev_left, prev_right = left, right
  return prev_left, prev_right


# ------------------------------------------------------------------------------------------------ segment mean pooling
def segment_mean_compose(x, seg_begin, lens):
  """x [B, S, W]; seg_begin: n_seg + 1 ascending Python ints from 0 to S; lens [B, n_seg] or None -> [B, n_seg, W]: per
  segment the sum of its first len rows over len (a masked sum and a count, reference layers/cmbf.py:306-316; len == 0
  gives 0 / 0 = NaN)."""
  outs = []
  for s in range(len(seg_begin) - 1):
    b0, b1 = seg_begin[s], seg_begin[s + 1]
    part = x[:, b0:b1, :]
    if lens is None:
      outs.append(part.sum(dim=1, keepdim=True) / float(b1 - b0))
    else:
      n = lens[:, s].clamp(0, b1 - b0)
      mask = (torch.arange(b1 - b0, device=x.device)[None, :] < n[:, None]).to(x.dtype).unsqueeze(-1)
      outs.append((part * mask).sum(dim=1, keepdim=True) / mask.sum(dim=1, keepdim=True))
  return torch.cat(outs, dim=1)


_SEG_BEGIN = {}


def _seg_begin_tensor(seg_begin, device):
  """The segment table on the device, made once per (table, device): a host-to-device copy is not capturable."""
  key = (tuple(seg_begin), str(device))
  t = _SEG_BEGIN.get(key)
  if t is None:
    t = _SEG_BEGIN[key] = torch.tensor(list(seg_begin), dtype=torch.int32, device=device)
  return t


def segment_mean(x, seg_begin, lens=None):
  """Mean pooling over consecutive segments of the token axis: x [B, S, W], seg_begin (n_seg + 1 ascending ints, 0 .. S),
  lens [B, n_seg] integer (a segment's valid prefix) or None (full) -> [B, n_seg, W].  One launch each way on the HIP
  backend (kernels.SegmentMeanFn), segment_mean_compose elsewhere."""
  seg_begin = [int(v) for v in seg_begin]
  B, S, W = (int(n) for n in x.shape)
  n_seg = len(seg_begin) - 1
  if n_seg < 1 or seg_begin[0] != 0 or seg_begin[-1] != S or any(a >= b for a, b in zip(seg_begin, seg_begin[1:])):
    raise ValueError('segment_mean: segment begins %r do not tile 0 .. %d' % (seg_begin, S))
  if _fused(x) and B > 0 and W <= SEGMENT_MEAN_MAX and S <= SEGMENT_MEAN_MAX and n_seg <= 64:
    lens32 = None if lens is None else lens.to(torch.int32).contiguous()
    return kernels.SegmentMeanFn.apply(x, _seg_begin_tensor(seg_begin, x.device), lens32, n_seg)
  return segment_mean_compose(x, seg_begin, lens)


def embedding_postprocessor(input_tensor, use_token_type=False, token_type_ids=None, token_type_vocab_size=16,
                            token_type_embedding_name='token_type_embeddings', reuse_token_type=None,
                            use_position_embeddings=True, position_embedding_name='position_embeddings',
                            reuse_position_embedding=None, initializer_range=0.02, max_position_embeddings=512,
                            dropout_prob=0.0):
  """input_tensor [B, S, W] + token-type embeddings + position embeddings -> LayerNorm -> dropout.  token_type_ids: an
  int (every token: the table's row, broadcast), a list / tensor [S] (per position) or a tensor [B, S] (a one-hot
  product, as the reference's :727-729)."""
  if input_tensor.dim() != 3:
    raise ValueError('embedding_postprocessor: a rank 3 input is expected, got rank %d' % input_tensor.dim())
  B, S, W = (int(n) for n in input_tensor.shape)
  vs = context.varstore()
  init = create_initializer(initializer_range)
  addend = None  # [S, W] (per position) or [B * S, W]
  if use_token_type:
    if token_type_ids is None:
      raise ValueError('`token_type_ids` must be specified if `use_token_type` is True.')
    with vs.scope('token_type'):
      table = vs.get_variable(token_type_embedding_name, (token_type_vocab_size, W), init)
    if isinstance(token_type_ids, int):
      # one type for every token (all of Uniter's calls): the table's row as a broadcast view, no launch
      if not 0 <= token_type_ids < token_type_vocab_size:
        raise ValueError('token_type_ids %d outside the vocabulary of %d' % (token_type_ids, token_type_vocab_size))
      addend = table[token_type_ids:token_type_ids + 1].expand(S, W)
    else:
      # per position [S] or per token [B, S]: the one-hot product of the reference (:727-729), whose gradient is a
      # product too and not a scatter.  A plain autograd matmul: several calls may share the table within one step, and
      # its gradient must then accumulate call after call (the step's queued weight-gradient launch takes each
      # variable once).  A host list costs a host-to-device copy (not capturable): pass a device tensor inside a step.
      ids = torch.as_tensor(token_type_ids).to(device=input_tensor.device, dtype=torch.int64).reshape(-1)
      if ids.numel() not in (S, B * S):
        raise ValueError('token_type_ids: %d ids for [%d, %d] tokens' % (ids.numel(), B, S))
      addend = torch.matmul(torch.nn.functional.one_hot(ids, token_type_vocab_size).to(table.dtype), table)
  if use_position_embeddings:
    if S > max_position_embeddings:
      raise ValueError('sequence length %d exceeds max_position_embeddings %d' % (S, max_position_embeddings))
    with vs.scope('position_embedding'):
      full = vs.get_variable(position_embedding_name, (max_position_embeddings, W), init)
    pos = full[:S]
    if addend is None:
      addend = pos
    elif addend.shape[0] == S:
      addend = addend + pos
    else:
      addend = (addend.reshape(B, S, W) + pos).reshape(B * S, W)
  return layer_norm_and_dropout(input_tensor, dropout_prob, residual=addend)
