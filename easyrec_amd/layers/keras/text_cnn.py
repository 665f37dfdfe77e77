"""Combining one sequence column over time: `TextCNN` (reference easy_rec/python/layers/keras/blocks.py:212-262) and
the attention pooling of a feature group's `sequence_combiner { attention {} }` (layers/input_layer.py:323-338).

  TextCNN    pad / truncate the [B, L, D] sequence to `pad_sequence_length` positions, one Conv1D (+ activation) per
             filter size, the maximum over the window positions of each filter, concatenated (-> `mlp` when configured).
             Lengths do not mask: windows that lie in the padding take part in the maximum, as in the reference.
  attention  logit_t = Dense(1, no bias)(x_t), -2^32 + 1 where t >= length, softmax over time, the weighted sum.

Which path runs is decided by what the code can see, as layers/multihead_cross_attention._fused does: a CUDA fp32
tensor on the HIP backend with a geometry inside the kernels' envelope (text_cnn_fits / seq_attn_pool_fits, the formulas
of include/easyrec_hip.h K8h) is ONE forward and ONE backward launch (kernels.TextCnnFn / SeqAttnPoolFn,
csrc/er_seq_combine.hip), which read the column in place from the embedding engine's [B * L, width] sequence output.
Anywhere else - a stand-in backend on the CPU, an activation other than relu / linear, pad_sequence_length <= 0 (the
time extent is then the loaded batch's, no build-time constant), a geometry outside the envelope, or
EASYREC_AMD_FUSED_SEQ_COMBINE=0 - the same function is composed of torch ops (text_cnn_compose /
seq_attn_pool_compose; torch.amax splits a tie's gradient evenly, TensorFlow's reduce_max rule).

Variables carry the reference's names: Keras numbers the unnamed Conv1D layers per graph where they are constructed (`conv1d`,
`conv1d_1`, ...; here VarStore.next_layer_names, taken in __init__), each under the TextCNN layer's name, then `<name>/mlp/...`.
"""
import logging
import math
import os

import numpy as np
import torch

from easyrec_amd import kernels
from easyrec_amd.core import context
from easyrec_amd.layers.keras.blocks import MLP
from easyrec_amd.layers.utils import Parameter

LDS_FLOATS = 16384  # 64 KiB per workgroup (csrc/er_seq_combine.hip)
MAX_P = MAX_D = MAX_FILTERS = 64
MAX_SIZES = 4
MAX_KERNEL = 8
POOL_MAX_L = 1024
POOL_MAX_D = 128
MASKED_LOGIT = float(-2 ** 32 + 1)


def fused_enabled():
  """EASYREC_AMD_FUSED_SEQ_COMBINE=0: the torch composition everywhere (the A/B switch of the K8h kernels)."""
  return os.environ.get('EASYREC_AMD_FUSED_SEQ_COMBINE', '1') != '0'


def _fused(x):
  return fused_enabled() and x.is_cuda and x.dtype == torch.float32 and isinstance(kernels.hip(), kernels.HipBackend)


def _grads_of(params):
  # (the variables' slices of the flat gradient buffer; None in the build pass, before VarStore.pack)
  return [p.grad for p in params] if all(p.grad is not None for p in params) else None


# ------------------------------------------------------------------------------------------------ the kernels' envelope
def _round4(n):
  return (n + 3) & ~3


def text_cnn_epb(pad_len, dim, sizes, filters):
  """er_text_cnn_epb: examples per workgroup round, 0 outside the envelope."""
  sizes, filters = [int(k) for k in sizes], [int(f) for f in filters]
  if not (1 <= pad_len <= MAX_P and 1 <= dim <= MAX_D and 1 <= len(sizes) <= MAX_SIZES and len(sizes) == len(filters)):
    return 0
  if any(k < 1 or k > min(pad_len, MAX_KERNEL) for k in sizes) or any(f < 1 for f in filters) or \
      sum(filters) > MAX_FILTERS:
    return 0
  per = _round4(pad_len * (dim | 1) + sum((pad_len - k + 1) * f for k, f in zip(sizes, filters)))
  theta = _round4(sum(k * dim * (f | 1) + f for k, f in zip(sizes, filters)))
  if theta + per > LDS_FLOATS:
    theta = 0  # (the kernels read theta in place)
  return min(8, (LDS_FLOATS - theta) // per)


def text_cnn_lds_bytes(pad_len, dim, sizes, filters):
  """er_text_cnn_lds_bytes."""
  epb = text_cnn_epb(pad_len, dim, sizes, filters)
  if epb == 0:
    return 0
  per = _round4(pad_len * (dim | 1) + sum((pad_len - k + 1) * f for k, f in zip(sizes, filters)))
  theta = _round4(sum(k * dim * (f | 1) + f for k, f in zip(sizes, filters)))
  return 4 * ((theta if theta + per <= LDS_FLOATS else 0) + epb * per)


def text_cnn_fits(pad_len, dim, sizes, filters):
  return text_cnn_epb(pad_len, dim, sizes, filters) > 0


def seq_attn_pool_fits(length, dim):
  return 1 <= length <= POOL_MAX_L and 1 <= dim <= POOL_MAX_D


def seq_attn_pool_lds_bytes(length, dim, bwd):
  """er_seq_attn_pool_lds_bytes."""
  if not seq_attn_pool_fits(length, dim):
    return 0
  return 16 * (2 * _round4(length) + 128) if bwd else 16 * _round4(length)


# ------------------------------------------------------------------------------------------------ the torch compositions
def pad_or_truncate(seq_emb, pad_len):
  """utils/shape_utils.py pad_or_truncate_sequence on the embedding: [B, L, D] -> [B, pad_len, D]."""
  L = seq_emb.shape[1]
  if L >= pad_len:
    return seq_emb[:, :pad_len]
  return torch.nn.functional.pad(seq_emb, (0, 0, 0, pad_len - L))


def _activate(z, activation):
  act = None if activation is None else str(activation).lower()
  if act in (None, '', 'linear'):
    return z
  if act == 'relu':
    return torch.relu(z)
  if act == 'tanh':
    return torch.tanh(z)
  if act == 'sigmoid':
    return torch.sigmoid(z)
  raise NotImplementedError('TextCNN: activation %r' % activation)


def text_cnn_compose(seq_emb, pad_len, kernels_, biases, activation='relu'):
  """TextCNN.call op by op up to the concatenation: seq_emb [B, L, D]; kernels_[i] [k_i, D, F_i] (Keras Conv1D),
  biases[i] [F_i] -> [B, sum F_i].  pad_len <= 0: no padding."""
  x = pad_or_truncate(seq_emb, pad_len) if pad_len > 0 else seq_emb
  xt = x.transpose(1, 2)  # [B, D, P]
  pooled = []
  for w, b in zip(kernels_, biases):
    z = torch.nn.functional.conv1d(xt, w.permute(2, 1, 0), b)  # [B, F, P - k + 1]
    pooled.append(torch.amax(_activate(z, activation), dim=2))
  return torch.cat(pooled, dim=-1)


def seq_attn_pool_compose(seq_emb, seq_len, w):
  """The attention branch of single_call_input_layer op by op: seq_emb [B, L, D], seq_len [B], w [D, 1] -> [B, D]."""
  logits = (seq_emb @ w).squeeze(-1)
  mask = torch.arange(seq_emb.shape[1], device=seq_emb.device)[None, :] < seq_len.to(torch.int64)[:, None]
  score = torch.softmax(torch.where(mask, logits, torch.full_like(logits, MASKED_LOGIT)), dim=-1)
  return (score[:, :, None] * seq_emb).sum(dim=1)


def seq_attention_pool(seq_emb, seq_len, scope, l2_reg=None, full_seq=None):
  """`sequence_combiner { attention {} }`: the variable `<scope>/attention/kernel` [D, 1] (tf.layers.dense, no bias).
  full_seq: the un-truncated column view of the engine's sequence output, which the kernels read in place (the masked
  positions weigh nothing, so the extent does not matter; a row of length 0 pools zero embeddings either way)."""
  D = int(seq_emb.shape[-1])
  w = context.varstore().get_variable(scope + '/attention/kernel', (D, 1), 'glorot_uniform', l2=l2_reg or 0.0)
  x = seq_emb if full_seq is None else full_seq
  if _fused(x) and x.shape[0] > 0 and seq_attn_pool_fits(int(x.shape[1]), D):
    return kernels.SeqAttnPoolFn.apply(x, seq_len.to(torch.int32).contiguous(), _grads_of([w]), w)
  return seq_attn_pool_compose(seq_emb, seq_len, w)


# ------------------------------------------------------------------------------------------------ the block
def _conv_glorot_uniform(shape, rng):
  """Keras glorot_uniform on a Conv1D kernel [k, D, F]: fan_in = k * D, fan_out = k * F."""
  k, d, f = shape
  limit = math.sqrt(6.0 / (k * d + k * f))
  return rng.uniform(-limit, limit, size=shape).astype(np.float32)


class TextCNN(object):
  """Called on (seq_emb [B, L, D], seq_len [B], ...); `full_seq`: the un-truncated column view of the engine's sequence
  output the kernels read in place (positions from the batch's longest sequence on hold zero embeddings)."""

  def __init__(self, params, name='text_cnn', reuse=None, **kwargs):
    self.name = name
    self.config = params.get_pb_config()
    self.pad_seq_length = int(self.config.pad_sequence_length)
    if self.pad_seq_length <= 0:
      logging.warning('run text cnn with pad_sequence_length <= 0, the predict of model may be unstable')
    self.sizes = [int(k) for k in self.config.filter_sizes]
    self.filters = [int(f) for f in self.config.num_filters]
    n = min(len(self.sizes), len(self.filters))  # (the reference zips the two lists)
    self.sizes, self.filters = self.sizes[:n], self.filters[:n]
    assert n > 0, 'TextCNN(%s) takes at least one filter size' % name
    self.activation = self.config.activation
    # (Keras numbers the unnamed Conv1D layers where TextCNN.__init__ constructs them)
    self._conv_names = context.varstore().next_layer_names('conv1d', n)
    if getattr(context.current(), 'dense_dtype', 'f32') == 'bf16':
      raise ValueError('TextCNN(%s): dense_dtype bf16 is not supported (the sequence combiners are fp32)' % name)
    self.mlp = None
    if self.config.HasField('mlp'):
      p = Parameter.make_from_pb(self.config.mlp)
      p.l2_regularizer = params.l2_regularizer
      self.mlp = MLP(p, name=name + '/mlp')

  def variables(self, dim, vs=None):
    """kernel and bias of each Conv1D, in the packed order."""
    vs = vs or context.varstore()
    out = []
    for cname, k, f in zip(self._conv_names, self.sizes, self.filters):
      out.append(vs.get_variable('%s/%s/kernel' % (self.name, cname), (k, dim, f), _conv_glorot_uniform))
      out.append(vs.get_variable('%s/%s/bias' % (self.name, cname), (f,), 'zeros'))
    return out

  def __call__(self, inputs, training=None, full_seq=None, **kwargs):
    assert isinstance(inputs, (list, tuple)) and len(inputs) >= 2
    seq_emb = inputs[0]
    assert seq_emb.dim() == 3, 'TextCNN(%s) takes a [B, L, D] sequence embedding' % self.name
    D = int(seq_emb.shape[2])
    P = self.pad_seq_length
    extent = P if P > 0 else int(seq_emb.shape[1])
    if extent < max(self.sizes):
      raise ValueError('TextCNN(%s): the time extent %d is shorter than the largest filter %d' % (
          self.name, extent, max(self.sizes)))
    params = self.variables(D)
    act = None if self.activation is None else str(self.activation).lower()
    x = seq_emb if full_seq is None else full_seq
    if P > 0 and act in ('relu', 'linear') and _fused(x) and x.shape[0] > 0 and \
        text_cnn_fits(P, D, self.sizes, self.filters):
      net = kernels.TextCnnFn.apply(x, P, self.sizes, self.filters, act == 'relu', _grads_of(params), *params)
    else:
      net = text_cnn_compose(seq_emb, P, params[0::2], params[1::2], self.activation)
    if self.mlp is not None:
      net = self.mlp(net, training=training)
    return net
