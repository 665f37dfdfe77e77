"""The BST transformer block of MultiTowerBST (reference model/multi_tower_bst.py:59-151, layers/layer_norm.py:9-40).

Variables, as the reference's TF1 graph names them:
  multi_head_{s}_{query|key|value}/multi_head_{s}_{query|key|value}_0/{kernel,bias}  [p_h, p_h] / [p_h], one per head,
      s = the head's start column (:104-113; dnn_net's only layer is its last one: no activation, :62-75)
  multi_head_attention/multi_head_attention_0/{kernel,bias}                          [E, E] / [E] (:116-117)
  feed_forward_net/feed_forward_net_0/{kernel,bias}                                  [E, E] / [E] (:141)
  layer_normalization[_k]/layer_norm_{scale,bias}                                    [E], ones / zeros (layer_norm.py:19-29)
The dense scopes are opened with AUTO_REUSE and bst() ignores its name: every BST tower of a model shares the dense
variables, while each LayerNormalization call is a new Keras-style layer with a uniquified name (two per tower).  None of
them carries a regulariser (tf.layers.dense without kernel_regularizer).

The whole block runs in two HIP launches per tower and step (er_bst_fwd / er_bst_bwd + the gradient reduction):
kernels.BSTBlockFn.
"""
import math

from easyrec_amd import kernels
from easyrec_amd.core import context

MAX_T = 64  # the kernels' envelope (csrc/er_bst.hip)
MAX_E = 64


def head_split(E, H):
  """[(start column, width)] of the heads (multi_tower_bst.py:102-113): width ceil(E / H), the last one narrower - so
  there can be fewer than H heads."""
  p = int(math.ceil(E / float(H)))
  return [(s, min(p, E - s)) for s in range(0, E, p)]


def check_envelope(T, E, H, name='bst'):
  if T < 2 or T > MAX_T:
    raise ValueError('%s: seq_len %d is outside the BST kernels\' envelope 2 <= seq_len <= %d' % (name, T, MAX_T))
  if E < 1 or E > MAX_E:
    raise ValueError('%s: embedding width %d is outside the BST kernels\' envelope E <= %d' % (name, E, MAX_E))
  if H < 1:
    raise ValueError('%s: multi_head_size must be at least 1, got %d' % (name, H))


def _ln_name(index):
  return 'layer_normalization' if index == 0 else 'layer_normalization_%d' % index


def bst_variables(vs, E, H, ln_index):
  """The block's variables in er_bst_param_count's order (see easyrec_hip.h K8b), created or fetched by name.
  ln_index: how many LayerNormalization layers the model created before this block."""
  heads = head_split(E, H)
  per_kind = {}
  for kind in ('query', 'key', 'value'):
    ws, bs = [], []
    for s, w in heads:
      scope = 'multi_head_%d_%s' % (s, kind)
      ws.append(vs.get_variable('%s/%s_0/kernel' % (scope, scope), (w, w), 'glorot_uniform'))
      bs.append(vs.get_variable('%s/%s_0/bias' % (scope, scope), (w,), 'zeros'))
    per_kind[kind] = ws + bs
  params = per_kind['query'] + per_kind['key'] + per_kind['value']
  for scope in ('multi_head_attention', 'feed_forward_net'):
    params.append(vs.get_variable('%s/%s_0/kernel' % (scope, scope), (E, E), 'glorot_uniform'))
    params.append(vs.get_variable('%s/%s_0/bias' % (scope, scope), (E,), 'zeros'))
  for i in (ln_index, ln_index + 1):
    params.append(vs.get_variable('%s/layer_norm_scale' % _ln_name(i), (E,), 'ones'))
    params.append(vs.get_variable('%s/layer_norm_bias' % _ln_name(i), (E,), 'zeros'))
  return params


def bst(key, hist, seq_len, seq_size, head_count, ln_index):
  """One BST tower (multi_tower_bst.py:127-151).  key [B, E]; hist [B, L, E]: the sequence lookup's STATIC buffer
  (L = max_seq_len, rows t >= len zero), which the kernels pad / slice to seq_size - 1 rows exactly as the reference
  pads / slices the batch-max view (:133-138: the rows in between are zero either way).  Returns [B, seq_size * E]."""
  B, L, E = hist.shape
  if key.shape[-1] != E:
    raise ValueError('BST: key width %d != history width %d' % (key.shape[-1], E))
  check_envelope(seq_size, E, head_count)
  vs = context.varstore()
  params = bst_variables(vs, E, head_count, ln_index)
  hist = hist if hist.is_contiguous() else hist.contiguous()
  hist = kernels.slot_gate(hist)
  # (the variables' slices of the flat gradient buffer; None in the build pass, before VarStore.pack)
  grads = [p.grad for p in params] if all(p.grad is not None for p in params) else None
  return kernels.BSTBlockFn.apply(key, hist, seq_len, int(seq_size), int(head_count), grads, *params)
