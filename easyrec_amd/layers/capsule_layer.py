"""MIND's capsule layer with dynamic routing (reference easy_rec/python/layers/capsule_layer.py:12-176) and the
label-aware attention of its user tower (reference model/mind.py:168-200), on the fused HIP kernels (csrc/er_capsule.hip,
easyrec_hip.h K8g) inside their envelope and composed of torch ops outside it and on a CPU backend.

EASYREC_AMD_FUSED_CAPSULE selects the path on a GPU: 1 (the default) the fused kernels, 0 the composition;
tools/mind_bench.py measures both.

Initial routing logits.  Evaluation and prediction use the reference's own table - np.random.seed(28);
np.random.uniform(high=stddev, size=[S, K]) as float32 - shared by the whole batch.  Training draws a truncated normal
(stddev, cut at two standard deviations) per step from torch's generator of the device, which a hipGraph replay
advances like Dropout's: parity with TensorFlow's generator holds IN DISTRIBUTION ONLY, never value by value.  The
tensor a call used stays reachable as `last_routing_logits`, so a step can be replayed elsewhere."""
import logging
import os

import numpy as np
import torch

from easyrec_amd import kernels
from easyrec_amd.core import context

MAX_K = 8
MAX_ITERS = 8
ATT_MAX_E = 128
MASK_VALUE = 1e32
# int(log(float(len))) steps up at these lengths: no integer lies near a power of e, so the thresholds are exact
CAPS_THRESHOLDS = (8, 21, 55, 149, 404, 1097, 2981)
fused_capsule = os.environ.get('EASYREC_AMD_FUSED_CAPSULE', '1') != '0'


def lds_bytes(S, D, E, K):
  """er_capsule_lds_bytes: one example's X, H, W, c, dc and row norms, each row at an odd pitch; 0 outside the envelope."""
  if not (1 <= S <= 128 and 1 <= D <= 128 and 1 <= E <= 128 and 1 <= K <= MAX_K and D * E < 65536):
    return 0
  return 4 * (S * (D | 1) + S * (E | 1) + S * K + 2 * K * (E | 1) + S)


def _on_hip(x):
  return x.is_cuda and x.dtype == torch.float32 and isinstance(kernels.hip(), kernels.HipBackend)


def capsule_fits(hist, S, E, K, num_iters):
  """Whether the capsule kernels take this operand: a HIP backend, a device tensor, fp32, the shape inside the envelope."""
  return _on_hip(hist) and lds_bytes(S, int(hist.shape[2]), E, K) > 0 and 1 <= num_iters <= MAX_ITERS


def attention_fits(interests):
  return _on_hip(interests) and 1 <= interests.shape[1] <= MAX_K and 1 <= interests.shape[2] <= ATT_MAX_E


def normalize_compose(x):
  """tf.nn.l2_normalize(x, axis=-1)"""
  return x * torch.rsqrt(torch.clamp((x * x).sum(dim=-1, keepdim=True), min=1e-12))


def num_capsules(seq_lens, S, K, const_caps_num):
  """[B] int32: K, or max(1, min(K, int(log(float(min(len, S))))))"""
  lens = seq_lens.clamp(0, S)
  if const_caps_num:
    return torch.full_like(lens, K, dtype=torch.int32)
  n = torch.ones_like(lens)
  for step in CAPS_THRESHOLDS:  # (comparisons with host scalars: nothing is copied to the device, so a capture takes it)
    n = n + (lens >= step).to(lens.dtype)
  return n.clamp(max=K).to(torch.int32)


def eval_routing_logits(S, K, stddev):
  """the reference's evaluation table (capsule_layer.py:87-92), float32 [S, K]"""
  state = np.random.get_state()
  try:
    np.random.seed(28)
    table = np.random.uniform(high=stddev, size=[S, K])
  finally:
    np.random.set_state(state)
  return table.astype(np.float32)


def capsule_compose(hist, seq_lens, Smat, logits0, S, K, num_iters, scale, squash_pow, scale_ratio, const_caps_num):
  """CapsuleLayer.__call__ as torch ops -> (high_capsules [B, K, E], num_caps [B] int32)."""
  B, L, _ = hist.shape
  dt, dev = hist.dtype, hist.device
  if L > S:
    hist = hist[:, :S]
  elif L < S:
    hist = torch.nn.functional.pad(hist, (0, 0, 0, S - L))
  lens = seq_lens.clamp(0, S)
  ncaps = num_capsules(seq_lens, S, K, const_caps_num)
  high = hist @ Smat
  high_stop = high.detach()
  high_norm = normalize_compose(high_stop)
  mask = (torch.arange(S, device=dev)[None, :] < lens[:, None]).to(dt)
  mask_cap = (torch.arange(K, device=dev)[None, :] < ncaps[:, None]).to(dt)
  thresh = ((mask_cap * 2 - 1) * MASK_VALUE)[:, None, :]
  r = logits0.detach().to(dt)
  r = r[None].expand(B, S, K) if r.dim() == 2 else r
  caps = None
  for it in range(num_iters):
    r = torch.softmax(torch.minimum(r, thresh), dim=2) * mask[:, :, None]
    last = it + 1 == num_iters
    caps = torch.einsum('bse,bsh->bhe', high if last else high_stop, r)
    if last:
      n = torch.clamp((caps * caps).sum(dim=-1, keepdim=True), min=1e-8)
      caps = torch.pow(n / (1 + n), squash_pow) * scale_ratio / torch.sqrt(n) * caps
      break
    caps = normalize_compose(caps)
    if scale > 0:
      r = torch.einsum('bse,bhe->bsh', high_norm, caps) * scale
    else:
      r = torch.einsum('bse,bhe->bsh', high_stop, caps)
  return caps * mask_cap[:, :, None], ncaps


def capsule_routing(hist, seq_lens, Smat, logits0, S, K, num_iters, scale, squash_pow, scale_ratio, const_caps_num,
                    grad=None):
  """(high_capsules, num_caps) on the kernels where they take the operand and the switch allows, else composed.  grad:
  Smat's gradient buffer, which the fused backward adds into (None: autograd receives the gradient)."""
  E = int(Smat.shape[1])
  if not (fused_capsule and capsule_fits(hist, S, E, K, num_iters)):
    return capsule_compose(hist, seq_lens, Smat, logits0, S, K, num_iters, scale, squash_pow, scale_ratio,
                           const_caps_num)
  cfg = (int(S), int(K), int(num_iters), float(scale), float(squash_pow), float(scale_ratio), bool(const_caps_num))
  return kernels.CapsuleRoutingFn.apply(hist, seq_lens.to(torch.int32), logits0.contiguous(), cfg,
                                        None if grad is None else [grad], Smat)


def attention_compose(interests, pos_item, num_caps, simi_pow):
  """mind.py:168-200 as torch ops -> (user_tower_emb [B, E], masked user_interests [B, K, E])."""
  K = interests.shape[1]
  simi = torch.einsum('bhe,be->bh', interests, pos_item) * simi_pow
  mask = (torch.arange(K, device=interests.device)[None, :] < num_caps[:, None]).to(interests.dtype)
  user_interests = interests * mask[:, :, None]
  simi = torch.softmax(torch.minimum(simi, (mask * 2 - 1) * MASK_VALUE), dim=1)
  if simi_pow >= 100:
    # (torch.argmax promises no tie rule; the first index among the maxima is tf.argmax's)
    first = (simi == simi.max(dim=1, keepdim=True).values).to(torch.int32).argmax(dim=1)
    simi = torch.nn.functional.one_hot(first, K).to(interests.dtype)
  return torch.einsum('bhe,bh->be', user_interests, simi), user_interests


def label_aware_attention(interests, pos_item, num_caps, simi_pow):
  if not (fused_capsule and attention_fits(interests) and pos_item.dtype == torch.float32):
    return attention_compose(interests, pos_item, num_caps, simi_pow)
  return kernels.MindAttentionFn.apply(interests, pos_item, num_caps.to(torch.int32), float(simi_pow))


class CapsuleLayer(object):

  def __init__(self, capsule_config, is_training):
    self._max_seq_len = int(capsule_config.max_seq_len)
    self._max_k = int(capsule_config.max_k)
    self._high_dim = int(capsule_config.high_dim)
    self._num_iters = int(capsule_config.num_iters)
    self._routing_logits_scale = float(capsule_config.routing_logits_scale)
    self._routing_logits_stddev = float(capsule_config.routing_logits_stddev)
    self._squash_pow = float(capsule_config.squash_pow)
    self._scale_ratio = float(capsule_config.scale_ratio)
    self._const_caps_num = bool(capsule_config.const_caps_num)
    self._is_training = is_training
    self._eval_logits = None
    self.last_routing_logits = None

  def routing_logits(self, batch_size, device):
    S, K, std = self._max_seq_len, self._max_k, self._routing_logits_stddev
    if self._is_training:
      r = torch.empty(batch_size, S, K, dtype=torch.float32, device=device)
      if std > 0:
        torch.nn.init.trunc_normal_(r, 0.0, std, -2 * std, 2 * std)
      else:
        r.zero_()
      return r
    if self._eval_logits is None or self._eval_logits.device != torch.device(device):
      self._eval_logits = torch.from_numpy(eval_routing_logits(S, K, std)).to(device)
    return self._eval_logits

  def __call__(self, seq_feas, seq_lens):
    """seq_feas [B, L, low_fea_dim], seq_lens [B] -> (high_capsules [B, max_k, high_dim], num_high_capsules [B])."""
    vs = context.varstore()
    D = int(seq_feas.shape[-1])
    Smat = vs.get_variable('capsule/S', (D, self._high_dim), 'glorot_uniform')
    if self._const_caps_num:
      logging.info('will use constant number of capsules: %d' % self._max_k)
    else:
      logging.info('will use log(seq_len) number of capsules, max_capsules: %d' % self._max_k)
    logits0 = self.routing_logits(seq_feas.shape[0], seq_feas.device)
    self.last_routing_logits = logits0
    grad = Smat.grad if (Smat.requires_grad and Smat.grad is not None and torch.is_grad_enabled()) else None
    return capsule_routing(seq_feas, seq_lens, Smat, logits0, self._max_seq_len, self._max_k, self._num_iters,
                           self._routing_logits_scale, self._squash_pow, self._scale_ratio, self._const_caps_num, grad)
