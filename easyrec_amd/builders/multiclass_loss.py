"""The losses of the heads that read more than one logit per example.

  softmax cross entropy   CLASSIFICATION with num_class > 1: tf.losses.sparse_softmax_cross_entropy(labels, logits,
                          weights), reduction SUM_BY_NONZERO_WEIGHTS (reference builders/loss_builder.py:40-46)
  JRC                     reference loss/jrc_loss.py ("Joint Optimization of Ranking and Calibration with Contextualized
                          Hybrid Model", arXiv 2208.06164): alpha * that cross entropy at two classes + (1 - alpha) * a
                          generative loss over the examples of one session

Which path runs is decided by what the code can see.  On the HIP backend, with fp32 logits on the GPU and a shape inside
the kernel's envelope (include/easyrec_hip.h K8l), ONE launch yields the loss (as per-workgroup partial sums that the
loss tail's launch finishes), d loss / d logits and the head's predictions (csrc/er_multiclass.hip).  Anywhere else - a
stand-in backend on the CPU, a shape outside the envelope, EASYREC_AMD_FUSED_MULTICLASS=0, JRC without same_label_loss -
the compositions below run: the reference's forms as torch ops ([B, B] masks included for JRC), differentiated by
autograd.

A python-scalar sample weight other than 1 multiplies JRC's cross entropy inside tf.losses and the WHOLE loss again on
return (jrc_loss.py:39-40, :126-127); kept.
"""
import os

import numpy as np
import torch

from easyrec_amd import kernels

FUSED_DEFAULT = '1'  # EASYREC_AMD_FUSED_MULTICLASS when the environment does not set it
MAX_CLASSES = 4096   # er_softmax_ce: C
JRC_MAX_BATCH = 8192  # er_jrc: B
JRC_STRATEGIES = ('fixed', 'random_uniform', 'random_normal', 'random_bernoulli', 'uncertainty')


def fused_enabled():
  """EASYREC_AMD_FUSED_MULTICLASS=0: the torch compositions everywhere (the A/B switch of the K8l kernels)."""
  return os.environ.get('EASYREC_AMD_FUSED_MULTICLASS', FUSED_DEFAULT) != '0'


def _on_kernels(logits):
  return fused_enabled() and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and \
      logits.stride(1) == 1 and isinstance(kernels.hip(), kernels.HipBackend)


def softmax_ce_fits(B, C):
  return B >= 1 and 2 <= C <= MAX_CLASSES


def jrc_fits(B):
  return 1 <= B <= JRC_MAX_BATCH


def check_class_labels(label):
  """The reference asserts an integer label dtype (loss_builder.py:41-44).  The device label rows are fp32 whatever the
  input field's type is; the estimator marks those of INT32 / INT64 fields (`_er_integral`)."""
  integral = not label.dtype.is_floating_point or bool(getattr(label, '_er_integral', False))
  assert integral, 'label.dtype must in [tf.int32, tf.int64] when use sparse_softmax_cross_entropy.'


def _f32_labels(label):
  return (label if label.dtype == torch.float32 else label.to(torch.float32)).contiguous()


# ------------------------------------------------------------------------------------------------ the torch compositions
def _weighted_mean_by_nonzero(per, weights):
  """tf.losses.compute_weighted_loss, SUM_BY_NONZERO_WEIGHTS: sum(per * w) / #(w != 0) with the safe division; a scalar
  weight broadcasts (all B present, or none)."""
  if torch.is_tensor(weights):
    w = weights.to(per.dtype)
    present = (w != 0).sum().clamp(min=1).to(per.dtype)
    return (per * w).sum() / present
  w = float(weights)
  if w == 0.0:
    return per.sum() * 0.0
  return (per * w).sum() / float(per.numel())


def softmax_ce_compose(labels, logits, weights=1.0):
  """tf.losses.sparse_softmax_cross_entropy(labels, logits, weights) -> scalar"""
  lab = labels.to(torch.int64).reshape(-1, 1)
  per = -torch.log_softmax(logits, dim=1).gather(1, lab).squeeze(1)
  return _weighted_mean_by_nonzero(per, weights)


def head_predictions_compose(logits):
  """The prediction tensors of a multi-class head (rank_model.py:112-122)."""
  probs = torch.softmax(logits, dim=1)
  return {'probs': probs, 'logits_y': logits.max(dim=1).values, 'probs_y': probs.max(dim=1).values,
          'y': first_argmax(logits)}


def first_argmax(logits):
  """tf.argmax(logits, axis=1): the first index among equal maxima"""
  C = logits.shape[1]
  idx = torch.arange(C, device=logits.device).expand_as(logits)
  top = logits == logits.max(dim=1, keepdim=True).values
  return torch.where(top, idx, torch.full_like(idx, C)).min(dim=1).values


def label_rank_compose(logits, labels):
  """#{c : z_c > z_label} + #{c < label : z_c == z_label}: the label's place in tf.nn.top_k's order (larger first, the
  lower index first among equals) -> int64 [B]"""
  lab = labels.to(torch.int64).reshape(-1, 1)
  zl = logits.gather(1, lab)
  idx = torch.arange(logits.shape[1], device=logits.device).expand_as(logits)
  return ((logits > zl) | ((logits == zl) & (idx < lab))).sum(dim=1)


def label_rank(logits, labels):
  """label_rank of every row -> integer [B]: er_softmax_ce's forward-only launch, or the composition"""
  if _on_kernels(logits) and softmax_ce_fits(*logits.shape):
    return kernels.hip().softmax_ce(logits, _f32_labels(labels), None, want=('label_rank',))['label_rank']
  return label_rank_compose(logits, labels)


def jrc_compose(labels, logits, session_ids, alpha=0.5, sample_weights=1.0, same_label_loss=True):
  """jrc_loss.py:12-128 with the `fixed` strategy, op by op -> scalar.  sample_weights: a python scalar or a [B] tensor."""
  dt = logits.dtype
  B = logits.shape[0]
  ce = softmax_ce_compose(labels, logits, sample_weights)
  y1 = labels.to(dt).reshape(-1, 1)
  onehot = torch.cat([1 - y1, y1], dim=1)                                   # [B, 2]
  mask = (session_ids.reshape(-1, 1) == session_ids.reshape(1, -1)).to(dt)  # [B, B]
  z = logits.unsqueeze(1).expand(B, B, 2)
  y = onehot.unsqueeze(1).expand(B, B, 2) * mask.unsqueeze(2)
  z = z + (1 - mask.unsqueeze(2)) * -1e9
  y_neg, y_pos = y[:, :, 0], y[:, :, 1]
  l_neg, l_pos = z[:, :, 0], z[:, :, 1]
  if torch.is_tensor(sample_weights):
    pairwise = sample_weights.to(dt).reshape(1, -1).expand(B, B)
    y_pos, y_neg = y_pos * pairwise, y_neg * pairwise
  if same_label_loss:
    loss_pos = -(y_pos * torch.log_softmax(l_pos, dim=0)).sum(dim=0)
    loss_neg = -(y_neg * torch.log_softmax(l_neg, dim=0)).sum(dim=0)
    ge = ((loss_pos + loss_neg) / mask.sum(dim=0)).mean()
  else:
    diag = torch.eye(B, dtype=dt, device=logits.device)
    l_pos = l_pos + (1 - diag) * y_pos * -1e9
    l_neg = l_neg + (1 - diag) * y_neg * -1e9
    loss_pos = -torch.diagonal(y_pos * torch.log_softmax(l_pos, dim=0))
    loss_neg = -torch.diagonal(y_neg * torch.log_softmax(l_neg, dim=0))
    ge = (loss_pos + loss_neg).mean()
  loss = alpha * ce + (1 - alpha) * ge
  if np.isscalar(sample_weights) and sample_weights != 1.0:
    return loss * sample_weights
  return loss


def _by_autograd(fn, pred, loss_scale):
  z = pred.detach().clone().requires_grad_(True)
  with torch.enable_grad():
    loss = fn(z) * loss_scale
    dz, = torch.autograd.grad(loss, z)
  return loss.detach().reshape(1), dz


# ------------------------------------------------------------------------------------------------ what loss_builder calls
def _scalar_or_tensor(loss_weight):
  """(weights tensor or None, python-scalar weight)"""
  if torch.is_tensor(loss_weight):
    return loss_weight, 1.0
  return None, float(loss_weight)


def softmax_ce(label, pred, loss_weight=1.0, loss_scale=1.0):
  """-> (loss [1], d loss / d pred [B, C], extras: the launch's other outputs or None).  pred [B, C]."""
  check_class_labels(label)
  weights, lw = _scalar_or_tensor(loss_weight)
  B, C = pred.shape
  if _on_kernels(pred) and softmax_ce_fits(B, C):
    res = kernels.hip().softmax_ce(pred.detach(), _f32_labels(label), weights, loss_scale * lw)
    return res['loss'], res['dlogits'], res
  loss, dz = _by_autograd(lambda z: softmax_ce_compose(label, z, loss_weight), pred, loss_scale)
  return loss, dz, None


def softmax_ce_many(entries):
  """[(label, pred, loss_weight, loss_scale)] -> [(loss, dpred, extras)]: on the kernels, one launch for up to 8 heads
  (er_softmax_ce_multi); otherwise one softmax_ce each."""
  entries = list(entries)
  if len(entries) >= 2 and all(_on_kernels(p) and softmax_ce_fits(*p.shape) for _, p, _, _ in entries):
    out = []
    for i in range(0, len(entries), 8):
      heads = []
      for label, pred, loss_weight, loss_scale in entries[i:i + 8]:
        check_class_labels(label)
        weights, lw = _scalar_or_tensor(loss_weight)
        heads.append((pred.detach(), _f32_labels(label), weights, loss_scale * lw))
      out.extend((r['loss'], r['dlogits'], r) for r in kernels.hip().softmax_ce_multi(heads))
    return out
  return [softmax_ce(*e) for e in entries]


def check_jrc_param(loss_param):
  """Build-time refusals of a JRC loss -> (alpha, same_label_loss, session_name)"""
  if loss_param is None or not loss_param.session_name:
    raise ValueError('JRC_LOSS needs `jrc_loss { session_name }`: the feature whose ids are the session keys')
  strategy = loss_param.loss_weight_strategy
  if strategy not in JRC_STRATEGIES:
    raise ValueError('Unsupported loss weight strategy `%s` for jrc loss' % strategy)
  if strategy != 'fixed':
    raise NotImplementedError('jrc_loss { loss_weight_strategy: "%s" }: only the `fixed` strategy is built (the random '
                              'and `uncertainty` strategies are not)' % strategy)
  return float(loss_param.alpha), bool(loss_param.same_label_loss), loss_param.session_name


def jrc(label, pred, session_ids, loss_weight=1.0, loss_scale=1.0, alpha=0.5, same_label_loss=True):
  """-> (loss [1], d loss / d pred [B, 2], extras or None).  pred [B, 2]; session_ids [B] integer keys."""
  assert pred.dim() == 2 and pred.shape[1] == 2, 'num_class must be 2 when loss type is JRC_LOSS'
  if session_ids is None:
    raise ValueError('JRC_LOSS needs session ids')
  weights, lw = _scalar_or_tensor(loss_weight)
  B = pred.shape[0]
  if same_label_loss and _on_kernels(pred) and jrc_fits(B):
    keys = session_ids.to(torch.int64).contiguous()
    res = kernels.hip().jrc(pred.detach(), _f32_labels(label), keys, weights, alpha, ce_scale=lw,
                            loss_scale=loss_scale * lw)
    return res['loss'], res['dlogits'], res
  loss, dz = _by_autograd(lambda z: jrc_compose(label, z, session_ids, alpha, loss_weight if weights is not None else lw,
                                                same_label_loss), pred, loss_scale)
  return loss, dz, None
