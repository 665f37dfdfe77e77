"""The pairwise ranking losses: reference loss/pairwise_loss.py.

  PAIR_WISE_LOSS           pairwise_loss (deprecated there, and the one its sample configs name)
  PAIRWISE_LOGISTIC_LOSS   pairwise_logistic_loss (RankNet)
  PAIRWISE_HINGE_LOSS      pairwise_hinge_loss
  PAIRWISE_FOCAL_LOSS      pairwise_focal_loss, through loss/focal_loss.py sigmoid_focal_loss_with_logits

All four run over the ordered pairs (i, j) with label_i > label_j, of one session when `session_name` gives keys (the
loss then optimises GAUC); per-example weights weigh the pairs of their FIRST member; the reduction is
SUM_BY_NONZERO_WEIGHTS with the safe division (no pair: loss 0).

Which path runs is decided by what the code can see.  On the HIP backend, with fp32 logits on the GPU, ohem_ratio == 1 and
B inside the kernel's envelope (include/easyrec_hip.h K8m), two launches (csrc/er_pairwise.hip) yield the loss - as
partial sums that the loss tail's launch finishes - d loss / d logits and the pair count in O(B) memory.  Beyond that
envelope, 8192 < B <= 131072, and with EASYREC_AMD_PAIRWISE_SORTED=1 the same outputs come from the sorted-run launches
(K8p, er_pairwise_sorted: K8o's sort by session key, then one lane per sorted row over its session's columns alone), the
pair count as int64.  Anywhere else -
a stand-in backend on the CPU, ohem_ratio < 1, a batch outside the envelopes, EASYREC_AMD_FUSED_PAIRWISE=0 - the
compositions below run: the reference's forms op for op as torch ops ([B, B] differences and masks, a boolean-mask
gather), differentiated by autograd.

A python-scalar sample weight multiplies the reduced loss in every one of the reference's forms (tf.losses broadcasts
it; focal multiplies its weights by it), so it folds into the loss scale on the host.
"""
import os

import torch

from easyrec_amd import kernels
from easyrec_amd.protos.loss_pb2 import LossType

FUSED_DEFAULT = '1'  # EASYREC_AMD_FUSED_PAIRWISE when the environment does not set it
MAX_BATCH = 8192     # er_pairwise: B
LOSS_TYPES = (LossType.PAIR_WISE_LOSS, LossType.PAIRWISE_LOGISTIC_LOSS, LossType.PAIRWISE_HINGE_LOSS,
              LossType.PAIRWISE_FOCAL_LOSS)


def fused_enabled():
  """EASYREC_AMD_FUSED_PAIRWISE=0: the torch compositions everywhere (the A/B switch of the K8m kernel)."""
  return os.environ.get('EASYREC_AMD_FUSED_PAIRWISE', FUSED_DEFAULT) != '0'


def fits(B):
  return 1 <= B <= MAX_BATCH


SORTED_DEFAULT = '1'      # EASYREC_AMD_PAIRWISE_SORTED when the environment does not set it
MAX_BATCH_SORTED = 131072  # er_pairwise_sorted: B
TILES = (1024, 2048, 4096, 8192)
DEFAULT_TILE = 1024        # what tile = 0 selects


def sorted_enabled():
  """EASYREC_AMD_PAIRWISE_SORTED=1: batches beyond er_pairwise's envelope run on er_pairwise_sorted (K8p), not on the
  compositions."""
  return os.environ.get('EASYREC_AMD_PAIRWISE_SORTED', SORTED_DEFAULT) != '0'


def fits_sorted(B):
  return MAX_BATCH < B <= MAX_BATCH_SORTED


def sorted_grid(B, tile=0):
  """er_pairwise_sorted_grid: the workgroups of 256 sorted rows, one row of partials each; 0 outside the envelope"""
  inside = fits_sorted(B) if tile == 0 else (tile in TILES and 1 <= B <= MAX_BATCH_SORTED)
  return -(-B // 256) if inside else 0


def sorted_workspace_bytes(B, tile=0):
  """er_pairwise_sorted_workspace_bytes: the sort's two buffers of G T records of 12 bytes, 24 bytes per example (column
  record, hi, sorted dz) and 20 per workgroup"""
  rows = sorted_grid(B, tile)
  T = tile or DEFAULT_TILE
  return -(-B // T) * T * 24 + 24 * B + 20 * rows if rows else 0


def params_of(loss_type, loss_param):
  """The reference's keyword arguments for `loss_type` (builders/loss_builder.py:90-161: its defaults without a
  loss_param, HasField for the optional margins) -> dict; build-time refusals raise here."""
  p = dict(temperature=1.0, ohem_ratio=1.0, margin=0.0, hinge_margin=None, use_label_margin=False, label_is_logits=True,
           gamma=2.0, alpha=None, session_name='')
  if loss_type == LossType.PAIRWISE_HINGE_LOSS:
    p.update(margin=1.0, use_label_margin=True)
  if loss_param is not None:
    p['session_name'] = loss_param.session_name
    p['temperature'] = float(loss_param.temperature)
    if loss_type == LossType.PAIR_WISE_LOSS:
      p['margin'] = float(loss_param.margin)
    else:
      p['ohem_ratio'] = float(loss_param.ohem_ratio)
    if loss_type in (LossType.PAIRWISE_LOGISTIC_LOSS, LossType.PAIRWISE_FOCAL_LOSS) and loss_param.HasField('hinge_margin'):
      p['hinge_margin'] = float(loss_param.hinge_margin)
    if loss_type == LossType.PAIRWISE_LOGISTIC_LOSS:
      p['use_label_margin'] = bool(loss_param.use_label_margin)
    if loss_type == LossType.PAIRWISE_HINGE_LOSS:
      p.update(margin=float(loss_param.margin), use_label_margin=bool(loss_param.use_label_margin),
               label_is_logits=bool(loss_param.label_is_logits))
      if loss_param.use_exponent:
        raise NotImplementedError('pairwise_hinge_loss { use_exponent: true } is not built: the reference\'s form overwrites '
                                  'the logits with sigmoid(labels), so the loss no longer depends on the model')
    if loss_type == LossType.PAIRWISE_FOCAL_LOSS:
      p['gamma'] = float(loss_param.gamma)
      p['alpha'] = float(loss_param.alpha) if loss_param.HasField('alpha') else None
      if p['gamma'] < 0:
        raise ValueError('Value of gamma should be greater than or equal to zero')
  name = LossType.Name(loss_type).lower()
  assert 0 < p['ohem_ratio'] <= 1.0, name + ' ohem_ratio must be in (0, 1]'
  return p


# ------------------------------------------------------------------------------------------------ the torch compositions
def _softplus_neg(x):
  """tf.nn.sigmoid_cross_entropy_with_logits(labels = 1, logits = x) in its own form: softplus(-x), with the exact
  derivative -1 / 2 at x == 0"""
  pos = x >= 0
  return torch.where(pos, x, torch.zeros_like(x)) - x + torch.log1p(torch.exp(torch.where(pos, -x, x)))


def _pair_mask(labels, session_ids):
  mask = labels[:, None] > labels[None, :]
  if session_ids is not None:
    mask = mask & (session_ids[:, None] == session_ids[None, :])
  return mask


def _pair_weights(weights, mask, dtype):
  """tf.tile(expand_dims(weights, -1), [1, B]) under the mask: the FIRST member's weight; None without a tensor"""
  if not torch.is_tensor(weights):
    return None
  return weights.to(dtype)[:, None].expand(mask.shape)[mask]


def _reduce(per, w, ohem_ratio=1.0):
  """compute_weighted_loss(per, w) with SUM_BY_NONZERO_WEIGHTS, or - ohem_ratio < 1 - the mean of the positive ones
  among the round(n * ohem_ratio) largest weighted losses"""
  if ohem_ratio == 1.0:
    if w is None:
      return per.sum() / max(int(per.numel()), 1)
    return (w * per).sum() / (w != 0).sum().clamp(min=1).to(per.dtype)
  losses = per if w is None else per * w
  k = int(torch.round(torch.tensor(float(losses.numel()) * ohem_ratio)).item())
  top = torch.topk(losses, k).values
  return top[top > 0].mean()


def pair_wise_compose(labels, logits, session_ids=None, margin=0.0, temperature=1.0, weights=None):
  """pairwise_loss.py:15-70 -> scalar"""
  y = labels.to(logits.dtype)
  z = logits / temperature if temperature != 1.0 else logits
  mask = _pair_mask(y, session_ids)
  x = (z[:, None] - z[None, :] - margin)[mask]
  return _reduce(_softplus_neg(x), _pair_weights(weights, mask, z.dtype))


def logistic_compose(labels, logits, session_ids=None, temperature=1.0, hinge_margin=None, weights=None, ohem_ratio=1.0,
                     use_label_margin=False):
  """pairwise_loss.py:128-210 -> scalar"""
  y = labels.to(logits.dtype)
  z = logits
  if temperature != 1.0:
    z = z / temperature
    if use_label_margin:
      y = y / temperature
  x = z[:, None] - z[None, :]
  if use_label_margin:
    x = x - (y[:, None] - y[None, :])
  elif hinge_margin is not None:
    x = x - hinge_margin
  mask = _pair_mask(y, session_ids)
  x = x[mask]
  # (the reference's own spelling of softplus(-x); through relu and abs its derivative at x == 0 is 0, not -1 / 2)
  per = torch.relu(-x) + torch.log1p(torch.exp(-torch.abs(x)))
  return _reduce(per, _pair_weights(weights, mask, z.dtype), ohem_ratio)


def hinge_compose(labels, logits, session_ids=None, temperature=1.0, margin=1.0, weights=None, ohem_ratio=1.0,
                  label_is_logits=True, use_label_margin=True):
  """pairwise_loss.py:213-307 without use_exponent -> scalar"""
  y = labels.to(logits.dtype)
  z = logits
  if temperature != 1.0:
    z = z / temperature
    if label_is_logits:
      y = y / temperature
  mask = _pair_mask(y, session_ids)
  pair_logits = (z[:, None] - z[None, :])[mask]
  diff = ((y[:, None] - y[None, :])[mask] if use_label_margin else margin) - pair_logits
  return _reduce(torch.relu(diff), _pair_weights(weights, mask, z.dtype), ohem_ratio)


def focal_compose(labels, logits, session_ids=None, hinge_margin=None, gamma=2.0, alpha=None, ohem_ratio=1.0,
                  temperature=1.0, weights=None):
  """pairwise_loss.py:73-125 and focal_loss.py:11-93 at labels = 1 -> scalar.  The modulating weights (1 - p)^gamma are a
  function of the logits and the reference stops no gradient there: autograd carries that term; the divisor is a count."""
  y = labels.to(logits.dtype)
  z = logits / temperature if temperature != 1.0 else logits
  pair_logits = z[:, None] - z[None, :]
  mask = y[:, None] > y[None, :]
  if hinge_margin is not None:
    mask = mask & (pair_logits < hinge_margin)
  if session_ids is not None:
    mask = mask & (session_ids[:, None] == session_ids[None, :])
  x = pair_logits[mask]
  p = torch.sigmoid(x).clamp(1e-7, 1 - 1e-7)
  w = torch.pow(1 - p, gamma)
  if alpha is not None:
    w = w * alpha
  pw = _pair_weights(weights, mask, z.dtype)
  if pw is not None:
    w = w * pw
  return _reduce(_softplus_neg(x), w, ohem_ratio)


def compose(loss_type, labels, logits, session_ids, weights, p):
  """The composition of `loss_type` under params_of's dict -> scalar"""
  if loss_type == LossType.PAIR_WISE_LOSS:
    return pair_wise_compose(labels, logits, session_ids, p['margin'], p['temperature'], weights)
  if loss_type == LossType.PAIRWISE_LOGISTIC_LOSS:
    return logistic_compose(labels, logits, session_ids, p['temperature'], p['hinge_margin'], weights, p['ohem_ratio'],
                            p['use_label_margin'])
  if loss_type == LossType.PAIRWISE_HINGE_LOSS:
    return hinge_compose(labels, logits, session_ids, p['temperature'], p['margin'], weights, p['ohem_ratio'],
                         p['label_is_logits'], p['use_label_margin'])
  assert loss_type == LossType.PAIRWISE_FOCAL_LOSS
  return focal_compose(labels, logits, session_ids, p['hinge_margin'], p['gamma'], p['alpha'], p['ohem_ratio'],
                       p['temperature'], weights)


# ------------------------------------------------------------------------------------------------ what loss_builder calls
def kernel_args(loss_type, p):
  """params_of's dict -> er_pairwise's keyword arguments (the reference's options folded as K8m states)"""
  T = p['temperature']
  if loss_type == LossType.PAIR_WISE_LOSS:
    return dict(kind=kernels.PAIR_WISE, temperature=T, margin=p['margin'])
  if loss_type == LossType.PAIRWISE_LOGISTIC_LOSS:
    if p['use_label_margin']:
      return dict(kind=kernels.PAIR_LOGISTIC, flags=kernels.PAIR_LABEL_MARGIN, temperature=T, label_div=T)
    return dict(kind=kernels.PAIR_LOGISTIC, temperature=T, margin=p['hinge_margin'] or 0.0)
  if loss_type == LossType.PAIRWISE_HINGE_LOSS:
    return dict(kind=kernels.PAIR_HINGE, flags=kernels.PAIR_LABEL_MARGIN if p['use_label_margin'] else 0, temperature=T,
                label_div=T if p['label_is_logits'] else 1.0, margin=p['margin'])
  flags = (kernels.PAIR_HINGE_MARGIN if p['hinge_margin'] is not None else 0) | (kernels.PAIR_ALPHA if p['alpha'] is not None else 0)
  return dict(kind=kernels.PAIR_FOCAL, flags=flags, temperature=T, hinge_margin=p['hinge_margin'] or 0.0, gamma=p['gamma'],
              alpha=p['alpha'] or 0.0)


def _on_kernel(pred, p):
  return fused_enabled() and pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 1 and fits(pred.shape[0]) and \
      p['ohem_ratio'] == 1.0 and p['temperature'] > 0 and isinstance(kernels.hip(), kernels.HipBackend)


def _on_sorted_kernel(pred, p):
  """the second branch: beyond er_pairwise's envelope, inside er_pairwise_sorted's, and switched on"""
  return fused_enabled() and sorted_enabled() and pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 1 and \
      fits_sorted(pred.shape[0]) and p['ohem_ratio'] == 1.0 and p['temperature'] > 0 and \
      isinstance(kernels.hip(), kernels.HipBackend)


def build(loss_type, label, pred, loss_weight=1.0, loss_scale=1.0, loss_param=None, session_ids=None):
  """-> (loss [1], d loss / d pred [B], extras: the launch's outputs - the pair count among them - or None).  pred [B]."""
  p = params_of(loss_type, loss_param)
  weights = loss_weight if torch.is_tensor(loss_weight) else None
  scale = loss_scale * (1.0 if weights is not None else float(loss_weight))
  on_sorted = not _on_kernel(pred, p) and _on_sorted_kernel(pred, p)
  if _on_kernel(pred, p) or on_sorted:
    labels = (label if label.dtype == torch.float32 else label.to(torch.float32)).contiguous()
    keys = None if session_ids is None else session_ids.to(torch.int64).contiguous()
    launch = kernels.hip().pairwise_loss_sorted if on_sorted else kernels.hip().pairwise_loss
    res = launch(pred.detach(), labels, keys, None if weights is None else weights.contiguous(), loss_scale=scale,
                 **kernel_args(loss_type, p))
    return res['loss'], res['dlogits'], res
  z = pred.detach().clone().requires_grad_(True)
  with torch.enable_grad():
    loss = compose(loss_type, label, z, session_ids, weights, p) * scale
    dz, = torch.autograd.grad(loss, z)
  return loss.detach().reshape(1), dz, None
