"""The listwise ranking losses: reference loss/listwise_loss.py.

  LISTWISE_RANK_LOSS      listwise_rank_loss: softmax cross entropy over the candidates of one session (GAUC)
  LISTWISE_DISTILL_LOSS   listwise_distill_loss: the same against a teacher's rank positions

Both group the batch by the session keys `session_name` gives, take -sum(t * log_softmax(logits)) inside every session -
t the labels' softmax (label_is_logits), the labels as they are, or the transformed rank positions over their session's
sum - and average over the sessions.

Sample weights: the reference ignores a TENSOR of weights for these two losses (it logs an error and returns the plain
mean) and multiplies a python-scalar weight into the loss.  So does this module: a tensor is logged and dropped, a
scalar folds into the loss scale on the host.

`transform_fn` is resolved as the reference's load_by_path does (a `lambda` is evaluated, a dotted path located) and is
applied to the labels with torch ops on the host: it receives and returns a torch tensor.  A path that yields no callable
raises at build time with the path named.

`scale_logits` trains the variables `<loss_name>/scale_w` (ones) and `<loss_name>/scale_b` (zeros), logits * |scale_w| +
scale_b, where <loss_name> is what the reference's loss function opens its variable scope with: its own `name` default,
since its loss_builder passes none - `listwise_loss` for the rank loss, `listwise_distill_loss` for the distill loss.

Which path runs is decided by what the code can see.  On the HIP backend, with fp32 logits on the GPU and B inside the
kernel's envelope (include/easyrec_hip.h K8n), ONE launch (csrc/er_listwise.hip: an in-LDS sort by key, then segmented
scans) yields the loss - as the partial the loss tail's launch takes - d loss / d logits, the scale variables' gradient
partials and the session count, without a device-to-host read.  Beyond that envelope, 8192 < B <= 131072, and with
EASYREC_AMD_LISTWISE_TILED=1 the same outputs come from the tiled launches (K8o, er_listwise_tiled: a tile sort, merge
passes, three reduction stages with one carry record per workgroup), one row of partials per workgroup.  Anywhere else -
a stand-in backend on the CPU, a batch outside the envelopes, EASYREC_AMD_FUSED_LISTWISE=0 - the compositions below run:
the reference's forms op for op as torch ops (unique keys, one boolean mask per session), differentiated by autograd.
"""
import functools
import logging
import os
import pydoc

import torch

from easyrec_amd import kernels
from easyrec_amd.protos.loss_pb2 import LossType

FUSED_DEFAULT = '1'  # EASYREC_AMD_FUSED_LISTWISE when the environment does not set it
MAX_BATCH = 8192     # er_listwise: B
LOSS_TYPES = (LossType.LISTWISE_RANK_LOSS, LossType.LISTWISE_DISTILL_LOSS)
# the variable scope the reference's function opens (its `name` default)
SCOPES = {LossType.LISTWISE_RANK_LOSS: 'listwise_loss', LossType.LISTWISE_DISTILL_LOSS: 'listwise_distill_loss'}


def fused_enabled():
  """EASYREC_AMD_FUSED_LISTWISE=0: the torch compositions everywhere (the A/B switch of the K8n kernel)."""
  return os.environ.get('EASYREC_AMD_FUSED_LISTWISE', FUSED_DEFAULT) != '0'


def fits(B):
  return 1 <= B <= MAX_BATCH


TILED_DEFAULT = '0'        # EASYREC_AMD_LISTWISE_TILED when the environment does not set it
TILED_MAX_BATCH = 131072   # er_listwise_tiled: B
TILES = (1024, 2048, 4096, 8192)
DEFAULT_TILE = 1024        # what tile = 0 selects


def tiled_enabled():
  """EASYREC_AMD_LISTWISE_TILED=1: batches beyond er_listwise's envelope run on er_listwise_tiled (K8o), not on the
  compositions."""
  return os.environ.get('EASYREC_AMD_LISTWISE_TILED', TILED_DEFAULT) != '0'


def fits_tiled(B):
  return MAX_BATCH < B <= TILED_MAX_BATCH


def tiled_grid(B, tile=0):
  """er_listwise_tiled_grid: the workgroups, one row of partials each; 0 outside the envelope"""
  if tile == 0:
    tile = DEFAULT_TILE if fits_tiled(B) else -1
  return -(-B // tile) if tile in TILES and 1 <= B <= TILED_MAX_BATCH else 0


def tiled_workspace_bytes(B, tile=0):
  """er_listwise_tiled_workspace_bytes: two buffers of G T records of 12 bytes and 16 words of carry per workgroup"""
  G = tiled_grid(B, tile)
  return G * (tile or DEFAULT_TILE) * 24 + G * 64


@functools.lru_cache(maxsize=None)
def load_transform(path):
  """reference utils/load_class.py load_by_path -> a callable; raises where the reference would go on with None"""
  stripped = path.strip()
  fn = None
  if 'lambda' in stripped:
    fn = eval(stripped)  # (the reference's own rule for a lambda in a config)
  elif stripped:
    parts = stripped.split('.')
    if parts[0] == 'tf':
      parts[0] = 'tensorflow'
    try:
      fn = pydoc.locate('.'.join(parts))
    except pydoc.ErrorDuringImport:
      fn = None
  if not callable(fn):
    raise ValueError('listwise loss: transform_fn "%s" does not import to a callable (it runs on torch tensors here)' % path)
  return fn


def params_of(loss_type, loss_param):
  """The reference's keyword arguments for `loss_type` (builders/loss_builder.py:162-197: its defaults without a
  loss_param) -> dict; build-time refusals raise here."""
  assert loss_type in LOSS_TYPES
  p = dict(temperature=1.0, session_name='', transform_fn=None, label_is_logits=False, label_clip_max=512.0,
           scale_logits=False, scope=SCOPES[loss_type])
  if loss_param is not None:
    p.update(temperature=float(loss_param.temperature), session_name=loss_param.session_name,
             scale_logits=bool(loss_param.scale_logits))
    if loss_param.HasField('transform_fn'):
      p['transform_fn'] = load_transform(loss_param.transform_fn)
    if loss_type == LossType.LISTWISE_RANK_LOSS:
      p['label_is_logits'] = bool(loss_param.label_is_logits)
    else:
      p['label_clip_max'] = float(loss_param.label_clip_max_value)
  if not p['session_name']:
    raise ValueError('%s needs a session_name: the reference squeezes the session ids it is given, and None fails there' %
                     LossType.Name(loss_type).lower())
  return p


def scale_variables(p):
  """(scale_w, scale_b) of params_of's dict, (None, None) without scale_logits.  Created in the build pass
  (RankModel._check_head), fetched afterwards."""
  if not p['scale_logits']:
    return None, None
  from easyrec_amd.core import context
  vs = context.varstore()
  return vs.get_variable(p['scope'] + '/scale_w', (1,), 'ones'), vs.get_variable(p['scope'] + '/scale_b', (1,), 'zeros')


# ------------------------------------------------------------------------------------------------ the torch compositions
def _rank_labels(y, p):
  """listwise_rank_loss' label steps: the temperature under label_is_logits, then transform_fn"""
  if p['temperature'] != 1.0 and p['label_is_logits']:
    y = y / p['temperature']
  return p['transform_fn'](y) if p['transform_fn'] is not None else y


def _distill_labels(y, p):
  """listwise_distill_loss' label steps: the clip, then transform_fn or log1p(clip max) - log"""
  y = torch.clamp(y, 1, p['label_clip_max'])
  if p['transform_fn'] is not None:
    return p['transform_fn'](y)
  return torch.log1p(torch.tensor(p['label_clip_max'], dtype=y.dtype, device=y.device)) - torch.log(y)


def compose(loss_type, labels, logits, session_ids, p, scale_w=None, scale_b=None):
  """listwise_loss.py:28-94 / :97-161 -> scalar: tf.unique over the session ids, tf.map_fn of the masked softmax cross
  entropy over the sessions, tf.reduce_mean.  (torch.unique sorts where tf.unique keeps first occurrences: the mean adds
  the same terms in another order.)"""
  y = labels.to(logits.dtype)
  z = logits
  if loss_type == LossType.LISTWISE_DISTILL_LOSS:
    y = _distill_labels(y, p)
  if scale_w is not None:
    z = z * torch.abs(scale_w) + scale_b
  if p['temperature'] != 1.0:
    z = z / p['temperature']
  if loss_type == LossType.LISTWISE_RANK_LOSS:
    y = _rank_labels(y, p)
  ids = session_ids.reshape(-1)
  losses = []
  for x in torch.unique(ids):
    mask = ids == x
    zs, ys = z[mask], y[mask]
    if loss_type == LossType.LISTWISE_DISTILL_LOSS:
      ys = ys / ys.sum()
    elif p['label_is_logits']:
      ys = torch.softmax(ys, dim=0)
    losses.append(-(ys * torch.log_softmax(zs, dim=0)).sum())
  return torch.stack(losses).mean()


# ------------------------------------------------------------------------------------------------ the kernel path
def kernel_args(loss_type, labels, p):
  """params_of's dict and the fp32 labels -> (labels for the launch, er_listwise's keyword arguments).  With a
  transform_fn the label steps run here with torch ops and the launch is told so (K8n ER_LIST_LABEL_READY)."""
  rank = loss_type == LossType.LISTWISE_RANK_LOSS
  flags = kernels.LIST_LABEL_IS_LOGITS if rank and p['label_is_logits'] else 0
  if p['transform_fn'] is not None:
    labels = (_rank_labels(labels, p) if rank else _distill_labels(labels, p)).to(torch.float32)
    flags |= kernels.LIST_LABEL_READY
  return labels.contiguous(), dict(kind=kernels.LIST_RANK if rank else kernels.LIST_DISTILL, flags=flags,
                                   temperature=p['temperature'], label_clip_max=p['label_clip_max'])


def on_kernel(pred, p):
  return fused_enabled() and pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 1 and fits(pred.shape[0]) and \
      p['temperature'] > 0 and isinstance(kernels.hip(), kernels.HipBackend)


def on_tiled_kernel(pred, p):
  """the second branch: beyond er_listwise's envelope, inside er_listwise_tiled's, and switched on"""
  return fused_enabled() and tiled_enabled() and pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 1 and \
      fits_tiled(pred.shape[0]) and p['temperature'] > 0 and isinstance(kernels.hip(), kernels.HipBackend)


def fused(loss_type, labels, logits, session_ids, p, scale_w=None, scale_b=None, loss_scale=1.0, tile=None):
  """The autograd function over er_listwise -> (loss [1], num_sessions [1] int32); differentiable in logits, scale_w and
  scale_b.  tile: er_listwise_tiled at that tile (0: its default); None: by the batch size as build() chooses."""
  y, kw = kernel_args(loss_type, labels.to(torch.float32), p)
  if tile is None and not on_kernel(logits, p) and on_tiled_kernel(logits, p):
    tile = 0
  if tile is not None:
    kw['tile'] = tile
  return kernels.ListwiseLossFn.apply(logits, y, session_ids.to(torch.int64).contiguous(), dict(loss_scale=loss_scale, **kw),
                                      scale_w, scale_b)


def _grad_buffers(variables):
  """The variables' gradient buffers (their slices of the flat buffer once the store is packed; zeros of their own for a
  caller without a packed store, as autograd would leave them)."""
  for v in variables:
    if v.grad is None:
      v.grad = torch.zeros_like(v)
  return [v.grad for v in variables]


def build(loss_type, label, pred, loss_weight=1.0, loss_scale=1.0, loss_param=None, session_ids=None, scale_vars=None):
  """-> (loss [1], d loss / d pred [B], extras: the launch's outputs - the session count among them - or None).  pred
  [B].  scale_vars: (scale_w, scale_b) when the caller holds them, else the variable store's under scale_logits; their
  gradients are ADDED into their .grad buffers."""
  p = params_of(loss_type, loss_param)
  assert session_ids is not None, '%s: no session ids for session_name "%s"' % (LossType.Name(loss_type), p['session_name'])
  if torch.is_tensor(loss_weight):
    logging.error('[%s] use unsupported sample weight' % p['scope'])
    loss_weight = 1.0
  scale = loss_scale * float(loss_weight)
  sw, sb = scale_vars if scale_vars is not None else scale_variables(p)
  tiled = not on_kernel(pred, p) and on_tiled_kernel(pred, p)
  if on_kernel(pred, p) or tiled:
    labels, kw = kernel_args(loss_type, label if label.dtype == torch.float32 else label.to(torch.float32), p)
    grads = None if sw is None else kernels.ThetaGradTable(_grad_buffers((sw, sb)))
    launch = kernels.hip().listwise_loss_tiled if tiled else kernels.hip().listwise_loss
    res = launch(pred.detach(), labels, session_ids.to(torch.int64).contiguous(),
                 scale_w=None if sw is None else sw.detach(), scale_b=None if sb is None else sb.detach(),
                 loss_scale=scale, grads=grads, acc=True, **kw)
    return res['loss'], res['dlogits'], res
  z = pred.detach().clone().requires_grad_(True)
  with torch.enable_grad():
    loss = compose(loss_type, label, z, session_ids, p, sw, sb) * scale
    grads = torch.autograd.grad(loss, [z] if sw is None else [z, sw, sb])
  if sw is not None:
    for buf, g in zip(_grad_buffers((sw, sb)), grads[1:]):
      buf.add_(g)
  return loss.detach().reshape(1), grads[0], None
