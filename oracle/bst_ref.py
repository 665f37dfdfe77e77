"""ORACLE - TEST INFRASTRUCTURE ONLY.  Never imported by easyrec_amd/.

A torch restatement of the BST block (reference model/multi_tower_bst.py:78-151, layers/layer_norm.py:28-37), written
op by op like the reference graph: the kernels' and the model's yardstick.  Any dtype / device.

  bst_block(key [B, E], hist [B, L, E], seq_len [B], T, H, params) -> [B, T * E]
with params the dict {name: tensor} of layers/bst.py's variable names (LayerNorms under ln names ln_names)."""
import math

import torch


def head_split(E, H):
  p = int(math.ceil(E / float(H)))
  return [(s, min(p, E - s)) for s in range(0, E, p)]


def _dense(x, params, scope):
  return x @ params['%s/%s_0/kernel' % (scope, scope)] + params['%s/%s_0/bias' % (scope, scope)]


def _layer_norm(x, scale, bias, eps=1e-6):
  mean = x.mean(dim=-1, keepdim=True)
  var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
  return (x - mean) * torch.rsqrt(var + eps) * scale + bias


def sequence(key, hist, T):
  """The reference's pad / slice of the history to T - 1 rows (:131-138) with the key appended (:139-140)."""
  B, L, E = hist.shape
  if T - 1 > L:
    hist = torch.cat([hist, hist.new_zeros(B, T - 1 - L, E)], dim=1)
  else:
    hist = hist[:, :T - 1]
  return torch.cat([hist, key[:, None, :]], dim=1)


def bst_block(key, hist, seq_len, T, H, params, ln_names=('layer_normalization', 'layer_normalization_1')):
  X = sequence(key, hist, T)
  B, _, E = X.shape
  hist_mask = torch.arange(T - 1, device=X.device)[None, :] < seq_len.to(torch.int64)[:, None]  # sequence_mask (:85-86)
  mask = torch.cat([hist_mask, torch.ones(B, 1, dtype=torch.bool, device=X.device)], dim=1)[:, None, :]
  outs = []
  for s, w in head_split(E, H):
    part = X[:, :, s:s + w]
    q = _dense(part, params, 'multi_head_%d_query' % s)
    k = _dense(part, params, 'multi_head_%d_key' % s)
    v = _dense(part, params, 'multi_head_%d_value' % s)
    scores = q @ k.transpose(1, 2)  # no scaling (:95)
    scores = torch.where(mask, scores, torch.full_like(scores, -2.0 ** 32 + 1))
    outs.append(torch.softmax(scores, dim=-1) @ v)
  att = _dense(torch.cat(outs, dim=2), params, 'multi_head_attention')
  ln1, ln2 = ln_names
  y1 = _layer_norm(X + att, params[ln1 + '/layer_norm_scale'], params[ln1 + '/layer_norm_bias'])
  y2 = _layer_norm(y1 + _dense(y1, params, 'feed_forward_net'), params[ln2 + '/layer_norm_scale'],
                   params[ln2 + '/layer_norm_bias'])
  return y2.reshape(B, T * E)


def unpack(theta, E, H, ln_names=('layer_normalization', 'layer_normalization_1')):
  """The kernels' packed parameter vector -> {name: view} (easyrec_hip.h K8b)."""
  heads = dict(head_split(E, H))
  out, o = {}, 0
  for n in param_names(E, H, ln_names):
    scope = n.split('/')[0]
    if scope.startswith('multi_head_') and scope != 'multi_head_attention':
      w = heads[int(scope.split('_')[2])]
      shape = (w, w) if n.endswith('kernel') else (w,)
    else:
      shape = (E, E) if n.endswith('kernel') else (E,)
    k = 1
    for d in shape:
      k *= d
    out[n] = theta[o:o + k].view(shape)
    o += k
  assert o == theta.numel()
  return out


def param_count(E, H):
  heads = head_split(E, H)
  return 3 * (sum(w * w for _, w in heads) + E) + 2 * (E * E + E) + 4 * E


def param_names(E, H, ln_names=('layer_normalization', 'layer_normalization_1')):
  """Names in the kernels' packed order (easyrec_hip.h K8b)."""
  heads = head_split(E, H)
  names = []
  for kind in ('query', 'key', 'value'):
    names += ['multi_head_%d_%s/multi_head_%d_%s_0/kernel' % (s, kind, s, kind) for s, _ in heads]
    names += ['multi_head_%d_%s/multi_head_%d_%s_0/bias' % (s, kind, s, kind) for s, _ in heads]
  for scope in ('multi_head_attention', 'feed_forward_net'):
    names += ['%s/%s_0/kernel' % (scope, scope), '%s/%s_0/bias' % (scope, scope)]
  for ln in ln_names:
    names += [ln + '/layer_norm_scale', ln + '/layer_norm_bias']
  return names


def random_case(B, L, T, E, H, seed, lengths=None, device='cpu', dtype=torch.float64):
  """Inputs as the lookup leaves them (rows t >= len zero) and non-trivial parameters (LayerNorm scales / biases off
  their ones / zeros initial values, so their gradients are exercised)."""
  g = torch.Generator().manual_seed(seed)
  if lengths is None:
    lengths = torch.randint(0, L + 3, (B,), generator=g)
  lengths = torch.as_tensor(lengths, dtype=torch.int32)
  hist = torch.randn(B, L, E, generator=g, dtype=torch.float64)
  hist = hist * (torch.arange(L)[None, :, None] < lengths.clamp(max=L)[:, None, None].to(torch.int64))
  key = torch.randn(B, E, generator=g, dtype=torch.float64)
  params = {}
  heads = dict((s, w) for s, w in head_split(E, H))
  for n in param_names(E, H):
    scope = n.split('/')[0]
    if scope.startswith('multi_head_') and scope != 'multi_head_attention':
      w = heads[int(scope.split('_')[2])]
      shape = (w, w) if n.endswith('kernel') else (w,)
    else:
      shape = (E, E) if n.endswith('kernel') else (E,)
    if n.endswith('kernel'):
      t = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1
      t = t * math.sqrt(6.0 / (shape[0] + shape[1]))
    elif n.endswith('layer_norm_scale'):
      t = 1.0 + 0.2 * torch.randn(shape, generator=g, dtype=torch.float64)
    else:
      t = 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
    params[n] = t
  cast = lambda t: t.to(device=device, dtype=dtype)
  return cast(key), cast(hist), lengths.to(device), {n: cast(t) for n, t in params.items()}
