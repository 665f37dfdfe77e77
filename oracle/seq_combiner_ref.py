"""fp64 torch restatements of the two sequence combiners (TextCNN, attention pooling): what the model oracle
(oracle/model_oracle.py: input_layer's sequence_combiner columns, the backbone's TextCNN block) and the kernels' tests
read.

text_cnn_ref is written from the definition (windows gathered by index, an einsum per filter size), not from conv1d, so
that it does not share code with the composition it checks.  `select`: evaluate chosen outputs (b, f) under a GIVEN
selection of window positions (a weight per position, summing to 1) and a given ReLU decision instead of fp64's own
arg-max: what a test does where fp64's top two candidates lie too close for fp32 to be held to fp64's choice."""
import torch

MASKED_LOGIT = float(-2 ** 32 + 1)


def pad_or_truncate(x, P):
  B, L, D = x.shape
  if L >= P:
    return x[:, :P]
  return torch.cat([x, torch.zeros(B, P - L, D, dtype=x.dtype)], dim=1)


def text_cnn_pre(x, P, kernels, biases):
  """-> per filter size the pre-activations [B, P - k + 1, F]; x [B, L, D] padded / truncated to P (P <= 0: as it is)."""
  xp = pad_or_truncate(x, P) if P > 0 else x
  n_pos = xp.shape[1]
  out = []
  for w, b in zip(kernels, biases):
    k = w.shape[0]
    idx = torch.arange(n_pos - k + 1)[:, None] + torch.arange(k)[None, :]  # [np, k]
    win = xp[:, idx]  # [B, np, k, D]
    out.append(torch.einsum('bpjd,jdf->bpf', win, w) + b)
  return out


def _act(z, act):
  if act in (None, '', 'linear'):
    return z
  return {'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[act](z)


def text_cnn_ref(x, P, kernels, biases, act='relu', select=None):
  """-> y [B, sum F].  select = (override bool [B, sum F], weight [B, sum F, max positions], active bool [B, sum F]):
  where override, y = active * sum_p weight_p pre_p (the gradient reaches exactly the given positions, through the
  ReLU only where `active`)."""
  pres = text_cnn_pre(x, P, kernels, biases)
  ys, c0 = [], 0
  for pre in pres:
    y = _act(pre, act).amax(dim=1)  # [B, F]
    F, n_pos = pre.shape[2], pre.shape[1]
    if select is not None:
      over, weight, active = select
      w = weight[:, c0:c0 + F, :n_pos].transpose(1, 2)  # [B, np, F]
      forced = (w * pre).sum(dim=1) * active[:, c0:c0 + F].to(pre.dtype)
      y = torch.where(over[:, c0:c0 + F], forced, y)
    ys.append(y)
    c0 += F
  return torch.cat(ys, dim=-1)


def near_ties(x, P, kernels, biases, act, tol):
  """bool [B, sum F]: outputs whose fp64 top two window values, or whose maximum and 0 under relu, lie within tol.  Under
  relu an output whose windows all lie below -tol is 0 with no gradient under any selection: not a near tie."""
  out = []
  for pre in text_cnn_pre(x, P, kernels, biases):
    if pre.shape[1] > 1:
      top = pre.topk(2, dim=1).values
      near = (top[:, 0] - top[:, 1]) <= tol
    else:
      near = torch.zeros(pre.shape[0], pre.shape[2], dtype=torch.bool)
    if act == 'relu':
      m = pre.amax(dim=1)
      near = (near | (m.abs() <= tol)) & (m >= -tol)
    out.append(near)
  return torch.cat(out, dim=-1)


def seq_attn_pool_ref(x, lens, w):
  """x [B, L, D], lens [B], w [D] or [D, 1] -> [B, D]; a masked logit is the constant (no gradient to <x_t, w> there)."""
  logits = (x * w.reshape(-1)).sum(dim=-1)
  mask = torch.arange(x.shape[1])[None, :] < lens.to(torch.int64)[:, None]
  logits = torch.where(mask, logits, torch.full_like(logits, MASKED_LOGIT))
  p = torch.softmax(logits, dim=-1)
  return (p[:, :, None] * x).sum(dim=1)
