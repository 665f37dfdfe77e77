"""ORACLE - TEST INFRASTRUCTURE ONLY.  Never imported by easyrec_amd/.

A torch restatement of AutoInt's interacting layers (reference layers/multihead_attention.py:50-161 with use_res,
model/autoint.py:54-75), written op by op like the reference graph: the kernels' and the model's yardstick.  Any dtype
/ device.

  mha_layer(x [B, F, d_in], H, ds, params, name) -> [B, F, H * ds]
  autoint_logits(x [B, F * D], F, D, H, ds, layers, params) -> [B, num_class]
with params the dict {name: tensor} of the reference's variable names."""
import math

import torch


def names(name):
  """The layer's variables in the packed operand's order (layers/multihead_attention.py variable_names)."""
  return ['%s/query/dnn/kernel' % name, '%s/key/dnn/kernel' % name, '%s/value/dnn/kernel' % name, '%s/dnn/kernel' % name]


def layer_name(i):
  return 'multi_head_self_attention_layer_%d' % i


def attention_core(q, k, v, r, H, ds, mask=None):
  """[B, F, d] each -> relu(concat_h softmax(Q_h K_h^T / ds ** -0.5) V_h + R).  mask: the ReLU's pattern given
  ((O + R) * mask: a gradient check through another computation's ReLU pattern, where O + R is within rounding of 0)."""
  B, F, _ = q.shape

  def split(t):  # _split_multihead_qkv: [B, F, H, ds] -> [B, H, F, ds]
    return t.reshape(B, F, H, ds).permute(0, 2, 1, 3)

  qh, kh, vh = split(q), split(k), split(v)
  product = (qh @ kh.transpose(-1, -2)) / (ds ** -0.5)  # (:67-69: a product by sqrt(ds))
  out = torch.softmax(product, dim=-1) @ vh
  out = out.permute(0, 2, 1, 3).reshape(B, F, H * ds)  # _combine_heads
  return torch.relu(out + r) if mask is None else (out + r) * mask


def mha_layer(x, H, ds, params, name, mask=None):
  wq, wk, wv, wr = [params[n] for n in names(name)]
  return attention_core(x @ wq, x @ wk, x @ wv, x @ wr, H, ds, mask)


def autoint_logits(x, F, D, H, ds, layers, params):
  B = x.shape[0]
  fea = x.reshape(B, F, D)
  for i in range(layers):
    fea = mha_layer(fea, H, ds, params, layer_name(i))
  fea = fea.reshape(B, -1)
  return fea @ params['output/kernel'] + params['output/bias']


def random_case(B, F, d_in, H, ds, seed, dtype=torch.float64, device='cpu'):
  """Inputs and glorot-uniform kernels [d_in, H * ds] of one layer (the packed order)."""
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(B, F, d_in, generator=g, dtype=torch.float64)
  d = H * ds
  lim = math.sqrt(6.0 / (d_in + d))
  ws = [(torch.rand(d_in, d, generator=g, dtype=torch.float64) * 2 - 1) * lim for _ in range(4)]
  return x.to(device=device, dtype=dtype), [w.to(device=device, dtype=dtype) for w in ws]

