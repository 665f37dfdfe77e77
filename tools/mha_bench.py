#!/usr/bin/env python
"""The K8f launches (csrc/er_mha.hip) at Uniter's sample shape, each timed forward + backward against the torch
composition of the same ops on the same inputs, in one process, alternating the two: the attention core
(kernels.MhaAttnFn vs layers.multihead_cross_attention.attention_compose), the residual add + LayerNorm
(kernels.AddLayerNormFn vs add_layer_norm_compose), and one whole encoder layer with EASYREC_AMD_FUSED_MHA=1 and =0.
Prints one JSON line (and appends it to --out when given): microseconds, and for the two launches the compulsory HBM
bytes and the achieved TB/s.

usage: python tools/mha_bench.py [--B 1024] [--S 33] [--hidden 512] [--H 4] [--intermediate 512] [--iters 30] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.core import context  # noqa: E402
from easyrec_amd.core.variables import VarStore  # noqa: E402
from easyrec_amd.layers import multihead_cross_attention as mca  # noqa: E402


def timed_pair(fa, fb, iters, warmup=3, rounds=3):
  """(us of fa, us of fb): `rounds` alternating windows of `iters` calls each, the best window of each."""
  for _ in range(warmup):
    fa()
    fb()
  torch.cuda.synchronize()
  best = [float('inf'), float('inf')]
  for _ in range(rounds):
    for i, fn in enumerate((fa, fb)):
      start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      for _ in range(iters):
        fn()
      end.record()
      torch.cuda.synchronize()
      best[i] = min(best[i], start.elapsed_time(end) * 1000.0 / iters)
  return best


def timed(fn, iters, warmup=3):
  return timed_pair(fn, lambda: None, iters, warmup)[0]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--B', type=int, default=1024)
  ap.add_argument('--S', type=int, default=33)
  ap.add_argument('--hidden', type=int, default=512)
  ap.add_argument('--H', type=int, default=4)
  ap.add_argument('--intermediate', type=int, default=512)
  ap.add_argument('--iters', type=int, default=30)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('mha_bench: needs a GPU')
  dev = 'cuda:0'
  B, S, W, H = a.B, a.S, a.hidden, a.H
  ds = W // H
  rows = B * S
  g = torch.Generator(device=dev).manual_seed(1)
  be = kernels.hip()
  mask = (torch.rand(B, S, device=dev, generator=g) < 0.8).to(torch.int32)
  mask[:, 0] = 1
  maskf = mask.to(torch.float32)

  # -- the attention core on a packed Q | K | V buffer
  qkv = torch.randn(rows, 3 * W, device=dev, generator=g)
  dctx = torch.randn(rows, W, device=dev, generator=g)
  qkv_h = qkv.clone().requires_grad_(True)
  qkv_t = qkv.clone().requires_grad_(True)

  def attn_hip():
    qkv_h.grad = None
    kernels.MhaAttnFn.apply(qkv_h, None, mask, B, S, S, H, ds).backward(dctx)

  def attn_torch():
    qkv_t.grad = None
    mca.attention_compose(qkv_t[:, :W], qkv_t[:, W:2 * W], qkv_t[:, 2 * W:], maskf, B, S, S, H, ds).backward(dctx)

  with context.use(context.ModelContext(None, None, is_training=True)):
    attn_hip()
    attn_torch()
    attn_diff = float((qkv_h.grad - qkv_t.grad).abs().max() / qkv_t.grad.abs().max())
    attn_us = timed_pair(attn_hip, attn_torch, a.iters)
    fwd_us = timed_pair(lambda: be.mha_fwd(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], mask, B, S, S, H, ds),
                        lambda: mca.attention_compose(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], maskf, B, S, S, H, ds),
                        a.iters)

  # -- add & LayerNorm
  x = torch.randn(rows, W, device=dev, generator=g)
  res = torch.randn(rows, W, device=dev, generator=g)
  dy = torch.randn(rows, W, device=dev, generator=g)
  gamma = (1.0 + 0.1 * torch.randn(W, device=dev, generator=g)).requires_grad_(True)
  beta = torch.randn(W, device=dev, generator=g).requires_grad_(True)
  ggrads = [torch.zeros(W, device=dev), torch.zeros(W, device=dev)]
  x_h, r_h = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
  x_t, r_t = x.clone().requires_grad_(True), res.clone().requires_grad_(True)

  def ln_hip():
    x_h.grad = r_h.grad = None
    kernels.AddLayerNormFn.apply(x_h, r_h, gamma, beta, mca.LN_EPSILON, ggrads).backward(dy)

  def ln_torch():
    x_t.grad = r_t.grad = gamma.grad = beta.grad = None
    mca.add_layer_norm_compose(x_t, r_t, gamma, beta).backward(dy)

  ln_hip()
  ln_torch()
  ln_diff = float((x_h.grad - x_t.grad).abs().max() / x_t.grad.abs().max())
  ln_us = timed_pair(ln_hip, ln_torch, a.iters)
  ln_fwd_us = timed_pair(lambda: be.add_ln_fwd(x, res, gamma.detach(), beta.detach(), mca.LN_EPSILON),
                         lambda: mca.add_layer_norm_compose(x, res, gamma.detach(), beta.detach()), a.iters)

  # -- one encoder layer, fused and composed (the same dense layers on the HIP contractions either way)
  xin = torch.randn(B, S, W, device=dev, generator=g)
  dout = torch.randn(B, S, W, device=dev, generator=g)
  vs = VarStore(dev, seed=3)
  ctx = context.ModelContext(vs, None, is_training=True)

  def encoder(inp):
    return mca.transformer_encoder(inp, mca.create_attention_mask_from_input_mask(inp, mask), hidden_size=W,
                                   num_hidden_layers=1, num_attention_heads=H, intermediate_size=a.intermediate)

  with context.use(ctx), torch.no_grad():
    encoder(xin)
  vs.pack()
  ctx.building = False

  def layer(flag):
    def run():
      os.environ['EASYREC_AMD_FUSED_MHA'] = flag
      vs.zero_grad()
      xi = xin.detach().requires_grad_(True)
      with context.use(ctx):
        encoder(xi).backward(dout)
    return run

  keep = os.environ.get('EASYREC_AMD_FUSED_MHA')
  try:
    layer_us = timed_pair(layer('1'), layer('0'), max(a.iters // 3, 5))
  finally:
    if keep is None:
      os.environ.pop('EASYREC_AMD_FUSED_MHA', None)
    else:
      os.environ['EASYREC_AMD_FUSED_MHA'] = keep

  # compulsory HBM bytes: attention forward reads Q | K | V and writes ctx; backward reads them and dctx and writes
  # dQ | dK | dV.  add & LayerNorm forward reads x, res and writes y; backward reads dy, x, res and writes dz
  attn_bytes = {'fwd': 4 * rows * 4 * W, 'bwd': 4 * rows * 7 * W}
  ln_bytes = {'fwd': 4 * rows * 3 * W, 'bwd': 4 * rows * 4 * W}
  res = {
      'shape': {'B': B, 'S': S, 'hidden': W, 'H': H, 'ds': ds, 'intermediate': a.intermediate},
      'attention_fwd_bwd_us': {'hip': attn_us[0], 'torch_ops': attn_us[1]},
      'attention_fwd_us': {'hip': fwd_us[0], 'torch_ops': fwd_us[1]},
      'attention_bytes': attn_bytes,
      'attention_hip_TBps': {'fwd': attn_bytes['fwd'] / fwd_us[0] * 1e-6,
                             'fwd_bwd': (attn_bytes['fwd'] + attn_bytes['bwd']) / attn_us[0] * 1e-6},
      'add_ln_fwd_bwd_us': {'hip': ln_us[0], 'torch_ops': ln_us[1]},
      'add_ln_fwd_us': {'hip': ln_fwd_us[0], 'torch_ops': ln_fwd_us[1]},
      'add_ln_bytes': ln_bytes,
      'add_ln_hip_TBps': {'fwd': ln_bytes['fwd'] / ln_fwd_us[0] * 1e-6,
                          'fwd_bwd': (ln_bytes['fwd'] + ln_bytes['bwd']) / ln_us[0] * 1e-6},
      'encoder_layer_fwd_bwd_us': {'fused': layer_us[0], 'composition': layer_us[1]},
      'max_rel_diff': {'attention_dqkv': attn_diff, 'add_ln_dx': ln_diff},
      'device': be.device_info(),
  }
  line = json.dumps(res)
  print(line)
  if a.out:
    with open(a.out, 'a') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
