#!/usr/bin/env python
"""One AutoInt interacting layer (forward + backward) at the flagship shape, timed two ways in one process on the same
inputs: the product's HIP path (kernels.AutoIntProjFn + AutoIntAttnFn: pack, one contraction, the attention launch;
backward: the attention launch, the input-gradient contraction, four weight-gradient contractions) and the same block
composed of torch-ROCm ops (matmul, reshape / permute, softmax, relu; autograd backward).  Also the attention launches
alone against the torch ops between the projections.  Prints one JSON line (and writes it to --out when given).

usage: python tools/autoint_attn_bench.py [--B 4096] [--F 18] [--d_in 16] [--iters 50] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from easyrec_amd import kernels  # noqa: E402


def torch_core(g, F, H, ds):
  B = g.shape[0] // F
  d = H * ds
  gv = g.view(B, F, 4 * d)

  def split(t):
    return t.reshape(B, F, H, ds).permute(0, 2, 1, 3)

  q, k, v = split(gv[..., :d]), split(gv[..., d:2 * d]), split(gv[..., 2 * d:3 * d])
  o = torch.softmax((q @ k.transpose(-1, -2)) * (ds ** 0.5), dim=-1) @ v
  return torch.relu(o.permute(0, 2, 1, 3).reshape(B * F, d) + gv[..., 3 * d:].reshape(B * F, d))


def timed(fn, iters, warmup=5):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(iters):
    fn()
  end.record()
  torch.cuda.synchronize()
  return start.elapsed_time(end) * 1000.0 / iters  # us


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--B', type=int, default=4096)
  ap.add_argument('--F', type=int, default=18)
  ap.add_argument('--d_in', type=int, default=16)
  ap.add_argument('--H', type=int, default=2)
  ap.add_argument('--ds', type=int, default=32)
  ap.add_argument('--iters', type=int, default=50)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('autoint_attn_bench: needs a GPU')
  dev = 'cuda:0'
  B, F, H, ds, d_in = a.B, a.F, a.H, a.ds, a.d_in
  d = H * ds
  g = torch.Generator(device=dev).manual_seed(1)
  x = torch.randn(B * F, d_in, device=dev, generator=g)
  ws = [torch.randn(d_in, d, device=dev, generator=g) * (6.0 / (d_in + d)) ** 0.5 for _ in range(4)]
  grads = [torch.zeros_like(w) for w in ws]
  dy = torch.randn(B * F, d, device=dev, generator=g)
  be = kernels.hip()

  def hip_layer():
    xi = x.detach().requires_grad_(True)
    y = kernels.AutoIntAttnFn.apply(kernels.AutoIntProjFn.apply(xi, grads, *ws), F, H, ds)
    y.backward(dy)

  wt = [w.detach().clone().requires_grad_(True) for w in ws]

  def torch_layer():
    xi = x.detach().requires_grad_(True)
    qkvr = xi @ torch.cat(wt, dim=1)
    y = torch_core(qkvr, F, H, ds)
    y.backward(dy)

  qkvr = (x @ torch.cat(ws, dim=1)).contiguous()
  y_hip = be.autoint_attn_fwd(qkvr, F, H, ds)
  gt = qkvr.detach().clone().requires_grad_(True)

  def hip_core():
    yy = be.autoint_attn_fwd(qkvr, F, H, ds)
    be.autoint_attn_bwd(qkvr, yy, dy, F, H, ds)

  def torch_core_fb():
    gt.grad = None
    torch_core(gt, F, H, ds).backward(dy)

  err = float((y_hip - torch_core(qkvr, F, H, ds)).abs().max())
  res = {
      'shape': {'B': B, 'F': F, 'd_in': d_in, 'H': H, 'ds': ds},
      'layer_fwd_bwd_us': {'hip': timed(hip_layer, a.iters), 'torch_ops': timed(torch_layer, a.iters)},
      'attention_fwd_bwd_us': {'hip': timed(hip_core, a.iters), 'torch_ops': timed(torch_core_fb, a.iters)},
      'attention_fwd_us': {'hip': timed(lambda: be.autoint_attn_fwd(qkvr, F, H, ds), a.iters),
                           'torch_ops': timed(lambda: torch_core(qkvr, F, H, ds), a.iters)},
      'max_abs_diff_y': err,
      # the attention launches' compulsory HBM bytes: forward reads [B F, 4d] and writes [B F, d]; backward reads
      # [B F, 4d] + 2 [B F, d] and writes [B F, 4d]
      'attention_bytes': {'fwd': 4 * B * F * 5 * d, 'bwd': 4 * B * F * 10 * d},
  }
  line = json.dumps(res)
  print(line)
  if a.out:
    with open(a.out, 'a') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
