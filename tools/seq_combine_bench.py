#!/usr/bin/env python
"""The sequence-combiner kernels (er_text_cnn_*, er_seq_attn_pool_*) against their torch compositions
(layers/keras/text_cnn.py text_cnn_compose / seq_attn_pool_compose), forward + backward through autograd, each pair
timed on the same inputs in one process in ALTERNATING windows.

TextCNN: x [B, 14, 16] with filters [2, 3, 4] x [8, 4, 4] (examples/configs/deepfm_on_movielens.config) and x [16, 8, 8]
(samples/model_config/text_cnn_on_movielens.config), pad length 14, relu.  Attention pooling: x [B, 50, 16] with random
lengths.  B = 1024 and 4096.  x is a column of a wider [B * L, 48] buffer, as the embedding engine leaves it.

Each pair is measured twice: issued call by call from the host (`host-issued`: what a step outside a captured graph
pays, the host's share of every launch included) and, the parameter gradients going into given buffers, replayed from
captured hipGraphs of 20 forward + backward calls (`graph replay`: the device's share, what a captured step pays).

Every window is kept: a line holds the three windows of each side (microseconds per call), their medians, and
`kernel_faster`: the medians differ in that direction by MORE than the larger spread (max - min) of the two sides'
windows.  Prints one JSON line per measurement and appends them to --out.

usage: python tools/seq_combine_bench.py [--iters 200] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cmbf_bench import clocks, verdict, windows  # noqa: E402
from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.layers.keras import text_cnn as tc  # noqa: E402

TEXT_CNN = [(14, 14, 16, [2, 3, 4], [8, 4, 4]), (14, 14, 16, [2, 3, 4], [16, 8, 8])]  # (L_buf, P, D, sizes, filters)
POOL = [(50, 16)]
WIDTH = 48


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('seq_combine_bench: needs a GPU')
  dev = 'cuda:0'
  be = kernels.hip()
  g = torch.Generator(device=dev).manual_seed(1)
  lines = []

  def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)

  def measure(line, hip_fn, torch_fn, diff):
    for timing, graph in (('host-issued', False), ('graph replay', True)):
      wk, wt = windows(hip_fn, torch_fn, a.iters, a.rounds, graph=graph)
      mk, mt, faster = verdict(wk, wt)
      emit(dict(line, timing=timing, kernel_us=wk, torch_ops_us=wt, kernel_median_us=mk, torch_ops_median_us=mt,
                kernel_faster=bool(faster), max_abs_diff_dx=diff))

  for B in (1024, 4096):
    for L, P, D, sizes, filters in TEXT_CNN:
      buf = torch.randn(B, L, WIDTH, device=dev, generator=g)
      x_h = buf[:, :, 16:16 + D].detach().requires_grad_(True)
      x_t = buf[:, :, 16:16 + D].detach().requires_grad_(True)
      ks = [torch.randn(k, D, f, device=dev, generator=g) * (k * D) ** -0.5 for k, f in zip(sizes, filters)]
      bs = [torch.randn(f, device=dev, generator=g) * 0.1 for f in filters]
      params = [t for pair in zip(ks, bs) for t in pair]
      grads = [torch.zeros_like(p) for p in params]
      tparams = [p.clone().requires_grad_(True) for p in params]
      dy = torch.randn(B, sum(filters), device=dev, generator=g)

      def cnn_hip():
        x_h.grad = None
        kernels.TextCnnFn.apply(x_h, P, sizes, filters, True, grads, *params).backward(dy)

      def cnn_torch():
        x_t.grad = None
        for p in tparams:
          p.grad = None
        tc.text_cnn_compose(x_t, P, tparams[0::2], tparams[1::2], 'relu').backward(dy)

      cnn_hip()
      cnn_torch()
      diff = float((x_h.grad - x_t.grad).abs().max())
      measure({'measure': 'text_cnn_fwd_bwd', 'B': B, 'L_buf': L, 'P': P, 'D': D, 'sizes': sizes, 'filters': filters,
               'epb': be.text_cnn_epb(P, D, sizes, filters), 'lds_bytes': be.text_cnn_lds_bytes(P, D, sizes, filters)},
              cnn_hip, cnn_torch, diff)
    for L, D in POOL:
      buf = torch.randn(B, L, WIDTH, device=dev, generator=g)
      lens = torch.randint(0, L + 1, (B,), device=dev, generator=g).to(torch.int32)
      buf = buf * (torch.arange(L, device=dev)[None, :] < lens[:, None]).float()[:, :, None]
      x_h = buf[:, :, 16:16 + D].detach().requires_grad_(True)
      x_t = buf[:, :, 16:16 + D].detach().requires_grad_(True)
      w = torch.randn(D, 1, device=dev, generator=g) * 0.5
      gw = [torch.zeros_like(w)]
      tw = w.clone().requires_grad_(True)
      dy = torch.randn(B, D, device=dev, generator=g)

      def pool_hip():
        x_h.grad = None
        kernels.SeqAttnPoolFn.apply(x_h, lens, gw, w).backward(dy)

      def pool_torch():
        x_t.grad = None
        tw.grad = None
        tc.seq_attn_pool_compose(x_t, lens, tw).backward(dy)

      pool_hip()
      pool_torch()
      diff = float((x_h.grad - x_t.grad).abs().max())
      measure({'measure': 'seq_attn_pool_fwd_bwd', 'B': B, 'L_buf': L, 'D': D,
               'lds_bytes_bwd': be.seq_attn_pool_lds_bytes(L, D, True)}, pool_hip, pool_torch, diff)

  summary = {'measure': 'summary',
             'kernel_faster_at_every_shape': all(ln['kernel_faster'] for ln in lines),
             'kernel_not_faster_at': [[ln['measure'], ln['B'], ln.get('filters'), ln['timing']] for ln in lines
                                      if not ln['kernel_faster']],
             'iters': a.iters, 'rounds': a.rounds, 'device': be.device_info(), 'clocks': clocks()}
  print(json.dumps(summary), flush=True)
  lines.append(summary)
  if a.out:
    with open(a.out, 'a') as f:
      for ln in lines:
        f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
  main()
