#!/usr/bin/env python
"""The variational dropout kernel (er_vdrop_*; kernels.VDropFn) against the torch composition
(layers/variational_dropout_layer.vdrop_compose), forward + backward through autograd with the penalty and its gradient,
replayed from captured hipGraphs, each pair timed on the same inputs and the same noise in one process in ALTERNATING
windows (tools/cmbf_bench.py windows / verdict).  The noise draw itself (one torch.rand either way) is left out.

Shapes: B = 1024 and 4096; W = 624 (39 features of 16: the deep group of configs/deepfm_vdrop_criteo.config) and W = 39
(39 features of 1: its wide group); embedding-wise and feature-wise.  logit_p's gradient is added into a given buffer
on the kernel's side and accumulated by autograd on the other.

Every window is kept: a line holds the windows of each side (microseconds per call), their medians, and
`kernel_faster`: the medians differ in that direction by MORE than the larger spread (max - min) of the two sides'
windows - the spread of repeating the same variant in the same call.  Each line carries the rocm-smi clocks read when
it was written.  Prints one JSON line per measurement and appends them to --out.

usage: python tools/vdrop_bench.py [--iters 200] [--rounds 3] [--out FILE]
"""
import argparse
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cmbf_bench import clocks, verdict, windows  # noqa: E402
from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.layers import variational_dropout_layer as vdl  # noqa: E402

SHAPES = [(16,) * 39, (1,) * 39]
LAMBDA = 0.01


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('vdrop_bench: needs a GPU')
  dev = 'cuda:0'
  be = kernels.hip()
  g = torch.Generator(device=dev).manual_seed(1)
  lines = []

  def emit(line):
    line = dict(line, clocks=clocks())
    print(json.dumps(line), flush=True)
    lines.append(line)

  for B in (1024, 4096):
    for dims in SHAPES:
      for embedding_wise in (True, False):
        W = sum(dims)
        P = W if embedding_wise else len(dims)
        x, dout = (torch.randn(B, W, device=dev, generator=g) for _ in range(2))
        u = torch.rand(B, P, device=dev, generator=g)
        logit_p = torch.rand(P, device=dev, generator=g) * 2 - 1
        one = torch.ones(1, device=dev)
        lam = LAMBDA / B
        seg = None if embedding_wise else kernels.VDropSeg(dims, dev)
        index = None if embedding_wise else torch.repeat_interleave(torch.arange(len(dims)), torch.tensor(dims)).to(dev)
        grads = [torch.zeros_like(logit_p)]
        tlogit = logit_p.clone().requires_grad_(True)
        leaves = {side: x.clone().requires_grad_(True) for side in ('hip', 'torch')}

        def run_hip():
          # (collected before each capture, as tools/ppnet_bench.py does: an autograd node left to the collector's own
          # schedule could be met again inside a capture on another stream.  Host time only: a replay does not run it.)
          gc.collect()
          xi = leaves['hip']
          xi.grad = None
          out, pen = kernels.VDropFn.apply(grads, xi, logit_p, u, seg, lam)
          torch.autograd.backward([out, pen], [dout, one])

        def run_torch():
          gc.collect()
          xi = leaves['torch']
          xi.grad = tlogit.grad = None
          out, pen = vdl.vdrop_compose(xi, tlogit, u, index, lam)
          torch.autograd.backward([out, pen], [dout, one])

        grads[0].zero_()
        run_hip()
        run_torch()
        diff = max(float((leaves['hip'].grad - leaves['torch'].grad).abs().max() / leaves['torch'].grad.abs().max()),
                   float((grads[0] - tlogit.grad).abs().max() / tlogit.grad.abs().max()))
        wk, wt = windows(run_hip, run_torch, a.iters, a.rounds, graph=True)
        mk, mt, faster = verdict(wk, wt)
        emit({'B': B, 'W': W, 'P': P, 'mode': 'embedding_wise' if embedding_wise else 'feature_wise',
              'measure': 'vdrop_fwd_bwd', 'grid': be.vdrop_grid(B, W), 'timing': 'graph replay', 'kernel_us': wk,
              'torch_ops_us': wt, 'kernel_median_us': mk, 'torch_ops_median_us': mt, 'kernel_faster': bool(faster),
              'max_rel_diff': diff})

  summary = {'measure': 'summary',
             'kernel_faster_at_every_shape': all(ln['kernel_faster'] for ln in lines),
             'kernel_not_faster_at': [[ln['B'], ln['W'], ln['mode']] for ln in lines if not ln['kernel_faster']],
             # the switch's default: 1 only if the kernel path is faster at every listed shape
             'switch_default_supported': '1' if lines and all(ln['kernel_faster'] for ln in lines) else '0',
             'iters': a.iters, 'rounds': a.rounds, 'device': be.device_info(), 'clocks': clocks()}
  print(json.dumps(summary), flush=True)
  lines.append(summary)
  if a.out:
    with open(a.out, 'a') as f:
      for ln in lines:
        f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
  main()
