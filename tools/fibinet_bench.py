#!/usr/bin/env python
"""FiBiNet's two field blocks (forward + backward) at the sample's geometry, each timed two ways in one process on the
same inputs, the two versions ALTERNATING round by round: the product's HIP path (kernels.BiLinearFn / SENetFn: one
packing launch, one launch each way, the fixed-order reduce of the parameter gradients) and the same block composed of
torch-ROCm ops with autograd (layers/keras/fibinet.py bilinear_compose / senet_compose, the path the blocks take on
another backend or outside the kernels' envelope).  Every round is warmed up and device-synchronised; the mean, the
minimum, the maximum and the standard deviation over the rounds are printed for each.  Prints one JSON line (and
appends it to --out when given).

usage: python tools/fibinet_bench.py [--B 4096] [--F 17] [--D 16] [--iters 50] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.layers.keras import fibinet as fb  # noqa: E402


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


def alternate(fns, iters, rounds):
  """{name: stats of `rounds` timings}, the versions taking turns inside every round."""
  runs = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      runs[k].append(timed(fn, iters))
  return {k: {'mean_us': statistics.mean(v), 'min_us': min(v), 'max_us': max(v), 'stdev_us': statistics.pstdev(v)}
          for k, v in runs.items()}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--B', type=int, default=4096)
  ap.add_argument('--F', type=int, default=17)
  ap.add_argument('--D', type=int, default=16)
  ap.add_argument('--groups', type=int, default=2)
  ap.add_argument('--ratio', type=int, default=4)
  ap.add_argument('--iters', type=int, default=50)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('fibinet_bench: needs a GPU')
  dev = 'cuda:0'
  B, F, D, G = a.B, a.F, a.D, a.groups
  R = fb.senet_reduction(F, G, a.ratio)
  assert fb.bilinear_fits(F, D) and fb.senet_fits(F, D, G, R), 'geometry outside the kernels\' envelope'
  g = torch.Generator(device=dev).manual_seed(1)
  rn = lambda *s: torch.randn(*s, device=dev, generator=g)
  x = rn(B, F * D)
  pairs = F * (F - 1) // 2
  res = {'shape': {'B': B, 'F': F, 'D': D, 'groups': G, 'reduction': R}, 'iters': a.iters, 'rounds': a.rounds}

  # bilinear, `each` with use_plus (the sample's)
  bp = []
  for _ in range(F - 1):
    bp += [rn(D, D) * (1.0 / D) ** 0.5, rn(D) * 0.1]
  bg = [torch.zeros_like(p) for p in bp]
  bt = [p.detach().clone().requires_grad_(True) for p in bp]
  dp = rn(B, pairs)

  def bilinear_hip():
    xi = x.detach().requires_grad_(True)
    kernels.BiLinearFn.apply(xi, F, D, True, True, bg, *bp).backward(dp)

  def bilinear_torch():
    xi = x.detach().requires_grad_(True)
    fb.bilinear_compose(xi, F, D, bt[0::2], bt[1::2], True).backward(dp)

  res['bilinear_max_abs_diff'] = float((kernels.BiLinearFn.apply(x, F, D, True, True, bg, *bp) -
                                        fb.bilinear_compose(x, F, D, bp[0::2], bp[1::2], True)).abs().max())
  res['bilinear_fwd_bwd'] = alternate({'hip': bilinear_hip, 'torch_ops': bilinear_torch}, a.iters, a.rounds)

  # SENet with the skip connection and the layer norm (the sample's)
  Z, FD = 2 * F * G, F * D
  sp = [rn(Z, R) * (2.0 / Z) ** 0.5, rn(R) * 0.1, rn(R, FD) * (2.0 / (R + FD)) ** 0.5, rn(FD) * 0.1,
        1.0 + 0.2 * rn(FD), 0.1 * rn(FD)]
  sg = [torch.zeros_like(p) for p in sp]
  stt = [p.detach().clone().requires_grad_(True) for p in sp]
  dy = rn(B, FD)

  def senet_hip():
    xi = x.detach().requires_grad_(True)
    kernels.SENetFn.apply(xi, F, D, G, R, True, True, sg, *sp).backward(dy)

  def senet_torch():
    xi = x.detach().requires_grad_(True)
    fields = [xi[:, i * D:(i + 1) * D] for i in range(F)]
    fb.senet_compose(fields, G, stt[0], stt[1], stt[2], stt[3], True, stt[4], stt[5]).backward(dy)

  fields = [x[:, i * D:(i + 1) * D] for i in range(F)]
  res['senet_max_abs_diff'] = float((kernels.SENetFn.apply(x, F, D, G, R, True, True, sg, *sp) -
                                     fb.senet_compose(fields, G, *sp[:4], True, sp[4], sp[5])).abs().max())
  res['senet_fwd_bwd'] = alternate({'hip': senet_hip, 'torch_ops': senet_torch}, a.iters, a.rounds)
  for blk in ('bilinear', 'senet'):
    t = res[blk + '_fwd_bwd']
    # faster by more than the spread: the slowest fused round against the fastest composed one
    res[blk + '_hip_faster_beyond_spread'] = t['hip']['max_us'] < t['torch_ops']['min_us']
  line = json.dumps(res)
  print(line)
  if a.out:
    with open(a.out, 'a') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
