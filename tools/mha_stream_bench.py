#!/usr/bin/env python
"""The streaming attention kernels (csrc/er_mha_stream.hip) against the torch composition of the same ops on the same
inputs: forward + backward of each captured as a hipGraph and replayed in alternating windows within one process.  Per
shape one JSON line (appended to --out when given): the spread of repeated identical windows of the kernel graph first,
then the median and the best window of each side, the algorithmic flops (4 B F T H ds forward, 10 backward: S is
recomputed once) over the kernels' median time as a share of the fp32-matrix peak, the largest relative difference of
the gradients, and the clocks read in the same call.

usage: python tools/mha_stream_bench.py [--B 1024] [--shapes F,T,ds,H ...] [--iters 20] [--rounds 5] [--out FILE]
A whole run is one step of a chain, under its own time limit:
  timeout -k 10 600 python tools/mha_stream_bench.py --out profiles/mha_stream_bench_lines.jsonl && <the next step>
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.core import context  # noqa: E402
from easyrec_amd.layers import multihead_cross_attention as mca  # noqa: E402

# (F, T, ds, H): the first square outside the LDS envelope, three encoder shapes, image -> text, the behaviour-sequence
# length, and uniter_long_movielens.config's own shape
SHAPES = [(35, 35, 128, 4), (64, 64, 64, 4), (129, 129, 128, 4), (1, 128, 16, 2), (200, 200, 32, 4), (81, 81, 128, 4)]
FP32_MATRIX_PEAK = 157.3e12


def captured(fn):
  """fn warmed up on a side stream, then captured: -> the graph."""
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    for _ in range(2):
      fn()
  torch.cuda.current_stream().wait_stream(s)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    fn()
  return graph


def window(graph, iters):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(iters):
    graph.replay()
  end.record()
  torch.cuda.synchronize()
  return start.elapsed_time(end) * 1000.0 / iters


def clocks():
  try:
    out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=30).stdout
    return [ln.strip() for ln in out.splitlines() if 'sclk' in ln or 'mclk' in ln][:4]
  except (OSError, subprocess.SubprocessError):
    return []


def bench(B, F, T, ds, H, iters, rounds, dev='cuda:0'):
  g = torch.Generator(device=dev).manual_seed(1)
  d = H * ds
  mask = (torch.rand(B, T, device=dev, generator=g) < 0.8).to(torch.int32)
  mask[:, 0] = 1
  packed = F == T
  q_src = torch.randn(B * F, 3 * d if packed else d, device=dev, generator=g)
  kv_src = None if packed else torch.randn(B * T, 2 * d, device=dev, generator=g)
  dctx = torch.randn(B * F, d, device=dev, generator=g)
  srcs = [t.clone().requires_grad_(True) for t in (q_src, kv_src) if t is not None]
  grads = {}

  def hip():
    grads['hip'] = torch.autograd.grad(kernels.MhaStreamAttnFn.apply(srcs[0], srcs[1] if not packed else None, mask, B, F,
                                                                     T, H, ds), srcs, dctx)

  def torch_ops():
    q, k, v = kernels.MhaAttnFn._split(srcs[0], None if packed else srcs[1], d)
    grads['torch'] = torch.autograd.grad(mca.attention_compose(q, k, v, mask, B, F, T, H, ds), srcs, dctx)

  with context.use(context.ModelContext(None, None, is_training=True)):
    graphs = [captured(hip), captured(torch_ops)]
  same = [window(graphs[0], iters) for _ in range(rounds)]
  us = [[], []]
  for _ in range(rounds):
    for i in (0, 1):
      us[i].append(window(graphs[i], iters))
  med = [statistics.median(x) for x in us]
  # (the graphs' outputs hold values only after a replay)
  diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads['hip'], grads['torch']))
  flops = 14.0 * B * F * T * d
  return {
      'shape': {'B': B, 'F': F, 'T': T, 'ds': ds, 'H': H}, 'iters': iters, 'rounds': rounds,
      'spread_identical_windows': (max(same) - min(same)) / min(same),
      'fwd_bwd_us': {'stream_median': med[0], 'stream_best': min(us[0]), 'torch_ops_median': med[1],
                     'torch_ops_best': min(us[1])},
      'speedup_median': med[1] / med[0],
      'algorithmic_flops': flops, 'stream_share_of_fp32_matrix_peak': flops / (med[0] * 1e-6) / FP32_MATRIX_PEAK,
      'max_rel_diff_gradients': diff, 'clocks': clocks(), 'device': kernels.hip().device_info(),
  }


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--B', type=int, default=1024)
  ap.add_argument('--shapes', nargs='*', default=[], help='F,T,ds,H (default: the recorded list)')
  ap.add_argument('--iters', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('mha_stream_bench: needs a GPU')
  shapes = [tuple(int(n) for n in s.split(',')) for s in a.shapes] or SHAPES
  for F, T, ds, H in shapes:
    line = json.dumps(bench(a.B, F, T, ds, H, a.iters, a.rounds))
    print(line, flush=True)
    if a.out:
      with open(a.out, 'a') as f:
        f.write(line + '\n')


if __name__ == '__main__':
  main()
