#!/usr/bin/env python
"""The weighted negative draw (er_neg_sample_weighted, easyrec_hip.h K1c) against the uniform in-memory kernel
(er_neg_sample, K1b) and against its own host composition (neg_sampler.draw_weighted plus the torch gathers), on one
table in one process in ALTERNATING windows.

Shape: the benchmark configs' - B 4096, N 1024, a 10 M-row table, 7 int64 columns, weights 1 / (1 + r % 1024), the batch
B distinct rows.  Each launch draws for the next step (a device counter is incremented between launches, as the step's
prologue does), so no two launches read the same rows.  The two kernels are replayed from captured hipGraphs of 20
(counter increment, launch) pairs; the composition reads the counter on the host and cannot be captured, so it is
issued call by call and timed by the host clock around a device synchronise - as is, for comparison on equal terms, the
weighted kernel once more (`weighted_eager`).

Every window is kept: microseconds per call, the medians, and `faster`: the medians differ by more than the larger
spread (max - min) of the two sides' windows.  Also one line that the kernel's draw equals the composition's on these
inputs.  Prints JSON lines and appends them to --out.

usage: python tools/neg_sampler_bench.py [--rows 10000000] [--iters 400] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.input import neg_sampler  # noqa: E402

GRAPH_CALLS = 20


def graphed(fn):
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    fn()
  torch.cuda.current_stream().wait_stream(s)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    for _ in range(GRAPH_CALLS):
      fn()
  return graph.replay


def event_window(fn, reps, per):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  end.record()
  torch.cuda.synchronize()
  return start.elapsed_time(end) * 1000.0 / (reps * per)


def wall_window(fn, reps):
  torch.cuda.synchronize()
  t = time.perf_counter()
  for _ in range(reps):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t) * 1e6 / reps


def verdict(a, b):
  med = lambda w: sorted(w)[len(w) // 2]  # noqa: E731
  spread = max(max(a) - min(a), max(b) - min(b))
  return med(a), med(b), abs(med(a) - med(b)) > spread


def clocks():
  try:
    from bench import gpu_clocks
    return gpu_clocks()
  except Exception as e:  # (the figures stand without them)
    return {'unavailable': str(e)[:80]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rows', type=int, default=10000000)
  ap.add_argument('--batch', type=int, default=4096)
  ap.add_argument('--num_sample', type=int, default=1024)
  ap.add_argument('--cols', type=int, default=7)
  ap.add_argument('--iters', type=int, default=400)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('neg_sampler_bench: needs a GPU')
  dev, be = 'cuda:0', kernels.hip()
  n, B, N = a.rows, a.batch, a.num_sample
  rng = np.random.default_rng(1)
  ids = np.arange(n, dtype=np.int64)
  t0 = time.perf_counter()
  host_alias = neg_sampler.alias_table(1.0 / (1.0 + (ids % 1024)))
  build_s = time.perf_counter() - t0
  batch = rng.choice(n, size=B, replace=False).astype(np.int64)
  d_alias, d_ids, d_batch = (torch.from_numpy(x).to(dev) for x in (host_alias.view(np.int64), ids, batch))
  cols = [(torch.from_numpy(rng.integers(0, 1 << 40, size=n)).to(dev), torch.from_numpy(rng.integers(0, 1 << 40, size=B)).to(dev),
           torch.zeros(B + N, dtype=torch.int64, device=dev)) for _ in range(a.cols)]
  sel = torch.zeros(N, dtype=torch.int32, device=dev)
  counter = torch.zeros(1, dtype=torch.int64, device=dev)
  seed = 7
  lines = []

  def emit(line):
    line.update(rows=n, batch=B, num_sample=N, cols=a.cols, clocks=clocks())
    print(json.dumps(line), flush=True)
    lines.append(line)

  def weighted():
    counter.add_(1)
    be.neg_sample_weighted(d_alias, d_ids, d_batch, N, counter, 0, seed, cols, sel)

  def in_memory():
    counter.add_(1)
    be.neg_sample(d_ids, d_batch, N, counter, 0, seed, cols, sel)

  def composed():
    counter.add_(1)
    step = int(counter.item())
    rows = torch.from_numpy(neg_sampler.draw_weighted(seed, step, host_alias, ids, d_batch.cpu().numpy(), N)).to(dev)
    sel.copy_(rows.to(torch.int32))
    for tab, bat, out in cols:
      out[:B].copy_(bat)
      out[B:].copy_(tab[rows])

  # the same draw on both paths
  counter.fill_(41)
  weighted()
  torch.cuda.synchronize()
  got = [sel.cpu().numpy().copy()] + [out.cpu().numpy().copy() for _, _, out in cols]
  counter.fill_(41)
  composed()
  torch.cuda.synchronize()
  want = [sel.cpu().numpy().copy()] + [out.cpu().numpy().copy() for _, _, out in cols]
  emit({'what': 'kernel_equals_composition', 'equal': all(np.array_equal(x, y) for x, y in zip(got, want)),
        'alias_table_build_s': round(build_s, 3)})

  gw, gm = graphed(weighted), graphed(in_memory)
  reps = max(1, a.iters // GRAPH_CALLS)
  for _ in range(5):
    gw()
    gm()
  torch.cuda.synchronize()
  w_win, m_win = [], []
  for _ in range(a.rounds):
    w_win.append(event_window(gw, reps, GRAPH_CALLS))
    m_win.append(event_window(gm, reps, GRAPH_CALLS))
  mw, mm, sig = verdict(w_win, m_win)
  emit({'what': 'weighted_vs_in_memory_graph_replay', 'unit': 'us per (counter increment + launch)', 'weighted': w_win,
        'in_memory': m_win, 'weighted_median': mw, 'in_memory_median': mm, 'differ_by_more_than_spread': sig})

  for _ in range(3):
    weighted()
    composed()
  e_win, c_win = [], []
  for _ in range(a.rounds):
    e_win.append(wall_window(weighted, a.iters))
    c_win.append(wall_window(composed, max(4, a.iters // 20)))
  me, mc, sig = verdict(e_win, c_win)
  emit({'what': 'weighted_eager_vs_composition', 'unit': 'us per call, host clock around a synchronise', 'weighted_eager': e_win,
        'composition': c_win, 'weighted_eager_median': me, 'composition_median': mc, 'differ_by_more_than_spread': sig})
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
      for line in lines:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
  main()
