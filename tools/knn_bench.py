"""Times the exact top-K item search (csrc/er_knn.hip through core/knn.py ItemIndex) against the same search composed of
torch ops (core/knn.py search_composed: chunked matmul + topk + merge) on one GPU: the two sides alternate in one
process, ROUNDS rounds of ITERS calls each, min / mean / max of the rounds' per-call times per side.  One JSON line per
shape, with the kernel's share of the 155 TF fp32-matrix peak (2 nq n D flop per call).
usage: python tools/knn_bench.py [--items 10000000] [--dim 32] [--queries 4096 20480] [--topk 5 100] [--metric 1 0]
                                 [--rounds 3] [--iters 2] [--slices 0]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 155.0  # fp32-input MFMA, measured (MI355X)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--items', type=int, default=10000000)
  ap.add_argument('--dim', type=int, default=32)
  ap.add_argument('--queries', type=int, nargs='+', default=[4096, 20480])
  ap.add_argument('--topk', type=int, nargs='+', default=[5, 100])
  ap.add_argument('--metric', type=int, nargs='+', default=[1, 0])
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--iters', type=int, default=2)
  ap.add_argument('--slices', type=int, default=0)
  args = ap.parse_args()
  from easyrec_amd import kernels
  from easyrec_amd.core import knn
  dev = 'cuda:0'
  info = kernels.hip().device_info()
  props = torch.cuda.get_device_properties(0)
  info.update(name=props.name)
  from bench import gpu_clocks  # (what rocm-smi --showclocks says right after the timed region)
  n, D = args.items, args.dim
  g = torch.Generator(device=dev).manual_seed(1)
  items = torch.randn(n, D, generator=g, device=dev) * 0.5
  ids = torch.randperm(n, generator=g, device=dev)
  for metric in args.metric:
    index = knn.ItemIndex(ids, items, metric, dev)
    for nq in args.queries:
      queries = torch.randn(nq, D, generator=g, device=dev) * 0.5
      for K in args.topk:
        assert index.uses_kernel(K, args.slices)
        sides = {
            'kernel': lambda: kernels.hip().knn_search(queries, index.item_emb, index.xx, index.item_ids, K, metric,
                                                       args.slices),
            'composed': lambda: knn.search_composed(queries, index.item_emb, index.xx, index.item_ids, K, metric),
        }
        times = {k: [] for k in sides}
        outs = {name: call() for name, call in sides.items()}  # (the warm-up call of either side)
        torch.cuda.synchronize()
        same_rows = float((outs['kernel'][1] == outs['composed'][1]).float().mean())
        del outs
        for _ in range(args.rounds):
          for name, call in sides.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
              call()
            stop.record()
            torch.cuda.synchronize()
            times[name].append(start.elapsed_time(stop) / args.iters)
        line = {'bench': 'knn_search', 'n': n, 'D': D, 'nq': nq, 'K': K, 'metric': metric,
                'slices': args.slices or knn.auto_slices(nq, n), 'rounds': args.rounds, 'iters': args.iters,
                'device': info}
        for name, ts in times.items():
          line[name + '_ms'] = {'min': round(min(ts), 2), 'mean': round(sum(ts) / len(ts), 2), 'max': round(max(ts), 2)}
        tf = 2.0 * nq * n * D / (line['kernel_ms']['mean'] * 1e-3) / 1e12
        line['kernel_tflops'] = round(tf, 1)
        line['kernel_share_of_fp32_matrix_peak'] = round(tf / PEAK_TF, 3)
        # (random fp32 scores: the composition's matmul need not round as the fmaf chain does, so a near-tie may swap)
        line['rows_equal_fraction'] = round(same_rows, 6)
        line['clocks'] = gpu_clocks()
        line['kernel_wins'] = line['kernel_ms']['max'] < line['composed_ms']['min']
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
  main()
