"""Times forward + backward of the fused two-tower head (csrc/er_match.hip) against the same head composed of torch
ops (layers/match_head.match_head_compose) on one GPU: the two sides alternate in one process, ROUNDS rounds of ITERS
calls each, min / mean / max of the rounds' per-call times per side.  One JSON line per shape.
usage: python tools/match_bench.py [--batch 4096] [--dim 32] [--extra 0 1024] [--rounds 7] [--iters 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=4096)
  ap.add_argument('--dim', type=int, default=32)
  ap.add_argument('--extra', type=int, nargs='+', default=[0, 1024])
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--iters', type=int, default=50)
  args = ap.parse_args()
  from easyrec_amd import kernels
  from easyrec_amd.layers import match_head
  dev = 'cuda:0'
  info = kernels.hip().device_info()
  for extra in args.extra:
    B, M, D = args.batch, args.batch + extra, args.dim
    g = torch.Generator().manual_seed(1)
    U = (torch.randn(B, D, generator=g) * 0.5).to(dev).requires_grad_(True)
    I = (torch.randn(M, D, generator=g) * 0.5).to(dev).requires_grad_(True)
    sw = torch.ones(1, device=dev, requires_grad=True)
    sb = torch.zeros(1, device=dev, requires_grad=True)
    ids = torch.randint(0, 10000000, (M,), generator=g).to(dev)

    def call(head):
      for t in (U, I, sw, sb):
        t.grad = None
      ce, reg = head(U, I, 1.0, sw, sb, ids, False, None)
      (ce + reg).backward()

    sides = {'fused': match_head.match_head, 'composed': match_head.match_head_compose}
    times = {k: [] for k in sides}
    for head in sides.values():
      for _ in range(5):
        call(head)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
      for name, head in sides.items():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
          call(head)
        stop.record()
        torch.cuda.synchronize()
        times[name].append(start.elapsed_time(stop) * 1e3 / args.iters)
    line = {'bench': 'match_head_fwd_bwd', 'B': B, 'M': M, 'D': D, 'rounds': args.rounds, 'iters': args.iters,
            'device': info}
    for name, ts in times.items():
      line[name + '_us'] = {'min': round(min(ts), 1), 'mean': round(sum(ts) / len(ts), 1), 'max': round(max(ts), 1)}
    line['fused_wins'] = line['fused_us']['max'] < line['composed_us']['min']
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
  main()
