#!/usr/bin/env python
"""The pair kernel (er_pairwise; builders/pairwise_loss.py) against the torch compositions of the four pairwise ranking
losses differentiated by autograd, forward plus gradient, each pair timed on the same inputs in one process in
ALTERNATING windows (tools/cmbf_bench.py windows / verdict).  Both sides yield the loss value and d loss / d logits; the
kernel's side includes the sum of its loss partials as a launch of its own, which inside a training step rides in the
loss tail's launch.

The compositions gather the pairs with a boolean mask, whose size the host reads back: they cannot be captured in a
hipGraph, so both sides are issued call by call from the host, as a training step issues them (`timing: eager`).  The
kernel's device time alone, replayed from a captured graph, is recorded beside it (`kernel_graph_us`).

Shapes: B = 1024 and 4096, each of the four kinds with per-example weights, without session keys and on the `user_id`
sessions that input/synthetic.py draws for configs/dbmtl_jrc_small_taobao.config.

Every window is kept: a line holds the windows of each side (microseconds per call), their medians, and
`kernel_faster`: the medians differ in that direction by MORE than the larger spread (max - min) of the two sides'
windows.  Each line carries the rocm-smi clocks read when it was written.  Prints one JSON line per measurement and
appends them to --out.

--sorted: the same two sides beyond er_pairwise's envelope, B = 16384 .. 131072, on er_pairwise_sorted (see
sorted_sweep(); its lines go to profiles/pairwise_sorted_bench_lines.jsonl).

usage: python tools/pairwise_bench.py [--iters 100] [--rounds 3] [--out FILE]
                                      [--sorted [--sorted-iters 10] [--torch-iters 1] [--batches B ...]]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cmbf_bench import GRAPH_CALLS, _graphed, clocks, verdict, windows  # noqa: E402
from multiclass_bench import session_keys  # noqa: E402
from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.builders import pairwise_loss as pwl  # noqa: E402
from easyrec_amd.protos import loss_pb2  # noqa: E402

LT = loss_pb2.LossType
KINDS = (('pair_wise', LT.PAIR_WISE_LOSS, None),
         ('logistic', LT.PAIRWISE_LOGISTIC_LOSS, None),
         ('hinge', LT.PAIRWISE_HINGE_LOSS, None),
         ('focal', LT.PAIRWISE_FOCAL_LOSS, loss_pb2.PairwiseFocalLoss(gamma=2.0, hinge_margin=1.0)))


def _window(fn, calls):
  """fn() `calls` times between two device events -> us per call"""
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(calls):
    fn()
  end.record()
  torch.cuda.synchronize()
  return start.elapsed_time(end) * 1000.0 / calls


def sorted_sweep(a):
  """--sorted: er_pairwise_sorted (K8p) against the composition at B = 16384 .. 131072, forward plus gradient, the four
  kinds with and without per-example weights, on `user_id` sessions of mean length 8 to 10 (folded to 1024 keys inside
  every block of 8192 examples, as tools/listwise_bench.py --tiled folds them), on one single session and without keys.
  Both sides are issued call by call in alternating windows, --sorted-iters calls of the kernel and --torch-iters of the
  composition a window; the kernel's launches replayed from a captured graph of GRAPH_CALLS calls are timed beside them
  (`kernel_graph_us`) where a call takes under 5 ms.  A composition that cannot allocate its [B, B] tensors is the
  cell's result (`torch_ops: 'out of memory'`), and the cell keeps the kernel's windows."""
  dev = 'cuda:0'
  be = kernels.hip()
  g = torch.Generator(device=dev).manual_seed(1)
  lines = []

  def emit(line):  # (written as it is measured: a sweep cut short keeps its lines)
    print(json.dumps(line), flush=True)
    lines.append(line)
    if a.out:
      with open(a.out, 'a') as f:
        f.write(json.dumps(line) + '\n')

  for B in a.batches:
    z = torch.randn(B, device=dev, generator=g)
    y = (torch.rand(B, device=dev, generator=g) < 0.25).to(torch.float32)
    w_all = torch.rand(B, device=dev, generator=g) + 0.5
    w_all[torch.rand(B, device=dev, generator=g) < 0.1] = 0.0
    block = torch.arange(B, device=dev) // 8192
    user = session_keys(B, dev) % 1024 + 1024 * block
    for sessions, keys in (('user_id', user), ('single', torch.zeros(B, dtype=torch.int64, device=dev)), ('none', None)):
      for name, loss_type, param in KINDS:
        for w in (w_all, None):
          p = pwl.params_of(loss_type, param)
          args = pwl.kernel_args(loss_type, p)
          got = {}

          def run_hip():
            o = be.pairwise_loss_sorted(z, y, keys, w, **args)
            loss = torch.empty(1, device=dev)
            be.reduce_sum(o['loss_partials'], 1.0, loss)  # (the loss tail's share of a step: the sum of the partial rows)
            got['hip'] = (loss, o['dlogits'], o['pair_count'])

          def run_torch():
            zr = z.detach().clone().requires_grad_(True)
            loss = pwl.compose(loss_type, y, zr, keys, w, p)
            dz, = torch.autograd.grad(loss, zr)
            got['torch'] = (loss.detach().reshape(1), dz)

          run_hip()
          torch.cuda.synchronize()
          line = dict(measure='pairwise_sorted_fwd_bwd', kind=name, B=B, sessions=sessions, weights=w is not None,
                      pairs=int(got['hip'][2]), grid=be.pairwise_sorted_grid(B), timing='eager')
          try:
            run_torch()
            torch.cuda.synchronize()
            composed = True
          except torch.cuda.OutOfMemoryError:
            composed = False
            torch.cuda.empty_cache()
          wk, wt = [], []
          for _ in range(a.rounds):  # alternating windows
            wk.append(_window(run_hip, a.sorted_iters))
            if composed:
              wt.append(_window(run_torch, a.torch_iters))
          med = lambda ws: sorted(ws)[len(ws) // 2]  # noqa: E731
          line.update(kernel_us=wk, kernel_median_us=med(wk))
          if composed:
            mk, mt, faster = verdict(wk, wt)
            diff = max(float((h - t).abs().max() / t.abs().max().clamp(min=1e-30)) for h, t in zip(got['hip'], got['torch']))
            line.update(torch_ops_us=wt, torch_ops_median_us=mt, kernel_faster=bool(faster), max_rel_diff=diff)
          else:
            line.update(torch_ops='out of memory', kernel_faster=None)
          if med(wk) < 5000.0:
            replay = _graphed(run_hip)
            line['kernel_graph_us'] = [_window(replay, 1) / GRAPH_CALLS for _ in range(a.rounds)]
          line['clocks'] = clocks()
          got.clear()
          torch.cuda.empty_cache()
          emit(line)
  measured = [ln for ln in lines if ln['kernel_faster'] is not None]
  summary = {'measure': 'summary',
             'kernel_faster_at_every_measured_shape': all(ln['kernel_faster'] for ln in measured),
             'kernel_not_faster_at': [[ln['kind'], ln['B'], ln['sessions'], ln['weights']] for ln in measured if not ln['kernel_faster']],
             'composition_out_of_memory_at': [[ln['kind'], ln['B'], ln['sessions'], ln['weights']] for ln in lines
                                              if ln['kernel_faster'] is None],
             # the switch's default: 1 only if the kernel path is faster at every shape the composition could run
             'switch_default_supported': '1' if measured and all(ln['kernel_faster'] for ln in measured) else '0',
             'sorted_iters': a.sorted_iters, 'torch_iters': a.torch_iters, 'rounds': a.rounds, 'device': be.device_info(),
             'clocks': clocks()}
  emit(summary)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=100)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  ap.add_argument('--sorted', action='store_true', help='the sweep of er_pairwise_sorted beyond B = 8192')
  ap.add_argument('--sorted-iters', type=int, default=10, help='--sorted: calls of the kernel a window')
  ap.add_argument('--torch-iters', type=int, default=1, help='--sorted: calls of the composition a window')
  ap.add_argument('--batches', type=int, nargs='+', default=[16384, 32768, 65536, 131072], help='--sorted: the sizes B')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('pairwise_bench: needs a GPU')
  if a.sorted:
    return sorted_sweep(a)
  dev = 'cuda:0'
  be = kernels.hip()
  g = torch.Generator(device=dev).manual_seed(1)
  lines = []
  for B in (1024, 4096):
    z = torch.randn(B, device=dev, generator=g)
    y = (torch.rand(B, device=dev, generator=g) < 0.25).to(torch.float32)
    w = torch.rand(B, device=dev, generator=g) + 0.5
    w[torch.rand(B, device=dev, generator=g) < 0.1] = 0.0
    for keyed in (False, True):
      keys = session_keys(B, dev) if keyed else None
      for name, loss_type, param in KINDS:
        p = pwl.params_of(loss_type, param)
        args = pwl.kernel_args(loss_type, p)
        got = {}

        def run_hip():
          o = be.pairwise_loss(z, y, keys, w, **args)
          got['hip'] = (o['loss_partials'].sum().reshape(1), o['dlogits'], o['pair_count'])

        def run_torch():
          zr = z.detach().clone().requires_grad_(True)
          loss = pwl.compose(loss_type, y, zr, keys, w, p)
          dz, = torch.autograd.grad(loss, zr)
          got['torch'] = (loss.detach().reshape(1), dz)

        run_hip()
        run_torch()
        torch.cuda.synchronize()
        diff = max(float((h - t).abs().max() / t.abs().max().clamp(min=1e-30)) for h, t in zip(got['hip'], got['torch']))
        wk, wt = windows(run_hip, run_torch, a.iters, a.rounds, graph=False)
        mk, mt, faster = verdict(wk, wt)
        wg, _ = windows(run_hip, run_hip, a.iters, a.rounds, graph=True)
        line = dict(measure='pairwise_fwd_bwd', kind=name, B=B, session_keys=keyed, pairs=int(got['hip'][2]),
                    grid=be.pairwise_grid(B), timing='eager', kernel_us=wk, torch_ops_us=wt, kernel_median_us=mk,
                    torch_ops_median_us=mt, kernel_faster=bool(faster), kernel_graph_us=wg, max_rel_diff=diff, clocks=clocks())
        print(json.dumps(line), flush=True)
        lines.append(line)
  summary = {'measure': 'summary',
             'kernel_faster_at_every_shape': all(ln['kernel_faster'] for ln in lines),
             'kernel_not_faster_at': [[ln['kind'], ln['B'], ln['session_keys']] for ln in lines if not ln['kernel_faster']],
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
