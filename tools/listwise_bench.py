#!/usr/bin/env python
"""The sorted-segment kernel (er_listwise; builders/listwise_loss.py) against the torch compositions of the two listwise
ranking losses differentiated by autograd, forward plus gradient, each pair timed on the same inputs in one process in
ALTERNATING windows (tools/cmbf_bench.py windows / verdict).  Both sides yield the loss value and d loss / d logits.

The compositions run torch.unique over the keys and one boolean-mask gather per session, whose sizes the host reads
back: they cannot be captured in a hipGraph (the summary's `composition_captures` records the attempt), so both sides are
issued call by call from the host, as a training step issues them (`timing: eager`).  The kernel's device time alone, replayed from
a captured graph, is recorded beside it (`kernel_graph_us`).

Shapes: B = 1024, 4096 and 8192, each kind on the `user_id` sessions that input/synthetic.py draws for
configs/dbmtl_jrc_small_taobao.config folded to a mean session length of about 8, and on one single session.

Every window is kept: a line holds the windows of each side (microseconds per call), their medians, and
`kernel_faster`: the medians differ in that direction by MORE than the larger spread (max - min) of the two sides'
windows.  Each line carries the rocm-smi clocks read when it was written.  Prints one JSON line per measurement and
appends them to --out.

--tiled: the same two sides beyond one workgroup's LDS, B = 16384 .. 131072, er_listwise_tiled at each of its tiles
(see tiled(); its lines go to profiles/listwise_tiled_bench_lines.jsonl).

usage: python tools/listwise_bench.py [--iters 20] [--rounds 3] [--out FILE] [--tiled [--torch-iters 1]]
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
from easyrec_amd.builders import listwise_loss as lwl  # noqa: E402
from easyrec_amd.protos import loss_pb2  # noqa: E402

LT = loss_pb2.LossType
KINDS = (('rank_logits', LT.LISTWISE_RANK_LOSS, loss_pb2.ListwiseRankLoss(session_name='u', label_is_logits=True, temperature=2.0)),
         ('distill', LT.LISTWISE_DISTILL_LOSS, loss_pb2.ListwiseDistillLoss(session_name='u')))


def _captures(fn):
  """whether fn() can be captured into a hipGraph"""
  torch.cuda.synchronize()
  try:
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
      fn()
    return True
  except Exception:  # (a device-to-host read inside the capture)
    torch.cuda.synchronize()
    return False


def _alternating(sides, rounds):
  """sides: [(fn, calls per window)] -> one list of windows (us per call) per side; every round times each side once, in
  turn, after one warm-up call of each."""
  for fn, _ in sides:
    fn()
  torch.cuda.synchronize()
  out = [[] for _ in sides]
  for _ in range(rounds):
    for i, (fn, calls) in enumerate(sides):
      start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      for _ in range(calls):
        fn()
      end.record()
      torch.cuda.synchronize()
      out[i].append(start.elapsed_time(end) * 1000.0 / calls)
  return out


def tiled(a):
  """--tiled: er_listwise_tiled (K8o) at every tile against the composition at B = 16384 .. 131072, forward plus
  gradient.  Two measurements a line: the kernel's launches at each tile replayed from captured graphs of GRAPH_CALLS
  calls, the tiles taking turns (`graph_us`: what the default tile is chosen by), and the default tile issued call by
  call against the composition in alternating windows (`kernel_us`, `torch_ops_us`).  The composition takes a large
  fraction of a second a call at these sizes and gets --torch-iters calls a window."""
  dev = 'cuda:0'
  be = kernels.hip()
  g = torch.Generator(device=dev).manual_seed(1)
  med = lambda w: sorted(w)[len(w) // 2]  # noqa: E731
  lines = []
  for B in (16384, 32768, 65536, 131072):
    z = torch.randn(B, device=dev, generator=g)
    # (user_id has about a thousand distinct ids: folded to 1024 keys inside every block of 8192 examples, as main() folds
    # B = 8192, the sessions keep a mean length of 8 to 10 at every B)
    block = torch.arange(B, device=dev) // 8192
    for sessions in ('user_id', 'single'):
      keys = session_keys(B, dev) % 1024 + 1024 * block if sessions == 'user_id' else torch.zeros(B, dtype=torch.int64, device=dev)
      for name, loss_type, param in KINDS:
        y = torch.rand(B, device=dev, generator=g) * (3.0 if loss_type == LT.LISTWISE_RANK_LOSS else 600.0)
        p = lwl.params_of(loss_type, param)
        labels, args = lwl.kernel_args(loss_type, y, p)
        got = {}

        def run_hip(tile=0):
          o = be.listwise_loss_tiled(z, labels, keys, tile=tile, **args)
          loss = torch.empty(1, device=dev)
          be.reduce_sum(o['loss_partials'], 1.0, loss)  # (the loss tail's share of a step: the sum of the partial rows)
          got[tile] = (loss, o['dlogits'], o['num_sessions'])

        def run_torch():
          zr = z.detach().clone().requires_grad_(True)
          loss = lwl.compose(loss_type, y, zr, keys, p)
          dz, = torch.autograd.grad(loss, zr)
          got['torch'] = (loss.detach().reshape(1), dz)

        run_torch()
        for tile in lwl.TILES + (0,):
          run_hip(tile)
        torch.cuda.synchronize()
        diff = {str(t): max(float((h - r).abs().max() / r.abs().max().clamp(min=1e-30)) for h, r in zip(got[t], got['torch']))
                for t in lwl.TILES}
        replays = [(_graphed(lambda t=t: run_hip(t)), max(1, a.iters // GRAPH_CALLS)) for t in lwl.TILES]
        wg = [[w / GRAPH_CALLS for w in ws] for ws in _alternating(replays, a.rounds)]
        wk, wt = _alternating([(run_hip, a.iters), (run_torch, a.torch_iters)], a.rounds)
        mk, mt, faster = verdict(wk, wt)
        line = dict(measure='listwise_tiled_fwd_bwd', kind=name, B=B, sessions=sessions, num_sessions=int(got[0][2]),
                    graph_us={str(t): w for t, w in zip(lwl.TILES, wg)},
                    graph_median_us={str(t): med(w) for t, w in zip(lwl.TILES, wg)}, default_tile=lwl.DEFAULT_TILE,
                    timing='eager', kernel_us=wk, torch_ops_us=wt, kernel_median_us=mk, torch_ops_median_us=mt,
                    kernel_faster=bool(faster), max_rel_diff=diff, clocks=clocks())
        print(json.dumps(line), flush=True)
        lines.append(line)
  summary = {'measure': 'summary', 'kernel_faster_at_every_shape': all(ln['kernel_faster'] for ln in lines),
             'fastest_tile': {'%s/%s/%d' % (ln['kind'], ln['sessions'], ln['B']): min(ln['graph_median_us'], key=ln['graph_median_us'].get)
                              for ln in lines},
             'iters': a.iters, 'torch_iters': a.torch_iters, 'rounds': a.rounds, 'device': be.device_info(), 'clocks': clocks()}
  print(json.dumps(summary), flush=True)
  return lines + [summary]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  ap.add_argument('--tiled', action='store_true', help='the sweep of er_listwise_tiled beyond B = 8192')
  ap.add_argument('--torch-iters', type=int, default=1, help='--tiled: calls of the composition a window')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('listwise_bench: needs a GPU')
  if a.tiled:
    lines = tiled(a)
    if a.out:
      with open(a.out, 'a') as f:
        for ln in lines:
          f.write(json.dumps(ln) + '\n')
    return
  dev = 'cuda:0'
  be = kernels.hip()
  g = torch.Generator(device=dev).manual_seed(1)
  lines = []
  for B in (1024, 4096, 8192):
    z = torch.randn(B, device=dev, generator=g)
    for sessions in ('user_id', 'single'):
      keys = session_keys(B, dev) % max(B // 8, 1) if sessions == 'user_id' else torch.zeros(B, dtype=torch.int64, device=dev)
      for name, loss_type, param in KINDS:
        y = torch.rand(B, device=dev, generator=g) * (3.0 if loss_type == LT.LISTWISE_RANK_LOSS else 600.0)
        p = lwl.params_of(loss_type, param)
        labels, args = lwl.kernel_args(loss_type, y, p)
        got = {}

        def run_hip():
          o = be.listwise_loss(z, labels, keys, **args)
          got['hip'] = (o['loss_partials'], o['dlogits'], o['num_sessions'])

        def run_torch():
          zr = z.detach().clone().requires_grad_(True)
          loss = lwl.compose(loss_type, y, zr, keys, p)
          dz, = torch.autograd.grad(loss, zr)
          got['torch'] = (loss.detach().reshape(1), dz)

        run_hip()
        run_torch()
        torch.cuda.synchronize()
        diff = max(float((h - t).abs().max() / t.abs().max().clamp(min=1e-30)) for h, t in zip(got['hip'], got['torch']))
        wk, wt = windows(run_hip, run_torch, a.iters, a.rounds, warmup=2, graph=False)
        mk, mt, faster = verdict(wk, wt)
        wg, _ = windows(run_hip, run_hip, 100, a.rounds, graph=True)
        line = dict(measure='listwise_fwd_bwd', kind=name, B=B, sessions=sessions, num_sessions=int(got['hip'][2]),
                    lds_bytes=int(be.lib.er_listwise_lds_bytes(B)), timing='eager', kernel_us=wk, torch_ops_us=wt,
                    kernel_median_us=mk, torch_ops_median_us=mt, kernel_faster=bool(faster), kernel_graph_us=wg,
                    max_rel_diff=diff, clocks=clocks())
        print(json.dumps(line), flush=True)
        lines.append(line)
  summary = {'measure': 'summary',
             'kernel_faster_at_every_shape': all(ln['kernel_faster'] for ln in lines),
             'kernel_not_faster_at': [[ln['kind'], ln['B'], ln['sessions']] for ln in lines if not ln['kernel_faster']],
             # the switch's default: 1 only if the kernel path is faster at every listed shape
             'switch_default_supported': '1' if lines and all(ln['kernel_faster'] for ln in lines) else '0',
             'iters': a.iters, 'rounds': a.rounds, 'device': be.device_info(), 'clocks': clocks()}
  # (the last thing this process does on the GPU: a refused capture ends here)
  summary['kernel_captures'], summary['composition_captures'] = _captures(run_hip), _captures(run_torch)
  print(json.dumps(summary), flush=True)
  lines.append(summary)
  if a.out:
    with open(a.out, 'a') as f:
      for ln in lines:
        f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
  main()
