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

usage: python tools/listwise_bench.py [--iters 20] [--rounds 3] [--out FILE]
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('listwise_bench: needs a GPU')
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
