#!/usr/bin/env python
"""The grouped-unit attention launches (er_mha_group_fwd / _bwd) against the one-unit launches (er_mha_fwd / _bwd) at
CMBF's sample shapes, and segment mean pooling (er_segment_mean_*) against its torch composition, each pair timed on
the same inputs in one process in ALTERNATING windows.

Attention: (F, T, ds) in (1, 33, 16), (33, 1, 16), (33, 33, 16), (1, 1, 16) with H = 2 at B = 1024 and 4096, forward
alone and forward + backward, separate Q and K | V buffers ((33, 33, 16) and (1, 1, 16) on the packed buffer too,
their form in the model); a [B, T] mask with random keys.  Segment mean: [B, 33, 32] in 11 segments (nine of width 1,
then 16 and 8) with random lengths, forward + backward through autograd.

The attention pairs are replayed from captured hipGraphs of 20 calls each (the host's share of a launch - allocation,
argument marshalling - is longer than these kernels and the same on both sides); segment mean forward + backward is
issued call by call (autograd runs its backward), its forward alone is replayed from graphs too.

Every window is kept: a line holds the three windows of each side (microseconds per call), their medians, and
`grouped_faster` / `kernel_faster`: the medians differ in that direction by MORE than the larger spread (max - min) of
the two sides' windows.  Prints one JSON line per measurement and appends them to --out.

usage: python tools/cmbf_bench.py [--iters 200] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.layers import multihead_cross_attention as mca  # noqa: E402

SHAPES = [(1, 33, 16), (33, 1, 16), (33, 33, 16), (1, 1, 16)]
H = 2
CMBF_SEG = list(range(10)) + [25, 33]


GRAPH_CALLS = 20  # calls per captured graph


def _graphed(fn):
  """fn() GRAPH_CALLS times as one hipGraph: a replay costs the device what the calls cost it, without the host's
  share of each launch (allocation, argument marshalling), which at these sizes is longer than the kernels."""
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


def windows(fa, fb, iters, rounds, warmup=5, graph=True):
  """-> (windows of fa, windows of fb) in us per call: `rounds` alternating windows of `iters` calls each; graph: the
  calls replayed from captured graphs of GRAPH_CALLS calls, else issued one by one from the host."""
  per = 1
  if graph:
    fa, fb, per = _graphed(fa), _graphed(fb), GRAPH_CALLS
  reps = max(1, iters // per)
  for _ in range(warmup):
    fa()
    fb()
  torch.cuda.synchronize()
  out = ([], [])
  for _ in range(rounds):
    for i, fn in enumerate((fa, fb)):
      start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      for _ in range(reps):
        fn()
      end.record()
      torch.cuda.synchronize()
      out[i].append(start.elapsed_time(end) * 1000.0 / (reps * per))
  return out


def verdict(new, old):
  """(median of new, median of old, new is faster by more than the larger spread of the windows)"""
  med = lambda w: sorted(w)[len(w) // 2]  # noqa: E731
  spread = max(max(new) - min(new), max(old) - min(old))
  return med(new), med(old), (med(old) - med(new)) > spread


def clocks():
  try:
    from bench import gpu_clocks
    return gpu_clocks()
  except Exception as e:  # (the figures stand without them)
    return {'unavailable': str(e)[:80]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('cmbf_bench: needs a GPU')
  dev = 'cuda:0'
  be = kernels.hip()
  g = torch.Generator(device=dev).manual_seed(1)
  lines = []

  def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)

  for B in (1024, 4096):
    for F, T, ds in SHAPES:
      d = H * ds
      G = be.mha_group_units(F, T, ds)
      forms = ['separate'] + (['packed'] if F == T else [])
      for form in forms:
        if form == 'packed':
          src = torch.randn(B * F, 3 * d, device=dev, generator=g)
          q, k, v = src[:, :d], src[:, d:2 * d], src[:, 2 * d:]
          dsrc = torch.empty_like(src)
          dq, dk, dv = dsrc[:, :d], dsrc[:, d:2 * d], dsrc[:, 2 * d:]
        else:
          q = torch.randn(B * F, d, device=dev, generator=g)
          kv = torch.randn(B * T, 2 * d, device=dev, generator=g)
          k, v = kv[:, :d], kv[:, d:]
          dq, dkv = torch.empty_like(q), torch.empty_like(kv)
          dk, dv = dkv[:, :d], dkv[:, d:]
        dctx = torch.randn(B * F, d, device=dev, generator=g)
        mask = (torch.rand(B, T, device=dev, generator=g) < 0.8).to(torch.int32)
        mask[:, 0] = 1

        def fwd(group):
          f = be.mha_group_fwd if group else be.mha_fwd
          return lambda: f(q, k, v, mask, B, F, T, H, ds)

        def both(group):
          f, b = (be.mha_group_fwd, be.mha_group_bwd) if group else (be.mha_fwd, be.mha_bwd)

          def run():
            f(q, k, v, mask, B, F, T, H, ds)
            b(q, k, v, mask, dctx, B, F, T, H, ds, dq, dk, dv)
          return run

        same = torch.equal(fwd(True)(), fwd(False)())
        for what, make in (('fwd', fwd), ('fwd_bwd', both)):
          wg, wo = windows(make(True), make(False), a.iters, a.rounds)
          mg, mo, faster = verdict(wg, wo)
          emit({'measure': 'attention_' + what, 'B': B, 'F': F, 'T': T, 'ds': ds, 'H': H, 'form': form, 'group_units': G,
                'lds_bytes_per_unit_bwd': be.mha_lds_bytes(F, T, ds, True), 'grouped_us': wg, 'one_unit_us': wo,
                'timing': 'graph replay', 'grouped_median_us': mg, 'one_unit_median_us': mo, 'grouped_faster': bool(faster), 'same_bits': bool(same)})

  # -- segment mean against its composition, forward + backward through autograd
  for B in (1024, 4096):
    x_h = torch.randn(B, 33, 32, device=dev, generator=g).requires_grad_(True)
    x_t = x_h.detach().clone().requires_grad_(True)
    widths = torch.tensor([b1 - b0 for b0, b1 in zip(CMBF_SEG, CMBF_SEG[1:])], device=dev)
    lens = ((torch.rand(B, 11, device=dev, generator=g) * widths).floor() + 1).to(torch.int32)
    dout = torch.randn(B, 11, 32, device=dev, generator=g)
    sb = torch.tensor(CMBF_SEG, dtype=torch.int32, device=dev)

    def seg_hip():
      x_h.grad = None
      kernels.SegmentMeanFn.apply(x_h, sb, lens, 11).backward(dout)

    def seg_torch():
      x_t.grad = None
      mca.segment_mean_compose(x_t, CMBF_SEG, lens).backward(dout)

    seg_hip()
    seg_torch()
    diff = float((x_h.grad - x_t.grad).abs().max())
    # (issued from the host one by one, as a step outside a captured graph issues them: autograd runs the backward)
    wk, wt = windows(seg_hip, seg_torch, a.iters, a.rounds, graph=False)
    mk, mt, faster = verdict(wk, wt)
    emit({'measure': 'segment_mean_fwd_bwd', 'timing': 'host-issued', 'B': B, 'S': 33, 'W': 32, 'n_seg': 11,
          'kernel_us': wk, 'torch_ops_us': wt, 'kernel_median_us': mk, 'torch_ops_median_us': mt,
          'kernel_faster': bool(faster), 'max_abs_diff_dx': diff})
    # the forward alone from captured graphs: the device's share
    xd = x_h.detach()
    wk, wt = windows(lambda: be.segment_mean_fwd(xd, sb, lens, 11), lambda: mca.segment_mean_compose(xd, CMBF_SEG, lens),
                     a.iters, a.rounds)
    mk, mt, faster = verdict(wk, wt)
    emit({'measure': 'segment_mean_fwd', 'timing': 'graph replay', 'B': B, 'S': 33, 'W': 32, 'n_seg': 11, 'kernel_us': wk,
          'torch_ops_us': wt, 'kernel_median_us': mk, 'torch_ops_median_us': mt, 'kernel_faster': bool(faster)})

  att = [ln for ln in lines if ln['measure'].startswith('attention')]
  summary = {'measure': 'summary',
             'grouped_faster_at_every_shape': all(ln['grouped_faster'] for ln in att),
             'grouped_not_faster_at': [[ln['measure'], ln['B'], ln['F'], ln['T'], ln['form']] for ln in att if not ln['grouped_faster']],
             'segment_mean_kernel_faster': all(ln['kernel_faster'] for ln in lines if ln['measure'].startswith('segment')),
             'iters': a.iters, 'rounds': a.rounds, 'device': be.device_info(), 'clocks': clocks()}
  print(json.dumps(summary), flush=True)
  lines.append(summary)
  if a.out:
    with open(a.out, 'a') as f:
      for ln in lines:
        f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
  main()
