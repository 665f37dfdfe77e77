#!/usr/bin/env python
"""MaskNet's kernels (er_mask_mul_*, er_ln_relu_*; kernels.MaskMulFn / LnReluFn) against the torch composition, forward +
backward through autograd, replayed from captured hipGraphs, each pair timed on the same inputs in one process in
ALTERNATING windows (tools/cmbf_bench.py windows / verdict).

Two measures per shape:
  masknet_fns_fwd_bwd    the part the switch replaces, alone: n mask multiplies of one input, and LayerNorm + ReLU of n
                         [B, O] tensors into their concatenation (the Dense layers between them left out on both sides).
  masknet_layer_fwd_bwd  the MaskNet layer (model-level input layer norm, n parallel blocks, no MLP) with
                         EASYREC_AMD_FUSED_MASKNET=1 and =0: the same HIP contractions either way.
Shapes: the sample's (samples/model_config/masknet_on_taobao.config: W = 272, aggregation 512, output 256, 3 blocks)
and the movielens sample's width (W = 128), at B = 1024 and 4096.

Every window is kept: a line holds the windows of each side (microseconds per call), their medians, and
`kernel_faster`: the medians differ in that direction by MORE than the larger spread (max - min) of the two sides'
windows - the spread of repeating the same variant in the same call.  Each line carries the rocm-smi clocks read when
it was written.  Prints one JSON line per measurement and appends them to --out.

usage: python tools/masknet_bench.py [--iters 200] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch
from google.protobuf import text_format

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cmbf_bench import clocks, verdict, windows  # noqa: E402
from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.core import context  # noqa: E402
from easyrec_amd.core.variables import VarStore  # noqa: E402
from easyrec_amd.layers.keras import mask_net as mn  # noqa: E402
from easyrec_amd.layers.utils import Parameter  # noqa: E402
from easyrec_amd.protos import layer_pb2  # noqa: E402

SHAPES = [(272, 512, 256, 3), (128, 512, 256, 3)]  # (W, aggregation, output, blocks)
SWITCH = 'EASYREC_AMD_FUSED_MASKNET'


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('masknet_bench: needs a GPU')
  dev = 'cuda:0'
  be = kernels.hip()
  g = torch.Generator(device=dev).manual_seed(1)
  lines = []

  def emit(line):
    line = dict(line, clocks=clocks())
    print(json.dumps(line), flush=True)
    lines.append(line)

  def measure(line, hip_fn, torch_fn, diff):
    wk, wt = windows(hip_fn, torch_fn, a.iters, a.rounds, graph=True)
    mk, mt, faster = verdict(wk, wt)
    emit(dict(line, timing='graph replay', kernel_us=wk, torch_ops_us=wt, kernel_median_us=mk, torch_ops_median_us=mt,
              kernel_faster=bool(faster), max_rel_diff_dx=diff))

  keep = os.environ.get(SWITCH)
  try:
    for B in (1024, 4096):
      for W, A, O, n in SHAPES:
        shape = {'B': B, 'W': W, 'aggregation': A, 'output': O, 'blocks': n}
        # -- the two functions alone
        x = torch.randn(B, W, device=dev, generator=g)
        vs_ = [torch.randn(B, W, device=dev, generator=g) for _ in range(n)]
        hs = [torch.randn(B, O, device=dev, generator=g) for _ in range(n)]
        gb = [t for _ in range(n) for t in (1.0 + 0.1 * torch.randn(O, device=dev, generator=g),
                                            0.1 * torch.randn(O, device=dev, generator=g))]
        grads = [torch.zeros_like(t) for t in gb]
        tgb = [t.clone().requires_grad_(True) for t in gb]
        douts = [torch.randn(B, W, device=dev, generator=g) for _ in range(n)]
        dy = torch.randn(B, n * O, device=dev, generator=g)
        leaves = {}
        for side in ('hip', 'torch'):
          leaves[side] = ([x.clone().requires_grad_(True)] + [v.clone().requires_grad_(True) for v in vs_],
                          [h.clone().requires_grad_(True) for h in hs])

        def clear(side):
          for group in leaves[side]:
            for t in group:
              t.grad = None

        def fns_hip():
          clear('hip')
          (xi, *vi), hi = leaves['hip']
          torch.autograd.backward(list(kernels.MaskMulFn.apply(xi, *vi)), douts)
          kernels.LnReluFn.apply(mn.LN_EPSILON, grads, None, 0, *(hi + gb)).backward(dy)

        def fns_torch():
          clear('torch')
          for t in tgb:
            t.grad = None
          (xi, *vi), hi = leaves['torch']
          torch.autograd.backward([xi * v for v in vi], douts)
          torch.cat([torch.relu(mn.layer_norm_compose(h, tgb[2 * i], tgb[2 * i + 1])) for i, h in enumerate(hi)],
                    dim=1).backward(dy)

        fns_hip()
        fns_torch()
        diff = max(float((p.grad - q.grad).abs().max() / q.grad.abs().max())
                   for p, q in zip(leaves['hip'][0][:1] + leaves['hip'][1], leaves['torch'][0][:1] + leaves['torch'][1]))
        measure(dict(shape, measure='masknet_fns_fwd_bwd', ln_relu_grid=be.ln_relu_grid(B, O, n)), fns_hip, fns_torch, diff)

        # -- the layer with the switch at 1 and at 0
        pb = layer_pb2.MaskNet()
        text_format.Merge(('mask_blocks { aggregation_size: %d output_size: %d } ' % (A, O)) * n, pb)
        store = VarStore(dev, seed=3)
        ctx = context.ModelContext(store, None, is_training=True)
        xin = torch.randn(B, W, device=dev, generator=g)
        dout = torch.randn(B, n * O, device=dev, generator=g)
        with context.use(ctx), torch.no_grad():
          layer = mn.MaskNet(Parameter(pb, False, l2_reg=1e-6), name='mask_net')
          layer(xin, training=True)
        store.pack()
        ctx.building = False
        got = {}

        def layer_run(flag):
          def run():
            os.environ[SWITCH] = flag
            store.zero_grad()
            ctx.grad_slots.clear()
            xi = xin.detach().requires_grad_(True)
            with context.use(ctx):
              layer(xi, training=True).backward(dout)
            got[flag] = xi.grad
          return run

        layer_run('1')()
        layer_run('0')()
        diff = float((got['1'] - got['0']).abs().max() / got['0'].abs().max())
        measure(dict(shape, measure='masknet_layer_fwd_bwd'), layer_run('1'), layer_run('0'), diff)
  finally:
    if keep is None:
      os.environ.pop(SWITCH, None)
    else:
      os.environ[SWITCH] = keep

  sample = [ln for ln in lines if ln['W'] == 272 and ln['measure'] == 'masknet_layer_fwd_bwd']
  summary = {'measure': 'summary',
             'kernel_faster_at_every_shape': all(ln['kernel_faster'] for ln in lines),
             'kernel_not_faster_at': [[ln['measure'], ln['B'], ln['W']] for ln in lines if not ln['kernel_faster']],
             # the switch's default: 1 only if the layer on the kernels is faster at both B of the sample shape
             'switch_default_supported': '1' if sample and all(ln['kernel_faster'] for ln in sample) else '0',
             'iters': a.iters, 'rounds': a.rounds, 'device': be.device_info(), 'clocks': clocks()}
  print(json.dumps(summary), flush=True)
  lines.append(summary)
  if a.out:
    with open(a.out, 'a') as f:
      for ln in lines:
        f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
  main()
