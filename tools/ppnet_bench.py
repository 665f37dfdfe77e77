#!/usr/bin/env python
"""PPNet's gate kernel (er_gate_scale_*; kernels.GateScaleFn) against the torch composition x * (2 * sigmoid(z + bias)),
forward + backward through autograd, replayed from captured hipGraphs, each pair timed on the same inputs in one process
in ALTERNATING windows (tools/cmbf_bench.py windows / verdict).

Two measures per batch size:
  ppnet_gate_fwd_bwd   the part the switch replaces, alone: the gate operation at W = 512 and W = 256 (the Dense layers
                       around it left out on both sides), the bias gradient added into a given buffer on the kernel's
                       side and accumulated by autograd on the other.
  ppnet_layer_fwd_bwd  the PPNet layer of the sample (samples/model_config/ppnet_on_taobao.config: x 224 wide, gate
                       input 272 wide, MLP [512, 256], mode lazy) with EASYREC_AMD_FUSED_PPNET=1 and =0: the same HIP
                       contractions and BatchNorm launches either way.
At B = 1024 and 4096.

Every window is kept: a line holds the windows of each side (microseconds per call), their medians, and
`kernel_faster`: the medians differ in that direction by MORE than the larger spread (max - min) of the two sides'
windows - the spread of repeating the same variant in the same call.  Each line carries the rocm-smi clocks read when
it was written.  Prints one JSON line per measurement and appends them to --out.

usage: python tools/ppnet_bench.py [--iters 200] [--rounds 3] [--out FILE]
"""
import argparse
import gc
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
from easyrec_amd.layers.keras import ppnet as pn  # noqa: E402
from easyrec_amd.layers.utils import Parameter  # noqa: E402
from easyrec_amd.protos import layer_pb2  # noqa: E402

GATE_WIDTHS = [512, 256]
SAMPLE = ('mlp { hidden_units: [512, 256] } mode: "lazy" full_gate_input: true', 224, 48)  # (message, x, gate_input)
SWITCH = 'EASYREC_AMD_FUSED_PPNET'


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('ppnet_bench: needs a GPU')
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
              kernel_faster=bool(faster), max_rel_diff=diff))

  keep = os.environ.get(SWITCH)
  try:
    for B in (1024, 4096):
      # -- the gate operation alone
      for W in GATE_WIDTHS:
        x, z, dout = (torch.randn(B, W, device=dev, generator=g) for _ in range(3))
        bias = 0.1 * torch.randn(W, device=dev, generator=g)
        grads = [torch.zeros_like(bias)]
        tbias = bias.clone().requires_grad_(True)
        leaves = {side: [x.clone().requires_grad_(True), z.clone().requires_grad_(True)] for side in ('hip', 'torch')}

        def gate_hip():
          xi, zi = leaves['hip']
          xi.grad = zi.grad = None
          kernels.GateScaleFn.apply(grads, xi, zi, bias).backward(dout)

        def gate_torch():
          xi, zi = leaves['torch']
          xi.grad = zi.grad = tbias.grad = None
          pn.gate_scale_compose(xi, zi, tbias).backward(dout)

        gate_hip()
        gate_torch()
        diff = max(float((p.grad - q.grad).abs().max() / q.grad.abs().max()) for p, q in zip(leaves['hip'], leaves['torch']))
        measure({'B': B, 'W': W, 'measure': 'ppnet_gate_fwd_bwd', 'grid': be.gate_scale_grid(B, W)}, gate_hip, gate_torch,
                diff)

      # -- the layer with the switch at 1 and at 0
      text, wx, wg = SAMPLE
      pb = layer_pb2.PPNet()
      text_format.Merge(text, pb)
      store = VarStore(dev, seed=3)
      ctx = context.ModelContext(store, None, is_training=True)
      xin = torch.randn(B, wx, device=dev, generator=g)
      uin = torch.randn(B, wg, device=dev, generator=g)
      dy = torch.randn(B, 256, device=dev, generator=g)
      with context.use(ctx), torch.no_grad():
        layer = pn.PPNet(Parameter(pb, False, l2_reg=1e-6), name='ppnet')
        layer((xin, uin), training=True)
      store.pack()
      ctx.building = False
      got = {}

      def layer_run(flag):
        def run():
          # A batch-normalised MLP layer's autograd node keeps its own output (kernels.LinearBNActFn: ctx.own.y), a
          # reference cycle that outlives the call, and upstream of layer_1's node the composition hands gate_1's bias
          # gradient to autograd's AccumulateGrad node.  Left to the collector's own schedule that node, made on the
          # stream of an earlier call, would be met again inside a capture on another stream (torch.cuda.graph no
          # longer collects on entry) and pull its stream - the default one after the first call - into the capture.
          # Host time only: a replay does not run it.
          ctx.grad_slots.clear()
          gc.collect()
          os.environ[SWITCH] = flag
          store.zero_grad()
          xi, ui = xin.detach().requires_grad_(True), uin.detach().requires_grad_(True)
          with context.use(ctx):
            layer((xi, ui), training=True).backward(dy)
          got[flag] = (xi.grad, ui.grad)
        return run

      layer_run('1')()
      layer_run('0')()
      diff = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(got['1'], got['0']))
      measure({'B': B, 'W': wx, 'gate_input': wx + wg, 'mlp': [512, 256], 'measure': 'ppnet_layer_fwd_bwd'},
              layer_run('1'), layer_run('0'), diff)
  finally:
    if keep is None:
      os.environ.pop(SWITCH, None)
    else:
      os.environ[SWITCH] = keep

  summary = {'measure': 'summary',
             'kernel_faster_at_every_shape': all(ln['kernel_faster'] for ln in lines),
             'kernel_not_faster_at': [[ln['measure'], ln['B'], ln['W']] for ln in lines if not ln['kernel_faster']],
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
