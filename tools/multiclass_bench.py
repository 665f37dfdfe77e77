#!/usr/bin/env python
"""The multi-logit head kernels (er_softmax_ce, er_jrc; builders/multiclass_loss.py) against their torch compositions
(softmax_ce_compose / jrc_compose differentiated by autograd, plus the softmax the head's `probs` need), replayed from
captured hipGraphs, each pair timed on the same inputs in one process in ALTERNATING windows (tools/cmbf_bench.py windows
/ verdict).  Both sides yield the loss value, d loss / d logits and the probabilities; the kernel's side includes the sum
of its per-workgroup loss partials as a launch of its own, which inside a training step rides in the loss tail's launch.

Shapes: B = 1024 and 4096; softmax cross entropy at C = 2, 5 and 64 with per-example weights; JRC on the `user_id`
sessions that input/synthetic.py draws for configs/dbmtl_jrc_small_taobao.config (the composition builds [B, B, 2]
tensors).

Every window is kept: a line holds the windows of each side (microseconds per call), their medians, and
`kernel_faster`: the medians differ in that direction by MORE than the larger spread (max - min) of the two sides'
windows.  Each line carries the rocm-smi clocks read when it was written.  Prints one JSON line per measurement and
appends them to --out.

usage: python tools/multiclass_bench.py [--iters 200] [--rounds 3] [--out FILE]
"""
import argparse
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cmbf_bench import clocks, verdict, windows  # noqa: E402
from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.builders import multiclass_loss as mcl  # noqa: E402


def _rel(a, b):
  return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def session_keys(B, dev):
  """the user_id id column of a synthetic batch of configs/dbmtl_jrc_small_taobao.config at batch size B"""
  from easyrec_amd.input.features import feature_name_of
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.utils import config_util
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'dbmtl_jrc_small_taobao.config'))
  fcs = config_util.get_compatible_feature_configs(cfg)
  gen = SyntheticBatches(cfg.data_config, fcs, batch_size=B, seed=3)
  col = gen.schema.hash_single['user_id']['col']
  assert 'user_id' in {feature_name_of(fc) for fc in fcs}
  return torch.from_numpy(gen.next_batch()['hash_ids'][col]).to(dev)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=200)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--out', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('multiclass_bench: needs a GPU')
  dev = 'cuda:0'
  be = kernels.hip()
  g = torch.Generator(device=dev).manual_seed(1)
  lines = []

  def emit(line):
    line = dict(line, clocks=clocks())
    print(json.dumps(line), flush=True)
    lines.append(line)

  def measure(tag, run_hip, run_torch, got, extra):
    run_hip()
    run_torch()
    torch.cuda.synchronize()
    diff = max(_rel(got['hip'][k], got['torch'][k]) for k in ('loss', 'dz', 'probs'))
    wk, wt = windows(run_hip, run_torch, a.iters, a.rounds, graph=True)
    mk, mt, faster = verdict(wk, wt)
    emit(dict(extra, measure=tag, timing='graph replay', kernel_us=wk, torch_ops_us=wt, kernel_median_us=mk,
              torch_ops_median_us=mt, kernel_faster=bool(faster), max_rel_diff=diff))

  for B in (1024, 4096):
    w = torch.rand(B, device=dev, generator=g) + 0.5
    w[torch.rand(B, device=dev, generator=g) < 0.1] = 0.0
    for C in (2, 5, 64):
      z = torch.randn(B, C, device=dev, generator=g)
      y = torch.randint(0, C, (B,), device=dev, generator=g)
      yf = y.to(torch.float32)
      got = {'hip': {}, 'torch': {}}

      def run_hip():
        o = be.softmax_ce(z, yf, w, 1.0)
        got['hip'] = {'loss': o['loss_partials'].sum().reshape(1), 'dz': o['dlogits'], 'probs': o['probs']}

      def run_torch():
        gc.collect()
        zr = z.detach().clone().requires_grad_(True)
        loss = mcl.softmax_ce_compose(y, zr, w)
        dz, = torch.autograd.grad(loss, zr)
        got['torch'] = {'loss': loss.detach().reshape(1), 'dz': dz, 'probs': torch.softmax(z, dim=1)}

      measure('softmax_ce_fwd_bwd', run_hip, run_torch, got, {'B': B, 'C': C, 'grid': be.softmax_ce_grid(B, C)})

    z = torch.randn(B, 2, device=dev, generator=g)
    y = (torch.rand(B, device=dev, generator=g) < 0.25).to(torch.int64)
    yf = y.to(torch.float32)
    keys = session_keys(B, dev)
    got = {'hip': {}, 'torch': {}}

    def run_hip_jrc():
      o = be.jrc(z, yf, keys, w, 0.5)
      got['hip'] = {'loss': o['loss_partials'].sum().reshape(1), 'dz': o['dlogits'], 'probs': o['probs']}

    def run_torch_jrc():
      gc.collect()
      zr = z.detach().clone().requires_grad_(True)
      loss = mcl.jrc_compose(y, zr, keys, 0.5, w, True)
      dz, = torch.autograd.grad(loss, zr)
      got['torch'] = {'loss': loss.detach().reshape(1), 'dz': dz, 'probs': torch.softmax(z, dim=1)[:, 1]}

    measure('jrc_fwd_bwd', run_hip_jrc, run_torch_jrc, got,
            {'B': B, 'C': 2, 'grid': be.jrc_grid(B), 'sessions': int(torch.unique(keys).numel())})

  summary = {'measure': 'summary',
             'kernel_faster_at_every_shape': all(ln['kernel_faster'] for ln in lines),
             'kernel_not_faster_at': [[ln['measure'], ln['B'], ln['C']] for ln in lines if not ln['kernel_faster']],
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
