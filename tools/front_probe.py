#!/usr/bin/env python
"""Probe: per-workgroup stamps of the fused front launch (emb_front_fwd_kernel: per-lookup sort + lookup) inside eager
DeepFM steps (er_debug_stamps; 100 MHz wall clock; the front's records stand 4096 * 16 words behind the backward launch's).

  python tools/front_probe.py [--steps N] [label:ENV=VALUE,ENV=VALUE ...]

Every argument is one variant: the environment it names is set while its steps run (the library reads its A/B switches
per launch).  Per variant, medians over the steps: the launch's span (first workgroup start to last wave end), the sort
workgroups' phases (build | radix sort, with its passes | key / entry stores | head flags, scan and their stores) of the
slowest sort workgroup, and the lookup workgroups' durations."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import logging  # noqa: E402

logging.disable(logging.WARNING)
from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.input.criteo_synthetic import SyntheticCriteo  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402

FRONT = 4096 * 16

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=12)
ap.add_argument('--config', default='configs/deepfm_criteo.config')
ap.add_argument('variants', nargs='*', default=['default:'])
args = ap.parse_args()

est = EasyRecEstimator(args.config, device='cuda:0', seed=1).build()
gen = SyntheticCriteo(est.pipeline_config.data_config, est.feature_configs, batch_size=4096, seed=3)
bs = [gen.next_batch() for _ in range(5 + args.steps)]
for b in bs[:5]:
  est.train_step(b)
torch.cuda.synchronize()
be = kernels.hip()
buf = torch.zeros(2 * FRONT, dtype=torch.int64, device='cuda:0')


def us(x):
  return float(x) / 100.0


for spec in args.variants:
  label, _, envs = spec.partition(':')
  pairs = [e.split('=', 1) for e in envs.split(',') if e]
  for k, v in pairs:
    os.environ[k] = v
  rows = []
  for b in bs[5:]:
    buf.zero_()
    torch.cuda.synchronize()
    be.lib.er_debug_stamps(buf.data_ptr())
    est.train_step(b)
    torch.cuda.synchronize()
    be.lib.er_debug_stamps(None)
    f = buf[FRONT:].cpu().numpy().reshape(-1, 16).astype(np.float64)
    used = f[:, 0] > 0
    if not used.any():
      raise SystemExit('no stamps: the fused front launch did not run')
    f = f[used]
    t0 = f[:, 0].min()
    is_sort = f[:, 2] > 0
    s, l = f[is_sort], f[~is_sort]
    slow = s[np.argmax(s[:, 1] - s[:, 0])]
    passes = [slow[8 + i] for i in range(8) if slow[8 + i] > 0]
    rec = dict(span=us(f[:, 1].max() - t0), n_sort=len(s), n_lookup=len(l),
               sort_max=us((s[:, 1] - s[:, 0]).max()), sort_end=us(s[:, 1].max() - t0),
               build=us(slow[2] - slow[0]), radix=us(slow[3] - slow[2]), stores=us(slow[4] - slow[3]),
               heads=us(slow[5] - slow[4]), n_pass=len(passes),
               per_pass=us((passes[-1] - slow[2]) / max(1, len(passes))) if passes else 0.0,
               look_p50=us(np.median(l[:, 1] - l[:, 0])) if len(l) else 0.0,
               look_max=us((l[:, 1] - l[:, 0]).max()) if len(l) else 0.0,
               look_start_last=us(l[:, 0].max() - t0) if len(l) else 0.0,
               look_end=us(l[:, 1].max() - t0) if len(l) else 0.0)
    rows.append(rec)
  for k, _ in pairs:
    del os.environ[k]
  med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
  print('%-14s span %6.2f us | sort wgs %d: slowest %5.2f (build %.2f | radix %.2f = %d passes of %.2f | stores %.2f | heads %.2f), '
        'last ends %5.2f | lookup wgs %d: dur p50 %.2f max %.2f, last starts %.2f, last ends %.2f   [%d steps, spans %.2f-%.2f]' % (
            label, med['span'], med['n_sort'], med['sort_max'], med['build'], med['radix'], med['n_pass'], med['per_pass'],
            med['stores'], med['heads'], med['sort_end'], med['n_lookup'], med['look_p50'], med['look_max'],
            med['look_start_last'], med['look_end'], len(rows), min(r['span'] for r in rows), max(r['span'] for r in rows)),
        flush=True)
