"""Times forward + backward of MIND's capsule routing and of its label-aware attention, the fused kernels
(csrc/er_capsule.hip) against the same ops composed of torch ops (layers/capsule_layer.py), on one GPU at the taobao
config's shape.  The two sides alternate in one process, ROUNDS rounds of ITERS calls each, first as eager calls and then
as replays of a captured hipGraph (what a training step is); min / mean / max of the rounds' per-call times per side, and
the device launches of one call per side counted by torch.profiler.  One JSON line per block and mode.
usage: python tools/mind_bench.py [--batch 4096] [--seq 64] [--dim 16] [--high 64] [--k 5] [--iters-routing 3]
                                  [--att-dim 32] [--rounds 7] [--iters 50] [--att-iters 1000]
(the attention call takes tens of microseconds, so a round of it times --att-iters calls: a window of 20 ms or more)"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def count_launches(call):
  """device kernels of one call, or None where the profiler reports no device activity"""
  from torch.profiler import ProfilerActivity, profile
  torch.cuda.synchronize()
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    call()
    torch.cuda.synchronize()
  n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
          and 'memset' not in e.name.lower())
  return n or None


def time_sides(sides, rounds, iters, graph):
  """per side the rounds' microseconds per call; graph: each side captured once, its replays timed"""
  runs = {}
  for name, call in sides.items():
    for _ in range(5):
      call()
    if graph:
      s = torch.cuda.Stream()
      s.wait_stream(torch.cuda.current_stream())
      with torch.cuda.stream(s):
        call()
      torch.cuda.current_stream().wait_stream(s)
      g = torch.cuda.CUDAGraph()
      with torch.cuda.graph(g):
        call()
      runs[name] = g.replay
    else:
      runs[name] = call
  torch.cuda.synchronize()
  times = {k: [] for k in sides}
  for _ in range(rounds):
    for name, run in runs.items():
      start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      for _ in range(iters):
        run()
      stop.record()
      torch.cuda.synchronize()
      times[name].append(start.elapsed_time(stop) * 1e3 / iters)
  return times


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=4096)
  ap.add_argument('--seq', type=int, default=64)
  ap.add_argument('--dim', type=int, default=16)
  ap.add_argument('--high', type=int, default=64)
  ap.add_argument('--k', type=int, default=5)
  ap.add_argument('--iters-routing', type=int, default=3)
  ap.add_argument('--att-dim', type=int, default=32)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--iters', type=int, default=50)
  ap.add_argument('--att-iters', type=int, default=1000)
  args = ap.parse_args()
  from easyrec_amd import kernels
  from easyrec_amd.layers import capsule_layer
  dev = 'cuda:0'
  info = kernels.hip().device_info()
  B, S, D, E, K = args.batch, args.seq, args.dim, args.high, args.k
  g = torch.Generator().manual_seed(1)
  hist = (torch.randn(B, S, D, generator=g) * 0.5).to(dev).requires_grad_(True)
  lens = torch.randint(1, S + 1, (B,), generator=g).to(torch.int32).to(dev)
  Smat = (torch.randn(D, E, generator=g) / D ** 0.5).to(dev).requires_grad_(True)
  logits0 = torch.clamp(torch.randn(B, S, K, generator=g), -2, 2).to(dev)
  d_high = torch.randn(B, K, E, generator=g).to(dev)
  cfg = (S, K, args.iters_routing, 20.0, 1.0, 1.0, False)
  assert capsule_layer.capsule_fits(hist, S, E, K, args.iters_routing)

  def capsule(fused):
    def call():
      hist.grad = Smat.grad = None
      if fused:
        high, _ = kernels.CapsuleRoutingFn.apply(hist, lens, logits0, cfg, None, Smat)
      else:
        high, _ = capsule_layer.capsule_compose(hist, lens, Smat, logits0, *cfg)
      high.backward(d_high)
    return call

  A = args.att_dim
  x = (torch.randn(B, K, A, generator=g) / A ** 0.5).to(dev).requires_grad_(True)
  pos = torch.randn(B, A, generator=g).to(dev).requires_grad_(True)
  ncaps = capsule_layer.num_capsules(lens, S, K, False)
  d_emb, d_ui = torch.randn(B, A, generator=g).to(dev), torch.randn(B, K, A, generator=g).to(dev)

  def attention(fused):
    def call():
      x.grad = pos.grad = None
      if fused:
        emb, ui = kernels.MindAttentionFn.apply(x, pos, ncaps, 10.0)
      else:
        emb, ui = capsule_layer.attention_compose(x, pos, ncaps, 10.0)
      torch.autograd.backward([emb, ui], [d_emb, d_ui])
    return call

  blocks = {'capsule_fwd_bwd': ({'fused': capsule(True), 'composed': capsule(False)},
                                dict(B=B, S=S, D=D, E=E, K=K, num_iters=args.iters_routing), args.iters),
            'mind_attention_fwd_bwd': ({'fused': attention(True), 'composed': attention(False)}, dict(B=B, K=K, E=A),
                                       args.att_iters)}
  for bench, (sides, shape, iters) in blocks.items():
    launches = {name: count_launches(call) for name, call in sides.items()}
    for mode in ('eager', 'graph'):
      times = time_sides(sides, args.rounds, iters, mode == 'graph')
      line = dict(bench=bench, mode=mode, rounds=args.rounds, iters=iters, device=info, **shape)
      for name, ts in times.items():
        line[name + '_us'] = {'min': round(min(ts), 1), 'mean': round(sum(ts) / len(ts), 1), 'max': round(max(ts), 1)}
        line[name + '_launches'] = launches[name]
      line['fused_wins'] = line['fused_us']['max'] < line['composed_us']['min']
      print(json.dumps(line), flush=True)


if __name__ == '__main__':
  main()
