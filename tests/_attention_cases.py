"""Cases, input builders and fp64 references for the attention cores at the edges of their envelopes: csrc/er_mha.hip
(er_mha_fwd / _bwd / er_mha_group_*) and csrc/er_autoint.hip (er_autoint_attn_fwd / _bwd).  No backend is imported
here: tests/test_attention_pins.py (CPU) and tests/test_attention_edges_gpu.py (GPU) share this module.

Reference.  Nothing is restated: the fp64 values are oracle/uniter_ref.attention_core (with its mixed_mask) and
oracle/autoint_ref.attention_core under torch.autograd.  Inputs are fp64 tensors that hold fp32 values, so the fp64
evaluation starts from exactly the numbers the kernels read.  The "plain fp32" evaluation the CPU test measures is the
product's composition (layers/multihead_cross_attention.attention_compose, which applies the mask's adder relative to
the row's largest as the kernels do) and the AutoInt oracle at torch.float32.

Bars.  tests/_oracle_steps.close (max error over max value): FWD_BAR forward, GRAD_BAR gradients.  A case whose plain
fp32 evaluation already sits above one third of a default bar gets a bar of its own, 4 x that measured error (the
headroom covers another summation order: the kernels sum k = 0, 1, .. in one thread, torch in blocks).  Such bars are
recorded in MHA_BARS / AI_BARS with the measurement beside them; test_attention_pins.py re-measures every (case,
tensor) and holds the record to it.
"""
import functools

import torch

from oracle import autoint_ref
from oracle import uniter_ref

F64, F32 = torch.float64, torch.float32
FWD_BAR, GRAD_BAR = 1e-5, 1e-4
MHA_BUDGET, MHA_MAX_LEN, MHA_MAX_DS, MHA_GRID = 81920, 4096, 128, 1024
AI_BUDGET, AI_MAX_EPB = 65536, 8
WAVE = 64


def odd(n):
  return n | 1


def mha_bytes(F, T, ds, bwd=True):
  """include/easyrec_hip.h K8f: er_mha_lds_bytes' closed form (0 for an empty argument)."""
  if F < 1 or T < 1 or ds < 1:
    return 0
  if bwd:
    return 4 * ((2 * F + 2 * T) * odd(ds) + 2 * F * odd(T) + T)
  return 4 * ((F + 2 * T) * odd(ds) + F * odd(T) + T)


def mha_inside(F, T, ds):
  """mha_shape_ok: the lengths 1 .. 4096, the head size 1 .. 128, the backward's bytes within the budget."""
  return 1 <= F <= MHA_MAX_LEN and 1 <= T <= MHA_MAX_LEN and 1 <= ds <= MHA_MAX_DS and mha_bytes(F, T, ds) <= MHA_BUDGET


def mha_units(F, T, ds):
  """er_mha_group_units' closed form."""
  if not mha_inside(F, T, ds):
    return 0
  for g in (8, 4, 2):
    if g * mha_bytes(F, T, ds) <= MHA_BUDGET:
      return g
  return 1


def ai_bytes(F, H, ds, bwd=True):
  """include/easyrec_hip.h K8c: er_autoint_lds_bytes' closed form; bwd=False: the forward kernel's (Q | K | V rows, P)."""
  d = H * ds
  return 4 * (F * odd(3 * d) + F * odd(d) + 2 * H * F * F) if bwd else 4 * (F * odd(3 * d) + H * F * F)


def ai_epb(F, H, ds, bwd):
  """er_autoint_epb: examples per workgroup, min(8, 65536 // bytes)."""
  return min(AI_MAX_EPB, AI_BUDGET // ai_bytes(F, H, ds, bwd))


# ------------------------------------------------------------------------------------------------------------------
# er_mha_*: (F, T, H, ds), the batch, the backward's LDS bytes and the units per workgroup the tag is named for
# ------------------------------------------------------------------------------------------------------------------
MHA_CASES = {
    't200_f1': dict(F=1, T=200, H=2, ds=8, B=5, bytes=16880, G=4),        # key stride, ragged last round (200 = 3 * 64 + 8)
    't70_f70': dict(F=70, T=70, H=1, ds=8, B=4, bytes=50120, G=1),        # one unit; the key and the row stride both
    'f130_t3': dict(F=130, T=3, H=2, ds=4, B=5, bytes=8452, G=8),         # grouped: 130 softmax rows on one wave
    'f4096_t1': dict(F=4096, T=1, H=1, ds=1, B=2, bytes=65548, G=1),      # one key: P = 1 exactly; 512 rows a wave
    't4095_f1': dict(F=1, T=4095, H=1, ds=1, B=2, bytes=81908, G=1),      # the last T inside; 64 rounds, the last ragged
    'edge_ds128': dict(F=34, T=34, H=2, ds=128, B=3, bytes=79832, G=1),   # the last square inside at ds = 128
    'g2': dict(F=48, T=48, H=2, ds=16, B=3, bytes=32064, G=2),            # two units per workgroup
    'm_rem2': dict(F=6, T=7, H=1, ds=5, B=9, bytes=884, G=8),             # mha_mm: M % 4 = 2 (F as M), 3 (T as M)
    'm_rem3': dict(F=7, T=6, H=1, ds=5, B=7, bytes=936, G=8),             # mha_mm: M % 4 = 3 (F as M), 2 (T as M)
}
# saturated rows: q scaled so that the largest score of the fp64 reference is `top`; never masked
MHA_SAT_CASES = {
    't70_f70_top30': dict(F=70, T=70, H=1, ds=8, B=4, top=30.0),
    't70_f70_top80': dict(F=70, T=70, H=1, ds=8, B=4, top=80.0),
    'sample_top30': dict(F=33, T=33, H=4, ds=128, B=5, top=30.0),
    'sample_top80': dict(F=33, T=33, H=4, ds=128, B=5, top=80.0),
}
MHA_ALL = dict(MHA_CASES, **MHA_SAT_CASES)
MHA_SEEDS = {tag: 100 + i for i, tag in enumerate(MHA_CASES)}
# (chosen for the gap between the two best scores of every row: SAT_MIN_GAP below.  Seed 109 leaves 3e-4 / 2e-5.)
MHA_SEEDS.update(t70_f70_top30=104, t70_f70_top80=104, sample_top30=101, sample_top80=101)
# (t4095_f1 has two context values in all, each a weighted mean of 4095 values of either sign: at seed 104 the fp64
# reference cancels to 0.009 against terms of 0.8 in sum; at 107 it is 0.04 and 0.07)
MHA_SEEDS.update(t4095_f1=107)
MHA_TENSORS = ('ctx', 'dq', 'dk', 'dv')
SAT_MIN_GAP = 1e-3  # between the two best scores of every row (fp64): no near tie for fp32 rounding to decide
# (tag, masked): every case masked and unmasked, the saturated ones unmasked
MHA_RUNS = [(tag, m) for tag in MHA_CASES for m in (False, True)] + [(tag, False) for tag in MHA_SAT_CASES]


def mha_run_id(v):
  return v if isinstance(v, str) else ('mask' if v else 'nomask')


# (tag, masked, tensor) -> (plain fp32 error over max value measured on the CPU, the bar = 4 x it); anything absent
# measured at or below a third of its default bar and keeps it
MHA_BARS = {
    # a score of 80 over ds = 128 carries ~1e-5 of absolute fp32 rounding: measured 6.65e-06, bar 2.66e-05
    ('sample_top80', False, 'ctx'): (6.65e-06, 2.66e-05),
}

# the envelope from both sides: both neighbours of every edge case, the bounds, empty arguments
MHA_GRID_SHAPES = sorted({(c['F'], c['T'], c['ds']) for c in MHA_CASES.values()} | {
    (34, 34, 127), (34, 34, 128), (34, 34, 129), (35, 34, 128), (34, 35, 128), (35, 35, 128), (33, 33, 128),
    (1, 4094, 1), (1, 4095, 1), (1, 4096, 1), (2, 4095, 1), (1, 4095, 2), (4095, 1, 1), (4096, 1, 1), (4097, 1, 1),
    (1, 4097, 1), (4096, 1, 2), (4096, 1, 3), (70, 70, 8), (71, 71, 8), (90, 90, 8), (91, 91, 8), (48, 48, 16),
    (47, 47, 16), (57, 57, 16), (58, 58, 16), (33, 33, 16), (32, 32, 16), (21, 21, 16), (22, 22, 16), (1, 1, 1),
    (1, 1, 128), (1, 1, 129), (0, 5, 4), (5, 0, 4), (5, 5, 0), (0, 0, 0), (-1, 5, 4),
})
MHA_OUTSIDE = dict(F=35, T=35, H=1, ds=128, B=3, bytes=82180)  # the first square outside at ds = 128: the composition


def mha_batch(tag, masked):
  """The mask's four special examples need four rows: a masked run with T > 64 has at least 4 examples."""
  c = MHA_ALL[tag]
  return max(c['B'], 4) if masked and c['T'] > WAVE else c['B']


def mha_mask(B, T, seed):
  """uniter_ref.mixed_mask (example 0 one open key, example 1 every key masked); where the key loop takes more than one
  round, example 2's only open key is the last one and example 3's only open key is j = 64, the first of round two."""
  m = uniter_ref.mixed_mask(B, T, seed)
  for row, key in ((2, T - 1), (3, WAVE)):
    if T > WAVE and row < B:  # (the case runs have B >= 4: mha_batch; a grouped launch of fewer units has what fits)
      m[row] = 0
      m[row, key] = 1
  return m


def _f32_values(t):
  return t.to(F32).to(F64)


def mha_scores(q, k, B, F, T, H, ds):
  """The fp64 scores [B, H, F, T] before the mask."""
  q4 = q.reshape(B, F, H, ds).permute(0, 2, 1, 3)
  k4 = k.reshape(B, T, H, ds).permute(0, 2, 1, 3)
  return torch.matmul(q4, k4.transpose(-1, -2)) / float(ds) ** 0.5


@functools.lru_cache(maxsize=None)
def mha_inputs(tag, masked):
  """-> dict(q [B F, d], k, v [B T, d], dctx [B F, d]: fp64 holding fp32 values; mask int32 [B, T] or None; B)"""
  c = MHA_ALL[tag]
  F, T, H, ds = c['F'], c['T'], c['H'], c['ds']
  B, d = mha_batch(tag, masked), H * ds
  g = torch.Generator().manual_seed(MHA_SEEDS[tag])
  q, k, v, dctx = (_f32_values(torch.randn(B * n, d, generator=g, dtype=F64)) for n in (F, T, T, F))
  if 'top' in c:
    assert not masked
    q = _f32_values(q * (c['top'] / float(mha_scores(q, k, B, F, T, H, ds).max())))
  mask = mha_mask(B, T, MHA_SEEDS[tag]) if masked else None
  return dict(q=q, k=k, v=v, dctx=dctx, mask=mask, B=B)


def mha_eval(tag, masked, dt, fn):
  """fn(q, k, v, mask, B, F, T, H, ds) at dtype dt under autograd -> dict(ctx, dq, dk, dv), detached."""
  c, inp = MHA_ALL[tag], mha_inputs(tag, masked)
  q, k, v = (inp[n].to(dt).clone().requires_grad_(True) for n in ('q', 'k', 'v'))
  ctx = fn(q, k, v, inp['mask'], inp['B'], c['F'], c['T'], c['H'], c['ds'])
  dq, dk, dv = torch.autograd.grad(ctx, (q, k, v), inp['dctx'].to(dt))
  return dict(ctx=ctx.detach(), dq=dq, dk=dk, dv=dv)


@functools.lru_cache(maxsize=None)
def mha_reference(tag, masked):
  """The fp64 reference of a case, computed once and shared: read it, never write to it."""
  return mha_eval(tag, masked, F64, uniter_ref.attention_core)


def mha_bar(tag, masked, tensor):
  return MHA_BARS.get((tag, masked, tensor), (None, FWD_BAR if tensor == 'ctx' else GRAD_BAR))[1]


def mha_top_gap(tag):
  """(the largest score, the smallest gap between the two best scores of a row) of the unmasked fp64 reference."""
  c, inp = MHA_ALL[tag], mha_inputs(tag, False)
  s = mha_scores(inp['q'], inp['k'], inp['B'], c['F'], c['T'], c['H'], c['ds'])
  best = s.topk(2, dim=-1).values
  return float(s.max()), float((best[..., 0] - best[..., 1]).min())


# ------------------------------------------------------------------------------------------------------------------
# er_autoint_attn_*: (F, H, ds) and the examples per workgroup of the backward and the forward kernel
# ------------------------------------------------------------------------------------------------------------------
AI_CASES = {
    'f1': dict(F=1, H=2, ds=4, epb_bwd=8, epb_fwd=8),        # one field: P = 1, dS = 0, dQ = dK = 0, y = relu(V + R)
    'f89': dict(F=89, H=1, ds=1, epb_bwd=1, epb_fwd=2),      # 64792 bytes: the last F inside (the forward's 32752: 2)
    'd128': dict(F=18, H=2, ds=64, epb_bwd=1, epb_fwd=2),    # the kernels disagree on the examples per workgroup
    'f60': dict(F=60, H=1, ds=4, epb_bwd=1, epb_fwd=3),
    'mid': dict(F=20, H=2, ds=16, epb_bwd=3, epb_fwd=5),     # 16800 bytes: an epb strictly between 1 and 8 in both
    'd128_top80': dict(F=18, H=2, ds=64, epb_bwd=1, epb_fwd=2, top=80.0),  # the largest sqrt(ds) q . k is 80
}
AI_SEEDS = {tag: 200 + i for i, tag in enumerate(AI_CASES)}
AI_TENSORS = ('y', 'dq', 'dk', 'dv', 'dr')

# (tag, tensor) -> (measured, bar), as MHA_BARS; one record per case, held at every batch size
AI_BARS = {
    # the largest over B in {1, 2, 3, 5}: measured 3.57e-06, bar 1.428e-05
    ('d128_top80', 'y'): (3.57e-06, 1.428e-05),
}

AI_GRID_SHAPES = sorted({(c['F'], c['H'], c['ds']) for c in AI_CASES.values()} | {
    (F, 1, 1) for F in (88, 89, 90, 91)} | {(88, 1, 2), (89, 1, 2), (89, 2, 1), (64, 2, 1), (63, 2, 1)} | {
    (F, 2, ds) for F in (17, 18, 19) for ds in (63, 64, 65, 79, 80, 81, 104, 105, 106)} | {(1, 1, 4095), (1, 1, 4096)})


def ai_batches(tag):
  """B in {1, epb - 1, epb, epb + 1, 2 epb + 1} for the larger of the two kernels' epb: both see a partial last
  workgroup."""
  e = max(AI_CASES[tag]['epb_bwd'], AI_CASES[tag]['epb_fwd'])
  return sorted({b for b in (1, e - 1, e, e + 1, 2 * e + 1) if b > 0})


def ai_scores(g, B, F, H, ds):
  """The fp64 scores sqrt(ds) q . k [B, H, F, F] of a [B F, 4d] block."""
  d = H * ds
  q = g[:, :d].reshape(B, F, H, ds).permute(0, 2, 1, 3)
  k = g[:, d:2 * d].reshape(B, F, H, ds).permute(0, 2, 1, 3)
  return torch.matmul(q, k.transpose(-1, -2)) * float(ds) ** 0.5


@functools.lru_cache(maxsize=None)
def ai_inputs(tag, B):
  """-> dict(g [B F, 4d] = Q | K | V | R, dy [B F, d]: fp64 holding fp32 values).  Q and K carry ds ** -0.5 each, so that
  the scores sqrt(ds) q . k are O(1) like BERT's; a `top` case then scales Q to its largest score."""
  c = AI_CASES[tag]
  F, H, ds = c['F'], c['H'], c['ds']
  d = H * ds
  gen = torch.Generator().manual_seed(AI_SEEDS[tag] + 1000 * B)
  g = torch.randn(B * F, 4 * d, generator=gen, dtype=F64)
  g[:, :2 * d] *= float(ds) ** -0.5
  g = _f32_values(g)
  if 'top' in c:
    g[:, :d] *= c['top'] / float(ai_scores(g, B, F, H, ds).max())
    g = _f32_values(g)
  return dict(g=g, dy=_f32_values(torch.randn(B * F, d, generator=gen, dtype=F64)))


def ai_eval(tag, B, dt, pattern=None):
  """autoint_ref.attention_core at dtype dt -> dict(y, and with the ReLU's pattern [B F, d] given: dq, dk, dv, dr, the
  gradient through that pattern)."""
  c, inp = AI_CASES[tag], ai_inputs(tag, B)
  F, H, ds = c['F'], c['H'], c['ds']
  d = H * ds
  g = inp['g'].to(dt).clone().requires_grad_(True)
  gv = g.view(B, F, 4 * d)
  q, k, v, r = (gv[..., i * d:(i + 1) * d] for i in range(4))
  out = dict(y=autoint_ref.attention_core(q, k, v, r, H, ds).reshape(B * F, d).detach())
  if pattern is not None:
    masked = autoint_ref.attention_core(q, k, v, r, H, ds, mask=pattern.to(dt).view(B, F, d)).reshape(B * F, d)
    dg, = torch.autograd.grad(masked, g, inp['dy'].to(dt))
    out.update(dq=dg[:, :d], dk=dg[:, d:2 * d], dv=dg[:, 2 * d:3 * d], dr=dg[:, 3 * d:])
  return out


def ai_bar(tag, tensor):
  return AI_BARS.get((tag, tensor), (None, FWD_BAR if tensor == 'y' else GRAD_BAR))[1]


def ai_top_gap(tag, B):
  c = AI_CASES[tag]
  s = ai_scores(ai_inputs(tag, B)['g'], B, c['F'], c['H'], c['ds'])
  best = s.topk(2, dim=-1).values
  return float(s.max()), float((best[..., 0] - best[..., 1]).min())


def measure(got, want, floor=1e-30):
  """close's measure: max error over max value."""
  want = want.detach().to('cpu', F64)
  return float((got.detach().to('cpu', F64) - want).abs().max()) / max(float(want.abs().max()), floor)
