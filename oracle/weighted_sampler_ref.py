"""Restatement of the weighted negative draw (negative_sampler), written from the text of include/easyrec_hip.h K1c and
not from the product's composition: what er_neg_sample_weighted and neg_sampler.draw_weighted are checked against.
Python integers and one struct-packed fp32 compare per attempt; nothing is vectorised.

  base = mix64(seed ^ mix64(s)); draw j, attempt a = 0 .. 31:
    r0 = mix64(base ^ mix64((j << 32) | a)); r1 = mix64(r0 + GOLDEN); k = (r0 * n) >> 64; f = (r1 >> 40) * 2^-24
    row = k if f < prob[k] else alias[k] (an alias outside [0, n): k)
    accepted unless table_ids[row] is a batch id
  32 rejections: row = (row + 1) mod n, at most B + 1 times, until table_ids[row] is no batch id."""
import struct

import numpy as np

from oracle.neg_sampler_ref import GOLDEN, M64, extended, mix64  # noqa: F401  (extended: the K1b column rule, unchanged)

ATTEMPTS = 32


def _mix(x):
  return int(mix64(x & M64))


def unpack(alias_tab):
  """uint64 records -> (prob as Python floats holding fp32 values, alias as Python ints)"""
  prob, alias = [], []
  for rec in np.asarray(alias_tab, dtype=np.uint64).tolist():
    prob.append(struct.unpack('<f', struct.pack('<I', rec & 0xFFFFFFFF))[0])
    alias.append(rec >> 32)
  return prob, alias


def implied_distribution(alias_tab):
  """p_i = (prob_i + sum over k with alias_k = i of (1 - prob_k)) / n, in fp64"""
  prob, alias = unpack(alias_tab)
  n = len(prob)
  p = np.array(prob, dtype=np.float64)
  for k in range(n):
    p[alias[k]] += 1.0 - prob[k]
  return p / n


def candidate(base, j, a, prob, alias):
  n = len(prob)
  r0 = _mix(base ^ _mix((j << 32) | a))
  r1 = _mix(r0 + GOLDEN)
  k = (r0 * n) >> 64
  f = (r1 >> 40) * 2.0 ** -24  # (24 bits: the same number in fp32 and fp64; prob[k] holds an fp32 value)
  if f < prob[k]:
    return k
  return alias[k] if alias[k] < n else k


def draw(seed, step, alias_tab, table_ids, batch_ids, N, stats=None):
  """sel [N] int64.  stats (a dict): counts 'rejected' attempts and 'walked' draws."""
  prob, alias = unpack(alias_tab)
  ids = [int(v) for v in np.asarray(table_ids).tolist()]
  n = len(ids)
  excluded = set(int(v) for v in np.asarray(batch_ids).tolist())
  B = len(np.asarray(batch_ids))
  base = _mix((seed & M64) ^ _mix(step))
  sel = []
  for j in range(N):
    row, accepted = 0, False
    for a in range(ATTEMPTS):
      row = candidate(base, j, a, prob, alias)
      if ids[row] not in excluded:
        accepted = True
        break
      if stats is not None:
        stats['rejected'] = stats.get('rejected', 0) + 1
    if not accepted:
      if stats is not None:
        stats['walked'] = stats.get('walked', 0) + 1
      for _ in range(B + 1):
        row = (row + 1) % n
        if ids[row] not in excluded:
          break
    sel.append(row)
  return np.asarray(sel, dtype=np.int64)
