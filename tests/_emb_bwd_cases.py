"""Cases and the float64 reference for the embedding backward: sort -> segmented reduce -> row optimizer
(emb_bwd_tile_kernel, emb_bwd_fix_kernel, finish_run, update_row of easyrec_amd/csrc/er_embedding.hip).
No backend and no library is imported here: tests/test_emb_bwd_pins.py (CPU) shows that the cases hold what they claim
and measures the float32 error of the source-order restatement; tests/test_emb_bwd_edges_gpu.py runs the kernels.

Lane geometry (lane_geom / tile_passes of er_embedding.hip, restated; the GPU test asserts it against the library):
  V = 4 if dim % 4 == 0 else 1;  G = next_pow2(dim / V);  T = tile_entries = (4 if V == 4 else 2) * 256 / G.
A workgroup reduces T consecutive entries of the key-sorted entry list; a run of equal keys that crosses a tile boundary
leaves partial sums (tile_first / tile_last) that the fix kernel combines.  Which branch handles a run is decided by where
it sits relative to the tile boundaries, so the cases PLACE runs there instead of drawing ids at random.

A case is (dim, plan, split, inputs):
  plan    run lengths in units of T, keys assigned in increasing order (key of run i = 2 i + 1: even rows and row 0 are
          never touched), ids = np.repeat(keys, lengths) shuffled by a seeded permutation:
            base           [T-1, 2, T-1, 3T+5, 1, T, pad, T, 1, 2T, 1,1,1,1,1,1,1]   pad = up to the next multiple of T
                           (the 3T+5 run starts ON a boundary - 2T entries precede it - and ends inside its fourth
                           tile; the 2T run starts one past a boundary; the T run after pad is one aligned whole tile)
            tail_aligned   base without its seven singles + (T-4) singles + one run of T+3: N % T == 0 and the last run
                           ends on the last entry
            tail_plus_one  base without its seven singles: N % T == 1
            all_distinct   2T+7 runs of length 1
            with_invalid   base, and on top of it 10 % of all entries with id -1 and 5 % with id rows + 3 (both pruned:
                           kInvalidKey, sorted to the end).  The invalid entries are ADDED, so the valid runs keep the
                           base plan's positions and the invalid keys fill the last tiles.
            all_invalid    2T+7 entries, every id -1 or rows + 3
  split   one          one dense lookup
          three        the same entries over three dense lookups of ONE table (overlapping key ranges: the device-wide
                       chunk sort + merge), the second weighted, gradient columns at a misaligned offset; at dims 1 and 4
                       the first lookup holds 8200 entries (> 8192; missing ids make up the count where the plan is shorter)
          two_tables   two tables in one group (key_base of the second = rows of the first), the long run in the second
          ragged       three tables: sum | weighted mean | weighted sqrtn bags of 0..4 ids, 20 % empty, 7 spare id slots
  inputs  exact   gradients k / 64 (1 <= |k| <= 8), weights in {-2, -1, 1, 2, 3}, tables multiples of 2**-10 in [-1, 1],
                  grad_scale 0.5, lr 0.125 (clip_scale 0.25 in the clipped variant): every float32 partial sum in any
                  order, and the SGD update, are exact (|sum| < 2**24 units of 2**-6: asserted in the builder)
          random  randn * 0.01 gradients, randn weights, m in [0, 0.01), v in [1e-4, 1e-2 + 1e-4), lr 0.05, t 3,
                  grad_scale 0.5

reference(): per-key sums by np.add.at over scale * dout[row] in float64, the optimizer formulas of update_row /
adam_elem in float64 on the hyper record's float32 scalars.  The scale of an entry is w / den with den the float32
source-order sum the lookup kernels define (sum w | sqrt(sum w^2) over the kept ids of the bag, 1 for `sum`), so that a
term carries two float32 roundings in the kernel (the division and the product) and none here.  Pruning follows
oracle/kernel_ref.py lookup_rows / sparse_grads: id < 0 or >= rows, and weight <= 0 under mean / sqrtn.

MEASURED (bottom of the file): max |float32 restatement - float64| / max |float64 - initial| per (case, optimizer,
quantity), as printed by `python tests/test_emb_bwd_pins.py --regen`; the GPU bar is GPU_FACTOR times that.
"""
import functools
import zlib

import numpy as np

F32 = np.float32
U = 2.0**-24
INVALID = 0xFFFFFFFF
OPT_SGD, OPT_ADAM, OPT_LAZY_ADAM, OPT_ADAGRAD = 0, 1, 2, 3
OPT_NAMES = {OPT_SGD: 'SGD', OPT_ADAM: 'ADAM', OPT_LAZY_ADAM: 'LAZY_ADAM', OPT_ADAGRAD: 'ADAGRAD'}
SUM, MEAN, SQRTN = 0, 1, 2
HYPER_FLOATS = 16  # sizeof(er_opt_hyper) / 4 (the GPU test asserts it against the library's record)
(H_LR, H_LR_T, H_B1, H_B2, H_OMB1, H_OMB2, H_EPS, H_GSCALE, H_CLIP) = range(9)

DIMS = (1, 2, 3, 5, 4, 12, 16, 20, 32, 64, 128, 256)
OPT_DIMS = (1, 3, 5, 4, 12, 16, 64, 128)
RAGGED_DIMS = (1, 5, 16, 64)
PLANS = ('base', 'tail_aligned', 'tail_plus_one', 'all_distinct', 'with_invalid')
SPLITS = ('one', 'three', 'two_tables')
WIDE_FIRST = 8200      # entries of the first lookup of the `three` split at dims 1 and 4 (> 8192: the per-lookup sort's limit)
GPU_FACTOR = 8.0       # the kernel sums in Hillis-Steele and cross-tile order, not in source order
BAR_CAP = 1e-3         # a dropped or doubled entry in a run of <= 8 moves the update by >= 10 %


def lane_geom(dim):
  V = 4 if dim % 4 == 0 else 1
  n, G = dim // V, 1
  while G < n:
    G <<= 1
  return V, G


def tile_entries(dim):
  V, G = lane_geom(dim)
  return (4 if V == 4 else 2) * 256 // G


def hyper_row(lr, t=1, gscale=1.0, clip=0.0, b1=0.9, b2=0.999):
  f = F32
  row = np.zeros(HYPER_FLOATS, dtype=np.float32)
  row[H_LR] = f(lr)
  row[H_LR_T] = f(lr) * np.sqrt(f(1) - f(b2)**t) / (f(1) - f(b1)**t)
  row[H_B1], row[H_B2], row[H_OMB1], row[H_OMB2] = f(b1), f(b2), f(1) - f(b1), f(1) - f(b2)
  row[H_EPS], row[H_GSCALE], row[H_CLIP] = f(1e-8), f(gscale), f(clip)
  return row


def hyper_of(inputs, clip=0.0):
  return hyper_row(0.125, 1, 0.5, clip) if inputs == 'exact' else hyper_row(0.05, 3, 0.5, clip)


# ---------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------
def plan_lengths(dim, plan):
  T = tile_entries(dim)
  head = [T - 1, 2, T - 1, 3 * T + 5, 1, T]
  pad = -sum(head) % T
  body = head + [pad, T, 1, 2 * T]
  assert pad > 0 and sum(head) + pad == 7 * T
  if plan in ('base', 'with_invalid'):
    return body + [1] * 7
  if plan == 'tail_aligned':
    return body + [1] * (T - 4) + [T + 3]
  if plan == 'tail_plus_one':
    return body
  if plan == 'all_distinct':
    return [1] * (2 * T + 7)
  raise KeyError(plan)


def _rng(*what):
  return np.random.default_rng(zlib.crc32(repr(what).encode()))


_NEG, _OOR = -1, -2  # markers of the two kinds of invalid entries in a plan's key list


def plan_keys(dim, plan, seed=0):
  """-> (keys int64 in shuffled entry order; _NEG / _OOR mark invalid entries, table rows)."""
  T = tile_entries(dim)
  rng = _rng('plan', dim, plan, seed)
  if plan == 'all_invalid':
    keys = np.where(np.arange(2 * T + 7) % 3 == 0, _OOR, _NEG).astype(np.int64)
    return keys, 10
  lengths = np.asarray(plan_lengths(dim, plan), dtype=np.int64)
  keys = np.repeat(2 * np.arange(len(lengths), dtype=np.int64) + 1, lengths)
  rows = 2 * len(lengths) + 2
  if plan == 'with_invalid':
    total = int(np.ceil(len(keys) / 0.85))
    n_neg, n_oor = int(round(0.10 * total)), int(round(0.05 * total))
    keys = np.concatenate([keys, np.full(n_neg, _NEG, dtype=np.int64), np.full(n_oor, _OOR, dtype=np.int64)])
  return keys[rng.permutation(len(keys))], rows


def _ids_of(keys, key_base, rows):
  ids = keys - key_base
  ids = np.where(keys == _NEG, -1, ids)
  return np.where(keys == _OOR, rows + 3, ids).astype(np.int64)


class Case(object):
  """numpy only.  lookups: dicts with ids, offsets, weights, combiner, rows, key_base, n_rows, max_nnz, out_col."""

  def __init__(self, **kw):
    self.__dict__.update(kw)

  @property
  def name(self):
    return 'd%d-%s-%s-%s' % (self.dim, self.plan, self.split, self.inputs)

  @property
  def num_entries(self):
    return sum(lk['max_nnz'] if lk['offsets'] is not None else lk['n_rows'] for lk in self.lookups)


def _dense_lookup(keys, key_base, rows, weights=None):
  return dict(ids=_ids_of(keys, key_base, rows), offsets=None, weights=weights, combiner=SUM, rows=rows, key_base=key_base,
              n_rows=len(keys), max_nnz=len(keys))


def _ragged_lookup(rng, keys, key_base, rows, combiner, weighted):
  n = len(keys)
  lens = []
  while sum(lens) < n:
    k = int(rng.integers(1, 5))
    lens.append(0 if rng.random() < 0.2 else min(k, n - sum(lens)))
  lens = np.asarray(lens, dtype=np.int64)
  offsets = np.zeros(len(lens) + 1, dtype=np.int32)
  offsets[1:] = np.cumsum(lens)
  cap = n + 7
  ids = np.full(cap, -1, dtype=np.int64)
  ids[:n] = _ids_of(keys, 0, rows)  # (a plan's keys are rows of ONE table; key_base places the table in the group)
  w = None
  if weighted:
    w = np.zeros(cap, dtype=np.float32)
    w[:n] = rng.standard_normal(n).astype(np.float32)  # the non-positive ones are pruned under mean / sqrtn
  return dict(ids=ids, offsets=offsets, weights=w, combiner=combiner, rows=rows, key_base=key_base, n_rows=len(lens),
              max_nnz=cap)


@functools.lru_cache(maxsize=None)
def make_case(dim, plan, split, inputs):
  T = tile_entries(dim)
  rng = _rng('case', dim, plan, split, inputs)
  exact = inputs == 'exact'
  keys, rows = plan_keys(dim, plan)
  if split == 'one':
    lookups, total_rows = [_dense_lookup(keys, 0, rows)], rows
  elif split == 'three':
    n = len(keys)
    if dim in (1, 4):
      if n < WIDE_FIRST + 128:  # missing ids, spread over the whole list, make up the count
        fill = -(-(WIDE_FIRST + 128 - n) // T) * T  # whole tiles of them: N % T stays the plan's
        keys = np.concatenate([keys, np.full(fill, _NEG, dtype=np.int64)])
        keys = keys[rng.permutation(len(keys))]
        n = len(keys)
      cuts = [0, WIDE_FIRST, WIDE_FIRST + (n - WIDE_FIRST) // 2, n]
    else:
      cuts = [0, n // 2 + 1, n // 2 + 1 + n // 3, n]
    lookups = []
    for i in range(3):
      part = keys[cuts[i]:cuts[i + 1]]
      w = None
      if i == 1:
        w = (rng.choice(np.array([-2, -1, 1, 2, 3], dtype=np.float32), size=len(part)) if exact else
             rng.standard_normal(len(part)).astype(np.float32))
      lookups.append(_dense_lookup(part, 0, rows, w))
    total_rows = rows
  elif split == 'two_tables':
    r1 = 7  # the key of run 3 (the run longer than three tiles in the base plans): the first row of the second table
    inv = keys < 0
    first = np.where(inv, np.arange(len(keys)) % 2 == 0, keys < r1)
    lookups = [_dense_lookup(keys[first], 0, r1), _dense_lookup(keys[~first], r1, rows - r1)]
    total_rows = rows
  elif split == 'ragged':
    assert not exact
    lookups = []
    for i, (comb, weighted) in enumerate(((SUM, False), (MEAN, True), (SQRTN, True))):
      k, _ = plan_keys(dim, plan, seed=i)
      lookups.append(_ragged_lookup(rng, k, i * rows, rows, comb, weighted))
    total_rows = 3 * rows
  else:
    raise KeyError(split)
  pad = 3 if split == 'three' else 0
  for i, lk in enumerate(lookups):
    lk['out_col'] = pad + i * dim
  out_rows = max(lk['n_rows'] for lk in lookups)
  width = pad + len(lookups) * dim
  if exact:
    # (no zeros: every entry then moves its row's sum, so a dropped or misattributed entry always shows)
    dout = (rng.choice(np.r_[-8:0, 1:9], size=(out_rows, width)) / 64.0).astype(np.float32)
    table = (rng.integers(-1024, 1025, size=(total_rows, dim)) / 1024.0).astype(np.float32)
    longest = max(plan_lengths(dim, plan)) if plan != 'all_invalid' else 0
    assert longest < 6 * 1024 and longest * 8 * 3 < 2**24  # |sum| in units of 2**-6: every partial sum is exact
  else:
    dout = (rng.standard_normal((out_rows, width)) * 0.01).astype(np.float32)
    table = (rng.standard_normal((total_rows, dim)) * 0.1).astype(np.float32)
  m = (rng.random((total_rows, dim)) * 0.01).astype(np.float32)
  v = (rng.random((total_rows, dim)) * 0.01 + 1e-4).astype(np.float32)
  return Case(dim=dim, plan=plan, split=split, inputs=inputs, T=T, total_rows=total_rows, lookups=lookups, dout=dout,
              table=table, m=m, v=v)


# ---------------------------------------------------------------------------------------------
# entries, sorted keys and the positions a plan reaches
# ---------------------------------------------------------------------------------------------
def entries(case):
  """Valid entries in entry order -> (keys int64 [n], scale float64 [n], dout rows float64 [n, dim], slot int64 [n]);
  slot = index of the entry in the group's entry list (the sort's payload)."""
  ks, ss, gs, slots = [], [], [], []
  base = 0
  for lk in case.lookups:
    ids, w, rows = lk['ids'], lk['weights'], lk['rows']
    if lk['offsets'] is None:
      n = lk['n_rows']
      row = np.arange(n)
      pos = np.zeros(n, dtype=np.int64)
      cap = n
    else:
      lens = np.diff(lk['offsets']).astype(np.int64)
      n = int(lk['offsets'][-1])
      row = np.repeat(np.arange(lk['n_rows']), lens)
      pos = np.arange(n) - np.repeat(lk['offsets'][:-1].astype(np.int64), lens)
      cap = lk['max_nnz']
    ids = ids[:n]
    ok = (ids >= 0) & (ids < rows)
    wk = np.ones(n, dtype=np.float32) if w is None else w[:n]
    if w is not None and lk['combiner'] != SUM:
      ok = ok & (wk > 0)
    den = np.ones(lk['n_rows'], dtype=np.float32)
    if lk['combiner'] != SUM:
      wsum = np.zeros(lk['n_rows'], dtype=np.float32)
      w2sum = np.zeros(lk['n_rows'], dtype=np.float32)
      for j in range(int(pos.max()) + 1 if n else 0):  # source order inside every bag, float32 like the kernels
        sel = ok & (pos == j)
        wsum[row[sel]] = wsum[row[sel]] + wk[sel]
        w2sum[row[sel]] = w2sum[row[sel]] + wk[sel] * wk[sel]
      den = np.where(wsum != 0, wsum if lk['combiner'] == MEAN else np.sqrt(w2sum, dtype=np.float32), F32(1))
    scale = wk.astype(np.float64) / den[row].astype(np.float64)
    g = case.dout[row, lk['out_col']:lk['out_col'] + case.dim].astype(np.float64)
    ks.append((lk['key_base'] + ids)[ok])
    ss.append(scale[ok])
    gs.append(g[ok])
    slots.append(base + np.arange(n)[ok])
    base += cap
  return np.concatenate(ks), np.concatenate(ss), np.concatenate(gs), np.concatenate(slots)


def sorted_keys(case):
  """The group's key list as the tile kernel sees it: valid keys ascending, then kInvalidKey up to num_entries."""
  k = np.sort(entries(case)[0])
  return np.concatenate([k, np.full(case.num_entries - len(k), INVALID, dtype=np.int64)])


def positions(skeys, T):
  """Which branches of tile_body / fix_body a sorted key list reaches, recomputed the way the kernels decide."""
  n = len(skeys)
  n_tiles = -(-n // T)
  key = lambda p: int(skeys[p]) if 0 <= p < n else INVALID  # noqa: E731
  out = dict(n=n, n_tiles=n_tiles, n_mod_T=n % T, from_prev=[], to_next=[], both_different=[], whole_tile_crossed=[],
             fix_owners=[], fix_whole_tiles=[], fix_ends_on_tile_end=0, fix_ends_in_last_tile_at_n=0,
             ends_on_tile_end_then_other_key=0, aligned_whole_tile_runs=0, minimal_crossings=0,
             last_run_ends_on_last_entry=bool(n and key(n - 1) != INVALID),
             invalid_in_last_tile=int(np.sum(np.asarray(skeys[(n_tiles - 1) * T:]) == INVALID)) if n else 0,
             invalid=int(np.sum(np.asarray(skeys) == INVALID)), longest_run=0)
  valid = np.asarray(skeys)[np.asarray(skeys) != INVALID]
  if len(valid):
    starts = np.flatnonzero(np.concatenate([[True], valid[1:] != valid[:-1]]))
    lens = np.diff(np.concatenate([starts, [len(valid)]]))
    out['longest_run'] = int(lens.max())
    out['aligned_whole_tile_runs'] = int(np.sum((starts % T == 0) & (lens == T)))
    out['minimal_crossings'] = int(np.sum((lens == 2) & (starts % T == T - 1)))
  for b in range(n_tiles):
    t0, t1 = b * T, (b + 1) * T
    fp = b > 0 and key(t0) != INVALID and key(t0 - 1) == key(t0)
    tn = t1 < n and key(t1 - 1) != INVALID and key(t1 - 1) == key(t1)
    if fp:
      out['from_prev'].append(b)
    if tn:
      out['to_next'].append(b)
    if fp and tn:
      (out['whole_tile_crossed'] if key(t0) == key(t1 - 1) else out['both_different']).append(b)
    if t1 < n and key(t1 - 1) != INVALID and key(t1) != INVALID and key(t1 - 1) != key(t1):
      out['ends_on_tile_end_then_other_key'] += 1
    if tn and not (b > 0 and key(t0 - 1) == key(t1 - 1)):  # fix_body's owner test
      out['fix_owners'].append(b)
      whole, m = 0, b + 1
      while True:
        mn = (m + 1) * T
        if mn < n and key(mn - 1) == key(t1) and key(mn) == key(t1):
          whole += 1
          m += 1
          continue
        last = min(mn, n) - 1
        if key(last) == key(t1):
          if mn >= n:
            out['fix_ends_in_last_tile_at_n'] += 1
          if last == mn - 1:
            out['fix_ends_on_tile_end'] += 1
        break
      out['fix_whole_tiles'].append(whole)
  return out


# ---------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------
def row_sums(case, broken=None):
  """-> (sums float64 [total_rows, dim], touched keys ascending, abs sums, counts).  broken: a deliberately wrong
  evaluation ('drop_last': without the last entry of the longest run; 'misattribute': the entry at sorted position T - 1
  - the first past a tile's last but one - counted for the key before it) that the checks must tell from the right one."""
  keys, scale, g, _ = entries(case)
  terms = scale[:, None] * g
  if broken == 'drop_last':
    uk, cnt = np.unique(keys, return_counts=True)
    last = np.flatnonzero(keys == uk[np.argmax(cnt)])[-1]
    keep = np.ones(len(keys), dtype=bool)
    keep[last] = False
    keys, terms = keys[keep], terms[keep]
  elif broken == 'misattribute':
    order = np.argsort(keys, kind='stable')
    keys = keys.copy()
    assert keys[order[case.T - 1]] != keys[order[case.T - 2]]
    keys[order[case.T - 1]] = keys[order[case.T - 2]]
  else:
    assert broken is None
  sums = np.zeros((case.total_rows, case.dim), dtype=np.float64)
  asum = np.zeros((case.total_rows, case.dim), dtype=np.float64)
  cnt = np.zeros(case.total_rows, dtype=np.int64)
  np.add.at(sums, keys, terms)
  np.add.at(asum, keys, np.abs(terms))
  np.add.at(cnt, keys, 1)
  return sums, np.unique(keys), asum, cnt


def reference(case, opt, hyper, steps=1, broken=None):
  """-> dict(var, m, v float64 [total_rows, dim], sums, touched) after `steps` updates with the same gradients."""
  h = np.asarray(hyper, dtype=np.float32).astype(np.float64)
  sums, touched, _, _ = row_sums(case, broken)
  g = sums * h[H_GSCALE]
  if h[H_CLIP] != 0:
    g = g * h[H_CLIP]
  var, m, v = case.table.astype(np.float64), case.m.astype(np.float64), case.v.astype(np.float64)
  rows = np.arange(case.total_rows) if opt == OPT_ADAM else touched  # TF's Adam: untouched rows take the g = 0 step
  for _ in range(steps):
    if opt in (OPT_ADAM, OPT_LAZY_ADAM):
      m[rows] = m[rows] * h[H_B1] + g[rows] * h[H_OMB1]
      v[rows] = v[rows] * h[H_B2] + (g[rows] * g[rows]) * h[H_OMB2]
      var[rows] = var[rows] - (h[H_LR_T] * m[rows]) / (np.sqrt(v[rows]) + h[H_EPS])
    elif opt == OPT_ADAGRAD:
      v[rows] = v[rows] + g[rows] * g[rows]
      var[rows] = var[rows] - (g[rows] * h[H_LR]) / np.sqrt(v[rows])
    else:
      assert opt == OPT_SGD
      var[rows] = var[rows] - h[H_LR] * g[rows]
  return dict(var=var, m=m, v=v, sums=sums, touched=touched)


def rel_err(got, want, initial):
  """max |got - want| / max |want - initial| (0 where nothing moved and nothing differs)."""
  num = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)))
  den = float(np.max(np.abs(want - np.asarray(initial, dtype=np.float64))))
  return 0.0 if num == 0.0 else (num / den if den > 0 else float('inf'))


def quantities(opt):
  return {OPT_SGD: ('var',), OPT_ADAGRAD: ('var', 'v')}.get(opt, ('var', 'm', 'v'))


def measured_key(case, opt, what):
  return '%s/%s/%s' % (case.name, OPT_NAMES[opt], what)


def gpu_bar(case, opt, what):
  bar = GPU_FACTOR * MEASURED[measured_key(case, opt, what)]
  assert bar <= BAR_CAP, (measured_key(case, opt, what), bar)
  return bar


# ---------------------------------------------------------------------------------------------
# grids
# ---------------------------------------------------------------------------------------------
def exact_grid():
  return [(d, p, s) for d in DIMS for p in PLANS for s in SPLITS]


def random_grid():
  """(case args, optimizers) whose float32 error MEASURED records."""
  out = [((d, p, 'three', 'random'), (OPT_ADAM, OPT_LAZY_ADAM, OPT_ADAGRAD)) for d in OPT_DIMS for p in ('base', 'with_invalid')]
  out += [((d, 'base', 'ragged', 'random'), (OPT_ADAM,)) for d in RAGGED_DIMS]
  return out


MEASURED = {
    'd1-base-three-random/ADAGRAD/v': 4.858e-07,
    'd1-base-three-random/ADAGRAD/var': 5.470e-07,
    'd1-base-three-random/ADAM/m': 4.481e-07,
    'd1-base-three-random/ADAM/v': 3.376e-06,
    'd1-base-three-random/ADAM/var': 5.983e-07,
    'd1-base-three-random/LAZY_ADAM/m': 4.481e-07,
    'd1-base-three-random/LAZY_ADAM/v': 3.376e-06,
    'd1-base-three-random/LAZY_ADAM/var': 5.983e-07,
    'd1-with_invalid-three-random/ADAGRAD/v': 3.507e-07,
    'd1-with_invalid-three-random/ADAGRAD/var': 6.161e-07,
    'd1-with_invalid-three-random/ADAM/m': 3.282e-07,
    'd1-with_invalid-three-random/ADAM/v': 1.046e-05,
    'd1-with_invalid-three-random/ADAM/var': 7.724e-07,
    'd1-with_invalid-three-random/LAZY_ADAM/m': 3.282e-07,
    'd1-with_invalid-three-random/LAZY_ADAM/v': 1.046e-05,
    'd1-with_invalid-three-random/LAZY_ADAM/var': 7.724e-07,
    'd3-base-three-random/ADAGRAD/v': 2.377e-07,
    'd3-base-three-random/ADAGRAD/var': 2.911e-07,
    'd3-base-three-random/ADAM/m': 1.495e-07,
    'd3-base-three-random/ADAM/v': 1.400e-05,
    'd3-base-three-random/ADAM/var': 1.682e-06,
    'd3-base-three-random/LAZY_ADAM/m': 1.495e-07,
    'd3-base-three-random/LAZY_ADAM/v': 1.258e-05,
    'd3-base-three-random/LAZY_ADAM/var': 1.682e-06,
    'd3-with_invalid-three-random/ADAGRAD/v': 2.770e-07,
    'd3-with_invalid-three-random/ADAGRAD/var': 8.252e-07,
    'd3-with_invalid-three-random/ADAM/m': 4.638e-07,
    'd3-with_invalid-three-random/ADAM/v': 4.673e-05,
    'd3-with_invalid-three-random/ADAM/var': 1.250e-06,
    'd3-with_invalid-three-random/LAZY_ADAM/m': 4.638e-07,
    'd3-with_invalid-three-random/LAZY_ADAM/v': 4.673e-05,
    'd3-with_invalid-three-random/LAZY_ADAM/var': 9.261e-07,
    'd5-base-three-random/ADAGRAD/v': 3.843e-07,
    'd5-base-three-random/ADAGRAD/var': 4.593e-07,
    'd5-base-three-random/ADAM/m': 2.176e-07,
    'd5-base-three-random/ADAM/v': 7.217e-05,
    'd5-base-three-random/ADAM/var': 1.384e-06,
    'd5-base-three-random/LAZY_ADAM/m': 2.176e-07,
    'd5-base-three-random/LAZY_ADAM/v': 7.433e-05,
    'd5-base-three-random/LAZY_ADAM/var': 1.007e-06,
    'd5-with_invalid-three-random/ADAGRAD/v': 3.420e-07,
    'd5-with_invalid-three-random/ADAGRAD/var': 3.768e-07,
    'd5-with_invalid-three-random/ADAM/m': 1.731e-07,
    'd5-with_invalid-three-random/ADAM/v': 1.611e-05,
    'd5-with_invalid-three-random/ADAM/var': 7.005e-07,
    'd5-with_invalid-three-random/LAZY_ADAM/m': 1.731e-07,
    'd5-with_invalid-three-random/LAZY_ADAM/v': 1.611e-05,
    'd5-with_invalid-three-random/LAZY_ADAM/var': 7.005e-07,
    'd4-base-three-random/ADAGRAD/v': 9.982e-07,
    'd4-base-three-random/ADAGRAD/var': 3.901e-06,
    'd4-base-three-random/ADAM/m': 9.369e-07,
    'd4-base-three-random/ADAM/v': 2.706e-06,
    'd4-base-three-random/ADAM/var': 1.102e-06,
    'd4-base-three-random/LAZY_ADAM/m': 9.369e-07,
    'd4-base-three-random/LAZY_ADAM/v': 2.706e-06,
    'd4-base-three-random/LAZY_ADAM/var': 1.102e-06,
    'd4-with_invalid-three-random/ADAGRAD/v': 6.838e-07,
    'd4-with_invalid-three-random/ADAGRAD/var': 1.765e-06,
    'd4-with_invalid-three-random/ADAM/m': 4.872e-07,
    'd4-with_invalid-three-random/ADAM/v': 3.871e-06,
    'd4-with_invalid-three-random/ADAM/var': 6.241e-07,
    'd4-with_invalid-three-random/LAZY_ADAM/m': 4.872e-07,
    'd4-with_invalid-three-random/LAZY_ADAM/v': 3.871e-06,
    'd4-with_invalid-three-random/LAZY_ADAM/var': 5.727e-07,
    'd12-base-three-random/ADAGRAD/v': 5.993e-07,
    'd12-base-three-random/ADAGRAD/var': 6.402e-07,
    'd12-base-three-random/ADAM/m': 3.976e-07,
    'd12-base-three-random/ADAM/v': 9.881e-06,
    'd12-base-three-random/ADAM/var': 1.348e-06,
    'd12-base-three-random/LAZY_ADAM/m': 3.976e-07,
    'd12-base-three-random/LAZY_ADAM/v': 9.881e-06,
    'd12-base-three-random/LAZY_ADAM/var': 1.348e-06,
    'd12-with_invalid-three-random/ADAGRAD/v': 1.499e-06,
    'd12-with_invalid-three-random/ADAGRAD/var': 6.377e-07,
    'd12-with_invalid-three-random/ADAM/m': 7.857e-07,
    'd12-with_invalid-three-random/ADAM/v': 9.051e-06,
    'd12-with_invalid-three-random/ADAM/var': 7.366e-07,
    'd12-with_invalid-three-random/LAZY_ADAM/m': 7.857e-07,
    'd12-with_invalid-three-random/LAZY_ADAM/v': 9.051e-06,
    'd12-with_invalid-three-random/LAZY_ADAM/var': 5.407e-07,
    'd16-base-three-random/ADAGRAD/v': 1.921e-06,
    'd16-base-three-random/ADAGRAD/var': 5.393e-07,
    'd16-base-three-random/ADAM/m': 9.840e-07,
    'd16-base-three-random/ADAM/v': 5.816e-06,
    'd16-base-three-random/ADAM/var': 4.060e-07,
    'd16-base-three-random/LAZY_ADAM/m': 9.840e-07,
    'd16-base-three-random/LAZY_ADAM/v': 5.816e-06,
    'd16-base-three-random/LAZY_ADAM/var': 4.054e-07,
    'd16-with_invalid-three-random/ADAGRAD/v': 1.203e-06,
    'd16-with_invalid-three-random/ADAGRAD/var': 6.854e-07,
    'd16-with_invalid-three-random/ADAM/m': 6.712e-07,
    'd16-with_invalid-three-random/ADAM/v': 1.022e-05,
    'd16-with_invalid-three-random/ADAM/var': 5.658e-07,
    'd16-with_invalid-three-random/LAZY_ADAM/m': 6.712e-07,
    'd16-with_invalid-three-random/LAZY_ADAM/v': 1.022e-05,
    'd16-with_invalid-three-random/LAZY_ADAM/var': 2.573e-07,
    'd64-base-three-random/ADAGRAD/v': 6.594e-07,
    'd64-base-three-random/ADAGRAD/var': 8.459e-07,
    'd64-base-three-random/ADAM/m': 4.579e-07,
    'd64-base-three-random/ADAM/v': 2.833e-05,
    'd64-base-three-random/ADAM/var': 7.516e-07,
    'd64-base-three-random/LAZY_ADAM/m': 4.579e-07,
    'd64-base-three-random/LAZY_ADAM/v': 2.833e-05,
    'd64-base-three-random/LAZY_ADAM/var': 7.516e-07,
    'd64-with_invalid-three-random/ADAGRAD/v': 7.714e-07,
    'd64-with_invalid-three-random/ADAGRAD/var': 5.630e-07,
    'd64-with_invalid-three-random/ADAM/m': 4.847e-07,
    'd64-with_invalid-three-random/ADAM/v': 3.000e-05,
    'd64-with_invalid-three-random/ADAM/var': 1.122e-06,
    'd64-with_invalid-three-random/LAZY_ADAM/m': 4.847e-07,
    'd64-with_invalid-three-random/LAZY_ADAM/v': 3.000e-05,
    'd64-with_invalid-three-random/LAZY_ADAM/var': 1.090e-06,
    'd128-base-three-random/ADAGRAD/v': 3.923e-07,
    'd128-base-three-random/ADAGRAD/var': 4.383e-07,
    'd128-base-three-random/ADAM/m': 2.541e-07,
    'd128-base-three-random/ADAM/v': 7.176e-05,
    'd128-base-three-random/ADAM/var': 7.921e-07,
    'd128-base-three-random/LAZY_ADAM/m': 2.541e-07,
    'd128-base-three-random/LAZY_ADAM/v': 7.176e-05,
    'd128-base-three-random/LAZY_ADAM/var': 7.561e-07,
    'd128-with_invalid-three-random/ADAGRAD/v': 3.576e-07,
    'd128-with_invalid-three-random/ADAGRAD/var': 3.588e-07,
    'd128-with_invalid-three-random/ADAM/m': 2.636e-07,
    'd128-with_invalid-three-random/ADAM/v': 3.491e-05,
    'd128-with_invalid-three-random/ADAM/var': 9.018e-07,
    'd128-with_invalid-three-random/LAZY_ADAM/m': 2.636e-07,
    'd128-with_invalid-three-random/LAZY_ADAM/v': 3.491e-05,
    'd128-with_invalid-three-random/LAZY_ADAM/var': 8.626e-07,
    'd1-base-ragged-random/ADAM/m': 9.426e-07,
    'd1-base-ragged-random/ADAM/v': 2.887e-05,
    'd1-base-ragged-random/ADAM/var': 1.167e-06,
    'd5-base-ragged-random/ADAM/m': 2.548e-07,
    'd5-base-ragged-random/ADAM/v': 3.669e-05,
    'd5-base-ragged-random/ADAM/var': 1.703e-06,
    'd16-base-ragged-random/ADAM/m': 1.352e-06,
    'd16-base-ragged-random/ADAM/v': 4.621e-06,
    'd16-base-ragged-random/ADAM/var': 7.715e-07,
    'd64-base-ragged-random/ADAM/m': 4.240e-07,
    'd64-base-ragged-random/ADAM/v': 3.106e-05,
    'd64-base-ragged-random/ADAM/var': 1.185e-06,
}
