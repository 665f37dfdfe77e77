"""Cases, the float64 reference, a float32 restatement and derived error bounds for the closed-form replay of Adam's
decay-only steps (easyrec_amd/csrc/er_decay.h, replay_closed of er_embedding.hip, the per-step table the step prologue
of er_dense.hip appends).  No backend and no library is imported here: tests/test_decay_pins.py (CPU) holds the
restatement to the bounds, shows that the reference is right and that seeded faults are noticed;
tests/test_decay_replay_gpu.py runs the kernels against the same reference and bounds.

Reference.  reference(): the recurrence itself, step by step in float64 from the float32 inputs (var0, m0, v0, the lr_t
history, beta1 / beta2 / eps as the float32 values the hyper record carries):
    for s = s_begin .. s_end-1:   m *= b1;  v *= b2;  var -= lr_t(s) * m / (sqrt(v) + eps)
with s_begin = last_step + 1 per row.  No hand-derived formula enters it.  adam_step() adds one float64 Adam step with a
gradient through _emb_bwd_cases.reference (the row update behind the lazy lookup).

Restatement.  Tables / restate(): er_decay_tables_create's coefficients in double, T_n summed in double and rounded to
float32, the choice k <= K ? A[k-1] : C[s_begin], p1 / p2 through double exp, the Horner chain in float32 - what
replay_closed computes, in numpy.  It is what the CPU pins hold to the bounds and the only place where faults are
seeded (FAULTS).  decay_terms / remainder / supported restate er_decay_tables_supported.

Bounds, per element, U = 2**-24 (the conventions of tests/_interaction_cases.py: an elementwise float32 operation is
held to faithful rounding, 2 U; a bound of 0 demands bit equality).  With a = sqrt(v0), d = a + eps, z = a / d,
q = sqrt(b2), w_s = 1 - q^s, x_s = z w_s, c_s = lr_t(t0+s) |m0| b1^s / d and u_s = c_s / (1 - x_s), the size of step s's
update (a q^s + eps = d (1 - x_s)):
  var  (closed form)  =  sum_{s > K} u_s                            the dropped tail, rows idle for k > K steps
                       + sum_{s <= min(k,K)} c_s x_s^N / (1 - x_s)   the series 1 / (1 - x) cut after N = kDecayN powers
                       + OPS_CLOSED * 2 U * sum_s u_s               the operations between the inputs and the update:
                            T_n rounded to float32 (1), the Horner chain's deepest monomial (5 products, 5 sums),
                            m * poly and the division by d (2), sqrt and the sum that make d (2): 15.  Every monomial
                            (m0 / d) z^n T_n has the sign of m0, so sum_s u_s is their absolute sum.
                       + Z_OPS * 2 U * sum_{s <= min(k,K)} c_s x_s / (1 - x_s)^2
                            z carries three roundings (sqrt, the sum, the division); z d/dz of the polynomial is
                            sum_n n z^n T_n, below sum_s lr_t b1^s x_s / (1 - x_s)^2
                       + 2 U |var'|                                 the final subtraction (0 where the update is 0:
                                                                    var - 0 is exact)
                       + 2**-149 (1 + 1 / d) where m0 != 0          m * poly may round to a subnormal before / d
       The two sums over s and sum_s u_s are accumulated by reference() in float64 while it steps; none is a constant.
  m, v (closed form)  =  M_OPS * 2 U * |m'|: p = float(exp(double)) and the product, counted as three operations,
                       + FLT_MIN * max(1, |m0|) where b^k or the result is below FLT_MIN (subnormal, or flushed: for
                         k near 1500 beta1^k is below the smallest float32 and the closed form returns 0).
  step by step (the exact replay and the streaming sweep): step s reads m and v after s products (2 U each, v's halved by
       the square root) and takes four operations of its own (lr_t * m, sqrt, the sum, the division), and each of the k
       subtractions rounds var:   var = sum_s (1.5 s + 4) 2 U u_s + sum_s 2 U |var_s|;   m, v = k * 2 U * |m'| (+ the
       same floor: m settles on a subnormal fixed point of fl(m * b1)).  The absorbed regime of the exact replay leaves
       out updates below a quarter ulp of var - less than the rounding of that step's subtraction, which is counted.
  Elements with m0 = v0 = 0 in a lane whose other elements are live are evaluated and must come out unchanged; rows
  with nothing pending, lanes with m0 = v0 = 0 throughout and rows a launch does not list keep every bit (bound 0).

Cases.  state(): ROWS rows; row r idles for k = idle_lengths(K)[r % n] steps before s_end (0, 1, 2, the 64-lane stride
of decay_sum_wave, the A / C switch at K, K + 64, 700: beta1^k subnormal, 1500: several K and beta1^k == 0 at 0.9,
'all': last_step = -1 with live state, a restored table).  Column c of variant j = r // n takes class (c + j) % 6:
sqrt(v) far above eps | near eps | far below eps | v = 0 with m != 0 | m = v = 0 | far above again; variant 9 is a
row of zeros (not live: untouched).  var0 = 0 where (j + r + c) % 3 == 0: there var' = -update and the update's relative
error shows at the level of U.  lr_history(): a halving staircase under a 256-step warm-up, Adam's bias correction
and a seeded factor in [0.6, 1.4] per step - an index off by one moves T_n by tens of percent.
PAIRS: 0.9 / 0.999 (K = 192); 0.9 / 0.996, the accepted edge of beta2 (remainder 2.8e-8 of the 3e-8 allowed; one float32
ulp of beta2 moves it by 5e-5 of itself); 0.96 / 0.999 (K = 512 = kDecayKMax); REFUSED = 0.9 / 0.99.

MEASURED ON CPU (python tests/test_decay_pins.py; worst error / bound of the float32 restatement over every case of
pins_grid(), the pins test asserts <= 0.5):  var 0.498, m 0.285, v 0.275 (closed form; var approaches 0.5 by
construction - the final subtraction rounds to nearest, U |var'|, and is allowed 2 U |var'|);  var 0.490, m 0.477,
v 0.489 (fp32 step by step, within the step-by-step bound);  var 0.473, m 0.282, v 0.306 with one Adam step behind the
replay.  Worst deviation of the closed form's update from the float64 recurrence where var0 = 0, in U: usual 3.8,
edge 8.0, long 3.8.  Seeded faults, worst error / bound: index and row faults 8e3 .. 7e5, K cut by 64: 21 (0.9 / 0.999),
22 (edge), 0.44 (0.96 / 0.999: beta1^448 is 1e-8), the n = 4 coefficient zeroed on the edge betas: 6.9.  Reported, not
asserted: the n = 5 coefficient zeroed reaches 0.92 on the edge betas against 0.46 for the right evaluation, and
changes nothing at 0.9 / 0.999.
"""
import functools
import math
import zlib

import numpy as np

from tests import _emb_bwd_cases as ec

F32 = np.float32
U = 2.0**-24
FLT_MIN = 2.0**-126
DENORM_MIN = 2.0**-149
N_POW = 6        # kDecayN
K_MAX = 512      # kDecayKMax
OPS_CLOSED = 15
Z_OPS = 3
M_OPS = 3
EPS = F32(1e-8)
S_TOTAL = 1700   # steps of history every case is built on (the step counter after the last prologue)
ROWS = 130
PAIRS = {'usual': (0.9, 0.999), 'edge': (0.9, 0.996), 'long': (0.96, 0.999)}
EXPECTED_K = {'usual': 192, 'edge': 192, 'long': 512}
REFUSED = (0.9, 0.99)
DIMS = (1, 3, 4, 16, 64, 256)
WIDE_DIM, WIDE_ROWS = 512, 39   # a row that spans wavefronts: single catch-up and full flush only
FAULTS = ('hist_shift', 'A_row_plus', 'A_row_minus', 'C_plus', 'C_minus', 'switch_past', 'K_cut', 'p2_ln_b1',
          'eps_dropped', 'coef4_zero')


def _rng(*what):
  return np.random.default_rng(zlib.crc32(repr(what).encode()))


def betas(pair):
  b1, b2 = REFUSED if pair == 'refused' else PAIRS[pair]
  return F32(b1), F32(b2)


# ---------------------------------------------------------------------------------------------
# er_decay_tables_supported, restated
# ---------------------------------------------------------------------------------------------
def decay_terms(beta1):
  """smallest multiple of 64 with beta1^K <= 2e-9"""
  beta1 = float(beta1)
  if not (0.0 < beta1 < 1.0):
    return 0
  k = math.ceil(math.log(2e-9) / math.log(beta1))
  K = (int(k) + 63) // 64 * 64
  return max(K, 64)


def remainder(beta1, beta2, K):
  """sum_s beta1^s w_s^N / (1 - w_s) / sum_s beta1^s, w_s = 1 - sqrt(beta2)^s"""
  q, b1 = math.sqrt(float(beta2)), float(beta1)
  num = den = 0.0
  for s in range(1, K + 1):
    w, p = -math.expm1(s * math.log(q)), b1**s
    num += p * w**N_POW / (1.0 - w)
    den += p
  return num / den


def supported(beta1, beta2):
  """K of the closed form for the float32 betas, or 0 (the exact replay is kept)."""
  beta1, beta2 = F32(beta1), F32(beta2)
  K = decay_terms(beta1)
  if K <= 0 or K > K_MAX or not (0.0 < float(beta2) < 1.0):
    return 0
  return K if remainder(beta1, beta2, K) <= 3e-8 else 0


# ---------------------------------------------------------------------------------------------
# history, hyper records, states
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lr_history(pair, n=S_TOTAL + 4):
  b1, b2 = (float(b) for b in betas(pair))
  rng = _rng('lr', pair)
  s = np.arange(n)
  lr = 1e-2 * 0.5**(s // 400) * np.minimum(1.0, (s + 1) / 256.0) * rng.uniform(0.6, 1.4, n)
  t = s + 1.0
  out = (lr * np.sqrt(1.0 - b2**t) / (1.0 - b1**t)).astype(np.float32)
  out.setflags(write=False)
  return out


def hyper_rows(pair, n=S_TOTAL + 4):
  """[n, HYPER_FLOATS] float32: the hyper table whose row s is step s's record (lr_t = lr_history(pair)[s])."""
  b1, b2 = betas(pair)
  rows = np.zeros((n, ec.HYPER_FLOATS), dtype=np.float32)
  rows[:, ec.H_LR] = F32(1e-2)
  rows[:, ec.H_LR_T] = lr_history(pair, n)
  rows[:, ec.H_B1], rows[:, ec.H_B2] = b1, b2
  rows[:, ec.H_OMB1], rows[:, ec.H_OMB2] = F32(1) - b1, F32(1) - b2
  rows[:, ec.H_EPS], rows[:, ec.H_GSCALE] = EPS, F32(1)
  return rows


def idle_lengths(K):
  return [0, 1, 2, 63, 64, 65, K - 1, K, K + 1, K + 64, 700, 1500, 'all']


class State(object):
  def __init__(self, **kw):
    self.__dict__.update(kw)


def last_step_of(ks, s_end):
  """last_step per row such that k decay-only steps are pending before s_end ('all': -1, a restored table)."""
  return np.asarray([-1 if k == 'all' else s_end - 1 - k for k in ks], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def state(pair, dim, s_end, rows=ROWS, ks=None, seed=0):
  """-> State(var, m, v float32 [rows, dim], last int32 [rows], k int64 [rows]); read-only arrays."""
  K = EXPECTED_K.get(pair, 192)  # ('refused': the same idle lengths as 0.9 / 0.999, replayed step by step)
  if ks is None:  # (early training: a flush at s_end <= 3 has rows at every last_step there is)
    ks = tuple(idle_lengths(K)) if s_end > 1564 else tuple(range(s_end)) + ('all',)
  n = len(ks)
  rng = _rng('state', pair, dim, rows, ks, seed)
  r, c = np.arange(rows)[:, None], np.arange(dim)[None, :]
  variant = r // n
  cls = (c + variant) % 6
  g = np.choose(cls, [1e-2, 3e-7, 1e-10, 0.0, 0.0, 1e-2])
  m = 0.1 * g * rng.standard_normal((rows, dim))
  m = np.where(cls == 3, 1e-9 * rng.standard_normal((rows, dim)), m)
  v = 1e-3 * g * g * (0.5 + rng.random((rows, dim)))
  var = 0.05 * rng.standard_normal((rows, dim))
  var = np.where((variant + r + c) % 3 == 0, 0.0, var)
  dead = (variant % 10 == 9) & np.ones((1, dim), dtype=bool)
  m, v = np.where(dead, 0.0, m), np.where(dead, 0.0, v)
  last = last_step_of([ks[i % n] for i in range(rows)], s_end)
  assert last.min() >= -1
  out = State(pair=pair, dim=dim, s_end=s_end, var=var.astype(np.float32), m=m.astype(np.float32),
              v=v.astype(np.float32), last=last, k=np.maximum(s_end - 1 - last.astype(np.int64), 0), cls=cls + 0 * r)
  for a in (out.var, out.m, out.v, out.last, out.k):
    a.setflags(write=False)
  return out


def live_lanes(m, v, dim):
  """[rows, dim] bool: the element's lane (V consecutive columns, lane_geom of er_embedding.hip) holds a nonzero m or v."""
  V, _ = ec.lane_geom(dim)
  nz = (m != 0) | (v != 0)
  rows = nz.shape[0]
  pad = -dim % V
  nzp = np.concatenate([nz, np.zeros((rows, pad), dtype=bool)], axis=1).reshape(rows, -1, V)
  return np.repeat(nzp.any(axis=2), V, axis=1)[:, :dim]


# ---------------------------------------------------------------------------------------------
# float64 reference: the recurrence, and the bounds' ingredients accumulated while it steps
# ---------------------------------------------------------------------------------------------
def reference(var0, m0, v0, last, s_end, hist, beta1, beta2, eps=EPS, K=None, listed=None):
  """-> dict: var, m, v (float64), k [rows], and per element upd (sum_s u_s), tail, rem, zsens, step_var (the step by
  step bound of var).  listed: bool [rows] - the rows the launch handles (the others keep their state)."""
  b1, b2, eps = float(F32(beta1)), float(F32(beta2)), float(F32(eps))
  var, m, v = (np.array(a, dtype=np.float64) for a in (var0, m0, v0))
  h = np.asarray(hist, dtype=np.float32).astype(np.float64)
  s_begin = np.asarray(last, dtype=np.int64) + 1
  if listed is not None:
    s_begin = np.where(listed, s_begin, s_end)
  k = np.maximum(s_end - s_begin, 0)
  K = (1 << 30) if K is None else K
  am0 = np.abs(m)
  a0 = np.sqrt(v)
  d0 = a0 + eps
  z0 = a0 / d0
  q = math.sqrt(b2)
  upd, tail, rem, zsens, step_var = (np.zeros_like(var) for _ in range(5))
  order = np.argsort(s_begin, kind='stable')
  sb_sorted = s_begin[order]
  for s in range(int(s_begin.min()) if len(s_begin) else s_end, s_end):
    act = order[:np.searchsorted(sb_sorted, s, side='right')]  # rows with s_begin <= s
    j = (s - s_begin[act] + 1).astype(np.float64)[:, None]      # the row's own step index, 1-based
    m[act] = m[act] * b1
    v[act] = v[act] * b2
    u = h[s] * m[act] / (np.sqrt(v[act]) + eps)
    var[act] = var[act] - u
    au = np.abs(u)
    upd[act] += au
    inside = j <= K
    tail[act] += np.where(inside, 0.0, au)
    x = z0[act] * (1.0 - q**j)
    base = h[s] * am0[act] * b1**j / d0[act]
    rem[act] += np.where(inside, base * x**N_POW / (1.0 - x), 0.0)
    zsens[act] += np.where(inside, base * x / (1.0 - x)**2, 0.0)
    step_var[act] += (1.5 * j + 4.0) * 2 * U * au + 2 * U * np.abs(var[act])
  return dict(var=var, m=m, v=v, k=k, upd=upd, tail=tail, rem=rem, zsens=zsens, step_var=step_var, m0=am0,
              v0=np.abs(np.asarray(v0, dtype=np.float64)), d0=d0, b1=b1, b2=b2)


def _slot_floor(ref, what):
  b, x0 = (ref['b1'], ref['m0']) if what == 'm' else (ref['b2'], ref['v0'])
  with np.errstate(under='ignore'):
    tiny = ((b**ref['k'].astype(np.float64))[:, None] < FLT_MIN) | (np.abs(ref[what]) < FLT_MIN)
  return np.where(tiny & (x0 != 0), FLT_MIN * np.maximum(1.0, x0), 0.0)


def bounds_closed(ref):
  moved = ref['upd'] > 0
  var = (ref['tail'] + ref['rem'] + OPS_CLOSED * 2 * U * ref['upd'] + Z_OPS * 2 * U * ref['zsens'] +
         np.where(moved, 2 * U * np.abs(ref['var']), 0.0) + np.where(ref['m0'] != 0, DENORM_MIN * (1.0 + 1.0 / ref['d0']), 0.0))
  pending = (ref['k'] > 0)[:, None]
  return dict(var=np.where(pending, var, 0.0),
              m=np.where(pending, M_OPS * 2 * U * np.abs(ref['m']) + _slot_floor(ref, 'm'), 0.0),
              v=np.where(pending, M_OPS * 2 * U * np.abs(ref['v']) + _slot_floor(ref, 'v'), 0.0))


def bounds_steps(ref):
  kk = ref['k'].astype(np.float64)[:, None]
  moved = ref['upd'] > 0
  pending = kk > 0
  return dict(var=np.where(moved, ref['step_var'], 0.0),
              m=np.where(pending, kk * 2 * U * np.abs(ref['m']) + _slot_floor(ref, 'm'), 0.0),
              v=np.where(pending, kk * 2 * U * np.abs(ref['v']) + _slot_floor(ref, 'v'), 0.0))


def bounds_two_pieces(ref1, ref2):
  """A replay in two closed-form pieces (ref2 started from ref1's float64 result): the first piece's errors in m (M_OPS
  roundings) and in sqrt(v) (half of v's) scale the second piece's update, which is linear in m and no steeper than
  linear in sqrt(v)."""
  b1, b2 = bounds_closed(ref1), bounds_closed(ref2)
  carry = (M_OPS + 0.5 * M_OPS) * 2 * U * ref2['upd']
  return dict(var=b1['var'] + b2['var'] + carry,
              m=b2['m'] + M_OPS * 2 * U * np.abs(ref2['m']) + _slot_floor(ref1, 'm'),
              v=b2['v'] + M_OPS * 2 * U * np.abs(ref2['v']) + _slot_floor(ref1, 'v'))


def adam_step(ref, bound, rows, g, hyper):
  """One float64 Adam step with the gradient entries g [len(rows), dim] on `rows` of a replay's result (the optimizer formulas of
  _emb_bwd_cases.reference) -> (state dict, bound dict): the replay's bound carried through the step plus the step's own
  operations - m: two products and a sum; v: g * g, two products, a sum; the update: lr_t * m, sqrt, the sum, the division."""
  dim = ref['var'].shape[1]
  total = ref['var'].shape[0]
  lk = dict(ids=np.asarray(rows, dtype=np.int64), offsets=None, weights=None, combiner=ec.SUM, rows=total, key_base=0,
            n_rows=len(rows), max_nnz=len(rows), out_col=0)
  case = ec.Case(dim=dim, total_rows=total, lookups=[lk], dout=np.asarray(g, dtype=np.float32), table=ref['var'],
                 m=ref['m'], v=ref['v'])
  want = ec.reference(case, ec.OPT_LAZY_ADAM, hyper)
  h = np.asarray(hyper, dtype=np.float32).astype(np.float64)
  out = {k: np.array(ref[k]) for k in ('var', 'm', 'v')}
  bnd = {k: np.array(bound[k]) for k in ('var', 'm', 'v')}
  rows = want['touched']                      # (an id may be listed more than once: the row takes the sum, which the
  g64 = want['sums'][rows] * h[ec.H_GSCALE]   # caller keeps exact in float32 in any order)
  m1, v1, m2, v2 = ref['m'][rows], ref['v'][rows], want['m'][rows], want['v'][rows]
  em = 3 * 2 * U * (np.abs(m1) * h[ec.H_B1] + np.abs(g64) * h[ec.H_OMB1]) + h[ec.H_B1] * bound['m'][rows]
  ev = 3 * 2 * U * v2 + h[ec.H_B2] * bound['v'][rows]
  root = np.sqrt(v2)
  den = root + h[ec.H_EPS]
  upd = np.abs(h[ec.H_LR_T] * m2 / den)
  with np.errstate(divide='ignore', invalid='ignore'):
    eden = np.where(ev > 0, ev / (2 * root), 0.0)
  evar = (bound['var'][rows] + 4 * 2 * U * upd + h[ec.H_LR_T] * em / den + upd * eden / den +
          2 * U * np.abs(want['var'][rows]) + DENORM_MIN * (1.0 + 1.0 / den))
  for k, e in (('var', evar), ('m', em + DENORM_MIN), ('v', ev + DENORM_MIN)):
    out[k][rows] = want[k][rows]
    bnd[k][rows] = e
  return out, bnd


# ---------------------------------------------------------------------------------------------
# float32 restatement of er_decay.h + replay_closed (faults are seeded here and nowhere else)
# ---------------------------------------------------------------------------------------------
class Tables(object):
  """coef as er_decay_tables_create builds it; A(s_end) as decay_tables_kernel; C as the step prologue appends it."""

  def __init__(self, pair, fault=None, n_steps=S_TOTAL):
    self.b1, self.b2 = betas(pair)
    self.K = supported(self.b1, self.b2)
    assert self.K == EXPECTED_K[pair]
    self.fault = fault
    if fault == 'K_cut':
      self.K -= 64
    b1, lq = float(self.b1), 0.5 * math.log(float(self.b2))
    s = np.arange(1, self.K + 1, dtype=np.float64)
    p, w = np.exp(s * math.log(b1)), -np.expm1(s * lq)
    self.coef = p[:, None] * w[:, None]**np.arange(N_POW)[None, :]   # [K, N] double
    if fault == 'coef4_zero':
      self.coef[:, 4] = 0.0
    if fault == 'coef5_zero':
      self.coef[:, 5] = 0.0
    self.ln_b1, self.ln_b2 = math.log(b1), math.log(float(self.b2))
    self.hist = lr_history(pair).astype(np.float64)
    self.n_steps = n_steps
    self._A = {}
    self._C = None

  def T(self, t0, k):
    """T_n(t0, k), n < N: sum_{s=1..k} lr_t(t0+s) coef[s-1][n] in double, rounded to float32 (steps before 0 skipped)."""
    s = np.arange(1, k + 1)
    idx = t0 + s + (1 if self.fault == 'hist_shift' else 0)
    ok = idx >= 0
    return (self.hist[idx[ok]] @ self.coef[s[ok] - 1]).astype(np.float32)

  def A(self, s_end):
    if s_end not in self._A:
      rows = [self.T(s_end - 1 - k, k) for k in range(1, self.K + 1)]
      self._A[s_end] = np.stack(rows + [np.zeros(N_POW, dtype=np.float32)])  # (+ the zeroed row behind the table)
    return self._A[s_end]

  def C(self):
    """C[t0+1] = T(t0, K), appended at step t0 + K: rows 0 .. n_steps - K."""
    if self._C is None:
      self._C = np.stack([self.T(j - 1, self.K) for j in range(self.n_steps - self.K + 1)])
    return self._C


@functools.lru_cache(maxsize=None)
def tables(pair, fault=None):
  return Tables(pair, fault if fault in ('K_cut', 'coef4_zero', 'coef5_zero', 'hist_shift') else None)


def restate(var0, m0, v0, last, s_end, pair, fault=None, listed=None, eps=EPS):
  """replay_closed on every pending live lane, float32 -> dict(var, m, v float32)."""
  tb = tables(pair, fault)
  K = tb.K
  var, m, v = (np.array(a, dtype=np.float32) for a in (var0, m0, v0))
  rows, dim = var.shape
  s_begin = np.asarray(last, dtype=np.int64) + 1
  k = s_end - s_begin
  pending = k > 0
  if listed is not None:
    pending = pending & listed
  A, C = tb.A(s_end), tb.C()
  T = np.zeros((rows, N_POW), dtype=np.float32)
  for r in np.flatnonzero(pending):
    kr, sb = int(k[r]), int(s_begin[r])
    use_a = kr <= K + 1 if fault == 'switch_past' else (kr < K if fault == 'switch_lt' else kr <= K)
    if use_a:
      i = kr - 1 + (1 if fault == 'A_row_plus' else (-1 if fault == 'A_row_minus' and kr > 1 else 0))
      T[r] = A[min(i, K)]
    else:
      i = sb + (1 if fault == 'C_plus' else (-1 if fault == 'C_minus' else 0))
      T[r] = C[min(max(i, 0), len(C) - 1)]
  kd = np.maximum(k, 0).astype(np.float64)
  with np.errstate(under='ignore'):
    p1 = np.exp(tb.ln_b1 * kd).astype(np.float32)[:, None]
    p2 = np.exp((tb.ln_b1 if fault == 'p2_ln_b1' else tb.ln_b2) * kd).astype(np.float32)[:, None]
  eps = F32(eps)
  with np.errstate(all='ignore'):
    a = np.sqrt(v)
    d = a if fault == 'eps_dropped' else a + eps
    z = a / d
    poly = np.broadcast_to(T[:, 5:6], var.shape).astype(np.float32)
    for n in (4, 3, 2, 1, 0):
      poly = poly * z + T[:, n:n + 1]
    nvar = var - (m * poly) / d
    nm, nv = m * p1, v * p2
  assert nvar.dtype == np.float32 and nm.dtype == np.float32 and nv.dtype == np.float32
  mask = pending[:, None] & live_lanes(m, v, dim)
  return dict(var=np.where(mask, nvar, var), m=np.where(mask, nm, m), v=np.where(mask, nv, v))


def restate_steps(var0, m0, v0, last, s_end, pair, eps=EPS):
  """The same steps one by one in float32 (what the streaming sweep and the exact replay's full regime compute)."""
  b1, b2 = betas(pair)
  h = lr_history(pair)
  var, m, v = (np.array(a, dtype=np.float32) for a in (var0, m0, v0))
  s_begin = np.asarray(last, dtype=np.int64) + 1
  with np.errstate(under='ignore'):
    for s in range(int(s_begin.min()), s_end):
      act = s_begin <= s
      m[act] = m[act] * b1
      v[act] = v[act] * b2
      var[act] = var[act] - (h[s] * m[act]) / (np.sqrt(v[act]) + F32(eps))
  return dict(var=var, m=m, v=v)


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------
def ratio(got, ref, bound):
  """max |got - ref| / bound; inf where the bound is 0 and the values differ, nan -> inf."""
  got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
  with np.errstate(all='ignore'):
    diff = np.abs(got - ref)
    r = np.where(bound > 0, diff / np.maximum(bound, 1e-300), np.where(diff == 0, 0.0, np.inf))
  r = np.where(np.isnan(r), np.inf, r)
  return float(r.max()) if r.size else 0.0


def check(who, case, got, ref, bound, frac=1.0, what=('var', 'm', 'v')):
  """Print every error-to-bound ratio, then assert each is at most `frac`."""
  rs = {k: ratio(got[k], ref[k], bound[k]) for k in what}
  for k, r in rs.items():
    print('RATIO who=%s case=%s tensor=%s ratio=%.4g' % (who, case, k, r))
  bad = {k: r for k, r in rs.items() if not r <= frac}
  assert not bad, '%s %s: error / bound above %g: %s' % (who, case, frac, bad)
  return rs


@functools.lru_cache(maxsize=None)
def case_reference(pair, dim, s_end, rows=ROWS, ks=None):
  """-> (state, reference dict) of state(pair, dim, s_end, rows, ks) replayed to s_end; shared, not to be written."""
  st = state(pair, dim, s_end, rows, ks)
  b1, b2 = betas(pair)
  ref = reference(st.var, st.m, st.v, st.last, s_end, lr_history(pair), b1, b2, K=EXPECTED_K.get(pair))
  return st, ref


def pins_grid():
  out = [('usual', d, S_TOTAL) for d in DIMS] + [('usual', 16, S_TOTAL - 1), ('usual', 16, 3), ('usual', 1, 2)]
  out += [(p, d, S_TOTAL) for p in ('edge', 'long') for d in (3, 16)]
  return out
