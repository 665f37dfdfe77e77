"""The closed-form decay replay's cases (tests/_decay_cases.py) without a GPU:
  * the float32 restatement of er_decay.h + replay_closed stays within HALF of every derived bound on every case (the
    ratios are printed; the worst are quoted in _decay_cases.py's docstring), and so does the plain float32 recurrence
    within the step-by-step bound;
  * the float64 reference is right: with a constant lr_t and eps = 0 the update is a geometric sum with a closed
    expression, which the recurrence must match to float64 accuracy;
  * a wrong replay would be noticed: every fault of _decay_cases.FAULTS, seeded into the restatement, exceeds the bound
    on at least one case.  Two variants are reported instead: the A / C switch at k < K is NOT a fault (at k = K the two
    tables hold the same sum T(t0, K), which the test asserts bit for bit; the switch one row late, `switch_past`, is the
    fault that shows), and a zeroed n = 5 coefficient sits inside the bound;
  * the cases reach the branches they claim (k <= K and k > K, p1 == 0, a subnormal m);
  * decay_terms / supported equal er_decay_tables_supported over a grid of betas (the library loads without a GPU).
`python tests/test_decay_pins.py` prints every figure.
"""
import os
import sys

import numpy as np
import pytest

if __name__ == '__main__':
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _decay_cases as dc  # noqa: E402
from tests import _emb_bwd_cases as ec  # noqa: E402

S = dc.S_TOTAL
FAULT_CASES = [('usual', 16, S), ('usual', 16, S - 1), ('edge', 16, S), ('long', 16, S)]


def _closed(pair, dim, s_end, fault=None):
  st, ref = dc.case_reference(pair, dim, s_end)
  return st, ref, dc.restate(st.var, st.m, st.v, st.last, s_end, pair, fault)


@pytest.mark.parametrize('pair,dim,s_end', dc.pins_grid())
def test_float32_restatement_stays_within_half_of_every_bound(pair, dim, s_end):
  st, ref, got = _closed(pair, dim, s_end)
  name = '%s-d%d-s%d' % (pair, dim, s_end)
  dc.check('restatement', name, got, ref, dc.bounds_closed(ref), frac=0.5)
  # rows with nothing pending, lanes that are not live: every bit
  still = (st.k == 0)[:, None] | ~dc.live_lanes(st.m, st.v, dim)
  for k, a in (('var', st.var), ('m', st.m), ('v', st.v)):
    assert np.array_equal(got[k][still], np.broadcast_to(a, still.shape)[still]), k
  zero_var = (st.var == 0) & (ref['upd'] > 0)
  assert zero_var.any()
  dev = np.abs(got['var'].astype(np.float64) - ref['var'])[zero_var] / ref['upd'][zero_var] / dc.U
  print('UPDATE-DEVIATION case=%s where var0 = 0: at most %.3g U' % (name, float(dev.max())))


@pytest.mark.parametrize('pair,dim,s_end', [('usual', 16, S), ('edge', 3, S), ('long', 16, S), ('usual', 16, 3)])
def test_float32_recurrence_stays_within_half_of_the_step_bound(pair, dim, s_end):
  st, ref = dc.case_reference(pair, dim, s_end)
  got = dc.restate_steps(st.var, st.m, st.v, st.last, s_end, pair)
  dc.check('fp32-steps', '%s-d%d-s%d' % (pair, dim, s_end), got, ref, dc.bounds_steps(ref), frac=0.5)


def test_reference_matches_the_geometric_sum():
  """constant lr_t, eps = 0:  var' = var0 - lr m0 / sqrt(v0) * r (1 - r^k) / (1 - r),  r = b1 / sqrt(b2)"""
  rng = np.random.default_rng(5)
  for pair in dc.PAIRS:
    b1f, b2f = dc.betas(pair)
    b1, b2 = float(b1f), float(b2f)
    ks = np.array([1, 2, 64, 191, 192, 193, 700, 1500])
    m0 = (rng.standard_normal((len(ks), 8)) * 1e-3).astype(np.float32)
    v0 = (rng.random((len(ks), 8)) * 1e-6 + 1e-8).astype(np.float32)
    var0 = np.zeros((len(ks), 8), dtype=np.float32)  # (var' = -update: no cancellation in the comparison)
    lr = np.float32(3e-3)
    hist = np.full(S, lr, dtype=np.float32)
    ref = dc.reference(var0, m0, v0, S - 1 - ks, S, hist, b1f, b2f, eps=0.0)
    r = b1 / np.sqrt(b2)
    kk = ks.astype(np.float64)[:, None]
    geo = float(lr) * m0.astype(np.float64) / np.sqrt(v0.astype(np.float64)) * r * (1.0 - r**kk) / (1.0 - r)
    assert np.allclose(-ref['var'], geo, rtol=1e-11, atol=0.0), pair
    assert np.allclose(ref['upd'], np.abs(geo), rtol=1e-11, atol=0.0)
    assert np.allclose(ref['m'], m0.astype(np.float64) * b1**kk, rtol=1e-12, atol=0.0)
    assert np.allclose(ref['v'], v0.astype(np.float64) * b2**kk, rtol=1e-12, atol=0.0)


def _worst(fault, cases):
  worst = {}
  for pair, dim, s_end in cases:
    st, ref, got = _closed(pair, dim, s_end, fault)
    bound = dc.bounds_closed(ref)
    worst[(pair, s_end)] = max(dc.ratio(got[k], ref[k], bound[k]) for k in ('var', 'm', 'v'))
  return worst


@pytest.mark.parametrize('fault', dc.FAULTS)
def test_a_seeded_fault_exceeds_the_bound(fault):
  cases = [c for c in FAULT_CASES if c[0] == 'edge'] if fault == 'coef4_zero' else FAULT_CASES
  worst = _worst(fault, cases)
  for c, r in worst.items():
    print('FAULT %s case=%s-s%d worst error / bound = %.4g' % (fault, c[0], c[1], r))
  assert max(worst.values()) > 1.0, (fault, worst)


def test_variants_that_are_reported_not_asserted():
  # the switch at k < K: row K reads C[s_begin] = T(t0, K), the very sum A[K-1] holds - the same bits, not a fault
  for pair, dim, s_end in FAULT_CASES:
    st, ref, right = _closed(pair, dim, s_end)
    wrong = dc.restate(st.var, st.m, st.v, st.last, s_end, pair, 'switch_lt')
    assert (st.k == dc.EXPECTED_K[pair]).any()
    for k in ('var', 'm', 'v'):
      assert np.array_equal(right[k], wrong[k]), (pair, k)
  for n, cases in (('coef5_zero', [c for c in FAULT_CASES if c[0] == 'edge']), ('coef5_zero', FAULT_CASES[:1])):
    right, wrong = _worst(None, cases), _worst(n, cases)
    for c in right:
      print('REPORT %s case=%s-s%d: worst error / bound %.4g (right evaluation: %.4g)' % (n, c[0], c[1], wrong[c], right[c]))


def test_the_cases_reach_the_branches_they_claim():
  for pair in dc.PAIRS:
    st, ref, got = _closed(pair, 16, S)
    K = dc.EXPECTED_K[pair]
    live = dc.live_lanes(st.m, st.v, 16).any(axis=1)
    ks = set(st.k[live].tolist())
    assert {0, 1, 2, 63, 64, 65, K - 1, K, K + 1, K + 64, 700, 1500, S} <= ks, (pair, sorted(ks))
    assert (st.last[live] == -1).any() and not live.all()
    cls = set(st.cls[live].ravel().tolist())
    assert cls == set(range(6))
    a = np.sqrt(st.v[live].astype(np.float64))
    assert (a > 1e3 * dc.EPS).any() and ((a > 0.3 * dc.EPS) & (a < 3 * dc.EPS)).any() and ((a > 0) & (a < 1e-3 * dc.EPS)).any()
    assert ((st.v == 0) & (st.m != 0)).any() and ((st.var == 0) & (st.m != 0)).any()
    assert (ref['tail'] > 0).any() and (ref['rem'] > 0).any()
  st, ref, got = _closed('usual', 16, S)
  p1 = np.exp(np.log(float(dc.betas('usual')[0])) * st.k.astype(np.float64)).astype(np.float32)
  assert (p1[st.k > 0] == 0).any(), 'beta1^k below the smallest float32'
  sub = (got['m'] != 0) & (np.abs(got['m']) < dc.FLT_MIN)
  assert sub.any(), 'a subnormal m'
  st3, _ = dc.case_reference('usual', 16, 3)
  assert set(st3.last.tolist()) == {-1, 0, 1, 2}


def test_adam_step_behind_the_replay_stays_within_half_of_its_bound():
  pair, dim, s_end = 'usual', 16, S - 1
  st, ref, got = _closed(pair, dim, s_end)
  rows = np.arange(0, dc.ROWS, 2)
  g = (np.random.default_rng(2).standard_normal((len(rows), dim)) * 1e-3).astype(np.float32)
  h = dc.hyper_rows(pair)[s_end]
  want, bound = dc.adam_step(ref, dc.bounds_closed(ref), rows, g, h)
  out = {k: got[k].copy() for k in got}
  m = out['m'][rows] * h[ec.H_B1] + g * h[ec.H_OMB1]
  v = out['v'][rows] * h[ec.H_B2] + (g * g) * h[ec.H_OMB2]
  out['var'][rows] = out['var'][rows] - (h[ec.H_LR_T] * m) / (np.sqrt(v) + h[ec.H_EPS])
  out['m'][rows], out['v'][rows] = m, v
  assert out['var'].dtype == np.float32
  dc.check('restatement+adam', '%s-d%d' % (pair, dim), out, want, bound, frac=0.5)


def test_acceptance_criterion_equals_the_library(built_lib):
  from easyrec_amd import kernels
  lib = kernels.load_library(built_lib)
  grid1 = [0.0, 0.5, 0.8, 0.9, 0.93, 0.95, 0.96, 0.9601, 0.962, 0.97, 0.99, 1.0]
  grid2 = [0.0, 0.9, 0.99, 0.995, 0.9955, 0.996, 0.9965, 0.997, 0.999, 0.9999, 1.0]
  seen = set()
  for b1 in grid1:
    for b2 in grid2:
      K = dc.supported(b1, b2)
      assert int(lib.er_decay_tables_supported(b1, b2)) == K, (b1, b2, K)
      seen.add(K)
  assert {0, 64, 128, 192, 512} <= seen, sorted(seen)
  for pair, (b1, b2) in dc.PAIRS.items():
    assert int(lib.er_decay_tables_supported(b1, b2)) == dc.EXPECTED_K[pair] == dc.supported(b1, b2)
  assert int(lib.er_decay_tables_supported(*dc.REFUSED)) == 0 == dc.supported(*dc.REFUSED)
  assert dc.supported(0.9, 0.995) == 0 and dc.decay_terms(0.9) == 192 and dc.decay_terms(0.96) == 512
  # the edge pair is accepted with margin: a float32 ulp of beta2 either way does not flip it
  b1, b2 = dc.betas('edge')
  for nb in (np.nextafter(b2, np.float32(0)), b2, np.nextafter(b2, np.float32(1))):
    r = dc.remainder(b1, nb, 192)
    assert 2.5e-8 < r < 2.95e-8, r
  assert dc.remainder(b1, np.float32(0.9965), 192) < r


if __name__ == '__main__':
  sys.exit(pytest.main([__file__, '-s', '-q']))
