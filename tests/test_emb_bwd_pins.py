"""The embedding-backward cases (tests/_emb_bwd_cases.py) without a GPU:
  * every plan really puts its runs where it claims (positions(): recomputed from the sorted keys the way tile_body /
    fix_body decide their branches);
  * on the exact inputs the float64 reference, cast to float32, equals the oracle's source-order float32 restatement
    (RefBackend.emb_bwd_reduce / emb_bwd_update) bit for bit, and two deliberately broken references do not;
  * on the random inputs the restatement's float32 error against the float64 reference is printed and must not exceed
    the MEASURED table of _emb_bwd_cases.py; the GPU bars (GPU_FACTOR x MEASURED) must stay under BAR_CAP.  If a bar
    exceeds the cap, change the case's inputs, not the cap.

Regenerating MEASURED (after a change of the cases): `python tests/test_emb_bwd_pins.py --regen` prints the table's
lines (each value rounded up to four digits); paste them over the table.  `--positions` prints, per dim, V, G, T and
the branches every plan variant reaches.
"""
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == '__main__':
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import kernel_ref  # noqa: E402
from tests import _emb_bwd_cases as ec  # noqa: E402


def _ref_group(case, with_state=True):
  """-> (RefBackend, its group over fresh copies of the case's arrays, (var, m, v))."""
  be = kernel_ref.RefBackend()
  var = torch.from_numpy(case.table.copy())
  m, v = torch.from_numpy(case.m.copy()), torch.from_numpy(case.v.copy())
  dout = torch.from_numpy(case.dout)
  t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
  specs = [kernel_ref._Spec(table=var[lk['key_base']:lk['key_base'] + lk['rows']], ids=t(lk['ids']), offsets=t(lk['offsets']),
                            weights=t(lk['weights']), out=dout, out_col=lk['out_col'], rows=lk['rows'],
                            key_base=lk['key_base'], dim=case.dim, combiner=lk['combiner'], n_rows=lk['n_rows'],
                            max_nnz=lk['max_nnz'], name='') for lk in case.lookups]
  g = be.emb_group_create(specs, case.dim, case.total_rows, var, m, v, None)
  assert g['num_entries'] == case.num_entries
  return be, g, (var, m, v)


# ------------------------------------------------------------------------------------------- geometry and positions
def test_tile_entries_table():
  want = {4: 1024, 8: 512, 1: 512, 16: 256, 12: 256, 2: 256, 32: 128, 3: 128, 20: 128, 64: 64, 5: 64, 128: 32, 256: 16}
  assert {d: ec.tile_entries(d) for d in want} == want
  assert ec.lane_geom(12) == (4, 4) and ec.lane_geom(5) == (1, 8) and ec.lane_geom(20) == (4, 8)  # idle lanes: col_ok false


def _expected_positions(T, plan):
  if plan in ('base', 'with_invalid'):
    return dict(from_prev=[1, 3, 4, 5, 6, 9, 10], to_next=[0, 2, 3, 4, 5, 8, 9], both_different=[5],
                whole_tile_crossed=[3, 4, 9], fix_owners=[0, 2, 5, 8], fix_whole_tiles=[0, 2, 0, 1],
                aligned_whole_tile_runs=1, minimal_crossings=1, longest_run=3 * T + 5)
  if plan == 'tail_aligned':
    return dict(from_prev=[1, 3, 4, 5, 6, 9, 10, 11], to_next=[0, 2, 3, 4, 5, 8, 9, 10], both_different=[5, 10],
                whole_tile_crossed=[3, 4, 9], fix_owners=[0, 2, 5, 8, 10], fix_whole_tiles=[0, 2, 0, 1, 0],
                aligned_whole_tile_runs=1, minimal_crossings=1, longest_run=3 * T + 5)
  if plan == 'tail_plus_one':
    return dict(from_prev=[1, 3, 4, 5, 6, 9, 10], to_next=[0, 2, 3, 4, 5, 8, 9], both_different=[5],
                whole_tile_crossed=[3, 4, 9], fix_owners=[0, 2, 5, 8], fix_whole_tiles=[0, 2, 0, 1],
                aligned_whole_tile_runs=1, minimal_crossings=1, longest_run=3 * T + 5)
  return dict(from_prev=[], to_next=[], both_different=[], whole_tile_crossed=[], fix_owners=[], fix_whole_tiles=[],
              aligned_whole_tile_runs=0, minimal_crossings=0, longest_run=1)


@pytest.mark.parametrize('dim', ec.DIMS)
def test_plans_reach_the_claimed_positions(dim):
  T = ec.tile_entries(dim)
  for plan in ec.PLANS:
    for split in ec.SPLITS:
      case = ec.make_case(dim, plan, split, 'exact')
      pos = ec.positions(ec.sorted_keys(case), T)
      want = _expected_positions(T, plan)
      assert {k: pos[k] for k in want} == want, (dim, plan, split)
      if plan != 'all_distinct':
        # a run that ends on a tile's last entry followed by another key: run 2 | the pad run | the aligned whole tile
        assert pos['ends_on_tile_end_then_other_key'] >= 3, (dim, plan, split)
      padded = split == 'three' and dim in (1, 4) and plan != 'tail_aligned'
      if plan == 'tail_aligned':
        assert pos['n_mod_T'] == 0 and pos['fix_ends_on_tile_end'] == 1
        if not (split == 'three' and dim == 1):  # (there whole tiles of missing ids follow: 8200 entries in one lookup)
          assert pos['n'] == 12 * T and pos['last_run_ends_on_last_entry'] and pos['fix_ends_in_last_tile_at_n'] == 1
          assert pos['invalid'] == 0
      elif plan == 'tail_plus_one':
        assert pos['n_mod_T'] == 1
        if not padded:
          assert pos['n'] == 10 * T + 1 and pos['fix_ends_in_last_tile_at_n'] == 1 and pos['last_run_ends_on_last_entry']
      elif plan == 'base':
        assert pos['n_mod_T'] == 8
        if not padded:
          assert pos['n'] == 10 * T + 8 and pos['invalid'] == 0
      elif plan == 'all_distinct':
        assert pos['n_mod_T'] == 7
        if not padded:
          assert pos['n'] == 2 * T + 7
      else:
        n_valid = 10 * T + 8
        assert pos['n'] - pos['invalid'] == n_valid and pos['invalid_in_last_tile'] > 0
        assert not pos['last_run_ends_on_last_entry']
        if not padded:
          assert abs(pos['invalid'] / pos['n'] - 0.15) < 0.01
          ids = case.lookups[0]['ids']
          assert (ids == -1).any() and (ids == case.lookups[0]['rows'] + 3).any()
  assert ec.positions(ec.sorted_keys(ec.make_case(dim, 'all_invalid', 'one', 'exact')), T)['invalid'] == 2 * T + 7


def test_wide_split_and_second_table():
  for dim in (1, 4):
    for plan in ec.PLANS:
      assert ec.make_case(dim, plan, 'three', 'exact').lookups[0]['n_rows'] == ec.WIDE_FIRST > 8192
  for dim in ec.DIMS:
    case = ec.make_case(dim, 'base', 'two_tables', 'exact')
    a, b = case.lookups
    assert b['key_base'] == a['rows'] and a['rows'] + b['rows'] == case.total_rows
    keys = ec.entries(case)[0]
    uk, cnt = np.unique(keys, return_counts=True)
    assert uk[np.argmax(cnt)] == b['key_base'] and cnt.max() == 3 * case.T + 5  # the long run: row 0 of the second table
    w = ec.make_case(dim, 'base', 'three', 'exact').lookups[1]['weights']
    assert set(np.unique(w)) <= {-2.0, -1.0, 1.0, 2.0, 3.0} and (w < 0).any()


def test_ragged_cases_have_the_bags_and_the_runs():
  for dim in ec.RAGGED_DIMS:
    case = ec.make_case(dim, 'base', 'ragged', 'random')
    assert [lk['combiner'] for lk in case.lookups] == [ec.SUM, ec.MEAN, ec.SQRTN]
    assert case.lookups[0]['weights'] is None and all(lk['weights'] is not None for lk in case.lookups[1:])
    for lk in case.lookups:
      lens = np.diff(lk['offsets'])
      assert 0.1 < np.mean(lens == 0) < 0.3 and lens.max() == 4 and lk['max_nnz'] == lk['offsets'][-1] + 7
    pos = ec.positions(ec.sorted_keys(case), case.T)
    want = _expected_positions(case.T, 'base')  # the first table's entries are all kept: the plan's positions hold in it
    assert pos['from_prev'][:7] == want['from_prev'] and pos['fix_whole_tiles'][:4] == want['fix_whole_tiles']
    assert pos['longest_run'] == 3 * case.T + 5


# ------------------------------------------------------------------------------------------- exact inputs
@pytest.mark.parametrize('dim', ec.DIMS)
def test_exact_reference_equals_the_restatement_bit_for_bit(dim):
  hyper = ec.hyper_of('exact')
  for plan in ec.PLANS + ('all_invalid',):
    for split in (ec.SPLITS if plan != 'all_invalid' else ('one',)):
      case = ec.make_case(dim, plan, split, 'exact')
      want = ec.reference(case, ec.OPT_SGD, hyper)
      for a in (want['sums'], want['var']):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), 'the exact inputs must be exact in float32'
      be, g, (var, _, _) = _ref_group(case)
      keys, grads, n = be.emb_bwd_reduce(g)
      n = int(n.item())
      assert np.array_equal(keys[:n].numpy(), want['touched']), (dim, plan, split)
      assert np.array_equal(grads[:n].numpy(), want['sums'][want['touched']].astype(np.float32)), (dim, plan, split)
      be.emb_bwd_update(g, ec.OPT_SGD, torch.from_numpy(hyper))
      assert np.array_equal(var.numpy(), want['var'].astype(np.float32)), (dim, plan, split)
      untouched = np.setdiff1d(np.arange(case.total_rows), want['touched'])
      assert len(untouched) and np.array_equal(want['var'][untouched], case.table[untouched].astype(np.float64))


@pytest.mark.parametrize('dim', ec.DIMS)
def test_a_broken_reference_differs(dim):
  hyper = ec.hyper_of('exact', clip=0.25)
  for split in ec.SPLITS:
    case = ec.make_case(dim, 'base', split, 'exact')
    good = ec.reference(case, ec.OPT_SGD, hyper)
    be, g, (var, _, _) = _ref_group(case)
    be.emb_bwd_update(g, ec.OPT_SGD, torch.from_numpy(hyper))
    assert np.array_equal(var.numpy(), good['var'].astype(np.float32))  # (clip_scale applied after grad_scale)
    for broken in ('drop_last', 'misattribute'):
      bad = ec.reference(case, ec.OPT_SGD, hyper, broken=broken)
      assert not np.array_equal(bad['sums'].astype(np.float32), good['sums'].astype(np.float32)), (dim, split, broken)
      assert not np.array_equal(bad['var'].astype(np.float32), var.numpy()), (dim, split, broken)


# ------------------------------------------------------------------------------------------- random inputs
def _measure(args, opts):
  """-> {MEASURED key: err} of the float32 source-order restatement after two updates, as the GPU test runs them."""
  case = ec.make_case(*args)
  hyper = ec.hyper_of('random')
  out = {}
  for opt in opts:
    want = ec.reference(case, opt, hyper, steps=2)
    be, g, (var, m, v) = _ref_group(case)
    for _ in range(2):
      be.emb_bwd_update(g, opt, torch.from_numpy(hyper))
    for what, got, init in (('var', var, case.table), ('m', m, case.m), ('v', v, case.v)):
      if what in ec.quantities(opt):
        out[ec.measured_key(case, opt, what)] = ec.rel_err(got.numpy(), want[what], init)
  return out


def _round_up(x):
  return float('%.3e' % (x * 1.001))


@pytest.mark.parametrize('args,opts', ec.random_grid(), ids=lambda a: '-'.join(map(str, a)))
def test_restatement_error_stays_under_the_measured_table(args, opts):
  for key, err in sorted(_measure(args, opts).items()):
    print('%-48s err %.3e  table %.3e' % (key, err, ec.MEASURED.get(key, float('nan'))))
    assert key in ec.MEASURED, key
    assert err <= ec.MEASURED[key], (key, err)
    assert ec.GPU_FACTOR * ec.MEASURED[key] <= ec.BAR_CAP, (key, 'change the inputs of the case, not the cap')


def test_measured_table_has_no_stale_entries():
  keys = set()
  for args, opts in ec.random_grid():
    case = ec.make_case(*args)
    keys |= {ec.measured_key(case, opt, what) for opt in opts for what in ec.quantities(opt)}
  assert keys == set(ec.MEASURED)


def _print_positions():
  for dim in ec.DIMS:
    V, G = ec.lane_geom(dim)
    T = ec.tile_entries(dim)
    print('dim %d: V %d G %d T %d' % (dim, V, G, T))
    for plan in ec.PLANS:
      p = ec.positions(ec.sorted_keys(ec.make_case(dim, plan, 'one', 'exact')), T)
      print('  %-13s N %5d N%%T %4d from_prev %s to_next %s both(different keys) %s whole tiles per fix owner %s '
            'ends at N %d invalid in last tile %d' % (plan, p['n'], p['n_mod_T'], p['from_prev'], p['to_next'], p['both_different'],
                                                     dict(zip(p['fix_owners'], p['fix_whole_tiles'])),
                                                     p['fix_ends_in_last_tile_at_n'], p['invalid_in_last_tile']))


if __name__ == '__main__':
  if '--positions' in sys.argv:
    _print_positions()
  if '--regen' in sys.argv:
    for args, opts in ec.random_grid():
      for key, err in sorted(_measure(args, opts).items()):
        print("    '%s': %.3e," % (key, _round_up(err)))
