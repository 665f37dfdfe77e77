"""-m gpu: the per-lookup LDS radix sort (seg_radix_sort_narrow: digit counts in registers, striped positions) and the
lookup half of the fused front launch (emb_front_fwd_kernel), through the wrappers tests/test_kernels_gpu.py uses, against
a host reference: a stable torch.sort of (row, position) per lookup.

The C ABI hands out no view of a group's sorted arrays, so they are held through what the library derives from them,
with values that make the derivation one-to-one:
  * er_emb_route (the stand-alone sort launch): the distinct-key list (the keys at the run heads, per lookup back to back),
    its length (the sum of seg_count) and every entry's index into it (head index + head flag - 1 + the distinct keys of
    the lookups before, scattered through the sorted entry numbers; -1 for a missing id);
  * er_emb_bwd_reduce: every distinct key's gradient, with integer-valued gradient rows (1, position, a hash of the
    position, a random integer): sums of at most 4096 of them are exact in fp32 in any order, so equality means every
    sorted key stands next to its own entry;
  * er_emb_front + er_emb_bwd_fused (the sort that builds its entries from the ids, with and without skip_one_row): SGD
    with lr = 0.5 from zero tables - var = -0.5 * the same exact sums, one-row tables reduced by columns.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402

DEV = 'cuda:0'
DIM = 4
INVALID = -1


@pytest.fixture(scope='module')
def hip():
  assert torch.cuda.is_available(), 'gpu tests need an MI355X'
  return kernels.hip()


def _ids(rng, n, rows):
  """Random ids with missing ones, a long run, and both ends of the table."""
  ids = rng.integers(-1, rows, size=n).astype(np.int64)
  ids[n // 2:n // 2 + n // 8] = ids[n // 2]
  ids[1], ids[-2] = rows - 1, 0
  return ids


def _case(name, n):
  """-> [(rows, ids)] of one table group."""
  rng = np.random.default_rng(n + sum(map(ord, name)))
  if name == 'all_equal':
    return [(1000, np.full(n, 7, dtype=np.int64))]
  if name == 'all_missing':
    return [(1000, np.full(n, -1, dtype=np.int64))]
  if name == 'one_row':
    ids = np.zeros(n, dtype=np.int64)
    ids[::5] = -1
    return [(1, ids)]
  if name.startswith('rows_'):
    rows = int(name[5:])
    return [(rows, _ids(rng, n, rows))]
  if name == 'short_lookup':  # fewer entries than the padded size: the padding sorts behind the missing ids
    return [(500, _ids(rng, n, 500)), (31, _ids(rng, n - n // 4 - 1, 31))]
  if name == 'mixed_1m_one_row':  # the number of key bits differs per workgroup
    one = np.zeros(n, dtype=np.int64)
    one[3::7] = -1
    return [(1000000, _ids(rng, n, 1000000)), (1, one), (33, _ids(rng, n, 33))]
  raise KeyError(name)


CASES = ['all_equal', 'all_missing', 'one_row', 'rows_31', 'rows_32', 'rows_33', 'rows_1024', 'rows_1000000',
         'short_lookup', 'mixed_1m_one_row']


def _grad_rows(rng, n):
  i = np.arange(n, dtype=np.int64)
  g = np.stack([np.ones(n, dtype=np.int64), i, (i * 7919) % 1009, rng.integers(-8, 9, size=n)], axis=1)
  return g.astype(np.float32)


def _reference(lookups, skip_one_row=False):
  """Stable sort of (row, position) per lookup -> per lookup: sorted keys, sorted entries, head flags, head indices,
  seg_count, distinct keys; and the group-wide outputs derived from them."""
  per, ukeys, uidx, base, n_before = [], [], [], 0, 0
  for rows, ids in lookups:
    ids_t = torch.from_numpy(ids)
    valid = (ids_t >= 0) & (ids_t < rows)
    if skip_one_row and rows == 1:
      valid = torch.zeros_like(valid)
    rel = torch.where(valid, ids_t, torch.full_like(ids_t, rows))
    srel, entries = torch.sort(rel, stable=True)
    ok = srel < rows
    keys = torch.where(ok, srel + base, torch.full_like(srel, INVALID))
    flags = ok.clone()
    flags[1:] &= srel[1:] != srel[:-1]
    hidx = torch.cumsum(flags.to(torch.int64), 0) - flags.to(torch.int64)
    seg_count = int(flags.sum())
    per.append(dict(keys=keys, entries=entries, flags=flags, hidx=hidx, seg_count=seg_count, ukeys=keys[flags]))
    ui = torch.full((len(ids),), -1, dtype=torch.int64)
    ui[entries[ok]] = (hidx + flags.to(torch.int64) - 1 + n_before)[ok]
    ukeys.append(keys[flags])
    uidx.append(ui)
    base += rows
    n_before += seg_count
  return per, torch.cat(ukeys), torch.cat(uidx), base


def _build(hip, lookups, rng):
  total = sum(r for r, _ in lookups)
  width = len(lookups) * DIM
  n_max = max(len(i) for _, i in lookups)
  dout = torch.zeros(n_max, width, device=DEV)
  var = torch.zeros(total, DIM, device=DEV)
  specs, sums, base = [], np.zeros((total, DIM), dtype=np.float64), 0
  col_sums = {}
  for li, (rows, ids) in enumerate(lookups):
    n = len(ids)
    g = _grad_rows(rng, n)
    dout[:n, li * DIM:(li + 1) * DIM] = torch.from_numpy(g).to(DEV)
    ok = (ids >= 0) & (ids < rows)
    np.add.at(sums, ids[ok] + base, g[ok].astype(np.float64))
    specs.append(kernels.LookupSpec(table=var[base:base + rows], ids=torch.from_numpy(ids).to(DEV), offsets=None,
                                    weights=None, out=dout, out_col=li * DIM, rows=rows, key_base=base, dim=DIM,
                                    combiner=0, n_rows=n, max_nnz=n))
    base += rows
  group = hip.emb_group_create(specs, DIM, total, var, None, None, None)
  return group, var, dout, sums


@pytest.mark.parametrize('n', [64, 4096])
@pytest.mark.parametrize('name', CASES)
def test_stand_alone_sort_outputs_equal_the_stable_host_sort(hip, name, n):
  lookups = _case(name, n)
  rng = np.random.default_rng(n)
  per, ukeys, uidx, total = _reference(lookups)
  group, var, dout, sums = _build(hip, lookups, rng)
  N = group['num_entries']
  assert N == sum(len(i) for _, i in lookups)
  uk = torch.full((N,), -7, dtype=torch.int32, device=DEV)
  nu = torch.zeros(1, dtype=torch.int32, device=DEV)
  ui = torch.full((N,), -7, dtype=torch.int64, device=DEV)
  hip.emb_route(group, uk, nu, ui, None)
  keys, grads, n_unique = hip.emb_bwd_reduce(group)
  torch.cuda.synchronize()
  k = len(ukeys)
  assert k == sum(p['seg_count'] for p in per)
  assert int(nu.item()) == k, 'sum of seg_count'
  assert torch.equal(uk[:k].cpu().to(torch.int64), ukeys), 'distinct-key lists'
  assert torch.equal(ui.cpu(), uidx), 'head index / head flag / sorted entry of every entry'
  assert int(n_unique.item()) == k
  assert torch.equal(keys[:k].cpu().to(torch.int64), ukeys)
  assert np.array_equal(grads[:k].cpu().numpy().astype(np.float64), sums[ukeys.numpy()]), 'sorted keys beside their entries'
  hip.emb_group_destroy(group)


def _sgd_hyper():
  row = np.zeros(kernels.HYPER_FLOATS, dtype=np.float32)
  row[kernels.HYPER_LR] = 0.5
  row[kernels.HYPER_LR_T] = 0.5
  row[kernels.HYPER_GSCALE] = 1.0
  return torch.from_numpy(row).to(DEV)


@pytest.mark.parametrize('skip_one_row', [False, True])
@pytest.mark.parametrize('n', [64, 4096])
@pytest.mark.parametrize('name', CASES)
def test_front_sort_feeds_the_fused_row_update_exact_sums(hip, name, n, skip_one_row):
  lookups = _case(name, n)
  rng = np.random.default_rng(n)
  group, var, dout, sums = _build(hip, lookups, rng)
  hyper = _sgd_hyper()
  out = torch.zeros_like(dout)
  assert hip.emb_front([group], None, skip_one_row)
  hip.emb_bwd_fused([group], [(dout, out, 0.0, True, [])], kernels.OPT_SGD, hyper)
  torch.cuda.synchronize()
  assert np.array_equal(var.cpu().numpy().astype(np.float64), -0.5 * sums), 'var = -lr * the exact gradient sums'
  hip.emb_group_destroy(group)


@pytest.mark.parametrize('B', [64, 4096])
def test_fused_front_lookup_equals_the_lookup_launch(hip, B):
  """The lookup half of the fused front (1024-thread workgroups of four 256-lane blocks, the last one partly empty:
  3 * B / 64 + 2 * B / 256 + (B - 300) / 256 blocks at B = 4096 is 239 = 59 workgroups and three blocks) against
  er_emb_fwd_lazy behind the front's sort as launches of their own: output rows and sumsq_partials bit for bit."""
  rng = np.random.default_rng(B)
  layout = [(16, B, 5000), (16, B, 33), (16, B, 1), (1, B, 700), (1, B, 1), (1, max(B - 300, 7), 64)]
  width = sum(d for d, _, _ in layout)
  results = []
  stor = {d: torch.from_numpy(rng.standard_normal((sum(r for dd, _, r in layout if dd == d), d)).astype(np.float32)).to(DEV)
          for d in (16, 1)}
  ids_all = []
  for d, n, rows in layout:
    ids = rng.integers(-1, rows, size=n).astype(np.int64)
    ids[rng.random(n) < 0.05] = rows + 2
    ids_all.append(torch.from_numpy(ids).to(DEV))
  for fused in (False, True):
    out = torch.full((B, width), 3.0, device=DEV)
    specs, base, col = [], {16: 0, 1: 0}, 0
    for (d, n, rows), ids in zip(layout, ids_all):
      specs.append(kernels.LookupSpec(table=stor[d][base[d]:base[d] + rows], ids=ids, offsets=None, weights=None, out=out,
                                      out_col=col, rows=rows, key_base=base[d], dim=d, combiner=0, n_rows=n, max_nnz=n))
      base[d] += rows
      col += d
    groups = [hip.emb_group_create([s for s in specs if s.dim == d], d, base[d], stor[d], None, None, None) for d in (16, 1)]
    plan = hip.emb_plan_create(specs)
    ssq = torch.full((plan['num_blocks'],), -1.0, device=DEV)
    if fused:
      assert hip.emb_front_fwd(groups, plan, None, True, ssq)
    else:
      assert hip.emb_front(groups, None, True, defer=True)
      hip.emb_fwd_lazy(plan, groups, None, ssq)
    torch.cuda.synchronize()
    results.append((out.cpu(), ssq.cpu(), plan['num_blocks']))
    hip.emb_plan_destroy(plan)
    for g in groups:
      hip.emb_group_destroy(g)
  (out_a, ssq_a, nb), (out_b, ssq_b, _) = results
  if B == 4096:
    assert nb % 4 != 0, 'the last fused workgroup must be partly empty'
  assert torch.equal(out_a, out_b), 'output rows'
  assert torch.equal(ssq_a, ssq_b), 'sumsq_partials'
  assert float(ssq_a.min()) >= 0.0 and float(ssq_a.sum()) > 0.0
