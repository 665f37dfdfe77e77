"""er_knn_search / er_knn_hits (csrc/er_knn.hip, include/easyrec_hip.h K9k) on the GPU.

Exact cases: embeddings drawn from the integers -3 .. 3, so every fp32 chain is exact and ties are plentiful; ids, rows
and distances must EQUAL a numpy integer computation sorted by (score, row), over table sizes around K and around the
item tile, query counts around the query tile, every D / K edge, both metrics, identical rows, and best rows on both
sides of a slice boundary.  Slice counts, repeated runs and a replayed graph give the same bits.  Random fp32 data is
held to an fp64 oracle with eps = 1e-6 * sum_d |q_d x_d| (ip) / 1e-6 * (|q|^2 + |x|^2 + 2 sum_d |q_d x_d|) (l2): three
times what an unfused fp32 chain reaches at D <= 128 (3.4e-7 of those sums)."""
import json
import os

import numpy as np
import pytest
import torch

from easyrec_amd import kernels
from easyrec_amd.core import hit_rate as hit_rate_lib
from easyrec_amd.core import knn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
QT, IT = knn.QUERY_TILE, knn.ITEM_TILE
HERE = os.path.dirname(os.path.abspath(__file__))


def int_data(seed, nq, n, D):
  rng = np.random.default_rng(seed)
  return rng.integers(-3, 4, size=(nq, D)), rng.integers(-3, 4, size=(n, D)), rng.permutation(n).astype(np.int64) + 10 ** 12


def int_oracle(Q, X, ids, K, metric):
  """(ids, rows, dist) of the integer computation, sorted by (score, row)"""
  s = Q.astype(np.int64) @ X.astype(np.int64).T
  if metric == 0:
    s = (Q.astype(np.int64) ** 2).sum(1)[:, None] + (X.astype(np.int64) ** 2).sum(1)[None, :] - 2 * s
    assert s.min() >= 0
  order = np.argsort(-s if metric == 1 else s, axis=1, kind='stable')[:, :K]  # (stable: the lower row first)
  nq, k = order.shape
  out_ids = np.full((nq, K), -1, dtype=np.int64)
  out_rows = np.full((nq, K), -1, dtype=np.int32)
  out_dist = np.full((nq, K), -np.inf if metric == 1 else np.inf, dtype=np.float32)
  out_ids[:, :k], out_rows[:, :k] = ids[order], order
  out_dist[:, :k] = np.take_along_axis(s, order, axis=1)
  return out_ids, out_rows, out_dist


def run_kernel(Q, X, ids, K, metric, slices=0):
  index = knn.ItemIndex(ids, np.ascontiguousarray(X, dtype=np.float32), metric, DEV)
  assert index.uses_kernel(K, slices)
  got = index.search_rows(np.ascontiguousarray(Q, dtype=np.float32), K, slices)
  torch.cuda.synchronize()
  return [t.cpu().numpy() for t in got]


def assert_equal(got, want, what):
  for g, w, name in zip(got, want, ('ids', 'rows', 'dist')):
    assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
    assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


def _cases():
  cases = []
  for K in (5, 100):
    for n in sorted({1, K - 1, K, K + 1, IT - 1, IT, IT + 1, 5000}):
      cases.append((QT + 1, n, 32, K))
  for nq in (1, QT - 1, QT, QT + 1):
    cases.append((nq, IT + 1, 3, 5))
  for D in (1, 3, 32, 33, 128):
    cases.append((QT + 1, 2 * IT + 44, D, 5))
  for K in (1, 5, 100, 128):
    cases += [(QT + 1, 2 * IT + 44, 32, K), (3, 5000, 128, K)]
  return sorted(set(cases))


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('nq,n,D,K', _cases())
def test_integer_cases_equal_the_integer_computation(built_lib, nq, n, D, K, metric):
  Q, X, ids = int_data(nq * 7 + n * 3 + D + K, nq, n, D)
  assert_equal(run_kernel(Q, X, ids, K, metric), int_oracle(Q, X, ids, K, metric), (nq, n, D, K, metric))


@pytest.mark.parametrize('metric', [0, 1])
def test_identical_rows_come_back_in_row_order(built_lib, metric):
  K, n = 100, 3 * IT + 5
  Q, X, ids = int_data(5, QT + 1, 1, 32)
  X = np.repeat(X, n, axis=0)
  ids = np.arange(n, dtype=np.int64) * 3
  for slices in (0, 1, 3):
    _, rows, _ = run_kernel(Q, X, ids, K, metric, slices)
    assert np.array_equal(rows, np.tile(np.arange(K, dtype=np.int32), (QT + 1, 1))), slices


@pytest.mark.parametrize('metric', [0, 1])
def test_best_rows_on_both_sides_of_a_slice_boundary(built_lib, metric):
  n, slices, K, D = 5000, 7, 5, 32
  L = -(-n // slices)
  rng = np.random.default_rng(11)
  Q = rng.integers(1, 4, size=(QT + 1, D))
  X = rng.integers(-3, 3, size=(n, D))
  ids = rng.permutation(n).astype(np.int64)
  if metric == 1:
    X[L - 1] = X[L] = 3   # the largest inner product with every positive query
  else:
    Q[:] = Q[0]
    X[L - 1] = X[L] = Q[0]  # distance 0
  want = int_oracle(Q, X, ids, K, metric)
  assert (want[1][:, :2] == [L - 1, L]).all()
  for s in (slices, 1, 0):
    assert_equal(run_kernel(Q, X, ids, K, metric, s), want, s)


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('K', [5, 100])
def test_slices_runs_and_graph_replay_give_the_same_bits(built_lib, K, metric):
  n, nq, D = 5000, QT + 1, 32
  Q, X, ids = int_data(3, nq, n, D)
  Q2 = int_data(4, nq, n, D)[0]
  want, want2 = int_oracle(Q, X, ids, K, metric), int_oracle(Q2, X, ids, K, metric)
  for slices in (1, 2, 7, 0, 0):
    assert_equal(run_kernel(Q, X, ids, K, metric, slices), want, slices)
  index = knn.ItemIndex(ids, X.astype(np.float32), metric, DEV)
  q_dev = torch.from_numpy(Q.astype(np.float32)).to(DEV)
  be = kernels.hip()
  be.knn_search(q_dev, index.item_emb, index.xx, index.item_ids, K, metric, 7)  # (first call outside the capture)
  torch.cuda.synchronize()
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    out = be.knn_search(q_dev, index.item_emb, index.xx, index.item_ids, K, metric, 7)
  for q_host, w in ((Q, want), (Q2, want2)):
    q_dev.copy_(torch.from_numpy(q_host.astype(np.float32)))
    g.replay()
    torch.cuda.synchronize()
    assert_equal([t.cpu().numpy() for t in out], w, 'replay')


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('K', [5, 100])
@pytest.mark.parametrize('D', [32, 128])
def test_random_fp32_against_the_fp64_oracle(built_lib, D, K, metric):
  n, nq = 5000, 65
  rng = np.random.default_rng(D + K + metric)
  Q = (0.5 * rng.standard_normal((nq, D))).astype(np.float32)
  X = (0.5 * rng.standard_normal((n, D))).astype(np.float32)
  ids = rng.permutation(n).astype(np.int64) + 77
  got_ids, rows, dist = run_kernel(Q, X, ids, K, metric)
  Q64, X64 = Q.astype(np.float64), X.astype(np.float64)
  s = Q64 @ X64.T
  mag = np.abs(Q64) @ np.abs(X64).T
  if metric == 1:
    eps, better = 1e-6 * mag, 1.0
  else:
    qq, xx = (Q64 ** 2).sum(1)[:, None], (X64 ** 2).sum(1)[None, :]
    s, eps, better = (qq + xx) - 2.0 * s, 1e-6 * (qq + xx + 2.0 * mag), -1.0
  assert ((rows >= 0) & (rows < n)).all() and np.array_equal(got_ids, ids[rows])
  worst_err = worst_miss = 0.0
  for q in range(nq):
    r = rows[q]
    assert len(set(r.tolist())) == K
    d = dist[q].astype(np.float64)
    step = better * np.diff(d)
    assert (step <= 0).all(), q                       # monotone: never better than the one before
    assert (np.diff(r)[step == 0] > 0).all(), q      # ties in ascending row
    err = np.abs(d - s[q, r]) / eps[q, r]
    worst_err = max(worst_err, err.max())
    assert (err <= 1.0).all(), (q, err.max())
    # every row not returned: no better than the worst returned oracle score by more than 2 eps
    rest = np.ones(n, dtype=bool)
    rest[r] = False
    worst = (better * s[q, r]).min()
    miss = (better * s[q, rest] - worst) / (2.0 * eps[q, rest])
    worst_miss = max(worst_miss, miss.max())
    assert (miss <= 1.0).all(), (q, miss.max())
  print('D %d K %d metric %d: worst |dist - oracle| / eps %.3g, worst miss / 2 eps %.3g' % (D, K, metric, worst_err, worst_miss))


def hits_restatement(ids, num, gt_items, I):
  hits = [len(set(g) & set(ids[u, :max(0, min(int(num[u]), I))].reshape(-1).tolist())) for u, g in enumerate(gt_items)]
  return np.array(hits, dtype=np.int32), np.array([len(g) for g in gt_items], dtype=np.int32)


def run_hits(ids, num, gt_items):
  off = np.zeros(len(gt_items) + 1, dtype=np.int64)
  np.cumsum([len(g) for g in gt_items], out=off[1:])
  flat = np.array([x for g in gt_items for x in g] + [0], dtype=np.int64)
  hits, count = kernels.hip().knn_hits(
      torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(DEV), torch.tensor(num, dtype=torch.int32, device=DEV),
      torch.from_numpy(off).to(DEV), torch.from_numpy(flat).to(DEV))
  torch.cuda.synchronize()
  return hits.cpu().numpy(), count.cpu().numpy()


def test_hits_equal_the_set_restatement(built_lib):
  U, I, K = 67, 4, 5
  rng = np.random.default_rng(9)
  ids = rng.integers(0, 60, size=(U, I, K)).astype(np.int64)  # (few values: an id recalled by several interests)
  ids[5, 1] = ids[5, 0]
  num = rng.integers(0, I + 1, size=U)
  num[:4] = [0, I, 1, I]
  gt_items = [rng.integers(0, 60, size=rng.integers(0, 9)).tolist() for _ in range(U)]
  gt_items[1] = []
  gt_items[3] = [int(ids[3, 0, 0]), int(ids[3, 0, 0]), int(ids[3, 3, 4]), 1000]  # a duplicate id, an absent one
  gt_items[5] = [int(ids[5, 0, 2])]
  gt_items[6] = rng.integers(0, 60, size=150).tolist()  # longer than a wave
  num[5] = 2
  got = run_hits(ids, num, gt_items)
  want = hits_restatement(ids, num, gt_items, I)
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
  assert want[0][3] == 2 and want[0][5] == 1 and want[0][0] == 0 and want[0].sum() > 50


@pytest.mark.parametrize('name', ['multi_m0', 'multi_m1', 'single_m1'])
def test_hits_equal_the_reference_fixture(built_lib, name):
  with open(os.path.join(HERE, 'golden', 'hit_rate_vectors.json')) as f:
    vec = json.load(f)
  for case_name in (name, 'empty_gt_' + name[-2:] if name.startswith('multi') else name):
    case = vec['cases'][case_name]
    src = vec['cases'][case['of']] if 'of' in case else case
    gt_items = case['gt_items'] if 'of' in case else [list(map(int, r[1].split(','))) for r in src['records']]
    hits, count = run_hits(np.array(src['recall_ids']), [r[3] for r in src['records']], gt_items)
    assert (float(hits.sum()), float(count.sum())) == (case['hits'], case['gt_count'])
    assert [h / c for h, c in zip(hits.tolist(), count.tolist()) if c] == case['hitrates']
  # and the whole path on the device: search + count through the accumulator
  case = vec['cases'][name]
  from easyrec_amd.tools.hit_rate import user_embeddings
  index = knn.ItemIndex(vec['item_ids'], np.array(vec['item_emb'], dtype=np.float32), case['metric'], DEV)
  acc = hit_rate_lib.HitRate(index, case['top_k'])
  rec_ids, rec_dist, _, _ = acc.update(user_embeddings([tuple(r) for r in case['records']], case['emb_dim'], case['num_interests']),
                                       [r[3] for r in case['records']], [list(map(int, r[1].split(','))) for r in case['records']])
  assert rec_ids.cpu().numpy().tolist() == case['recall_ids']
  assert rec_dist.cpu().numpy().astype(np.float64).tolist() == case['recall_distances']
  assert (acc.total_hits, acc.total_gt_count) == (case['hits'], case['gt_count'])


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('nq,n,D,K', [(QT + 1, 5000, 32, 100), (3, IT + 1, 33, 5), (QT, 4, 128, 128)])
def test_kernel_and_composition_agree_on_integer_cases(built_lib, monkeypatch, nq, n, D, K, metric):
  Q, X, ids = int_data(21, nq, n, D)
  got = run_kernel(Q, X, ids, K, metric)
  monkeypatch.setenv('EASYREC_AMD_KNN_KERNEL', '0')
  index = knn.ItemIndex(ids, X.astype(np.float32), metric, DEV)
  assert not index.uses_kernel(K)
  composed = [t.cpu().numpy() for t in index.search_rows(Q.astype(np.float32), K)]
  assert_equal(got, composed, 'kernel against composition')
