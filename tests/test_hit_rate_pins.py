"""Full-corpus hit rate on the host: batch_hitrate, the composed search, the HitRate accumulator and the command-line
tool against what the reference's own hit_rate_utils.py produced (tests/golden/make_hit_rate_vectors.py), and the LDS /
workspace formulas of er_knn_search against their Python mirrors.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from easyrec_amd.core import hit_rate as hit_rate_lib
from easyrec_amd.core import knn

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def vec():
  with open(os.path.join(HERE, 'golden', 'hit_rate_vectors.json')) as f:
    return json.load(f)


SEARCHED = ['single_m0', 'single_m1', 'multi_m0', 'multi_m1']


def _gt(case):
  return [list(map(int, r[1].split(','))) for r in case['records']]


def _user_emb(case):
  from easyrec_amd.tools.hit_rate import user_embeddings
  return user_embeddings([tuple(r) for r in case['records']], case['emb_dim'], case['num_interests'])


@pytest.mark.parametrize('name', SEARCHED + ['empty_gt_m0', 'empty_gt_m1'])
def test_batch_hitrate_equals_the_reference(vec, name):
  case = vec['cases'][name]
  src = vec['cases'][case['of']] if 'of' in case else case
  gt = case['gt_items'] if 'of' in case else _gt(case)
  mask = hit_rate_lib.interest_mask([r[3] for r in src['records']], src['num_interests'])
  got = hit_rate_lib.batch_hitrate(np.array(src['src_ids']), np.array(src['recall_ids']),
                                   np.array(src['recall_distances'], dtype=np.float32), gt, src['num_interests'], mask)
  hitrates, bad_cases, bad_dists, hits, gt_count = got
  assert hitrates == case['hitrates']
  assert [[int(x) for x in b] for b in bad_cases] == case['bad_cases']
  assert [[float(x) for x in b] for b in bad_dists] == case['bad_dists']
  assert (hits, gt_count) == (case['hits'], case['gt_count'])


@pytest.mark.parametrize('name', SEARCHED)
def test_composed_search_equals_the_reference_recall(vec, name):
  case = vec['cases'][name]
  index = knn.ItemIndex(vec['item_ids'], np.array(vec['item_emb'], dtype=np.float32), case['metric'], 'cpu')
  assert not index.uses_kernel(case['top_k'])
  user = _user_emb(case)
  ids, dist = index.search(user.reshape(-1, case['emb_dim']), case['top_k'])
  shape = (len(case['records']), case['num_interests'], case['top_k'])
  assert ids.dtype == torch.int64 and dist.dtype == torch.float32
  assert ids.numpy().reshape(shape).tolist() == case['recall_ids']
  assert dist.numpy().reshape(shape).astype(np.float64).tolist() == case['recall_distances']


def test_composed_search_pads_past_the_table():
  index = knn.ItemIndex([7, 8, 9], np.array([[1.0], [3.0], [3.0]], dtype=np.float32), knn.METRIC_IP, 'cpu')
  ids, rows, dist = index.search_rows(np.array([[2.0]], dtype=np.float32), 5)
  assert ids.tolist() == [[8, 9, 7, -1, -1]] and rows.tolist() == [[1, 2, 0, -1, -1]]
  assert dist.tolist() == [[6.0, 6.0, 2.0, float('-inf'), float('-inf')]]
  l2 = knn.ItemIndex([7, 8, 9], np.array([[1.0], [3.0], [3.0]], dtype=np.float32), knn.METRIC_L2, 'cpu')
  ids, dist = l2.search(np.array([[2.0]], dtype=np.float32), 4)
  assert ids.tolist() == [[7, 8, 9, -1]] and dist.tolist() == [[1.0, 1.0, 1.0, float('inf')]]


@pytest.mark.parametrize('name', SEARCHED)
def test_hit_rate_accumulator_on_the_cpu_backend(vec, name):
  case = vec['cases'][name]
  index = knn.ItemIndex(vec['item_ids'], np.array(vec['item_emb'], dtype=np.float32), case['metric'], 'cpu')
  acc = hit_rate_lib.HitRate(index, case['top_k'])
  gt, user, num = _gt(case), _user_emb(case), [r[3] for r in case['records']]
  half = len(gt) // 2  # two updates add up
  acc.update(user[:half], num[:half], gt[:half])
  _, _, hits, count = acc.update(user[half:], num[half:], gt[half:])
  assert (acc.total_hits, acc.total_gt_count) == (case['hits'], case['gt_count'])
  assert acc.result() == case['hits'] / case['gt_count']
  assert count.tolist() == [len(g) for g in gt[half:]]
  assert (hits.numpy() / count.numpy()).tolist() == case['hitrates'][half:]


def test_hit_rate_accumulator_skips_an_empty_list(vec):
  case, src = vec['cases']['empty_gt_m1'], vec['cases']['multi_m1']
  index = knn.ItemIndex(vec['item_ids'], np.array(vec['item_emb'], dtype=np.float32), 1, 'cpu')
  acc = hit_rate_lib.HitRate(index, src['top_k'])
  _, _, hits, count = acc.update(_user_emb(src), [r[3] for r in src['records']], case['gt_items'])
  assert (acc.total_hits, acc.total_gt_count) == (case['hits'], case['gt_count'])
  assert (hits[4].item(), count[4].item()) == (0, 0)


@pytest.mark.parametrize('name', SEARCHED)
def test_tool_end_to_end(vec, name, tmp_path):
  from easyrec_amd.tools import hit_rate as tool
  case = vec['cases'][name]
  items = tmp_path / 'items.txt'
  items.write_text(''.join('%d;%s\n' % (i, ','.join(repr(float(x)) for x in e))
                           for i, e in zip(vec['item_ids'], vec['item_emb'])))
  gt = tmp_path / 'gt.txt'
  gt.write_text(''.join('\t'.join(str(x) for x in r) + '\n' for r in case['records']))
  details, total = tmp_path / 'details.txt', tmp_path / 'total.txt'
  got = tool.main(['--item_emb_table', str(items), '--item_emb_table_field_sep', ';', '--gt_table', str(gt),
                   '--top_k', str(case['top_k']), '--knn_metric', str(case['metric']), '--emb_dim', str(case['emb_dim']),
                   '--num_interests', str(case['num_interests']), '--batch_size', '4', '--knn_strict', '--device', 'cpu',
                   '--hitrate_details_result', str(details), '--total_hitrate_result', str(total)])
  assert got == case['hits'] / case['gt_count']
  assert total.read_text() == case['total']
  assert details.read_text().split('\n') == case['detail_lines']


def test_lds_and_workspace_mirrors(built_lib):
  from easyrec_amd import kernels
  lib = kernels.load_library(built_lib)
  # the tile heights the GPU tests take their edge shapes from are the kernel's own
  assert (lib.er_knn_query_tile(), lib.er_knn_item_tile()) == (knn.QUERY_TILE, knn.ITEM_TILE)
  for D in (1, 2, 3, 31, 32, 33, 62, 64, 100, 127, 128):
    for K in (1, 5, 31, 32, 33, 100, 127, 128):
      got = lib.er_knn_lds_bytes(D, K)
      assert got == knn.lds_bytes(D, K) and 0 < got <= 160 * 1024, (D, K, got)
      assert knn.list_capacity(D, K) >= knn.ITEM_TILE + K
  for D, K in ((129, 5), (0, 5), (32, 129), (32, 0), (-1, 5), (32, -1)):
    assert lib.er_knn_lds_bytes(D, K) == 0 == knn.lds_bytes(D, K)
  for nq in (1, 31, 32, 33, 4096, 20480, 100000):
    for K in (1, 5, 128):
      for slices in (0, 1, 2, 7, 64):
        got = lib.er_knn_workspace_bytes(nq, K, slices)
        assert got == knn.workspace_bytes(nq, K, slices) and got >= 8 * nq * K, (nq, K, slices)
  assert lib.er_knn_workspace_bytes(4096, 5, 0) == 8 * 4 * 4096 * 5
  for nq, K, slices in ((0, 5, 1), (8, 129, 1), (8, 0, 1), (8, 5, -1), (8, 5, 65)):
    assert lib.er_knn_workspace_bytes(nq, K, slices) == 0 == knn.workspace_bytes(nq, K, slices)
  # n = 0 is outside the envelope of the search itself (host check, no launch)
  assert lib.er_knn_search(None, None, None, None, 1, 0, 32, 5, 1, 0, None, None, None, None, None) != 0
  assert b'n < 2^31' in lib.er_last_error()


def test_embedding_parallel_engine_refuses():
  from easyrec_amd.model.embedding_parallel import EmbeddingParallelEstimator
  with pytest.raises(NotImplementedError, match='single-GPU engine'):
    EmbeddingParallelEstimator.hit_rate(object.__new__(EmbeddingParallelEstimator), [], [], [], 5)
