"""EasyRecEstimator.hit_rate on the GPU: a DSSM and a MIND config at the sizes of tests/test_match_pins.py /
tests/test_mind_pins.py, a corpus of 256 items fed as item batches, against the same quantities computed from
est.predict's outputs by an fp64 numpy search and the host batch_hitrate.  The inputs are chosen (and checked) so that
the oracle's K-th and (K + 1)-th scores of every query differ by more than 2 eps: rounding cannot move a hit.  hit_rate
leaves the training state untouched."""
import numpy as np
import pytest
import torch

import test_match_pins
import test_mind_pins
from easyrec_amd.core import hit_rate as hit_rate_lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, ITEM_BATCHES, USER_BATCHES, TOP_K = 32, 8, 2, 10


def _cfg(kind):
  return test_match_pins.dssm_cfg(True, B) if kind == 'dssm' else test_mind_pins.mind_cfg(True, B)


def _build(kind, seed=4):
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  return EasyRecEstimator(_cfg(kind), device=DEV, batch_size=B, seed=seed).build()


def _batches(est, seed):
  """item batches whose adgroup_id column holds distinct ids (a corpus without duplicate rows), user batches"""
  from easyrec_amd.input.synthetic import SyntheticBatches
  gen = SyntheticBatches(est.pipeline_config.data_config, est.feature_configs, batch_size=B, seed=seed)
  col = est.features.schema.hash_single['adgroup_id']['col']
  items = [gen.next_batch() for _ in range(ITEM_BATCHES)]
  top = int(max(np.asarray(b['hash_ids'])[col].max() for b in items))
  assert top + 1 >= B * ITEM_BATCHES
  unique = np.random.default_rng(seed).permutation(top + 1)[:B * ITEM_BATCHES]
  for i, b in enumerate(items):
    hash_ids = np.array(b['hash_ids'])
    hash_ids[col] = unique[i * B:(i + 1) * B]
    b['hash_ids'] = hash_ids
  return items, [gen.next_batch() for _ in range(USER_BATCHES)], col


def _eval_predict(est, batch, keys):
  was = (est.model._is_training, est.ctx.is_training)
  est.model._is_training, est.ctx.is_training = False, False
  try:
    pred = est.predict(batch)
    return [pred[k].detach().double().cpu().numpy().copy() for k in keys]
  finally:
    est.model._is_training, est.ctx.is_training = was


def oracle_search(Q, X, ids, K, metric):
  """fp64 flat search -> (ids, dist, every query's (K-th to (K + 1)-th gap) / (2 eps))"""
  s = Q @ X.T
  mag = np.abs(Q) @ np.abs(X).T
  if metric == 1:
    eps, key = 1e-6 * mag, -s
  else:
    qq, xx = (Q ** 2).sum(1)[:, None], (X ** 2).sum(1)[None, :]
    s = (qq + xx) - 2.0 * s
    eps, key = 1e-6 * (qq + xx + 2.0 * mag), s
  order = np.argsort(key, axis=1, kind='stable')
  kth, nxt = order[:, K - 1], order[:, K]
  rows = np.arange(Q.shape[0])
  with np.errstate(invalid='ignore'):  # (0 / 0 for an all-zero query)
    gap = (key[rows, nxt] - key[rows, kth]) / (2.0 * np.maximum(eps[rows, kth], eps[rows, nxt]))
  return ids[order[:, :K]], np.take_along_axis(s, order[:, :K], axis=1), gap


def _oracle_hit_rate(est, kind, metric, seed):
  """-> (item batches, user batches, ground truth, hits, gt_count, the least gap / (2 eps) over the counted queries) from
  est.predict's outputs, the fp64 search and the host batch_hitrate"""
  items, users, col = _batches(est, seed)
  corpus_ids = np.concatenate([np.asarray(b['hash_ids'])[col] for b in items]).astype(np.int64)
  X = np.concatenate([_eval_predict(est, b, ['item_tower_emb'])[0][:B] for b in items])
  assert X.shape == (B * ITEM_BATCHES, 32) and len(set(corpus_ids.tolist())) == len(corpus_ids)
  rng = np.random.default_rng(7)
  want_hits = want_count = 0.0
  gt_all, least = [], np.inf
  for batch in users:
    if kind == 'mind':
      Q, num = _eval_predict(est, batch, ['user_interests', 'user_emb_num'])
    else:
      Q, num = _eval_predict(est, batch, ['user_tower_emb'])[0][:, None, :], np.ones(B)
    I = Q.shape[1]
    rec_ids, rec_dist, gap = oracle_search(Q.reshape(B * I, -1), X, corpus_ids, TOP_K, metric)
    mask = hit_rate_lib.interest_mask(num, I)
    counted = gap[mask.reshape(-1) > 0]  # (an interest that does not count is all zeros: 0 / 0)
    assert not np.isnan(counted).any(), 'a counted query has eps 0: its gap cannot be judged'
    least = min(least, float(counted.min()))
    rec_ids, rec_dist = rec_ids.reshape(B, I, TOP_K), rec_dist.reshape(B, I, TOP_K)
    # ground truth: one recalled item of the first interest for the even users, three random corpus items, one
    # duplicate, one id outside the corpus; user 3 has none
    gt = []
    for u in range(B):
      g = rng.choice(corpus_ids, size=3).tolist() + [10 ** 9]
      if u % 2 == 0:
        g += [int(rec_ids[u, 0, TOP_K - 1]), int(rec_ids[u, 0, TOP_K - 1])]
      gt.append([] if u == 3 else g)
    gt_all.append(gt)
    _, _, _, hits, count = hit_rate_lib.batch_hitrate(np.arange(B), rec_ids, rec_dist, gt, I, mask)
    want_hits += hits
    want_count += count
  return items, users, gt_all, want_hits, want_count, least


@pytest.mark.parametrize('metric', [1, 0])
@pytest.mark.parametrize('kind', ['dssm', 'mind'])
def test_hit_rate_equals_the_fp64_computation(built_lib, kind, metric):
  est = _build(kind)
  for seed in range(44, 50):  # the first seed whose inputs leave every counted query a gap of more than 2 eps
    items, users, gt_all, want_hits, want_count, gap = _oracle_hit_rate(est, kind, metric, seed)
    if gap > 1.0:
      break
  assert gap > 1.0, 'the K-th and (K + 1)-th oracle scores of a query are within 2 eps for every seed tried (%g)' % gap
  assert want_hits >= B * USER_BATCHES / 4  # (the recalled items are found: the comparison is not of zeros)
  got = est.hit_rate(items, users, gt_all, TOP_K, knn_metric=metric)
  assert (got['hits'], got['gt_count']) == (want_hits, want_count)
  assert got['hitrate'] == want_hits / want_count


@pytest.mark.parametrize('kind', ['dssm', 'mind'])
def test_hit_rate_leaves_the_training_state_untouched(built_lib, kind):
  losses = []
  for with_call in (False, True):
    torch.manual_seed(3)  # (MIND's training routing logits come from the global generator)
    est = _build(kind)
    items, users, _ = _batches(est, 45)
    est.train_step(users[0])
    if with_call:
      est.hit_rate(items, users, [[[1]] * B] * USER_BATCHES, TOP_K)
      assert est.model._is_training and est.ctx.is_training
    est.train_step(users[1])
    losses.append(dict(est.loss_values()))
  assert losses[0] == losses[1] and losses[0]

