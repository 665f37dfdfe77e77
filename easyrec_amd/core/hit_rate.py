"""Full-corpus hit rate (reference utils/hit_rate_utils.py, tools/hit_rate_ds.py): the top K items of the whole corpus
are searched for every user vector - for every valid interest of a multi-interest model - and the user's ground-truth
items found among them are counted: hitrate = hits / gt_count.

batch_hitrate is the host restatement of the reference's function, bad cases included.  HitRate is the accumulator the
estimator and the command-line tool use: search (core/knn.py) and count (er_knn_hits, include/easyrec_hip.h K9k) on the
device, one small read-back of two totals per update."""
import numpy as np
import torch

from easyrec_amd import kernels
from easyrec_amd.core import knn


def batch_hitrate(src_ids, recall_ids, recall_distances, gt_items, num_interests, mask=None):
  """reference hit_rate_utils.py:37-94.  recall_ids / recall_distances [U, num_interests, K], gt_items: a list of U
  lists, mask [U, num_interests] (None: every interest counts) -> (hitrates, bad_cases, bad_dists, hits, gt_count).
  A user with an empty ground-truth list is skipped: the three lists have no entry for it.  A recalled id outside the
  ground truth is a bad case, kept with the SMALLER of its distances whatever the metric, as the reference keeps it."""
  hitrates, bad_cases, bad_dists = [], [], []
  hits = gt_count = 0.0
  for idx in range(len(src_ids)):
    gt = gt_items[idx]
    if len(gt) == 0:
      continue
    hit_ids, bad = [], {}
    for h in range(num_interests):
      if mask is not None and not mask[idx, h]:
        continue
      for k, rid in enumerate(recall_ids[idx][h]):
        if rid in gt:
          if rid not in hit_ids:
            hit_ids.append(rid)
        else:
          dis = recall_distances[idx][h][k]
          if rid not in bad or dis < bad[rid]:
            bad[rid] = dis
    hitrates.append(float(len(hit_ids)) / len(gt))
    hits += float(len(hit_ids))
    gt_count += len(gt)
    bad_cases.append(list(bad))
    bad_dists.append([bad[x] for x in bad])
  return hitrates, bad_cases, bad_dists, hits, gt_count


def interest_mask(user_emb_num, num_interests):
  """reference compute_hitrate_batch `_make_mask`: interest h of user u counts iff h < user_emb_num[u]"""
  n = np.asarray(user_emb_num).astype(np.int64).reshape(-1, 1)
  return (np.arange(num_interests).reshape(1, -1) < n).astype(np.float32)


def count_hits(ids, user_emb_num, gt_offsets, gt_ids):
  """er_knn_hits, or on a CPU backend the same rule on the host -> (hits, gt_count) int32 [U] tensors on ids' device"""
  if ids.device.type == 'cuda' and isinstance(kernels.hip(), kernels.HipBackend):
    return kernels.hip().knn_hits(ids, user_emb_num, gt_offsets, gt_ids)
  U, I, _ = ids.shape
  ids_h, num_h, off_h, gt_h = ids.numpy(), user_emb_num.numpy(), gt_offsets.numpy(), gt_ids.numpy()
  hits, count = np.zeros(U, dtype=np.int32), np.zeros(U, dtype=np.int32)
  for u in range(U):
    gt = gt_h[off_h[u]:off_h[u + 1]]
    seen = set(ids_h[u, :max(0, min(int(num_h[u]), I))].reshape(-1).tolist())
    hits[u] = len(set(gt.tolist()) & seen)
    count[u] = gt.size
  return torch.from_numpy(hits), torch.from_numpy(count)


class HitRate(object):
  """hits / gt_count over every update(): `index` an ItemIndex, top_k the number of items recalled per interest."""

  def __init__(self, index, top_k):
    self.index = index
    self.top_k = int(top_k)
    self.total_hits = 0
    self.total_gt_count = 0

  def update(self, user_emb, user_emb_num, gt_items, slices=0):
    """user_emb [U, I, D] (or [U, D]: one interest), user_emb_num [U] or None (every interest counts), gt_items: a list
    of U lists of item ids -> (ids [U, I, K], dist [U, I, K], hits [U], gt_count [U]) of this batch, on the device."""
    dev = self.index.device
    user_emb = torch.as_tensor(user_emb, dtype=torch.float32).to(dev)
    if user_emb.dim() == 2:
      user_emb = user_emb.unsqueeze(1)
    U, I, D = user_emb.shape
    if len(gt_items) != U:
      raise ValueError('HitRate.update: %d ground-truth lists for %d users' % (len(gt_items), U))
    if user_emb_num is None:
      num = torch.full((U,), I, dtype=torch.int32, device=dev)
    else:
      num = torch.as_tensor(user_emb_num).to(dev, torch.int32).contiguous()
    lens = np.array([len(g) for g in gt_items], dtype=np.int64)
    offsets = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    flat = np.array([x for g in gt_items for x in g], dtype=np.int64)
    ids, dist = self.index.search(user_emb.reshape(U * I, D), self.top_k, slices)
    ids, dist = ids.view(U, I, self.top_k), dist.view(U, I, self.top_k)
    # (one spare element: an all-empty batch still hands the kernel a buffer)
    gt_dev = torch.from_numpy(np.concatenate([flat, np.zeros(1, dtype=np.int64)])).to(dev)
    hits, count = count_hits(ids, num, torch.from_numpy(offsets).to(dev), gt_dev)
    totals = torch.stack([hits.sum(), count.sum()]).tolist()
    self.total_hits += int(totals[0])
    self.total_gt_count += int(totals[1])
    return ids, dist, hits, count

  def result(self):
    return self.total_hits / self.total_gt_count if self.total_gt_count else 0.0
