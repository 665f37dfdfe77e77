"""Exact top-K item search over a whole corpus: the step the reference's hit-rate tool hands to graphlearn's KNN index
(tools/hit_rate_ds.py, utils/hit_rate_utils.py:204 `g.search`).

ItemIndex keeps the item embeddings and ids on the device and searches them with er_knn_search (csrc/er_knn.hip; the
semantics are stated in include/easyrec_hip.h K9k): fp32 fmaf-chain scores, inner product (metric 1, larger is better)
or squared L2 (metric 0, smaller is better), a strict total order on (score, row) and the first min(K, n) rows of it.
Outside the kernel's envelope, on a CPU backend and with EASYREC_AMD_KNN_KERNEL=0 the same semantics are composed of
torch operations (`search_composed`): chunked matmul, topk, merge, ties resolved by row.  The composition's scores are
torch's matmul, which need not round as the fmaf chain does: the two agree bit for bit where every chain is exact
(small integers), and within rounding elsewhere."""
import os

import numpy as np
import torch

from easyrec_amd import kernels

QUERY_TILE = 32    # queries of a workgroup (kKnnQT)
ITEM_TILE = 128    # item rows of a tile (kKnnIT)
MAX_D = 128
MAX_K = 128
MAX_SLICES = 64
METRIC_L2, METRIC_IP = 0, 1
_BUDGET = 152 * 1024


def knn_kernel_enabled():
  return os.environ.get('EASYREC_AMD_KNN_KERNEL', '1') != '0'


def pitch(D):
  """the LDS row pitch in floats: even, >= D, pitch / 2 odd"""
  p = (D + 1) & ~1
  return p + 2 if (p // 2) % 2 == 0 else p


def list_capacity(D, K):
  fixed = 4 * (QUERY_TILE + ITEM_TILE) * pitch(D) + 4 * ITEM_TILE + 8 * QUERY_TILE
  return min(ITEM_TILE + max(2 * K, 64), (_BUDGET - fixed) // (8 * QUERY_TILE), 384)


def lds_bytes(D, K):
  """er_knn_lds_bytes: both operand tiles, the tile's xx, thresholds, counters and 32 candidate lists; 0 outside the
  envelope."""
  if D < 1 or D > MAX_D or K < 1 or K > MAX_K:
    return 0
  return 4 * (QUERY_TILE + ITEM_TILE) * pitch(D) + 4 * ITEM_TILE + 8 * QUERY_TILE + 8 * QUERY_TILE * list_capacity(D, K)


def auto_slices(nq, n=None):
  """the slice count er_knn_search picks with slices = 0 (n = None: the most it picks for nq, whatever n is)"""
  s = -(-512 // -(-nq // QUERY_TILE))
  if n is not None:
    s = min(s, n // (16 * ITEM_TILE))
  return max(1, min(s, MAX_SLICES))


def workspace_bytes(nq, K, slices=0):
  """er_knn_workspace_bytes: the [S, nq, K] partial lists of 8-byte keys; 0 outside the envelope."""
  if nq < 1 or K < 1 or K > MAX_K or slices < 0 or slices > MAX_SLICES:
    return 0
  return 8 * (slices or auto_slices(nq)) * nq * K


def search_composed(queries, items, xx, table_ids, K, metric, chunk=1 << 16):
  """The semantics of er_knn_search composed of torch operations -> (ids int64, rows int32, dist fp32), each [nq, K]."""
  nq, n = queries.shape[0], items.shape[0]
  dev = queries.device
  queries = queries.float()
  chunk = max(K + 1, min(chunk, (1 << 28) // nq))  # (at most 1 GiB of scores at a time)
  best_v = best_r = None
  qq = (queries * queries).sum(dim=1, keepdim=True) if metric == METRIC_L2 else None
  for c0 in range(0, n, chunk):
    blk = items[c0:c0 + chunk]
    s = queries @ blk.t()
    if metric == METRIC_L2:
      s = torch.clamp((qq + xx[c0:c0 + chunk].unsqueeze(0)) - 2.0 * s, min=0.0)
    s = s + 0.0  # (-0 -> +0, as the kernel reports it)
    rows = torch.arange(c0, c0 + blk.shape[0], device=dev, dtype=torch.int64).unsqueeze(0).expand(nq, -1)
    if s.shape[1] > K:
      # topk gives the K-th score t; the chunk's K are the scores better than t and the lowest rows among those equal
      # to t (topk itself breaks ties in no stated order); nonzero lists them in ascending row
      t = torch.topk(s, K, dim=1, largest=(metric == METRIC_IP)).values[:, K - 1:K]
      better = s > t if metric == METRIC_IP else s < t
      ties = s == t
      room = K - better.sum(dim=1, keepdim=True)
      keep = better | (ties & (torch.cumsum(ties, dim=1) <= room))
      cols = torch.nonzero(keep)[:, 1].view(nq, K)
      s, rows = torch.gather(s, 1, cols), torch.gather(rows, 1, cols)
    if best_v is not None:
      s, rows = torch.cat([best_v, s], dim=1), torch.cat([best_r, rows], dim=1)
    # rows are ascending among equal scores (the kept list holds earlier rows): one stable sort gives the total order
    order = torch.sort(s, dim=1, descending=(metric == METRIC_IP), stable=True).indices[:, :K]
    best_v, best_r = torch.gather(s, 1, order), torch.gather(rows, 1, order)
  k = best_v.shape[1]
  ids = torch.full((nq, K), -1, dtype=torch.int64, device=dev)
  out_rows = torch.full((nq, K), -1, dtype=torch.int32, device=dev)
  dist = torch.full((nq, K), float('-inf') if metric == METRIC_IP else float('inf'), dtype=torch.float32, device=dev)
  ids[:, :k] = table_ids[best_r]
  out_rows[:, :k] = best_r.to(torch.int32)
  dist[:, :k] = best_v
  return ids, out_rows, dist


class ItemIndex(object):
  """The item corpus of a retrieval model, resident on `device`: item_ids int64 [n] and item_emb fp32 [n, D]."""

  def __init__(self, item_ids, item_emb, metric=METRIC_IP, device='cuda:0'):
    if metric not in (METRIC_L2, METRIC_IP):
      raise ValueError('ItemIndex: knn_metric %r (0: l2, 1: inner product)' % (metric,))
    self.device = torch.device(device)
    self.metric = int(metric)
    self.item_ids = torch.as_tensor(np.asarray(item_ids, dtype=np.int64) if not torch.is_tensor(item_ids) else item_ids,
                                    dtype=torch.int64).to(self.device).contiguous()
    emb = item_emb if torch.is_tensor(item_emb) else torch.from_numpy(np.ascontiguousarray(item_emb, dtype=np.float32))
    self.item_emb = emb.detach().to(self.device, torch.float32).contiguous()
    self.n, self.D = self.item_emb.shape
    if self.item_ids.shape != (self.n,) or self.n < 1:
      raise ValueError('ItemIndex: %d ids for %d embeddings' % (self.item_ids.numel(), self.n))
    self.xx = None
    if self.metric == METRIC_L2:
      if self._kernel_device() and 1 <= self.D <= MAX_D and self.n < 2 ** 31:
        self.xx = kernels.hip().knn_norms(self.item_emb)
      else:
        self.xx = (self.item_emb * self.item_emb).sum(dim=1)

  def _kernel_device(self):
    return self.device.type == 'cuda' and isinstance(kernels.hip(), kernels.HipBackend)

  def uses_kernel(self, k, slices=0):
    return (knn_kernel_enabled() and self._kernel_device() and lds_bytes(self.D, k) > 0 and self.n < 2 ** 31 and
            0 <= slices <= MAX_SLICES)

  def search_rows(self, queries, k, slices=0):
    """queries [nq, D] -> (ids int64 [nq, k], rows int32 [nq, k], dist fp32 [nq, k])"""
    queries = torch.as_tensor(queries, dtype=torch.float32).to(self.device).contiguous()
    if queries.dim() != 2 or queries.shape[1] != self.D or queries.shape[0] < 1 or k < 1:
      raise ValueError('ItemIndex.search: queries %s for an index of width %d, k %d' % (tuple(queries.shape), self.D, k))
    if self.uses_kernel(k, slices):
      return kernels.hip().knn_search(queries, self.item_emb, self.xx, self.item_ids, k, self.metric, slices)
    return search_composed(queries, self.item_emb, self.xx, self.item_ids, k, self.metric)

  def search(self, queries, k, slices=0):
    """-> (ids int64 [nq, k], dist fp32 [nq, k]): the first min(k, n) rows of every query in the total order, places past
    n with id -1 and distance -inf (inner product) / +inf (l2)."""
    ids, _, dist = self.search_rows(queries, k, slices)
    return ids, dist
