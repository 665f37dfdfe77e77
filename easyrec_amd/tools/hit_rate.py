"""Top-K hit rate over local files: the command-line tool of reference tools/hit_rate_ds.py with its flag names, the
search done exactly on the device (core/knn.py) instead of by graphlearn's index.

  python -m easyrec_amd.tools.hit_rate --item_emb_table items.txt --gt_table gt.txt --emb_dim 32 --top_k 100 \\
      --knn_metric 1 --num_interests 4 --hitrate_details_result details.txt --total_hitrate_result total.txt

item_emb_table: rows `id<sep>v0,v1,...`.  gt_table: rows `id<sep>gt ids joined by ','<sep>user_emb, interests joined by
'|'<sep>emb_num`; an empty user_emb stands for zeros.  The details file has the reference's six tab-separated columns
(id, recalled ids, recalled distances, hitrate, bad cases, bad-case distances), the total file the single ratio.  The TF
cluster, Hive and ODPS paths of the reference are out of scope; --knn_strict is accepted and changes nothing (the search
is always exact)."""
import argparse
import glob
import os

import numpy as np
import torch

from easyrec_amd.core import hit_rate as hit_rate_lib
from easyrec_amd.core import knn


def _paths(spec):
  if os.path.isdir(spec):
    return sorted(glob.glob(os.path.join(spec, '*')))
  out = []
  for part in spec.split(','):
    out += sorted(glob.glob(part)) if '*' in part else [part]
  return out


def read_item_table(spec, sep, emb_dim):
  ids, rows = [], []
  for path in _paths(spec):
    with open(path) as fin:
      for line in fin:
        line = line.rstrip('\n')
        if not line:
          continue
        fields = line.split(sep)
        emb = np.array(fields[1].split(','), dtype=np.float32)
        assert len(emb) == emb_dim, 'item %s: %d values, --emb_dim is %d' % (fields[0], len(emb), emb_dim)
        ids.append(int(fields[0]))
        rows.append(emb)
  return np.array(ids, dtype=np.int64), np.stack(rows)


def read_gt_batches(spec, sep, batch_size):
  """reference `gt_hdfs`: lists of (id, gt string, user_emb string, emb_num)"""
  batch = []
  for path in _paths(spec):
    with open(path) as fin:
      for line in fin:
        line = line.rstrip('\n')
        if not line:
          continue
        f = line.split(sep)
        batch.append((int(f[0]), f[1], f[2], int(f[3])))
        if len(batch) >= batch_size:
          yield batch
          batch = []
  if batch:
    yield batch


def user_embeddings(records, emb_dim, num_interests):
  """reference compute_hitrate_batch `_to_multi_float_attrs` -> fp32 [U, num_interests, emb_dim]"""
  out = np.zeros((len(records), num_interests, emb_dim), dtype=np.float32)
  for u, rec in enumerate(records):
    if rec[2] == '':
      continue
    parts = rec[2].split('|')
    assert len(parts) == num_interests, 'user %s: %d interests, --num_interests is %d' % (rec[0], len(parts), num_interests)
    for h, part in enumerate(parts):
      if part == '':
        continue
      emb = np.array(part.split(','), dtype=np.float32)
      assert len(emb) == emb_dim, 'user %s: %d values in an interest, --emb_dim is %d' % (rec[0], len(emb), emb_dim)
      out[u, h] = emb
  return out


def detail_lines(src_ids, recall_ids, recall_distances, hitrates, bad_cases, bad_dists):
  """One line per user with ground truth, six tab-separated columns in the reference tool's format: the id; per interest
  the recalled ids as numpy prints an integer row (`[a b c]`), interests joined by ','; per interest the distances joined
  by '|', interests joined by ','; the hit rate; the bad cases and their distances, each joined by ','."""
  lines = []
  for u, src in enumerate(src_ids):
    columns = (
        str(src),
        ','.join(str(row) for row in recall_ids[u]),
        ','.join('|'.join(str(d) for d in row) for row in recall_distances[u]),
        str(hitrates[u]),
        ','.join(str(x) for x in bad_cases[u]),
        ','.join(str(x) for x in bad_dists[u]),
    )
    lines.append('\t'.join(columns))
  return lines


def run(args):
  device = args.device or ('cuda:0' if torch.cuda.is_available() else 'cpu')
  ids, emb = read_item_table(args.item_emb_table, args.item_emb_table_field_sep, args.emb_dim)
  acc = hit_rate_lib.HitRate(knn.ItemIndex(ids, emb, args.knn_metric, device), args.top_k)
  lines = []
  for records in read_gt_batches(args.gt_table, args.gt_table_field_sep, args.batch_size):
    src_ids = np.array([r[0] for r in records])
    gt_items = [list(map(int, r[1].split(','))) if r[1] != '' else [] for r in records]
    emb_num = np.array([r[3] for r in records], dtype=np.int32)
    user_emb = user_embeddings(records, args.emb_dim, args.num_interests)
    rec_ids, rec_dist, _, _ = acc.update(user_emb, emb_num, gt_items)
    rec_ids, rec_dist = rec_ids.cpu().numpy(), rec_dist.cpu().numpy()
    # the per-user columns come from the host restatement; users without ground truth have no line
    keep = [u for u, g in enumerate(gt_items) if len(g)]
    hitrates, bad_cases, bad_dists, _, _ = hit_rate_lib.batch_hitrate(
        src_ids, rec_ids, rec_dist, gt_items, args.num_interests, hit_rate_lib.interest_mask(emb_num, args.num_interests))
    lines += detail_lines(src_ids[keep], rec_ids[keep], rec_dist[keep], hitrates, bad_cases, bad_dists)
  if args.hitrate_details_result:
    with open(args.hitrate_details_result, 'w') as fout:
      fout.write('\n'.join(lines))
  total = acc.result()
  if args.total_hitrate_result:
    with open(args.total_hitrate_result, 'w') as fout:
      fout.write(str(np.float32(total)))
  print('total_hits: ', float(acc.total_hits))
  print('total_gt_count: ', float(acc.total_gt_count))
  return total


def _bool(v):
  return str(v).lower() in ('1', 'true', 'yes')


def main(argv=None):
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--item_emb_table', required=True, help='item embedding table: a file, a directory, a glob or a list')
  p.add_argument('--gt_table', required=True, help='ground truth table')
  p.add_argument('--hitrate_details_result', default='', help='hitrate detail file path')
  p.add_argument('--total_hitrate_result', default='', help='total hitrate result file path')
  p.add_argument('--batch_size', type=int, default=512)
  p.add_argument('--emb_dim', type=int, default=128)
  p.add_argument('--top_k', type=int, default=5)
  p.add_argument('--knn_metric', type=int, default=0, help='0(l2) or 1(ip).')
  p.add_argument('--knn_strict', type=_bool, nargs='?', const=True, default=False, help='accepted; the search is exact')
  p.add_argument('--num_interests', type=int, default=1, help='max number of interests')
  p.add_argument('--gt_table_field_sep', default='\t')
  p.add_argument('--item_emb_table_field_sep', default='\t')
  p.add_argument('--device', default='', help="torch device (default: cuda:0 when there is one, else cpu)")
  return run(p.parse_args(argv))


if __name__ == '__main__':
  main()
