#!/usr/bin/env python
"""Golden vectors from the REFERENCE'S OWN hit-rate functions (utils/hit_rate_utils.py `batch_hitrate`,
`compute_hitrate_batch`), run where a checkout of the reference is available.

hit_rate_utils.py imports graphlearn and tensorflow; both get stand-in modules here.  Of tensorflow only `__version__`
is touched by the two functions.  Of graphlearn they use `g.search('i', vectors, gl.KnnOption(k=top_k))`: the stand-in is
an exact flat search in numpy under the order this project states (include/easyrec_hip.h K9k): inner product (metric 1,
larger first) or squared L2 max(0, (qq + xx) - 2 s) (metric 0, smaller first), ties by the lower row.  Embeddings are
multiples of 1/2 in [-1.5, 1.5], so every fp32 sum is exact and ties are plentiful.  The two functions then run
unmodified; inputs and every output go to tests/golden/hit_rate_vectors.json.

Cases, each under both metrics:
  single   one interest per user
  multi    4 interests, user_emb_num 0, 1, 3, 4, .. ; a ground-truth list with a duplicate id; a user whose interests
           0 and 1 are the same vector (its items are recalled twice); a user with an empty user_emb string
  empty_gt batch_hitrate alone on `multi`'s recall with one user's ground-truth list emptied (compute_hitrate_batch
           cannot parse an empty list: int('') raises)
The detail lines come from the reference too: tools/hit_rate_ds.py imports the TF cluster stack and cannot be loaded, so
the statements of its `compute_hitrate` that format a batch are taken from the checkout's syntax tree and executed on
the arrays above (`detail_lines`), and the interest mask of the empty_gt cases is hit_rate_utils.py's own `_make_mask`
(`reference_mask`).  No statement of the reference is written out in this file.

usage: python tests/golden/make_hit_rate_vectors.py [<reference checkout>]   (default: make_reference_layer_vectors.REF)
"""
import ast
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_ITEMS, D, TOP_K = 40, 4, 5


class FlatIndex(object):
  """the stand-in for a graphlearn graph with a KNN index on node type 'i'"""

  def __init__(self, ids, emb, metric):
    self.ids, self.emb, self.metric = ids, emb.astype(np.float32), metric

  def search(self, node_type, vectors, option):
    assert node_type == 'i'
    q = np.asarray(vectors, dtype=np.float32)
    s = (q[:, None, :].astype(np.float64) * self.emb[None, :, :]).sum(-1)  # (exact: multiples of 1/4)
    if self.metric == 0:
      qq = (q.astype(np.float64) ** 2).sum(-1)[:, None]
      xx = (self.emb.astype(np.float64) ** 2).sum(-1)[None, :]
      s = np.maximum(0.0, (qq + xx) - 2.0 * s)
    s = s + 0.0
    rows = np.arange(self.emb.shape[0])
    out_ids, out_dist = [], []
    for r in range(q.shape[0]):
      order = np.lexsort((rows, -s[r] if self.metric == 1 else s[r]))[:option.k]
      out_ids.append(self.ids[order])
      out_dist.append(s[r][order].astype(np.float32))
    return np.array(out_ids), np.array(out_dist)


def load_reference(ref):
  tf = types.ModuleType('tensorflow')
  tf.__version__ = '1.15.0'
  gl = types.ModuleType('graphlearn')
  gl.KnnOption = lambda k: types.SimpleNamespace(k=k)
  sys.modules['tensorflow'], sys.modules['graphlearn'] = tf, gl
  path = os.path.join(ref, 'easy_rec', 'python', 'utils', 'hit_rate_utils.py')
  spec = importlib.util.spec_from_file_location('ref_hit_rate_utils', path)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def emb_str(v):
  return ','.join(repr(float(x)) for x in v)


def _function(path, name):
  """the ast of top-level function `name` in the reference file at `path`"""
  with open(path) as f:
    tree = ast.parse(f.read(), path)
  return next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name), path


def _run(stmts, path, namespace):
  exec(compile(ast.Module(body=list(stmts), type_ignores=[]), path, 'exec'), namespace)
  return namespace


class _Writer(object):
  def __init__(self):
    self.text = ''

  def write(self, text):
    self.text += text


def detail_lines(ref, src_ids, recall_ids, recall_distances, hitrates, bad_cases, bad_dists):
  """The statements of the reference's tools/hit_rate_ds.py `compute_hitrate` that turn one batch's results into the
  details file's text - everything in its loop body after the compute_hitrate_batch call and the two running totals -
  taken from the checkout's syntax tree and executed on these arrays with a writer that keeps the text.  (The file itself
  cannot be imported: it pulls in the TF cluster stack.)"""
  fn, path = _function(os.path.join(ref, 'easy_rec', 'python', 'tools', 'hit_rate_ds.py'), 'compute_hitrate')
  loop = next(n for n in fn.body if isinstance(n, ast.For))
  uses_writer = [i for i, n in enumerate(loop.body) if any(isinstance(x, ast.Name) and x.id == 'hitrate_writer'
                                                            for x in ast.walk(n))]
  first = max(i for i, n in enumerate(loop.body) if isinstance(n, ast.AugAssign)) + 1  # (after the running totals)
  writer = _Writer()
  _run(loop.body[first:uses_writer[-1] + 1], path,
       dict(src_ids=src_ids, recall_ids=recall_ids, recall_distances=recall_distances, hitrates=hitrates,
            bad_cases=bad_cases, bad_dists=bad_dists, hitrate_writer=writer))
  return writer.text.split('\n')


def reference_mask(ref, user_emb_num, num_interests):
  """the reference's own `_make_mask` (nested in hit_rate_utils.py compute_hitrate_batch), taken from the checkout"""
  fn, path = _function(os.path.join(ref, 'easy_rec', 'python', 'utils', 'hit_rate_utils.py'), 'compute_hitrate_batch')
  make_mask = next(n for n in fn.body if isinstance(n, ast.FunctionDef) and n.name == '_make_mask')
  return _run([make_mask], path, dict(np=np, num_interests=num_interests))['_make_mask'](user_emb_num)


def make_case(ref_dir, ref, rng, item_ids, item_emb, metric, num_interests, emb_nums, specials):
  g = FlatIndex(item_ids, item_emb, metric)
  U = len(emb_nums)
  user = rng.integers(-3, 4, size=(U, num_interests, D)).astype(np.float32) / 2
  if specials:
    user[2, 1] = user[2, 0]  # one item recalled by two interests
  first = g.search('i', user.reshape(-1, D), types.SimpleNamespace(k=TOP_K))[0].reshape(U, num_interests, TOP_K)
  records = []
  for u in range(U):
    gt = [int(first[u, 0, 0]), int(first[u, num_interests - 1, 1])] + [int(x) for x in rng.choice(item_ids, size=2)]
    if specials and u == 1:
      gt = gt + [gt[0]]  # a duplicate id
    if specials and u == 2:
      gt = [int(first[u, 0, 0]), int(first[u, 0, 2])]
    ustr = '|'.join(emb_str(v) for v in user[u])
    if specials and u == 3:
      ustr = ''  # user embedding not present: zeros
    records.append((1000 + u, ','.join(str(x) for x in gt), ustr, int(emb_nums[u])))
  hits, gt_count, src_ids, rec_ids, rec_dist, hitrates, bad_cases, bad_dists = ref.compute_hitrate_batch(
      g, records, D, num_interests, TOP_K)
  case = dict(
      metric=metric, num_interests=num_interests, top_k=TOP_K, emb_dim=D,
      records=[list(r) for r in records], hits=float(hits), gt_count=float(gt_count),
      src_ids=[int(x) for x in src_ids], recall_ids=np.asarray(rec_ids).tolist(),
      recall_distances=np.asarray(rec_dist, dtype=np.float64).tolist(), hitrates=[float(h) for h in hitrates],
      bad_cases=[[int(x) for x in b] for b in bad_cases], bad_dists=[[float(x) for x in b] for b in bad_dists],
      detail_lines=detail_lines(ref_dir, src_ids, rec_ids, rec_dist, hitrates, bad_cases, bad_dists),
      total=str(np.float32(hits / gt_count)))
  return case, (src_ids, rec_ids, rec_dist, records)


def main():
  if len(sys.argv) > 1:
    ref = sys.argv[1]
  else:
    sys.path.insert(0, HERE)
    import make_reference_layer_vectors as mrl
    ref = mrl.REF
  mod = load_reference(ref)
  rng = np.random.default_rng(20261019)
  item_ids = rng.permutation(np.arange(500, 500 + N_ITEMS)).astype(np.int64)
  item_emb = rng.integers(-3, 4, size=(N_ITEMS, D)).astype(np.float32) / 2
  out = dict(item_ids=item_ids.tolist(), item_emb=item_emb.tolist(), cases={})
  for metric in (0, 1):
    case, _ = make_case(ref, mod, rng, item_ids, item_emb, metric, 1, [1, 1, 1, 1, 1], False)
    out['cases']['single_m%d' % metric] = case
    case, (src_ids, rec_ids, rec_dist, records) = make_case(ref, mod, rng, item_ids, item_emb, metric, 4,
                                                            [0, 1, 3, 4, 4, 2], True)
    out['cases']['multi_m%d' % metric] = case
    gt_items = [list(map(int, r[1].split(','))) for r in records]
    gt_items[4] = []
    mask = reference_mask(ref, [r[3] for r in records], 4)
    hitrates, bad_cases, bad_dists, hits, gt_count = mod.batch_hitrate(src_ids, rec_ids, rec_dist, gt_items, 4, mask)
    out['cases']['empty_gt_m%d' % metric] = dict(
        of='multi_m%d' % metric, gt_items=gt_items, hits=float(hits), gt_count=float(gt_count),
        hitrates=[float(h) for h in hitrates], bad_cases=[[int(x) for x in b] for b in bad_cases],
        bad_dists=[[float(x) for x in b] for b in bad_dists])
  with open(os.path.join(HERE, 'hit_rate_vectors.json'), 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
  print('wrote hit_rate_vectors.json: %s' % sorted(out['cases']))


if __name__ == '__main__':
  main()
