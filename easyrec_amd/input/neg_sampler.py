"""negative_sampler_in_memory (reference core/sampler.py:321-472 `NegativeSamplerInMemory`, input/input.py:823-845): every
step N rows of an item table, uniform without replacement and none of them an item of the batch, are appended to the
batch's attribute columns, so the item tower sees B + N rows.

The reference draws on the host in a tf.py_func.  Here the table is resident in HBM (converted once, at load, by the
code path the batch's own values take) and the draw is one launch inside the captured step, keyed by the device step
counter (csrc/er_sampler.hip; the semantics are stated in include/easyrec_hip.h K1b).  Outside the kernel's envelope and
on a CPU backend the same draw is composed here of numpy / torch operations (`draw`); EASYREC_AMD_DEVICE_SAMPLER=0 selects
the composition on a GPU as well.  The composition reads the step counter and the batch's ids back to the host, so it
cannot be captured into a hipGraph.

The exclusion compares ids as the embedding of `item_id_field` sees them: two raw ids that share a hash bucket count as
the same item.  The reference's np.random stream cannot be reproduced; the two agree in distribution.

negative_sampler (reference core/sampler.py:261-318 `NegativeSampler`) is the same producer with another draw: N rows in
proportion to a per-item weight (the `weight` column of the table file), with replacement, none of them an item of the
batch.  The reference hands that draw to graphlearn; here it is Vose's alias table, built once on the host
(`alias_table`), and one launch per step (easyrec_hip.h K1c; `draw_weighted` composes the same draw).  Agreement with the
reference is in distribution only.  An estimator built with is_training=False draws num_eval_sample rows when that is
set (the reference's evaluator: set_eval_num_sample)."""
import os
from collections import OrderedDict

import numpy as np
import torch

from easyrec_amd import kernels
from easyrec_amd.input.features import feature_name_of
from easyrec_amd.protos.feature_config_pb2 import FeatureConfig

MAX_B = 4096
device_sampler = os.environ.get('EASYREC_AMD_DEVICE_SAMPLER', '1') != '0'
SYNTHETIC = 'synthetic://'
_U = np.uint64


def lds_bytes(B):
  """er_neg_sample_lds_bytes: the batch ids as an open-addressing set of capacity max(64, 2^c >= 2 B) and the 16 wave
  counts; 0 outside the envelope."""
  return 8 * set_capacity(B) + 128 if 1 <= B <= MAX_B else 0


def set_capacity(B):
  """slots of the batch-id set in LDS: max(64, the power of two >= 2 B)"""
  cap = 64
  while cap < 2 * B:
    cap *= 2
  return cap


# ------------------------------------------------------------------------------------------------ the draw, composed
def mix64(x):
  """the splitmix64 finaliser on a uint64 array"""
  x = np.asarray(x, dtype=_U).copy()
  x ^= x >> _U(30)
  x *= _U(0xBF58476D1CE4E5B9)
  x ^= x >> _U(27)
  x *= _U(0x94D049BB133111EB)
  x ^= x >> _U(31)
  return x


def _keys(seed, step, n):
  bits = max(2, int(n - 1).bit_length())
  h = (bits + 1) // 2
  base = mix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=_U) ^ mix64(np.array([int(step) & 0xFFFFFFFFFFFFFFFF], dtype=_U)))
  keys = mix64(base + np.arange(4, dtype=_U) * _U(0xD1B54A32D192ED03))
  return keys, _U(h), _U((1 << h) - 1)


def perm(seed, step, n, count):
  """P(0), .., P(count - 1) of the step's permutation of [0, n) -> int64 [count]"""
  keys, h, mask = _keys(seed, step, n)
  x = np.arange(count, dtype=_U)
  todo = np.arange(count)
  while todo.size:
    v = x[todo]
    L, R = v >> h, v & mask
    for r in range(4):
      L, R = R, L ^ (mix64(keys[r] ^ R) & mask)
    v = (L << h) | R
    x[todo] = v
    todo = todo[v >= _U(n)]
  return x.astype(np.int64)


def draw(seed, step, table_ids, batch_ids, N):
  """sel int64 [N]: the first N candidates P(k), k = 0 .. B + N - 1, whose id is not in the batch (numpy arrays)."""
  table_ids, batch_ids = np.asarray(table_ids, dtype=np.int64), np.asarray(batch_ids, dtype=np.int64)
  n, B = table_ids.size, batch_ids.size
  assert N >= 1 and B + N <= n
  cand = perm(seed, step, n, B + N)
  kept = cand[~np.isin(table_ids[cand], batch_ids)][:N]
  if kept.size < N:  # (only a table with duplicate ids: the kernel's rule)
    kept = np.concatenate([kept, np.zeros(N - kept.size, dtype=np.int64)])
  return kept


# ------------------------------------------------------------------------------------------------ the weighted draw
def wlds_bytes(B):
  """er_neg_sample_weighted_lds_bytes: the batch-id set and its empty-mark flag; 0 outside the envelope."""
  return 8 * set_capacity(B) + 16 if 1 <= B <= MAX_B else 0


def check_weights(weights):
  """-> fp64 [n]; negative or non-finite weights and a zero total are refused"""
  w = np.ascontiguousarray(weights, dtype=np.float64)
  if w.ndim != 1 or not np.isfinite(w).all() or (w < 0).any():
    raise ValueError('item table: weights must be finite and non-negative, one per row')
  if w.size and not w.sum() > 0:
    raise ValueError('item table: the weights sum to zero')
  return w


def alias_table(weights):
  """Vose's alias table of `weights` [n] -> uint64 [n] records, low 32 bits the fp32 bits of prob[k], high 32 bits
  alias[k] (easyrec_hip.h K1c).  fp64 arithmetic, prob rounded to fp32 once at the end.  Vose's pairing - a row below the
  mean is topped up by the current row above it, and a row that drops below the mean by giving is topped up by the
  next - written with cumulative sums instead of its two work lists, so that a 10 M-row table builds in numpy:
  with D the running deficit of the small rows and E the running excess of the large ones, small row i is topped up
  by the large row whose excess interval holds D_(i-1), and large row l, overdrawn by the small row that carries D past
  E_l, keeps 1 minus the overdraft and is topped up by large row l + 1.  Equal weights whose w * (n / sum w) all round
  just below 1 leave no large row: nothing is owed beyond rounding, and every row keeps prob 1 and itself as alias."""
  w = check_weights(weights)
  n = w.size
  p = w * (n / w.sum())
  prob, alias = np.ones(n), np.arange(n, dtype=np.int64)
  small, large = np.nonzero(p < 1.0)[0], np.nonzero(p >= 1.0)[0]
  if small.size and large.size:
    deficit = 1.0 - p[small]
    D, E = np.cumsum(deficit), np.cumsum(p[large] - 1.0)
    D_before = D - deficit
    last = large.size - 1
    prob[small] = p[small]
    alias[small] = large[np.minimum(np.searchsorted(E, D_before, side='right'), last)]
    first_past = np.searchsorted(D, E[:last], side='right')  # per large row but the last: the small row that carries D past E_l
    ok = first_past < small.size
    at = np.minimum(first_past, small.size - 1)
    overdrawn = ok & (D_before[at] < E[:last])  # (== : the small row before it ended exactly at E_l, nothing is owed)
    rows = large[:last][overdrawn]
    prob[rows] = np.clip(1.0 - (D[at][overdrawn] - E[:last][overdrawn]), 0.0, 1.0)
    alias[rows] = large[1:][overdrawn]
  bits = prob.astype(np.float32).view(np.uint32).astype(_U)
  return (alias.astype(_U) << _U(32)) | bits


def _candidates(base, tab, j, a):
  """the candidate rows of draws `j` at attempts `a` (uint64 arrays)"""
  n = _U(tab.size)
  r0 = mix64(base ^ mix64((j << _U(32)) | a))
  r1 = mix64(r0 + _U(0xD1B54A32D192ED03))
  hi, lo = r0 >> _U(32), r0 & _U(0xFFFFFFFF)
  k = (hi * n + ((lo * n) >> _U(32))) >> _U(32)
  f = (r1 >> _U(40)).astype(np.float32) * np.float32(2.0 ** -24)
  rec = tab[k.astype(np.int64)]
  prob = (rec & _U(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
  alias = rec >> _U(32)
  return np.where(f < prob, k, np.where(alias < n, alias, k)).astype(np.int64)


ATTEMPTS = 32


def draw_weighted(seed, step, alias_tab, table_ids, batch_ids, N):
  """sel int64 [N] of easyrec_hip.h K1c: per draw the first of 32 candidates whose id is not in the batch, else the next
  eligible row after the last candidate (numpy arrays; like `draw` it runs on the host and cannot be captured)."""
  tab = np.asarray(alias_tab, dtype=_U)
  table_ids, batch_ids = np.asarray(table_ids, dtype=np.int64), np.asarray(batch_ids, dtype=np.int64)
  n, B = table_ids.size, batch_ids.size
  assert tab.size == n and N >= 1 and B + N <= n
  with np.errstate(over='ignore'):
    base = mix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=_U) ^ mix64(np.array([int(step) & 0xFFFFFFFFFFFFFFFF], dtype=_U)))
    row = _candidates(base, tab, np.arange(N, dtype=_U), _U(0))
    todo = np.nonzero(np.isin(table_ids[row], batch_ids))[0]
    for a in range(1, ATTEMPTS):
      if not todo.size:
        break
      row[todo] = _candidates(base, tab, todo.astype(_U), _U(a))
      todo = todo[np.isin(table_ids[row[todo]], batch_ids)]
  for _ in range(B + 1):  # the walk behind the attempts: the weights are left behind
    if not todo.size:
      break
    row[todo] = (row[todo] + 1) % n
    todo = todo[np.isin(table_ids[row[todo]], batch_ids)]
  return row


# ------------------------------------------------------------------------------------------------ the item table
WEIGHTED, IN_MEMORY = 'negative_sampler', 'negative_sampler_in_memory'


def sampler_kind(data_config):
  """which of the two samplers built here the config names (a config without either: the in-memory one's defaults)"""
  return WEIGHTED if data_config.WhichOneof('sampler') == WEIGHTED else IN_MEMORY


def _sampler_config(data_config):
  return getattr(data_config, sampler_kind(data_config))


def attr_features(data_config, feature_configs):
  """-> (item id feature config, [(attr field, [feature configs reading it])]); raises the build-time refusals that
  depend on the configs alone."""
  sc, kind = _sampler_config(data_config), sampler_kind(data_config)
  if sc.num_sample == 0:
    raise ValueError('%s: num_sample must be positive' % kind)
  if kind == IN_MEMORY and sc.num_eval_sample not in (0, sc.num_sample):
    # (the reference asserts num_eval_sample > 0 whenever it evaluates; here 0 means evaluation draws num_sample)
    raise NotImplementedError('negative_sampler_in_memory: num_eval_sample %d differs from num_sample %d (one table of '
                              'extended buffers serves both modes)' % (sc.num_eval_sample, sc.num_sample))
  by_field = OrderedDict((f, []) for f in sc.attr_fields)
  id_fc = None
  for fc in feature_configs:
    for f in fc.input_names:
      if f in by_field:
        by_field[f].append(fc)
    if sc.item_id_field in fc.input_names and id_fc is None:
      id_fc = fc
  if id_fc is None or id_fc.feature_type != FeatureConfig.IdFeature or len(id_fc.input_names) != 1:
    raise ValueError('%s: item_id_field %s must be the input of an IdFeature' % (kind, sc.item_id_field))
  for f, fcs in by_field.items():
    for fc in fcs:
      ok = len(fc.input_names) == 1 and (fc.feature_type == FeatureConfig.IdFeature or
                                         (fc.feature_type == FeatureConfig.RawFeature and fc.raw_input_dim <= 1))
      if not ok:
        raise NotImplementedError(
            '%s: attr field %s feeds feature %s, a %s: only IdFeatures and one-dimensional '
            'RawFeatures can be sampled' % (kind, f, feature_name_of(fc), FeatureConfig.FeatureType.Name(fc.feature_type)))
      if fc.HasField('ev_params'):
        raise NotImplementedError('%s: attr field %s feeds feature %s, a hash-table (ev_params) '
                                  'embedding' % (kind, f, feature_name_of(fc)))
  return id_fc, list(by_field.items())


def _convert(data_config, fcs, columns, n):
  """{feature name: int64 / float32 [n]} of the features `fcs` from raw string columns {input name: [n]}, through
  Input.preprocess - the batch's own path (hash_bucket_fast for hashed ids, the clamp of identity ids, the vocabulary,
  min/max normalisation and normalizer_fn of raw values)."""
  from easyrec_amd.input.input import Input
  from easyrec_amd.protos.dataset_pb2 import DatasetConfig
  dc = DatasetConfig()
  dc.CopyFrom(data_config)
  del dc.label_fields[:]
  dc.ClearField('sample_weight')
  dc.ClearField('sampler')
  inp = Input(dc, fcs, batch_size=n, hash_on_host=True)
  out = inp.preprocess(columns)
  sch, res = inp.schema, OrderedDict()
  for fc in fcs:
    name = feature_name_of(fc)
    res[name] = {}
    if name in sch.hash_single:
      res[name]['ids'] = np.ascontiguousarray(out['hash_ids'][sch.hash_single[name]['col']], dtype=np.int64)
    if name in sch.int_single:
      res[name]['ids'] = np.ascontiguousarray(out['int_ids'][sch.int_single[name]['col']], dtype=np.int64)
    if name in sch.raw:
      res[name]['raw'] = np.ascontiguousarray(out['raw'][sch.raw[name]['row']], dtype=np.float32)
  return res


class ItemTable(object):
  """The sampler's table on the host: `ids` int64 [n] (converted like the item-id feature, unique) and per feature name
  {'ids': int64 [n]} and / or {'raw': float32 [n]} (a bucketized RawFeature has both); `weights` fp64 [n] or None: what
  negative_sampler draws in proportion to (None: uniform)."""

  def __init__(self, ids, columns, weights=None):
    self.ids = np.ascontiguousarray(ids, dtype=np.int64)
    self.n = int(self.ids.size)
    self.weights = None
    if weights is not None:
      self.weights = check_weights(weights)
      if self.weights.shape != (self.n,):
        raise ValueError('item table: %d weights, the table %d rows' % (self.weights.size, self.n))
    self.columns = OrderedDict()
    for name, col in columns.items():
      if not isinstance(col, dict):
        col = np.asarray(col)
        col = {'raw': col} if col.dtype.kind == 'f' else {'ids': col}
      self.columns[name] = {k: np.ascontiguousarray(v, dtype=np.float32 if k == 'raw' else np.int64) for k, v in col.items()}
      for v in self.columns[name].values():
        if v.shape != (self.n,):
          raise ValueError('item table: column %s has shape %s, the table %d rows' % (name, v.shape, self.n))
    self.check_unique = True

  @classmethod
  def from_arrays(cls, ids, columns, weights=None):
    """ids and columns already converted (what the embedding lookups read): for tests and tools."""
    return cls(ids, columns, weights)

  @classmethod
  def from_file(cls, path, data_config, feature_configs):
    """The reference's local file (sampler.py:398-423): a header row naming the columns (`id...` and `feature...` are
    found by prefix), then one item per row: id, weight, the attributes joined by attr_delimiter.  negative_sampler
    reads the `weight...` column too (graphlearn's node file, id:int64 \t weight:float \t feature:string); the in-memory
    sampler ignores it, as the reference's does."""
    sc, weighted = _sampler_config(data_config), sampler_kind(data_config) == WEIGHTED
    id_fc, by_field = attr_features(data_config, feature_configs)
    fields = [f for f, _ in by_field]
    item_ids, weights, cols = [], [], [[] for _ in fields]
    item_id_col, weight_col, fea_id_col = 0, 1, 2
    with open(path, 'r') as fin:
      for line_id, line in enumerate(fin):
        parts = line.strip().split('\t')
        if line_id == 0:
          for tid, col in enumerate(parts):
            if col.split(':')[0].startswith('id'):
              item_id_col = tid
            if col.split(':')[0].startswith('weight'):
              weight_col = tid
            if col.split(':')[0].startswith('feature'):
              fea_id_col = tid
          continue
        if not line.strip():
          continue
        item_ids.append(str(int(parts[item_id_col])))
        if weighted:
          try:
            weights.append(float(parts[weight_col]))
          except ValueError:
            raise ValueError('%s row %d: weight %r is no number' % (path, line_id, parts[weight_col]))
        vals = parts[fea_id_col].split(sc.attr_delimiter)
        if len(vals) != len(fields):
          raise ValueError('%s row %d: %d attributes, attr_fields names %d' % (path, line_id, len(vals), len(fields)))
        for c, v in zip(cols, vals):
          c.append(v)
    n = len(item_ids)
    columns = dict(zip(fields, cols))
    fcs = [fc for _, group in by_field for fc in group]
    conv = _convert(data_config, fcs, columns, n) if fcs and n else {}
    ids = _convert(data_config, [id_fc], {id_fc.input_names[0]: item_ids}, n)[feature_name_of(id_fc)]['ids'] if n else []
    return cls(ids, conv, weights if weighted else None)

  @classmethod
  def synthetic(cls, rows, data_config, feature_configs, seed=20240607):
    """synthetic://<rows>: the item id is the row number (in the table's id column and in the attribute column of the
    item-id feature), every other id uniform over its feature's bucket range, raw values uniform in [0, 1); under
    negative_sampler row r has the weight 1 / (1 + r % 1024)."""
    from easyrec_amd.input.features import FeatureSchema
    id_fc, by_field = attr_features(data_config, feature_configs)
    fcs = [fc for _, group in by_field for fc in group]
    sch = FeatureSchema(data_config, fcs, batch_size=1)
    rng = np.random.default_rng(seed)
    ids = np.arange(rows, dtype=np.int64)
    columns = OrderedDict()
    for fc in fcs:
      name = feature_name_of(fc)
      col = {}
      buckets = sch.hash_single[name]['buckets'] if name in sch.hash_single else \
          (sch.int_single[name]['num_buckets'] if name in sch.int_single else None)
      if name in sch.raw:
        col['raw'] = rng.random(rows).astype(np.float32)
        if buckets is not None:
          from easyrec_amd.input.features import bucketize
          col['ids'] = bucketize(col['raw'], sch.int_single[name]['bounds'])
      elif fc is id_fc or feature_name_of(fc) == feature_name_of(id_fc):
        if rows > buckets:
          raise ValueError('%s: %d synthetic items do not fit the %d buckets of %s' %
                           (sampler_kind(data_config), rows, buckets, name))
        col['ids'] = ids
      else:
        col['ids'] = rng.integers(0, max(buckets, 1), size=rows, dtype=np.int64)
      columns[name] = col
    weights = 1.0 / (1.0 + (ids % 1024)) if sampler_kind(data_config) == WEIGHTED else None
    table = cls(ids, columns, weights)
    table.check_unique = False  # (row numbers)
    return table

  @classmethod
  def load(cls, data_config, feature_configs):
    path = _sampler_config(data_config).input_path
    if path.startswith(SYNTHETIC):
      return cls.synthetic(int(path[len(SYNTHETIC):]), data_config, feature_configs)
    return cls.from_file(path, data_config, feature_configs)


# ------------------------------------------------------------------------------------------------ the sampler
class NegativeSampler(object):
  """The table on the device, the extended buffers of DeviceFeatures, and the per-step draw: negative_sampler_in_memory's
  uniform one without replacement, or negative_sampler's weighted one with replacement (`weighted`)."""

  def __init__(self, data_config, feature_configs, features, seed, item_table=None, is_training=True):
    sc, self.kind = _sampler_config(data_config), sampler_kind(data_config)
    self.weighted = self.kind == WEIGHTED
    id_fc, by_field = attr_features(data_config, feature_configs)
    table = item_table if item_table is not None else ItemTable.load(data_config, feature_configs)
    self.N, self.seed, self.features = int(sc.num_sample), int(seed), features
    if self.weighted and not is_training and sc.num_eval_sample > 0:
      self.N = int(sc.num_eval_sample)  # (the reference's evaluator: BaseSampler.set_eval_num_sample)
    self.item_id_feature = feature_name_of(id_fc)
    B, dev = features.batch_size, features.device
    self.B, self.n = B, table.n
    if self.weighted and table.n >= 2 ** 31:  # (K1c's envelope; the composition's k is exact below it only)
      raise ValueError('%s: the item table has %d rows, the weighted draw takes fewer than 2^31' % (self.kind, table.n))
    if table.n < B + self.N:
      raise ValueError('%s: the item table has %d rows, batch_size + num_sample = %d' % (self.kind, table.n, B + self.N))
    if table.check_unique and np.unique(table.ids).size != table.n:
      raise ValueError('%s: duplicate item ids in the table (as the embedding of %s sees them: '
                       'raw ids that share a hash bucket count as one item)' % (self.kind, self.item_id_feature))
    self.table_ids = torch.from_numpy(table.ids).to(dev)
    self._host_ids = table.ids
    if self.weighted:
      # (a table without weights: uniform.)  The records travel as int64: torch has no arithmetic on uint64, none is needed
      self._host_alias = alias_table(table.weights if table.weights is not None else np.ones(table.n))
      self.alias_tab = torch.from_numpy(self._host_alias.view(np.int64)).to(dev)
    self.sel = torch.zeros(self.N, dtype=torch.int32, device=dev)
    self.columns = []  # (feature name, 'ids' | 'raw', table column, extended buffer)
    ext = OrderedDict()
    for field, fcs in by_field:
      for fc in fcs:
        name = feature_name_of(fc)
        if name not in table.columns:
          raise ValueError('%s: the item table has no column for feature %s (attr field %s)' % (self.kind, name, field))
        ext[name] = {}
        for kind, col in table.columns[name].items():
          buf = torch.zeros(B + self.N, dtype=torch.float32 if kind == 'raw' else torch.int64, device=dev)
          ext[name][kind] = buf
          self.columns.append((name, kind, torch.from_numpy(col).to(dev), buf))
    features.attach_sampler(self, ext)

  def uses_kernel(self):
    return (device_sampler and self.features.device.type == 'cuda' and lds_bytes(self.B) > 0 and  # (one envelope)
            len(self.columns) <= kernels.HipBackend.NEG_SAMPLE_MAX_COLS and isinstance(kernels.hip(), kernels.HipBackend))

  def _batch_column(self, name, kind):
    f = self.features
    return f.batch_ids_of(name) if kind == 'ids' else f.batch_raw(name)

  def run(self, step_counter, step_offset, sample=True):
    """Fill the extended buffers for the step *step_counter + step_offset: [0, B) the batch's values, and with `sample`
    [B, B + N) the drawn rows.  Sets what ids_of / raw of the attribute features return until the next call."""
    f = self.features
    if not sample:
      for name, kind, _, buf in self.columns:
        buf[:self.B].copy_(self._batch_column(name, kind))
      f.sampling = False
      return
    batch_ids = f.batch_ids_of(self.item_id_feature)
    if self.uses_kernel():
      columns = [(tab, self._batch_column(name, kind), buf) for name, kind, tab, buf in self.columns]
      if self.weighted:
        kernels.hip().neg_sample_weighted(self.alias_tab, self.table_ids, batch_ids, self.N, step_counter, step_offset,
                                          self.seed, columns, self.sel)
      else:
        kernels.hip().neg_sample(self.table_ids, batch_ids, self.N, step_counter, step_offset, self.seed, columns, self.sel)
    else:
      if f.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
        raise RuntimeError('%s: the composed draw reads the step counter and the batch ids on the '
                           'host and cannot be captured into a hipGraph (batch_size %d is outside the kernel\'s envelope, '
                           'or EASYREC_AMD_DEVICE_SAMPLER=0)' % (self.kind, self.B))
      step = int(step_counter.item()) + int(step_offset)
      if self.weighted:
        sel = draw_weighted(self.seed, step, self._host_alias, self._host_ids, batch_ids.cpu().numpy(), self.N)
      else:
        sel = draw(self.seed, step, self._host_ids, batch_ids.cpu().numpy(), self.N)
      sel = torch.from_numpy(sel).to(f.device)
      self.sel.copy_(sel.to(torch.int32))
      for name, kind, tab, buf in self.columns:
        buf[:self.B].copy_(self._batch_column(name, kind))
        buf[self.B:].copy_(tab[sel])
    f.sampling = True
