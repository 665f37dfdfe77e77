"""negative_sampler (the weighted draw with replacement) on the CPU: the host alias builder implies the weights, the
product's composed draw (easyrec_amd/input/neg_sampler.py draw_weighted) equals the restatement
(oracle/weighted_sampler_ref.py, written from include/easyrec_hip.h K1c) bit for bit, the draw's distribution, the
table file's weight column, the build-time refusals and the num_eval_sample rule, the reference's own composition
around the graphlearn call (tests/golden/weighted_sampler_vectors.npz), and a DSSM config with the sampler training on
the stand-in backend against the fp64 oracle fed the restatement's rows."""
import functools
import os

import numpy as np
import pytest
import torch

import _oracle_steps
import test_match_pins
import test_neg_sampler_pins as pins
from oracle import match_ref as mref
from oracle import weighted_sampler_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
# (B, N, n): one draw from two rows; the chi-square inputs; several waves; more than one drawing workgroup; the largest
# envelope batch over a uniform table that it nearly fills - q = 4096 / 4200, so 0.975^32 = 45 % of the draws walk
CASES = [(1, 1, 2), (5, 40, 61), (67, 130, 300), (1024, 1030, 5000), (4096, 64, 4200)]
STEPS = (0, 1, 5000000000)


# ---------------------------------------------------------------------------------------- inputs shared with the GPU tests
def chi_inputs():
  """n = 61, w_r = 1 + 1.5 (r % 7), w[5] = 0, w[17] = 40, ids 3 r + 1; the batch: the ids of rows {2, 9, 17, 30, 44}"""
  n = 61
  w = 1.0 + 1.5 * (np.arange(n) % 7)
  w[5], w[17] = 0.0, 40.0
  ids = (3 * np.arange(n) + 1).astype(np.int64)
  rows = np.array([2, 9, 17, 30, 44])
  return w, ids, ids[rows], rows


@functools.lru_cache(maxsize=None)
def case_inputs(B, N, n):
  """-> (weights [n], table ids [n], batch ids [B]) of a case: computed once, shared, never written to"""
  rng = np.random.default_rng(1000 * B + N)
  if (B, N, n) == (5, 40, 61):
    w, ids, batch, _ = chi_inputs()
  elif (B, N, n) == (4096, 64, 4200):
    w, ids = np.ones(n), pins.table_ids_of(n, seed=3)
    batch = rng.choice(ids, size=B, replace=False)
  elif n == 2:
    w, ids, batch = np.array([1.0, 3.0]), np.array([11, 7], dtype=np.int64), np.array([7], dtype=np.int64)
  else:
    w, ids = rng.random(n) * (rng.random(n) < 0.9), pins.table_ids_of(n, seed=4)  # (a tenth of the rows weigh nothing)
    w[rng.integers(0, n)] = 0.2 * w.sum()  # one dominant row ...
    batch = rng.choice(ids, size=B, replace=False)
    batch[0] = ids[int(np.argmax(w))]      # ... which the batch holds: rejection is exercised
    batch[1::5] = 10 ** 6 + rng.integers(0, 1000, size=batch[1::5].size)  # ids no table row has
    batch[-1] = batch[0] if B > 2 else batch[-1]                         # a duplicate
  for a in (w, ids, batch):
    a.setflags(write=False)
  return w, ids, batch.astype(np.int64)


@functools.lru_cache(maxsize=None)
def alias_of(B, N, n):
  from easyrec_amd.input import neg_sampler
  tab = neg_sampler.alias_table(case_inputs(B, N, n)[0])
  tab.setflags(write=False)
  return tab


@functools.lru_cache(maxsize=None)
def expected(B, N, n, step, seed=SEED):
  """the restatement's sel of a case at a step (the reference of the CPU and the GPU tests: computed once)"""
  w, ids, batch = case_inputs(B, N, n)
  sel = ref.draw(seed, step, alias_of(B, N, n), ids, batch, N)
  sel.setflags(write=False)
  return sel


def sampler_on(device, B, N, n, seed=SEED, is_training=True, num_eval_sample=0, table=None):
  """A weighted NegativeSampler over a case's table with an id column, a second id column and a raw column, on bare
  DeviceFeatures -> (sampler, features, the table's host columns)"""
  from easyrec_amd.input.features import DeviceFeatures, FeatureSchema
  from easyrec_amd.input.neg_sampler import ItemTable, NegativeSampler
  from easyrec_amd.protos.dataset_pb2 import DatasetConfig
  from easyrec_amd.protos.feature_config_pb2 import FeatureConfig
  dc = DatasetConfig()
  dc.batch_size = B
  fcs = []
  for name, kind in (('item', 'hash'), ('cate', 'int'), ('price', 'raw'), ('user', 'hash')):
    f = dc.input_fields.add()
    f.input_name, f.input_type = name, DatasetConfig.STRING
    fc = FeatureConfig()
    fc.input_names.append(name)
    if kind == 'raw':
      fc.feature_type = FeatureConfig.RawFeature
    else:
      fc.feature_type = FeatureConfig.IdFeature
      fc.embedding_dim = 4
      if kind == 'hash':
        fc.hash_bucket_size = 2 * 10 ** 6
      else:
        fc.num_buckets = 1000
    fcs.append(fc)
  ns = dc.negative_sampler
  ns.input_path, ns.num_sample, ns.item_id_field, ns.num_eval_sample = 'unused', N, 'item', num_eval_sample
  ns.attr_fields.extend(['item', 'cate', 'price'])
  cols = None
  if table is None:  # the case's
    w, ids, _ = case_inputs(B, N, n)
    rng = np.random.default_rng(5)
    cols = {'item': ids.copy(), 'cate': rng.integers(0, 1000, size=n).astype(np.int64), 'price': rng.random(n).astype(np.float32)}
    table = ItemTable.from_arrays(cols['item'], cols, weights=w)
  features = DeviceFeatures(FeatureSchema(dc, fcs, batch_size=B), device)
  sampler = NegativeSampler(dc, fcs, features, seed, table, is_training=is_training)
  return sampler, features, cols


def assert_draw_is_the_restatement(sampler, features, cols, batch, want):
  """sel and every extended column of the step just run, bit for bit"""
  assert np.array_equal(sampler.sel.cpu().numpy(), want.astype(np.int32))
  assert features.sampling
  for name in ('item', 'cate'):
    got = features.ids_of(name).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, ref.extended(batch[name], cols[name], want)), name
  got = features.raw('price').cpu().numpy()
  assert got.dtype == np.float32
  assert np.array_equal(got.view(np.uint32), ref.extended(batch['price'], cols['price'], want).view(np.uint32))
  assert features.ids_of('user').shape == (features.batch_size,)


# ---------------------------------------------------------------------------------------- the alias table
def _table_weights():
  rng = np.random.default_rng(11)
  # (constant weights other than 1: w * (n / sum w) rounds just below 1 for every row of 0.1 x 3 and 0.3 x 7 - no row is
  # above the mean)
  return [np.array([2.5]), np.array([1.0, 3.0]), np.array([0.0, 3.0]), chi_inputs()[0], rng.random(1000) ** 3,
          np.ones(64), np.arange(5, dtype=np.float64), np.full(3, 0.1), np.full(7, 0.3), np.full(39, rng.random()),
          np.full(1000, 1e-3), np.r_[np.full(6, 0.3), 0.3 * (1 + 2.0 ** -50)]]


@pytest.mark.parametrize('w', _table_weights(), ids=lambda w: 'n%d_%.3g' % (w.size, w[-1]))
def test_alias_table_implies_the_weights(w):
  """(prob_i + sum over alias_k = i of (1 - prob_k)) / n equals w / sum(w) within 1e-7: each prob is rounded once to fp32
  (<= 2^-25 of error each, prob <= 1), a row receives at most n contributions and the sum is divided by n, so the
  error is below 2^-25 = 3e-8."""
  from easyrec_amd.input import neg_sampler
  tab = neg_sampler.alias_table(w)
  prob, alias = ref.unpack(tab)
  assert tab.dtype == np.uint64 and tab.shape == w.shape
  assert all(0.0 <= p <= 1.0 for p in prob) and all(0 <= a < w.size for a in alias)
  err = np.abs(ref.implied_distribution(tab) - w / w.sum()).max()
  print('n %d: max |implied - w / sum w| = %.3g' % (w.size, err))
  assert err <= 1e-7
  assert np.array_equal(neg_sampler.alias_table(w.astype(np.float32)), neg_sampler.alias_table(w.astype(np.float32).astype(np.float64)))


@pytest.mark.parametrize('w', [[1.0, -0.5], [1.0, float('nan')], [float('inf'), 1.0], [0.0, 0.0]])
def test_bad_weights_are_refused(w):
  from easyrec_amd.input import neg_sampler
  with pytest.raises(ValueError, match='weights'):
    neg_sampler.alias_table(np.array(w))
  with pytest.raises(ValueError, match='weights'):
    neg_sampler.ItemTable.from_arrays([1, 2], {}, weights=w)
  with pytest.raises(ValueError, match='3 weights'):
    neg_sampler.ItemTable.from_arrays([1, 2], {}, weights=[1.0, 1.0, 1.0])


# ---------------------------------------------------------------------------------------- the draw
@pytest.mark.parametrize('B,N,n', CASES)
def test_composition_equals_the_restatement(B, N, n):
  from easyrec_amd.input import neg_sampler
  sampler, features, cols = sampler_on('cpu', B, N, n)
  assert sampler.weighted and not sampler.uses_kernel()
  w, ids, batch_ids = case_inputs(B, N, n)
  batch = pins.load_batch(features, batch_ids.copy())
  counter = torch.zeros(1, dtype=torch.int64)
  for step in STEPS:
    counter.fill_(step + 1)
    sampler.run(counter, -1)
    want = expected(B, N, n, step)
    assert_draw_is_the_restatement(sampler, features, cols, batch, want)
    assert np.array_equal(neg_sampler.draw_weighted(SEED, step, alias_of(B, N, n), ids, batch_ids, N), want)
    assert want.min() >= 0 and want.max() < n and not set(ids[want].tolist()) & set(batch_ids.tolist())
  assert not np.array_equal(expected(B, 1030, 5000, 0), expected(B, 1030, 5000, 1)) if n == 5000 else True
  sampler.run(counter, 0, sample=False)
  assert not features.sampling and features.ids_of('item').shape == (B,)


def test_the_walk_is_taken_and_the_draw_repeats_rows():
  """the (4096, 64, 4200) case: about 45 % of its draws end in the walk behind the 32 attempts; with replacement: the
  (1024, 1030, 5000) case draws its heaviest eligible rows more than once; a permuted batch draws the same rows."""
  from easyrec_amd.input import neg_sampler
  B, N, n = 4096, 64, 4200
  w, ids, batch = case_inputs(B, N, n)
  stats = {}
  sel = ref.draw(SEED, 0, alias_of(B, N, n), ids, batch, N, stats)
  assert np.array_equal(sel, expected(B, N, n, 0)) and 15 <= stats['walked'] <= 45, stats
  assert len(set(expected(1024, 1030, 5000, 0).tolist())) < 1030
  perm = np.random.default_rng(2).permutation(batch)
  assert np.array_equal(neg_sampler.draw_weighted(SEED, 0, alias_of(B, N, n), ids, perm, N), sel)


def chi_square(draw, steps=500, N=40, seed=12345):
  """chi-square of the row counts of `steps` steps against w with the batch rows zeroed, over the rows of positive
  eligible weight -> (chi-square, degrees of freedom, draws that fell on a zero-weight or batch row)"""
  from easyrec_amd.input import neg_sampler
  w, ids, batch, rows = chi_inputs()
  tab = neg_sampler.alias_table(w)
  counts = np.zeros(w.size)
  for step in range(steps):
    np.add.at(counts, draw(seed, step, tab, ids, batch, N), 1)
  eligible = w.copy()
  eligible[rows] = 0.0
  live = eligible > 0
  exp = eligible[live] / eligible.sum() * steps * N
  return float(((counts[live] - exp) ** 2 / exp).sum()), int(live.sum()) - 1, int(counts[~live].sum()), counts


CHI_BAR = 91.9  # the 0.999 chi-square quantile at 54 degrees of freedom


@pytest.mark.parametrize('which', ['restatement', 'composition'])
def test_draw_follows_the_weights(which):
  """n = 61, N = 40, seed 12345, steps 0..499: the dominant row is in the batch, so rejection is exercised; the bar is the
  0.999 quantile at 54 degrees of freedom.  The specified algorithm gives 39.1."""
  from easyrec_amd.input import neg_sampler
  chi, df, outside, _ = chi_square(ref.draw if which == 'restatement' else neg_sampler.draw_weighted)
  print('%s: chi-square %.1f (df %d, bar %.1f), %d draws outside the eligible rows' % (which, chi, df, CHI_BAR, outside))
  assert df == 54 and outside == 0
  assert chi <= CHI_BAR


def test_lds_formula_is_the_library_s(built_lib):
  from easyrec_amd import kernels
  from easyrec_amd.input import neg_sampler
  be = kernels.HipBackend()
  for B in list(range(0, 70)) + [2047, 2048, 2049, 4095, 4096, 4097, 10 ** 6]:
    assert be.neg_sample_weighted_lds_bytes(B) == neg_sampler.wlds_bytes(B), B
  assert neg_sampler.wlds_bytes(4096) == 8 * 8192 + 16 and neg_sampler.wlds_bytes(4097) == 0 == neg_sampler.wlds_bytes(0)


# ---------------------------------------------------------------------------------------- the item table
def weighted_table_config(**kw):
  cfg = pins.table_config(**kw)
  ns = cfg.data_config.negative_sampler_in_memory.SerializeToString()
  cfg.data_config.negative_sampler.ParseFromString(ns)  # (the two messages have the same fields)
  assert cfg.data_config.WhichOneof('sampler') == 'negative_sampler'
  return cfg


WEIGHTS = [0.5, 2.0, 0.0, 1e-3, 7.25, 3.0]


def write_weighted_table(path, weights=WEIGHTS, header='id:int64\tweight:float\tfeature:string'):
  with open(path, 'w') as f:
    f.write(header + '\n')
    for (item, shop, level, price), w in zip(pins.ROWS, weights):
      f.write('%d\t%s\t%s:%s:%s\n' % (item, w, shop, level, price))
  return str(path)


def test_table_file_round_trips_ids_weights_and_columns(ref_backend, tmp_path):
  """graphlearn's node file, id:int64 \\t weight:float \\t feature:string: the ids and the columns as the in-memory
  sampler's loader reads them, the weight column as fp64; the columns are found by their header prefixes"""
  from easyrec_amd.input.neg_sampler import ItemTable
  cfg = weighted_table_config()
  fcs = list(cfg.feature_config.features)
  table = ItemTable.from_file(write_weighted_table(tmp_path / 'items.tsv'), cfg.data_config, fcs)
  plain = pins.table_config()
  same = ItemTable.from_file(pins.write_table(tmp_path / 'plain.tsv'), plain.data_config, list(plain.feature_config.features))
  assert same.weights is None  # (the in-memory sampler does not read the column)
  assert table.weights.dtype == np.float64 and table.weights.tolist() == WEIGHTS
  assert np.array_equal(table.ids, same.ids) and list(table.columns) == list(same.columns)
  for name, col in same.columns.items():
    for kind, v in col.items():
      assert np.array_equal(table.columns[name][kind], v), (name, kind)
  path = tmp_path / 'swapped.tsv'
  with open(path, 'w') as f:
    f.write('weight:float\tfeature:string\tid:int64\n')
    for (item, shop, level, price), w in zip(pins.ROWS, WEIGHTS):
      f.write('%r\t%s:%s:%s\t%d\n' % (w, shop, level, price, item))
  swapped = ItemTable.from_file(str(path), cfg.data_config, fcs)
  assert swapped.weights.tolist() == WEIGHTS and np.array_equal(swapped.ids, table.ids)
  for bad in ('-1.0', 'nan', 'inf', 'heavy'):
    with pytest.raises(ValueError, match='weight'):
      ItemTable.from_file(write_weighted_table(tmp_path / 'bad.tsv', WEIGHTS[:3] + [bad] + WEIGHTS[4:]), cfg.data_config, fcs)
  with pytest.raises(ValueError, match='sum to zero'):
    ItemTable.from_file(write_weighted_table(tmp_path / 'zero.tsv', [0.0] * 6), cfg.data_config, fcs)


def test_synthetic_table_has_the_stated_weights(ref_backend):
  from easyrec_amd.input.neg_sampler import ItemTable
  cfg = weighted_table_config()
  cfg.data_config.negative_sampler.attr_fields.insert(0, 'item')
  cfg.data_config.negative_sampler.input_path = 'synthetic://3000'
  table = ItemTable.load(cfg.data_config, list(cfg.feature_config.features))
  assert table.n == 3000 and np.array_equal(table.weights, 1.0 / (1.0 + np.arange(3000) % 1024))
  plain = pins.table_config()
  plain.data_config.negative_sampler_in_memory.attr_fields.insert(0, 'item')
  plain.data_config.negative_sampler_in_memory.input_path = 'synthetic://3000'
  same = ItemTable.load(plain.data_config, list(plain.feature_config.features))
  assert same.weights is None and np.array_equal(same.columns['shop']['ids'], table.columns['shop']['ids'])


# ---------------------------------------------------------------------------------------- refusals and routing
def wnegsam_cfg(B, N, rows, model='dssm', num_eval_sample=0):
  mc = pins._make_configs()
  base = mc.dssm_taobao(in_batch=True, batch_size=B, scale=0.01) if model == 'dssm' else \
      mc.mind_taobao(list_wise=True, batch_size=B, scale=0.01)
  cfg = mc.with_negative_sampler(base, rows, num_sample=N, weighted=True)
  cfg.data_config.negative_sampler.num_eval_sample = num_eval_sample
  return cfg


def weighted_item_table_for(cfg, rows, seed=3):
  """pins.item_table_for's columns with weights: a tenth of the rows weigh nothing, one row a fifth of the total"""
  from easyrec_amd.input.neg_sampler import ItemTable
  plain = pins.negsam_cfg(cfg.data_config.batch_size, cfg.data_config.negative_sampler.num_sample, rows)
  table = pins.item_table_for(plain, rows, seed)
  rng = np.random.default_rng(seed + 1)
  w = rng.random(rows) * (rng.random(rows) < 0.9)
  w[7] = 0.25 * w.sum()
  return ItemTable.from_arrays(table.ids, table.columns, weights=w)


@pytest.mark.parametrize('model', ['dssm', 'mind'])
def test_a_sampler_without_a_table_is_refused(ref_backend, model):
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  mc = pins._make_configs()
  cfg = mc.dssm_taobao(in_batch=True, batch_size=16, scale=0.01) if model == 'dssm' else \
      mc.mind_taobao(list_wise=True, batch_size=16, scale=0.01)
  cfg.data_config.negative_sampler.SetInParent()
  with pytest.raises(NotImplementedError, match='negative_sampler: no input_path'):
    EasyRecEstimator(cfg, device='cpu', batch_size=16, seed=4)
  # a model that is no two-tower model
  cfg = mc.din_taobao(batch_size=16, scale=0.01, seq_len=12)
  mc.with_negative_sampler(cfg, 301, num_sample=8, weighted=True)
  with pytest.raises(NotImplementedError, match='negative_sampler: DIN takes no sampled negatives|takes no sampled negatives'):
    EasyRecEstimator(cfg, device='cpu', batch_size=16, seed=4)


@pytest.mark.parametrize('is_training,num_eval_sample,want', [(True, 24, 8), (False, 24, 24), (False, 0, 8), (True, 0, 8)])
def test_num_eval_sample_rule(ref_backend, is_training, num_eval_sample, want):
  """an estimator built with is_training=False draws num_eval_sample rows when that is positive, else num_sample"""
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  B, N, rows = 16, 8, 301
  cfg = wnegsam_cfg(B, N, rows, num_eval_sample=num_eval_sample)
  est = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4, is_training=is_training,
                         item_table=weighted_item_table_for(cfg, rows))
  assert est.sampler.weighted and est.sampler.N == want
  assert est.features.ids_of('adgroup_id').shape == (B,) and est.sampler.sel.shape == (want,)


def test_build_time_refusals(ref_backend):
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  B, N, rows = 16, 8, 301
  for other in ('negative_sampler_v2', 'hard_negative_sampler', 'hard_negative_sampler_v2'):
    cfg = wnegsam_cfg(B, N, rows)
    getattr(cfg.data_config, other).SetInParent()
    with pytest.raises(NotImplementedError, match=other + ':'):
      EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4)
  cfg = wnegsam_cfg(B, N, rows)
  with pytest.raises(ValueError, match='bf16'):
    EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4, dense_dtype='bf16', item_table=weighted_item_table_for(cfg, rows))
  cfg = wnegsam_cfg(B, N, rows)
  cfg.data_config.negative_sampler.attr_fields.append('tag_brand_list')  # a sequence attribute
  with pytest.raises(NotImplementedError, match='negative_sampler: attr field tag_brand_list'):
    EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4, item_table=weighted_item_table_for(wnegsam_cfg(B, N, rows), rows))
  cfg = wnegsam_cfg(B, N, rows)
  [fc for fc in cfg.feature_config.features if list(fc.input_names) == ['brand']][0].ev_params.SetInParent()
  with pytest.raises(NotImplementedError, match='negative_sampler: attr field brand .*ev_params'):
    EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4, item_table=weighted_item_table_for(wnegsam_cfg(B, N, rows), rows))
  cfg = wnegsam_cfg(B, N, 20)
  with pytest.raises(ValueError, match='negative_sampler: the item table has 20 rows'):
    EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4, item_table=weighted_item_table_for(cfg, 20))


@pytest.mark.parametrize('weighted', [True, False])
def test_target_attention_keyed_by_sampled_fields_is_refused(ref_backend, weighted):
  """a sequence_features block of the user group whose key is an attribute field of the sampler (the reference's
  dssm_neg_sampler_need_key_feature): the key has B + N rows, the history B - a named refusal when the group is built"""
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  B, N, rows = 16, 8, 301
  cfg = wnegsam_cfg(B, N, rows) if weighted else pins.negsam_cfg(B, N, rows)
  table = weighted_item_table_for(wnegsam_cfg(B, N, rows), rows)
  user = [g for g in cfg.model_config.feature_groups if g.group_name == 'user'][0]
  sf = user.sequence_features.add()
  sf.group_name, sf.allow_key_search = 'seq_fea', True
  m = sf.seq_att_map.add()
  m.key.append('brand')
  m.hist_seq.append('tag_brand_list')
  with pytest.raises(NotImplementedError, match='sequence_features keys brand are attribute fields of the negative sampler'):
    EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4, item_table=table).build()


def test_a_table_of_2_to_the_31_rows_is_refused():
  """the kernel's envelope and the composition's exact k end below 2^31 rows: refused by name when the sampler is built
  (a stand-in table: only its row count is read before the refusal)"""
  import types
  table = types.SimpleNamespace(n=2 ** 31, ids=np.zeros(1, np.int64), weights=None, columns={}, check_unique=False)
  with pytest.raises(ValueError, match='negative_sampler: the item table has 2147483648 rows'):
    sampler_on('cpu', 5, 40, 61, table=table)


def test_the_composition_cannot_be_captured(monkeypatch):
  """EASYREC_AMD_DEVICE_SAMPLER=0 (or a batch outside the envelope) selects the composition, which reads the step counter
  on the host: inside a capture it raises before it touches the device"""
  from easyrec_amd.input import neg_sampler
  sampler, features, cols = sampler_on('cpu', 5, 40, 61)
  monkeypatch.setattr(neg_sampler, 'device_sampler', False)
  monkeypatch.setattr(features, 'device', torch.device('cuda', 0))
  monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
  assert not sampler.uses_kernel()
  with pytest.raises(RuntimeError, match='negative_sampler: the composed draw .* cannot be captured'):
    sampler.run(torch.zeros(1, dtype=torch.int64), -1)


def test_committed_configs_are_the_generated_ones():
  from easyrec_amd.utils import config_util
  mc = pins._make_configs()
  for name, base in (('dssm', mc.dssm_taobao(in_batch=True, item_rows=10000000)),
                     ('mind', mc.mind_taobao(list_wise=True, item_rows=10000000))):
    cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', name + '_wnegsam_taobao_10m.config'))
    base.model_dir = 'experiments/%s_wnegsam_taobao_ckpt' % name
    assert cfg == mc.with_negative_sampler(base, 10000000, weighted=True)
    ns = cfg.data_config.negative_sampler
    assert cfg.data_config.WhichOneof('sampler') == 'negative_sampler' and ns.num_sample == 1024
    assert ns.input_path == 'synthetic://10000000' and ns.item_id_field == 'adgroup_id'
    sibling = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', name + '_negsam_taobao_10m.config'))
    assert ns.SerializeToString() == sibling.data_config.negative_sampler_in_memory.SerializeToString()
    assert cfg.model_config == sibling.model_config and cfg.feature_config == sibling.feature_config


# ---------------------------------------------------------------------------------------- the reference's composition
def test_extended_columns_are_the_reference_s_composition(monkeypatch):
  """tests/golden/weighted_sampler_vectors.npz (make_weighted_sampler_vectors.py): the reference's sampler.build,
  NegativeSampler._get_impl / _parse_nodes and the sampler branch of Input._preprocess around a recording stand-in for
  graphlearn.  It declares a weighted item node with the attr fields' types, asks for expand_factor = ceil(N /
  batch_size) rows per id by 'node_weight', hands over the ids padded to batch_size with the last one, flattens the
  [batch_size, expand_factor] result, cuts it to N and appends it behind the batch's rows.  Given the stand-in's rows
  as sel, the product's extended columns are the reference's."""
  from easyrec_amd.input import neg_sampler
  g = np.load(os.path.join(ROOT, 'tests', 'golden', 'weighted_sampler_vectors.npz'))
  batch_size, rows_in, N, n = int(g['batch_size']), int(g['short_batch']), int(g['num_sample']), int(g['table_rows'])
  E = int(g['expand_factor'])
  assert E == -(-N // batch_size) and E * batch_size > N  # (the cut is exercised)
  assert str(g['strategy']) == 'node_weight' and bool(g['decoder_weighted']) and str(g['sampled_type']) == 'item'
  assert g['decoder_attr_types'].tolist() == ['string', 'int', 'float'] and str(g['decoder_attr_delimiter']) == ';'
  assert rows_in < batch_size and g['got_ids'].tolist() == g['batch_item'].tolist() + [int(g['batch_item'][-1])] * (batch_size - rows_in)
  assert g['standin_rows'].shape == (batch_size, E)
  sel = g['standin_rows'].reshape(-1)[:N]  # flatten, then cut
  assert g['concat_user'].shape == (rows_in,)  # (no attribute field: the batch's own rows)
  # the product on the same table and batch, its draw replaced by the stand-in's rows
  from easyrec_amd.input.neg_sampler import ItemTable
  cols = {'item': g['table_item'], 'cate': g['table_cate'], 'price': g['table_price'].astype(np.float32)}
  sampler, features, _ = sampler_on('cpu', rows_in, N, n, table=ItemTable.from_arrays(cols['item'], cols, weights=np.ones(n)))
  monkeypatch.setattr(neg_sampler, 'draw_weighted', lambda seed, step, tab, ids, batch_ids, count: sel.copy())
  sch = features.schema
  features.hash_ids[sch.hash_single['item']['col']].copy_(torch.from_numpy(g['batch_item']))
  features.int_ids[sch.int_single['cate']['col']].copy_(torch.from_numpy(g['batch_cate']))
  features.raw_block[sch.raw['price']['row']].copy_(torch.from_numpy(g['batch_price'].astype(np.float32)))
  sampler.run(torch.ones(1, dtype=torch.int64), -1)
  assert np.array_equal(features.ids_of('item').numpy(), g['concat_item'])
  assert np.array_equal(features.ids_of('cate').numpy(), g['concat_cate'])
  assert np.array_equal(features.raw('price').numpy(), g['concat_price'].astype(np.float32))
  assert np.array_equal(ref.extended(g['batch_cate'], g['table_cate'], sel), g['concat_cate'])  # (the restatement's rule too)


# ---------------------------------------------------------------------------------------- the model
def test_dssm_with_the_sampler_steps_on_the_stand_in(ref_backend, built_lib):
  """tests/test_neg_sampler_pins.py's step test with the weighted sampler: two steps against the fp64 model oracle fed the
  restatement's rows, the item group's rows being B + N; then predict() without and with negatives."""
  from easyrec_amd.input import neg_sampler
  from easyrec_amd.input.synthetic import SyntheticBatches
  B, N, rows = 16, 8, 301
  cfg = wnegsam_cfg(B, N, rows)
  table = weighted_item_table_for(cfg, rows)
  tab = neg_sampler.alias_table(table.weights)

  def check(est, orc, step, batch):
    assert est.model._prediction_dict['item_tower_emb'].shape == (B + N, 32)
    batch_ids = batch['hash_ids'][est.schema.hash_single['adgroup_id']['col']]
    sel = ref.draw(4, step, tab, table.ids, batch_ids, N)
    assert np.array_equal(est.sampler.sel.numpy(), sel.astype(np.int32))
    assert np.array_equal(est.features.ids_of('adgroup_id').numpy(), ref.extended(batch_ids, table.columns['adgroup_id']['ids'], sel))
    assert (table.weights[sel] > 0).all()
  est = _oracle_steps.first_steps(cfg, B, seed=4, device='cpu', oracle_dtype=torch.float64,
                                  coverage=test_match_pins.dssm_coverage, est_kw=dict(item_table=table),
                                  oracle_kw=dict(item_table=table, sampler_seed=4, alias_tab=tab), after_step=check)
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=44)
  est.model._is_training = est.ctx.is_training = False
  pred = est.predict(gen.next_batch())
  assert pred['item_tower_emb'].shape == (B, 32) and pred['logits'].shape == (B, B)
  pred = est.predict(sample_negatives=True)
  assert pred['item_tower_emb'].shape == (B + N, 32) and pred['logits'].shape == (B, B + N)
  metrics = est.model.build_metric_graph(cfg.eval_config)
  assert set(metrics) == {'recall@10', 'recall_neg_sam@10', 'recall_in_batch@10'}
  assert metrics == pytest.approx(mref.recall_at_k(pred['logits'].double().numpy(), 10))
