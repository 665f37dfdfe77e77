"""negative_sampler_in_memory on the CPU: the restated permutation is a bijection, the product's composed draw
(easyrec_amd/input/neg_sampler.py) equals the restatement (oracle/neg_sampler_ref.py, written from include/easyrec_hip.h
K1b) bit for bit, its properties, its uniformity, the item table's loading and build-time refusals, and a DSSM config
with the sampler training on the stand-in backend with the fp64 restatement's losses over B + N item rows."""
import os
import sys

import numpy as np
import pytest
import torch

import test_match_pins
from _oracle_steps import first_steps
from oracle import match_ref as mref
from oracle import neg_sampler_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
CASES = [(301, 67, 40), (107, 67, 40), (1025, 16, 1)]  # (n, B, N); n == B + N: every eligible row is walked


def _make_configs():
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  return make_configs


def table_ids_of(n, seed=0):
  """n distinct ids, not in row order, none of them negative or >= 10^6"""
  return np.random.default_rng(seed).permutation(10 ** 6)[:n].astype(np.int64)


def batch_ids_of(kind, table_ids, B, seed=1):
  rng = np.random.default_rng(seed)
  absent = 10 ** 6 + rng.integers(0, 1000, size=B)  # (no table id is that large)
  if kind == 'duplicates':
    ids = rng.choice(table_ids, size=B, replace=False)
    ids[B // 2:] = ids[:B - B // 2]
  elif kind == 'some_absent':
    ids = rng.choice(table_ids, size=B, replace=False)
    ids[::3] = absent[::3]
    ids[-1] = -1  # (a dropped empty string)
  elif kind == 'only_absent':
    ids = absent
  else:
    ids = rng.choice(table_ids, size=B, replace=False)
  return ids.astype(np.int64)


def test_restated_permutation_is_a_bijection():
  for n in (1, 2, 3, 5, 301, 1024, 1025):
    for step in (0, 1, 77):
      assert sorted(ref.perm(SEED, step, n).tolist()) == list(range(n)), (n, step)
  assert not np.array_equal(ref.perm(SEED, 0, 301), ref.perm(SEED, 1, 301))
  assert not np.array_equal(ref.perm(SEED, 0, 301), ref.perm(SEED + 1, 0, 301))


def sampler_on(device, n, B, N, seed=SEED):
  """A NegativeSampler over a table with an id column, a second id column and a raw column, on bare DeviceFeatures
  -> (sampler, features, the table's host columns)"""
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
  ns = dc.negative_sampler_in_memory
  ns.input_path, ns.num_sample, ns.item_id_field = 'unused', N, 'item'
  ns.attr_fields.extend(['item', 'cate', 'price'])
  rng = np.random.default_rng(5)
  ids = table_ids_of(n)
  cols = {'item': ids, 'cate': rng.integers(0, 1000, size=n).astype(np.int64), 'price': rng.random(n).astype(np.float32)}
  features = DeviceFeatures(FeatureSchema(dc, fcs, batch_size=B), device)
  sampler = NegativeSampler(dc, fcs, features, seed, ItemTable.from_arrays(ids, cols))
  return sampler, features, cols


def load_batch(features, batch_ids, seed=9):
  """the batch's own columns: the item ids, and arbitrary values in the other attribute columns -> host copies"""
  rng = np.random.default_rng(seed)
  B = features.batch_size
  sch = features.schema
  cate, price = rng.integers(0, 1000, size=B).astype(np.int64), rng.random(B).astype(np.float32)
  features.hash_ids[sch.hash_single['item']['col']].copy_(torch.from_numpy(batch_ids))
  features.int_ids[sch.int_single['cate']['col']].copy_(torch.from_numpy(cate))
  features.raw_block[sch.raw['price']['row']].copy_(torch.from_numpy(price))
  return {'item': batch_ids, 'cate': cate, 'price': price}


def assert_draw_is_the_restatement(sampler, features, cols, batch, step):
  """sel and every extended column of the step just run, bit for bit"""
  want = ref.draw(sampler.seed, step, cols['item'], batch['item'], sampler.N)
  assert np.array_equal(sampler.sel.cpu().numpy(), want.astype(np.int32)), step
  assert features.sampling
  for name in ('item', 'cate'):
    got = features.ids_of(name).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, ref.extended(batch[name], cols[name], want)), name
  got = features.raw('price').cpu().numpy()
  assert got.dtype == np.float32
  assert np.array_equal(got.view(np.uint32), ref.extended(batch['price'], cols['price'], want).view(np.uint32))
  assert features.ids_of('user').shape == (features.batch_size,)  # (no attribute field: the batch's own rows)
  return want


@pytest.mark.parametrize('kind', ['duplicates', 'some_absent', 'only_absent'])
@pytest.mark.parametrize('n,B,N', CASES)
def test_composition_equals_the_restatement(n, B, N, kind):
  from easyrec_amd.input import neg_sampler
  sampler, features, cols = sampler_on('cpu', n, B, N)
  assert not sampler.uses_kernel()
  batch = load_batch(features, batch_ids_of(kind, cols['item'], B))
  counter = torch.zeros(1, dtype=torch.int64)
  for step in (0, 1, 5000000000):
    counter.fill_(step + 1)
    sampler.run(counter, -1)  # (inside a training step the prologue has advanced the counter)
    want = assert_draw_is_the_restatement(sampler, features, cols, batch, step)
    assert np.array_equal(neg_sampler.draw(SEED, step, cols['item'], batch['item'], N), want)
    assert np.array_equal(neg_sampler.perm(SEED, step, n, B + N), ref.perm(SEED, step, n, np.arange(B + N)))
  sampler.run(counter, 0, sample=False)
  assert not features.sampling and features.ids_of('item').shape == (B,) and features.raw('price').shape == (B,)


def test_draw_properties():
  from easyrec_amd.input import neg_sampler
  n, B, N = 301, 67, 40
  table = table_ids_of(n)
  batch = batch_ids_of('plain', table, B)
  sel = neg_sampler.draw(SEED, 3, table, batch, N)
  assert len(set(sel.tolist())) == N and sel.min() >= 0 and sel.max() < n
  assert not set(table[sel].tolist()) & set(batch.tolist())
  rng = np.random.default_rng(2)
  assert np.array_equal(neg_sampler.draw(SEED, 3, table, rng.permutation(batch), N), sel)
  dup = batch.copy()
  dup[1] = dup[0]  # the set loses one id: only that id's row may come back
  sel_dup = neg_sampler.draw(SEED, 3, table, dup, N)
  assert set(table[sel_dup].tolist()) - set(table[sel].tolist()) <= {int(batch[1])}
  twice = np.concatenate([batch[:B // 2], batch[:B - B // 2]])  # duplicates of a subset, B unchanged
  again = np.concatenate([batch[:B - B // 2], batch[:B // 2]])
  assert np.array_equal(neg_sampler.draw(SEED, 3, table, twice, N), neg_sampler.draw(SEED, 3, table, again, N))
  assert not np.array_equal(neg_sampler.draw(SEED, 4, table, batch, N), sel)
  assert not np.array_equal(neg_sampler.draw(SEED + 1, 3, table, batch, N), sel)


def chi_squares(draw, n, N, steps):
  """(chi-square of the per-row selection counts, chi-square of the first draw) over `steps` consecutive steps"""
  table = np.arange(n, dtype=np.int64)
  batch = np.array([-5], dtype=np.int64)  # no exclusions
  rows, first = np.zeros(n), np.zeros(n)
  for step in range(steps):
    sel = draw(SEED, step, table, batch, N)
    rows[sel] += 1
    first[sel[0]] += 1
  chi = lambda obs, exp: float(((obs - exp) ** 2 / exp).sum())
  return chi(rows, steps * N / n), chi(first, steps / n)


def test_draw_is_uniform():
  """seed 1234, n = 301, N = 40, 3000 steps, no exclusions: both chi-squares within df +- 5 sqrt(2 df), df = 300.  A
  condition on the specified algorithm, which gives 269.8 and 303.6."""
  from easyrec_amd.input import neg_sampler
  n, N, steps = 301, 40, 3000
  got_rows, got_first = chi_squares(neg_sampler.draw, n, N, steps)
  print('chi-square of the selection counts %.1f, of the first draw %.1f (df %d)' % (got_rows, got_first, n - 1))
  df = n - 1
  for v in (got_rows, got_first):
    assert abs(v - df) <= 5 * np.sqrt(2 * df), (got_rows, got_first)
  assert got_rows == pytest.approx(269.8, abs=0.06) and got_first == pytest.approx(303.6, abs=0.06)


def test_lds_formula_is_the_library_s(built_lib):
  from easyrec_amd import kernels
  from easyrec_amd.input import neg_sampler
  be = kernels.HipBackend()
  for B in list(range(0, 70)) + [2047, 2048, 2049, 4095, 4096, 4097, 10 ** 6]:
    assert be.neg_sample_lds_bytes(B) == neg_sampler.lds_bytes(B), B
  assert neg_sampler.lds_bytes(4096) == 8 * 8192 + 128 <= 160 * 1024 and neg_sampler.lds_bytes(4097) == 0 == neg_sampler.lds_bytes(0)


# ---------------------------------------------------------------------------------------- the item table
def table_config(n_items=6, num_sample=2, batch_size=3):
  from easyrec_amd.protos.pipeline_pb2 import EasyRecConfig
  from google.protobuf import text_format
  cfg = EasyRecConfig()
  text_format.Merge('''
    data_config {
      batch_size: %d
      input_fields { input_name: 'clk' input_type: INT32 }
      input_fields { input_name: 'item' input_type: STRING }
      input_fields { input_name: 'shop' input_type: STRING }
      input_fields { input_name: 'level' input_type: INT32 }
      input_fields { input_name: 'price' input_type: DOUBLE }
      input_fields { input_name: 'tags' input_type: STRING }
      label_fields: 'clk'
      negative_sampler_in_memory { input_path: 'unset' num_sample: %d attr_fields: ['shop', 'level', 'price']
                                   item_id_field: 'item' attr_delimiter: ':' }
    }
    feature_config {
      features { input_names: 'item' feature_type: IdFeature embedding_dim: 4 hash_bucket_size: 100000 }
      features { input_names: 'shop' feature_type: IdFeature embedding_dim: 4 hash_bucket_size: 1000 }
      features { input_names: 'level' feature_type: IdFeature embedding_dim: 4 num_buckets: 10 }
      features { input_names: 'price' feature_type: RawFeature min_val: 10 max_val: 110 }
      features { input_names: 'tags' feature_type: TagFeature embedding_dim: 4 hash_bucket_size: 100 separator: '|' }
    }
  ''' % (batch_size, num_sample), cfg)
  return cfg


ROWS = [(101, 'shop_a', '3', '60'), (7, 'shop_b', '12', '10.5'), (55, '', '0', '110'), (9000000000, 'shop_a', '9', '35'),
        (12, 'shop_c', '-1', '85'), (13, 'shop_d', '4', '20')]


def write_table(path, rows=ROWS, header='id:int64\tweight:float\tfeature:string'):
  with open(path, 'w') as f:
    f.write(header + '\n')
    for item, shop, level, price in rows:
      f.write('%d\t1.0\t%s:%s:%s\n' % (item, shop, level, price))
  return str(path)


def test_table_file_loads_to_the_batch_path_s_columns(ref_backend, tmp_path):
  """the hashed attr through hash_bucket_fast (an empty string: dropped, -1), the identity attr clamped to its buckets,
  the raw attr min/max-normalised in fp32; the id column hashed like the item-id feature's strings"""
  from easyrec_amd.input.neg_sampler import ItemTable
  from oracle import hashing
  cfg = table_config()
  fcs = list(cfg.feature_config.features)
  table = ItemTable.from_file(write_table(tmp_path / 'items.tsv'), cfg.data_config, fcs)

  def hashed(strings, buckets):
    enc = [s.encode() for s in strings]
    offsets = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int64)
    data = np.frombuffer(b''.join(enc), dtype=np.uint8)
    return hashing.hash_bucket_fast(data, offsets, len(enc), np.array([buckets], dtype=np.uint64), True)

  assert table.n == 6 and list(table.columns) == ['shop', 'level', 'price']
  assert np.array_equal(table.ids, hashed([str(r[0]) for r in ROWS], 100000))
  assert np.array_equal(table.columns['shop']['ids'], hashed([r[1] for r in ROWS], 1000)) and table.columns['shop']['ids'][2] == -1
  assert table.columns['level']['ids'].tolist() == [3, 0, 0, 9, 0, 4]
  want = (np.array([60, 10.5, 110, 35, 85, 20], dtype=np.float32) - np.float32(10)) / np.float32(100)
  assert np.array_equal(table.columns['price']['raw'].view(np.uint32), want.view(np.uint32))
  # a file whose header puts the columns elsewhere (found by their prefixes, sampler.py:406-412)
  path = tmp_path / 'swapped.tsv'
  with open(path, 'w') as f:
    f.write('feature:string\tweight:float\tid:int64\n')
    for item, shop, level, price in ROWS:
      f.write('%s:%s:%s\t1.0\t%d\n' % (shop, level, price, item))
  swapped = ItemTable.from_file(str(path), cfg.data_config, fcs)
  assert np.array_equal(swapped.ids, table.ids) and np.array_equal(swapped.columns['level']['ids'], table.columns['level']['ids'])


def build(cfg, **kw):
  from easyrec_amd.input.features import DeviceFeatures, FeatureSchema
  from easyrec_amd.input.neg_sampler import NegativeSampler
  fcs = list(cfg.feature_config.features)
  features = DeviceFeatures(FeatureSchema(cfg.data_config, fcs), 'cpu')
  return NegativeSampler(cfg.data_config, fcs, features, SEED, **kw)


def test_build_time_refusals(ref_backend, tmp_path):
  from easyrec_amd.input.neg_sampler import ItemTable
  path = write_table(tmp_path / 'items.tsv')

  def cfg_with(edit=None, **kw):
    cfg = table_config(**kw)
    cfg.data_config.negative_sampler_in_memory.input_path = path
    if edit:
      edit(cfg.data_config.negative_sampler_in_memory, cfg)
    return cfg
  sampler = build(cfg_with())
  assert sampler.n == 6 and sampler.N == 2 and [c[0] for c in sampler.columns] == ['shop', 'level', 'price']
  with pytest.raises(NotImplementedError, match='tags'):  # a TagFeature among the attr fields
    build(cfg_with(lambda ns, cfg: ns.attr_fields.append('tags')))

  def multi_raw(ns, cfg):
    cfg.feature_config.features[3].raw_input_dim = 3
  with pytest.raises(NotImplementedError, match='price'):
    build(cfg_with(multi_raw))

  def sequence(ns, cfg):
    fc = cfg.feature_config.features[1]
    fc.feature_type = fc.SequenceFeature
  with pytest.raises(NotImplementedError, match='shop'):
    build(cfg_with(sequence))

  def combo(ns, cfg):
    fc = cfg.feature_config.features.add()
    fc.input_names.extend(['shop', 'level'])
    fc.feature_type, fc.hash_bucket_size, fc.embedding_dim = fc.ComboFeature, 100, 4
  with pytest.raises(NotImplementedError, match='shop'):
    build(cfg_with(combo))

  def raw_item_id(ns, cfg):
    ns.item_id_field = 'price'
  with pytest.raises(ValueError, match='item_id_field price'):
    build(cfg_with(raw_item_id))
  with pytest.raises(ValueError, match='num_sample'):
    build(cfg_with(num_sample=0))
  with pytest.raises(ValueError, match='6 rows'):  # n_items < batch_size + num_sample
    build(cfg_with(num_sample=4))

  def eval_sample(ns, cfg):
    ns.num_eval_sample = 1
  with pytest.raises(NotImplementedError, match='num_eval_sample'):
    build(cfg_with(eval_sample))

  def same_eval_sample(ns, cfg):
    ns.num_eval_sample = 2
  assert build(cfg_with(same_eval_sample)).N == 2
  dup = tmp_path / 'dup.tsv'
  write_table(dup, ROWS[:5] + [(101, 'shop_e', '1', '50')])
  cfg = cfg_with()
  cfg.data_config.negative_sampler_in_memory.input_path = str(dup)
  with pytest.raises(ValueError, match='duplicate item ids'):
    build(cfg)
  with pytest.raises(ValueError, match='duplicate item ids'):
    build(cfg_with(), item_table=ItemTable.from_arrays([1, 2, 3, 2, 5, 6], {'shop': np.arange(6), 'level': np.arange(6),
                                                                             'price': np.zeros(6, np.float32)}))
  short = tmp_path / 'short.tsv'
  with open(short, 'w') as f:
    f.write('id:int64\tweight:float\tfeature:string\n1\t1.0\tshop_a:3\n')
  cfg.data_config.negative_sampler_in_memory.input_path = str(short)
  with pytest.raises(ValueError, match='2 attributes'):
    build(cfg)


def test_synthetic_table(ref_backend):
  from easyrec_amd.input.neg_sampler import ItemTable
  cfg = table_config()
  cfg.data_config.negative_sampler_in_memory.attr_fields.insert(0, 'item')
  cfg.data_config.negative_sampler_in_memory.input_path = 'synthetic://500'
  table = ItemTable.load(cfg.data_config, list(cfg.feature_config.features))
  assert table.n == 500 and np.array_equal(table.ids, np.arange(500)) and np.array_equal(table.columns['item']['ids'], table.ids)
  shop, level, price = table.columns['shop']['ids'], table.columns['level']['ids'], table.columns['price']['raw']
  assert 0 <= shop.min() and shop.max() < 1000 and len(set(shop.tolist())) > 300
  assert set(level.tolist()) == set(range(10)) and 0.0 <= price.min() and price.max() < 1.0
  again = ItemTable.load(cfg.data_config, list(cfg.feature_config.features))
  assert np.array_equal(again.columns['shop']['ids'], shop)


# ---------------------------------------------------------------------------------------- the model
def negsam_cfg(B, N, rows, model='dssm'):
  mc = _make_configs()
  base = mc.dssm_taobao(in_batch=True, batch_size=B, scale=0.01) if model == 'dssm' else \
      mc.mind_taobao(list_wise=True, batch_size=B, scale=0.01)
  return mc.with_negative_sampler(base, rows, num_sample=N)


def item_table_for(cfg, rows, seed=3):
  """an ItemTable.from_arrays over the Taobao item fields: distinct adgroup ids out of row order, the other ids uniform
  over their features' buckets"""
  from easyrec_amd.input.neg_sampler import ItemTable
  rng = np.random.default_rng(seed)
  buckets = {fc.input_names[0]: int(fc.hash_bucket_size or fc.num_buckets) for fc in cfg.feature_config.features}
  cols = {}
  for name in cfg.data_config.negative_sampler_in_memory.attr_fields:
    cols[name] = rng.permutation(buckets[name])[:rows].astype(np.int64) if name == 'adgroup_id' else \
        rng.integers(0, buckets[name], size=rows).astype(np.int64)
  return ItemTable.from_arrays(cols['adgroup_id'], cols)


def test_committed_configs_are_the_generated_ones():
  from easyrec_amd.utils import config_util
  mc = _make_configs()
  for name, base in (('dssm', mc.dssm_taobao(in_batch=True, item_rows=10000000)),
                     ('mind', mc.mind_taobao(list_wise=True, item_rows=10000000))):
    cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', name + '_negsam_taobao_10m.config'))
    base.model_dir = 'experiments/%s_negsam_taobao_ckpt' % name
    assert cfg == mc.with_negative_sampler(base, 10000000)
    ns = cfg.data_config.negative_sampler_in_memory
    assert cfg.data_config.WhichOneof('sampler') == 'negative_sampler_in_memory' and ns.num_sample == 1024
    assert ns.input_path == 'synthetic://10000000' and ns.item_id_field == 'adgroup_id'
    item_group = [g for g in cfg.model_config.feature_groups if g.group_name == 'item'][0]
    assert list(ns.attr_fields) == list(item_group.feature_names)


def test_dssm_with_the_sampler_steps_on_the_stand_in(ref_backend, built_lib):
  """tests/test_match_pins.py's step test with the sampler: two steps against the fp64 model oracle drawing from the
  same table (tests/_oracle_steps.first_steps), the item group's rows being B + N; then predict() without and with
  negatives."""
  from easyrec_amd.input.synthetic import SyntheticBatches
  B, N, rows = 16, 8, 301
  cfg = negsam_cfg(B, N, rows)
  table = item_table_for(cfg, rows)

  def check(est, orc, step, batch):
    assert est.model._prediction_dict['item_tower_emb'].shape == (B + N, 32)
    assert est.model._prediction_dict['user_tower_emb'].shape == (B, 32)
    ids = est.features.ids_of('adgroup_id')
    batch_ids = batch['hash_ids'][est.schema.hash_single['adgroup_id']['col']]
    sel = ref.draw(4, step, table.ids, batch_ids, N)
    assert np.array_equal(est.sampler.sel.numpy(), sel.astype(np.int32))
    assert np.array_equal(ids.numpy(), ref.extended(batch_ids, table.columns['adgroup_id']['ids'], sel))
    assert np.array_equal(est.features.ids_of('price').numpy()[B:], table.columns['price']['ids'][sel])
  est = first_steps(cfg, B, seed=4, device='cpu', oracle_dtype=torch.float64, coverage=test_match_pins.dssm_coverage,
                    est_kw=dict(item_table=table), oracle_kw=dict(item_table=table, sampler_seed=4), after_step=check)
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=44)
  # predict() does not sample; predict(sample_negatives=True) is the evaluation mode
  est.model._is_training = est.ctx.is_training = False
  pred = est.predict(gen.next_batch())
  assert pred['item_tower_emb'].shape == (B, 32) and pred['logits'].shape == (B, B)
  assert est.features.ids_of('adgroup_id').shape == (B,)
  pred = est.predict(sample_negatives=True)
  assert pred['item_tower_emb'].shape == (B + N, 32) and pred['logits'].shape == (B, B + N)
  assert pred['user_tower_emb'].shape == (B, 32) and est.features.label('clk').shape == (B,)
  sel = ref.draw(4, 2, table.ids, est.features.batch_ids_of('adgroup_id').numpy(), N)  # (two steps done: step 2's draw)
  assert np.array_equal(est.sampler.sel.numpy(), sel.astype(np.int32))
  metrics = est.model.build_metric_graph(cfg.eval_config)
  assert set(metrics) == {'recall@10', 'recall_neg_sam@10', 'recall_in_batch@10'}
  assert metrics == pytest.approx(mref.recall_at_k(pred['logits'].double().numpy(), 10))
  out = est.model.build_output_dict()
  assert len(out['user_emb']) == B and len(out['item_emb']) == B + N


def test_mind_with_the_sampler_builds_on_the_stand_in(ref_backend, built_lib):
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  B, N, rows = 16, 8, 301
  cfg = negsam_cfg(B, N, rows, model='mind')
  est = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4, item_table=item_table_for(cfg, rows)).build()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=44)
  est.train_step(gen.next_batch())
  assert np.isfinite(list(est.loss_values().values())).all()
  assert est.model._prediction_dict['item_tower_emb'].shape == (B + N, 32)
  assert est.model._prediction_dict['user_tower_emb'].shape == (B, 32)
  est.model._is_training = est.ctx.is_training = False
  est.predict(gen.next_batch(), sample_negatives=True)
  metrics = est.model.build_metric_graph(cfg.eval_config)
  assert {'recall@10', 'recall_neg_sam@10', 'interests_neg_sam_recall@10'} <= set(metrics)


def test_model_refusals(ref_backend):
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  from easyrec_amd.protos.loss_pb2 import LossType
  B, N, rows = 16, 8, 301
  cfg = negsam_cfg(B, N, rows)
  cfg.model_config.loss_type = LossType.CLASSIFICATION
  with pytest.raises(ValueError, match='list-wise loss'):
    EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4, item_table=item_table_for(cfg, rows))
  # a group that mixes attribute fields with other features has no row count
  cfg = negsam_cfg(B, N, rows)
  [g for g in cfg.model_config.feature_groups if g.group_name == 'item'][0].feature_names.append('user_id')
  est = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4, item_table=item_table_for(cfg, rows))
  with pytest.raises(ValueError, match='mixes attribute fields'):
    est.build()
  # a model that is no two-tower model
  cfg = _make_configs().din_taobao(batch_size=B, scale=0.01, seq_len=12)
  _make_configs().with_negative_sampler(cfg, rows, num_sample=N)
  with pytest.raises(NotImplementedError, match='takes no sampled negatives'):
    EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4)
  # bf16 dense stays refused with a sampler
  cfg = negsam_cfg(B, N, rows)
  with pytest.raises(ValueError, match='bf16'):
    EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4, dense_dtype='bf16', item_table=item_table_for(cfg, rows))
