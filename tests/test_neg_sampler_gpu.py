"""negative_sampler_in_memory on the GPU: er_neg_sample (csrc/er_sampler.hip) against the numpy restatement
(oracle/neg_sampler_ref.py) bit for bit - sel and every extended column - over table sizes at and above B + N, the
largest envelope batch, repeated runs, a captured graph replayed over three steps, the composed path outside the
envelope; DSSM's and MIND's first steps with sampled negatives against their fp64 restatements at the bars of
tests/test_match_gpu.py and tests/test_mind_gpu.py; the recall metrics over B + N columns."""
import numpy as np
import pytest
import torch

import test_match_pins
import test_mind_pins
import test_neg_sampler_pins as pins
from _oracle_steps import first_steps
from oracle import match_ref as mref
from oracle import neg_sampler_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def run_and_check(sampler, features, cols, batch, counter, step):
  counter.fill_(step + 1)
  sampler.run(counter, -1)
  torch.cuda.synchronize()
  return pins.assert_draw_is_the_restatement(sampler, features, cols, batch, step)


# (5000, 4096, 130): the largest envelope batch - the LDS set half full, more than 64 KiB of LDS, five chunks of candidates
@pytest.mark.parametrize('kind', ['duplicates', 'some_absent', 'only_absent'])
@pytest.mark.parametrize('n,B,N', pins.CASES + [(5000, 4096, 130)])
def test_kernel_equals_the_restatement(built_lib, n, B, N, kind):
  sampler, features, cols = pins.sampler_on(DEV, n, B, N)
  assert sampler.uses_kernel()
  batch = pins.load_batch(features, pins.batch_ids_of(kind, cols['item'], B))
  counter = torch.zeros(1, dtype=torch.int64, device=DEV)
  for step in (0, 1, 5000000000):
    run_and_check(sampler, features, cols, batch, counter, step)


def test_an_id_that_equals_the_empty_mark(built_lib):
  """INT64_MIN marks an empty slot of the LDS set: a table row with that id is still excluded exactly when the batch
  holds it, and eligible when it does not"""
  n, B, N = 107, 67, 40
  sampler, features, cols = pins.sampler_on(DEV, n, B, N)
  lowest = np.iinfo(np.int64).min
  cols['item'][5] = lowest  # (the host copy the restatement and the composition read)
  sampler.table_ids[5] = lowest
  assert sampler.columns[0][:2] == ('item', 'ids')
  sampler.columns[0][2][5] = lowest
  counter = torch.zeros(1, dtype=torch.int64, device=DEV)
  drawn = []
  for member in (True, False):
    ids = pins.batch_ids_of('only_absent', cols['item'], B)
    if member:
      ids[3] = lowest
    batch = pins.load_batch(features, ids)
    want = run_and_check(sampler, features, cols, batch, counter, 2)
    drawn.append(5 in want.tolist())
  assert drawn == [False, True]  # (no other id is excluded, and row 5 is among P(0) .. P(N - 1) at step 2)


def test_two_runs_are_bit_identical(built_lib):
  sampler, features, cols = pins.sampler_on(DEV, 5000, 4096, 130)
  pins.load_batch(features, pins.batch_ids_of('duplicates', cols['item'], 4096))
  counter = torch.full((1,), 8, dtype=torch.int64, device=DEV)
  outs = []
  for _ in range(2):
    sampler.run(counter, -1)
    outs.append([sampler.sel.clone()] + [buf.clone() for _, _, _, buf in sampler.columns])
    sampler.sel.fill_(-1)
    for _, _, _, buf in sampler.columns:
      buf.zero_()
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(*outs)) and int(outs[0][0].min()) >= 0


def test_a_replayed_graph_draws_the_next_steps(built_lib):
  """The step is read on the device: a graph captured at one step and replayed three times gives the restatement's
  draws for steps s, s + 1, s + 2 (a step number baked in at capture would give the same rows three times)."""
  n, B, N = 301, 67, 40
  sampler, features, cols = pins.sampler_on(DEV, n, B, N)
  batch = pins.load_batch(features, pins.batch_ids_of('some_absent', cols['item'], B))
  counter = torch.zeros(1, dtype=torch.int64, device=DEV)

  def step_fn():
    counter.add_(1)  # (the prologue's part)
    sampler.run(counter, -1)
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    step_fn()  # step 0, eager
  torch.cuda.current_stream().wait_stream(s)
  torch.cuda.synchronize()
  pins.assert_draw_is_the_restatement(sampler, features, cols, batch, 0)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    step_fn()
  seen = []
  for step in (1, 2, 3):
    graph.replay()
    torch.cuda.synchronize()
    assert int(counter.item()) == step + 1
    seen.append(pins.assert_draw_is_the_restatement(sampler, features, cols, batch, step).tolist())
  assert seen[0] != seen[1] != seen[2]


def test_outside_the_envelope_is_composed(built_lib):
  from easyrec_amd.input import neg_sampler
  n, B, N = 4200, 4097, 40
  assert neg_sampler.lds_bytes(B) == 0
  sampler, features, cols = pins.sampler_on(DEV, n, B, N)
  assert not sampler.uses_kernel()
  batch = pins.load_batch(features, pins.batch_ids_of('some_absent', cols['item'], B))
  counter = torch.zeros(1, dtype=torch.int64, device=DEV)
  run_and_check(sampler, features, cols, batch, counter, 3)


def test_switch_selects_the_composition(built_lib, monkeypatch):
  from easyrec_amd.input import neg_sampler
  sampler, features, cols = pins.sampler_on(DEV, 301, 67, 40)
  monkeypatch.setattr(neg_sampler, 'device_sampler', False)
  assert not sampler.uses_kernel()
  batch = pins.load_batch(features, pins.batch_ids_of('duplicates', cols['item'], 67))
  run_and_check(sampler, features, cols, batch, torch.zeros(1, dtype=torch.int64, device=DEV), 1)


# ---------------------------------------------------------------------------------------- the models
B, N, ROWS = 67, 40, 301


def _estimator(model):
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  cfg = pins.negsam_cfg(B, N, ROWS, model=model)
  table = pins.item_table_for(cfg, ROWS)
  est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=5, item_table=table).build()
  assert est.sampler.uses_kernel()
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=105)
  return cfg, table, est, gen


def _first_steps(model, coverage, after_step=None):
  """first_steps of a config with the sampler (seed 5, the fp64 oracle drawing from the same table); after each of the
  product's steps: the item group had B + N rows, the draw and - after the first - the trained rows are the restatement's"""
  cfg = pins.negsam_cfg(B, N, ROWS, model=model)
  table = pins.item_table_for(cfg, ROWS)

  def check(est, orc, step, batch):
    assert est.sampler.uses_kernel()
    pd = est.model._prediction_dict
    assert pd['item_tower_emb'].shape[0] == B + N and pd['user_tower_emb'].shape[0] == B
    assert est.features.ids_of('adgroup_id').shape == (B + N,)
    _check_the_draw_and_the_trained_rows(cfg, table, est, batch, step, est.state_dict(slots=True) if step == 0 else None)
    if after_step is not None:
      after_step(est, orc, step, batch)
  est = first_steps(cfg, B, seed=5, oracle_dtype=torch.float64, coverage=coverage, est_kw=dict(item_table=table),
                    oracle_kw=dict(item_table=table, sampler_seed=5), after_step=check)
  return cfg, table, est


def _check_the_draw_and_the_trained_rows(cfg, table, est, batch, step, st=None):
  """the step's extended columns are the restatement's; with `st` (the state after step one): for each item-side
  embedding table the rows with a nonzero first moment are exactly the ids of the extended column - positives and
  negatives (a dropped id, -1, has no row)"""
  batch_ids = batch['hash_ids'][est.schema.hash_single['adgroup_id']['col']]
  sel = ref.draw(5, step, table.ids, batch_ids, N)
  assert np.array_equal(est.sampler.sel.cpu().numpy(), sel.astype(np.int32))
  for name in cfg.data_config.negative_sampler_in_memory.attr_fields:
    sch = est.schema
    own = batch['hash_ids'][sch.hash_single[name]['col']] if name in sch.hash_single else \
        batch['int_ids'][sch.int_single[name]['col']]
    ext = ref.extended(own, table.columns[name]['ids'], sel)
    assert np.array_equal(est.features.ids_of(name).cpu().numpy(), ext), name
    if st is None:
      continue
    key = [k for k in st if k.endswith('/%s_embedding/embedding_weights/m' % name)]
    assert len(key) == 1, (name, key)
    touched = set(np.nonzero(np.abs(st[key[0]]).max(axis=1))[0].tolist())
    assert touched == set(int(v) for v in ext.tolist() if v >= 0), name
    if name == 'adgroup_id':  # (the exclusion: every negative's row is touched by the negatives alone)
      assert not set(int(v) for v in ext[B:].tolist()) & set(int(v) for v in ext[:B].tolist())


def test_dssm_first_steps_with_sampled_negatives(built_lib):
  """tests/test_match_gpu.py test_model_first_steps with the sampler: B = 67, N = 40, a 301-row table, two steps."""
  _first_steps('dssm', test_match_pins.dssm_coverage)


def test_mind_first_steps_with_sampled_negatives(built_lib, monkeypatch):
  """tests/test_mind_gpu.py test_model_first_steps (list-wise) with the sampler, then the step as a hipGraph: each
  replay draws the next step's negatives."""
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.layers import capsule_layer
  monkeypatch.setattr(capsule_layer, 'fused_capsule', True)
  cfg, table, est = _first_steps('mind', test_mind_pins.mind_coverage, test_mind_pins.hand_over_routing_logits())
  # the captured step (capture() warms up over three steps: 2, 3, 4; the replays are steps 5 and 6)
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=105)
  est.capture()
  for step in (5, 6):
    batch = gen.next_batch()
    est.train_step(batch)
    torch.cuda.synchronize()
    assert est.graph is not None and est.global_step == step + 1
    _check_the_draw_and_the_trained_rows(cfg, table, est, batch, step)


def test_recall_metrics_over_the_sampled_columns(built_lib):
  cfg, table, est, gen = _estimator('dssm')
  est.train_step(gen.next_batch())
  est.model._is_training = est.ctx.is_training = False
  pred = est.predict(gen.next_batch())
  assert pred['item_tower_emb'].shape == (B, 32) and pred['logits'].shape == (B, B)
  pred = est.predict(gen.next_batch(), sample_negatives=True)
  assert pred['item_tower_emb'].shape == (B + N, 32) and pred['logits'].shape == (B, B + N)
  metrics = est.model.build_metric_graph(cfg.eval_config)
  u, i = pred['user_tower_emb'].double().cpu(), pred['item_tower_emb'].double().cpu()
  st = est.state_dict()
  z = mref.logits(u, i, 1.0, torch.from_numpy(st['sim_w']).double(), torch.from_numpy(st['sim_b']).double(),
                  est.features.ids_of('adgroup_id').cpu())
  want = mref.recall_at_k(z.numpy(), 10)
  assert set(metrics) == {'recall@10', 'recall_neg_sam@10', 'recall_in_batch@10'}
  assert metrics == pytest.approx(want, abs=1e-12)
