"""Embedding-parallel (row-sharded tables) path on CPU: host logic + collectives.

The HIP kernels are replaced by the CPU oracle backend (tests only); what is under test is the
routing / sharding / exchange logic of layers/sharded_embedding.py, core/comm.py and
model/embedding_parallel.py:
  * world 1 (LocalComm): the sharded engine must reproduce the single-GPU engine exactly;
  * world 2 over gloo (two processes): with the SAME batch on both ranks every embedding row
    receives 2 * g / 2 and every dense gradient (g + g) / 2, so the sharded two-rank run must equal the
    single-process run - a whole-path check of id % world routing, the three all-to-alls, the
    replicated small tables and the 1/world gradient scaling (compat/optimizers.py:315-316).
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'deepfm_criteo_small.config')


def _run_single(cfg, batches, B, seed):
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  est = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=seed).build()
  losses = []
  for b in batches:
    est.train_step(b)
    losses.append(est.loss_values())
  return est.state_dict(slots=True), losses


def _compare(a, b, tol):
  assert set(a) == set(b)
  for k in a:
    d = float(np.max(np.abs(a[k] - b[k]))) if a[k].size else 0.0
    scale = float(np.max(np.abs(b[k]))) + 1e-12
    assert d <= tol * max(scale, 1e-3), (k, d, scale)


def _cfg_and_batches(B, n, optimizer=None, config=None):
  from easyrec_amd.input.criteo_synthetic import SyntheticCriteo
  from easyrec_amd.utils import config_util
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', config) if config else CFG)
  if optimizer == 'lazy':
    oc = cfg.train_config.optimizer_config[0]
    oc.lazy_adam_optimizer.learning_rate.CopyFrom(oc.adam_optimizer.learning_rate)
  feats = list(cfg.feature_config.features)
  gen = SyntheticCriteo(cfg.data_config, feats, batch_size=B, seed=5)
  return cfg, [gen.next_batch() for _ in range(n)]


@pytest.mark.parametrize('optimizer,padded', [(None, True), ('lazy', True), ('lazy', False)])
def test_world1_sharded_engine_equals_single_gpu_engine(ref_backend, optimizer, padded, monkeypatch):
  """padded: the fixed-capacity exchange (equal-split all-to-alls, no host sync); else the compact one."""
  from easyrec_amd.model.embedding_parallel import EmbeddingParallelEstimator
  monkeypatch.setenv('EASYREC_AMD_PADDED_EXCHANGE', '1' if padded else '0')
  B = 32
  cfg, batches = _cfg_and_batches(B, 2, optimizer)
  ref_state, ref_losses = _run_single(cfg, batches, B, seed=3)
  est = EmbeddingParallelEstimator(cfg, device='cpu', batch_size=B, seed=3, rank=0, world=1,
                                   replicate_bytes=1024).build()
  assert any(p[0] == 'rep' for p in est.engine.placement.values())
  assert any(p[0] == 'shard' for p in est.engine.placement.values())
  assert est.engine.padded == padded
  for b, rl in zip(batches, ref_losses):
    est.train_step(b)
    got = est.loss_values()
    for k in rl:
      assert abs(got[k] - rl[k]) <= 1e-6 * max(1.0, abs(rl[k])), (k, got[k], rl[k])
  _compare(est.state_dict(slots=True), ref_state, 1e-6)


def _gloo_worker(rank, world, port, B, optimizer, out_dir, config=None):
  sys.path.insert(0, ROOT)
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  import torch.distributed as dist
  dist.init_process_group('gloo', rank=rank, world_size=world)
  torch.set_num_threads(1)
  from easyrec_amd import kernels
  from oracle.kernel_ref import RefBackend
  kernels._BACKEND = RefBackend()  # CPU stand-in for the HIP kernels (tests only)
  from easyrec_amd.model.embedding_parallel import EmbeddingParallelEstimator
  cfg, batches = _cfg_and_batches(B, 2, optimizer, config)
  est = EmbeddingParallelEstimator(cfg, device='cpu', batch_size=B, seed=3, rank=rank, world=world,
                                   replicate_bytes=1024).build()
  for b in batches:  # the SAME batch on every rank
    est.train_step(b)
  state = est.state_dict(slots=True)  # collective: gathers the shards
  # ... and only chosen rows (unsorted, repeated, spread over both shards), in the order asked for
  picks = {n: np.random.default_rng(5).integers(0, t['rows'], size=37) for n, t in est.engine.tables.items() if not t['kv']}
  rows = est.state_dict(slots=True, rows_of=picks)
  losses = est.loss_values(average=True)
  if rank == 0:
    np.savez(os.path.join(out_dir, 'state.npz'), **{k.replace('/', '|'): v for k, v in state.items()})
    np.savez(os.path.join(out_dir, 'rows.npz'), **{k.replace('/', '|'): v for k, v in rows.items()})
    np.savez(os.path.join(out_dir, 'picks.npz'), **{k.replace('/', '|'): v for k, v in picks.items()})
    np.save(os.path.join(out_dir, 'loss.npy'), np.array([losses['total_loss']]))
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.parametrize('optimizer,padded,config', [
    (None, True, None), ('lazy', True, None), (None, False, None),
    ('lazy', True, 'deepfm_shared_criteo_small.config')])  # ONE table behind all categorical features
def test_world2_gloo_same_batch_equals_single_process(ref_backend, tmp_path, optimizer, padded, config, monkeypatch):
  import torch.multiprocessing as mp
  monkeypatch.setenv('EASYREC_AMD_PADDED_EXCHANGE', '1' if padded else '0')  # (inherited by the spawned ranks)
  B, world = 24, 2
  port = 29500 + (os.getpid() % 2000) + (7 if optimizer else 0) + (13 if padded else 0) + (29 if config else 0)
  mp.spawn(_gloo_worker, args=(world, port, B, optimizer, str(tmp_path), config), nprocs=world, join=True)
  cfg, batches = _cfg_and_batches(B, 2, optimizer, config)
  ref_state, ref_losses = _run_single(cfg, batches, B, seed=3)
  got = {k.replace('|', '/'): v for k, v in np.load(os.path.join(str(tmp_path), 'state.npz')).items()}
  _compare(got, ref_state, 2e-5)
  rows = {k.replace('|', '/'): v for k, v in np.load(os.path.join(str(tmp_path), 'rows.npz')).items()}
  picks = {k.replace('|', '/'): v for k, v in np.load(os.path.join(str(tmp_path), 'picks.npz')).items()}
  assert picks and sorted(rows) == sorted(got)
  for k in got:
    table = k.rsplit('/', 1)[0] if k.endswith(('/m', '/v')) else k
    assert np.array_equal(rows[k], got[k][picks[table]] if table in picks else got[k]), k
  loss = float(np.load(os.path.join(str(tmp_path), 'loss.npy'))[0])
  assert abs(loss - ref_losses[-1]['total_loss']) <= 1e-5 * abs(ref_losses[-1]['total_loss'])


def _gloo_worker_own_batches(rank, world, port, B, steps, lazy, clip, out_dir):
  """like _gloo_worker, but every rank trains on ITS OWN batches (tests/_multi_rank.py rank_batches)"""
  sys.path.insert(0, ROOT)
  sys.path.insert(0, os.path.join(ROOT, 'tests'))
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  import pickle
  import torch.distributed as dist
  dist.init_process_group('gloo', rank=rank, world_size=world)
  torch.set_num_threads(1)
  from easyrec_amd import kernels
  from oracle.kernel_ref import RefBackend
  kernels._BACKEND = RefBackend()  # CPU stand-in for the HIP kernels (tests only)
  from _multi_rank import make_cfg, rank_batches
  from easyrec_amd.model.embedding_parallel import EmbeddingParallelEstimator
  cfg = make_cfg('deepfm_criteo_small.config', lazy=lazy, clip=clip)
  batches = rank_batches(cfg, list(cfg.feature_config.features), B, world, steps)
  est = EmbeddingParallelEstimator(cfg, device='cpu', batch_size=B, seed=4, rank=rank, world=world,
                                   replicate_bytes=1024).build()
  init = est.state_dict()  # collective: rank 0's copy seeds the oracle
  # the order in which the step issues and joins its collectives (the overlap of the dense all-reduce, model/embedding_parallel.py)
  events = []
  comm = est.comm

  def logged(name, fn, note=None):
    def call(*a, **k):
      events.append((name if note is None else note(*a, **k), 'issue'))
      out = fn(*a, **k)
      events.append((name if note is None else note(*a, **k), 'return'))
      return out
    return call

  grad_bufs = {sh['ugrads_all'].data_ptr() for sh in est.engine.shard.values() if sh['leader'] is None}
  comm.all_reduce_sum_async = logged('dense all-reduce (async)', comm.all_reduce_sum_async)
  comm.wait = logged('dense all-reduce joined', comm.wait)
  comm.all_reduce_sum = logged('all-reduce', comm.all_reduce_sum)
  comm.all_to_all_equal = logged('all-to-all', comm.all_to_all_equal,
                                 note=lambda send, recv: 'gradient all-to-all' if send.data_ptr() in grad_bufs else 'all-to-all')
  assert est.overlap == (clip == 0.0)  # (with clipping the buffer's tail needs the sharded reduction: serial order)
  losses, norms = [], []
  for step_batches in batches:
    events.append(('step', 'begin'))
    est.train_step(step_batches[rank])
    losses.append(est.loss_values())
    norms.append(float(est.grad_norm.item()))
  for name in ('all_reduce_sum_async', 'wait', 'all_reduce_sum', 'all_to_all_equal'):
    delattr(comm, name)  # (state_dict's collectives are not the step's)
  state = est.state_dict(slots=True)
  with open(os.path.join(out_dir, 'rank%d.pkl' % rank), 'wb') as f:
    pickle.dump({'init': init if rank == 0 else None, 'state': state, 'losses': losses, 'norms': norms, 'events': events}, f)
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.parametrize('lazy,clip,steps', [(False, 0.0, 1), (True, 0.05, 1), (True, 0.0, 3)])
def test_world2_gloo_own_batches_match_the_w_worker_oracle(ref_backend, tmp_path, lazy, clip, steps):
  """Two PROCESSES over gloo (torch.distributed all-to-alls and all-reduce, not the in-process SimWorld), each rank on
  its own batches, against the oracle's W-worker step: per-rank losses, Adam's first moments after the first update,
  per-rank BatchNorm statistics, the clipped global norm (tests/_multi_rank.py check_against_oracle)."""
  import pickle
  import torch.multiprocessing as mp
  sys.path.insert(0, os.path.join(ROOT, 'tests'))
  from _multi_rank import check_against_oracle, make_cfg, rank_batches
  from oracle.model_oracle import OracleTrainer
  B, world = 24, 2
  port = 33500 + (os.getpid() % 2000) + (3 if lazy else 0) + (5 if clip else 0) + steps
  mp.spawn(_gloo_worker_own_batches, args=(world, port, B, steps, lazy, clip, str(tmp_path)), nprocs=world, join=True)
  ranks = [pickle.load(open(os.path.join(str(tmp_path), 'rank%d.pkl' % r), 'rb')) for r in range(world)]
  cfg = make_cfg('deepfm_criteo_small.config', lazy=lazy, clip=clip)
  batches = rank_batches(cfg, list(cfg.feature_config.features), B, world, steps)
  orc = OracleTrainer(cfg, ranks[0]['init'], batch_size=B)
  exp_losses = [orc.train_step_world(batches[0])]
  orc_first = {k: v.copy() for k, v in orc.slots.items()}
  orc_norm0, moving0 = orc.last_grad_norm, [dict(m) for m in orc.rank_moving]
  for step_batches in batches[1:]:
    exp_losses.append(orc.train_step_world(step_batches))
  results = [(r['state'], r['losses'], r['norms']) for r in ranks]
  check_against_oracle(results, orc, exp_losses, orc_first, orc_norm0, moving0, steps_checked=steps, clip=clip > 0)
  # Overlap (no clipping): in every step of every rank the ONE all-reduce (dense gradients + replicated tables' row sums) is
  # ISSUED (asynchronously, second communicator) before the gradient all-to-all is issued and JOINED only after the
  # all-to-all has returned - the two are in flight together, and with them the sharded half of the local reduction that
  # runs between (it produces what the all-to-all sends).  No other all-reduce in the step.
  for r in ranks:
    ev = r['events']
    starts = [i for i, e in enumerate(ev) if e == ('step', 'begin')] + [len(ev)]
    assert len(starts) - 1 == steps
    for a, b in zip(starts[:-1], starts[1:]):
      step = ev[a:b]
      if clip > 0:
        assert ('dense all-reduce (async)', 'issue') not in step and step.count(('all-reduce', 'issue')) == 1
        continue
      issue = step.index(('dense all-reduce (async)', 'issue'))
      a2a_issue, a2a_done = step.index(('gradient all-to-all', 'issue')), step.index(('gradient all-to-all', 'return'))
      join = step.index(('dense all-reduce joined', 'issue'))
      assert issue < a2a_issue < a2a_done < join, step
      assert step.count(('dense all-reduce (async)', 'issue')) == 1 and step.count(('dense all-reduce joined', 'return')) == 1
      assert ('all-reduce', 'issue') not in step


def test_evaluate_through_the_sharded_engine(ref_backend):
  """EasyRecEstimator.evaluate() on the embedding-parallel estimator: the eval-mode forward goes through the same
  route / exchange / lookup, gives the single-process metrics, and training continues identically afterwards."""
  from easyrec_amd.model.embedding_parallel import EmbeddingParallelEstimator
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  B = 32
  cfg, batches = _cfg_and_batches(B, 3)
  ref = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=3).build()
  est = EmbeddingParallelEstimator(cfg, device='cpu', batch_size=B, seed=3, rank=0, world=1, replicate_bytes=1024).build()
  for b in batches[:2]:
    ref.train_step(b)
    est.train_step(b)
  a, c = ref.evaluate(batches), est.evaluate(batches)
  assert a.keys() == c.keys() and all(abs(a[k] - c[k]) < 1e-6 for k in a), (a, c)
  ref.train_step(batches[2])
  est.train_step(batches[2])
  ra, rc = ref.loss_values(), est.loss_values()
  assert all(abs(ra[k] - rc[k]) <= 1e-6 * max(1.0, abs(ra[k])) for k in ra), (ra, rc)


# ---- hash-table (ev_params) tables under embedding parallelism: the ids travel to their owners (id % world) --------
def _kv_cfg(filtered):
  from easyrec_amd.utils import config_util
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'deepfm_kv_criteo_small.config'))
  if filtered:
    by_name = {f.input_names[0]: f for f in cfg.feature_config.features}
    by_name['C1'].ev_params.filter_freq = 2
    by_name['C2'].ev_params.steps_to_live = 2
  return cfg


def _kv_compare(a, b, names, tol=1e-6):
  for n in names:
    for suffix in ('/keys', '/kv_seen_keys', '/kv_freq', '/kv_version'):
      assert ((n + suffix) in a) == ((n + suffix) in b), (n, suffix)
      if (n + suffix) in a:
        assert np.array_equal(a[n + suffix], b[n + suffix]), (n, suffix)
    for suffix in ('', '/m', '/v'):
      d = float(np.abs(a[n + suffix] - b[n + suffix]).max()) if a[n + suffix].size else 0.0
      assert d <= tol * max(float(np.abs(b[n + suffix]).max()) if b[n + suffix].size else 0.0, 1e-3), (n, suffix, d)


@pytest.mark.parametrize('filtered,padded', [(False, True), (True, True), (False, False)])
def test_world1_sharded_kv_tables_equal_the_single_gpu_engine(ref_backend, filtered, padded, monkeypatch):
  from easyrec_amd.input.criteo_synthetic import SyntheticCriteo
  monkeypatch.setenv('EASYREC_AMD_PADDED_EXCHANGE', '1' if padded else '0')  # (else the compact exchange)
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  from easyrec_amd.model.embedding_parallel import EmbeddingParallelEstimator
  B = 32
  cfg = _kv_cfg(filtered)
  gen = SyntheticCriteo(cfg.data_config, list(cfg.feature_config.features), batch_size=B, seed=13)
  batches = [gen.next_batch() for _ in range(3)]
  unseen = gen.next_batch()  # (one generator: building its Zipf tables is most of this test's time)
  ref = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=3).build()
  est = EmbeddingParallelEstimator(cfg, device='cpu', batch_size=B, seed=3, rank=0, world=1, replicate_bytes=1024).build()
  names = sorted(ref.engine.kv_tables)
  assert names == sorted(est.engine.kv_tables) and all(est.engine.placement[n][0] == 'shard' for n in names)
  assert est.engine.padded == padded
  for b in batches:
    ref.train_step(b)
    est.train_step(b)
    ra, rc = ref.loss_values(), est.loss_values()
    assert all(abs(ra[k] - rc[k]) <= 1e-6 * max(1.0, abs(ra[k])) for k in ra), (ra, rc)
  _kv_compare(est.state_dict(slots=True), ref.state_dict(slots=True), names)
  # evaluation creates no rows; a state loaded into a fresh sharded estimator continues alike
  before = est.state_dict()
  est.evaluate([unseen])
  assert all(np.array_equal(before[n + '/keys'], est.state_dict()[n + '/keys']) for n in names)
  # (same seed: rows created after the load are drawn from the table's generator, whose seed derives from it)
  twin = EmbeddingParallelEstimator(cfg, device='cpu', batch_size=B, seed=3, rank=0, world=1, replicate_bytes=1024).build()
  twin.load_state_dict(est.state_dict(slots=True))
  est.train_step(batches[0])
  twin.train_step(batches[0])
  a, c = est.loss_values(), twin.loss_values()
  assert all(abs(a[k] - c[k]) <= 1e-6 * max(1.0, abs(a[k])) for k in a), (a, c)


def _gloo_worker_kv(rank, world, port, B, steps, filtered, out_dir):
  sys.path.insert(0, ROOT)
  sys.path.insert(0, os.path.join(ROOT, 'tests'))
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  import pickle
  import torch.distributed as dist
  dist.init_process_group('gloo', rank=rank, world_size=world)
  torch.set_num_threads(1)
  from easyrec_amd import kernels
  from oracle.kernel_ref import RefBackend
  kernels._BACKEND = RefBackend()  # CPU stand-in for the HIP kernels (tests only)
  from _multi_rank import rank_batches
  from easyrec_amd.model.embedding_parallel import EmbeddingParallelEstimator
  from test_embedding_parallel import _kv_cfg
  cfg = _kv_cfg(filtered)
  batches = rank_batches(cfg, list(cfg.feature_config.features), B, world, steps)
  est = EmbeddingParallelEstimator(cfg, device='cpu', batch_size=B, seed=4, rank=rank, world=world,
                                   replicate_bytes=1024).build()
  init = est.state_dict()  # collective
  losses, states = [], []
  for step_batches in batches:
    est.train_step(step_batches[rank])
    losses.append(est.loss_values())
    states.append(est.state_dict(slots=True))  # collective
  owned = {n: int(kv_n) for n, kv_n in ((n, len(kv['map'])) for n, kv in est.engine.kv_tables.items())}
  from easyrec_amd.utils import checkpoint
  checkpoint.save(est, os.path.join(out_dir, 'model.ckpt-%d' % est.global_step))  # every rank its part files
  states.append(est.state_dict(slots=True))  # (after the save: steps_to_live evicts when a checkpoint is written)
  with open(os.path.join(out_dir, 'rank%d.pkl' % rank), 'wb') as f:
    pickle.dump({'init': init, 'states': states, 'losses': losses, 'owned': owned}, f)
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.parametrize('filtered', [False, True])
def test_world2_gloo_kv_tables_match_the_w_worker_oracle(ref_backend, tmp_path, filtered):
  """Two processes over gloo, each on its own batches, hash-table tables sharded by id % 2: the ids travel to their
  owners and back (er_kv_bucket / translate / er_kv_unbucket around two all-to-alls), the owners count EVERY rank's
  occurrences towards filter_freq.  Against the oracle's W-worker step after every step: per-rank losses, the ids that
  have a row, the filter's counts and stamps, the rows and Adam's moments by id."""
  import pickle
  import torch.multiprocessing as mp
  sys.path.insert(0, os.path.join(ROOT, 'tests'))
  from _multi_rank import rank_batches
  from oracle.model_oracle import OracleTrainer
  B, world, steps = 24, 2, 2
  port = 35500 + (os.getpid() % 2000) + (7 if filtered else 0)
  mp.spawn(_gloo_worker_kv, args=(world, port, B, steps, filtered, str(tmp_path)), nprocs=world, join=True)
  ranks = [pickle.load(open(os.path.join(str(tmp_path), 'rank%d.pkl' % r), 'rb')) for r in range(world)]
  cfg = _kv_cfg(filtered)
  batches = rank_batches(cfg, list(cfg.feature_config.features), B, world, steps)
  orc = OracleTrainer(cfg, ranks[0]['init'], batch_size=B)
  names = sorted(n for n in orc.kv)
  assert len(names) == 8 and all(min(r['owned'][n] for r in ranks) > 0 for n in names), 'both ranks own ids of every table'
  for step in range(steps):
    exp = orc.train_step_world(batches[step])
    for r in range(world):
      for k, v in exp[r].items():
        got = ranks[r]['losses'][step][k]
        assert abs(got - v) <= 1e-4 * max(1.0, abs(v)), (step, r, k, got, v)
    st = ranks[0]['states'][step]
    for n in names:
      keys, rows = orc.kv_state(n)
      assert np.array_equal(st[n + '/keys'], keys), (step, n, st[n + '/keys'].size, keys.size)
      assert np.array_equal(ranks[1]['states'][step][n + '/keys'], keys), 'state_dict gathers the same table on every rank'
      _, m_rows = orc.kv_state(n, orc.slots[n + '/m'])
      m_scale = float(np.abs(m_rows).max())
      assert float(np.abs(st[n + '/m'] - m_rows).max()) <= 2e-4 * m_scale + 1e-9, (step, n)
      if step == 0:  # (later: Adam's noise amplification on near-zero gradients, tests/test_kv_embedding.py)
        assert float(np.abs(st[n] - rows).max()) <= 2e-4 * float(np.abs(rows).max()) + 1e-5, (step, n)
      if (n + '/kv_seen_keys') in st:
        seen, freq, version = orc.kv_filter_state(n)
        assert np.array_equal(st[n + '/kv_seen_keys'], seen) and np.array_equal(st[n + '/kv_freq'], freq), (step, n)
        assert np.array_equal(st[n + '/kv_version'], version), (step, n)
  # the two ranks' checkpoint parts restored into ONE process: the same table (ids, rows, moments, filter state)
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  from easyrec_amd.utils import checkpoint
  single = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=11).build()
  checkpoint.restore(single, os.path.join(str(tmp_path), 'model.ckpt-%d' % steps))
  _kv_compare(single.state_dict(slots=True), ranks[0]['states'][-1], names, tol=0.0)
