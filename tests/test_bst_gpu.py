"""MultiTowerBST's fused HIP block (csrc/er_bst.hip) on the GPU: forward and every gradient against the fp64 torch
restatement (oracle/bst_ref.py), bit-identity (two runs, eager vs hipGraph replay, accumulation into shared buffers),
and the model's first training steps."""
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from oracle import bst_ref as ref  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical, close, first_steps  # noqa: E402

logging.disable(logging.WARNING)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

# (B, L = max_seq_len, T = seq_len, E, H, lengths or None)
CASES = [
    (6, 12, 8, 32, 4, [0, 1, 7, 12, 20, 3]),     # truncation: T - 1 < L; lengths 0, 1, T-1, L, > L
    (5, 12, 20, 20, 3, [0, 1, 12, 19, 30]),      # padding: T - 1 > L; heads 7, 7, 6
    (4, 4, 5, 9, 6, [0, 4, 2, 9]),               # L == T - 1; 5 heads of widths 2, 2, 2, 2, 1
    (3, 70, 64, 64, 1, [70, 10, 63]),            # the envelope's corner: T = E = 64, one head
    (4096, 50, 50, 32, 4, None),                 # the flagship shape
]


def _device_case(case, seed):
  B, L, T, E, H, lens = case
  key, hist, lens_t, params = ref.random_case(B, L, T, E, H, seed, lengths=lens)
  names = ref.param_names(E, H)
  dev = {n: params[n].to(DEV, torch.float32) for n in names}
  grads = [torch.zeros_like(dev[n]) for n in names]
  return key, hist, lens_t, params, names, dev, grads


def _fused(key, hist, lens, T, H, names, dev, grads, dout):
  k = key.to(DEV, torch.float32).requires_grad_(True)
  h = hist.to(DEV, torch.float32).requires_grad_(True)
  out = kernels.BSTBlockFn.apply(k, h, lens.to(DEV), T, H, grads, *[dev[n] for n in names])
  out.backward(dout)
  torch.cuda.synchronize()
  return out.detach(), k.grad, h.grad


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'B%d_L%d_T%d_E%d_H%d' % c[:5])
def test_kernels_match_the_fp64_restatement(case):
  B, L, T, E, H, _ = case
  key, hist, lens, params, names, dev, grads = _device_case(case, seed=B + T + E)
  dout64 = torch.randn(B, T * E, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
  out, dkey, dhist = _fused(key, hist, lens, T, H, names, dev, grads, dout64.to(DEV, torch.float32))

  k64, h64 = key.clone().requires_grad_(True), hist.clone().requires_grad_(True)
  p64 = {n: t.clone().requires_grad_(True) for n, t in params.items()}
  exp = ref.bst_block(k64, h64, lens, T, H, p64)
  (exp * dout64).sum().backward()

  close(out, exp, 1e-5, 'forward')
  close(dkey, k64.grad, 1e-4, 'dkey')
  close(dhist, h64.grad, 1e-4, 'dhist')
  for n, g in zip(names, grads):
    # the key bias adds the same q . b_k to every score of a row: softmax cancels it and its gradient is zero up to
    # rounding - held against its head's key-kernel gradient instead
    floor = float(p64[n[:-len('bias')] + 'kernel'].grad.abs().max()) if '_key_0/bias' in n else None
    close(g, p64[n].grad, 1e-4, n, floor)


def test_two_runs_and_graph_replay_are_bit_identical():
  case = (1000, 50, 50, 32, 4, None)
  B, L, T, E, H, _ = case
  key, hist, lens, params, names, dev, grads = _device_case(case, seed=3)
  be = kernels.hip()
  k, h, ln = key.to(DEV, torch.float32), hist.to(DEV, torch.float32), lens.to(DEV)
  theta = torch.cat([dev[n].reshape(-1) for n in names])
  dout = torch.randn(B, T * E, device=DEV)
  table = kernels.ThetaGradTable(grads)

  def run():
    for g in grads:
      g.zero_()
    out = be.bst_fwd(k, h, ln, theta, T, H)
    dkey, dhist = be.bst_bwd(k, h, ln, theta, dout, T, H, table)
    return [out, dkey, dhist] + [g.clone() for g in grads]

  assert_runs_and_replay_bit_identical(run)


def test_accumulation_into_filled_buffers():
  case = (300, 12, 8, 20, 3, None)
  B, L, T, E, H, _ = case
  key, hist, lens, params, names, dev, grads = _device_case(case, seed=11)
  be = kernels.hip()
  k, h, ln = key.to(DEV, torch.float32), hist.to(DEV, torch.float32), lens.to(DEV)
  theta = torch.cat([dev[n].reshape(-1) for n in names])
  dout = torch.randn(B, T * E, device=DEV)
  table = kernels.ThetaGradTable(grads)
  dkey, dhist = be.bst_bwd(k, h, ln, theta, dout, T, H, table)
  once = [g.clone() for g in grads]
  # a second tower sharing the variables: its gradient is added in
  be.bst_bwd(k, h, ln, theta, dout, T, H, table)
  assert all(torch.equal(g, a + a) for g, a in zip(grads, once))
  # a gradient buffer that already holds a term (grad_slot: the history's other consumer went first)
  filled = torch.randn_like(h)
  acc = filled.clone()
  be.bst_bwd(k, h, ln, theta, dout, T, H, table, dhist=acc, acc_h=True)
  keep = min(T - 1, L)
  want = filled.clone()
  want[:, :keep] += dhist[:, :keep]
  assert torch.equal(acc, want)
  assert torch.count_nonzero(dhist[:, keep:]) == 0


def _bst_cfg(seq_len=8, towers=1, lazy=False, heads=4):
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'din_taobao_small.config'))
  mc = cfg.model_config
  mc.model_class = 'MultiTowerBST'
  mt = mc.multi_tower
  del mt.din_towers[:]
  groups = [mc.seq_att_groups[0].group_name]
  if towers == 2:  # a second group over the same pairs: its own tables (own scope), the shared dense variables
    g2 = mc.seq_att_groups.add()
    g2.CopyFrom(mc.seq_att_groups[0])
    g2.group_name = 'bst2'
    groups.append('bst2')
  for gname in groups:
    t = mt.bst_towers.add()
    t.input = gname
    t.seq_len = seq_len
    t.multi_head_size = heads
  if lazy:
    oc = cfg.train_config.optimizer_config[0]
    oc.lazy_adam_optimizer.learning_rate.CopyFrom(oc.adam_optimizer.learning_rate)
  return cfg


@pytest.mark.parametrize('seq_len,towers,lazy', [(8, 1, False), (20, 1, True), (8, 2, False)])
def test_model_trains_deterministically(seq_len, towers, lazy):
  """Two estimators from the same seed: bit-identical losses and state after two eager steps."""
  cfg = _bst_cfg(seq_len, towers, lazy)
  runs = []
  for _ in range(2):
    est = EasyRecEstimator(cfg, device=DEV, batch_size=128, seed=5).build()
    gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=128, seed=105)
    losses = []
    for _ in range(2):
      est.train_step(gen.next_batch())
      losses.append(est.loss_values()['total_loss'])
    st = est.state_dict(slots=True)
    runs.append((losses, st))
    assert all(np.isfinite(x) for x in losses)
  (l0, s0), (l1, s1) = runs
  assert l0 == l1
  assert set(s0) == set(s1)
  assert all(np.array_equal(s0[k], s1[k]) for k in s0)
  names = set(s0)
  assert 'multi_head_0_query/multi_head_0_query_0/kernel' in names
  assert ('layer_normalization_3/layer_norm_scale' in names) == (towers == 2)


# ---------------------------------------------------------------------------------------- the reference's own outputs
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'bst_vectors.npz'))
GOLD_CASES = sorted({k.split(':')[0] for k in GOLD.files})


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_kernels_match_the_reference_fixture(tag):
  B, L, T, E, H, towers = [int(v) for v in GOLD['%s:cfg' % tag]]
  var = {k.split(':var:')[1]: torch.from_numpy(GOLD[k]).to(DEV, torch.float32) for k in GOLD.files
         if k.startswith(tag + ':var:')}
  lens = torch.from_numpy(GOLD['%s:len' % tag]).to(DEV, torch.int32)
  for i in range(towers):
    lns = ('layer_normalization' if i == 0 else 'layer_normalization_%d' % (2 * i), 'layer_normalization_%d' % (2 * i + 1))
    names = ref.param_names(E, H, lns)
    theta = torch.cat([var[n].reshape(-1) for n in names])
    key = torch.from_numpy(GOLD['%s:key%d' % (tag, i)]).to(DEV, torch.float32)
    hist = torch.from_numpy(GOLD['%s:hist%d' % (tag, i)]).to(DEV, torch.float32)
    out = kernels.hip().bst_fwd(key, hist, lens, theta, T, H)
    want = GOLD['%s:out%d' % (tag, i)]
    assert np.abs(out.double().cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max(), (tag, i)


# ---------------------------------------------------------------------------------------- the model against the oracle
def _coverage(names, cfg):
  n_bst = sum(k.startswith(('multi_head_', 'layer_normalization', 'feed_forward_net')) for k in names)
  n_emb = sum('embedding_weights' in k for k in names)
  assert n_bst >= 20 and n_emb >= 2, (len(names), n_bst, n_emb)


@pytest.mark.parametrize('seq_len,towers,lazy', [(8, 1, False), (8, 1, True), (20, 1, False), (20, 1, True),
                                                 (8, 2, False)])
def test_model_matches_the_oracle(seq_len, towers, lazy):
  """B = 128, two steps: seq_len 8 truncates the max_seq_len-12 histories, 20 pads them; two towers share the dense
  variables."""
  first_steps(_bst_cfg(seq_len, towers, lazy), 128, 31 + seq_len + towers, coverage=_coverage)


def test_full_size_config_matches_the_oracle():
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'bst_taobao_10m.config'))
  first_steps(cfg, 4096, 8, step0_tol=1e-4, coverage=_coverage)


# ---------------------------------------------------------------------------------------- the static sequence buffer
def _shorten(batch, keep):
  """The same batch with every history cut to at most `keep` items (one length per example for all the group's
  sequences, as the reference's single hist_seq_len assumes), except example 0 (the batch's longest sequence, hence the
  captured graph's shape signature, stays the same)."""
  out = dict(batch)
  names = [k[len('seq/'):-len('/ids')] for k in sorted(batch) if k.startswith('seq/') and k.endswith('/ids')]
  common = np.minimum(np.asarray(batch['seq/%s/len' % names[0]]), keep)
  for name in names:
    ids = np.array(batch['seq/%s/ids' % name], copy=True)
    lens = np.array(batch['seq/%s/len' % name], copy=True)
    t = np.arange(ids.shape[1])[None, :]
    ids[1:] = np.where(t < common[1:, None], np.where(ids[1:] < 0, 1, ids[1:]), -1)
    lens[1:] = common[1:]
    out['seq/%s/ids' % name], out['seq/%s/len' % name] = ids, lens
  return out


def _lengthen(batch):
  out = dict(batch)
  for k in list(batch):
    if k.startswith('seq/') and k.endswith('/ids'):
      name = k[len('seq/'):-len('/ids')]
      ids = np.array(batch[k], copy=True)
      ids[ids < 0] = 1  # every history full
      out[k] = ids
      out['seq/%s/len' % name] = np.full_like(np.asarray(batch['seq/%s/len' % name]), ids.shape[1])
  return out


@pytest.mark.parametrize('graph', [False, True])
def test_short_histories_after_long_ones_see_no_stale_rows(graph, monkeypatch):
  """A step on full-length histories, then one on short ones through the same static buffer (eagerly, and as replays of
  a captured step): the padded rows the kernels read are zero, and the block's output is the restatement of the short
  batch alone.  Both paths give the same losses bit for bit."""
  from easyrec_amd.layers import bst as bst_layer
  cfg = _bst_cfg(seq_len=12)
  B = 128
  seen = {}
  real = bst_layer.bst

  def spy(key, hist, seq_len, seq_size, head_count, ln_index):
    out = real(key, hist, seq_len, seq_size, head_count, ln_index)
    seen.update(key=key, hist=hist, len=seq_len, out=out)
    return out

  monkeypatch.setattr(bst_layer, 'bst', spy)
  losses = {}
  for g in (False, True) if graph else (False,):
    est = EasyRecEstimator(cfg, device=DEV, batch_size=B, seed=12).build()
    gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=112)
    long_b = _lengthen(gen.next_batch())
    short_b = _shorten(gen.next_batch(), 2)
    for k in long_b:
      if k.startswith('seq/') and k.endswith('/len'):
        short_b[k][0] = long_b[k][0]  # (same batch max: the captured step replays)
        short_b[k.replace('/len', '/ids')][0] = long_b[k.replace('/len', '/ids')][0]
    if g:
      est.features.load({k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in long_b.items()})
      est.capture(warmup=0)
      est.train_step()
    else:
      est.train_step(long_b)
    first = est.loss_values()['total_loss']
    torch.cuda.synchronize()
    st = est.state_dict()
    est.train_step(short_b)
    torch.cuda.synchronize()
    losses[g] = (first, est.loss_values()['total_loss'])
    hist = seen['hist'].detach()
    lens = seen['len'].to(torch.int64)
    t = torch.arange(hist.shape[1], device=DEV)[None, :, None]
    assert torch.count_nonzero(hist * (t >= lens[:, None, None])) == 0  # every padded row rewritten with zero
    assert int(lens[1:].max()) <= 2
    E = hist.shape[2]
    params = {n: torch.from_numpy(st[n]).double() for n in ref.param_names(E, 4)}
    Lm = int(lens.max())
    want = ref.bst_block(seen['key'].detach().cpu().double(), hist[:, :Lm].cpu().double(), lens.cpu(), 12, 4, params)
    got = seen['out'].detach().cpu().double()
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
  if graph:
    assert losses[False] == losses[True], losses
