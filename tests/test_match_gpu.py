"""The two-tower head on the GPU: the fused kernels (csrc/er_match.hip) against fp64 autograd of the restatement
(oracle/match_ref.py) on shapes that cross the tiles' edges in rows (32), columns (64) and depth (32 / 64 / 128), every
mask and weight option, the rank counts against a sort, bit identity of runs and graph replays, and both DSSM configs'
first steps.  Tolerances: tests/_oracle_steps.close, 1e-5 forward and 1e-4 gradients."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import match_ref as ref
from _oracle_steps import assert_runs_and_replay_bit_identical, close, first_steps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def fused_head(monkeypatch):
  """The kernels are what is under test, whichever path EASYREC_AMD_FUSED_MATCH makes the default."""
  from easyrec_amd.layers import match_head
  monkeypatch.setattr(match_head, 'fused_match', True)


def make_case(B, extra, D, seed, cosine=False, scale=None, ids=None, ignore=False, weights=False, spread=1.0):
  """fp32 operands (as fp64 tensors holding fp32 values) of one head call"""
  g = torch.Generator().manual_seed(seed)
  M = B + extra
  f32 = lambda t: t.float().double()
  c = dict(U=f32(torch.randn(B, D, generator=g, dtype=torch.float64) * spread),
           I=f32(torch.randn(M, D, generator=g, dtype=torch.float64) * spread),
           inv_t=1.0, sim_w=None, sim_b=None, ids=None, ignore=ignore, w=None, cosine=cosine)
  if cosine:
    c['inv_t'] = 2.0  # temperature 0.5
  if scale is not None:
    c['sim_w'], c['sim_b'] = f32(torch.tensor([scale[0]], dtype=torch.float64)), f32(torch.tensor([scale[1]], dtype=torch.float64))
  if ids == 'dup':
    c['ids'] = torch.randint(0, max(2, B // 3), (M,), generator=g, dtype=torch.int64)
  elif ids == 'all_same':
    c['ids'] = torch.zeros(M, dtype=torch.int64)  # every j != i of every column is a duplicate
  if weights:
    w = torch.rand(B, generator=g, dtype=torch.float64) + 0.5
    w[::3] = 0.0
    if B < 4:
      w[-1] = 1.0
    c['w'] = f32(w)
  return c


def reference(c):
  """fp64: (ce, reg, dU, dI, dsim_w, dsim_b), cosine through the normalisation as the model runs it"""
  leaves = {k: c[k].clone().requires_grad_(True) for k in ('U', 'I')}
  for k in ('sim_w', 'sim_b'):
    if c[k] is not None:
      leaves[k] = c[k].clone().requires_grad_(True)
  u, i = (ref.l2_normalize(leaves['U']), ref.l2_normalize(leaves['I'])) if c['cosine'] else (leaves['U'], leaves['I'])
  ce, reg = ref.list_wise_losses(u, i, c['inv_t'], leaves.get('sim_w'), leaves.get('sim_b'), c['ids'], c['ignore'], c['w'])
  names = list(leaves)
  grads = torch.autograd.grad(ce + reg, [leaves[n] for n in names], allow_unused=True)
  out = {'ce': ce.detach(), 'reg': reg.detach()}
  out.update({'d' + n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, grads)})
  # d(loss)/d(sim_b) = sum_ij dz_ij is zero by the softmax's shift invariance (every row of dz sums to 0): what is left is
  # the rounding of its terms, so its scale is the sum of their magnitudes
  z = ref.logits(u, i, c['inv_t'], leaves.get('sim_w'), leaves.get('sim_b'), c['ids'], c['ignore']).detach().requires_grad_(True)
  hit = ref.hit_prob(z)
  w = torch.ones_like(hit) if c['w'] is None else c['w']
  dz, = torch.autograd.grad(-(torch.log(hit + 1e-12) * w).mean() / w.mean(), z)
  out['_floor_dsim_b'] = float(dz.abs().sum())
  return out


def fused(c, head):
  """the product on the device: head(...) -> (ce, reg); the same outputs as reference()"""
  from easyrec_amd.layers import match_head
  leaves = {k: c[k].float().to(DEV).requires_grad_(True) for k in ('U', 'I')}
  for k in ('sim_w', 'sim_b'):
    if c[k] is not None:
      leaves[k] = c[k].float().to(DEV).requires_grad_(True)
  u, i = (match_head.normalize(leaves['U']), match_head.normalize(leaves['I'])) if c['cosine'] else (leaves['U'], leaves['I'])
  ids = None if c['ids'] is None else c['ids'].to(DEV)
  w = None if c['w'] is None else c['w'].float().to(DEV)
  ce, reg = head(u, i, c['inv_t'], leaves.get('sim_w'), leaves.get('sim_b'), ids, c['ignore'], w)
  (ce + reg).backward()
  out = {'ce': ce.detach(), 'reg': reg.detach()}
  out.update({'d' + n: t.grad for n, t in leaves.items()})
  return out


def check(c, head=None, scale=None):
  from easyrec_amd.layers import match_head
  got, want = fused(c, head or match_head.match_head), reference(c)
  floor_b = want.pop('_floor_dsim_b')
  assert set(got) == set(want)
  for k in want:
    close(got[k], want[k], 1e-4 if k.startswith('d') else 1e-5, k, scale=max(scale or 0.0, floor_b) if k == 'dsim_b' else scale)


# B, M - B, D and one option each: every value of B in {1, 5, 67, 257}, M - B in {0, 3, 130}, D in {4, 32, 33, 128}
HEAD_CASES = {
    'b5_d4': dict(B=5, extra=0, D=4),
    'b5_e3_d33_cosine_negw': dict(B=5, extra=3, D=33, cosine=True, scale=(-1.5, 0.25)),
    'b67_d32_ids': dict(B=67, extra=0, D=32, ids='dup', spread=0.5),
    'b67_e130_d4_scale': dict(B=67, extra=130, D=4, scale=(0.7, -0.1)),
    'b67_e3_d128_weights': dict(B=67, extra=3, D=128, weights=True, spread=0.3),
    # (ignore_in_batch always with extra negatives: without them every row is its positive alone, hit = 1 and the loss
    # log(1 + 1e-12) is below fp32's resolution - test_single_logit covers that shape of case)
    'b257_e3_d33_ignore': dict(B=257, extra=3, D=33, ignore=True, spread=0.5),
    'b257_e130_d32_ids_weights': dict(B=257, extra=130, D=32, ids='dup', weights=True, scale=(1.0, 0.0), spread=0.5),
    'b257_d128_cosine': dict(B=257, extra=0, D=128, cosine=True, scale=(2.0, 0.5)),
    'b5_e130_d32_all_dup': dict(B=5, extra=130, D=32, ids='all_same', spread=0.5),
    'b1_e3_d4': dict(B=1, extra=3, D=4),
    'b67_e130_d64_ignore': dict(B=67, extra=130, D=64, ignore=True, weights=True, spread=0.4),
    'b5_d32_zero_w': dict(B=5, extra=0, D=32, scale=(0.0, 0.1)),  # sign(0) = 0: no gradient reaches sim_w
}


@pytest.mark.parametrize('tag', sorted(HEAD_CASES))
def test_head_matches_fp64_autograd(built_lib, tag):
  check(make_case(seed=11, **HEAD_CASES[tag]))


def test_single_logit(built_lib):
  """B = M = 1: hit = 1, every gradient of the softmax is 0 (the reg_pos_loss term stays)"""
  c = make_case(1, 0, 4, seed=3, scale=(1.5, 0.2))
  c['U'], c['I'] = c['U'].abs(), c['I'].abs()  # a positive similarity: no reg_pos_loss gradient either
  want = reference(c)
  assert float(want['dU'].abs().max()) < 1e-9 and abs(float(want['ce'])) < 1e-9
  check(c, scale=1.0)


def test_tiny_hit_probability(built_lib):
  """A positive about 28 below its row's best negative: hit is of the order of 1e-12 and hit / (hit + 1e-12) decides
  the row's gradient."""
  c = make_case(5, 3, 4, seed=5, spread=0.3)
  c['U'][0] = torch.tensor([3.0, 0, 0, 0], dtype=torch.float64)
  c['I'][0] = torch.tensor([-5.0, 0, 0, 0], dtype=torch.float64)
  c['I'][1] = torch.tensor([13.0 / 3, 0, 0, 0], dtype=torch.float64).float().double()
  hit = ref.hit_prob(ref.logits(c['U'], c['I']))
  factor = float(hit[0] / (hit[0] + 1e-12))
  assert 0.1 < factor < 0.9, factor
  check(c)


def test_normalize_with_a_zero_row(built_lib):
  from easyrec_amd.layers import match_head
  g = torch.Generator().manual_seed(2)
  for R, D in [(7, 33), (130, 4), (5, 200)]:
    x = torch.randn(R, D, generator=g, dtype=torch.float64).float().double()
    x[1] = 0.0
    dy = torch.randn(R, D, generator=g, dtype=torch.float64).float().double()
    xr = x.clone().requires_grad_(True)
    want = ref.l2_normalize(xr)
    want_dx, = torch.autograd.grad(want, xr, dy)
    xg = x.float().to(DEV).requires_grad_(True)
    got = match_head.normalize(xg)
    got.backward(dy.float().to(DEV))
    assert torch.isfinite(got).all() and torch.isfinite(xg.grad).all()
    close(got, want.detach(), 1e-5, 'y')
    close(xg.grad, want_dx, 1e-4, 'dx')
    close(xg.grad[1], want_dx[1], 1e-5, 'dx of the zero row')


def _tied_case(B, extra, D, seed):
  """small integer operands: many exactly equal logits, also with the diagonal"""
  g = torch.Generator().manual_seed(seed)
  U = torch.randint(-1, 2, (B, D), generator=g).double()
  I = torch.randint(-1, 2, (B + extra, D), generator=g).double()
  I[B // 2] = I[0]
  return U, I


@pytest.mark.parametrize('B,extra,D,opt', [(5, 0, 4, None), (67, 130, 4, 'ids'), (257, 3, 33, None), (67, 3, 128, 'ignore'),
                                           (1, 0, 4, None), (257, 130, 32, 'scale')])
def test_rank_counts_match_a_sort(built_lib, B, extra, D, opt):
  from easyrec_amd.layers import match_head
  U, I = _tied_case(B, extra, D, seed=B + D)
  ids = torch.randint(0, max(2, B // 3), (B + extra,), generator=torch.Generator().manual_seed(1)) if opt == 'ids' else None
  sw, sb = (torch.tensor([-2.0]), torch.tensor([0.5])) if opt == 'scale' else (None, None)
  z = ref.logits(U, I, 1.0, None if sw is None else sw.double(), None if sb is None else sb.double(), ids, opt == 'ignore')
  want_in, want_neg = ref.rank_counts(z.numpy())
  dev = lambda t: None if t is None else t.to(DEV)
  c_in, c_neg = match_head.rank_counts(U.float().to(DEV), I.float().to(DEV), 1.0, dev(sw), dev(sb), dev(ids),
                                       opt == 'ignore')
  assert c_in.dtype == torch.int32
  assert np.array_equal(c_in.cpu().numpy(), want_in) and np.array_equal(c_neg.cpu().numpy(), want_neg)
  assert len(np.unique(z.numpy()[0])) < z.shape[1] or B == 1  # (the case does have ties)
  for k in (1, 3, 10):
    got, want = match_head.recall_at_k(c_in, c_neg, k), ref.recall_at_k(z.numpy(), k)
    assert got == pytest.approx(want, abs=1e-12), k


def test_runs_and_graph_replay_are_bit_identical(built_lib):
  from easyrec_amd import kernels
  be = kernels.hip()
  c = make_case(1001, 130, 32, seed=9, ids='dup', weights=True, scale=(-1.2, 0.3), spread=0.4)
  U, I = c['U'].float().to(DEV), c['I'].float().to(DEV)
  sw, sb, ids, w = c['sim_w'].float().to(DEV), c['sim_b'].float().to(DEV), c['ids'].to(DEV), c['w'].float().to(DEV)
  one = torch.ones(1, device=DEV)

  def run():
    losses, stats = be.match_softmax_fwd(U, I, 1.0, sw, sb, ids, False, w)
    dw, db = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
    dU, dI = be.match_softmax_bwd(U, I, 1.0, sw, sb, ids, False, w, stats, losses, one, one,
                                  kernels.ThetaGradTable([dw, db]), acc=False)
    c_in, c_neg = be.match_rank_counts(U, I, 1.0, sw, sb, ids, False)
    y, inv = be.match_normalize_fwd(U)
    return [losses, stats, dU, dI, dw, db, c_in, c_neg, y, be.match_normalize_bwd(U, inv, dU)]

  assert_runs_and_replay_bit_identical(run)


def test_outside_the_envelope_is_composed(built_lib):
  """D = 129: no kernel takes it; the same head from torch ops still matches"""
  from easyrec_amd.layers import match_head
  assert match_head.lds_bytes(129) == 0 and not match_head.fused(torch.zeros(2, 129, device=DEV))
  check(make_case(67, 3, 129, seed=4, ids='dup', scale=(1.1, 0.1), spread=0.3))


def test_composition_matches_too(built_lib):
  from easyrec_amd.layers import match_head
  check(make_case(67, 3, 32, seed=4, ids='dup', weights=True, scale=(-1.1, 0.1), spread=0.5),
        head=match_head.match_head_compose)


# ---------------------------------------------------------------------------------------- the model
def _configs():
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  return make_configs


@pytest.mark.parametrize('in_batch', [False, True])
def test_model_first_steps(built_lib, in_batch):
  """Two steps of a DSSM config at small table sizes, B = 67, against the fp64 model oracle from the batch on
  (tests/_oracle_steps.first_steps: every loss, the tower embeddings or logits, every variable's first moment)."""
  first_steps(_configs().dssm_taobao(in_batch=in_batch, batch_size=67, scale=0.01), 67, seed=5, oracle_dtype=torch.float64,
              coverage=pins.dssm_coverage)


# ---------------------------------------------------------------------------------------- the reference's own outputs
import test_match_pins as pins  # noqa: E402  (the fixture readers, configs and coverage sets shared with the CPU tests)

LIST_WISE_GOLD = [t for t in pins.GOLD_CASES if pins.gold_case(t)[0]['loss'] == 'SOFTMAX_CROSS_ENTROPY']


@pytest.mark.parametrize('tag', pins.GOLD_CASES)
def test_fixture_cases_through_the_kernels(built_lib, tag):
  """The reference's own tower outputs, normalised embeddings, losses and rank order, from the kernels."""
  from easyrec_amd.layers import match_head
  from easyrec_amd.protos.simi_pb2 import Similarity
  o, head, loss_type, arr, var = pins.gold_case(tag)
  ids, w, ignore = pins.gold_head_args(o, arr)
  u, i = [t.float().to(DEV) for t in pins.gold_towers(o, arr, var)]
  inv_t = 1.0
  if head.simi_func == Similarity.COSINE:
    u, i, inv_t = match_head.normalize(u), match_head.normalize(i), 1.0 / head.temperature
  close(u, arr['user_tower_emb'], 1e-5, 'user_tower_emb')
  close(i, arr['item_tower_emb'], 1e-5, 'item_tower_emb')
  if tag not in LIST_WISE_GOLD:
    return
  dev = lambda t: None if t is None else t.to(DEV)
  sw, sb = (var['sim_w'].float().to(DEV), var['sim_b'].float().to(DEV)) if head.scale_simi else (None, None)
  assert match_head.fused(u)
  ce, reg = match_head.match_head(u, i, inv_t, sw, sb, dev(ids), ignore, None if w is None else w.float().to(DEV))
  close(ce, arr['loss:cross_entropy_loss'], 1e-5, 'cross_entropy_loss')
  close(reg, arr['loss:reg_pos_loss'], 1e-5, 'reg_pos_loss', scale=1e-3)
  c_in, c_neg = match_head.rank_counts(u, i, inv_t, sw, sb, dev(ids), ignore)
  want_in, want_neg = ref.rank_counts(arr['logits'].numpy())
  assert np.array_equal(c_in.cpu().numpy(), want_in) and np.array_equal(c_neg.cpu().numpy(), want_neg)


@pytest.mark.parametrize('kind', ['backbone', 'l2'])
def test_backbone_and_l2_first_steps(built_lib, kind):
  """MatchModel over a backbone (fused list-wise head, temperature 0.01) and the point-wise L2 head on the device."""
  cfg, coverage = (pins.backbone_cfg(67), pins.backbone_coverage) if kind == 'backbone' else (pins.l2_cfg(67), pins.dssm_coverage)
  first_steps(cfg, 67, seed=5, oracle_dtype=torch.float64, coverage=coverage)
