"""MIND on the GPU: the capsule-routing and label-aware attention kernels (csrc/er_capsule.hip) against fp64 autograd of
the restatement (oracle/mind_ref.py) over the envelope's edges, bit identity of runs and graph replays, the composed path
outside the envelope, and both MIND configs' first steps.  Tolerances: tests/_oracle_steps.close, 1e-5 forward and 1e-4
gradients."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import mind_ref as ref
from _oracle_steps import assert_runs_and_replay_bit_identical, close, first_steps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
EDGE_LENS = [0, 1, 2, 7, 8, 20, 21, 54, 55]  # + S + 3: every step of the capsule count, an empty and an overlong row


@pytest.fixture(autouse=True)
def fused_path(monkeypatch):
  """The kernels are what is under test, whichever path EASYREC_AMD_FUSED_CAPSULE makes the default."""
  from easyrec_amd.layers import capsule_layer
  monkeypatch.setattr(capsule_layer, 'fused_capsule', True)


# One option varies per case.  Between them: B in {1, 5, 67}; (S, L) in {(1, 1), (7, 7), (64, 64), (50, 70), (50, 40),
# (128, 128)}; D in {4, 16, 33, 128}; E in {4, 33, 64, 128}; K in {1, 3, 5, 8}; num_iters in {1, 2, 3}; scale 20 and 0;
# const_caps_num; squash_pow 0.5; acc on dhist; shared and per-example logits0; with B = 67 the length vector starts with
# EDGE_LENS and S + 3.
#
# Every case keeps the default bars.  With scale 20 the routing softmax multiplies the rounding of the logits by up to 20
# per iteration, so the same ops in fp32 torch on the CPU (layers/capsule_layer.py capsule_compose) were measured against
# fp64 on each of these cases: the largest error over the largest value is 2.0e-6 on high_capsules (b67_taobao_shared),
# 2.4e-6 on dhist (b67_taobao_shared) and 5.3e-7 on dSmat (b67_squash_half) - inside 1e-5 / 1e-4 with room for another
# summation order, so no case needs a bar of its own.  tests/test_mind_pins.py repeats that measurement.
CAPSULE_CASES = {
    'b1_s1': dict(B=1, S=1, L=1, D=4, E=4, K=1, iters=1),
    'b5_s7_k3_iters2': dict(B=5, S=7, L=7, D=4, E=33, K=3, iters=2),
    'b67_taobao': dict(B=67, S=64, L=64, D=16, E=64, K=5, iters=3),
    'b67_taobao_shared': dict(B=67, S=64, L=64, D=16, E=64, K=5, iters=3, shared=True),
    'b67_scale0': dict(B=67, S=64, L=64, D=16, E=64, K=5, iters=3, scale=0.0),
    'b67_const_caps': dict(B=67, S=64, L=64, D=16, E=64, K=5, iters=3, const=True),
    'b67_squash_half': dict(B=67, S=64, L=64, D=16, E=64, K=5, iters=3, squash_pow=0.5, scale_ratio=2.0),
    'b67_acc': dict(B=67, S=64, L=64, D=16, E=64, K=5, iters=3, acc=True),
    'b67_clip_l70': dict(B=67, S=50, L=70, D=33, E=33, K=5, iters=3),
    'b67_pad_l40': dict(B=67, S=50, L=40, D=33, E=4, K=3, iters=2, acc=True),
    'b5_corner': dict(B=5, S=128, L=128, D=128, E=128, K=8, iters=3),
    'b67_s128_k8': dict(B=67, S=128, L=128, D=4, E=64, K=8, iters=3, shared=True),
    'b5_iters1': dict(B=5, S=64, L=64, D=16, E=64, K=5, iters=1),
}


def capsule_case(B, S, L, D, E, K, iters, scale=20.0, const=False, squash_pow=1.0, scale_ratio=1.0, acc=False,
                 shared=False, seed=21):
  """fp32 operands (as fp64 tensors holding fp32 values) of one capsule call"""
  g = torch.Generator().manual_seed(seed)
  f32 = lambda t: t.float().double()
  lens = torch.randint(0, S + 4, (B,), generator=g)
  edge = [v for v in EDGE_LENS + [S + 3]]
  if B >= len(edge):
    lens[:len(edge)] = torch.tensor(edge)
  elif B > 1:
    lens[0], lens[1] = S + 3, 1
  else:
    lens[0] = S
  return dict(hist=f32(torch.randn(B, L, D, generator=g, dtype=torch.float64) * 0.5),  # rows past the length hold data too
              lens=lens.to(torch.int32), Smat=f32(torch.randn(D, E, generator=g, dtype=torch.float64) / D ** 0.5),
              logits0=f32(torch.clamp(torch.randn(*((S, K) if shared else (B, S, K)), generator=g, dtype=torch.float64), -2, 2)),
              d_high=f32(torch.randn(B, K, E, generator=g, dtype=torch.float64)),
              dhist0=f32(torch.randn(B, L, D, generator=g, dtype=torch.float64)),
              cfg=(S, K, iters, scale, squash_pow, scale_ratio, const), acc=acc)


def capsule_reference(c, fn=ref.capsule, dtype=torch.float64):
  """(high_capsules, num_caps, dhist, dSmat) by autograd of `fn` in `dtype`"""
  S, K, iters, scale, squash_pow, scale_ratio, const = c['cfg']
  hist = c['hist'].to(dtype).clone().requires_grad_(True)  # (a copy: the case's own tensors stay leaves without a graph)
  Smat = c['Smat'].to(dtype).clone().requires_grad_(True)
  high, ncaps = fn(hist, c['lens'], Smat, c['logits0'].to(dtype), S, K, iters, scale, squash_pow, scale_ratio, const)
  dhist, dS = torch.autograd.grad(high, [hist, Smat], c['d_high'].to(dtype))
  return high.detach(), ncaps, dhist, dS


def valid_rows(c):
  """[B, L] bool: the rows of hist that reach the capsules"""
  S, L = c['cfg'][0], c['hist'].shape[1]
  n = torch.clamp(c['lens'].to(torch.int64), 0, min(S, L))
  return torch.arange(L)[None, :] < n[:, None]


def check_capsule(tag, c):
  from easyrec_amd import kernels
  be = kernels.hip()
  S, K, iters, scale, squash_pow, scale_ratio, const = c['cfg']
  want_high, want_n, want_dh, want_dS = capsule_reference(c)
  dev = lambda t: t.float().to(DEV).contiguous()
  hist, Smat, lens = dev(c['hist']), dev(c['Smat']), c['lens'].to(DEV)
  assert be.capsule_lds_bytes(S, hist.shape[2], Smat.shape[1], K) > 0
  high, ncaps, W = be.capsule_fwd(hist, lens, Smat, dev(c['logits0']), S, K, iters, scale, squash_pow, scale_ratio, const)
  dS = torch.full_like(Smat, float('nan'))
  buf = dev(c['dhist0']) if c['acc'] else None
  dhist = be.capsule_bwd(hist, lens, Smat, W, dev(c['d_high']), squash_pow, scale_ratio, const,
                         kernels.ThetaGradTable([dS]), dhist=buf, acc_h=c['acc'], acc=False)
  fwd_tol, grad_tol = 1e-5, 1e-4
  errs = {}
  for name, got, want in (('high', high, want_high), ('dhist', dhist.double().cpu() - (c['dhist0'] if c['acc'] else 0),
                                                     want_dh), ('dSmat', dS, want_dS)):
    w = want.double().numpy()
    errs[name] = float(np.abs(got.double().cpu().numpy() - w).max() / max(np.abs(w).max(), 1e-30))
  print('capsule case %s: max error / max value %s' % (tag, errs))
  assert np.array_equal(ncaps.cpu().numpy(), want_n.numpy().astype(np.int32)) and ncaps.dtype == torch.int32
  close(high, want_high, fwd_tol, 'high_capsules')
  if c['acc']:
    close(dhist.double().cpu() - c['dhist0'], want_dh, grad_tol, 'dhist (accumulated)')
  else:
    close(dhist, want_dh, grad_tol, 'dhist')
  close(dS, want_dS, grad_tol, 'dSmat')
  # rows past the valid length: exactly zero (written), exactly untouched (accumulated)
  dead = ~valid_rows(c)
  base = c['dhist0'].float() if c['acc'] else torch.zeros_like(c['dhist0']).float()
  assert torch.equal(dhist.cpu()[dead], base[dead])
  rows = torch.arange(S)[None, :] >= torch.clamp(c['lens'].to(torch.int64), 0, S)[:, None]
  assert float(W.cpu()[rows].abs().max() if rows.any() else 0.0) == 0.0


@pytest.mark.parametrize('tag', sorted(CAPSULE_CASES))
def test_capsule_matches_fp64_autograd(built_lib, tag):
  check_capsule(tag, capsule_case(**CAPSULE_CASES[tag]))


def test_capsule_autograd_function(built_lib):
  """The same through layers/capsule_layer.py's entry and torch.autograd (no gradient buffer: autograd gets dSmat)."""
  from easyrec_amd.layers import capsule_layer
  c = capsule_case(B=5, S=7, L=9, D=4, E=33, K=3, iters=2, scale=0.0)
  want_high, want_n, want_dh, want_dS = capsule_reference(c)
  hist = c['hist'].float().to(DEV).requires_grad_(True)
  Smat = c['Smat'].float().to(DEV).requires_grad_(True)
  assert capsule_layer.capsule_fits(hist, 7, 33, 3, 2)
  high, ncaps = capsule_layer.capsule_routing(hist, c['lens'].to(DEV), Smat, c['logits0'].float().to(DEV), *c['cfg'])
  high.backward(c['d_high'].float().to(DEV))
  assert np.array_equal(ncaps.cpu().numpy(), want_n.numpy())
  close(high, want_high, 1e-5, 'high_capsules')
  close(hist.grad, want_dh, 1e-4, 'dhist')
  close(Smat.grad, want_dS, 1e-4, 'dSmat')


# ---------------------------------------------------------------------------------------- the attention
def attention_case(B, K, E, simi_pow, seed=31):
  g = torch.Generator().manual_seed(seed)
  f32 = lambda t: t.float().double()
  ncaps = (torch.arange(B) % K) + 1  # every count from 1 to K
  return dict(interests=f32(torch.randn(B, K, E, generator=g, dtype=torch.float64) / E ** 0.5),
              pos=f32(torch.randn(B, E, generator=g, dtype=torch.float64)), ncaps=ncaps.to(torch.int32), simi_pow=simi_pow,
              d_emb=f32(torch.randn(B, E, generator=g, dtype=torch.float64)),
              d_ui=f32(torch.randn(B, K, E, generator=g, dtype=torch.float64)))


@pytest.mark.parametrize('simi_pow', [10.0, 100.0])
@pytest.mark.parametrize('B,K,E', [(5, 1, 4), (67, 5, 33), (67, 8, 128), (9, 8, 4), (67, 5, 32)])
def test_attention_matches_fp64_autograd(built_lib, B, K, E, simi_pow):
  from easyrec_amd.layers import capsule_layer
  c = attention_case(B, K, E, simi_pow)
  x = c['interests'].clone().requires_grad_(True)
  p = c['pos'].clone().requires_grad_(True)
  emb, ui, w = ref.attention(x, p, c['ncaps'].to(torch.int64), simi_pow)
  want_dx, want_dp = torch.autograd.grad([emb, ui], [x, p], [c['d_emb'], c['d_ui']], allow_unused=True)
  want_dp = torch.zeros_like(p) if want_dp is None else want_dp
  if simi_pow >= 100:
    # the argmax must not hang on fp32 rounding: the two best similarities of every row are apart in the reference
    simi = torch.einsum('bhe,be->bh', c['interests'], c['pos'])
    simi = torch.where(torch.arange(K)[None, :] < c['ncaps'][:, None], simi, torch.full_like(simi, -1e30))
    top = torch.sort(simi, dim=1, descending=True).values
    if K > 1:
      gap = (top[:, 0] - top[:, 1])[c['ncaps'] > 1]
      assert float(gap.min()) > 1e-3, float(gap.min())
    assert float(want_dp.abs().max()) == 0.0
  xg = c['interests'].float().to(DEV).requires_grad_(True)
  pg = c['pos'].float().to(DEV).requires_grad_(True)
  assert capsule_layer.attention_fits(xg)
  got_emb, got_ui = capsule_layer.label_aware_attention(xg, pg, c['ncaps'].to(DEV), simi_pow)
  torch.autograd.backward([got_emb, got_ui], [c['d_emb'].float().to(DEV), c['d_ui'].float().to(DEV)])
  close(got_emb, emb.detach(), 1e-5, 'user_tower_emb')
  assert torch.equal(got_ui.cpu(), ui.detach().float())  # a masked copy
  close(xg.grad, want_dx, 1e-4, 'd_interests')
  close(pg.grad, want_dp, 1e-4, 'd_pos_item', scale=1e-6)
  # without a gradient for user_interests
  xg.grad = pg.grad = None
  got_emb, _ = capsule_layer.label_aware_attention(xg, pg, c['ncaps'].to(DEV), simi_pow)
  got_emb.backward(c['d_emb'].float().to(DEV))
  want_dx2, = torch.autograd.grad(ref.attention(x, p, c['ncaps'].to(torch.int64), simi_pow)[0], [x], [c['d_emb']])
  close(xg.grad, want_dx2, 1e-4, 'd_interests (user_emb only)')


def test_runs_and_graph_replay_are_bit_identical(built_lib):
  from easyrec_amd import kernels
  be = kernels.hip()
  c = capsule_case(B=1001, S=64, L=50, D=16, E=64, K=5, iters=3)
  a = attention_case(1001, 5, 32, 10.0)
  dev = lambda t: t.float().to(DEV).contiguous()
  hist, Smat, lens, l0, d_high = dev(c['hist']), dev(c['Smat']), c['lens'].to(DEV), dev(c['logits0']), dev(c['d_high'])
  x, p, n, d_emb, d_ui = dev(a['interests']), dev(a['pos']), a['ncaps'].to(DEV), dev(a['d_emb']), dev(a['d_ui'])

  def run():
    high, ncaps, W = be.capsule_fwd(hist, lens, Smat, l0, *c['cfg'])
    dS = torch.empty_like(Smat)
    dhist = be.capsule_bwd(hist, lens, Smat, W, d_high, 1.0, 1.0, False, kernels.ThetaGradTable([dS]), acc=False)
    emb, ui, w = be.mind_attention_fwd(x, p, n, 10.0)
    di, dp = be.mind_attention_bwd(x, p, n, w, d_emb, d_ui, 10.0)
    return [high, ncaps, W, dS, dhist, emb, ui, w, di, dp]

  assert_runs_and_replay_bit_identical(run)


@pytest.mark.parametrize('K,D', [(9, 16), (5, 129)])
def test_outside_the_envelope_is_composed(built_lib, K, D):
  from easyrec_amd import kernels
  from easyrec_amd.layers import capsule_layer
  assert kernels.hip().capsule_lds_bytes(64, D, 64, K) == 0 == capsule_layer.lds_bytes(64, D, 64, K)
  c = capsule_case(B=5, S=64, L=64, D=D, E=64, K=K, iters=2, scale=0.0)
  want_high, want_n, want_dh, want_dS = capsule_reference(c)
  hist = c['hist'].float().to(DEV).requires_grad_(True)
  Smat = c['Smat'].float().to(DEV).requires_grad_(True)
  assert not capsule_layer.capsule_fits(hist, 64, 64, K, 2)
  high, ncaps = capsule_layer.capsule_routing(hist, c['lens'].to(DEV), Smat, c['logits0'].float().to(DEV), *c['cfg'])
  high.backward(c['d_high'].float().to(DEV))
  assert np.array_equal(ncaps.cpu().numpy(), want_n.numpy())
  close(high, want_high, 1e-5, 'high_capsules')
  close(hist.grad, want_dh, 1e-4, 'dhist')
  close(Smat.grad, want_dS, 1e-4, 'dSmat')


def test_lds_formula_is_the_library_s(built_lib):
  from easyrec_amd import kernels
  from easyrec_amd.layers import capsule_layer
  be = kernels.hip()
  for S, D, E, K in [(64, 16, 64, 5), (128, 128, 128, 8), (1, 1, 1, 1), (129, 16, 64, 5), (64, 16, 129, 5), (64, 0, 64, 5),
                     (64, 16, 64, 0), (0, 16, 64, 5)]:
    assert be.capsule_lds_bytes(S, D, E, K) == capsule_layer.lds_bytes(S, D, E, K), (S, D, E, K)
  assert capsule_layer.lds_bytes(128, 128, 128, 8) == 144960 <= 160 * 1024


# ---------------------------------------------------------------------------------------- the model
def _configs():
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  try:
    import make_configs
  finally:
    sys.path.pop(0)
  return make_configs


@pytest.mark.parametrize('list_wise', [False, True])
def test_model_first_steps(built_lib, list_wise):
  """Two steps of a MIND config at small table sizes, B = 67, against the fp64 model oracle from the batch on, run on
  the routing logits each step drew (tests/_oracle_steps.first_steps: every loss, the tower embeddings or logits, every
  variable's first moment).  Then the step as a hipGraph: each replay draws fresh routing noise."""
  from easyrec_amd.input.synthetic import SyntheticBatches
  B = 67
  cfg = _configs().mind_taobao(list_wise=list_wise, batch_size=B, scale=0.01)
  noise = []
  est = first_steps(cfg, B, seed=5, oracle_dtype=torch.float64, coverage=pins.mind_coverage,
                    after_step=pins.hand_over_routing_logits(noise))
  assert all(n.shape == (B, 64, 5) and float(np.abs(n).max()) <= 2.0 for n in noise)
  assert not np.array_equal(noise[0], noise[1])
  from easyrec_amd.layers import capsule_layer
  width = est.state_dict()['capsule/S'].shape[0]  # (an operand of the model's: the steps above ran the kernels)
  assert capsule_layer.capsule_fits(torch.empty(B, 64, width, device=DEV), 64, 64, 5, 3)
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=105)
  # the captured step: a replay must draw fresh noise
  est.capture()
  replayed = []
  for _ in range(2):
    est.train_step(gen.next_batch())
    replayed.append(est.model._capsule_layer.last_routing_logits.detach().clone())
  assert est.graph is not None and not torch.equal(replayed[0], replayed[1])
  assert float(replayed[1].abs().max()) <= 2.0 and float(replayed[1].std()) > 0.5


# ---------------------------------------------------------------------------------------- the reference's own outputs
import test_mind_pins as pins  # noqa: E402  (the fixture readers shared with the CPU tests)


@pytest.mark.parametrize('tag', pins.GOLD_CASES)
def test_fixture_cases_through_the_kernels(built_lib, tag):
  """The reference's own high_capsules, capsule counts, user_interests and user_tower_emb, from the kernels (the towers
  between them from the restatement)."""
  from easyrec_amd.layers import capsule_layer
  from easyrec_amd.protos.simi_pb2 import Similarity
  o, msg, loss_type, arr, var, seqs = pins.gold_case(tag)
  c = msg.capsule_config
  hist = ref.combine_hist(msg, seqs, arr['lens']).float().to(DEV)
  Smat = var['capsule/S'].float().to(DEV)
  assert capsule_layer.capsule_fits(hist, c.max_seq_len, c.high_dim, c.max_k, c.num_iters)
  high, ncaps = capsule_layer.capsule_routing(hist, arr['lens'].to(torch.int32).to(DEV), Smat,
                                              pins.gold_logits0(o, msg, arr).float().to(DEV), c.max_seq_len, c.max_k,
                                              c.num_iters, c.routing_logits_scale, c.squash_pow, c.scale_ratio,
                                              c.const_caps_num)
  assert ncaps.cpu().tolist() == arr['num_high_capsules'].tolist()
  close(high, arr['high_capsules'], 1e-5, 'high_capsules')
  B, K, _ = high.shape
  t = o['training']
  u = ref.dnn(ref.batch_norm(arr['user'], var, 'user_fea_bn', t), var, 'user_dnn', training=t)
  ui = torch.cat([arr['high_capsules'], u[:, None, :].expand(B, K, u.shape[1])], dim=2).reshape(B * K, -1)
  ui = ref.dnn(ui, var, 'concat_dnn', last_plain=True, training=t).reshape(B, K, -1)
  if msg.simi_func == Similarity.COSINE:
    ui = ref.mref.l2_normalize(ui)
  ui = ui.float().to(DEV)
  assert capsule_layer.attention_fits(ui)
  emb, masked = capsule_layer.label_aware_attention(ui, arr['item_tower_emb'].float().to(DEV), ncaps, msg.simi_pow)
  close(emb, arr['user_tower_emb'], 1e-5, 'user_tower_emb')
  close(masked, arr['user_interests'], 1e-5, 'user_interests')
