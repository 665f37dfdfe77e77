"""The tiled sorted-segment kernels (csrc/er_listwise.hip K8o: tile sort, merge passes, three reduction stages with
carries between the workgroups) on the GPU against fp64 torch autograd of K8n's formulas in vectorised form (unique with
inverse, scatter_reduce amax, index_add), at the bars of tests/test_listwise_loss_gpu.py: 1e-5 of the expected loss, 1e-4
of the largest expected d loss / d logits, 1e-4 of sum |g_i z_i| and sum |g_i| for the scale gradients; where the fp32
formula itself misses a bar, four times the error of the same code in float32 on the same inputs."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.builders import listwise_loss as lwl  # noqa: E402
from easyrec_amd.builders import loss_builder  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402
from tests.test_listwise_loss_gpu import CONFIGS, DEV, I64, LT, ROOT, SCALE  # noqa: E402

# (tile, B): two tiles with one record in the second; an exact fit; three runs (one without a partner in the first pass);
# four runs, the last short; five runs over three passes; then the first, third and fifth at the public path's tile
SHAPES = ((1024, 1025), (1024, 2048), (1024, 2049), (1024, 3073), (1024, 5000), (8192, 8193), (8192, 16385), (8192, 40000))
PATTERNS = ('one', 'distinct', 'runs', 'interleaved', 'wide')
CASES = [(tile, B, pat, (i * len(PATTERNS) + j) % len(CONFIGS)) for i, (tile, B) in enumerate(SHAPES)
         for j, pat in enumerate(PATTERNS)]


def _keys(pattern, B, rng):
  i = np.arange(B, dtype=np.int64)
  if pattern == 'one':  # spans every chunk
    return np.full(B, -7, dtype=np.int64)
  if pattern == 'distinct':
    return rng.permutation(B).astype(np.int64) * 3 - B
  if pattern == 'runs':  # sorted already; lengths that end on and off lane, wave and chunk edges.  The first 1024 fills a
    # chunk of 1024; 2043 covers another and parts of its neighbours; the 8192 lies on 8192 .. 16383, a chunk of its own
    lengths = np.resize(np.array([1024, 1, 7, 8, 56, 64, 3, 61, 448, 512, 5, 2043, 960, 3000, 8192, 1023, 1, 1024]), B // 64 + 18)
    return np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)[:B] - 11
  if pattern == 'interleaved':  # a session's members B / 8 apart
    return (i % max(B // 8, 1)) * 7919 - 5
  keys = ((i % 5) << 33) * np.where(i % 2 == 0, 1, -1)  # differ only above bit 32, both signs
  keys[::7] = I64.max
  keys[B // 2::11] = I64.min
  return keys


def _inputs(B, pattern, kind):
  rng = np.random.default_rng(B * 16 + len(pattern))
  keys = _keys(pattern, B, rng)
  z = rng.standard_normal(B) * 2.0
  z[keys == keys[0]] *= np.where(rng.random(int((keys == keys[0]).sum())) < 0.5, 40.0, 1.0)
  z[0] = 80.0
  y = np.exp(rng.random(B) * 8.0 - 1.4) if kind == LT.LISTWISE_DISTILL_LOSS else np.round(rng.random(B) * 3.0, 2)
  exact = lambda v: torch.from_numpy(v.astype(np.float32).astype(np.float64))  # noqa: E731 (fp32 values: no input rounding)
  return exact(z), exact(y), torch.from_numpy(keys)


def _reference(kind, p, z, y, keys, scale, dtype):
  """K8n's formulas, vectorised -> (loss, d loss / d z, d / d scale_w, d / d scale_b, number of sessions)"""
  z = z.to(dtype).clone().requires_grad_(True)
  w, b = (torch.tensor([v], dtype=dtype, requires_grad=True) for v in (scale or (1.0, 0.0)))
  y, T = y.to(dtype), p['temperature']
  if kind == LT.LISTWISE_DISTILL_LOSS:
    y = torch.log1p(torch.tensor(p['label_clip_max'], dtype=dtype)) - torch.log(torch.clamp(y, 1, p['label_clip_max']))
  a = (z * torch.abs(w) + b) if scale else z
  if T != 1.0:
    a = a / T
    y = y / T if p['label_is_logits'] else y
  inv = torch.unique(keys, return_inverse=True)[1]
  S = int(inv.max()) + 1
  seg_sum = lambda x: torch.zeros(S, dtype=dtype).index_add(0, inv, x)  # noqa: E731

  def log_softmax(x):
    x = x - torch.full((S,), -np.inf, dtype=dtype).scatter_reduce(0, inv, x.detach(), 'amax')[inv]
    return x - torch.log(seg_sum(torch.exp(x)))[inv]
  t = y / seg_sum(y)[inv] if kind == LT.LISTWISE_DISTILL_LOSS else (torch.exp(log_softmax(y)) if p['label_is_logits'] else y)
  loss = -seg_sum(t * log_softmax(a)).mean() * SCALE
  loss.backward()
  return loss.detach(), z.grad, w.grad, b.grad, S


def _check(got, kind, p, z, y, keys, scale):
  want = _reference(kind, p, z, y, keys, scale, torch.float64)
  comp = None
  wabs = abs(scale[0]) if scale else 1.0  # g = dz / |w|
  bars = (max(abs(float(want[0])), 1e-30), max(float(want[1].abs().max()), 1e-30),
          float((want[1] * z).abs().sum()) / wabs + 1e-30, float(want[1].abs().sum()) / wabs + 1e-30)
  for i, tol in enumerate((1e-5, 1e-4, 1e-4, 1e-4)):
    if got[i] is None:
      continue
    err = float((got[i].double().cpu().reshape(-1) - want[i].reshape(-1)).abs().max()) / bars[i]
    print('  output %d: error %.2e of %.3e' % (i, err, bars[i]))
    if not err <= tol:  # the fp32 formula's own error decides
      comp = comp or _reference(kind, p, z, y, keys, scale, torch.float32)
      ref = float((comp[i].double().reshape(-1) - want[i].reshape(-1)).abs().max()) / bars[i]
      print('  output %d: fp32 composition %.2e' % (i, ref))
      assert np.isfinite(err) and err <= 4.0 * ref, (i, err, ref)
  return want


def _fused(kind, p, z, y, keys, scale, tile, pitch):
  zd = torch.zeros(z.numel(), pitch, device=DEV)
  zd[:, 0] = z.to(DEV, torch.float32)
  zd.requires_grad_(True)
  w, b = (torch.tensor([v], device=DEV, requires_grad=True) for v in scale) if scale else (None, None)
  loss, n = lwl.fused(kind, y.to(DEV, torch.float32), zd[:, 0], keys.to(DEV), p, w, b, loss_scale=SCALE, tile=tile)
  (loss * 2.0).backward()  # (an upstream gradient that is not 1)
  return loss.detach(), zd.grad[:, 0] / 2.0, None if w is None else w.grad / 2.0, None if b is None else b.grad / 2.0, n


@pytest.mark.parametrize('tile,B,pattern,config', CASES, ids=lambda v: str(v))
def test_tiled_kernels_against_fp64_autograd(tile, B, pattern, config):
  (kind, param), scale = CONFIGS[config]
  p = lwl.params_of(kind, param)
  z, y, keys = _inputs(B, pattern, kind)
  got = _fused(kind, p, z, y, keys, scale, tile, pitch=3 if B % 2 else 1)
  again = _fused(kind, p, z, y, keys, scale, tile, pitch=3 if B % 2 else 1)
  assert all(a is None or torch.equal(a, b) for a, b in zip(got, again))  # two runs: the same bits
  want = _check(got[:4], kind, p, z, y, keys, scale)
  assert int(got[4]) == want[4] == len(set(keys.tolist()))


def test_null_outputs_envelope_and_graph_replay():
  be = kernels.hip()
  z, y, keys = (t.to(DEV) for t in _inputs(16385, 'interleaved', LT.LISTWISE_RANK_LOSS))
  z, y = z.float(), y.float()
  w, b = torch.tensor([-1.5], device=DEV), torch.tensor([0.25], device=DEV)
  grads = [torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)]
  kw = dict(kind=kernels.LIST_RANK, flags=kernels.LIST_LABEL_IS_LOGITS, temperature=0.5, scale_w=w, scale_b=b)

  def run():
    o = be.listwise_loss_tiled(z, y, keys, grads=kernels.ThetaGradTable(grads), acc=False, **kw)
    return [o['loss_partials'], o['dlogits'], o['num_sessions']] + grads
  full = [t.clone() for t in run()]
  assert full[0].numel() == be.listwise_tiled_grid(16385) > 1
  assert_runs_and_replay_bit_identical(run)
  # every optional output left out in turn: the others keep their bits
  assert torch.equal(be.listwise_loss_tiled(z, y, keys, want=('loss',), **kw)['loss_partials'], full[0])
  assert torch.equal(be.listwise_loss_tiled(z, y, keys, want=('dlogits',), **kw)['dlogits'], full[1])
  assert torch.equal(be.listwise_loss_tiled(z, y, keys, want=('num_sessions',), **kw)['num_sessions'], full[2])
  with pytest.raises(RuntimeError, match='er_listwise_tiled'):
    be.listwise_loss_tiled(z, y, keys, kind=kernels.LIST_RANK, temperature=0.0)


def test_with_the_switch_on_the_builder_launches_beyond_8192(monkeypatch):
  monkeypatch.setenv('EASYREC_AMD_LISTWISE_TILED', '1')
  for (kind, param), scale in (CONFIGS[1], CONFIGS[4]):
    z, y, keys = _inputs(8193, 'interleaved', kind)
    sv = tuple(torch.tensor([v], device=DEV, requires_grad=True) for v in scale)
    loss, dz = loss_builder.build(kind, y.to(DEV, torch.float32), z.to(DEV, torch.float32), 1.0, loss_scale=SCALE,
                                  loss_param=param, session_ids=keys.to(DEV), scale_vars=sv)
    assert loss._er_extras is not None  # (the launch; the loss tail would sum its partial rows)
    total = loss._er_extras['loss_partials'].double().sum()
    _check((total, dz, sv[0].grad, sv[1].grad), kind, lwl.params_of(kind, param), z, y, keys, scale)


@pytest.mark.parametrize('kind', ['listwise_rank_loss', 'listwise_distill_loss'])
def test_the_step_beyond_8192_replays_from_a_graph(kind, monkeypatch):
  """configs/multi_tower_f1_pairwise_criteo_small.config with its pairwise loss replaced, at batch_size 8193: three steps
  replayed from a captured hipGraph give the losses of three eager steps (the composition cannot be captured)."""
  monkeypatch.setenv('EASYREC_AMD_LISTWISE_TILED', '1')
  losses = {}
  for graph in (False, True):
    cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'multi_tower_f1_pairwise_criteo_small.config'))
    entry = cfg.model_config.losses[1]
    entry.loss_type = LT.Value(kind.upper())
    getattr(entry, kind).session_name = 'C1'
    getattr(entry, kind).scale_logits = True
    est = EasyRecEstimator(cfg, device=DEV, batch_size=8193, seed=11).build()
    gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=8193, seed=111)
    est.train_step(gen.next_batch())  # (one eager step before a capture: lazily created workspaces exist)
    if graph:
      est.capture(warmup=0)
    seen = []
    for _ in range(3):
      est.train_step(gen.next_batch())
      seen.append(est.loss_values())
    assert (est.graph is not None) == graph and kind in seen[0] and np.isfinite(seen[-1][kind])
    losses[graph] = seen
  assert losses[True] == losses[False], (losses[True], losses[False])
