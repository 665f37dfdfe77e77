"""The sorted-run pair kernels (csrc/er_pairwise.hip K8p: K8o's record sort, gather and bounds, pairs, finish) on the GPU
against the fp64 CPU evaluation of the torch compositions differentiated by autograd, with the inputs, the reference and
the bars of tests/test_pairwise_loss_gpu.py: 1e-5 of the expected loss, 1e-4 of the largest expected gradient; where the
fp32 formula itself misses those, four times the fp32 composition's own measured error on the same inputs.  The pair
count is exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from easyrec_amd.builders import loss_builder  # noqa: E402
from easyrec_amd.builders import pairwise_loss as pwl  # noqa: E402
from easyrec_amd.input.synthetic import SyntheticBatches  # noqa: E402
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator  # noqa: E402
from easyrec_amd.utils import config_util  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402
from tests.test_pairwise_loss_gpu import DEV, KINDS, LT, OFF, ROOT, SCALE, _reference, _rel  # noqa: E402

SWITCH = 'EASYREC_AMD_PAIRWISE_SORTED'
I64_MAX = np.iinfo(np.int64).max
# (tile, B): two tiles with one record in the second; three runs (one without a merge partner) and nine row blocks, the
# last ragged; four runs and thirteen row blocks; two tiles of 2048
SHAPES = ((1024, 1025), (1024, 2049), (1024, 3073), (2048, 2049))
PATTERNS = ('none', 'one', 'distinct', 'runs', 'interleaved')
# the kinds and the plain / temperature_margin parameters rotate through the cases: every kind meets every pattern, both
# parameter sets and both weightings
CASES = [(tile, B, pat, list(KINDS)[(i + j + k) % 4], bool(k), ('plain', 'temperature_margin')[i % 2])
         for i, (tile, B) in enumerate(SHAPES) for j, pat in enumerate(PATTERNS) for k in (0, 1)]


def _keys(pattern, B):
  i = np.arange(B, dtype=np.int64)
  if pattern == 'none':
    return None
  if pattern == 'one':
    return np.full(B, -7, dtype=np.int64)
  if pattern == 'distinct':
    return np.random.default_rng(B).permutation(B).astype(np.int64) * 3 - B
  if pattern == 'runs':  # sorted already; lengths that end on and off wave, row-block and 1024-column chunk edges
    lengths = np.array([1, 63, 64, 65, 255, 256, 257, 1023, 1025, 1300])
    ids = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)[:B]
    keys = (ids - 3) * ((1 << 33) + 1)  # three negative keys, the others beyond 32 bits
    keys[ids == ids[-1]] = I64_MAX      # the last run: a real key equal to the padding's
    return keys
  keys = (i % (B // 8)) * 7919 - 5      # interleaved: a session's members B / 8 apart; session 0 has a negative key
  keys[i % (B // 8) == 1] = 1 << 40
  keys[i % (B // 8) == 2] = I64_MAX
  return keys


def _inputs(B, pattern, weighted):
  rng = np.random.default_rng(B * 8 + weighted * 2 + len(pattern))
  z = torch.from_numpy(rng.integers(-256, 257, size=B) / 64.0)
  y = torch.from_numpy(rng.integers(0, 4, size=B) * 0.5)  # graded, with ties
  keys = _keys(pattern, B)
  w = None
  if weighted:
    w = torch.from_numpy(np.round(rng.random(B) * 2, 2) + 0.25)
    w[torch.from_numpy(rng.random(B) < 0.2)] = 0.0  # a few zeros
  return z, y, None if keys is None else torch.from_numpy(keys), w


def _dev(t, dtype=torch.float32):
  return None if t is None else t.to(DEV, dtype)


def _launch(loss_type, param, z, y, keys, w, tile):
  o = kernels.hip().pairwise_loss_sorted(_dev(z), _dev(y), _dev(keys, torch.int64), _dev(w), loss_scale=SCALE, tile=tile,
                                         **pwl.kernel_args(loss_type, pwl.params_of(loss_type, param)))
  return o['loss_partials'], o['dlogits'], o['pair_count']


def _check(got_loss, dz, loss_type, param, z, y, keys, w, want):
  """the bars of the module's docstring; want: _reference(..) in fp64"""
  want_loss, want_dz, _ = want
  assert bool(torch.isfinite(got_loss)) and bool(torch.isfinite(dz).all())
  errs = [_rel(got_loss, want_loss), _rel(dz, want_dz)]
  print('  loss error %.2e, dlogits error %.2e' % tuple(errs))
  if errs[0] > 1e-5 or errs[1] > 1e-4:  # the fp32 formula's own error decides
    comp_loss, comp_dz, _ = _reference(loss_type, param, z, y, keys, w, torch.float32)
    comp = (_rel(comp_loss, want_loss), _rel(comp_dz, want_dz))
    print('  fp32 composition: loss %.2e, dlogits %.2e' % comp)
    assert errs[0] <= max(1e-5, 4.0 * comp[0]) and errs[1] <= max(1e-4, 4.0 * comp[1]), (errs, comp)


@pytest.mark.parametrize('tile,B,pattern,kind,weighted,variant', CASES, ids=lambda v: str(v))
def test_sorted_kernels_against_fp64_composition(tile, B, pattern, kind, weighted, variant):
  loss_type, plain, temp = KINDS[kind]
  param = temp if variant == 'temperature_margin' else plain
  z, y, keys, w = _inputs(B, pattern, weighted)
  want = _reference(loss_type, param, z, y, keys, w, torch.float64)
  partials, dz, pairs = _launch(loss_type, param, z, y, keys, w, tile)
  again = _launch(loss_type, param, z, y, keys, w, tile)
  assert all(torch.equal(a, b) for a, b in zip((partials, dz, pairs), again))  # two runs: the same bits
  assert pairs.dtype == torch.int64 and int(pairs) == want[2]
  assert partials.numel() == kernels.hip().pairwise_sorted_grid(B, tile) == -(-B // 256)
  got_loss = partials.double().sum().cpu()
  if pattern == 'distinct':  # no pair: exactly nothing
    assert want[2] == 0 and float(got_loss) == 0.0 and float(dz.abs().max()) == 0.0
    return
  assert want[2] > 0
  _check(got_loss, dz, loss_type, param, z, y, keys, w, want)


def _raw(be, z, y, keys, w, tile, work, nbytes, outs, temperature=1.0):
  """the library call itself, focal with a hinge margin: outs = (loss_partials, dlogits, pair_count), each may be None"""
  p = kernels._p
  be.ck.er_pairwise_sorted(p(z), 1, p(y), p(keys), p(w), z.numel(), kernels.PAIR_FOCAL, kernels.PAIR_HINGE_MARGIN, temperature,
                           1.0, 0.0, 1.0 + OFF, 2.0, 0.0, 1.0, tile, p(work), nbytes, p(outs[0]), p(outs[1]), p(outs[2]),
                           kernels._stream())


def test_launch_contract():
  be = kernels.hip()
  B, tile = 2049, 1024
  z, y, keys, w = _inputs(B, 'interleaved', True)
  z, y, keys, w = _dev(z), _dev(y), _dev(keys, torch.int64), _dev(w)

  def run():
    o = be.pairwise_loss_sorted(z, y, keys, w, kernels.PAIR_FOCAL, kernels.PAIR_HINGE_MARGIN, hinge_margin=1.0 + OFF, tile=tile)
    return [o['loss_partials'], o['dlogits'], o['pair_count']]
  full = [t.clone() for t in run()]
  assert int(full[2]) > 0
  assert_runs_and_replay_bit_identical(run)
  # every output left out in turn: the others keep their bits
  nbytes = pwl.sorted_workspace_bytes(B, tile)
  work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=DEV)
  for skip in range(3):
    outs = [None if i == skip else torch.empty_like(t) for i, t in enumerate(full)]
    _raw(be, z, y, keys, w, tile, work, work.numel() * 8, outs)
    assert all(o is None or torch.equal(o, t) for o, t in zip(outs, full)), skip
  # outside the envelope the launch returns an error
  outs = [torch.empty_like(t) for t in full]
  big = torch.zeros(8192, device=DEV)
  roomy = torch.empty(1 << 17, dtype=torch.int64, device=DEV)
  for args in ((z, y, keys, w, 3000, work, work.numel() * 8, outs),       # no such tile
               (big, big, None, None, 0, roomy, roomy.numel() * 8, outs),  # B = 8192 is er_pairwise's
               (z, y, keys, w, tile, work, work.numel() * 8, outs, 0.0),   # temperature 0
               (z, y, keys, w, tile, work, nbytes - 8, outs)):             # a short workspace
    with pytest.raises(RuntimeError, match='er_pairwise_sorted'):
      _raw(be, *args)


@pytest.mark.parametrize('kind,keyed', [('logistic', True), ('focal', False)])
def test_with_the_switch_on_the_builder_launches_beyond_8192(kind, keyed, monkeypatch):
  monkeypatch.setenv(SWITCH, '1')
  loss_type, param = KINDS[kind][0], KINDS[kind][2]
  z, y, keys, w = _inputs(8193, 'interleaved' if keyed else 'none', True)
  loss, dz = loss_builder.build(loss_type, _dev(y), _dev(z), _dev(w), loss_scale=SCALE, loss_param=param,
                                session_ids=_dev(keys, torch.int64))
  extras = loss._er_extras
  assert extras is not None and loss._er_partials[1:] == (1.0, 1.0)  # the launch; the loss tail sums its partial rows
  want = _reference(loss_type, param, z, y, keys, w, torch.float64)
  assert int(extras['pair_count']) == want[2] > 0
  _check(extras['loss_partials'].double().sum().cpu(), dz, loss_type, param, z, y, keys, w, want)
  monkeypatch.setenv(SWITCH, '0')  # and without it, the composition
  assert loss_builder.build(loss_type, _dev(y), _dev(z), _dev(w), loss_scale=SCALE, loss_param=param,
                            session_ids=_dev(keys, torch.int64))[0]._er_extras is None


@pytest.mark.parametrize('keyed', [False, True])
def test_the_step_beyond_8192_replays_from_a_graph(keyed, monkeypatch):
  """configs/multi_tower_f1_pairwise_criteo_small.config at batch_size 8193, its pairwise loss as it is or as a logistic
  loss keyed by an id feature: three steps replayed from a captured hipGraph give the losses of three eager steps (the
  composition cannot be captured)."""
  monkeypatch.setenv(SWITCH, '1')
  be, calls = kernels.hip(), []
  inner = be.pairwise_loss_sorted
  monkeypatch.setattr(be, 'pairwise_loss_sorted', lambda *a, **k: (calls.append(a[2] is not None), inner(*a, **k))[1],
                      raising=False)
  losses = {}
  for graph in (False, True):
    cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'multi_tower_f1_pairwise_criteo_small.config'))
    entry = cfg.model_config.losses[1]
    assert entry.loss_type == LT.PAIR_WISE_LOSS
    name = 'pair_wise_loss'
    if keyed:
      entry.loss_type = LT.PAIRWISE_LOGISTIC_LOSS
      entry.pairwise_logistic_loss.session_name = 'C1'
      name = 'pairwise_logistic_loss'
    est = EasyRecEstimator(cfg, device=DEV, batch_size=8193, seed=11).build()
    gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=8193, seed=111)
    est.train_step(gen.next_batch())  # (one eager step before a capture: lazily created workspaces exist)
    if graph:
      est.capture(warmup=0)
    seen = []
    for _ in range(3):
      est.train_step(gen.next_batch())
      seen.append(est.loss_values())
    assert (est.graph is not None) == graph and name in seen[0] and np.isfinite(seen[-1][name])
    losses[graph] = seen
  assert calls and all(k == keyed for k in calls), calls  # (the sorted launch served the loss, with keys or without)
  assert losses[True] == losses[False], (losses[True], losses[False])
