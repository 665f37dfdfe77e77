"""Test infrastructure shared by the model tests (-m gpu: tests/test_models_gpu.py, test_bst_gpu.py,
test_autoint_gpu.py, test_fibinet_gpu.py, test_match_gpu.py, test_mind_gpu.py, test_neg_sampler_gpu.py,
test_uniter_model_gpu.py, test_cmbf_model_gpu.py, test_seq_combiner_gpu.py, test_weighted_sampler_gpu.py; on the CPU
stand-in: test_match_pins.py, test_mind_pins.py, test_neg_sampler_pins.py, test_uniter_model_pins.py,
test_cmbf_model_pins.py, test_seq_combiner_pins.py, test_weighted_sampler_pins.py): a model's first training steps
against the CPU oracle - as figures in units of their bars (step_figures) and held to them (first_steps) - the
two-runs-and-a-hipGraph-replay bit identity check of a kernel sequence, and the max-error-over-max-value comparison."""
import numpy as np
import torch

from easyrec_amd.input.synthetic import SyntheticBatches
from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
from oracle.model_oracle import OracleTrainer


def _f64(x):
  return x.detach().cpu().double().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)


def close(got, want, tol, what, scale=None):
  """max |got - want| <= tol * max |want|; scale: a floor for max |want| (a gradient that is zero up to rounding)."""
  got, want = _f64(got), _f64(want)
  scale = max(float(np.abs(want).max()), scale or 1e-30)
  err = float(np.abs(got - want).max())
  assert err <= tol * scale, (what, err, scale)


def step_figures(cfg, B, seed, steps=2, step0_tol=1e-5, device='cuda:0', grad_views=True, skip_bn_shadowed_bias=True,
                 oracle_dtype=torch.float32, est_kw=None, oracle_kw=None, after_step=None):
  """`steps` training steps of the product and of the oracle from the same state on the same synthetic batches
  -> (the estimator, {comparison: its error in units of its bar - <= 1 holds it}, the names of the compared variables).
  The comparisons: ('loss', step, name): every loss, the bar step0_tol (first step) / 1e-4 (later steps) of
  max(1e-3, |expected|); after the first step ('logits', key): the logits, the bar atol 1e-5 + rtol 1e-4 elementwise
  (np.allclose's inequality divided through), and ('grad', variable): the gradient of every variable, read back as
  Adam's first moment, the bar 2e-4 of the tensor's gradient scale + 2e-6 of the largest one.
  grad_views: autograd accumulated in place into the flat gradient buffer; skip_bn_shadowed_bias: a dense bias under
  BatchNorm has a zero gradient (rounding noise) and is not compared.  oracle_dtype: the oracle's forward and backward
  pass; est_kw / oracle_kw: further constructor arguments (an item table, the sampler's seed); after_step(est, orc,
  step, batch): called between the product's step and the oracle's (MIND: hands the routing logits the product drew to
  the oracle).  A list-wise two-tower model never builds its logits while training: the two tower embeddings they are
  the product of are compared instead.  A regression tower's output is `y_<tower>`."""
  est = EasyRecEstimator(cfg, device=device, batch_size=B, seed=seed, **(est_kw or {})).build()
  orc = OracleTrainer(cfg, est.state_dict(), batch_size=B, dtype=oracle_dtype, **(oracle_kw or {}))
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=seed + 100)
  fig, compared = {}, []
  for step in range(steps):
    b = gen.next_batch()
    est.train_step(b)
    if after_step is not None:
      after_step(est, orc, step, b)
    got, exp = est.loss_values(), orc.train_step(b)
    assert sorted(got) == sorted(exp)
    for k in exp:
      fig['loss', step, k] = abs(got[k] - exp[k]) / ((step0_tol if step == 0 else 1e-4) * max(1e-3, abs(exp[k])))
    if step > 0:
      continue
    got_pred = est.model._prediction_dict
    keys = [k for k in orc.last_pred if k.startswith('logits') or k.startswith('y_')]
    if keys == ['logits'] and 'logits' not in got_pred:  # (a list-wise two-tower model while training)
      keys = ['user_tower_emb', 'item_tower_emb']
    for k in keys:
      got_l, ref = got_pred[k].detach().cpu().numpy(), orc.last_pred[k]
      fig['logits', k] = float(np.max(np.abs(got_l - ref) / (1e-5 + 1e-4 * np.abs(ref))))
    if grad_views:
      est.varstore.check_grad_views()
    st = est.state_dict(slots=True)
    names = set(orc.state)
    gmax = max(float(np.max(np.abs(v))) for kk, v in orc.slots.items() if kk.endswith('/m'))
    for k in orc.state:
      key = k + '/m'
      if key not in orc.slots or key not in st:
        continue
      if skip_bn_shadowed_bias and k.endswith('/bias') and (k[:-len('/bias')] + '/bn/gamma') in names:
        continue  # d(loss)/d(bias) == 0 under BatchNorm: rounding noise
      ref = orc.slots[key]
      fig['grad', k] = float(np.max(np.abs(st[key] - ref))) / (2e-4 * float(np.max(np.abs(ref))) + 2e-6 * gmax)
      compared.append(k)
  return est, fig, compared


def worst(fig):
  """step_figures' figures by kind -> {'loss<step>', 'logits', 'grads': the largest}"""
  out = {}
  for k, v in fig.items():
    name = {'loss': 'loss%s' % k[1], 'grad': 'grads'}.get(k[0], k[0])
    out[name] = v if np.isnan(v) else max(out.get(name, 0.0), v)
  return out


def first_steps(cfg, B, seed, coverage=None, **kw):
  """step_figures with every figure held to its bar; coverage(names, cfg): the caller's own assertions on the list of
  compared variables.  -> the estimator"""
  est, fig, compared = step_figures(cfg, B, seed, **kw)
  for k, v in fig.items():
    assert v <= 1.0, (k, v)
  assert len(compared) > 5
  if coverage is not None:
    coverage(compared, cfg)
  return est


def covers(names, cfg, dense, groups=('user', 'item')):
  """a coverage callback's body: the compared variables hold `dense` and an embedding table of each of `groups` (a plain
  column's `<scope>/<feature>_embedding`, a sequence kept over time's `input_layer/<feature>`)"""
  assert set(dense) <= set(names), set(dense) - set(names)
  for g in cfg.model_config.feature_groups:
    if g.group_name in groups:
      assert any(n.endswith('/%s_embedding/embedding_weights' % f) or n == 'input_layer/%s/embedding_weights' % f
                 for n in names for f in g.feature_names), g.group_name


def assert_runs_and_replay_bit_identical(run):
  """run() -> list of tensors: two eager runs, and a replay of run() captured as a hipGraph, give the same bits."""
  first = run()
  second = run()
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(first, second))
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    run()  # (warm-up on the capture stream)
  torch.cuda.current_stream().wait_stream(s)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    static = run()
  graph.replay()
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(first, static))
