"""-m gpu: every device path of the closed-form decay replay (er_decay.h, replay_closed, the tables of the step prologue)
against the float64 recurrence and the derived bounds of tests/_decay_cases.py; the exact step-by-step replay and the
streaming sweep through the same harness against the same reference (tests/test_decay_pins.py shows on the CPU that the
reference is right, that the bounds hold a correct float32 evaluation at half and that seeded faults exceed them).

Per beta pair one history is built once (module scope): the hyper table's rows, then one step_prologue(history=,
decay_tables=) per step - that fills the lr_t history, the running maxima and the per-step table C.  Every test creates
its groups against that history and counter and writes var, m, v and last_step itself; last_step is the caller's
tensor, so one launch covers every idle length of the case.  A test that needs another step counter sets it and puts
it back.  Every error-to-bound ratio is printed (RATIO ...); a bound of 0 demands bit equality.  No number here comes
from a kernel.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from tests import _decay_cases as dc  # noqa: E402
from tests import _emb_bwd_cases as ec  # noqa: E402

DEV = 'cuda:0'
S = dc.S_TOTAL
CAP = S + 8
CLOSED_GRID = [('usual', d) for d in dc.DIMS] + [('edge', 3), ('edge', 16), ('long', 3), ('long', 16)]


@pytest.fixture(scope='module')
def hip():
  assert torch.cuda.is_available(), 'gpu tests need an MI355X'
  assert kernels.HYPER_FLOATS == ec.HYPER_FLOATS
  assert (kernels.HYPER_LR_T, kernels.HYPER_BETA1, kernels.HYPER_BETA2, kernels.HYPER_EPS) == (ec.H_LR_T, ec.H_B1, ec.H_B2, ec.H_EPS)
  return kernels.hip()


class _History(object):
  """S steps of one beta pair on the device: counter == S, hist, the hyper record of step S - 1, the tables (or None)."""

  def __init__(self, hip, pair):
    self.hip, self.pair = hip, pair
    b1, b2 = dc.REFUSED if pair == 'refused' else dc.PAIRS[pair]
    self.rows_h = torch.from_numpy(dc.hyper_rows(pair)).to(DEV)
    self.counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    self.hist = torch.zeros(2 * CAP, device=DEV)
    self.hyper = torch.zeros(kernels.HYPER_FLOATS, device=DEV)
    self.tabs = hip.decay_tables_create(self.hist, self.counter, b1, b2)
    assert (self.tabs is None) == (pair == 'refused'), 'er_decay_tables_supported: %s' % pair
    if self.tabs is not None:
      assert hip.lib.er_decay_tables_supported(b1, b2) == dc.EXPECTED_K[pair]
    for _ in range(S):
      self.prologue(self.tabs)
    torch.cuda.synchronize()
    assert int(self.counter.item()) == S
    want = dc.lr_history(pair)[:S]
    assert np.array_equal(self.hist[:S].cpu().numpy(), want)
    assert np.array_equal(self.hist[CAP:CAP + S].cpu().numpy(), np.maximum.accumulate(want))
    assert np.array_equal(self.hyper.cpu().numpy(), dc.hyper_rows(pair)[S - 1])

  def prologue(self, tabs):
    self.hip.step_prologue(self.rows_h, self.counter, self.hyper, history=self.hist, decay_tables=tabs)

  def close(self):
    self.hip.decay_tables_destroy(self.tabs)


@pytest.fixture(scope='module')
def histories(hip):
  made = {}

  def get(pair):
    if pair not in made:
      made[pair] = _History(hip, pair)
    return made[pair]
  yield get
  torch.cuda.synchronize()
  for h in made.values():
    h.close()


class _Dev(object):
  """A case's state on the device as one lazily decaying table group with one dense lookup over `ids`."""

  def __init__(self, hip, H, st, ids=None, tables=True, pitched=False):
    self.hip, self.H, self.st = hip, H, st
    rows, dim = st.var.shape
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731
    if pitched:  # var | m | v | last_step as column blocks of one record buffer
      ld = 3 * dim + 4
      self.rec = torch.zeros(rows, ld, device=DEV)
      self.var, self.m, self.v = (self.rec[:, i * dim:(i + 1) * dim] for i in range(3))
      self.last = self.rec.view(torch.int32)[:, 3 * dim]
      self.var.copy_(t(st.var)), self.m.copy_(t(st.m)), self.v.copy_(t(st.v)), self.last.copy_(t(st.last))
      assert self.last.stride(0) == ld and self.var.stride(0) == ld
    else:
      self.var, self.m, self.v, self.last = t(st.var), t(st.m), t(st.v), t(st.last)
    ids = np.arange(rows) if ids is None else ids
    self.ids = t(np.asarray(ids, dtype=np.int64))
    self.buf = torch.zeros(len(ids), dim, device=DEV)
    self.spec = kernels.LookupSpec(table=self.var, ids=self.ids, offsets=None, weights=None, out=self.buf, out_col=0,
                                   rows=rows, key_base=0, dim=dim, combiner=0, n_rows=len(ids), max_nnz=len(ids))
    self.g = hip.emb_group_create([self.spec], dim, rows, self.var, self.m, self.v, None)
    hip.emb_group_enable_lazy_decay(self.g, self.last, H.hist, H.counter)
    if tables and H.tabs is not None:
      hip.emb_group_set_decay_tables(self.g, H.tabs)

  def got(self):
    torch.cuda.synchronize()
    return {'var': self.var.cpu().numpy(), 'm': self.m.cpu().numpy(), 'v': self.v.cpu().numpy(),
            'last': self.last.cpu().numpy()}

  def close(self):
    self.hip.emb_group_destroy(self.g)


class _counter_at(object):
  """The step counter at `value` inside the block, S again behind it."""

  def __init__(self, H, value):
    self.H, self.value = H, value

  def __enter__(self):
    self.H.counter.fill_(self.value)

  def __exit__(self, *exc):
    torch.cuda.synchronize()
    self.H.counter.fill_(S)


def _reference(pair, st, s_end, listed=None):
  b1, b2 = dc.betas(pair)
  return dc.reference(st.var, st.m, st.v, st.last, s_end, dc.lr_history(pair), b1, b2, K=dc.EXPECTED_K.get(pair),
                      listed=listed)


def _expect_last(got, st, s_end, listed=None):
  """Every listed row with pending steps is marked s_end - 1; the others keep their mark."""
  moved = (st.last < s_end - 1) if listed is None else ((st.last < s_end - 1) & listed)
  assert np.array_equal(got['last'], np.where(moved, s_end - 1, st.last))


# ------------------------------------------------------------------------------------------- the tables themselves
@pytest.mark.parametrize('pair', sorted(dc.PAIRS))
def test_tables_equal_the_restatement(hip, histories, pair):
  """coef (double), the per-step table C and the lag-0 table A behind a full flush, read from the tables' buffer (coef |
  A[2][kDecayKMax] | C[capacity + 1], kDecayLd = 8 per row) against tests/_decay_cases.Tables: C and A within one
  float32 rounding of the double sum (the device adds 64 partial sums, the restatement one dot product)."""
  H = histories(pair)
  tb = dc.tables(pair)
  K = tb.K
  st, _ = dc.case_reference(pair, 16, S)
  dev = _Dev(hip, H, st)
  hip.emb_flush_decay(dev.g, H.hyper)
  torch.cuda.synchronize()
  buf = H.tabs['buffer']
  coef = buf[:dc.K_MAX * 8].cpu().numpy().reshape(dc.K_MAX, 8)
  f = buf.view(torch.float32)[2 * dc.K_MAX * 8:].cpu().numpy()
  A = f[:dc.K_MAX * 8].reshape(dc.K_MAX, 8)
  C = f[2 * dc.K_MAX * 8:2 * dc.K_MAX * 8 + (CAP + 1) * 8].reshape(CAP + 1, 8)
  assert np.allclose(coef[:K, :dc.N_POW], tb.coef, rtol=1e-13, atol=0.0)
  assert not coef[:, dc.N_POW:].any() and not coef[K:].any()
  for name, got, want in (('A', A[:K, :dc.N_POW], tb.A(S)[:K]), ('C', C[:S - K + 1, :dc.N_POW], tb.C())):
    r = dc.ratio(got, want.astype(np.float64), 2 * dc.U * np.abs(want.astype(np.float64)))
    print('RATIO who=tables case=%s tensor=%s ratio=%.4g' % (pair, name, r))
    assert r <= 1.0, (name, r)
  assert not A[:, dc.N_POW:].any() and not C[:, dc.N_POW:].any() and not C[S - K + 1:].any()
  dev.close()


def test_refused_betas_keep_the_exact_replay(hip, histories):
  H = histories('refused')
  assert H.tabs is None and hip.lib.er_decay_tables_supported(*dc.REFUSED) == 0


# ------------------------------------------------------------------------------------------- full flush
@pytest.mark.parametrize('pair,dim,s_end,pitched', [(p, d, S, False) for p, d in CLOSED_GRID] +
                         [('usual', 16, S, True), ('usual', 16, 3, False), ('usual', 1, 2, False), ('usual', 4, 3, True)])
def test_flush_decay(hip, histories, pair, dim, s_end, pitched):
  """emb_flush_decay_kernel behind the lag-0 table built in front of it; s_end <= 3: early training, the tables' rows
  beyond s_end read no history."""
  H = histories(pair)
  st, ref = dc.case_reference(pair, dim, s_end)
  dev = _Dev(hip, H, st, pitched=pitched)
  with _counter_at(H, s_end):
    hip.emb_flush_decay(dev.g, H.hyper)
  got = dev.got()
  dc.check('flush_decay', '%s-d%d-s%d%s' % (pair, dim, s_end, '-pitched' if pitched else ''), got, ref, dc.bounds_closed(ref))
  assert (got['last'] == s_end - 1).all()
  dev.close()


def test_rows_that_span_wavefronts(hip, histories):
  """dim 512 (G = 128 lanes): the full flush and the single catch-up through replay_block take it; the rolling flush
  and the fused front refuse it."""
  H = histories('usual')
  st, ref = dc.case_reference('usual', dc.WIDE_DIM, S, dc.WIDE_ROWS)
  dev = _Dev(hip, H, st)
  hip.emb_flush_decay(dev.g, H.hyper)
  dc.check('flush_decay', 'usual-d512', dev.got(), ref, dc.bounds_closed(ref))
  dev.close()
  st, _ = dc.case_reference('usual', dc.WIDE_DIM, S - 1, dc.WIDE_ROWS)
  listed = np.arange(dc.WIDE_ROWS) % 3 != 1
  ref = _reference('usual', st, S - 1, listed)
  dev = _Dev(hip, H, st)
  keys = torch.from_numpy(np.flatnonzero(listed).astype(np.int32)).to(DEV)
  nu = torch.tensor([len(keys)], dtype=torch.int32, device=DEV)
  hip.emb_catch_up(dev.g, keys, nu, H.hyper)
  got = dev.got()
  dc.check('catch_up(replay_block)', 'usual-d512', got, ref, dc.bounds_closed(ref))
  _expect_last(got, st, S - 1, listed)
  with pytest.raises(RuntimeError, match='er_emb_flush_window.*one wavefront'):
    hip.emb_flush_window([dev.g], 7, H.hyper)
  assert hip.emb_front([dev.g], H.hyper, False, defer=True) is False
  after = dev.got()
  assert all(np.array_equal(after[k], got[k]) for k in got)
  dev.close()


# ------------------------------------------------------------------------------------------- catch-up launches
def _listed(rows):
  return (np.arange(rows) * 7 + 3) % 5 != 0   # four rows of five, every idle length among them


def _keys(listed):
  keys = torch.from_numpy(np.flatnonzero(listed).astype(np.int32)).to(DEV)
  return keys, torch.tensor([len(keys)], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize('pair,dim', CLOSED_GRID)
def test_catch_up(hip, histories, pair, dim):
  """emb_catch_up_closed_kernel: the listed keys are brought to counter - 2, the others keep every bit."""
  H = histories(pair)
  st, _ = dc.case_reference(pair, dim, S - 1)
  listed = _listed(dc.ROWS)
  ref = _reference(pair, st, S - 1, listed)
  dev = _Dev(hip, H, st)
  keys, nu = _keys(listed)
  hip.emb_catch_up(dev.g, keys, nu, H.hyper)
  got = dev.got()
  dc.check('catch_up', '%s-d%d' % (pair, dim), got, ref, dc.bounds_closed(ref))
  _expect_last(got, st, S - 1, listed)
  dev.close()


def test_catch_up_multi_with_two_lane_widths(hip, histories):
  H = histories('usual')
  devs, refs, lists = [], [], []
  for dim in (16, 3):
    st, _ = dc.case_reference('usual', dim, S - 1)
    listed = _listed(dc.ROWS) if dim == 16 else ~_listed(dc.ROWS) | (np.arange(dc.ROWS) % 2 == 0)
    devs.append(_Dev(hip, H, st))
    refs.append(_reference('usual', st, S - 1, listed))
    lists.append(listed)
  kn = [_keys(li) for li in lists]
  hip.emb_catch_up_multi([d.g for d in devs], [k for k, _ in kn], [n for _, n in kn], H.hyper)
  for dev, ref, listed in zip(devs, refs, lists):
    got = dev.got()
    dc.check('catch_up_multi', 'usual-d%d' % dev.st.dim, got, ref, dc.bounds_closed(ref))
    _expect_last(got, dev.st, S - 1, listed)
    dev.close()


@pytest.mark.parametrize('dim', [16, 3])
@pytest.mark.parametrize('lag,n_windows,max_blocks', [(0, 7, 0), (0, 11, 0), (1, 17, 0), (1, 17, 1)])
def test_flush_window(hip, histories, dim, lag, n_windows, max_blocks):
  """The rolling flush: window (counter - lag) % n_windows.  1700 % 7 = 6 and 1699 % 17 = 16 are the LAST windows, 16 and 2
  rows of chunks of 19 and 8 (ragged); 1700 % 11 = 6 is a window in the middle.  Only the window's rows move."""
  H = histories('usual')
  s_end = S - lag
  st, _ = dc.case_reference('usual', dim, s_end)
  chunk = -(-dc.ROWS // n_windows)
  w = s_end % n_windows
  r = np.arange(dc.ROWS)
  listed = (r >= w * chunk) & (r < (w + 1) * chunk)
  assert 0 < listed.sum() and (listed.sum() < chunk) == (n_windows != 11)
  ref = _reference('usual', st, s_end, listed)
  dev = _Dev(hip, H, st)
  hip.emb_flush_window([dev.g], n_windows, H.hyper, lag=lag, max_blocks=max_blocks)
  got = dev.got()
  dc.check('flush_window', 'usual-d%d-lag%d-w%d-mb%d' % (dim, lag, n_windows, max_blocks), got, ref, dc.bounds_closed(ref))
  _expect_last(got, st, s_end, listed)
  dev.close()


def test_front_catches_up_from_the_heads(hip, histories):
  """emb_front without defer: the catch-up launch fed by the front's sort (the ids' rows are brought to counter - 2)."""
  H = histories('usual')
  for dim in (16, 1):
    st, _ = dc.case_reference('usual', dim, S - 1)
    listed = _listed(dc.ROWS)
    ids = np.random.default_rng(dim).permutation(np.flatnonzero(listed))
    ref = _reference('usual', st, S - 1, listed)
    dev = _Dev(hip, H, st, ids=ids)
    assert hip.emb_front([dev.g], H.hyper, False)
    got = dev.got()
    dc.check('front(catch-up from heads)', 'usual-d%d' % dim, got, ref, dc.bounds_closed(ref))
    _expect_last(got, st, S - 1, listed)
    dev.close()


# ------------------------------------------------------------------------------------------- lookup and row update in registers
def _lazy_step(hip, H, dev, grad):
  """emb_front(defer) + emb_fwd_lazy, then the row update with `grad` -> (looked-up rows, state after the lookup, state
  after the update)."""
  plan = hip.emb_plan_create([dev.spec])
  assert hip.emb_front([dev.g], H.hyper, False, defer=True)
  hip.emb_fwd_lazy(plan, [dev.g], H.hyper)
  torch.cuda.synchronize()
  out = dev.buf.cpu().numpy()
  mid = dev.got()
  dev.buf.copy_(torch.from_numpy(grad))
  scratch = torch.zeros_like(dev.buf)
  hip.emb_bwd_fused([dev.g], [(dev.buf, scratch, 0.0, True, [])], kernels.OPT_ADAM, H.hyper)
  end = dev.got()
  hip.emb_plan_destroy(plan)
  return out, mid, end


def _lazy_case(pair, dim, copies=1):
  """copies = 3: every id three times - runs of three sorted entries straddle the backward's tile boundaries (16 entries
  at dim 256, 64 at dim 64, 256 at dim 16), so the cross-tile fix launch applies update_row_lazy too; the gradients are
  then multiples of 2**-13, whose float32 sums are exact in any order."""
  st, _ = dc.case_reference(pair, dim, S - 1)
  listed = _listed(dc.ROWS)
  rng = np.random.default_rng(dim + copies)
  ids = rng.permutation(np.repeat(np.flatnonzero(listed), copies))
  if copies == 1:
    grad = (rng.standard_normal((len(ids), dim)) * 1e-3).astype(np.float32)
    grad[::5] = 0.0   # (a gradient of zero: the decay-only step through the row update)
  else:
    grad = (rng.integers(-8, 9, size=(len(ids), dim)) * 2.0**-13).astype(np.float32)
  return st, listed, ids, grad


@pytest.mark.parametrize('pair,dim,pitched,copies', [(p, d, False, 1) for p, d in CLOSED_GRID] +
                         [('usual', 16, True, 1), ('usual', 1, True, 1)] + [('usual', d, d == 64, 3) for d in (3, 16, 64, 256)])
def test_lazy_lookup_and_row_update(hip, histories, pair, dim, pitched, copies):
  """lazy_row: the looked-up rows are the reference's caught-up var and nothing is written back.  update_row_lazy
  (emb_bwd_fused behind the deferred front): replay followed by one Adam step, within the replay's bound carried through
  the step plus the step's own; rows without a gradient keep every bit."""
  H = histories(pair)
  st, listed, ids, grad = _lazy_case(pair, dim, copies)
  ref = _reference(pair, st, S - 1, listed)
  bound = dc.bounds_closed(ref)
  dev = _Dev(hip, H, st, ids=ids, pitched=pitched)
  if copies > 1:
    T = hip.emb_group_tile_entries(dev.g)
    assert T == ec.tile_entries(dim) and (dim == 3 or any(np.sort(ids)[t - 1] == np.sort(ids)[t] for t in range(T, len(ids), T)))
  out, mid, end = _lazy_step(hip, H, dev, grad)
  name = '%s-d%d%s-x%d' % (pair, dim, '-pitched' if pitched else '', copies)
  dc.check('fwd_lazy', name, {'var': out}, {'var': ref['var'][ids]}, {'var': bound['var'][ids]}, what=('var',))
  for k, a in (('var', st.var), ('m', st.m), ('v', st.v), ('last', st.last)):
    assert np.array_equal(mid[k], a), 'the lookup writes nothing back: %s' % k
  want, wbound = dc.adam_step(ref, bound, ids, grad, dc.hyper_rows(pair)[S - 1])
  dc.check('update_row_lazy', name, end, want, wbound)
  assert np.array_equal(end['last'], np.where(listed, S - 1, st.last))
  dev.close()


# ------------------------------------------------------------------------------------------- two pieces
@pytest.mark.parametrize('pair', ['usual', 'edge'])
def test_a_flush_in_the_middle_of_an_idle_interval(hip, histories, pair):
  """k1 steps by a flush at counter S - 100, the remaining 100 by a flush at S: two closed-form pieces against the
  recurrence over k1 + 100."""
  H = histories(pair)
  K, k2 = dc.EXPECTED_K[pair], 100
  ks = (k2 + 1, k2 + 2, k2 + 63, k2 + 64, k2 + 65, k2 + K - 1, k2 + K, k2 + K + 1, K - 1, K, K + 1, 700, 1500, 'all')
  st, ref = dc.case_reference(pair, 16, S, dc.ROWS, ks)
  assert (st.last < S - k2 - 1).all()
  b1, b2 = dc.betas(pair)
  ref1 = _reference(pair, st, S - k2)
  ref2 = dc.reference(ref1['var'], ref1['m'], ref1['v'], np.full(dc.ROWS, S - k2 - 1), S, dc.lr_history(pair), b1, b2, K=K)
  for k in ('var', 'm', 'v'):
    assert np.allclose(ref2[k], ref[k], rtol=1e-12, atol=1e-300)
  dev = _Dev(hip, H, st)
  with _counter_at(H, S - k2):
    hip.emb_flush_decay(dev.g, H.hyper)
  dc.check('flush_decay(first piece)', pair, dev.got(), ref1, dc.bounds_closed(ref1))
  hip.emb_flush_decay(dev.g, H.hyper)
  got = dev.got()
  dc.check('flush_decay(two pieces)', pair, got, ref, dc.bounds_two_pieces(ref1, ref2))
  assert (got['last'] == S - 1).all()
  dev.close()


# ------------------------------------------------------------------------------------------- the prologue-built lag-1 table
def test_prologue_built_table_equals_the_consumers_own(hip, histories):
  """decay_tables_set_prologue_build: the step prologue builds the lag-1 table from the counter decay_tables_sync left.
  Lookup and row update then give, bit for bit, what they give behind the table the front's own launch builds, and the
  stale-table flag stays down."""
  H = histories('usual')
  st, listed, ids, grad = _lazy_case('usual', 16)
  res = {}
  for mode in ('own', 'prologue'):
    dev = _Dev(hip, H, st, ids=ids)
    try:
      if mode == 'prologue':
        hip.decay_tables_set_prologue_build(H.tabs, True)
        H.counter.fill_(S - 1)       # step S - 1 once more: the same history entry, the same C row, counter == S again
        hip.decay_tables_sync(H.tabs)
        H.prologue(H.tabs)
      res[mode] = _lazy_step(hip, H, dev, grad)
      assert int(H.counter.item()) == S
    finally:
      hip.decay_tables_set_prologue_build(H.tabs, False)
      H.counter.fill_(S)
    dev.close()
  assert not hip.decay_tables_error(H.tabs)
  (out_a, mid_a, end_a), (out_b, mid_b, end_b) = res['own'], res['prologue']
  assert np.array_equal(out_a, out_b)
  for k in end_a:
    assert np.array_equal(end_a[k], end_b[k]) and np.array_equal(mid_a[k], mid_b[k]), k
  assert np.array_equal(H.hist[:S].cpu().numpy(), dc.lr_history('usual')[:S])


def test_a_table_built_for_another_step_raises_the_sticky_flag(hip, histories):
  """Two prologues with no lookup between: the second builds the table for the step the first one saw, the next lookup
  finds it stale and raises the flag; a correct step afterwards does not lower it.  (A flagged condition, not a fault:
  the lookup evaluates the table it was given.)"""
  H = histories('usual')
  tabs = hip.decay_tables_create(H.hist, H.counter, *dc.PAIRS['usual'])
  ks = (0, 1, 2, 63, 64, 65, dc.EXPECTED_K['usual'])   # (this table set has no C rows of its own: k <= K only)
  st, _ = dc.case_reference('usual', 16, S - 1, 35, ks)
  ids = np.arange(35)
  grad = np.zeros((35, 16), dtype=np.float32)
  try:
    hip.decay_tables_set_prologue_build(tabs, True)
    for stale in (True, False):
      dev = _Dev(hip, H, st, ids=ids, tables=False)
      hip.emb_group_set_decay_tables(dev.g, tabs)
      H.counter.fill_(S - 2 if stale else S - 1)
      hip.decay_tables_sync(tabs)
      for _ in range(2 if stale else 1):
        hip.step_prologue(H.rows_h, H.counter, H.hyper, history=H.hist, decay_tables=tabs)
      if stale:
        assert not hip.decay_tables_error(tabs)
      _lazy_step(hip, H, dev, grad)
      assert int(H.counter.item()) == S
      assert hip.decay_tables_error(tabs), 'raised by the stale table, and sticky'
      dev.close()
  finally:
    H.counter.fill_(S)
    torch.cuda.synchronize()
    hip.decay_tables_destroy(tabs)
  assert not hip.decay_tables_error(H.tabs)
  assert np.array_equal(H.hist[:S].cpu().numpy(), dc.lr_history('usual')[:S])
  assert np.array_equal(H.hyper.cpu().numpy(), dc.hyper_rows('usual')[S - 1])


# ------------------------------------------------------------------------------------------- step by step: exact replay, sweep
def _sweep(hip, H, st, s_end):
  """adam_decay_sweep once per step over the rows whose idle interval has begun (the bitmap skips the others)."""
  rows, dim = st.var.shape
  t = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731
  var, m, v = t(st.var), t(st.m), t(st.v)
  s_begin = st.last.astype(np.int64) + 1
  words = (rows + 31) // 32
  bitmap = torch.zeros(words, dtype=torch.int32, device=DEV)
  maps = {}
  for s in sorted(set(s_begin.tolist())):
    bits = np.zeros(words * 32, dtype=np.uint8)
    bits[:rows] = s_begin > s   # not idle yet at step s: skipped
    maps[s] = t(np.packbits(bits, bitorder='little').view(np.int32))
  hyper = torch.zeros_like(H.hyper)
  for s in range(int(s_begin.min()), s_end):
    if s in maps:
      bitmap.copy_(maps[s])
    hyper.copy_(H.rows_h[s])
    hip.adam_decay_sweep(var, m, v, bitmap, rows, dim, hyper)
  torch.cuda.synchronize()
  return {'var': var.cpu().numpy(), 'm': m.cpu().numpy(), 'v': v.cpu().numpy()}


@pytest.mark.parametrize('dim', [16, 3, 1])
def test_step_by_step_paths_and_which_form_is_closer(hip, histories, dim):
  """The exact replay (a group without tables: emb_flush_decay's and emb_catch_up's step-by-step branches) and the
  streaming sweep, on the closed form's cases against the same float64 recurrence, within the step-by-step bound.
  The sweep and the exact replay must agree bit for bit in var and m (the anchor of test_lazy_dense_decay_equals_the_sweep).
  Printed: the worst error of each form in units of the closed form's bound - er_decay.h claims the closed form is the
  closer one, which is asserted."""
  H = histories('usual')
  st, ref = dc.case_reference('usual', dim, S)
  sb, cb = dc.bounds_steps(ref), dc.bounds_closed(ref)
  dev = _Dev(hip, H, st, tables=False)
  hip.emb_flush_decay(dev.g, H.hyper)
  exact = dev.got()
  dev.close()
  dc.check('exact_replay(flush)', 'usual-d%d' % dim, exact, ref, sb)
  assert (exact['last'] == S - 1).all()
  swept = _sweep(hip, H, st, S)
  dc.check('sweep', 'usual-d%d' % dim, swept, ref, sb)
  assert np.array_equal(swept['var'], exact['var']) and np.array_equal(swept['m'], exact['m'])
  dev = _Dev(hip, H, st)
  hip.emb_flush_decay(dev.g, H.hyper)
  closed = dev.got()
  dev.close()
  worst = {}
  for who, got in (('closed', closed), ('exact', exact)):
    worst[who] = dc.ratio(got['var'], ref['var'], cb['var'])
    print('RATIO who=%s-in-units-of-the-closed-bound case=usual-d%d tensor=var ratio=%.4g' % (who, dim, worst[who]))
  assert worst['closed'] <= worst['exact']
  # the exact catch-up launch (emb_catch_up_kernel -> replay_block's queues)
  st1, _ = dc.case_reference('usual', dim, S - 1)
  listed = _listed(dc.ROWS)
  ref1 = _reference('usual', st1, S - 1, listed)
  dev = _Dev(hip, H, st1, tables=False)
  keys, nu = _keys(listed)
  hip.emb_catch_up(dev.g, keys, nu, H.hyper)
  got = dev.got()
  dc.check('exact_replay(catch_up)', 'usual-d%d' % dim, got, ref1, dc.bounds_steps(ref1))
  _expect_last(got, st1, S - 1, listed)
  dev.close()


def test_refused_betas_replay_step_by_step(hip, histories):
  H = histories('refused')
  st, ref = dc.case_reference('refused', 16, S)
  dev = _Dev(hip, H, st)
  assert dev.g.get('decay_tables') is None
  hip.emb_flush_decay(dev.g, H.hyper)
  got = dev.got()
  dc.check('exact_replay(refused betas)', 'refused-d16', got, ref, dc.bounds_steps(ref))
  assert (got['last'] == S - 1).all()
  dev.close()
