"""-m gpu: the embedding backward (key sort -> emb_bwd_tile_kernel -> emb_bwd_fix_kernel -> finish_run / update_row)
against the float64 reference of tests/_emb_bwd_cases.py at every lane geometry, with runs of equal keys PLACED on the
tile boundaries (tests/test_emb_bwd_pins.py shows on the CPU that the cases reach the branches they claim, that the
reference is right and that a wrong one would be noticed).

Bars: bit equality on the exact inputs (every float32 partial sum in any order is exact there); on the random inputs
GPU_FACTOR x the measured float32 error of the source-order restatement (MEASURED, all under BAR_CAP = 1e-3); for the
ragged row sums the bound of any float32 summation order.  No number here comes from the kernels.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from tests import _emb_bwd_cases as ec  # noqa: E402

DEV = 'cuda:0'
OPTS = {ec.OPT_SGD: kernels.OPT_SGD, ec.OPT_ADAM: kernels.OPT_ADAM, ec.OPT_LAZY_ADAM: kernels.OPT_LAZY_ADAM,
        ec.OPT_ADAGRAD: kernels.OPT_ADAGRAD}


@pytest.fixture(scope='module')
def hip():
  assert torch.cuda.is_available(), 'gpu tests need an MI355X'
  assert kernels.HYPER_FLOATS == ec.HYPER_FLOATS
  assert (kernels.COMBINERS['sum'], kernels.COMBINERS['mean'], kernels.COMBINERS['sqrtn']) == (ec.SUM, ec.MEAN, ec.SQRTN)
  return kernels.hip()


def _accepts(dim):
  """validate_descs of er_embedding.hip: 1..1024, and a multiple of 4 or <= 64."""
  return 0 < dim <= 1024 and (dim % 4 == 0 or dim <= 64)


class _Group(object):
  """A case on the device: fresh copies of its table / m / v, the group handle, the bitmap."""

  def __init__(self, hip, case):
    self.hip, self.case = hip, case
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)  # noqa: E731
    self.var, self.m, self.v = dev(case.table.copy()), dev(case.m.copy()), dev(case.v.copy())
    self.dout = dev(case.dout)
    self.bitmap = torch.zeros((case.total_rows + 31) // 32, dtype=torch.int32, device=DEV)
    specs = [kernels.LookupSpec(table=self.var[lk['key_base']:lk['key_base'] + lk['rows']], ids=dev(lk['ids']),
                                offsets=dev(lk['offsets']), weights=dev(lk['weights']), out=self.dout, out_col=lk['out_col'],
                                rows=lk['rows'], key_base=lk['key_base'], dim=case.dim, combiner=lk['combiner'],
                                n_rows=lk['n_rows'], max_nnz=lk['max_nnz']) for lk in case.lookups]
    self.g = hip.emb_group_create(specs, case.dim, case.total_rows, self.var, self.m, self.v, self.bitmap)
    assert self.g['num_entries'] == case.num_entries
    assert hip.emb_group_tile_entries(self.g) == ec.tile_entries(case.dim) == case.T

  def state(self):
    torch.cuda.synchronize()
    return {'var': self.var.cpu().numpy(), 'm': self.m.cpu().numpy(), 'v': self.v.cpu().numpy()}

  def close(self):
    self.hip.emb_group_destroy(self.g)


def _open(hip, case):
  """-> _Group, or None after asserting the library's refusal of the dim."""
  if _accepts(case.dim):
    return _Group(hip, case)
  with pytest.raises(RuntimeError, match='er_emb_group_create.*dim %d (out of range|must be a multiple of 4 or <= 64)' % case.dim):
    _Group(hip, case)
  return None


def _hyper(inputs, clip=0.0):
  h = ec.hyper_of(inputs, clip)
  return h, torch.from_numpy(h).to(DEV)


def _f32(a):
  return torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))


def _reduce(hip, grp):
  keys, grads, n = hip.emb_bwd_reduce(grp.g)
  torch.cuda.synchronize()
  n = int(n.item())
  return keys[:n].cpu(), grads[:n].cpu(), n


def test_every_dim_of_the_grid_is_accepted_or_refused_with_a_reason(hip):
  assert all(_accepts(d) for d in ec.DIMS)  # (none refused today: _open asserts the message for one that is)
  case = ec.make_case(5, 'all_distinct', 'one', 'exact')
  case = ec.Case(**dict(case.__dict__, dim=65, table=np.zeros((case.total_rows, 65), dtype=np.float32),
                        m=np.zeros((case.total_rows, 65), dtype=np.float32), v=np.ones((case.total_rows, 65), dtype=np.float32),
                        dout=np.zeros((case.dout.shape[0], 65), dtype=np.float32)))
  assert _open(hip, case) is None


# ------------------------------------------------------------------------------------------- exact inputs
@pytest.mark.parametrize('dim,plan,split', ec.exact_grid())
def test_reduce_is_exact(hip, dim, plan, split):
  case = ec.make_case(dim, plan, split, 'exact')
  grp = _open(hip, case)
  if grp is None:
    return
  sums, touched, _, _ = ec.row_sums(case)
  keys, grads, n = _reduce(hip, grp)
  assert n == len(touched)
  assert np.array_equal(keys.numpy(), touched)
  assert torch.equal(grads, _f32(sums[touched])), float((grads.double() - torch.from_numpy(sums[touched])).abs().max())
  keys2, grads2, n2 = _reduce(hip, grp)
  assert n2 == n and torch.equal(keys2, keys) and torch.equal(grads2, grads)
  assert torch.equal(grp.var.cpu(), torch.from_numpy(case.table))  # (reduce mode applies nothing)
  grp.close()


@pytest.mark.parametrize('dim,plan,split,clip', [g + (0.0,) for g in ec.exact_grid()] + [(d, 'base', 'one', 0.25) for d in ec.DIMS])
def test_sgd_update_is_exact(hip, dim, plan, split, clip):
  case = ec.make_case(dim, plan, split, 'exact')
  grp = _open(hip, case)
  if grp is None:
    return
  h, hd = _hyper('exact', clip)
  want = ec.reference(case, ec.OPT_SGD, h)
  hip.emb_bwd_update(grp.g, kernels.OPT_SGD, hd)
  got = grp.state()
  assert torch.equal(torch.from_numpy(got['var']), _f32(want['var'])), float(np.abs(got['var'] - want['var']).max())
  untouched = np.setdiff1d(np.arange(case.total_rows), want['touched'])
  assert len(untouched) and np.array_equal(got['var'][untouched], case.table[untouched])
  assert np.array_equal(got['m'], case.m) and np.array_equal(got['v'], case.v)  # (SGD has no slots)
  grp.close()


@pytest.mark.parametrize('dim', ec.DIMS)
def test_a_group_of_invalid_ids_changes_nothing(hip, dim):
  case = ec.make_case(dim, 'all_invalid', 'one', 'exact')
  grp = _open(hip, case)
  if grp is None:
    return
  _, _, n = _reduce(hip, grp)
  assert n == 0
  h, hd = _hyper('random')
  for opt in (ec.OPT_SGD, ec.OPT_LAZY_ADAM, ec.OPT_ADAGRAD):
    hip.emb_bwd_update(grp.g, OPTS[opt], hd)
    got = grp.state()
    assert np.array_equal(got['var'], case.table) and np.array_equal(got['m'], case.m) and np.array_equal(got['v'], case.v)
    assert int(grp.bitmap.abs().sum()) == 0
  # TF's Adam: every row takes the g = 0 step.  m, v: one product (U |result|).  var: the step lr_t m_t / (sqrt(v_t) + eps)
  # carries m_t's and v_t's roundings (1 + 1/2), sqrtf, the addition, the product and the division: <= 6 U |step|, then the
  # subtraction's U |result|
  want = ec.reference(case, ec.OPT_ADAM, h)
  hip.emb_bwd_update(grp.g, kernels.OPT_ADAM, hd)
  got = grp.state()
  assert int(grp.bitmap.abs().sum()) == 0
  for what, init in (('var', case.table), ('m', case.m), ('v', case.v)):
    bound = ec.U * (np.abs(want[what]) + 6 * np.abs(want[what] - init))
    assert np.all(np.abs(got[what] - want[what]) <= bound), what
  grp.close()


# ------------------------------------------------------------------------------------------- random inputs
def _two_updates_within_the_bars(hip, grp, opt):
  case = grp.case
  h, hd = _hyper('random')
  want = ec.reference(case, opt, h, steps=2)
  for _ in range(2):
    hip.emb_bwd_update(grp.g, OPTS[opt], hd)
  got = grp.state()
  assert int(grp.bitmap.abs().sum()) == 0  # Adam's touched-row bitmap comes back clean
  for what, init in (('var', case.table), ('m', case.m), ('v', case.v)):
    if what in ec.quantities(opt):
      err, bar = ec.rel_err(got[what], want[what], init), ec.gpu_bar(case, opt, what)
      print('%-52s err %.3e bar %.3e' % (ec.measured_key(case, opt, what), err, bar))
      assert err <= bar, (ec.measured_key(case, opt, what), err, bar)
    else:
      assert np.array_equal(got[what], init), what
  if opt != ec.OPT_ADAM:
    untouched = np.setdiff1d(np.arange(case.total_rows), want['touched'])
    assert len(untouched)
    for what, init in (('var', case.table), ('m', case.m), ('v', case.v)):
      assert np.array_equal(got[what][untouched], init[untouched]), what


@pytest.mark.parametrize('opt', [ec.OPT_ADAM, ec.OPT_LAZY_ADAM, ec.OPT_ADAGRAD], ids=lambda o: ec.OPT_NAMES[o])
@pytest.mark.parametrize('plan', ['base', 'with_invalid'])
@pytest.mark.parametrize('dim', ec.OPT_DIMS)
def test_optimizers_match_fp64(hip, dim, plan, opt):
  grp = _open(hip, ec.make_case(dim, plan, 'three', 'random'))
  if grp is None:
    return
  _two_updates_within_the_bars(hip, grp, opt)
  grp.close()


@pytest.mark.parametrize('dim', ec.RAGGED_DIMS)
def test_ragged_combiners_match_fp64(hip, dim):
  case = ec.make_case(dim, 'base', 'ragged', 'random')
  grp = _open(hip, case)
  if grp is None:
    return
  sums, touched, asum, cnt = ec.row_sums(case)
  keys, grads, n = _reduce(hip, grp)
  assert n == len(touched) and np.array_equal(keys.numpy(), touched)
  # any float32 summation order of n terms: (n - 1) U sum|terms|; each term carries two roundings (w / den, the product)
  bound = ((cnt[touched] - 1)[:, None] + 2) * ec.U * asum[touched]
  diff = np.abs(grads.numpy().astype(np.float64) - sums[touched])
  print('ragged dim %d: max |diff| / bound = %.3f' % (dim, float(np.max(diff / np.maximum(bound, 1e-300)))))
  assert np.all(diff <= bound)
  _two_updates_within_the_bars(hip, grp, ec.OPT_ADAM)
  grp.close()


# ------------------------------------------------------------------------------------------- the other entry points
@pytest.mark.parametrize('dim', ec.RAGGED_DIMS)
def test_apply_unique_and_dense_reduce_agree_with_update(hip, dim):
  case = ec.make_case(dim, 'base', 'three', 'exact')
  a, b = _open(hip, case), _open(hip, case)
  h, hd = _hyper('exact')
  hip.emb_bwd_update(a.g, kernels.OPT_SGD, hd)
  keys, grads, n = hip.emb_bwd_reduce(b.g)
  hip.emb_apply_unique(b.g, keys, grads, n, kernels.OPT_SGD, hd)
  sa, sb = a.state(), b.state()
  assert np.array_equal(sa['var'], sb['var'])
  assert np.array_equal(sa['var'], ec.reference(case, ec.OPT_SGD, h)['var'].astype(np.float32))
  # mode 2: the sums at key * ld, 1.0 at column dim; columns past it and the rows of other keys stay as they were
  sums, touched, _, _ = ec.row_sums(case)
  ld = dim + 3
  dense = torch.full((case.total_rows, ld), -7.0, device=DEV)
  hip.emb_bwd_reduce_dense([b.g], [dense])
  torch.cuda.synchronize()
  want = np.full((case.total_rows, ld), -7.0, dtype=np.float32)
  want[touched, :dim] = sums[touched].astype(np.float32)
  want[touched, dim] = 1.0
  assert np.array_equal(dense.cpu().numpy(), want)
  assert np.array_equal(b.state()['var'], sb['var'])
  a.close()
  b.close()


def test_update_multi_equals_single_launches(hip):
  cases = [ec.make_case(d, 'base', 'three', 'random') for d in ec.RAGGED_DIMS]
  single, multi = [_open(hip, c) for c in cases], [_open(hip, c) for c in cases]
  _, hd = _hyper('random')
  for _ in range(2):
    for grp in single:
      hip.emb_bwd_update(grp.g, kernels.OPT_ADAM, hd)
    hip.emb_bwd_update_multi([grp.g for grp in multi], kernels.OPT_ADAM, hd)
  for s, m in zip(single, multi):
    ss, sm = s.state(), m.state()
    for what in ('var', 'm', 'v'):
      assert np.array_equal(ss[what], sm[what]), (s.case.name, what)
      assert not np.array_equal(ss[what], getattr(s.case, {'var': 'table'}.get(what, what)))
    assert int(m.bitmap.abs().sum()) == 0 and int(s.bitmap.abs().sum()) == 0
    s.close()
    m.close()
