"""The packed-parameter gradient reduce (csrc/er_theta.hip, easyrec_hip.h K8e) on the GPU, called directly: exact sums
on integer inputs, the summation order easyrec_hip.h states for row_groups 1 and 8 bit for bit, and the calls it
refuses."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from easyrec_amd import kernels  # noqa: E402
from tests._oracle_steps import assert_runs_and_replay_bit_identical  # noqa: E402

DEV = 'cuda:0'
P = 1111  # neither a multiple of 256 nor of 32: the last workgroup of either order is partly idle
MAX_SEGS = 392


def _full():
  lens = [(1, 2, 5)[i % 3] for i in range(MAX_SEGS - 1)]
  return lens + [P - sum(lens)]


SEGMENTS = {'single': [P], 'with_ones': [1, 1, 300, 1, 255, 1, 33, P - 592], 'full_392': _full()}
assert all(sum(v) == P and min(v) >= 1 for v in SEGMENTS.values()) and len(SEGMENTS['full_392']) == MAX_SEGS


def _buffers(lens, seed):
  """The gradient buffers (one tensor each, as the variables' are) and what they hold before the reduce."""
  gen = torch.Generator().manual_seed(seed)
  before = [torch.randint(-4, 5, (n,), generator=gen).to(DEV, torch.float32) for n in lens]
  grads = [torch.empty_like(b) for b in before]
  return grads, before


def _reduce_runs(partials, rows, lens, row_groups, acc, seed=1):
  """-> the buffers after the reduce (two runs and a graph replay agree), and what they held before"""
  be = kernels.hip()
  grads, before = _buffers(lens, seed)
  table = kernels.ThetaGradTable(grads)

  def run():
    for g, b in zip(grads, before):
      g.copy_(b)
    be.theta_grad_reduce(partials, rows, table, row_groups, acc)
    return [g.clone() for g in grads]

  assert_runs_and_replay_bit_identical(run)
  torch.cuda.synchronize()
  return torch.cat(grads).cpu().numpy(), torch.cat(before).cpu().numpy()


@pytest.mark.parametrize('acc', [False, True], ids=['write', 'add'])
@pytest.mark.parametrize('row_groups', [1, 8])
@pytest.mark.parametrize('segs', sorted(SEGMENTS))
@pytest.mark.parametrize('rows', [1, 7, 512])
def test_integer_partials_sum_exactly(rows, segs, row_groups, acc):
  """Small integers in fp32: every order of summation gives the same bits, so the result IS partials.sum(0), split by
  the segments' lengths (and added to what the buffers held, with acc)."""
  lens = SEGMENTS[segs]
  gen = torch.Generator().manual_seed(rows + len(lens))
  partials = torch.randint(-8, 9, (rows, P), generator=gen).to(DEV, torch.float32)
  got, before = _reduce_runs(partials, rows, lens, row_groups, acc)
  want = partials.sum(0).cpu()
  assert torch.equal(want.double(), partials.double().sum(0).cpu())  # (the expectation itself is exact)
  want = want.numpy() + before if acc else want.numpy()
  assert got.dtype == np.float32 and np.array_equal(got, want)
  o = 0
  for n in lens:  # (split by lens: every buffer holds its own stretch)
    assert np.array_equal(got[o:o + n], want[o:o + n])
    o += n


def _ordered_sum(p, row_groups):
  """easyrec_hip.h K8e in NumPy float32: row group g sums rows g, g + row_groups, .. in order from 0.f; the groups' sums
  are combined in order 0, 1, ...  (The library is built with -ffp-contract=off and the kernel only adds.)"""
  sums = []
  for g in range(row_groups):
    s = np.zeros(p.shape[1], np.float32)
    for r in range(g, p.shape[0], row_groups):
      s = s + p[r]
    sums.append(s)
  total = sums[0]
  for s in sums[1:]:
    total = total + s
  assert total.dtype == np.float32
  return total


@pytest.mark.parametrize('acc', [False, True], ids=['write', 'add'])
@pytest.mark.parametrize('row_groups', [1, 8])
@pytest.mark.parametrize('rows', [1, 7, 512])
def test_summation_order_is_the_stated_one(rows, row_groups, acc):
  """Random fp32 partials over several binades: bit-equal to the stated order, which BST (1) and FiBiNet (8) rely on."""
  gen = torch.Generator().manual_seed(100 + rows)
  partials = (torch.randn(rows, P, generator=gen) * torch.exp2(torch.randint(-6, 7, (rows, P), generator=gen).float()))
  partials = partials.to(DEV)
  got, before = _reduce_runs(partials, rows, SEGMENTS['full_392'], row_groups, acc)
  want = _ordered_sum(partials.cpu().numpy(), row_groups)
  if row_groups == 8 and rows == 512:  # (the two orders do differ on these inputs: the comparison can tell them apart)
    assert not np.array_equal(want, _ordered_sum(partials.cpu().numpy(), 1))
  if acc:
    want = before + want
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('row_groups', [1, 8])
def test_bad_calls_raise_and_launch_nothing(row_groups):
  be = kernels.hip()
  lens = SEGMENTS['with_ones']
  rows = 7
  grads, before = _buffers(lens, seed=5)
  for g, b in zip(grads, before):
    g.copy_(b)
  good = torch.ones(rows, P, device=DEV)
  table = kernels.ThetaGradTable(grads)
  with pytest.raises(RuntimeError, match='er_theta_grad_reduce'):  # sum(lens) != P
    be.theta_grad_reduce(torch.ones(rows, P + 1, device=DEV), rows, table, row_groups, False)
  with pytest.raises(RuntimeError, match='er_theta_grad_reduce'):
    be.theta_grad_reduce(torch.ones(rows, P - 1, device=DEV), rows, table, row_groups, False)
  holed = kernels.ThetaGradTable(grads)
  holed.table[3] = None  # a null pointer in the table
  with pytest.raises(RuntimeError, match='is null'):
    be.theta_grad_reduce(good, rows, holed, row_groups, False)
  with pytest.raises(RuntimeError, match='row_groups'):
    be.theta_grad_reduce(good, rows, table, 4, False)
  ones = [torch.zeros(1, device=DEV) for _ in range(MAX_SEGS + 1)]  # one segment beyond the table's capacity
  with pytest.raises(RuntimeError, match='segments'):
    be.theta_grad_reduce(torch.ones(rows, MAX_SEGS + 1, device=DEV), rows, kernels.ThetaGradTable(ones), row_groups, False)
  torch.cuda.synchronize()
  assert all(torch.equal(g, b) for g, b in zip(grads, before))
  assert all(float(t) == 0.0 for t in ones)
  be.theta_grad_reduce(good, rows, table, row_groups, False)  # (and the same table and partials are accepted)
  torch.cuda.synchronize()
  assert all(torch.equal(g, torch.full_like(g, float(rows))) for g in grads)
