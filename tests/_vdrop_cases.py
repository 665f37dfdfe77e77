"""Variational dropout restated in plain torch, fp64, from the formulas of the reference's
layers/variational_dropout_layer.py; the fixture tests/golden/vdrop_vectors.npz; and the seeded inputs of the kernel
tests.  Shared by tests/test_vdrop_pins.py and tests/test_vdrop_gpu.py."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)
TEMP = 0.1
ROWS_PER_WG, GRID_CAP, MAX_W = 8, 1024, 4096  # er_vdrop_grid = min(ceil(B / 8), 1024) for 1 <= W <= 4096, B >= 1

# (B, the features' widths): the smallest; scalar lanes with unaligned segments; vector lanes; mixed widths; a wide group
# of one-column features; more than one workgroup; the sample (39 features of 16, batch 4096); the envelope's edge
KERNEL_CASES = [(5, (1,)), (13, (1, 3, 4)), (9, (16, 16, 16)), (77, (16, 8, 1, 4, 3)), (64, (1,) * 22), (301, (16,) * 17),
                (4096, (16,) * 39), (3, (4096,))]
MODES = ('embedding_wise', 'feature_wise')
LAMBDA = 0.01
DPENALTY = 0.75  # the upstream gradient of the penalty in the kernel tests


def gold():
  return np.load(os.path.join(ROOT, 'tests', 'golden', 'vdrop_vectors.npz'))


def seg_of(dims):
  """the column -> parameter map of the feature-wise form"""
  return np.repeat(np.arange(len(dims)), np.asarray(dims, dtype=np.int64))


def grid_of(B, W):
  """the Python twin of er_vdrop_grid"""
  if B < 1 or W < 1 or W > MAX_W:
    return 0
  return min(-(-B // ROWS_PER_WG), GRID_CAP)


# ------------------------------------------------------------------------------------------------ the restatement
def mask(logit_p, u):
  """m [rows, P] (training) or [1, P] (u None: evaluation and prediction)"""
  p = 1.0 / (1.0 + torch.exp(-logit_p))
  if u is None:
    return (1.0 - p)[None, :]
  a = torch.log(p + EPS) - torch.log(1.0 - p + EPS) + torch.log(u + EPS) - torch.log(1.0 - u + EPS)
  return 1.0 - torch.sigmoid(a / TEMP)


def vdrop(x, logit_p, u, dims, embedding_wise, lam):
  """-> (out [rows, W], penalty): dims the features' widths; lam = regularization_lambda"""
  m = mask(logit_p, u)
  if not embedding_wise:
    m = m[:, torch.from_numpy(seg_of(dims))]
  p = 1.0 / (1.0 + torch.exp(-logit_p))
  return x * m, lam / x.shape[0] * (1.0 - p).sum()


# ------------------------------------------------------------------------------------------------ the kernel tests' inputs
def kernel_inputs(B, dims, embedding_wise, seed=0, logit_range=10.0):
  """(x, logit_p, u, dout), fp64 tensors holding fp32 values; logit_p uniform in [-10, 10]; u uniform in [0, 1) with an
  exact 0 and the largest fp32 below 1"""
  W = int(sum(dims))
  P = W if embedding_wise else len(dims)
  g = torch.Generator().manual_seed(1000 * seed + 7 * B + W + (1 if embedding_wise else 0))
  f32 = lambda t: t.float().double()
  x = f32(torch.randn(B, W, generator=g, dtype=torch.float64))
  d = f32(torch.randn(B, W, generator=g, dtype=torch.float64))
  logit_p = f32((torch.rand(P, generator=g, dtype=torch.float64) * 2 - 1) * logit_range)
  u = torch.rand(B, P, generator=g, dtype=torch.float32)
  u[0, 0] = 0.0
  u[-1, -1] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
  assert float(u.max()) < 1.0
  return x, logit_p, u.double(), d


def want(x, logit_p, u, d, dims, embedding_wise, lam=LAMBDA, dpenalty=DPENALTY):
  """fp64 autograd of the restatement: (out, penalty, dx, dlogit_p of out alone, dlogit_p of the penalty alone)"""
  xr, lr = x.clone().requires_grad_(True), logit_p.clone().requires_grad_(True)
  out, pen = vdrop(xr, lr, u, dims, embedding_wise, lam)
  out.backward(d, retain_graph=True)
  dx, dl_out = xr.grad.clone(), lr.grad.clone()
  lr.grad = None
  (pen * dpenalty).backward()
  return out.detach(), pen.detach(), dx, dl_out, lr.grad.clone()
