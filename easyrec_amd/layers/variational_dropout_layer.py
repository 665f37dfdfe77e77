"""Variational dropout on the input layer (reference easy_rec/python/layers/variational_dropout_layer.py; "Dropout Feature
Ranking for Deep Learning Models", arXiv 1712.08645): a learned dropout probability per feature - or, embedding-wise,
per embedding column - on a feature group's concatenated output, and a penalty on the loss that pushes the
probabilities up.  The trained probabilities rank the features (EasyRecEstimator.feature_importance,
tools/feature_selection.py).

  variable    logit_p_<group> (`logit_p` for the group `all`), shape [W] embedding-wise, [number of features] otherwise;
              tf.get_variable's default initializer, glorot uniform (rank 1: fan_in = fan_out = the length); no L2.
  training    p = sigmoid(logit_p), u ~ U[0, 1) of shape [rows, P], EPS = np.finfo(float).eps:
              a = log(p + EPS) - log(1 - p + EPS) + log(u + EPS) - log(1 - u + EPS);  m = 1 - sigmoid(a / 0.1)
              out[b, c] = x[b, c] * m[b, seg(c)], seg(c) the feature that owns column c (embedding-wise: c itself)
  otherwise   out = x * (1 - p[seg(c)])
  penalty     regularization_lambda / rows * sum(1 - p), collected per step in the model context (`vdrop_losses`) as
              the reference collects it in `variational_dropout_loss`.

The noise is drawn by this layer with torch.rand on the device's generator and handed to the kernel as an operand, so a
test can feed the same draw to a restatement; it matches TensorFlow's noise in distribution only.

Which path runs is decided by what the code can see.  On the HIP backend, with fp32 tensors on the GPU, a 2-D non-empty x
and a width inside the kernel's envelope (vdrop_fits, include/easyrec_hip.h K8k), ONE launch each way does the mask, the
multiply, the penalty and - with the shared fixed-order reduce - logit_p's gradient (kernels.VDropFn, csrc/er_vdrop.hip).
Anywhere else - a stand-in backend on the CPU, a width outside the envelope, EASYREC_AMD_FUSED_VDROP=0 - vdrop_compose
runs: the same formulas as torch ops.
"""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from easyrec_amd import kernels
from easyrec_amd.core import context

FUSED_DEFAULT = '1'  # EASYREC_AMD_FUSED_VDROP when the environment does not set it
MAX_WIDTH = 4096     # er_vdrop_*: W
EPSILON = float(np.finfo(float).eps)
TEMPERATURE = 1.0 / 10.0


def fused_enabled():
  """EASYREC_AMD_FUSED_VDROP=0: the torch composition everywhere (the A/B switch of the K8k kernel)."""
  return os.environ.get('EASYREC_AMD_FUSED_VDROP', FUSED_DEFAULT) != '0'


def vdrop_fits(W):
  """er_vdrop_grid(B, W) > 0 for B >= 1"""
  return 1 <= W <= MAX_WIDTH


def vdrop_compose(x, logit_p, u, seg, lam):
  """x [rows, W], logit_p [P], u [rows, P] or None (evaluation), seg: int64 [W] column -> parameter or None (identity),
  lam = regularization_lambda / rows -> (x * m, penalty [1])"""
  p = torch.sigmoid(logit_p)
  if u is None:
    m = (1. - p).unsqueeze(0)
  else:
    approx = torch.log(p + EPSILON) - torch.log(1. - p + EPSILON) + torch.log(u + EPSILON) - torch.log(1. - u + EPSILON)
    m = 1 - torch.sigmoid(approx / TEMPERATURE)
  if seg is not None:
    m = m.index_select(1, seg)
  return x * m, (lam * (1. - p).sum()).reshape(1)


def feature_importance(logit_p, features_dimension, embedding_wise):
  """reference tools/feature_selection.py:116-151: feature -> its dropout probability sigmoid(logit_p) (embedding-wise:
  the mean over the feature's columns), sorted ascending - the features a model can least do without come first."""
  p = 1.0 / (1.0 + np.exp(-np.asarray(logit_p, dtype=np.float32).astype(np.float64)))
  importance, end = {}, 0
  for i, (name, dim) in enumerate(features_dimension.items()):
    if embedding_wise:
      start, end = end, end + dim
      importance[name] = np.mean(p[start:end])
    else:
      importance[name] = p[i]
  return OrderedDict(sorted(importance.items(), key=lambda e: e[1]))


def _fused(x):
  return x.is_cuda and x.dtype == torch.float32 and isinstance(kernels.hip(), kernels.HipBackend)


class VariationalDropoutLayer(object):
  """Rank features by variational dropout: the reference's constructor and call contract."""

  def __init__(self, variational_dropout_config, features_dimension, is_training=False, name=''):
    self._config = variational_dropout_config
    self.features_dimension = OrderedDict(features_dimension)
    self.features_total_dimension = sum(self.features_dimension.values())
    if self.variational_dropout_wise():
      self._dropout_param_size = self.features_total_dimension
    else:
      self._dropout_param_size = len(self.features_dimension)
    self.drop_param_shape = [self._dropout_param_size]
    self.evaluate = not is_training
    self.name = name
    logit_p_name = 'logit_p' if name == 'all' else 'logit_p_%s' % name
    self.logit_p = context.varstore().get_variable(logit_p_name, tuple(self.drop_param_shape), 'glorot_uniform')
    # (what the reference adds to the `variational_dropout` collection: the group and its features' widths)
    self.collection_entry = json.dumps([name, list(self.features_dimension.items())])
    self._seg = {}  # device -> (kernels.VDropSeg or None, int64 index or None)

  def get_lambda(self):
    return self._config.regularization_lambda

  def variational_dropout_wise(self):
    return self._config.embedding_wise_variational_dropout

  def _segments(self, device, fused):
    """the column -> parameter map as the path that runs reads it; None embedding-wise"""
    if self.variational_dropout_wise():
      return None
    key = (str(device), fused)
    if key not in self._seg:
      dims = list(self.features_dimension.values())
      if fused:
        self._seg[key] = kernels.VDropSeg(dims, device)
      else:
        self._seg[key] = torch.repeat_interleave(torch.arange(len(dims)), torch.tensor(dims)).to(device)
    return self._seg[key]

  def sample_noise(self, rows, device):
    """unif_noise: [rows, P] on the device's generator; None outside training (a layer built for evaluation, or a
    training estimator's evaluate(), which clears the context's is_training)"""
    if self.evaluate or not getattr(context.current(), 'is_training', True):
      return None
    return torch.rand(rows, self._dropout_param_size, dtype=torch.float32, device=device)

  def apply(self, output_features, u):
    """(noisy input, penalty [1]) for the draw u"""
    x = output_features
    assert x.dim() == 2 and int(x.shape[1]) == self.features_total_dimension, \
        'variational dropout %s: input %s, the features are %d wide' % (self.name, tuple(x.shape), self.features_total_dimension)
    lam = float(self.get_lambda()) / max(int(x.shape[0]), 1)
    fused = fused_enabled() and x.numel() > 0 and _fused(x) and vdrop_fits(int(x.shape[1]))
    seg = self._segments(x.device, fused)
    if fused:
      grads = [self.logit_p.grad] if self.logit_p.grad is not None else None
      return kernels.VDropFn.apply(grads, x, self.logit_p, u, seg, lam)
    return vdrop_compose(x, self.logit_p, u, seg, lam)

  def __call__(self, output_features):
    out, penalty = self.apply(output_features, self.sample_noise(int(output_features.shape[0]), output_features.device))
    context.current().vdrop_losses.append(penalty)
    return out
