"""FiBiNET's backbone blocks (reference easy_rec/python/layers/keras/fibinet.py): `SENet` (:15-93), `BiLinear`
(:103-203) and `FiBiNet` (:206-251), over a list of field embeddings [B, D_f].

  SENet    per field and squeeze group the max and the mean over the group's columns -> Dense W1 (relu) -> Dense W2
           (sum of the dims) -> re-weight the concatenated embeddings (+ skip connection, + LayerNormalization).
  BiLinear u_i = Dense_i(x_i) for i < F - 1 (`each`; `all`: one Dense for every field), then for the pairs (i, j) in
           itertools.combinations order <u_i, x_j> (use_plus) or u_i * x_j, concatenated, -> Dense `output`.
  FiBiNet  concat(SENet(x), BiLinear(x)) -> MLP; only the MLP carries the block's L2 regulariser (:228-231).

Which path runs is decided by what the code can see.  On the HIP backend, with fields of one width side by side in one
[B, F * D] tensor and a geometry inside the kernels' LDS envelope (bilinear_fits / senet_fits below, the formulas of
include/easyrec_hip.h K8d), BiLinear's interaction and FiBiNet's SENet are one forward and one backward launch each
(kernels.BiLinearFn / SENetFn, csrc/er_fibinet.hip).  Anywhere else - a stand-in backend on the CPU, unequal widths for
SENet, a geometry outside the envelope - the same block is composed of torch ops (bilinear_compose / senet_compose).

The STAND-ALONE `SENet` block keeps the composed path and its bits on every backend: the reference fixture
`samples/model_config/mmoe_backbone_on_taobao.config` puts it in front of MMoE, tests/test_models_gpu.py holds that
model to the oracle with seeds picked to avoid ReLU ties, and a last-bit change upstream of MMoE could land on one.
Only `FiBiNet` routes its SENet through the fused kernels; moving the stand-alone block over is a follow-up.

`type: interaction` cannot run in the reference: BiLinear.call (:197-201) indexes its list of F (F - 1) / 2 layers
with i * field_num + j, which leaves the list for every F >= 2 (IndexError; recorded in
tests/golden/fibinet_vectors.npz).  Here it raises NotImplementedError at build time.  fp32 only: with
--dense_dtype bf16 the blocks raise ValueError at build time.
"""
import itertools
import logging
import math

import torch

from easyrec_amd import kernels
from easyrec_amd.core import context
from easyrec_amd.core.variables import truncated_normal
from easyrec_amd.layers import dnn
from easyrec_amd.layers.keras.blocks import MLP
from easyrec_amd.layers.utils import Parameter

LN_EPSILON = 1e-3  # keras LayerNormalization default
_TRUNC_STD = 0.87962566103423978  # std of a unit normal truncated to 2 sigma (keras VarianceScaling divides by it)

LDS_BUDGET = 65536  # bytes per workgroup of the fused kernels (csrc/er_fibinet.hip)
MAX_FIELDS = 64
MAX_DIM = 64


def _he_normal(shape, rng):
  return truncated_normal(shape, rng, 0.0, math.sqrt(2.0 / shape[0]) / _TRUNC_STD)


def _glorot_normal(shape, rng):
  return truncated_normal(shape, rng, 0.0, math.sqrt(2.0 / (shape[0] + shape[1])) / _TRUNC_STD)


# ------------------------------------------------------------------------------------------------ the kernels' envelope
def bilinear_lds_bytes(fields, dim):
  """er_bilinear_lds_bytes: the `each` parameters at an odd row pitch, the pair table, one example's x, u and du."""
  if fields < 2 or dim < 1:
    return 0
  return 4 * ((fields - 1) * (dim * (dim | 1) + dim) + fields * (fields - 1) // 2 + fields * dim +
              2 * (fields - 1) * dim)


def bilinear_fits(fields, dim):
  return 2 <= fields <= MAX_FIELDS and 1 <= dim <= MAX_DIM and bilinear_lds_bytes(fields, dim) <= LDS_BUDGET


def senet_reduction(fields, groups, ratio):
  return max(1, fields * groups * 2 // ratio)


def senet_lds_bytes(fields, dim, groups, reduction):
  """er_senet_lds_bytes: theta (with the layer norm's gamma and beta) and one example's backward state."""
  if fields < 1 or dim < 1 or groups < 1 or reduction < 1 or groups > dim:
    return 0
  z, fd = 2 * fields * groups, fields * dim
  return 4 * (z * reduction + reduction + reduction * fd + fd + 2 * fd + 4 * fd + 2 * z + 2 * reduction + 2)


def senet_fits(fields, dim, groups, reduction):
  return (1 <= fields <= MAX_FIELDS and 1 <= dim <= MAX_DIM and groups >= 1 and dim % groups == 0 and
          1 <= reduction <= 2 * fields * groups and senet_lds_bytes(fields, dim, groups, reduction) <= LDS_BUDGET)


def _reject_bf16(what):
  if getattr(context.current(), 'dense_dtype', 'f32') == 'bf16':
    raise ValueError('%s: dense_dtype bf16 is not supported (the field kernels are fp32)' % what)


def _field_block(inputs):
  """(x [B, F * D], F, D) when the fields have one width; the list's own concat block when it has one (no copy)."""
  inputs = list(inputs) if not hasattr(inputs, 'uniform_block') else inputs
  dims = {int(e.shape[-1]) for e in inputs}
  if len(dims) != 1:
    return None
  F, D = len(inputs), dims.pop()
  blk = inputs.uniform_block() if hasattr(inputs, 'uniform_block') else None
  if blk is not None:
    base, col0, _, _ = blk
    return (base if (col0 == 0 and base.shape[1] == F * D) else base[:, col0:col0 + F * D]), F, D
  return torch.cat(list(inputs), dim=-1), F, D


def _fused(x):
  return x.is_cuda and x.dtype == torch.float32 and isinstance(kernels.hip(), kernels.HipBackend)


def _grads_of(params):
  # (the variables' slices of the flat gradient buffer; None in the build pass, before VarStore.pack)
  return [p.grad for p in params] if all(p.grad is not None for p in params) else None


# ------------------------------------------------------------------------------------------------ the torch compositions
def senet_compose(inputs, groups, w1, b1, w2, b2, skip, gamma=None, beta=None):
  """SENet.call op by op over a list of [B, D_f] fields (any widths); gamma / beta: the output layer norm's."""
  squeezed = []
  for emb in inputs:
    grouped = emb.reshape(emb.shape[0], groups, -1)
    squeezed.append(grouped.max(dim=-1).values)
    squeezed.append(grouped.mean(dim=-1))
  z = torch.cat(squeezed, dim=1)  # [B, fields * groups * 2]
  a1 = torch.relu(z @ w1 + b1)
  weights = a1 @ w2 + b2
  x = torch.cat(list(inputs), dim=-1)
  out = x * weights
  if skip:
    out = out + x
  if gamma is not None:
    mean = out.mean(dim=-1, keepdim=True)
    var = ((out - mean) ** 2).mean(dim=-1, keepdim=True)
    out = (out - mean) * torch.rsqrt(var + LN_EPSILON) * gamma + beta
  return out


def bilinear_compose(x, F, D, ws, bs, plus):
  """BiLinear.call up to the concatenation for types `all` (one kernel) and `each` (F - 1): x [B, F * D]."""
  B = x.shape[0]
  xf = x.reshape(B, F, D)
  if len(ws) == 1:
    u = xf[:, :-1] @ ws[0] + bs[0]
  else:
    u = torch.einsum('bik,ikc->bic', xf[:, :-1], torch.stack(list(ws))) + torch.stack(list(bs))
  pairs = list(itertools.combinations(range(F), 2))
  i = torch.tensor([p[0] for p in pairs], device=x.device)
  j = torch.tensor([p[1] for p in pairs], device=x.device)
  p = u[:, i] * xf[:, j]  # [B, pairs, D]
  return p.sum(dim=-1) if plus else p.reshape(B, -1)


# ------------------------------------------------------------------------------------------------ the blocks
class SENet(object):

  def __init__(self, params, name='SENet', reuse=None, **kwargs):
    self.name = name
    self.config = params.get_pb_config()
    self.fused = False  # (FiBiNet switches its own SENet to the fused kernels; see the module docstring)

  def _call_fused(self, x, F, D, g, reduction):
    vs = context.varstore()
    cfg = self.config
    names = [('W1/kernel', (2 * F * g, reduction), _he_normal), ('W1/bias', (reduction,), 'zeros'),
             ('W2/kernel', (reduction, F * D), _glorot_normal), ('W2/bias', (F * D,), 'zeros')]
    if cfg.use_output_layer_norm:
      names += [('output_ln/gamma', (F * D,), 'ones'), ('output_ln/beta', (F * D,), 'zeros')]
    params = [vs.get_variable('%s/%s' % (self.name, n), shape, init) for n, shape, init in names]
    return kernels.SENetFn.apply(x, F, D, g, reduction, bool(cfg.use_skip_connection), bool(cfg.use_output_layer_norm),
                                 _grads_of(params), *params)

  def __call__(self, inputs, **kwargs):
    g = int(self.config.num_squeeze_group)
    for emb in inputs:
      assert emb.dim() == 2, 'field embeddings must be rank 2 tensors'
      d = int(emb.shape[-1])
      assert d >= g and d % g == 0, 'field embedding dimension %d must be divisible by %d' % (d, g)
    reduction = senet_reduction(len(inputs), g, int(self.config.reduction_ratio))
    if self.fused:
      blk = _field_block(inputs)
      if blk is not None and _fused(blk[0]) and senet_fits(blk[1], blk[2], g, reduction):
        return self._call_fused(blk[0], blk[1], blk[2], g, reduction)
    inputs = list(inputs)
    emb_size = sum(int(e.shape[-1]) for e in inputs)
    squeezed = []
    for emb in inputs:
      grouped = emb.reshape(emb.shape[0], g, -1)
      squeezed.append(grouped.max(dim=-1).values)
      squeezed.append(grouped.mean(dim=-1))
    z = torch.cat(squeezed, dim=1)  # [B, fields * groups * 2]
    a1 = torch.relu(dnn.dense(z, reduction, self.name + '/W1', kernel_initializer=_he_normal))
    weights = dnn.dense(a1, emb_size, self.name + '/W2', kernel_initializer=_glorot_normal)
    x = torch.cat(inputs, dim=-1)
    out = x * weights
    if self.config.use_skip_connection:
      out = out + x
    if self.config.use_output_layer_norm:
      vs = context.varstore()
      gamma = vs.get_variable(self.name + '/output_ln/gamma', (emb_size,), 'ones')
      beta = vs.get_variable(self.name + '/output_ln/beta', (emb_size,), 'zeros')
      mean = out.mean(dim=-1, keepdim=True)
      var = ((out - mean) ** 2).mean(dim=-1, keepdim=True)
      out = (out - mean) * torch.rsqrt(var + LN_EPSILON) * gamma + beta
    return out


class BiLinear(object):

  def __init__(self, params, name='bilinear', reuse=None, **kwargs):
    self.name = name
    params.check_required(['num_output_units'])
    self.use_plus = bool(params.get_or_default('use_plus', True))
    self.output_size = int(params.num_output_units)
    self.bilinear_type = str(params.get_or_default('type', 'interaction')).lower()
    if self.bilinear_type not in ['all', 'each', 'interaction']:
      raise NotImplementedError("bilinear_type only support: ['all', 'each', 'interaction']")
    if self.bilinear_type == 'interaction':
      raise NotImplementedError(
          'BiLinear(%s): type `interaction` cannot run in the reference either: its call indexes the list of '
          'F (F - 1) / 2 layers with i * field_num + j, which is out of range for every F >= 2; use `all` or `each`' % name)
    _reject_bf16('BiLinear(%s)' % name)

  def variables(self, fields, dim, vs=None):
    """kernel and bias of each dense layer, in the packed order: `all`, or each_0 .. each_{F-2}."""
    vs = vs or context.varstore()
    layers = ['all'] if self.bilinear_type == 'all' else ['each_%d' % i for i in range(fields - 1)]
    out = []
    for ly in layers:
      out.append(vs.get_variable('%s/%s/kernel' % (self.name, ly), (dim, dim), 'glorot_uniform'))
      out.append(vs.get_variable('%s/%s/bias' % (self.name, ly), (dim,), 'zeros'))
    return out

  def __call__(self, inputs, **kwargs):
    if not isinstance(inputs, (tuple, list)):
      raise TypeError('input of BiLinear layer must be a list')
    field_num = len(inputs)
    logging.info('Bilinear Layer with %d inputs' % field_num)
    for emb in inputs:
      assert emb.dim() == 2, 'field embeddings must be rank 2 tensors'
    blk = _field_block(inputs)
    if blk is None:
      raise ValueError('all embedding dimensions must be same when not use bilinear type: interaction')
    x, F, D = blk
    params = self.variables(F, D)
    each = self.bilinear_type == 'each'
    if F >= 2 and _fused(x) and bilinear_fits(F, D):
      p = kernels.BiLinearFn.apply(x, F, D, each, self.use_plus, _grads_of(params), *params)
    else:
      p = bilinear_compose(x, F, D, params[0::2], params[1::2], self.use_plus)
    return dnn.dense(p, self.output_size, self.name + '/output')


class FiBiNet(object):
  """FiBiNet++ (reference layers/keras/fibinet.py:206-251)."""

  def __init__(self, params, name='fibinet', reuse=None, **kwargs):
    self.name = name
    self._config = params.get_pb_config()
    _reject_bf16('FiBiNet(%s)' % name)
    self.senet_layer = SENet(Parameter.make_from_pb(self._config.senet), name=name + '/senet')
    self.senet_layer.fused = True
    self.bilinear_layer = None
    if self._config.HasField('bilinear'):
      self.bilinear_layer = BiLinear(Parameter.make_from_pb(self._config.bilinear), name=name + '/bilinear')
    self.final_mlp = None
    if self._config.HasField('mlp'):
      p = Parameter.make_from_pb(self._config.mlp)
      p.l2_regularizer = params.l2_regularizer
      self.final_mlp = MLP(p, name=name + '/mlp')

  def __call__(self, inputs, training=None, **kwargs):
    feature = self.senet_layer(inputs)
    if self.bilinear_layer is not None:
      feature = torch.cat([feature, self.bilinear_layer(inputs)], dim=-1)
    if self.final_mlp is not None:
      feature = self.final_mlp(feature, training=training)
    return feature
