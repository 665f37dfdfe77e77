"""MaskNet's blocks (reference easy_rec/python/layers/keras/mask_net.py): `MaskBlock` (:15-107) and `MaskNet` (:110-166).

  MaskBlock  (net, mask_input) or one tensor for both.  [input_ln(net)] ; [project(mask_input)] -> aggregation (relu,
             he_uniform) -> weights (bias, width of net) ; net * weights ; without output_size that is the result, with
             it output (no bias) -> output_ln -> relu.  aggregation_size = int(mask_input_dim * reduction_factor) when
             reduction_factor is set, else aggregation_size.
  MaskNet    [input_ln] ; use_parallel: every block on (x, x), concatenated ; serial: net = block_i((net, x)) ; [mlp].
             Only aggregation, project and the MLP carry the block's L2 regulariser (:52-65, :123).

Variables: <name>/block_<i>/{aggregation,weights,project,output}/{kernel,bias}, <name>/block_<i>/{input_ln,output_ln}/
{gamma,beta}, <name>/input_ln/{gamma,beta}, <name>/mlp/..; a stand-alone MaskBlock under `repeat`: <block>_<i>/...

Which path runs is decided by what the code can see.  On the HIP backend, with fp32 tensors on the GPU and widths inside
the kernels' envelopes (mask_mul_fits / ln_relu_fits below, include/easyrec_hip.h K8i), the mask multiply and the
LayerNormalization + ReLU are one launch each way (kernels.MaskMulFn / LnReluFn, csrc/er_masknet.hip): in the parallel
form with one output_size ONE launch of each for all blocks, the second writing the concatenation; otherwise one per
block (blocks of unequal output_size still fill one concatenation buffer).  Both input_ln go through
kernels.AddLayerNormFn.  Anywhere else - a stand-in backend on the CPU, a width outside the envelope,
EASYREC_AMD_FUSED_MASKNET=0 - the same function is composed of torch ops between the same dense layers.

The reference tests `HasField('aggregation_size') is not None`, which is always true, and would build a Dense of 0 units
when neither size is set; here that raises ValueError.  fp32 only: with --dense_dtype bf16 the blocks raise ValueError at
build time.
"""
import logging
import os

import torch

from easyrec_amd import kernels
from easyrec_amd.core import context
from easyrec_amd.layers import dnn
from easyrec_amd.layers.keras.blocks import MLP
from easyrec_amd.layers.keras.fibinet import _fused, _grads_of, _reject_bf16
from easyrec_amd.layers.utils import Parameter

LN_EPSILON = 1e-3  # keras LayerNormalization default (reference layers/keras/layer_norm.py:173)
FUSED_DEFAULT = '1'  # EASYREC_AMD_FUSED_MASKNET when the environment does not set it

MAX_WIDTH = 4096   # er_mask_mul_*: W; er_ln_relu_*: O; er_add_ln_*: W
MAX_BLOCKS = 8     # blocks per launch
MAX_THETA = 65536  # er_theta_grad_reduce: a row of partials (2 n O floats) stays below this


def fused_enabled():
  """EASYREC_AMD_FUSED_MASKNET=0: the torch composition everywhere (the A/B switch of the K8i kernels)."""
  return os.environ.get('EASYREC_AMD_FUSED_MASKNET', FUSED_DEFAULT) != '0'


def mask_mul_fits(W, n):
  return 1 <= W <= MAX_WIDTH and 1 <= n <= MAX_BLOCKS


def ln_relu_fits(O, n):
  """er_ln_relu_grid(B, O, n) > 0 for B >= 1"""
  return 1 <= O <= MAX_WIDTH and 1 <= n <= MAX_BLOCKS and 2 * n * O < MAX_THETA


# ------------------------------------------------------------------------------------------------ the torch compositions
def layer_norm_compose(x, gamma, beta):
  mean = x.mean(dim=-1, keepdim=True)
  var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
  return (x - mean) * torch.rsqrt(var + LN_EPSILON) * gamma + beta


def _layer_norm(x, name):
  """keras LayerNormalization over the last axis: variables <name>/gamma, /beta."""
  vs = context.varstore()
  W = int(x.shape[-1])
  gamma = vs.get_variable(name + '/gamma', (W,), 'ones')
  beta = vs.get_variable(name + '/beta', (W,), 'zeros')
  if fused_enabled() and x.dim() == 2 and _fused(x) and 1 <= W <= MAX_WIDTH and x.numel() > 0:
    return kernels.AddLayerNormFn.apply(x, None, gamma, beta, LN_EPSILON, _grads_of([gamma, beta]))
  return layer_norm_compose(x, gamma, beta)


def _device_path(x):
  return fused_enabled() and x.dim() == 2 and _fused(x) and x.numel() > 0


# ------------------------------------------------------------------------------------------------ the blocks
class MaskBlock(object):

  def __init__(self, params, name='mask_block', reuse=None, **kwargs):
    self.name = name
    self.config = params.get_pb_config()
    self.l2_reg = params.l2_regularizer
    self._projection_dim = params.get_or_default('projection_dim', None)
    _reject_bf16('MaskBlock(%s)' % name)
    cfg = self.config
    if not cfg.HasField('reduction_factor') and int(cfg.aggregation_size) <= 0:
      raise ValueError('Need one of reduction factor or aggregation size for MaskBlock.')
    if self._projection_dim is not None:
      logging.info('%s project dim is %d', name, self._projection_dim)

  @property
  def output_size(self):
    return int(self.config.output_size) if self.config.HasField('output_size') else None

  def _aggregation_size(self, mask_input_dim):
    if self.config.HasField('reduction_factor'):
      size = int(mask_input_dim * self.config.reduction_factor)
    else:
      size = int(self.config.aggregation_size)
    if size <= 0:
      raise ValueError('MaskBlock(%s): aggregation size %d (mask input width %d)' % (self.name, size, mask_input_dim))
    return size

  def mask_weights(self, net, mask_input, training=None):
    """-> (net [after the block's input_ln], the instance-guided mask `weights` [B, width of net])"""
    if self.config.input_layer_norm:
      net = _layer_norm(net, self.name + '/input_ln')
    u = mask_input
    if self._projection_dim is not None:
      u = dnn.dense(u, int(self._projection_dim), self.name + '/project', l2_reg=self.l2_reg, use_bias=False)
    aggr = dnn.dense_bn_act(u, self._aggregation_size(int(mask_input.shape[-1])), self.name + '/aggregation', self.l2_reg,
                            True, False, True, training, kernel_initializer='he_uniform')
    return net, dnn.dense(aggr, int(net.shape[-1]), self.name + '/weights')

  def hidden(self, masked):
    return dnn.dense(masked, self.output_size, self.name + '/output', use_bias=False)

  def output_ln_variables(self):
    vs = context.varstore()
    O = self.output_size
    return [vs.get_variable(self.name + '/output_ln/gamma', (O,), 'ones'),
            vs.get_variable(self.name + '/output_ln/beta', (O,), 'zeros')]

  def finish(self, masked, out=None, col0=0):
    """The block from the masked net on; out, col0: a concatenation buffer to fill in place (device path only)."""
    if self.output_size is None:
      return masked
    h = self.hidden(masked)
    gb = self.output_ln_variables()
    if _device_path(h) and ln_relu_fits(self.output_size, 1):
      return kernels.LnReluFn.apply(LN_EPSILON, _grads_of(gb), out, col0, h, *gb)
    return torch.relu(layer_norm_compose(h, *gb))

  def __call__(self, inputs, training=None, **kwargs):
    if type(inputs) in (tuple, list):
      assert len(inputs) >= 2, 'MaskBlock must has at least two inputs'
      net, mask_input = inputs[:2]
    else:
      net, mask_input = inputs, inputs
    net, weights = self.mask_weights(net, mask_input, training)
    if _device_path(net) and mask_mul_fits(int(net.shape[-1]), 1):
      masked, = kernels.MaskMulFn.apply(net, weights)
    else:
      masked = net * weights
    return self.finish(masked)


class MaskNet(object):
  """MaskNet: Introducing Feature-Wise Multiplication to CTR Ranking Models by Instance-Guided Mask
  (https://arxiv.org/pdf/2102.07619.pdf)."""

  def __init__(self, params, name='mask_net', reuse=None, **kwargs):
    self.name = name
    self.config = params.get_pb_config()
    _reject_bf16('MaskNet(%s)' % name)
    self.mlp = None
    if self.config.HasField('mlp'):
      p = Parameter.make_from_pb(self.config.mlp)
      p.l2_regularizer = params.l2_regularizer
      self.mlp = MLP(p, name=name + '/mlp')
    self.mask_layers = []
    for i, block_conf in enumerate(self.config.mask_blocks):
      p = Parameter.make_from_pb(block_conf)
      p.l2_regularizer = params.l2_regularizer
      self.mask_layers.append(MaskBlock(p, name='%s/block_%d' % (name, i)))

  def _parallel(self, x, training):
    blocks = self.mask_layers
    n, W = len(blocks), int(x.shape[-1])
    if not (n >= 1 and _device_path(x) and mask_mul_fits(W, 1)):
      return torch.cat([blk((x, x), training=training) for blk in blocks], dim=1)
    pairs = [blk.mask_weights(x, x, training) for blk in blocks]
    sizes = [blk.output_size for blk in blocks]
    shared_net = all(p[0] is x for p in pairs)  # (no block-level input_ln: one input for every multiply)
    if shared_net and n > 1 and mask_mul_fits(W, n):
      masked = list(kernels.MaskMulFn.apply(x, *[p[1] for p in pairs]))
    else:
      masked = [kernels.MaskMulFn.apply(net, v)[0] for net, v in pairs]
    if n > 1 and sizes[0] is not None and len(set(sizes)) == 1 and ln_relu_fits(sizes[0], n):
      # one output width: ONE LayerNorm + ReLU launch, its output the concatenation
      hs = [blk.hidden(m) for blk, m in zip(blocks, masked)]
      gb = [v for blk in blocks for v in blk.output_ln_variables()]
      return kernels.LnReluFn.apply(LN_EPSILON, _grads_of(gb), None, 0, *(hs + gb))
    if n > 1 and all(s is not None and ln_relu_fits(s, 1) for s in sizes):
      # unequal widths: a launch per block, each writing its columns of the one concatenation buffer
      out = torch.empty(x.shape[0], sum(sizes), dtype=x.dtype, device=x.device)
      col0 = 0
      for blk, m in zip(blocks, masked):
        out = blk.finish(m, out, col0)
        col0 += blk.output_size
      return out
    outs = [blk.finish(m) for blk, m in zip(blocks, masked)]
    return outs[0] if n == 1 else torch.cat(outs, dim=1)

  def __call__(self, inputs, training=None, **kwargs):
    if self.config.input_layer_norm:
      inputs = _layer_norm(inputs, self.name + '/input_ln')
    if self.config.use_parallel:
      net = self._parallel(inputs, training)
    else:
      net = inputs
      for blk in self.mask_layers:
        net = blk((net, inputs), training=training)
    if self.mlp is not None:
      net = self.mlp(net, training=training)
    return net
