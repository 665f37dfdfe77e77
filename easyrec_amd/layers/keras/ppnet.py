"""PEPNet's parameter-personalised MLP (reference easy_rec/python/layers/keras/ppnet.py): `GateNN` (:15-70) and `PPNet`
(:73-194).

  GateNN  Dense(hidden_dim, he_uniform, bias unless use_bn) -> [BatchNormalization] -> activation (relu) -> [Dropout,
          training only] -> Dense(output_dim, sigmoid, he_uniform, bias unless use_bn; named `weight`) -> * 2.
          output_dim = output_units, or params.output_dim when that is None; hidden_dim defaults to output_dim.  No
          regulariser on either Dense.
  PPNet   inputs (x, gate_input).  full_gate_input (default): gate_input = concat([stop_gradient(x), gate_input]), built
          ONCE from the layer's input, so every gate reads the same tensor.  The MLP is layers/keras/blocks.MLP's, layer
          by layer (its fields, defaults and the assertion on use_bn_after_activation), with a gate multiplied onto a
          layer's output:
            lazy   layer_0, gate_1, .., layer_n, gate_{n+1}
            else   gate_0 on the input, then layer_i, gate_{i+1} for all but the last layer; no gate after the last one.
          The proto's default `eager` applies when `mode` is unset (an unset string field yields its proto default).

Variables, under the layer's name: layer_<i>/dense/{kernel,bias}, layer_<i>/bn/{gamma,beta,moving_mean,moving_variance},
gate_<i>/weight/{kernel,bias}.  The first Dense and the BatchNormalization of a GateNN are unnamed in the reference, and
keras numbers unnamed layers per graph, so the reference has no stable name for them; gate_<i>/dense/{kernel,bias} and
gate_<i>/batch_normalization/{gamma,beta,moving_mean,moving_variance} are THIS PROJECT'S choice.

Which path runs is decided by what the code can see.  On the HIP backend, with fp32 tensors on the GPU, a 2-D non-empty x
and a width inside the kernel's envelope (gate_scale_fits, include/easyrec_hip.h K8j), the `weight` Dense runs without
its bias and the bias, the sigmoid, the doubling and the multiply are ONE launch each way (kernels.GateScaleFn,
csrc/er_ppnet.hip), the bias gradient going through the shared fixed-order reduce.  Anywhere else - a stand-in backend on
the CPU, a width outside the envelope, EASYREC_AMD_FUSED_PPNET=0 - the same function is composed of torch ops between
the same Dense layers: x * (2 * sigmoid(z + bias)).

Raised at build time (ValueError): a dropout rate >= 1; a mode other than lazy whose gate_params.output_dim is not the
width of x (the reference would build gate_0's `weight` of that width and fail in the multiply); --dense_dtype bf16.
"""
import os

import torch

from easyrec_amd import kernels
from easyrec_amd.core import context
from easyrec_amd.layers import dnn
from easyrec_amd.layers.keras.blocks import MLP
from easyrec_amd.layers.keras.fibinet import _fused, _grads_of, _reject_bf16
from easyrec_amd.utils.activation import get_activation, is_relu

FUSED_DEFAULT = '1'  # EASYREC_AMD_FUSED_PPNET when the environment does not set it
MAX_WIDTH = 4096     # er_gate_scale_*: W


def fused_enabled():
  """EASYREC_AMD_FUSED_PPNET=0: the torch composition everywhere (the A/B switch of the K8j kernel)."""
  return os.environ.get('EASYREC_AMD_FUSED_PPNET', FUSED_DEFAULT) != '0'


def gate_scale_fits(W):
  """er_gate_scale_grid(B, W) > 0 for B >= 1"""
  return 1 <= W <= MAX_WIDTH


def gate_scale_compose(x, z, bias):
  return x * (2 * torch.sigmoid(z if bias is None else z + bias))


class GateNN(object):

  def __init__(self, params, output_units=None, name='gate_nn', reuse=None, **kwargs):
    self.name = name
    self.output_dim = int(output_units if output_units is not None else params.output_dim)
    self.hidden_dim = int(params.get_or_default('hidden_dim', self.output_dim))
    self.initializer = params.get_or_default('initializer', 'he_uniform')
    self.use_bn = bool(params.get_or_default('use_bn', False))
    self.activation = params.get_or_default('activation', 'relu')
    self.dropout_rate = float(params.get_or_default('dropout_rate', 0.0))
    _reject_bf16('GateNN(%s)' % name)
    if self.dropout_rate >= 1.0:
      raise ValueError('invalid dropout_ratio: %.3f' % self.dropout_rate)

  def hidden(self, u, training):
    """the gate up to its `weight` layer"""
    act = None if (self.activation is None or str(self.activation).lower() == 'linear') else self.activation
    fuse_relu = act is not None and is_relu(act)
    h = dnn.dense_bn_act(u, self.hidden_dim, self.name + '/dense', None, not self.use_bn, self.use_bn, fuse_relu, training,
                         bn_name=self.name + '/batch_normalization', kernel_initializer=self.initializer)
    if act is not None and not fuse_relu:
      fn = get_activation(act, training=training) if str(act).lower() == 'dice' else get_activation(act)
      if fn is not None:
        h = fn(h, name=self.name + '/act')
    if 0.0 < self.dropout_rate and training:
      h = torch.nn.functional.dropout(h, p=self.dropout_rate, training=True)
    return h

  def weight(self, u, training):
    """-> (z, bias): the `weight` Dense before its bias, and its bias variable (None with use_bn)"""
    z = dnn.dense(self.hidden(u, training), self.output_dim, self.name + '/weight', use_bias=False,
                  kernel_initializer=self.initializer)
    bias = None
    if not self.use_bn:
      bias = context.varstore().get_variable(self.name + '/weight/bias', (self.output_dim,), 'zeros')
    return z, bias

  def scale(self, x, u, training=None):
    """x * gate(u)"""
    z, bias = self.weight(u, training)
    if fused_enabled() and x.dim() == 2 and x.numel() > 0 and _fused(x) and _fused(z) and gate_scale_fits(int(x.shape[-1])):
      return kernels.GateScaleFn.apply(None if bias is None else _grads_of([bias]), x, z, bias)
    return gate_scale_compose(x, z, bias)

  def __call__(self, u, training=None, **kwargs):
    z, bias = self.weight(u, training)
    return 2 * torch.sigmoid(z if bias is None else z + bias)


class PPNet(object):
  """PEPNet: Parameter and Embedding Personalized Network for Infusing with Personalized Prior Information."""

  def __init__(self, params, name='ppnet', reuse=None, **kwargs):
    self.name = name
    params.check_required('mlp')
    _reject_bf16('PPNet(%s)' % name)
    self.full_gate_input = bool(params.get_or_default('full_gate_input', True))
    self.lazy = params.get_or_default('mode', 'lazy') == 'lazy'
    self.gate_params = params.gate_params
    self.mlp = MLP(params.mlp, name=name)  # (layer_<i>/.. directly under this layer's name)
    units = self.mlp.units
    if any(r >= 1.0 for r in self.mlp.dropout_rate):
      raise ValueError('invalid dropout_ratio: %.3f' % max(self.mlp.dropout_rate))
    gate = lambda i, width: GateNN(self.gate_params, width, '%s/gate_%d' % (name, i))
    self.gates = {}
    if not self.lazy:
      self.gates[0] = gate(0, None)
    for i, u in enumerate(units[:-1]):
      self.gates[i + 1] = gate(i + 1, u)
    if self.lazy:
      self.gates[len(units)] = gate(len(units), units[-1])

  def gate_input(self, x, gate_input):
    """what every gate reads: built once, from the layer's input"""
    return torch.cat([x.detach(), gate_input], dim=-1) if self.full_gate_input else gate_input

  def __call__(self, inputs, training=None, **kwargs):
    x, gate_input = inputs
    gate_input = self.gate_input(x, gate_input)
    m = self.mlp
    if 0 in self.gates:
      if self.gates[0].output_dim != int(x.shape[-1]):
        raise ValueError('PPNet(%s): mode eager needs gate_params.output_dim = %d, the width of its input (got %d)' %
                         (self.name, int(x.shape[-1]), self.gates[0].output_dim))
      x = self.gates[0].scale(x, gate_input, training)
    nd, n = len(m.dropout_rate), len(m.units) - 1
    for i, u in enumerate(m.units):
      last = i == n
      x = m._layer(x, i, u, m.use_final_bn if last else m.use_bn, m.final_activation if last else m.activation,
                   m.use_final_bias if last else m.use_bias, m.dropout_rate[i] if i < nd else 0.0, training)
      if i + 1 in self.gates:
        x = self.gates[i + 1].scale(x, gate_input, training)
    return x
