"""Keras-style `MLP` block (reference easy_rec/python/layers/keras/blocks.py:22-128) and `Highway` (:131-177).

Differs from the legacy `DNN` (layers/dnn.py): no bias by default, `he_uniform` kernels, BatchNorm +
activation also on the LAST layer unless `use_final_bn` / `final_activation` say otherwise
(SURVEY.md App. B.10).  Variables: `<name>/layer_<i>/dense/kernel[, bias]`, `<name>/layer_<i>/bn/*`.
Per layer: one MFMA GEMM (er_gemm) + one fused bias/BatchNorm/ReLU kernel pair (er_bn_act).

`Highway`: value = gate * act(transform(value)) + (1 - gate) * value per layer, composed of the dense layers below and
torch elementwise ops (no kernel of its own).  Variables: `<name>/input_projection/*` when emb_size differs from the
input width, `<name>/gate_<i>/*` (bias initialised to init_gate_bias) and the unnamed transform layers, which Keras
numbers per graph in creation order (`<name>/dense`, `<name>/dense_1`, ...; here VarStore.next_layer_names, taken at
the first call, where Keras' build() constructs them).
"""
import logging

import numpy as np
import torch

from easyrec_amd import kernels
from easyrec_amd.core import context
from easyrec_amd.layers import dnn
from easyrec_amd.layers.utils import Parameter
from easyrec_amd.utils.activation import get_activation, is_relu


class MLP(object):

  def __init__(self, params, name='mlp', reuse=None, **kwargs):
    self.name = name
    self.layer_name = name
    params.check_required('hidden_units')
    self.use_bn = params.get_or_default('use_bn', True)
    self.use_final_bn = params.get_or_default('use_final_bn', True)
    self.use_bias = params.get_or_default('use_bias', False)
    self.use_final_bias = params.get_or_default('use_final_bias', False)
    self.dropout_rate = list(params.get_or_default('dropout_ratio', []))
    self.activation = params.get_or_default('activation', 'relu')
    self.initializer = params.get_or_default('initializer', 'he_uniform')
    self.final_activation = params.get_or_default('final_activation', None)
    assert not params.get_or_default('use_bn_after_activation', False), \
        'use_bn_after_activation is outside the hot-path scope'
    self.units = [int(u) for u in params.hidden_units]  # (st_params hold doubles; keras Dense takes int(units))
    assert len(self.units) > 0, 'MLP(%s) takes at least one hidden units' % name
    self.l2_reg = params.l2_regularizer
    self.add_to_outputs = params.get_or_default('add_to_outputs', False)
    logging.info('MLP(%s) units: %s, activate=%s, use_bn=%r, final_bn=%r, final_activate=%s, bias=%r, '
                 'initializer=%s' % (name, self.units, self.activation, self.use_bn, self.use_final_bn,
                                     self.final_activation, self.use_bias, self.initializer))

  def _layer(self, x, i, units, use_bn, act, use_bias, drop, training):
    lname = '%s/layer_%d' % (self.name, i)
    act = None if (act is None or str(act).lower() == 'linear') else act
    fuse_relu = act is not None and is_relu(act)
    x = dnn.dense_bn_act(x, units, lname + '/dense', self.l2_reg, use_bias, use_bn, fuse_relu, training,
                         bn_name=lname + '/bn', kernel_initializer=self.initializer)
    if act is not None and not fuse_relu:
      fn = get_activation(act, training=training) if str(act).lower() == 'dice' else get_activation(act)
      if fn is not None:
        x = fn(x, name=lname + '/act')
    if 0.0 < drop < 1.0 and training:
      x = torch.nn.functional.dropout(x, p=drop, training=True)
    elif drop >= 1.0:
      raise ValueError('invalid dropout_ratio: %.3f' % drop)
    return x

  def __call__(self, x, training=None, **kwargs):
    nd = len(self.dropout_rate)
    n = len(self.units) - 1
    for i, u in enumerate(self.units[:-1]):
      x = self._layer(x, i, u, self.use_bn, self.activation, self.use_bias,
                      self.dropout_rate[i] if i < nd else 0.0, training)
    x = self._layer(x, n, self.units[-1], self.use_final_bn, self.final_activation, self.use_final_bias,
                    self.dropout_rate[n] if nd > n else 0.0, training)
    if self.add_to_outputs and 'prediction_dict' in kwargs:
      kwargs['prediction_dict'][self.layer_name] = x.squeeze(1)
    return x


class Add(object):
  """tf.keras.layers.Add, which backbone configs name directly (`class_name: 'Add'` with `merge_inputs_into_list`,
  e.g. the final logit of examples/configs/wide_and_deep_backbone_on_movielens.config): the sum of a list of tensors."""

  def __init__(self, params=None, name=None, reuse=None, **kwargs):
    self.name = name

  def __call__(self, inputs, **kwargs):
    inputs = list(inputs)
    assert len(inputs) >= 2, 'A merge layer should be called on a list of at least 2 inputs'
    out = inputs[0]
    for t in inputs[1:]:
      out = out + t
    return out


class Gate(object):
  """Weighted sum gate (reference layers/keras/blocks.py:180-209): inputs[weight_index] [B, >= len(inputs) - 1] holds
  the weights; the other inputs, in order, are scaled by its columns 0, 1, .. and summed; optional `top_mlp`
  (variables `<name>/top_mlp/..`).  Composed of torch ops (no kernel of its own)."""

  def __init__(self, params, name='gate', reuse=None, **kwargs):
    self.name = name
    self.weight_index = int(params.get_or_default('weight_index', 0))
    self.top_mlp = None
    if params.has_field('mlp'):
      mlp_cfg = params.mlp
      if not isinstance(mlp_cfg, Parameter):
        mlp_cfg = Parameter.make_from_pb(mlp_cfg)
      mlp_cfg.l2_regularizer = params.l2_regularizer
      self.top_mlp = MLP(mlp_cfg, name='%s/top_mlp' % name)

  def __call__(self, inputs, training=None, **kwargs):
    assert len(inputs) > 1, 'input of Gate layer must be a list containing at least 2 elements'
    weights = inputs[self.weight_index]
    output, j = None, 0
    for i, x in enumerate(inputs):
      if i == self.weight_index:
        continue
      term = weights[:, j, None] * x
      output = term if output is None else output + term
      j += 1
    if self.top_mlp is not None:
      output = self.top_mlp(output, training=training)
    return output


class Highway(object):

  def __init__(self, params, name='highway', reuse=None, **kwargs):
    self.name = name
    self.emb_size = params.get_or_default('emb_size', None)
    self.num_layers = int(params.get_or_default('num_layers', 1))
    self.activation = params.get_or_default('activation', 'relu')
    self.dropout_rate = float(params.get_or_default('dropout_rate', 0.0))
    self.init_gate_bias = float(params.get_or_default('init_gate_bias', -3.0))
    self._transform_names = None

  def _act(self, x, training):
    act = None if self.activation is None else str(self.activation).lower()
    if act in (None, '', 'linear'):
      return x
    if is_relu(act):
      return torch.relu(x)
    fn = get_activation(act, training=training) if act == 'dice' else get_activation(act)
    return x if fn is None else fn(x)

  def __call__(self, inputs, training=None, **kwargs):
    vs = context.varstore()
    value = inputs
    dim = int(inputs.shape[-1])
    if self.emb_size is not None and dim != int(self.emb_size):
      dim = int(self.emb_size)
      value = dnn.dense(inputs, dim, self.name + '/input_projection')
    if self._transform_names is None:  # (Keras constructs the unnamed transform layers in build(): the first call)
      self._transform_names = vs.next_layer_names('dense', self.num_layers)
    gate_bias = self.init_gate_bias
    for i in range(self.num_layers):
      gname = '%s/gate_%d' % (self.name, i)
      # (created here so that the bias starts at init_gate_bias; dnn.dense below fetches it)
      vs.get_variable(gname + '/kernel', (dim, dim), 'glorot_uniform')
      vs.get_variable(gname + '/bias', (dim,), lambda shape, rng: np.full(shape, gate_bias, dtype=np.float32))
      gate = torch.sigmoid(dnn.dense(value, dim, gname))
      transformed = self._act(dnn.dense(value, dim, '%s/%s' % (self.name, self._transform_names[i])), training)
      if self.dropout_rate > 0.0 and training:
        transformed = torch.nn.functional.dropout(transformed, p=self.dropout_rate, training=True)
      value = gate * transformed + (1.0 - gate) * value
    return value
