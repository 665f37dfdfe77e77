"""ORACLE - TEST INFRASTRUCTURE ONLY.  Never imported by easyrec_amd/.

A torch restatement of FiBiNet's blocks (reference layers/keras/fibinet.py: SENet :63-93, BiLinear :175-203,
FiBiNet.call :235-251) and of the input-layer block's batch norm (layers/common_layers.py:142-191), written op by op
like the reference graph: the kernels' and the model's yardstick.  Any dtype / device.

  senet(fields, groups, params, name, skip, ln, relu_mask=None, max_weight=None) -> [B, sum of dims]
  bilinear_pairs(fields, kind, plus, params, name) -> the concatenated pair terms (before the `output` Dense)
  bilinear(fields, kind, plus, params, name) -> [B, num_output_units]
  fibinet(fields, pb, params, name) -> the block's output (MLP in training mode)
  input_batch_norm(fields, params) -> the per-feature normalised list
with fields a list of [B, D_f] tensors and params the dict {name: tensor} of the reference's variable names.

relu_mask [B, R] / max_weight [B, sum of dims]: the excitation's ReLU pattern and the squeeze's arg-max choice GIVEN
(a1 = pre * mask; max = sum of x * weight over the group, weight = 1 / ties on the maximal columns, 0 elsewhere): a
gradient check through another computation's pattern where the two differ only within rounding.  Without them the
max is torch.amax, whose gradient is TensorFlow reduce_max's: split evenly among the tied maxima."""
import itertools

import torch

LN_EPS = 1e-3
BN_EPS = 1e-3


def squeeze(fields, groups, max_weight=None):
  out, col = [], 0
  for emb in fields:
    B, d = emb.shape
    grouped = emb.reshape(B, groups, d // groups)
    if max_weight is None:
      out.append(grouped.amax(dim=-1))
    else:
      out.append((grouped * max_weight[:, col:col + d].reshape(B, groups, d // groups)).sum(dim=-1))
    out.append(grouped.mean(dim=-1))
    col += d
  return torch.cat(out, dim=1)


def max_weight_of(x, fields, dim, groups):
  """The arg-max choice of x [B, F * D] as squeeze() takes it: 1 / ties on each group's maximal columns."""
  B = x.shape[0]
  g = x.reshape(B, fields * groups, dim // groups)
  is_max = (g == g.amax(dim=-1, keepdim=True)).to(x.dtype)
  return (is_max / is_max.sum(dim=-1, keepdim=True)).reshape(B, fields * dim)


def senet_pre(fields, groups, params, name, max_weight=None):
  """The excitation's hidden layer before its ReLU [B, R]."""
  return squeeze(fields, groups, max_weight) @ params[name + '/W1/kernel'] + params[name + '/W1/bias']


def senet(fields, groups, params, name, skip=True, ln=True, relu_mask=None, max_weight=None):
  pre = senet_pre(fields, groups, params, name, max_weight)
  a1 = torch.relu(pre) if relu_mask is None else pre * relu_mask
  weights = a1 @ params[name + '/W2/kernel'] + params[name + '/W2/bias']
  x = torch.cat(list(fields), dim=-1)
  out = x * weights
  if skip:
    out = out + x
  if ln:
    mean = out.mean(dim=-1, keepdim=True)
    var = ((out - mean) ** 2).mean(dim=-1, keepdim=True)
    out = (out - mean) / torch.sqrt(var + LN_EPS) * params[name + '/output_ln/gamma'] + params[name + '/output_ln/beta']
  return out


def bilinear_layers(kind, fields):
  return ['all'] if kind == 'all' else ['each_%d' % i for i in range(fields - 1)]


def bilinear_pairs(fields, kind, plus, params, name):
  F = len(fields)
  lys = bilinear_layers(kind, F)
  v_dot = []
  for i, v in enumerate(fields[:-1]):
    ly = lys[0] if kind == 'all' else lys[i]
    v_dot.append(v @ params['%s/%s/kernel' % (name, ly)] + params['%s/%s/bias' % (name, ly)])
  p = []
  for i, j in itertools.combinations(range(F), 2):
    p.append((v_dot[i] * fields[j]).sum(dim=-1, keepdim=True) if plus else v_dot[i] * fields[j])
  return torch.cat(p, dim=-1)


def bilinear(fields, kind, plus, params, name):
  return bilinear_pairs(fields, kind, plus, params, name) @ params[name + '/output/kernel'] + params[name + '/output/bias']


def batch_norm(x, params, name):
  """tf.layers.batch_normalization(training=True): batch statistics, epsilon 1e-3."""
  mean = x.mean(dim=0)
  var = ((x - mean) ** 2).mean(dim=0)
  return (x - mean) / torch.sqrt(var + BN_EPS) * params[name + '/gamma'] + params[name + '/beta']


def keras_mlp(x, units, params, name):
  """layers/keras/blocks.py MLP with its defaults: Dense without bias -> BatchNormalization -> relu, every layer."""
  for i in range(len(units)):
    x = x @ params['%s/layer_%d/dense/kernel' % (name, i)]
    x = torch.relu(batch_norm(x, params, '%s/layer_%d/bn' % (name, i)))
  return x


def fibinet(fields, pb, params, name='fibinet', relu_mask=None, max_weight=None):
  se = pb.senet
  feats = [senet(fields, int(se.num_squeeze_group), params, name + '/senet', se.use_skip_connection,
                 se.use_output_layer_norm, relu_mask, max_weight)]
  if pb.HasField('bilinear'):
    feats.append(bilinear(fields, pb.bilinear.type, pb.bilinear.use_plus, params, name + '/bilinear'))
  out = torch.cat(feats, dim=-1) if len(feats) > 1 else feats[0]
  if pb.HasField('mlp'):
    out = keras_mlp(out, list(pb.mlp.hidden_units), params, name + '/mlp')
  return out


def bn_name(k):
  return 'batch_normalization' if k == 0 else 'batch_normalization_%d' % k


def input_batch_norm(fields, params):
  """do_batch_norm with only_output_feature_list: feature k through batch_normalization_<k + 1> (the whole-tensor
  batch_normalization's output is unused)."""
  return [batch_norm(f, params, bn_name(k + 1)) for k, f in enumerate(fields)]


def split(x, fields, dim):
  return [x[:, i * dim:(i + 1) * dim] for i in range(fields)]


def random_senet(B, F, D, G, R, ln, seed):
  """x [B, F * D] and the SENet variables (he_normal / glorot_normal-like scales, non-trivial biases), fp64."""
  g = torch.Generator().manual_seed(seed)
  Z, FD = 2 * F * G, F * D
  rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
  p = {'s/W1/kernel': rn(Z, R) * (2.0 / Z) ** 0.5, 's/W1/bias': rn(R) * 0.1,
       's/W2/kernel': rn(R, FD) * (2.0 / (R + FD)) ** 0.5, 's/W2/bias': rn(FD) * 0.1}
  if ln:
    p['s/output_ln/gamma'] = 1.0 + 0.2 * rn(FD)
    p['s/output_ln/beta'] = 0.1 * rn(FD)
  return rn(B, FD), p


def senet_names(name, ln):
  ns = ['/W1/kernel', '/W1/bias', '/W2/kernel', '/W2/bias'] + (['/output_ln/gamma', '/output_ln/beta'] if ln else [])
  return [name + n for n in ns]


def random_bilinear(B, F, D, kind, seed):
  g = torch.Generator().manual_seed(seed)
  rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
  p = {}
  for ly in bilinear_layers(kind, F):
    p['b/%s/kernel' % ly] = rn(D, D) * (1.0 / D) ** 0.5
    p['b/%s/bias' % ly] = rn(D) * 0.1
  return rn(B, F * D), p


def bilinear_names(name, kind, fields):
  return [n for ly in bilinear_layers(kind, fields) for n in ('%s/%s/kernel' % (name, ly), '%s/%s/bias' % (name, ly))]
