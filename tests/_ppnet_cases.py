"""PPNet and GateNN restated in plain torch, fp64, from the formulas of the reference's layers/keras/ppnet.py and keras'
Dense / BatchNormalization defaults; the fixture tests/golden/ppnet_vectors.npz; the seeded inputs of the kernel tests;
and the seeded layer cases of the GPU tests, whose ReLU pre-activations are kept away from zero.  Shared by
tests/test_ppnet_pins.py and tests/test_ppnet_gpu.py."""
import os

import numpy as np
import torch
from google.protobuf import text_format

from easyrec_amd.protos import layer_pb2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'ppnet_vectors.npz'))
GOLD_CASES = sorted({k.split(':')[0] for k in GOLD.files if k.endswith(':pb')})
BN_EPS = 1e-3
NAME = 'ppnet'

ROWS_PER_WG, GRID_CAP = 8, 1024  # er_gate_scale_grid = min(ceil(B / 8), 1024)
# (B, W) of the kernel tests: the sample's two gates; B not a multiple of the 8 rows per workgroup; widths that are no
# multiple of 4 (the 4-byte path) and width 1; a single row; more than 256 four-byte pieces per row; the envelope's edge
# (1024 sixteen-byte pieces); and a narrow case whose B is past the row count at which the grid reaches its cap, so that
# workgroups own more than the base rows (9 each, the last one fewer)
KERNEL_CASES = [(4096, 512), (4096, 256), (301, 256), (77, 128), (13, 7), (5, 1), (1, 16), (64, 1027), (3, 4096),
                (ROWS_PER_WG * GRID_CAP + 5, 8)]
# the sample's shape (samples/model_config/ppnet_on_taobao.config): x 14 fields of 16, gate_input 3 fields of 16
SAMPLE = ('mlp { hidden_units: [512, 256] } mode: "lazy" full_gate_input: true', 224, 48)
RELU_MARGIN = 1e-5  # no ReLU pre-activation of a layer case within this of zero, relative to the largest one


def gold_case(tag):
  """(message, [x, gate_input], {name: variable}, output) of a fixture case, fp64."""
  pb = layer_pb2.PPNet()
  text_format.Merge(str(GOLD['%s:pb' % tag]), pb)
  xs = [torch.from_numpy(GOLD['%s:x%d' % (tag, i)]) for i in range(2)]
  var = {k.split(':var:')[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith(tag + ':var:')}
  return pb, xs, var, torch.from_numpy(GOLD['%s:out' % tag])


# ------------------------------------------------------------------------------------------------ the restatement
def _batch_norm(x, var, p):
  mean = x.mean(dim=0, keepdim=True)
  v = ((x - mean) ** 2).mean(dim=0, keepdim=True)
  return (x - mean) / torch.sqrt(v + BN_EPS) * var[p + '/gamma'] + var[p + '/beta']


def _act(x, kind, name, pres):
  """pres: a list that collects (the layer whose output this is, the ReLU's pre-activation)"""
  if kind in (None, '', 'linear'):
    return x
  if kind == 'relu':
    if pres is not None:
      pres.append((name, x))
    return torch.relu(x)
  assert kind == 'tanh', kind
  return torch.tanh(x)


def _dense_bn_act(x, var, dense, bn, act, pres):
  x = x @ var[dense + '/kernel']
  if dense + '/bias' in var:
    x = x + var[dense + '/bias']
  if bn + '/gamma' in var:
    x = _batch_norm(x, var, bn)
  return _act(x, act, dense, pres)


def gate_nn(cfg, var, name, u, pres=None):
  """2 * sigmoid(weight(act([bn](dense(u))))); which of the biases and the BatchNormalization exist is the variables'"""
  h = _dense_bn_act(u, var, name + '/dense', name + '/batch_normalization', cfg.activation, pres)
  z = h @ var[name + '/weight/kernel']
  if name + '/weight/bias' in var:
    z = z + var[name + '/weight/bias']
  return 2 * torch.sigmoid(z)


def ppnet(cfg, var, name, x, gate_input, pres=None, through=None):
  """training mode, dropout 0.  A proto-configured MLP: activation and final_activation default to relu (an unset string
  field yields its proto default); mode likewise defaults to eager.  through: the one gate to apply (the others are
  left out), for a loss that reaches x through a gate only."""
  if cfg.full_gate_input:
    gate_input = torch.cat([x.detach(), gate_input], dim=-1)
  gate = lambda i, t: t * gate_nn(cfg.gate_params, var, '%s/gate_%d' % (name, i), gate_input, pres) \
      if through in (None, i) else t
  lazy = cfg.mode == 'lazy'
  if not lazy:
    x = gate(0, x)
  n = len(cfg.mlp.hidden_units)
  for i in range(n):
    p = '%s/layer_%d' % (name, i)
    x = _dense_bn_act(x, var, p + '/dense', p + '/bn', cfg.mlp.final_activation if i == n - 1 else cfg.mlp.activation, pres)
    if lazy or i < n - 1:
      x = gate(i + 1, x)
  return x


# ------------------------------------------------------------------------------------------------ the kernel's inputs
def kernel_inputs(B, W):
  """fp64: x, z, dout [B, W] and bias [W], on values fp32 holds exactly."""
  g = torch.Generator().manual_seed(B + W)
  rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
  f = lambda t: t.float().double()
  return f(rnd(B, W) * 1.7 + 0.3), f(rnd(B, W) * 1.7 + 0.3), f(rnd(B, W) * 1.7 + 0.3), f(0.5 * rnd(W))


def gate_scale(x, z, bias):
  return x * 2 * torch.sigmoid(z if bias is None else z + bias)


# ------------------------------------------------------------------------------------------------ the layer cases
def variable_shapes(cfg, wx, wg):
  """{name: shape} of the variables a PPNet of message cfg creates on inputs wx, wg wide."""
  shapes = {}
  wu = wx + wg if cfg.full_gate_input else wg
  gp = cfg.gate_params

  def gate(i, out):
    p = '%s/gate_%d' % (NAME, i)
    hidden = int(gp.hidden_dim) if gp.HasField('hidden_dim') else out
    shapes[p + '/dense/kernel'] = (wu, hidden)
    if gp.use_bn:
      for v in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
        shapes['%s/batch_normalization/%s' % (p, v)] = (hidden,)
    else:
      shapes[p + '/dense/bias'] = (hidden,)
      shapes[p + '/weight/bias'] = (out,)
    shapes[p + '/weight/kernel'] = (hidden, out)

  lazy = cfg.mode == 'lazy'
  if not lazy:
    gate(0, int(gp.output_dim))
  m, width = cfg.mlp, wx
  n = len(m.hidden_units)
  for i, u in enumerate(m.hidden_units):
    p = '%s/layer_%d' % (NAME, i)
    last = i == n - 1
    shapes[p + '/dense/kernel'] = (width, int(u))
    if (m.use_final_bias if last else m.use_bias):
      shapes[p + '/dense/bias'] = (int(u),)
    if (m.use_final_bn if last else m.use_bn):
      for v in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
        shapes['%s/bn/%s' % (p, v)] = (int(u),)
    if lazy or not last:
      gate(i + 1, int(u))
    width = int(u)
  return shapes


def relu_margin(pres):
  """min |pre-activation| / max |pre-activation| over every ReLU of a forward pass (inf without one)"""
  if not pres:
    return float('inf')
  return min(float(p.abs().min()) for _, p in pres) / max(float(p.abs().max()) for _, p in pres)


def _redraw(var, layer, cols, g):
  """fresh values for what shifts the columns `cols` of the pre-activation behind `layer` (a dense layer's name): its
  BatchNormalization's beta, else its bias, else those columns of its kernel"""
  bn = layer[:-len('/dense')] + ('/bn' if '/layer_' in layer else '/batch_normalization')
  for name, scale in ((bn + '/beta', 0.2), (layer + '/bias', 0.2), (layer + '/kernel', None)):
    if name in var:
      t = var[name]
      fresh = torch.randn(t.shape, generator=g, dtype=torch.float64)
      fresh = fresh * (scale if scale is not None else float(t.std()))
      t[..., cols] = fresh[..., cols].float().double()
      return
  raise AssertionError(layer)


_LAYER_CASES = {}


def layer_case(tag, B):
  """(message, x, gate_input, {name: variable}) - fp64 on values fp32 holds exactly - of a layer case: a fixture case's
  message and widths, or 'sample', at B rows, seeded.  Wherever a ReLU's pre-activation comes within 4 * RELU_MARGIN of
  zero (relative to the pass's largest), the additive parameter of that column is drawn again from the same generator,
  layer by layer, until none does: fp32 and fp64 then agree on every ReLU's pattern, and no element needs an excuse."""
  if (tag, B) in _LAYER_CASES:
    return _LAYER_CASES[tag, B]
  if tag == 'sample':
    text, wx, wg = SAMPLE
  else:
    text, wx, wg = str(GOLD['%s:pb' % tag]), GOLD['%s:x0' % tag].shape[1], GOLD['%s:x1' % tag].shape[1]
  pb = layer_pb2.PPNet()
  text_format.Merge(text, pb)
  g = torch.Generator().manual_seed(1000 * B + len(text))
  rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
  f = lambda t: t.float().double()
  x, u = f(rnd(B, wx) * 1.3 + 0.2), f(rnd(B, wg) * 1.3 + 0.2)
  var = {}
  for name, shape in variable_shapes(pb, wx, wg).items():
    if name.endswith('/kernel'):
      v = rnd(*shape) * (2.0 / shape[0]) ** 0.5
    elif name.endswith('/gamma'):
      v = 1.0 + 0.2 * rnd(*shape)
    elif name.endswith('/moving_mean'):
      v = torch.zeros(shape, dtype=torch.float64)
    elif name.endswith('/moving_variance'):
      v = torch.ones(shape, dtype=torch.float64)
    else:
      v = 0.2 * rnd(*shape)
    var[name] = f(v)
  for _ in range(200):
    pres = []
    ppnet(pb, var, NAME, x, u, pres)
    if not pres:
      break
    lim = 4 * RELU_MARGIN * max(float(p.abs().max()) for _, p in pres)
    near = [(layer, (p.abs() <= lim).any(dim=0).nonzero().flatten()) for layer, p in pres]
    near = [(layer, cols) for layer, cols in near if cols.numel()]
    if not near:
      break
    _redraw(var, near[0][0], near[0][1], g)  # (the first such layer: what follows it changes with it)
  else:
    raise AssertionError('layer_case(%s, %d) did not settle' % (tag, B))
  _LAYER_CASES[tag, B] = (pb, x, u, var)
  return _LAYER_CASES[tag, B]
