"""MultiHeadAttention of AutoInt (reference easy_rec/python/layers/multihead_attention.py:9-161).

Variables, as the reference's TF1 graph names them (tf.layers.dense, use_bias=False, glorot_uniform, each with the
kernel regulariser l2_reg):
  <name>/query/dnn/kernel, <name>/key/dnn/kernel, <name>/value/dnn/kernel   [d_in, head_num * head_size]
  <name>/dnn/kernel                                                          [d_in, head_num * head_size] (use_res)
The heads are contiguous column blocks of width head_size.  Scores are Q_h K_h^T / head_size ** -0.5, i.e. multiplied
by sqrt(head_size) (:67-69), with no mask; the layer returns relu(concat_h softmax(S_h) V_h + X W_res).

Per call: one packing launch and one contraction for the four projections (kernels.AutoIntProjFn), one attention launch
(kernels.AutoIntAttnFn); the backward is one attention launch, one input-gradient contraction and four weight-gradient
contractions queued with the step's other weight gradients.
"""
from easyrec_amd import kernels
from easyrec_amd.core import context

LDS_BUDGET = 65536  # bytes per workgroup of the attention kernels (csrc/er_autoint.hip)


def lds_bytes(fields, head_num, head_size):
  """The attention backward's LDS per example (er_autoint_lds_bytes): Q | K | V and dA rows at odd pitches, P and dS."""
  d = head_num * head_size
  return 4 * (fields * ((3 * d) | 1) + fields * (d | 1) + 2 * head_num * fields * fields)


def check_envelope(fields, head_num, head_size, name='multi_head_attention'):
  if fields < 1 or head_num < 1 or head_size < 1:
    raise ValueError('%s: fields %d, head_num %d and head_size %d must all be at least 1' %
                     (name, fields, head_num, head_size))
  if lds_bytes(fields, head_num, head_size) > LDS_BUDGET:
    raise ValueError('%s: %d fields x %d heads of %d are outside the attention kernels\' envelope: '
                     '4 * (F * odd(3d) + F * odd(d) + 2 * H * F^2) = %d bytes > %d' %
                     (name, fields, head_num, head_size, lds_bytes(fields, head_num, head_size), LDS_BUDGET))


def variable_names(name):
  """In the packed operand's order: query, key, value, residual."""
  return ['%s/query/dnn/kernel' % name, '%s/key/dnn/kernel' % name, '%s/value/dnn/kernel' % name, '%s/dnn/kernel' % name]


class MultiHeadAttention(object):

  def __init__(self, head_num, head_size, l2_reg, use_res=False, name=''):
    if not use_res:
      raise NotImplementedError('MultiHeadAttention: use_res=False is not implemented (AutoInt always uses the residual)')
    self._head_num = head_num
    self._head_size = head_size
    self._l2_reg = l2_reg
    self._use_res = use_res
    self._name = name

  def variables(self, d_in, vs=None):
    vs = vs or context.varstore()
    d = self._head_num * self._head_size
    return [vs.get_variable(n, (d_in, d), 'glorot_uniform', l2=self._l2_reg or 0.0) for n in variable_names(self._name)]

  def __call__(self, deep_fea):
    """deep_fea [B, F, d_in] -> [B, F, head_num * head_size]."""
    B, F, d_in = deep_fea.shape
    check_envelope(F, self._head_num, self._head_size, self._name)
    ws = self.variables(d_in)
    # (the variables' slices of the flat gradient buffer; None in the build pass, before VarStore.pack)
    grads = [w.grad for w in ws] if all(w.grad is not None for w in ws) else None
    qkvr = kernels.AutoIntProjFn.apply(deep_fea.reshape(B * F, d_in), grads, *ws)
    y = kernels.AutoIntAttnFn.apply(qkvr, F, self._head_num, self._head_size)
    return y.view(B, F, self._head_num * self._head_size)
