#!/usr/bin/env python
"""Multi-class softmax and JRC head values from the REFERENCE'S OWN code - builders/loss_builder.py `build`
(CLASSIFICATION with num_class > 1, JRC_LOSS), loss/jrc_loss.py, and model/rank_model.py's
`_output_to_prediction_impl`, `_build_loss_impl` and `_get_outputs_impl` (prediction, loss and output key names with and
without a tower suffix) - run in the build container where /root/reference exists, on a numpy (fp64) stand-in for the
tf ops they call.  tf.losses.sparse_softmax_cross_entropy is the documented one: per example logsumexp(z) - z[label],
times the broadcast weights, summed and divided by the number of non-zero weights.  Besides the values, the fixture
holds the central-difference gradient of THE REFERENCE'S forward with respect to every logit, which
tests/test_multiclass_pins.py compares with the gradient easyrec_amd/builders/loss_builder.py seeds the backward with.

usage: python tests/golden/make_multiclass_vectors.py [/root/reference]
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def _lse(x, axis):
  m = np.max(x, axis=axis, keepdims=True)
  return m + np.log(np.sum(np.exp(x - m), axis=axis, keepdims=True))


def make_tf():
  tf = types.ModuleType('tensorflow')
  tf.__version__ = '1.15.0'
  tf.float32, tf.int32, tf.int64 = np.float64, np.int32, np.int64
  a = np.asarray

  def sparse_softmax_cross_entropy(labels, logits, weights=1.0, **kw):
    z, y = a(logits, dtype=np.float64), a(labels).astype(np.int64)
    per = _lse(z, 1)[:, 0] - z[np.arange(z.shape[0]), y]
    w = np.broadcast_to(a(weights, dtype=np.float64), per.shape)
    present = float((w != 0).sum())
    return float((per * w).sum() / present) if present > 0 else 0.0

  tf.losses = types.SimpleNamespace(sparse_softmax_cross_entropy=sparse_softmax_cross_entropy)
  tf.nn = types.SimpleNamespace(log_softmax=lambda x, axis=-1: a(x) - _lse(a(x), axis),
                                softmax=lambda x, axis=-1: np.exp(a(x) - _lse(a(x), axis)))
  tf.sigmoid = lambda x: 1.0 / (1.0 + np.exp(-a(x)))
  tf.squeeze = lambda x, axis=None: np.squeeze(a(x), axis=axis)
  tf.argmax = lambda x, axis=None: np.argmax(a(x), axis=axis)
  tf.expand_dims = lambda x, axis: np.expand_dims(a(x), axis)
  tf.concat = lambda xs, axis: np.concatenate([a(x) for x in xs], axis=axis)
  tf.shape = lambda x: a(a(x).shape)
  tf.equal = lambda p, q: a(p) == a(q)
  tf.to_float = lambda x: a(x, dtype=np.float64)
  tf.cast = lambda x, d: a(x, dtype=np.float64)
  tf.tile = lambda x, m: np.tile(a(x), [int(v) for v in m])
  tf.stack = lambda xs: a([int(v) for v in xs])
  tf.is_numeric_tensor = lambda x: isinstance(x, np.ndarray)
  tf.reduce_sum = lambda x, axis=None: np.sum(a(x), axis=axis)
  tf.reduce_mean = lambda x, axis=None: np.mean(a(x), axis=axis)
  tf.one_hot = lambda idx, depth: np.eye(int(depth), dtype=np.float64)[a(idx)]
  tf.range = lambda n: np.arange(int(n))
  tf.linalg = types.SimpleNamespace(diag_part=lambda x: np.diagonal(a(x)).copy())
  tf.summary = types.SimpleNamespace(scalar=lambda *p, **k: None)
  return tf


def load(rel, name):
  spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
  m = importlib.util.module_from_spec(spec)
  sys.modules[name] = m
  spec.loader.exec_module(m)
  return m


def numgrad(f, z, h=1e-6):
  g = np.zeros_like(z)
  flat = g.reshape(-1)
  for i in range(z.size):
    p, q = z.copy(), z.copy()
    p.reshape(-1)[i] += h
    q.reshape(-1)[i] -= h
    flat[i] = (f(p) - f(q)) / (2 * h)
  return g


def main():
  from easyrec_amd.protos import loss_pb2
  LossType = loss_pb2.LossType
  tf = make_tf()
  sys.modules['tensorflow'] = tf
  stubs = ('tensorflow.python', 'tensorflow.python.ops', 'tensorflow.python.ops.math_ops', 'easy_rec', 'easy_rec.python',
           'easy_rec.python.loss', 'easy_rec.python.builders', 'easy_rec.python.model', 'easy_rec.python.protos',
           'easy_rec.python.loss.focal_loss', 'easy_rec.python.loss.f1_reweight_loss', 'easy_rec.python.loss.listwise_loss',
           'easy_rec.python.loss.pairwise_loss', 'easy_rec.python.loss.zero_inflated_lognormal',
           'easy_rec.python.model.easy_rec_model', 'easy_rec.python.protos.loss_pb2')
  for name in stubs:
    sys.modules[name] = types.ModuleType(name)
  sys.modules['tensorflow.python.ops'].math_ops = sys.modules['tensorflow.python.ops.math_ops']
  sys.modules['tensorflow.python.ops.math_ops'].reduce_max = lambda x, axis=None: np.max(np.asarray(x), axis=axis)
  sys.modules['easy_rec.python.protos.loss_pb2'].LossType = LossType
  sys.modules['easy_rec.python.model.easy_rec_model'].EasyRecModel = object
  for mod, names in (('focal_loss', ['sigmoid_focal_loss_with_logits']), ('f1_reweight_loss', ['f1_reweight_sigmoid_cross_entropy']),
                     ('listwise_loss', ['listwise_distill_loss', 'listwise_rank_loss']),
                     ('pairwise_loss', ['pairwise_focal_loss', 'pairwise_hinge_loss', 'pairwise_logistic_loss', 'pairwise_loss']),
                     ('zero_inflated_lognormal', ['zero_inflated_lognormal_loss', 'zero_inflated_lognormal_pred'])):
    for n in names:
      setattr(sys.modules['easy_rec.python.loss.' + mod], n, None)
  load('easy_rec/python/loss/jrc_loss.py', 'easy_rec.python.loss.jrc_loss')
  lb = load('easy_rec/python/builders/loss_builder.py', 'easy_rec.python.builders.loss_builder')
  sys.modules['easy_rec.python.builders'].loss_builder = lb
  rm = load('easy_rec/python/model/rank_model.py', 'easy_rec.python.model.rank_model')

  rng = np.random.default_rng(20241021)
  B = 24
  w = np.round(rng.random(B) * 2, 1) + 0.1
  w[rng.random(B) < 0.2] = 0.0
  out = {'weights': w}
  # -- loss_builder.build, CLASSIFICATION with num_class 3 and 5
  for C in (3, 5):
    z = rng.standard_normal((B, C)) * 1.5
    y = rng.integers(0, C, size=B).astype(np.int64)
    out['smc_c%d_logits' % C], out['smc_c%d_labels' % C] = z, y
    for tag, weights in (('', 1.0), ('_w', w)):
      fn = lambda zz: lb.build(LossType.CLASSIFICATION, y, zz, loss_weight=weights, num_class=C)  # noqa: E731
      out['smc_c%d%s_loss' % (C, tag)], out['smc_c%d%s_grad' % (C, tag)] = fn(z), numgrad(fn, z)
  # -- jrc_loss through loss_builder.build: weights x alpha x same_label_loss, and a python-scalar weight
  z = rng.standard_normal((B, 2)) * 1.5
  y = (rng.random(B) < 0.4).astype(np.int64)
  keys = rng.integers(0, 7, size=B).astype(np.int64)
  keys[0] = keys[B - 1] = 100  # one session holds the first and the last example
  out['jrc_logits'], out['jrc_labels'], out['jrc_sessions'] = z, y, keys
  for wtag, weights in (('', 1.0), ('_w', w), ('_s2', 2.0)):
    for alpha in (0.5, 0.3):
      for same in (True, False):
        param = loss_pb2.JRCLoss(session_name='user_id', alpha=alpha, same_label_loss=same)
        fn = lambda zz: float(lb.build(LossType.JRC_LOSS, y, zz, loss_weight=weights, num_class=2, loss_param=param,  # noqa: E731
                                       session_ids=keys))
        tag = 'jrc%s_a%d_%s' % (wtag, round(alpha * 10), 'same' if same else 'diff')
        out[tag + '_loss'], out[tag + '_grad'] = fn(z), numgrad(fn, z)
  # -- RankModel: prediction values and key names, loss names, output names
  z5 = out['multiclass_logits'] = out['smc_c5_logits'].copy()
  z5[3, 1] = z5[3, 4] = z5[3].max() + 0.5  # a tie at the maximum: tf.argmax takes the first
  for suffix in ('', '_cvr'):
    me = types.SimpleNamespace(_prediction_dict={}, _labels={'lbl': out['smc_c5_labels'], 'clk': y},
                               _feature_dict={'user_id': keys})
    pred = rm.RankModel._output_to_prediction_impl(me, z5, LossType.CLASSIFICATION, num_class=5, suffix=suffix)
    out['names_multiclass_pred%s' % suffix] = np.array(list(pred))
    for k, v in pred.items():
      out['multiclass%s/%s' % (suffix, k)] = np.asarray(v)
    me._prediction_dict.update(pred)
    for given in ('', 'my_loss'):
      ld = rm.RankModel._build_loss_impl(me, LossType.CLASSIFICATION, 'lbl', 1.0, 5, suffix, given)
      out['names_multiclass_loss%s_%s' % (suffix, given or 'default')] = np.array(list(ld))
    out['names_multiclass_outputs%s' % suffix] = np.array(rm.RankModel._get_outputs_impl(me, LossType.CLASSIFICATION, 5, suffix))
    pred = rm.RankModel._output_to_prediction_impl(me, z, LossType.JRC_LOSS, num_class=2, suffix=suffix)
    out['names_jrc_pred%s' % suffix] = np.array(list(pred))
    for k, v in pred.items():
      out['jrc%s/%s' % (suffix, k)] = np.asarray(v)
    me._prediction_dict = dict(pred)
    param = loss_pb2.JRCLoss(session_name='user_id', alpha=0.5)
    for given in ('', 'my_loss'):
      ld = rm.RankModel._build_loss_impl(me, LossType.JRC_LOSS, 'clk', 1.0, 2, suffix, given, param)
      out['names_jrc_loss%s_%s' % (suffix, given or 'default')] = np.array(list(ld))
      out['jrc_model_loss%s' % suffix] = float(list(ld.values())[0])
    out['names_jrc_outputs%s' % suffix] = np.array(rm.RankModel._get_outputs_impl(me, LossType.JRC_LOSS, 2, suffix))
  path = os.path.join(HERE, 'multiclass_vectors.npz')
  np.savez(path, **out)
  print('wrote %s: %d arrays; softmax ce %.6f / %.6f, jrc %.6f / %.6f' % (
      path, len(out), out['smc_c3_loss'], out['smc_c5_w_loss'], out['jrc_a5_same_loss'], out['jrc_w_a3_diff_loss']))
  for k in sorted(out):
    if k.startswith('names_'):
      print(' ', k, list(out[k]))


if __name__ == '__main__':
  main()
