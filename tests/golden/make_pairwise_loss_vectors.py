#!/usr/bin/env python
"""Pairwise ranking loss values from the REFERENCE'S OWN code - loss/pairwise_loss.py (pairwise_loss with session ids,
pairwise_logistic_loss, pairwise_hinge_loss, pairwise_focal_loss) and loss/focal_loss.py - run in the build container
where /root/reference exists, on make_loss_vectors.py's numpy (fp64) stand-in for tf plus the few more ops these call.
compute_weighted_loss is the documented one: losses times the broadcast weights, summed and divided by the number of
non-zero weights (reduction NONE: the product).  Besides the values, the fixture holds the central-difference gradient of
THE REFERENCE'S forward with respect to every logit - the focal weights are a function of the logits and TensorFlow
differentiates through them - which tests/test_pairwise_loss_pins.py compares with the compositions' autograd gradient.

usage: python tests/golden/make_pairwise_loss_vectors.py [/root/reference]
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_loss_vectors as base  # noqa: E402

t, a = base.t, np.asarray


def compute_weighted_loss(losses, weights=1.0, reduction='sum_by_nonzero_weights'):
  per = a(losses, dtype=np.float64)
  w = np.broadcast_to(a(weights, dtype=np.float64), per.shape)
  if reduction == 'none':
    return t(per * w)
  present = float((w != 0).sum())
  return float((per * w).sum() / present) if present > 0 else 0.0


def make_tf():
  tf = base.make_tf()
  sce = tf.losses.sigmoid_cross_entropy
  tf.losses = types.SimpleNamespace(
      sigmoid_cross_entropy=lambda labels, logits, weights=1.0, label_smoothing=0, reduction='sum_by_nonzero_weights':
      sce(labels, logits, weights, label_smoothing) if reduction != 'none' else
      compute_weighted_loss(np.maximum(a(logits), 0) - a(logits) * a(labels) + np.log1p(np.exp(-np.abs(a(logits)))), weights, 'none'),
      Reduction=types.SimpleNamespace(NONE='none'))
  tf.nn.relu = lambda x: t(np.maximum(a(x), 0.0))
  tf.nn.top_k = lambda x, k: types.SimpleNamespace(values=t(np.sort(a(x))[::-1][:int(k)]))
  tf.math.log1p = lambda x: t(np.log1p(a(x)))
  tf.exp = lambda x: t(np.exp(a(x)))
  tf.abs = lambda x: t(np.abs(a(x)))
  tf.pow = lambda x, g: t(np.power(a(x), g))
  tf.less = lambda p, q: a(p) < a(q)
  tf.clip_by_value = lambda x, lo, hi: t(np.clip(a(x), lo, hi))
  tf.convert_to_tensor = lambda x: x
  tf.to_int32 = lambda x: int(x)
  tf.math.rint = lambda x: np.rint(x)
  tf.reduce_mean = lambda x, axis=None: float(np.mean(a(x), axis=axis))
  return tf


def main():
  sys.modules['tensorflow'] = make_tf()
  for name in ('tensorflow.python', 'tensorflow.python.ops', 'tensorflow.python.ops.losses', 'tensorflow.python.ops.losses.losses_impl',
               'easy_rec', 'easy_rec.python', 'easy_rec.python.loss', 'easy_rec.python.utils', 'easy_rec.python.utils.shape_utils'):
    sys.modules[name] = types.ModuleType(name)
  sys.modules['tensorflow.python.ops.losses.losses_impl'].compute_weighted_loss = compute_weighted_loss
  sys.modules['easy_rec.python.utils.shape_utils'].get_shape_list = lambda x, rank=None: list(a(x).shape)
  sys.modules['easy_rec.python.loss.focal_loss'] = base.load('easy_rec/python/loss/focal_loss.py', 'easy_rec.python.loss.focal_loss')
  pw = base.load('easy_rec/python/loss/pairwise_loss.py', 'ref_pairwise_loss')

  rng = np.random.default_rng(20261126)
  B = 36
  z = rng.standard_normal(B) * 1.5
  y = rng.integers(0, 4, size=B) * 0.5            # graded labels with ties
  keys = rng.integers(0, 5, size=B).astype(np.int64)
  keys[0] = keys[B - 1] = 100                     # one session holds the first and the last example
  keys[7] = 200                                   # a singleton session
  w = np.round(rng.random(B) * 2, 1) + 0.1
  w[rng.random(B) < 0.2] = 0.0
  out = {'logits': z, 'labels': y, 'sessions': keys, 'weights': w}
  # name -> (the reference's function, its keyword arguments); `sessions` / `weights` name the arrays above
  cases = {
      'pair_wise_s': (pw.pairwise_loss, dict(sessions=True)),
      'pair_wise_s_w_mt': (pw.pairwise_loss, dict(sessions=True, weights=True, margin=0.25, temperature=2.0)),
      'logistic': (pw.pairwise_logistic_loss, dict()),
      'logistic_s_w_hinge': (pw.pairwise_logistic_loss, dict(sessions=True, weights=True, hinge_margin=0.5, temperature=0.5)),
      'logistic_s_label_margin': (pw.pairwise_logistic_loss, dict(sessions=True, use_label_margin=True, temperature=2.0)),
      'logistic_ohem': (pw.pairwise_logistic_loss, dict(weights=True, ohem_ratio=0.5)),
      'hinge': (pw.pairwise_hinge_loss, dict()),
      'hinge_s_w': (pw.pairwise_hinge_loss, dict(sessions=True, weights=True, temperature=2.0)),
      'hinge_s_margin': (pw.pairwise_hinge_loss, dict(sessions=True, use_label_margin=False, margin=0.75, label_is_logits=False,
                                                      temperature=0.5)),
      'hinge_ohem': (pw.pairwise_hinge_loss, dict(sessions=True, ohem_ratio=0.3)),
      'focal': (pw.pairwise_focal_loss, dict()),
      'focal_s_w': (pw.pairwise_focal_loss, dict(sessions=True, weights=True, gamma=1.5, alpha=0.25, temperature=2.0)),
      'focal_s_hinge': (pw.pairwise_focal_loss, dict(sessions=True, hinge_margin=1.0, gamma=2.0)),
      'focal_ohem': (pw.pairwise_focal_loss, dict(weights=True, ohem_ratio=0.5, gamma=3.0)),
  }
  for name, (fn, kw) in cases.items():
    kw = dict(kw)
    sessions = keys if kw.pop('sessions', False) else None
    weights = kw.pop('weights', False)
    f = lambda zz: float(fn(t(y), t(zz), session_ids=sessions, weights=t(w) if weights else 1.0, **kw))  # noqa: E731
    out[name], out[name + '_grad'] = f(z), base.numgrad(f, z)
    print('%-26s %.9f' % (name, out[name]))
  path = os.path.join(HERE, 'pairwise_loss_vectors.npz')
  np.savez(path, **out)
  print('wrote %s: %d arrays' % (path, len(out)))


if __name__ == '__main__':
  main()
