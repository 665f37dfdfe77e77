#!/usr/bin/env python
"""Listwise ranking loss values from the REFERENCE'S OWN code - loss/listwise_loss.py (listwise_rank_loss,
listwise_distill_loss) - run in the build container where /root/reference exists, on make_loss_vectors.py's numpy (fp64)
stand-in for tf plus the few more ops these call.  tf.get_variable hands out the scale values the case names (the
reference initialises them to one and zero; other values make the scaled form visible).  Besides the values, the fixture
holds the central-difference gradient of THE REFERENCE'S forward with respect to every logit and to scale_w / scale_b,
which tests/test_listwise_loss_pins.py compares with the compositions' autograd gradient.

usage: python tests/golden/make_listwise_loss_vectors.py [/root/reference]
"""
import contextlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_loss_vectors as base  # noqa: E402

t, a = base.t, np.asarray
SCALE = {}  # 'scale_w' / 'scale_b' -> the value tf.get_variable returns


def _softmax(x):
  e = np.exp(a(x) - np.max(a(x)))
  return e / e.sum()


def make_tf():
  tf = base.make_tf()
  tf.variable_scope = lambda name: contextlib.nullcontext()
  tf.get_variable = lambda name, dtype=None, shape=None, initializer=None: t([SCALE[name]])
  tf.ones_initializer = tf.zeros_initializer = lambda: None
  tf.abs = lambda x: t(np.abs(a(x)))
  tf.squeeze = lambda x: a(x).reshape(-1)
  tf.unique = lambda x: (a(x)[np.sort(np.unique(a(x), return_index=True)[1])], None)  # first occurrences, in order
  tf.map_fn = lambda fn, xs, dtype=None: t([float(fn(x)) for x in xs])
  tf.nn.softmax = lambda x: t(_softmax(x))
  tf.nn.log_softmax = lambda x: t(a(x) - np.max(a(x)) - np.log(np.exp(a(x) - np.max(a(x))).sum()))
  tf.reduce_mean = lambda x: float(np.mean(a(x)))
  tf.clip_by_value = lambda x, lo, hi: t(np.clip(a(x), lo, hi))
  tf.log1p = lambda x: t(np.log1p(a(x, dtype=np.float64)))
  tf.log = lambda x: t(np.log(a(x)))
  return tf


def main():
  sys.modules['tensorflow'] = make_tf()
  for name in ('easy_rec', 'easy_rec.python', 'easy_rec.python.utils', 'easy_rec.python.utils.load_class'):
    sys.modules[name] = types.ModuleType(name)
  sys.modules['easy_rec.python.utils.load_class'].load_by_path = lambda path: eval(path)  # (the cases use lambdas)
  lw = base.load('easy_rec/python/loss/listwise_loss.py', 'ref_listwise_loss')

  rng = np.random.default_rng(20261127)
  B = 40
  z = rng.standard_normal(B) * 1.5
  y = np.round(rng.random(B) * 3, 2)                   # graded relevance
  pos = np.exp(rng.random(B) * 7 - 1)                  # teacher positions 0.4 .. 400: below 1 and above a clip of 64
  keys = rng.integers(0, 6, size=B).astype(np.int64) * (1 << 33) - 3
  keys[0] = keys[B - 1] = np.iinfo(np.int64).max       # one session holds the first and the last example
  keys[7] = np.iinfo(np.int64).min                     # a singleton session
  out = {'logits': z, 'labels': y, 'positions': pos, 'sessions': keys}
  # name -> (the reference's function, the labels' array, its keyword arguments, (scale_w, scale_b) under scale_logits)
  cases = {
      'rank': (lw.listwise_rank_loss, 'labels', dict(), None),
      'rank_logits_t': (lw.listwise_rank_loss, 'labels', dict(label_is_logits=True, temperature=0.5), None),
      'rank_scale_t': (lw.listwise_rank_loss, 'labels', dict(scale_logits=True, temperature=2.0), (-1.5, 0.25)),
      'rank_logits_fn_w': (lw.listwise_rank_loss, 'labels',
                           dict(label_is_logits=True, temperature=2.0, transform_fn='lambda x: x * 2.0 + 1.0', weights=0.5), None),
      'distill': (lw.listwise_distill_loss, 'positions', dict(), None),
      'distill_clip_scale_t': (lw.listwise_distill_loss, 'positions',
                               dict(label_clip_max_value=64.0, scale_logits=True, temperature=0.5), (1.25, -0.5)),
      'distill_fn': (lw.listwise_distill_loss, 'positions', dict(transform_fn='lambda x: 1.0 / x', weights=2.0), None),
      'rank_tensor_weights': (lw.listwise_rank_loss, 'labels', dict(weights=t(np.full(B, 3.0))), None),  # ignored there
  }
  for name, (fn, labels, kw, scale) in cases.items():
    def f(v, fn=fn, labels=labels, kw=kw):
      SCALE.update(scale_w=v[B], scale_b=v[B + 1])
      return float(fn(t(out[labels]), t(v[:B]), keys, **kw))
    v = np.concatenate([z, scale or (1.0, 0.0)])
    g = base.numgrad(f, v)
    out[name], out[name + '_grad'] = f(v), g[:B]
    if scale:
      out[name + '_scale'], out[name + '_scale_grad'] = np.asarray(scale), g[B:]
    print('%-22s %.9f' % (name, out[name]))
  path = os.path.join(HERE, 'listwise_loss_vectors.npz')
  np.savez(path, **out)
  print('wrote %s: %d arrays' % (path, len(out)))


if __name__ == '__main__':
  main()
