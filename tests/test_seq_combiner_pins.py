"""sequence_combiner (TextCNN, attention pooling) off the GPU: the torch compositions against the fp64 restatement
(oracle/seq_combiner_ref.py), the combined group's column order, feature list and variable names, the embedding
regulariser on the raw sequence embedding, every configuration that must raise, the model sections that did not build
before (on the stand-in backend, against the fp64 oracle), the max's tie rule, the Python envelope functions against the
header's formulas, the share of near-tie outputs in the GPU tests' inputs, and the Highway block."""
import logging
import os

import numpy as np
import pytest
import torch

from _oracle_steps import close as _close
from easyrec_amd.layers.keras import text_cnn as tc
from easyrec_amd.utils import config_util
from oracle import seq_combiner_ref as sref

logging.disable(logging.WARNING)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_TOL = 1e-5
NEAR_TIE_CAP = 0.02

# (B, L_buf, P, D, sizes, filters, act): the sample's geometry at B = 1; pad + odd D; truncate + B no multiple of the
# examples per workgroup round; a single window; the sample's at B = 4096 (8 examples per round); theta too large for
# LDS (read in place); 3 examples per round with a last round of 2
TEXT_CNN_CASES = [
    (1, 14, 14, 16, [2, 3, 4], [8, 4, 4], 'relu'),
    (13, 5, 7, 5, [2, 3], [3, 2], 'relu'),
    (301, 20, 14, 16, [2, 3, 4], [16, 8, 8], 'relu'),
    (9, 4, 4, 3, [4], [5], 'linear'),
    (4096, 14, 14, 16, [2, 3, 4], [8, 4, 4], 'relu'),
    (5, 10, 12, 64, [8], [64], 'relu'),
    (1301, 14, 14, 16, [2, 3, 4], [8, 4, 4], 'relu'),
]
POOL_CASES = [(1, 1, 1), (13, 7, 5), (301, 50, 16), (64, 256, 128)]


def case_id(c):
  return 'B%d_L%d_P%d_D%d_k%s_f%s_%s' % (c[0], c[1], c[2], c[3], '-'.join(map(str, c[4])), '-'.join(map(str, c[5])), c[6])


def random_text_cnn(case, seed=None):
  """-> (x [B, L_buf, D], kernels, biases), fp64 holding fp32-representable values."""
  B, L, P, D, sizes, filters, act = case
  g = torch.Generator().manual_seed(1000 + B + D if seed is None else seed)
  x = torch.randn(B, L, D, generator=g).double()
  ks = [(torch.randn(k, D, f, generator=g) * (1.0 / (k * D) ** 0.5)).double() for k, f in zip(sizes, filters)]
  bs = [(torch.randn(f, generator=g) * 0.1).double() for f in filters]
  return x, ks, bs


def random_pool(case, seed=None):
  """-> (x [B, L, D] with zero rows from the length on, lens int64 [B] holding 0, 1 and L, w [D])."""
  B, L, D = case
  g = torch.Generator().manual_seed(2000 + B + L if seed is None else seed)
  x = torch.randn(B, L, D, generator=g).double()
  lens = torch.randint(0, L + 1, (B,), generator=g)
  for i, v in enumerate((L, 0, 1)[:B]):
    lens[i] = v
  x = x * (torch.arange(L)[None, :] < lens[:, None]).double()[:, :, None]
  w = (torch.randn(D, generator=g) * 0.5).double()
  return x, lens, w


# ------------------------------------------------------------------------------------------------ model sections
def base_cfg(batch_size):
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(ROOT, 'configs', 'deepfm_textcnn_movielens.config'))
  cfg.data_config.batch_size = batch_size
  for fc in cfg.feature_config.features:
    if fc.hash_bucket_size > 500:
      fc.hash_bucket_size = 500
  return cfg


def _feature(cfg, name):
  return [fc for fc in cfg.feature_config.features if fc.input_names[0] == name][0]


def model_cfg(kind, batch_size=8):
  """deepfm_textcnn: configs/deepfm_textcnn_movielens.config with small tables; deepfm_attention: `title` and `genres`
  as SequenceFeatures with `attention {}`; deepfm_no_pad: pad_sequence_length 0; backbone_mlp: the `deep` group
  under a backbone's MLP and Dense blocks; backbone_textcnn[_bn]: a RankModel whose
  backbone feeds `title` kept over time to a `TextCNN` block with an mlp (without / with BatchNorm); highway: a RankModel with a `Highway` block
  over the plain columns."""
  from google.protobuf import text_format
  cfg = base_cfg(batch_size)
  mc = cfg.model_config
  if kind == 'deepfm_textcnn':
    return cfg
  if kind == 'deepfm_no_pad':
    _feature(cfg, 'title').sequence_combiner.text_cnn.pad_sequence_length = 0
    return cfg
  if kind == 'backbone_mlp':
    # a RankModel whose backbone feeds the `deep` group - plain columns and `title` through its text_cnn combiner - to
    # an MLP block and a Dense(1) block
    deep = [n for g in mc.feature_groups if g.group_name == 'deep' for n in g.feature_names]
    del mc.feature_groups[:]
    mc.ClearField('deepfm')
    mc.model_class = 'RankModel'
    text_format.Merge("""
      feature_groups { group_name: 'features' %s wide_deep: DEEP }
      backbone {
        blocks { name: 'mlp' inputs { feature_group_name: 'features' }
                 keras_layer { class_name: 'MLP' mlp { hidden_units: [32, 16] } } }
        blocks { name: 'logit' inputs { block_name: 'mlp' }
                 keras_layer { class_name: 'Dense' st_params { fields { key: 'units' value { number_value: 1 } } } } }
        concat_blocks: 'logit'
      }
      model_params { l2_regularization: 1e-4 }""" % ' '.join("feature_names: '%s'" % n for n in deep), mc)
    return cfg
  if kind == 'deepfm_attention':
    for name in ('title', 'genres'):
      fc = _feature(cfg, name)
      fc.feature_type = fc.SequenceFeature
      fc.sequence_combiner.Clear()
      fc.sequence_combiner.attention.SetInParent()
    wide = [g for g in mc.feature_groups if g.group_name == 'wide'][0]
    names = [n for n in wide.feature_names if n != 'genres']
    del wide.feature_names[:]
    wide.feature_names.extend(names)
    return cfg
  _feature(cfg, 'title').ClearField('sequence_combiner')
  del mc.feature_groups[:]
  mc.ClearField('deepfm')
  mc.model_class = 'RankModel'
  mc.embedding_regularization = 1e-4
  if kind in ('backbone_textcnn', 'backbone_textcnn_bn'):
    bn = '' if kind == 'backbone_textcnn_bn' else ' use_bn: false'
    text_format.Merge("""
      feature_groups { group_name: 'text_seq' feature_names: 'title' wide_deep: DEEP }
      backbone {
        blocks { name: 'text_seq' inputs { feature_group_name: 'text_seq' }
                 input_layer { output_seq_and_normal_feature: true } }
        blocks { name: 'textcnn' inputs { block_name: 'text_seq' }
                 keras_layer { class_name: 'TextCNN' text_cnn { filter_sizes: [2, 3, 4] num_filters: [16, 8, 8]
                               pad_sequence_length: 14 mlp { hidden_units: [32, 16]%s } } } }
      }
      model_params { l2_regularization: 1e-4 }""" % bn, mc)
    return cfg
  assert kind == 'highway', kind
  text_format.Merge("""
    feature_groups { group_name: 'general' feature_names: 'user_id' feature_names: 'movie_id' feature_names: 'age'
                     wide_deep: DEEP }
    backbone {
      blocks { name: 'highway' inputs { feature_group_name: 'general' } keras_layer { class_name: 'Highway' } }
      blocks { name: 'top_mlp' inputs { block_name: 'highway' } keras_layer { class_name: 'MLP' mlp { hidden_units: [16, 8] } } }
    }
    model_params { l2_regularization: 1e-4 }""", mc)
  return cfg


def coverage(kind):
  def check(names, cfg):
    if kind in ('deepfm_textcnn', 'deepfm_no_pad', 'backbone_mlp'):
      scope = ('input_layer' if kind == 'backbone_mlp' else 'input_layer_1') + '/title_embedding'
      want = ['%s/title_embedding_text_cnn/conv1d%s/%s' % (scope, s, v) for s in ('', '_1', '_2') for v in ('kernel', 'bias')]
      want.append(scope + '/embedding_weights')
    elif kind == 'deepfm_attention':
      want = ['input_layer_1/%s_embedding/%s' % (n, v) for n in ('title', 'genres')
              for v in ('attention/kernel', 'embedding_weights')]
    else:
      want = ['textcnn/conv1d%s/%s' % (s, v) for s in ('', '_1', '_2') for v in ('kernel', 'bias')]
      want += ['textcnn/mlp/layer_0/dense/kernel', 'input_layer/title/embedding_weights']
    assert set(want) <= set(names), sorted(set(want) - set(names))
  return check


def steps_against_the_oracle(kind, B, seed, device):
  """Two steps of tests/_oracle_steps.first_steps (its own bars).
  backbone_textcnn_bn: its Conv1D biases sit under the mlp's bias-free Dense + BatchNorm, so their gradient is zero up
  to rounding (compared all the same in the first step, against the floor first_steps gives such a tensor), and Adam
  turns that rounding noise into steps of the learning rate in directions no two arithmetics share.  Those bias
  tensors alone are left out of the second step's comparison: before its second forward pass the oracle is handed the
  values the product's first step left in them; every other variable is the oracle's own.  backbone_textcnn is the same
  section without that BatchNorm, where the biases have a gradient to check."""
  import _oracle_steps
  after_step = None
  if kind.endswith('_bn'):
    kept = {}

    def after_step(est, orc, step, batch):
      if step == 0:  # (the product has taken its first step, the oracle none yet)
        kept.update({k: v.copy() for k, v in est.state_dict().items() if '/conv1d' in k and k.endswith('/bias')})
        assert len(kept) == 3
      else:
        for k, v in kept.items():
          orc.state[k] = v.astype(orc.state[k].dtype)
  return _oracle_steps.first_steps(model_cfg(kind, B), B, seed=seed, device=device, oracle_dtype=torch.float64,
                                   coverage=coverage(kind), after_step=after_step)


# ------------------------------------------------------------------------------------------------ the reference's outputs
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'seq_combiner_vectors.npz'))
GOLD_CNN = sorted({k.split(':')[0] for k in GOLD.files if k.startswith('cnn_')})


def gold_cnn(tag):
  """-> (the layer's config, x [B, L, D], lens, {TF name: variable}, the reference's output), fp64."""
  from google.protobuf import text_format
  from easyrec_amd.protos import layer_pb2
  pb = layer_pb2.TextCNN()
  text_format.Merge(str(GOLD[tag + ':text']), pb)
  var = {k[len(tag) + 5:]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith(tag + ':var:')}
  return pb, torch.from_numpy(GOLD[tag + ':x']), torch.from_numpy(GOLD[tag + ':len']), var, torch.from_numpy(GOLD[tag + ':out'])


def gold_conv_params(pb, var, prefix='text_cnn'):
  names = ['conv1d' if i == 0 else 'conv1d_%d' % i for i in range(len(pb.filter_sizes))]
  return [var['%s/%s/kernel' % (prefix, n)] for n in names], [var['%s/%s/bias' % (prefix, n)] for n in names]


def gold_mlp(pb, var, net, prefix='text_cnn/mlp'):
  """The keras MLP after the pooling (Dense without bias -> BatchNorm on batch statistics, epsilon 1e-3 -> relu)."""
  for i in range(len(pb.mlp.hidden_units)):
    z = net @ var['%s/layer_%d/dense/kernel' % (prefix, i)]
    z = (z - z.mean(dim=0)) / torch.sqrt(z.var(dim=0, unbiased=False) + 1e-3)
    net = torch.relu(z * var['%s/layer_%d/bn/gamma' % (prefix, i)] + var['%s/layer_%d/bn/beta' % (prefix, i)])
  return net


def test_fixture_covers_the_cases():
  assert GOLD_CNN == ['cnn_exact', 'cnn_linear', 'cnn_mlp', 'cnn_one_size', 'cnn_pad', 'cnn_predict', 'cnn_truncate']
  for tag, L in (('cnn_pad', 5), ('cnn_truncate', 9), ('cnn_exact', 7)):
    pb, x, lens, _, _ = gold_cnn(tag)
    assert x.shape == (6, L, 4) and pb.pad_sequence_length == 7
  assert sorted(GOLD['input_layer:len:hist'])[:2] == [0, 1] and max(GOLD['input_layer:len:hist']) == 5
  assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'seq_combiner_vectors.npz')) < 100000


@pytest.mark.parametrize('tag', GOLD_CNN)
def test_text_cnn_composition_matches_the_reference(tag):
  pb, x, lens, var, want = gold_cnn(tag)
  ks, bs = gold_conv_params(pb, var)
  assert list(GOLD[tag + ':names']) == ['text_cnn/conv1d%s/%s' % ('' if i == 0 else '_%d' % i, v)
                                        for i in range(len(ks)) for v in ('kernel', 'bias')]
  got = tc.text_cnn_compose(x, int(pb.pad_sequence_length), ks, bs, pb.activation)
  _close(sref.text_cnn_ref(x, int(pb.pad_sequence_length), ks, bs, pb.activation), got, 1e-6, 'restatement')
  if pb.HasField('mlp'):
    got = gold_mlp(pb, var, got)
  _close(got, want, 1e-6, tag)


def test_input_layer_branches_match_the_reference():
  """The attention branch (lengths 0, 1 and the maximum) and the text_cnn branch of single_call_input_layer: the
  columns sorted by name in the concat."""
  from google.protobuf import text_format
  from easyrec_amd.protos import layer_pb2
  var = {k[len('input_layer:var:'):]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith('input_layer:var:')}
  hist, hist_len = torch.from_numpy(GOLD['input_layer:x:hist']), torch.from_numpy(GOLD['input_layer:len:hist'])
  att = tc.seq_attn_pool_compose(hist, hist_len, var['hist_embedding/attention/kernel'])
  _close(sref.seq_attn_pool_ref(hist, hist_len, var['hist_embedding/attention/kernel']), att, 1e-6, 'restatement')
  pb = layer_pb2.TextCNN()
  text_format.Merge('filter_sizes: [2, 3] num_filters: [3, 2] pad_sequence_length: 7', pb)
  ks, bs = gold_conv_params(pb, var, 'title_embedding/title_embedding_text_cnn')
  cnn = tc.text_cnn_compose(torch.from_numpy(GOLD['input_layer:x:title']), 7, ks, bs, 'relu')
  _close(torch.cat([att, cnn], dim=1), GOLD['input_layer:out'], 1e-6, 'input layer')
  assert float(att[hist_len == 0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the compositions
@pytest.mark.parametrize('case', TEXT_CNN_CASES[:4] + TEXT_CNN_CASES[5:6], ids=case_id)
def test_text_cnn_composition_matches_the_restatement(case):
  B, L, P, D, sizes, filters, act = case
  x, ks, bs = random_text_cnn(case)
  for pad in (P, 0 if L >= max(sizes) else P):
    xs = [t.clone().requires_grad_(True) for t in [x] + ks + bs]
    got = tc.text_cnn_compose(xs[0], pad, xs[1:1 + len(ks)], xs[1 + len(ks):], act)
    xr = [t.clone().requires_grad_(True) for t in [x] + ks + bs]
    exp = sref.text_cnn_ref(xr[0], pad, xr[1:1 + len(ks)], xr[1 + len(ks):], act)
    assert got.shape == (B, sum(filters))
    _close(got, exp, 1e-6, 'forward')
    d = torch.randn(got.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (got * d).sum().backward()
    (exp * d).sum().backward()
    for a, b, what in zip(xs, xr, ['dx'] + ['dkernel'] * len(ks) + ['dbias'] * len(bs)):
      _close(a.grad, b.grad, 1e-6, what)


@pytest.mark.parametrize('case', POOL_CASES[:3], ids=lambda c: 'B%d_L%d_D%d' % c)
def test_attention_composition_matches_the_restatement(case):
  x, lens, w = random_pool(case)
  xs = [x.clone().requires_grad_(True), w.reshape(-1, 1).clone().requires_grad_(True)]
  got = tc.seq_attn_pool_compose(xs[0], lens, xs[1])
  xr = [x.clone().requires_grad_(True), w.clone().requires_grad_(True)]
  exp = sref.seq_attn_pool_ref(xr[0], lens, xr[1])
  _close(got, exp, 1e-6, 'forward')
  assert float(got.detach()[lens == 0].abs().max() if bool((lens == 0).any()) else 0.0) == 0.0  # (a row of length 0 pools to 0)
  d = torch.randn(got.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
  (got * d).sum().backward()
  (exp * d).sum().backward()
  _close(xs[0].grad, xr[0].grad, 1e-6, 'dx')
  _close(xs[1].grad.reshape(-1), xr[1].grad, 1e-6, 'dw')


def test_a_tied_max_shares_the_gradient_evenly():
  """Two identical windows: torch.amax (the composition) gives each half of dy; the bias the whole."""
  D, k, F = 3, 2, 2
  x = torch.randn(1, 4, D, generator=torch.Generator().manual_seed(5)).double()
  x[0, 2:] = x[0, :2]  # windows 0 and 2 are the same; window 1 differs
  w = torch.zeros(k, D, F, dtype=torch.float64)
  w[:, :, 0] = x[0, :2]  # filter 0 = window 0 itself: its response there is |w|^2, the largest (Cauchy-Schwarz)
  w[:, :, 1] = -x[0, :2]
  b = torch.tensor([0.5, 100.0], dtype=torch.float64)
  xs = [x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)]
  y = tc.text_cnn_compose(xs[0], 4, [xs[1]], [xs[2]], 'linear')
  dy = torch.tensor([[2.0, 0.0]], dtype=torch.float64)
  (y * dy).sum().backward()
  half = 0.5 * 2.0 * w[:, :, 0]  # dy / 2 through each of the two windows
  assert torch.allclose(xs[0].grad[0, :2], half) and torch.allclose(xs[0].grad[0, 2:], half)
  assert torch.allclose(xs[2].grad, torch.tensor([2.0, 0.0], dtype=torch.float64))
  xr = [x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)]
  (sref.text_cnn_ref(xr[0], 4, [xr[1]], [xr[2]], 'linear') * dy).sum().backward()
  assert torch.allclose(xs[0].grad, xr[0].grad) and torch.allclose(xs[1].grad, xr[1].grad)


@pytest.mark.parametrize('case', TEXT_CNN_CASES, ids=case_id)
def test_near_ties_stay_under_the_cap_in_the_gpu_tests_inputs(case):
  """tests/test_seq_combiner_gpu.py compares an output whose fp64 top two window values (or maximum and 0 under relu)
  lie within PATTERN_TOL under the kernel's own selection; the seeded inputs keep those under 2 % of the outputs."""
  B, L, P, D, sizes, filters, act = case
  x, ks, bs = random_text_cnn(case)
  near = sref.near_ties(x, P, ks, bs, act, PATTERN_TOL)
  assert float(near.double().mean()) <= NEAR_TIE_CAP, float(near.double().mean())


# ------------------------------------------------------------------------------------------------ the envelope
def test_envelope_functions_agree_with_the_library(built_lib):
  from easyrec_amd import kernels
  be = kernels.HipBackend.__new__(kernels.HipBackend)
  from easyrec_amd import abi
  be.lib = abi.load_library()
  shapes = [(14, 16, [2, 3, 4], [8, 4, 4]), (14, 16, [2, 3, 4], [16, 8, 8]), (7, 5, [2, 3], [3, 2]), (4, 3, [4], [5]),
            (64, 64, [8, 8, 8, 8], [16, 16, 16, 16]), (64, 64, [8], [64]), (12, 64, [8], [64]), (64, 64, [1], [1]),
            (65, 16, [2], [4]), (14, 65, [2], [4]), (14, 16, [9], [4]), (3, 16, [4], [4]), (14, 16, [2, 3], [60, 5]),
            (14, 16, [2, 2, 2, 2, 2], [1, 1, 1, 1, 1]), (14, 16, [0], [4]), (14, 16, [2], [0]), (1, 1, [1], [1])]
  for P, D, sizes, filters in shapes:
    assert tc.text_cnn_epb(P, D, sizes, filters) == be.text_cnn_epb(P, D, sizes, filters), (P, D, sizes, filters)
    assert tc.text_cnn_fits(P, D, sizes, filters) == (be.text_cnn_epb(P, D, sizes, filters) > 0)
    if len(sizes) <= 4:
      assert tc.text_cnn_lds_bytes(P, D, sizes, filters) == be.text_cnn_lds_bytes(P, D, sizes, filters) <= 65536
  # the issue's envelope: P, D <= 64, sum F <= 64, k <= min(P, 8), up to 4 sizes
  assert all(tc.text_cnn_fits(*s) for s in shapes[:8])
  assert not any(tc.text_cnn_fits(*s) for s in shapes[8:16])
  for L, D in ((1, 1), (50, 16), (256, 128), (1024, 128), (1025, 16), (50, 129), (0, 4)):
    assert tc.seq_attn_pool_fits(L, D) == (be.seq_attn_pool_epb(L, D) > 0), (L, D)
    for bwd in (False, True):
      assert tc.seq_attn_pool_lds_bytes(L, D, bwd) == be.seq_attn_pool_lds_bytes(L, D, bwd) <= 65536
  assert tc.seq_attn_pool_fits(256, 128)


# ------------------------------------------------------------------------------------------------ the input layer
def _build(cfg, B=8, **kw):
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  return EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=1, **kw).build()


def test_combined_group_order_feature_list_and_names(ref_backend, built_lib):
  """Two plain and two sequence columns: the plain columns in group order, then the sequence columns sorted by name
  (genres before title, whatever the group lists first); tables and combiner variables under the column's scope."""
  from easyrec_amd.core import context
  from easyrec_amd.input.synthetic import SyntheticBatches
  cfg = model_cfg('deepfm_attention')
  fc = _feature(cfg, 'title')
  fc.sequence_combiner.Clear()
  fc.sequence_combiner.text_cnn.filter_sizes.extend([2, 3])
  fc.sequence_combiner.text_cnn.num_filters.extend([10, 6])  # (DeepFM's FM takes fields of one width)
  fc.sequence_combiner.text_cnn.pad_sequence_length = 6
  deep = [g for g in cfg.model_config.feature_groups if g.group_name == 'deep'][0]
  del deep.feature_names[:]
  deep.feature_names.extend(['title', 'user_id', 'genres', 'age'])
  est = _build(cfg)
  est.train_step(SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=8, seed=2).next_batch())
  with context.use(est.ctx):
    out, flist, by_name = est.model._input_layer(est.model._feature_dict, 'deep', is_dict=True)
  assert [int(f.shape[1]) for f in flist] == [16, 16, 16, 16] and out.shape == (8, 64)
  assert list(by_name) == ['user_id', 'age', 'genres', 'title']
  assert torch.equal(out[:, 32:48], by_name['genres']) and torch.equal(out[:, 48:], by_name['title'])
  # the feature LIST keeps the group's own order of the sequence columns (title before genres), as the fixture's
  # widths do (its group lists title [5 wide] before hist [4 wide]; the concat is hist, title)
  assert flist[2] is by_name['title'] and flist[3] is by_name['genres']
  assert list(GOLD['input_layer:order']) == ['hist', 'title'] and list(GOLD['input_layer:widths']) == [5, 4]
  names = list(est.state_dict())
  scope = 'input_layer_1/'
  want = [scope + 'genres_embedding/attention/kernel', scope + 'title_embedding/title_embedding_text_cnn/conv1d/kernel',
          scope + 'title_embedding/title_embedding_text_cnn/conv1d/bias',
          scope + 'title_embedding/title_embedding_text_cnn/conv1d_1/kernel',
          scope + 'title_embedding/title_embedding_text_cnn/conv1d_1/bias']
  dense = [n for n in names if 'attention' in n or 'conv1d' in n]
  assert dense == want, dense  # (creation order)
  assert dense == [scope + n.replace('hist_', 'genres_') for n in GOLD['input_layer:names']]  # (the reference's own)
  assert scope + 'genres_embedding/embedding_weights' in names and scope + 'title_embedding/embedding_weights' in names
  assert est.state_dict()[want[1]].shape == (2, 16, 10)


@pytest.mark.parametrize('kind', ['deepfm_textcnn', 'deepfm_attention', 'deepfm_no_pad', 'backbone_mlp',
                                  'backbone_textcnn', 'backbone_textcnn_bn'])
def test_model_sections_build_and_step_against_the_oracle(kind, ref_backend, built_lib):
  """Each section builds and takes two training steps on the stand-in backend (the compositions), at first_steps' bars
  against the fp64 oracle: every loss key - the regularisation loss holds the embedding regulariser on the RAW [B, L, D]
  sequence embedding and the kernel regulariser on `attention` - the logits and every variable's first moment."""
  steps_against_the_oracle(kind, 8, 4, 'cpu')


def test_what_must_raise_raises(ref_backend, built_lib):
  # a sequence column without a combiner: the reference's ValueError
  cfg = model_cfg('deepfm_textcnn')
  _feature(cfg, 'title').ClearField('sequence_combiner')
  with pytest.raises(ValueError, match='sequence_combiner is none'):
    _build(cfg)
  # multi_head_attention: NotImplementedError, as in the reference
  cfg = model_cfg('deepfm_textcnn')
  _feature(cfg, 'title').sequence_combiner.Clear()
  _feature(cfg, 'title').sequence_combiner.multi_head_attention.SetInParent()
  with pytest.raises(NotImplementedError, match='multi_head_attention'):
    _build(cfg)
  # bf16 dense
  with pytest.raises(ValueError, match='bf16'):
    _build(model_cfg('deepfm_textcnn'), dense_dtype='bf16')
  with pytest.raises(ValueError, match='bf16'):
    _build(model_cfg('backbone_textcnn'), dense_dtype='bf16')
  # variational dropout
  cfg = model_cfg('deepfm_textcnn')
  cfg.model_config.variational_dropout.SetInParent()
  with pytest.raises(NotImplementedError, match='variational dropout'):
    _build(cfg)
  # a time extent shorter than the largest filter, without padding: names the layer of the feature
  from easyrec_amd.input.synthetic import SyntheticBatches
  cfg = model_cfg('deepfm_no_pad')
  _feature(cfg, 'title').sequence_combiner.text_cnn.filter_sizes[2] = 400
  with pytest.raises(ValueError, match='title'):
    est = _build(cfg)
    est.train_step(SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=8, seed=2).next_batch())


def test_embedding_parallel_and_negative_sampler_are_refused():
  """The build-time checks of a combining group, on the check itself (no process group / sampler table is set up)."""
  import types
  from easyrec_amd.core import context
  from easyrec_amd.layers.input_layer import InputLayer
  from easyrec_amd.layers.sharded_embedding import ShardedEmbeddingEngine
  col = types.SimpleNamespace(name='t_embedding', raw_name='t', sequence_combiner=types.SimpleNamespace(
      WhichOneof=lambda _: 'attention'))
  plain = types.SimpleNamespace(raw_name='item_id')

  def group(sampler):
    return types.SimpleNamespace(config=types.SimpleNamespace(HasField=lambda f: sampler, negative_sampler=sampler),
                                 select_columns=lambda parser: ([plain], [col]))
  layer = InputLayer.__new__(InputLayer)
  layer._fc_parser = None
  ctx = types.SimpleNamespace(dense_dtype='f32')
  with context.use(ctx):
    layer._engine = object.__new__(ShardedEmbeddingEngine)
    with pytest.raises(ValueError, match='embedding-parallel'):
      layer._check_sequence_combiners(types.SimpleNamespace(extended={}), 'g', group(False), [col])
    layer._engine = object()
    with pytest.raises(ValueError, match='negative sampler'):
      layer._check_sequence_combiners(types.SimpleNamespace(extended={}), 'g', group(True), [col])
    with pytest.raises(ValueError, match='negative sampler'):
      layer._check_sequence_combiners(types.SimpleNamespace(extended={'item_id': 1}), 'g', group(False), [col])
    layer._check_sequence_combiners(types.SimpleNamespace(extended={}), 'g', group(False), [col])


def test_the_switch_reads_the_environment(monkeypatch):
  monkeypatch.setenv('EASYREC_AMD_FUSED_SEQ_COMBINE', '0')
  assert not tc.fused_enabled()
  monkeypatch.delenv('EASYREC_AMD_FUSED_SEQ_COMBINE')
  assert tc.fused_enabled()


# ------------------------------------------------------------------------------------------------ Highway
def test_highway_block(ref_backend, built_lib):
  """value = gate * relu(transform(value)) + (1 - gate) * value with the reference's variable names and
  init_gate_bias = -3."""
  from easyrec_amd.core import context
  from easyrec_amd.input.synthetic import SyntheticBatches
  cfg = model_cfg('highway')
  est = _build(cfg)
  st = est.state_dict()
  assert st['highway/gate_0/kernel'].shape == (48, 48) and st['highway/dense/kernel'].shape == (48, 48)
  assert np.all(st['highway/gate_0/bias'] == -3.0) and np.all(st['highway/dense/bias'] == 0.0)
  assert 'highway/input_projection/kernel' not in st
  batch = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=8, seed=2).next_batch()
  est.train_step(batch)
  assert np.isfinite(est.loss_values()['total_loss'])
  from easyrec_amd.layers.keras.blocks import Highway
  from easyrec_amd.layers.utils import Parameter
  from google.protobuf import struct_pb2
  layer = Highway(Parameter(struct_pb2.Struct(), True), name='highway')
  layer._transform_names = ['dense']  # (the built model's layer took the store's first number)
  x = torch.randn(8, 48, generator=torch.Generator().manual_seed(1))
  with context.use(est.ctx), torch.no_grad():
    got = layer(x, training=False)
  st = {k: torch.as_tensor(v) for k, v in est.state_dict().items()}
  gate = torch.sigmoid(x @ st['highway/gate_0/kernel'] + st['highway/gate_0/bias'])
  exp = gate * torch.relu(x @ st['highway/dense/kernel'] + st['highway/dense/bias']) + (1 - gate) * x
  _close(got, exp, 1e-5, 'highway')
