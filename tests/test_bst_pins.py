"""MultiTowerBST on the CPU: the model class resolves, the layer's variable names and head split follow the reference
(model/multi_tower_bst.py), the restatement behaves as the reference's graph does, and out-of-envelope shapes raise."""
import numpy as np
import pytest
import torch

from easyrec_amd.core.variables import VarStore
from easyrec_amd.layers import bst as bst_layer
from easyrec_amd.utils import load_class
from oracle import bst_ref as ref


def test_model_class_is_registered():
  load_class.import_all_models()
  from easyrec_amd.model.easy_rec_model import _EASY_REC_MODEL_CLASS_MAP
  assert 'MultiTowerBST' in _EASY_REC_MODEL_CLASS_MAP


@pytest.mark.parametrize('E,H,widths', [(32, 4, [8, 8, 8, 8]), (20, 3, [7, 7, 6]), (9, 6, [2, 2, 2, 2, 1]),
                                        (64, 1, [64])])
def test_head_split(E, H, widths):
  assert [w for _, w in bst_layer.head_split(E, H)] == widths
  assert [s for s, _ in bst_layer.head_split(E, H)] == list(range(0, E, widths[0]))


@pytest.mark.parametrize('E,H', [(32, 4), (9, 6)])
def test_variable_names_and_order(E, H):
  vs = VarStore('cpu')
  params = bst_layer.bst_variables(vs, E, H, ln_index=0)
  names = ref.param_names(E, H)
  assert sorted(vs.names()) == sorted(names)
  assert all(p is vs._vars[n]['tensor'] for p, n in zip(params, names))  # the kernels' packed order
  # a second tower: the dense variables are shared, the LayerNorms are new
  bst_layer.bst_variables(vs, E, H, ln_index=2)
  extra = vs.names()[len(names):]
  assert sorted(extra) == sorted(['layer_normalization_2/layer_norm_scale', 'layer_normalization_2/layer_norm_bias',
                   'layer_normalization_3/layer_norm_scale', 'layer_normalization_3/layer_norm_bias'])
  assert all(vs.l2_of(n) == 0.0 for n in vs.names())
  assert np.all(vs.state_dict()['layer_normalization/layer_norm_scale'] == 1.0)


def test_restatement_masks_keys_only_and_pads_or_slices():
  B, L, T, E, H = 4, 6, 5, 9, 6
  key, hist, lens, params = ref.random_case(B, L, T, E, H, seed=1, lengths=[0, 2, 4, 6])
  out = ref.bst_block(key, hist, lens, T, H, params)
  # rows past the mask are free: changing them leaves the non-masked rows' outputs alone only through their queries
  h2 = hist.clone()
  h2[0, :] = 5.0  # example 0 has length 0: every history key is masked, but the history rows are queries
  out2 = ref.bst_block(key, h2, lens, T, H, params)
  assert torch.equal(out[1:], out2[1:])
  assert torch.equal(out[0].reshape(T, E)[T - 1], out2[0].reshape(T, E)[T - 1])  # the key row attends to itself only
  assert not torch.equal(out[0], out2[0])
  # padding the history with zero rows to T - 1 changes nothing
  longer = torch.cat([hist[:, :3], hist.new_zeros(B, 10, E)], dim=1)
  short = hist[:, :3]
  l3 = lens.clamp(max=3)
  assert torch.allclose(ref.bst_block(key, longer, l3, T, H, params), ref.bst_block(key, short, l3, T, H, params),
                        rtol=0, atol=1e-12)


@pytest.mark.parametrize('T,E,H', [(65, 32, 4), (1, 32, 4), (50, 65, 4), (50, 32, 0)])
def test_out_of_envelope_raises(T, E, H):
  with pytest.raises(ValueError):
    bst_layer.check_envelope(T, E, H)


def test_key_width_must_match_history():
  with pytest.raises(ValueError, match='key width'):
    bst_layer.bst(torch.zeros(2, 8), torch.zeros(2, 4, 16), torch.zeros(2, dtype=torch.int32), 5, 2, 0)


# ---------------------------------------------------------------------------------------- the reference's own bst()
import os  # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bst_vectors.npz'))
GOLD_CASES = sorted({k.split(':')[0] for k in GOLD.files})


def _gold(tag):
  B, L, T, E, H, towers = [int(v) for v in GOLD['%s:cfg' % tag]]
  var = {k.split(':var:')[1]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith(tag + ':var:')}
  return B, L, T, E, H, towers, torch.from_numpy(GOLD['%s:len' % tag]), var


def _lns(i):
  return ('layer_normalization' if i == 0 else 'layer_normalization_%d' % (2 * i), 'layer_normalization_%d' % (2 * i + 1))


def test_fixture_covers_the_cases():
  assert len(GOLD_CASES) == 6
  heads = {tuple(int(v) for v in GOLD['%s:cfg' % t][3:5]) for t in GOLD_CASES}
  assert {(32, 4), (20, 3), (9, 6)} <= heads
  rel = {np.sign(int(GOLD['%s:cfg' % t][1]) - (int(GOLD['%s:cfg' % t][2]) - 1)) for t in GOLD_CASES}
  assert rel == {-1, 0, 1}  # batch max below, equal to and above T - 1


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_restatement_matches_the_reference(tag):
  B, L, T, E, H, towers, lens, var = _gold(tag)
  for i in range(towers):
    got = ref.bst_block(torch.from_numpy(GOLD['%s:key%d' % (tag, i)]), torch.from_numpy(GOLD['%s:hist%d' % (tag, i)]),
                        lens, T, H, var, ln_names=_lns(i))
    want = GOLD['%s:out%d' % (tag, i)]
    assert np.abs(got.numpy() - want).max() <= 1e-9 * np.abs(want).max(), (tag, i)


@pytest.mark.parametrize('tag', GOLD_CASES)
def test_product_variable_names_are_the_reference_names(tag):
  B, L, T, E, H, towers, lens, var = _gold(tag)
  vs = VarStore('cpu')
  for i in range(towers):
    params = bst_layer.bst_variables(vs, E, H, ln_index=2 * i)
    assert [tuple(p.shape) for p in params] == [tuple(var[n].shape) for n in ref.param_names(E, H, _lns(i))]
  assert sorted(vs.names()) == sorted(var)


@pytest.mark.parametrize('tag', ['e32h4_long', 'e9h6'])
def test_stand_in_block_matches_the_reference(ref_backend, tag):
  from easyrec_amd import kernels
  B, L, T, E, H, towers, lens, var = _gold(tag)
  f32 = {n: v.float() for n, v in var.items()}
  names = ref.param_names(E, H)
  grads = [torch.zeros_like(f32[n]) for n in names]
  out = kernels.BSTBlockFn.apply(torch.from_numpy(GOLD['%s:key0' % tag]).float(),
                                 torch.from_numpy(GOLD['%s:hist0' % tag]).float(), lens.to(torch.int32), T, H, grads,
                                 *[f32[n] for n in names])
  want = GOLD['%s:out0' % tag]
  assert np.abs(out.double().numpy() - want).max() <= 2e-5 * np.abs(want).max()


def _bst_cfg(seq_len=8, towers=1, lazy=False, heads=4):
  from easyrec_amd.utils import config_util
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  cfg = config_util.get_configs_from_pipeline_file(os.path.join(root, 'configs', 'din_taobao_small.config'))
  mc = cfg.model_config
  mc.model_class = 'MultiTowerBST'
  mt = mc.multi_tower
  del mt.din_towers[:]
  groups = [mc.seq_att_groups[0].group_name]
  if towers == 2:
    g2 = mc.seq_att_groups.add()
    g2.CopyFrom(mc.seq_att_groups[0])
    g2.group_name = 'bst2'
    groups.append('bst2')
  for gname in groups:
    t = mt.bst_towers.add()
    t.input = gname
    t.seq_len = seq_len
    t.multi_head_size = heads
  if lazy:
    oc = cfg.train_config.optimizer_config[0]
    oc.lazy_adam_optimizer.learning_rate.CopyFrom(oc.adam_optimizer.learning_rate)
  return cfg


def test_model_builds_and_steps_on_the_stand_in(ref_backend, built_lib):
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  from oracle.model_oracle import OracleTrainer
  B = 16
  cfg = _bst_cfg(seq_len=8)
  est = EasyRecEstimator(cfg, device='cpu', batch_size=B, seed=4).build()
  orc = OracleTrainer(cfg, est.state_dict(), batch_size=B)
  gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=B, seed=44)
  for _ in range(2):
    b = gen.next_batch()
    est.train_step(b)
    got, exp = est.loss_values(), orc.train_step(b)
    for k in exp:
      assert abs(got[k] - exp[k]) <= 1e-4 * max(1e-3, abs(exp[k])), (k, got[k], exp[k])


def test_rejected_combinations():
  from easyrec_amd.layers.sharded_embedding import ShardedEmbeddingEngine
  from easyrec_amd.model.multi_tower_bst import MultiTowerBST
  mt = _bst_cfg().model_config.multi_tower
  MultiTowerBST.check_supported(mt, 'f32', None)
  with pytest.raises(ValueError, match='bf16'):
    MultiTowerBST.check_supported(mt, 'bf16', None)
  with pytest.raises(ValueError, match='embedding-parallel'):
    MultiTowerBST.check_supported(mt, 'f32', object.__new__(ShardedEmbeddingEngine))
  twice = _bst_cfg().model_config.multi_tower
  twice.bst_towers.add().CopyFrom(twice.bst_towers[0])
  with pytest.raises(ValueError, match='same seq_att_group'):
    MultiTowerBST.check_supported(twice, 'f32', None)
  too_long = _bst_cfg(seq_len=65).model_config.multi_tower
  with pytest.raises(ValueError, match='envelope'):
    MultiTowerBST.check_supported(too_long, 'f32', None)
  with_din = _bst_cfg().model_config.multi_tower
  with_din.din_towers.add().input = 'din'
  with pytest.raises(ValueError, match='din_towers'):
    MultiTowerBST.check_supported(with_din, 'f32', None)
