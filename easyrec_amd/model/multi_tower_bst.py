"""MultiTowerBST (reference easy_rec/python/model/multi_tower_bst.py:19-190).

Plain towers: BatchNorm on the tower input (`<tower>_fea_bn`) -> DNN, as in MultiTowerDIN.  BST towers: the key
appended to the history (sliced / zero-padded to seq_len - 1 rows), multi-head self-attention + add & LayerNorm +
feed-forward dense + add & LayerNorm, flattened to [B, seq_len * E] (layers/bst.py: two HIP launches per tower and step).
The tower outputs are concatenated (plain towers first, then the BST towers in config order) -> final_dnn -> output.

Embedding L2 (:55-60): SeqInputLayer regularises the key and the history once; the model applies the regulariser AGAIN
to the key (and to the whole history, which SeqInputLayer's history term already is here - the reference's
SeqInputLayer leaves the history to the model).  The second key term is a second lookup of the key columns into a
regularised group nobody reads: its sum of squares joins the loss and lambda * key its gradient, through the embedding
engine's own regulariser path.
"""
import logging

from easyrec_amd import kernels

from easyrec_amd.core import context
from easyrec_amd.layers import bst as bst_layer
from easyrec_amd.layers import dnn
from easyrec_amd.layers import seq_input_layer
from easyrec_amd.layers.input_layer import declare_lookup
from easyrec_amd.layers.sharded_embedding import ShardedEmbeddingEngine
from easyrec_amd.model.rank_model import RankModel
from easyrec_amd.protos.multi_tower_pb2 import MultiTower as MultiTowerConfig


class MultiTowerBST(RankModel):

  def __init__(self, model_config, feature_configs, features, labels=None, is_training=False):
    super(MultiTowerBST, self).__init__(model_config, feature_configs, features, labels, is_training)
    ctx = context.current()
    self._seq_input_layer = seq_input_layer.SeqInputLayer(
        feature_configs, model_config.seq_att_groups, embedding_regularizer=self._emb_reg,
        ev_params=self._global_ev_params, engine=ctx.engine)
    assert self._model_config.WhichOneof('model') == 'multi_tower', \
        'invalid model config: %s' % self._model_config.WhichOneof('model')
    self._model_config = self._model_config.multi_tower
    assert isinstance(self._model_config, MultiTowerConfig)
    self.check_supported(self._model_config, getattr(ctx, 'dense_dtype', 'f32'), ctx.engine)
    self._tower_num = len(self._model_config.towers)
    self._bst_tower_num = len(self._model_config.bst_towers)
    logging.info('all tower num: {0}'.format(self._tower_num + self._bst_tower_num))
    logging.info('bst tower num: {0}'.format(self._bst_tower_num))

  @staticmethod
  def check_supported(mt, dense_dtype, engine):
    """Build-time rejection of what the BST path does not cover (ValueError)."""
    if len(mt.din_towers):
      raise ValueError('MultiTowerBST: din_towers are not part of this model (the reference ignores them); use '
                       'MultiTowerDIN')
    if dense_dtype == 'bf16':
      raise ValueError('MultiTowerBST: dense_dtype bf16 is not supported with BST towers (the BST kernels are fp32)')
    if isinstance(engine, ShardedEmbeddingEngine):
      raise ValueError('MultiTowerBST: embedding-parallel training of a BST model is not supported')
    inputs = [t.input for t in mt.bst_towers]
    if len(set(inputs)) != len(inputs):
      # the reference regularises the key twice and the history once PER TOWER (:55-60); one group's lookups serve
      # every tower here, so a repeated group would count them fewer times than the reference does
      raise ValueError('MultiTowerBST: two BST towers read the same seq_att_group (%s); give each tower its own group'
                       % ', '.join(inputs))
    for tower in mt.bst_towers:
      bst_layer.check_envelope(tower.seq_len, 1, tower.multi_head_size, name='bst tower %s' % tower.input)

  def _declare_key_l2(self, tower_index, group_name):
    """The second L2 term of the key (multi_tower_bst.py:57-58): one more lookup of the key columns into a regularised
    group of its own (build pass only)."""
    eng = self._seq_input_layer._engine
    if not self._emb_reg or eng.finalized:
      return
    plan = self._seq_input_layer._plan[(group_name, group_name)]
    if plan['kkey'] is None:
      return
    gkey = 'bst:%d:%s:key_l2' % (tower_index, group_name)
    if gkey in eng.groups:
      return
    cols = sorted(plan['own_cols'].values())
    eng.declare_group(gkey, sum(d for _, d in cols), self._emb_reg)
    by_id = {id(c): c for kind, c in plan['key_plan'] if kind == 'own'}
    for cid, (c0, _) in plan['own_cols'].items():
      declare_lookup(eng, self._feature_dict, by_id[cid], group_name, gkey, c0, eng.batch_size)

  def build_predict_graph(self):
    # input layer calls in the reference's constructor order: plain towers, then BST towers (:40-60)
    tower_features = []
    for tower in self._model_config.towers:
      tower_feature, _ = self._input_layer(self._feature_dict, tower.input)
      tower_features.append(tower_feature)
    bst_features = []
    for i, tower in enumerate(self._model_config.bst_towers):
      fea = self._seq_input_layer(self._feature_dict, tower.input, requires_grad=self._is_training,
                                  static_history=True)
      if fea['aux_hist_seq_emb_list']:
        raise ValueError('MultiTowerBST: aux_hist_seq is not supported')
      self._declare_key_l2(i, tower.input)
      bst_features.append(fea)

    stacks, inputs = [], []
    for tower, tower_fea in zip(self._model_config.towers, tower_features):
      tower_name = tower.input
      inputs.append(dnn.batch_norm(tower_fea, '%s_fea_bn' % tower_name, self._is_training))
      stacks.append(dnn.DNN(tower.dnn, self._l2_reg, '%s_dnn' % tower_name, self._is_training))
    tower_fea_arr, _ = dnn.run_parallel(stacks, inputs) if stacks else ([], [])
    for i, (tower, fea) in enumerate(zip(self._model_config.bst_towers, bst_features)):
      tower_fea_arr.append(bst_layer.bst(fea['key'], fea['hist_seq_emb'], fea['hist_seq_len'], tower.seq_len,
                                         tower.multi_head_size, ln_index=2 * i))

    all_fea = kernels.concat_cols(tower_fea_arr)
    final_dnn_layer = dnn.DNN(self._model_config.final_dnn, self._l2_reg, 'final_dnn', self._is_training)
    all_fea = final_dnn_layer(all_fea)
    output = dnn.dense(all_fea, self._num_class, 'output', head=True)
    self._add_to_prediction_dict(output)
    return self._prediction_dict
