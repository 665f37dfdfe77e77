"""OracleTrainer for MultiTowerBST (reference model/multi_tower_bst.py:19-190), test-side: oracle/ stays as it is.

A MultiTowerBST config is dispatched as MultiTowerDIN, and _multi_tower_din is overridden with the BST assembly: the
plain towers (BatchNorm + DNN), then every BST tower's block (tests/_bst_ref.py, on the oracle's batch-max history)
in config order, concatenated -> final_dnn -> output.  The oracle's seq_input_layer regularises the key and the history
once; the second L2 term of the key (:57-58) is added here."""
import torch

from oracle.model_oracle import OracleTrainer
from tests import _bst_ref


class BSTOracle(OracleTrainer):

  def __init__(self, cfg, state, batch_size, **kw):
    super(BSTOracle, self).__init__(cfg, state, batch_size, **kw)
    self._bst = self.model_class == 'MultiTowerBST'
    if self._bst:
      self.model_class = 'MultiTowerDIN'
    self.last_bst = []

  def _multi_tower_din(self, V, batch):
    if not self._bst:
      return super(BSTOracle, self)._multi_tower_din(V, batch)
    mc = self.cfg.model_config
    c = mc.multi_tower
    l2 = self._l2_of(mc)
    lam = mc.embedding_regularization
    feas, scope_id = [], 0
    for tower in c.towers:
      scope = 'input_layer' if scope_id == 0 else 'input_layer_%d' % scope_id
      scope_id += 1
      fea, _ = self.input_layer(V, batch, tower.input, scope)
      feas.append(fea)
    bst_feas = []
    for tower in c.bst_towers:
      fea = self.seq_input_layer(V, batch, tower.input)
      if lam > 0:  # the key's second term (the history's is seq_input_layer's own)
        self._reg = self._reg + lam * 0.5 * (fea['key'] * fea['key']).sum()
      bst_feas.append(fea)
    arr = []
    for tower, fea in zip(c.towers, feas):
      fea = self.batch_norm(V, fea, '%s_fea_bn' % tower.input)
      arr.append(self.dnn(V, fea, tower.dnn, '%s_dnn' % tower.input, l2))
    self.last_bst = []
    for i, (tower, fea) in enumerate(zip(c.bst_towers, bst_feas)):
      E = fea['hist_seq_emb'].shape[-1]
      lns = ('layer_normalization' if i == 0 else 'layer_normalization_%d' % (2 * i), 'layer_normalization_%d' % (2 * i + 1))
      params = {n: V.get(n) for n in _bst_ref.param_names(E, tower.multi_head_size, lns)}
      out = _bst_ref.bst_block(fea['key'], fea['hist_seq_emb'], torch.as_tensor(fea['hist_seq_len']), tower.seq_len,
                               tower.multi_head_size, params, ln_names=lns)
      self.last_bst.append(out.detach())
      arr.append(out)
    all_fea = self.dnn(V, torch.cat(arr, dim=1), c.final_dnn, 'final_dnn', l2)
    out = self.dense(V, all_fea, mc.num_class, 'output', 0.0)
    return {'logits': out.squeeze(1)}
