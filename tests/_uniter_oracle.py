"""OracleTrainer for `model_class: Uniter` and for DBMTL with `bottom_uniter`, test-side: oracle/ stays as it is.

The input layer, the DNNs, BatchNorm, the losses, the regularisers and the optimizer are the parent's.  The Uniter layer
(reference layers/uniter.py, model/uniter.py:38-46, model/dbmtl.py:35-53) is tests/_uniter_ref.py's restatement over the
parent's variables: groups read in the reference constructor's order (image, general, text with is_combine=False,
other; each combined call takes the next `input_layer[_n]` scope, the sequence tables are
`input_layer/<feature>/embedding_weights`), the [CLS] feature of the encoder, `other_dnn` (or the raw `other` features)
beside it, then `final_dnn` and dense `output` (Uniter) or the towers (DBMTL).  Only final_dnn, other_dnn and DBMTL's
towers carry the kernel regulariser.  Dropout is not restated: configs with a dropout probability above 0 are refused
in training."""
import torch

from oracle.model_oracle import OracleTrainer
from tests import _uniter_ref as ref


class _Params(object):
  """name -> the oracle's variable (no regulariser), created on first use"""

  def __init__(self, V):
    self.V = V

  def __getitem__(self, name):
    return self.V.get(name)


class UniterOracle(OracleTrainer):

  def _uniter_layer(self, V, batch, c, l2):
    mc = self.cfg.model_config
    groups = {g.group_name: g for g in mc.feature_groups}
    if self.is_training_step and (c.hidden_dropout_prob > 0 or c.attention_probs_dropout_prob > 0):
      raise NotImplementedError('UniterOracle: dropout is not restated')
    scopes = iter(['input_layer'] + ['input_layer_%d' % i for i in range(1, 4)])
    img = general = None
    if 'image' in groups:
      fea, _ = self.input_layer(V, batch, 'image', next(scopes))
      img = fea.reshape(fea.shape[0], len(groups['image'].feature_names), -1)
    if 'general' in groups:
      fea, _ = self.input_layer(V, batch, 'general', next(scopes))
      general = fea.reshape(fea.shape[0], len(groups['general'].feature_names), -1)
    seqs = []
    if 'text' in groups:
      lam = mc.embedding_regularization
      for n in groups['text'].feature_names:
        e, lens = self._seq_lookup(V, 'input_layer/%s/embedding_weights' % n, batch, n)
        if lam > 0:
          self._reg = self._reg + lam * 0.5 * (e * e).sum()
        seqs.append((e, lens))
    parts = []
    if img is not None or general is not None or seqs:
      parts.append(ref.uniter_cls(_Params(V), c, img, general, seqs))
    if 'other' in groups:
      other, _ = self.input_layer(V, batch, 'other', next(scopes))
      if c.HasField('other_feature_dnn'):
        other = self.dnn(V, other, c.other_feature_dnn, 'other_dnn', l2)
      parts.append(other)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)

  is_training_step = True

  def _uniter(self, V, batch):
    mc = self.cfg.model_config
    l2 = self._l2_of(mc)
    hidden = self._uniter_layer(V, batch, mc.uniter.config, l2)
    x = self.dnn(V, hidden, mc.uniter.final_dnn, 'final_dnn', l2)
    return {'logits': self.dense(V, x, mc.num_class, 'output', 0.0).squeeze(1)}

  def _autoint(self, V, batch):  # (forward()'s dispatch knows no Uniter: it is reached under AutoInt's name)
    if self.cfg.model_config.model_class == 'Uniter':
      return self._uniter(V, batch)
    return super(UniterOracle, self)._autoint(V, batch)

  def input_layer(self, V, batch, group_name, scope, wide_dim=None, only=None):
    if group_name == 'all' and self.cfg.model_config.model_class == 'DBMTL' and \
        self.cfg.model_config.dbmtl.HasField('bottom_uniter'):
      # (dbmtl.py:35-53: the Uniter layer in place of the `all` group; _dbmtl's bottom_dnn is not set beside it)
      mc = self.cfg.model_config
      return self._uniter_layer(V, batch, mc.dbmtl.bottom_uniter, self._l2_of(mc)), None
    return super(UniterOracle, self).input_layer(V, batch, group_name, scope, wide_dim=wide_dim, only=only)

  def forward(self, batch):
    if self.cfg.model_config.model_class != 'Uniter':
      return super(UniterOracle, self).forward(batch)
    self.model_class = 'AutoInt'
    try:
      return super(UniterOracle, self).forward(batch)
    finally:
      self.model_class = 'Uniter'

  def train_step(self, batch):
    out = super(UniterOracle, self).train_step(batch)
    mc = self.cfg.model_config
    if mc.model_class == 'DBMTL':
      # a regression tower's output is `y_<tower>` in the product (rank_model.py: the reference's name); the parent
      # keeps every tower's under logits_<tower>
      from easyrec_amd.protos.loss_pb2 import LossType
      for tower in mc.dbmtl.task_towers:
        if tower.loss_type in (LossType.L2_LOSS, LossType.SIGMOID_L2_LOSS) and 'logits_' + tower.tower_name in self.last_pred:
          self.last_pred['y_' + tower.tower_name] = self.last_pred.pop('logits_' + tower.tower_name)
    return out
