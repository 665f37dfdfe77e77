"""OracleTrainer for `model_class: CMBF`, test-side: oracle/ stays as it is.

The input layer, the DNNs, BatchNorm, the losses, the regularisers and the optimizer are the parent's.  The CMBF layer
(reference layers/cmbf.py, model/cmbf.py:39-47) is tests/_cmbf_ref.py's restatement over the parent's variables: groups
read in the reference constructor's order (image, general, text with is_combine=False, other; each combined call takes
the next `input_layer[_n]` scope, the sequence tables are `input_layer/<feature>/embedding_weights`), both towers, the
cross-attention tower, the poolings, `other_dnn` (or the raw `other` features) beside them, then `final_dnn` and dense
`output`.  Only final_dnn and other_dnn carry the kernel regulariser.  Dropout is not restated: configs with a dropout
probability above 0 are refused in training."""
import torch

from oracle.model_oracle import OracleTrainer
from tests import _cmbf_ref as cref
from tests._uniter_oracle import _Params


class CMBFOracle(OracleTrainer):

  def _cmbf_layer(self, V, batch, c, l2):
    mc = self.cfg.model_config
    groups = {g.group_name: g for g in mc.feature_groups}
    if c.hidden_dropout_prob > 0 or c.attention_probs_dropout_prob > 0 or c.text_seq_emb_dropout_prob > 0:
      raise NotImplementedError('CMBFOracle: dropout is not restated')
    scopes = iter(['input_layer'] + ['input_layer_%d' % i for i in range(1, 4)])
    img = general = None
    n_img = 0
    if 'image' in groups:
      img, _ = self.input_layer(V, batch, 'image', next(scopes))
      n_img = len(groups['image'].feature_names)
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
      parts.append(cref.cmbf_towers(_Params(V), c, img, n_img, general, seqs)['fused'])
    if 'other' in groups:
      other, _ = self.input_layer(V, batch, 'other', next(scopes))
      if c.HasField('other_feature_dnn'):
        other = self.dnn(V, other, c.other_feature_dnn, 'other_dnn', l2)
      parts.append(other)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)

  def _cmbf(self, V, batch):
    mc = self.cfg.model_config
    l2 = self._l2_of(mc)
    hidden = self._cmbf_layer(V, batch, mc.cmbf.config, l2)
    x = self.dnn(V, hidden, mc.cmbf.final_dnn, 'final_dnn', l2)
    return {'logits': self.dense(V, x, mc.num_class, 'output', 0.0).squeeze(1)}

  def _autoint(self, V, batch):  # (forward()'s dispatch knows no CMBF: it is reached under AutoInt's name)
    if self.cfg.model_config.model_class == 'CMBF':
      return self._cmbf(V, batch)
    return super(CMBFOracle, self)._autoint(V, batch)

  def forward(self, batch):
    if self.cfg.model_config.model_class != 'CMBF':
      return super(CMBFOracle, self).forward(batch)
    self.model_class = 'AutoInt'
    try:
      return super(CMBFOracle, self).forward(batch)
    finally:
      self.model_class = 'CMBF'
