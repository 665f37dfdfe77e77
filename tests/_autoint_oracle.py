"""OracleTrainer for AutoInt (reference model/autoint.py:16-80), test-side: oracle/ stays as it is.

An AutoInt config is dispatched as FM, and _fm is overridden with the AutoInt assembly: the `all` group through the
oracle's input layer (its sequence_features' target attention appended, embedding L2 included), reshaped to [B, F, D],
the interacting layers of tests/_autoint_ref.py with their kernels' L2 (l2_regularization of the autoint message), then
dense(num_class, 'output') without a regulariser."""
from oracle.model_oracle import OracleTrainer
from tests import _autoint_ref


class AutoIntOracle(OracleTrainer):

  def __init__(self, cfg, state, batch_size, **kw):
    super(AutoIntOracle, self).__init__(cfg, state, batch_size, **kw)
    self._autoint = self.model_class == 'AutoInt'
    if self._autoint:
      self.model_class = 'FM'

  def _fm(self, V, batch):
    if not self._autoint:
      return super(AutoIntOracle, self)._fm(V, batch)
    mc = self.cfg.model_config
    ai = mc.autoint
    l2 = self._l2_of(mc)
    fea, _ = self.input_layer(V, batch, 'all', 'input_layer')
    D = self.features[0].embedding_dim
    B = fea.shape[0]
    x = fea.reshape(B, -1, D)
    for i in range(ai.interacting_layer_num):
      name = _autoint_ref.layer_name(i)
      params = {n: V.get(n, l2=l2) for n in _autoint_ref.names(name)}
      x = _autoint_ref.mha_layer(x, ai.multi_head_num, ai.multi_head_size, params, name)
    out = self.dense(V, x.reshape(B, -1), mc.num_class, 'output', 0.0)
    return {'logits': out.squeeze(1)}
