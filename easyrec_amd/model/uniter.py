"""Uniter (reference easy_rec/python/model/uniter.py:15-46): the multi-modal layer of layers/uniter.py (feature groups
`image`, `general`, `text`, `other`; a BERT-style encoder on HIP launches, layers/multihead_cross_attention.py), then
`final_dnn` and dense(num_class, name='output').  Only `final_dnn` and the layer's `other_dnn` carry the model's L2
regulariser; the encoder's dense layers have none."""
from easyrec_amd.layers import dnn
from easyrec_amd.layers import uniter
from easyrec_amd.model.rank_model import RankModel


class Uniter(RankModel):

  def __init__(self, model_config, feature_configs, features, labels=None, is_training=False):
    super(Uniter, self).__init__(model_config, feature_configs, features, labels, is_training)
    config = self._take_config('uniter')
    self._uniter_layer = uniter.Uniter(model_config, feature_configs, self._feature_dict, config.config, self._input_layer)

  def build_predict_graph(self):
    hidden = self._uniter_layer(self._is_training, l2_reg=self._l2_reg)
    all_fea = self._dnn(hidden, self._model_config.final_dnn, 'final_dnn')
    return self._emit(dnn.dense(all_fea, self._num_class, 'output', head=True))
