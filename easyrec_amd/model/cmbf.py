"""CMBF (reference easy_rec/python/model/cmbf.py:15-47): the cross-modal fusion layer of layers/cmbf.py (feature groups
`image`, `general`, `text`, `other`; BERT-style towers and cross-attention blocks on HIP launches,
layers/multihead_cross_attention.py), then `final_dnn` and dense(num_class, name='output').  Only `final_dnn` and the
layer's `other_dnn` carry the model's L2 regulariser; the towers' dense layers have none."""
from easyrec_amd.layers import cmbf
from easyrec_amd.layers import dnn
from easyrec_amd.model.rank_model import RankModel


class CMBF(RankModel):

  def __init__(self, model_config, feature_configs, features, labels=None, is_training=False):
    super(CMBF, self).__init__(model_config, feature_configs, features, labels, is_training)
    config = self._take_config('cmbf')
    self._cmbf_layer = cmbf.CMBF(model_config, feature_configs, self._feature_dict, config.config, self._input_layer)

  def build_predict_graph(self):
    hidden = self._cmbf_layer(self._is_training, l2_reg=self._l2_reg)
    all_fea = self._dnn(hidden, self._model_config.final_dnn, 'final_dnn')
    return self._emit(dnn.dense(all_fea, self._num_class, 'output', head=True))
