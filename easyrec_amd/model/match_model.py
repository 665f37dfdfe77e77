"""MatchModel: two tower embeddings -> similarity -> point-wise or list-wise loss.

API and key names of reference easy_rec/python/model/match_model.py:18-357: `loss_type` CLASSIFICATION / L2_LOSS make
a point-wise model (one similarity per example, sigmoid cross-entropy or L2 against the label), SOFTMAX_CROSS_ENTROPY a
list-wise one (every user against every item of the batch, softmax, the diagonal is the positive); `item_id` /
`ignore_in_batch_neg_sam` mask in-batch negatives; prediction keys `logits` / `probs` / `y`, `user_tower_emb` /
`item_tower_emb`, `user_emb` / `item_emb`; loss keys `cross_entropy_loss`, `reg_pos_loss`, `l2_loss`; the metrics
`recall@k`, `recall_neg_sam@k`, `recall_in_batch@k`, `auc`, `mean_absolute_error`.  `model_params` configures the backbone
form (:145-205).

While training, the list-wise head never builds its [B, B] logits: build_predict_graph stops at the tower embeddings and
build_loss_graph hands them to layers/match_head.py (one fused forward, the backward recomputing the logits).  Outside
training `logits` and `probs` are composed of torch ops.  Item rows beyond the batch come from
`negative_sampler_in_memory` and `negative_sampler` (input/neg_sampler.py: N rows drawn on the device inside the step -
uniform without replacement, or weighted with replacement - the item group then has B + N rows and every head function
here takes M = B + N columns); the per-user and hard-negative graphlearn samplers are refused at build time.  predict() does not sample (the reference's PREDICT mode): the item tower sees the batch's B rows.
"""
import logging

import torch

from easyrec_amd.builders import loss_builder
from easyrec_amd.core import context
from easyrec_amd.layers import match_head
from easyrec_amd.layers.sharded_embedding import ShardedEmbeddingEngine
from easyrec_amd.model.easy_rec_model import EasyRecModel
from easyrec_amd.protos.loss_pb2 import LossType
from easyrec_amd.protos.simi_pb2 import Similarity

_REFUSED_SAMPLERS = ('negative_sampler_v2', 'hard_negative_sampler', 'hard_negative_sampler_v2')


class MatchModel(EasyRecModel):

  def __init__(self, model_config, feature_configs, features, labels=None, is_training=False):
    super(MatchModel, self).__init__(model_config, feature_configs, features, labels, is_training)
    self._loss_type = self._model_config.loss_type
    self._num_class = self._model_config.num_class
    self._outputs = []
    if self._loss_type == LossType.CLASSIFICATION:
      assert self._num_class == 1
    self._is_point_wise = self._loss_type in (LossType.CLASSIFICATION, LossType.L2_LOSS)
    logging.info('Use %s wise dssm.' % ('point' if self._is_point_wise else 'list'))
    cls_mem = self._model_config.WhichOneof('model')
    sub_model_config = getattr(self._model_config, cls_mem)
    self._item_id_name = getattr(sub_model_config, 'item_id', '') or None
    if self._item_id_name:
      logging.info('item_id feature is: %s' % self._item_id_name)
      features.ids_of(self._item_id_name)  # (KeyError now rather than at the first step)
    ctx = context.current()
    self.check_supported(self._loss_type, getattr(ctx, 'dense_dtype', 'f32'), ctx.engine, type(self).__name__)
    if getattr(features, 'sampler', None) is not None and self._is_point_wise:
      raise ValueError('%s: a negative sampler needs a list-wise loss (SOFTMAX_CROSS_ENTROPY): the sampled rows have no '
                       'labels for %s' % (type(self).__name__, LossType.Name(self._loss_type)))
    if 'hard_neg_indices' in features:
      raise NotImplementedError('%s: a batch with hard_neg_indices (hard negative examples) is not supported' %
                                type(self).__name__)

  # -- build-time refusals
  @staticmethod
  def check_supported(loss_type, dense_dtype, engine, what='MatchModel'):
    if dense_dtype == 'bf16':
      raise ValueError('%s: dense_dtype bf16 is not supported (the head kernels are fp32)' % what)
    if isinstance(engine, ShardedEmbeddingEngine):
      raise ValueError('%s: embedding-parallel training of a two-tower model is not supported' % what)
    if loss_type not in (LossType.CLASSIFICATION, LossType.L2_LOSS, LossType.SOFTMAX_CROSS_ENTROPY):
      raise ValueError('invalid loss type: %s' % LossType.Name(loss_type))

  supports_sampled_negatives = True

  @staticmethod
  def check_data_config(data_config):
    """The estimator's build-time hook: negative_sampler_in_memory and negative_sampler are built
    (input/neg_sampler.py); the other three draw per user or hard negatives along graphlearn edges, which nothing
    here restates."""
    sampler = data_config.WhichOneof('sampler')
    if sampler in _REFUSED_SAMPLERS:
      raise NotImplementedError('data_config.%s: negative sampling is not supported (the item tower sees the '
                                "batch's own rows only)" % sampler)

  @property
  def _item_ids(self):
    return self._feature_dict.ids_of(self._item_id_name) if self._item_id_name else None

  @property
  def _ignore_in_batch(self):
    return bool(getattr(self._model_config, 'ignore_in_batch_neg_sam', False))

  # -- similarity
  def norm(self, fea):
    return match_head.normalize(fea)

  def _mask_in_batch(self, logits):
    B = logits.shape[0]
    eye = torch.eye(B, dtype=logits.dtype, device=logits.device)
    if self._ignore_in_batch:
      mask = 1 - eye
    elif self._item_ids is not None:
      ids = self._item_ids
      mask = (ids[None, :B] == ids[:B, None]).to(logits.dtype) - eye
    else:
      return logits
    return torch.cat([logits[:, :B] - mask * match_head.MASK_VALUE, logits[:, B:]], dim=1)

  def _point_wise_sim(self, user_emb, item_emb):
    return (user_emb * item_emb).sum(dim=1, keepdim=True)

  def _list_wise_sim(self, user_emb, item_emb):
    if self._is_predicting:
      # (the exported model scores (user, item) pairs row by row: never a sampled step, the towers have the same rows)
      assert user_emb.shape[0] == item_emb.shape[0], 'a predicting model does not sample negatives'
      return self._point_wise_sim(user_emb, item_emb)
    return user_emb @ item_emb.t()

  def sim(self, user_emb, item_emb):
    return self._point_wise_sim(user_emb, item_emb) if self._is_point_wise else self._list_wise_sim(user_emb, item_emb)

  def _scale_variables(self):
    vs = context.varstore()
    return vs.get_variable('sim_w', (1,), 'ones'), vs.get_variable('sim_b', (1,), 'zeros')

  def _finish_predict_graph(self, user_tower_emb, item_tower_emb, simi_func, temperature, scale_simi):
    """dssm.py:64-106 / match_model.py:161-205 from the two tower outputs on"""
    cosine = simi_func == Similarity.COSINE
    if cosine:
      user_tower_emb, item_tower_emb = self.norm(user_tower_emb), self.norm(item_tower_emb)
    self._inv_temperature = 1.0 / temperature if cosine else 1.0
    self._sim_w, self._sim_b = self._scale_variables() if scale_simi else (None, None)
    pd = self._prediction_dict
    pd['user_tower_emb'], pd['item_tower_emb'] = user_tower_emb, item_tower_emb
    lazy = not self._is_point_wise and self._is_training and not self._is_predicting and torch.is_grad_enabled()
    if not lazy:
      y_pred = self.sim(user_tower_emb, item_tower_emb) * self._inv_temperature
      if scale_simi:
        y_pred = y_pred * torch.abs(self._sim_w) + self._sim_b
      if self._is_point_wise:
        y_pred = y_pred.reshape(-1)
      if self._loss_type == LossType.CLASSIFICATION:
        pd['logits'] = y_pred
        pd['probs'] = torch.sigmoid(y_pred.detach())
      elif self._loss_type == LossType.SOFTMAX_CROSS_ENTROPY:
        y_pred = y_pred if self._is_predicting else self._mask_in_batch(y_pred)
        pd['logits'] = y_pred
        pd['probs'] = torch.softmax(y_pred, dim=1)
      else:
        pd['y'] = y_pred
    return pd

  @staticmethod
  def emb_strings(emb):
    """tf.reduce_join(tf.as_string(emb), axis=-1, separator=','): built on the host, only when asked for"""
    return [','.join('%f' % v for v in row) for row in emb.detach().cpu().tolist()]

  def build_predict_graph(self):
    if not self.has_backbone:
      raise NotImplementedError('method `build_predict_graph` must be implemented when you donot use backbone network')
    assert self._model_config.WhichOneof('model') == 'model_params', '`model_params` must be configured'
    mp = self._model_config.model_params
    self._outputs.extend(mp.outputs)
    output = self.backbone
    return self._finish_predict_graph(output[mp.user_tower_idx_in_output], output[mp.item_tower_idx_in_output],
                                      mp.simi_func, mp.temperature, mp.scale_simi)

  # -- losses
  def build_loss_graph(self):
    return self._build_point_wise_loss_graph() if self._is_point_wise else self._build_list_wise_loss_graph()

  def _build_list_wise_loss_graph(self):
    if self._loss_type != LossType.SOFTMAX_CROSS_ENTROPY:
      raise ValueError('invalid loss type: %s' % str(self._loss_type))
    pd = self._prediction_dict
    weight = self._sample_weight if torch.is_tensor(self._sample_weight) else None
    grads = None
    if self._sim_w is not None and self._sim_w.grad is not None and self._sim_b.grad is not None:
      grads = (self._sim_w.grad, self._sim_b.grad)
    ce, reg = match_head.match_head(pd['user_tower_emb'], pd['item_tower_emb'], self._inv_temperature, self._sim_w,
                                    self._sim_b, self._item_ids, self._ignore_in_batch, weight, grads)
    logging.info('softmax cross entropy loss is used')
    for name, value in (('cross_entropy_loss', ce), ('reg_pos_loss', reg)):
      self._loss_dict[name] = value.detach()
      if value.requires_grad:
        self._backward_seeds.append((value, torch.ones_like(value)))
    return self._loss_dict

  def _build_point_wise_loss_graph(self):
    label = next(iter(self._labels.values()))
    if self._loss_type == LossType.CLASSIFICATION:
      pred, loss_name = self._prediction_dict['logits'], 'cross_entropy_loss'
    elif self._loss_type == LossType.L2_LOSS:
      pred, loss_name = self._prediction_dict['y'], 'l2_loss'
    else:
      raise ValueError('invalid loss type: %s' % str(self._loss_type))
    value, dpred = loss_builder.build(self._loss_type, label, pred, self._sample_weight)
    self._backward_seeds.append((pred, dpred))
    self._loss_dict[loss_name] = value
    return self._loss_dict

  # -- metrics
  def build_metric_graph(self, eval_config):
    return self._build_point_wise_metric_graph(eval_config) if self._is_point_wise \
        else self._build_list_wise_metric_graph(eval_config)

  def _build_list_wise_metric_graph(self, eval_config):
    """match_model.py:287-317 on the batch currently loaded, from the rank counts of the positives (no sort)."""
    pd = self._prediction_dict
    c_in, c_neg = match_head.rank_counts(pd['user_tower_emb'], pd['item_tower_emb'], self._inv_temperature, self._sim_w,
                                         self._sim_b, self._item_ids, self._ignore_in_batch)
    metric_dict = {}
    for metric in eval_config.metrics_set:
      if metric.WhichOneof('metric') != 'recall_at_topk':
        raise ValueError('invalid metric type: %s' % str(metric))
      metric_dict.update(match_head.recall_at_k(c_in, c_neg, metric.recall_at_topk.topk))
    self._metric_dict.update(metric_dict)
    return metric_dict

  def _build_point_wise_metric_graph(self, eval_config):
    from easyrec_amd.core import metrics as metrics_lib
    metric_dict = {}
    label = next(iter(self._labels.values()))
    for metric in eval_config.metrics_set:
      kind = metric.WhichOneof('metric')
      if kind == 'auc':
        assert self._loss_type == LossType.CLASSIFICATION
        m = metrics_lib.AUC(int(metric.auc.num_thresholds), label.device)
        m.update(torch.trunc(label) if label.dtype.is_floating_point else label, self._prediction_dict['probs'], None)
        metric_dict['auc'] = m.result()
      elif kind == 'mean_absolute_error':
        assert self._loss_type == LossType.L2_LOSS
        metric_dict['mean_absolute_error'] = float(
            (label.to(torch.float32) - self._prediction_dict['y'].detach()).abs().mean())
      else:
        raise ValueError('invalid metric type: %s' % str(metric))
    self._metric_dict.update(metric_dict)
    return metric_dict

  # -- exported outputs
  def get_outputs(self):
    if not self.has_backbone and type(self) is MatchModel:
      raise NotImplementedError('could not call get_outputs on abstract class MatchModel')
    tail = ['user_emb', 'item_emb', 'user_tower_emb', 'item_tower_emb']
    if self._loss_type in (LossType.CLASSIFICATION, LossType.SOFTMAX_CROSS_ENTROPY):
      return ['logits', 'probs'] + tail
    if self._loss_type == LossType.L2_LOSS:
      return ['y'] + tail
    raise ValueError('invalid loss type: %s' % str(self._loss_type))

  def build_output_dict(self):
    pd = self._prediction_dict
    for key in ('user', 'item'):
      if key + '_emb' not in pd and key + '_tower_emb' in pd:
        pd[key + '_emb'] = self.emb_strings(pd[key + '_tower_emb'])
    if self._loss_type == LossType.SOFTMAX_CROSS_ENTROPY and 'logits' in pd and pd['logits'].dim() == 2 and \
        pd['logits'].shape[-1] == 1:
      # the exported list-wise model scores (user, item) pairs row by row (match_model.py:345-349)
      pd['logits'] = pd['logits'].squeeze(-1)
      pd['probs'] = torch.sigmoid(pd['logits'])
    return super(MatchModel, self).build_output_dict()
