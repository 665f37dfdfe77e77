"""MIND (reference easy_rec/python/model/mind.py:21-445): multi-interest retrieval.

The `hist` group's sequences (read uncombined; SUM: their mean, CONCAT: side by side) go through an optional
`pre_capsule_dnn`, an optional softmax over the `time_id_fea` column, and the capsule layer with dynamic routing
(layers/capsule_layer.py: one HIP launch each way).  The `user` group goes through `user_fea_bn` -> `user_dnn`, is tiled
over the max_k capsules and concatenated with them; `concat_dnn` runs over the [B * max_k, .] rows on all hidden units
but the last (its BatchNorm statistics cover every row, padded capsule rows included, as the reference's do), then a
plain dense `concat_dnn/dnn_<n-1>`.  The `item` group goes through `item_dnn` with the same last-layer rule.  With
COSINE both are L2-normalised (no temperature).  The label-aware attention weighs the interests by their similarity to
the positive item (simi_pow; >= 100: the most similar one only) into `user_tower_emb`; from there on the head, the
losses and the recall metrics are MatchModel's.  `reg_interest_simi` joins the losses when max_interests_simi < 1.

With `negative_sampler_in_memory` or `negative_sampler` (input/neg_sampler.py) the `item` group has B + N rows: item_dnn's
BatchNorm covers them all, the label-aware attention reads the batch's own B, the head and the recall metrics take all
B + N columns.

Not built: the per-user and hard-negative samplers (refused at build time by MatchModel, `hard_neg_acc` with them),
bf16 dense and the embedding-parallel engine (MatchModel.check_supported)."""
import logging

import torch

from easyrec_amd.layers import capsule_layer
from easyrec_amd.layers import dnn
from easyrec_amd.layers import match_head
from easyrec_amd.model.match_model import MatchModel
from easyrec_amd.protos import dnn_pb2
from easyrec_amd.protos.loss_pb2 import LossType
from easyrec_amd.protos.mind_pb2 import MIND as MINDConfig
from easyrec_amd.protos.simi_pb2 import Similarity


def interest_similarity(user_interests, high_capsules, user_emb_num):
  """MIND._build_interest_simi (mind.py:260-299) -> (avg_interest_simi, avg_capsule_simi), composed of torch ops."""
  K = user_interests.shape[1]
  num = user_emb_num.to(torch.int64)
  mask = (torch.arange(K, device=num.device)[None, :] < num[:, None]).to(user_interests.dtype)[:, :, None]
  div = torch.clamp((num * (num - 1)).to(user_interests.dtype), min=1.0)
  multi = (num > 1).to(user_interests.dtype)
  sum_div = torch.clamp(multi.sum(), min=1.0)

  def avg(x):
    x = capsule_layer.normalize_compose(x) * mask
    simi = (x.sum(dim=1) ** 2 - (x * x).sum(dim=1)).sum(dim=1) / div
    return ((simi + 1) * multi).sum() / 2.0 / sum_div

  return avg(user_interests), avg(high_capsules)


class MIND(MatchModel):

  def __init__(self, model_config, feature_configs, features, labels=None, is_training=False):
    super(MIND, self).__init__(model_config, feature_configs, features, labels, is_training)
    self._take_config('mind')
    cfg = self._model_config
    self.user_dnn, self.item_dnn, self.concat_dnn = cfg.user_dnn, cfg.item_dnn, cfg.concat_dnn
    assert cfg.simi_func in (Similarity.COSINE, Similarity.INNER_PRODUCT)
    self._capsule_layer = capsule_layer.CapsuleLayer(cfg.capsule_config, self._is_training)

  def _last_layer_dense(self, x, config, name):
    """a DNN over all hidden units but the last, then a plain dense <name>/dnn_<n-1> (mind.py:138-158)"""
    units = list(config.hidden_units)
    body = dnn_pb2.DNN()
    body.CopyFrom(config)  # (a copy: the config itself keeps every hidden unit)
    del body.hidden_units[:]
    body.hidden_units.extend(units[:-1])
    if units[:-1]:
      x = dnn.DNN(body, self._l2_reg, name, self._is_training)(x)
    return dnn.dense(x, units[-1], '%s/dnn_%d' % (name, len(units) - 1), l2_reg=self._l2_reg)

  def _hist_sequence(self):
    """-> (hist_seq_feas [B, L, D], hist_seq_len [B]) in front of the capsule layer (mind.py:54-101)"""
    cfg = self._model_config
    seqs, _, _ = self._input_layer(self._feature_dict, 'hist', is_combine=False)
    names = self._input_layer.sequence_names('hist')
    time_id_fea = None
    if cfg.time_id_fea:
      found = [fea for (fea, _), name in zip(seqs, names) if cfg.time_id_fea in name]
      logging.info('time_id_fea is set(%s), find num: %d' % (cfg.time_id_fea, len(found)))
      time_id_fea = found[0] if found else None
    feas = [fea for (fea, _), name in zip(seqs, names) if time_id_fea is None or cfg.time_id_fea not in name]
    hist_seq_len = seqs[0][1]  # it is assumed that all hist have the same length
    if cfg.user_seq_combine == MINDConfig.SUM:
      shapes = [tuple(f.shape[1:]) for f in feas]
      assert all(s == shapes[0] for s in shapes), 'all hist seq must have the same embedding shape, but: %s' % str(shapes)
      hist = feas[0]
      for f in feas[1:]:
        hist = hist + f
      hist = hist / len(feas)
    else:
      hist = feas[0] if len(feas) == 1 else torch.cat(feas, dim=2)
    if cfg.HasField('pre_capsule_dnn') and len(cfg.pre_capsule_dnn.hidden_units) > 0:
      B, L, D = hist.shape
      hist = dnn.DNN(cfg.pre_capsule_dnn, self._l2_reg, 'pre_capsule_dnn', self._is_training)(hist.reshape(B * L, D))
      hist = hist.reshape(B, L, -1)
    if time_id_fea is not None:
      assert time_id_fea.shape[-1] == 1, 'time_id must have only embedding_size of 1'
      Lt = time_id_fea.shape[1]
      tmask = torch.arange(Lt, device=hist.device)[None, :] < hist_seq_len[:, None]
      tmask = (tmask.to(hist.dtype) * 2 - 1) * capsule_layer.MASK_VALUE
      hist = hist * torch.softmax(torch.minimum(time_id_fea, tmask[:, :, None]), dim=1)
    return hist, hist_seq_len

  def build_predict_graph(self):
    cfg = self._model_config
    # (the three input-layer calls first, in the reference's constructor order)
    hist, hist_seq_len = self._hist_sequence()
    user_features = self._group('user')[0]
    item_features = self._group('item')[0]

    self._capsule_layer._is_training = self._is_training
    high_capsules, num_high_capsules = self._capsule_layer(hist, hist_seq_len)
    B, K, _ = high_capsules.shape

    user_features = dnn.batch_norm(user_features, 'user_fea_bn', self._is_training)
    user_features = dnn.DNN(self.user_dnn, self._l2_reg, 'user_dnn', self._is_training)(user_features)
    user_tile = user_features[:, None, :].expand(B, K, user_features.shape[1])
    user_interests = torch.cat([high_capsules, user_tile], dim=2).reshape(B * K, -1)
    user_interests = self._last_layer_dense(user_interests, self.concat_dnn, 'concat_dnn')
    item_tower_emb = self._last_layer_dense(item_features, self.item_dnn, 'item_dnn')
    if cfg.simi_func == Similarity.COSINE:
      item_tower_emb = self.norm(item_tower_emb)
      user_interests = self.norm(user_interests)
    user_interests = user_interests.reshape(B, K, -1)

    # label guided attention: the item features attend over the interests
    user_tower_emb, user_interests = capsule_layer.label_aware_attention(user_interests, item_tower_emb[:B],
                                                                         num_high_capsules, cfg.simi_pow)
    # (both embeddings are final: MatchModel's head takes them as an inner product, MIND has no temperature)
    pd = self._finish_predict_graph(user_tower_emb, item_tower_emb, Similarity.INNER_PRODUCT, 1.0, cfg.scale_simi)
    pd['high_capsules'] = high_capsules
    pd['user_interests'] = user_interests
    pd['user_emb_num'] = num_high_capsules
    if self._labels is not None:
      pd['interests_simi'], self._capsule_simi = interest_similarity(user_interests, high_capsules, num_high_capsules)
    return pd

  def build_loss_graph(self):
    loss_dict = super(MIND, self).build_loss_graph()
    if self._model_config.max_interests_simi < 1.0:
      value = torch.relu(self._prediction_dict['interests_simi'] - self._model_config.max_interests_simi)
      loss_dict['reg_interest_simi'] = value.detach()
      if value.requires_grad:
        self._backward_seeds.append((value, torch.ones_like(value)))
    return loss_dict

  def build_metric_graph(self, eval_config):
    pd = self._prediction_dict
    interest_simi, capsule_simi = interest_similarity(pd['user_interests'].detach(), pd['high_capsules'].detach(),
                                                      pd['user_emb_num'])
    metric_dict = {'interest_similarity': float(interest_simi), 'capsule_similarity': float(capsule_simi)}
    if self._is_point_wise:
      metric_dict.update(self._build_point_wise_metric_graph(eval_config))
      self._metric_dict.update(metric_dict)
      return metric_dict
    # the best interest's similarity to every item of the batch: the rank of each row's positive (mind.py:322-368)
    user_interests, item_tower_emb = pd['user_interests'].detach(), pd['item_tower_emb'].detach()
    B = user_interests.shape[0]
    sim = torch.einsum('bhe,ne->bhn', user_interests, item_tower_emb).max(dim=1).values
    diag = torch.diagonal(sim[:, :B])[:, None]
    idx = torch.arange(B, device=sim.device)
    above = (sim[:, :B] > diag) | ((sim[:, :B] == diag) & (idx[None, :] < idx[:, None]))
    c_in, c_neg = above.sum(dim=1), (sim[:, B:] > diag).sum(dim=1)
    for metric in eval_config.metrics_set:
      if metric.WhichOneof('metric') != 'recall_at_topk':
        continue
      k = metric.recall_at_topk.topk
      r = match_head.recall_at_k(c_in, c_neg, k)
      metric_dict['interests_recall@%d' % k] = r['recall@%d' % k]
      metric_dict['interests_neg_sam_recall@%d' % k] = r['recall_neg_sam@%d' % k]
    metric_dict.update(self._build_list_wise_metric_graph(eval_config))
    self._metric_dict.update(metric_dict)
    return metric_dict

  def get_outputs(self):
    tail = ['user_emb', 'item_emb', 'user_emb_num', 'user_interests', 'item_tower_emb']
    if self._loss_type in (LossType.CLASSIFICATION, LossType.SOFTMAX_CROSS_ENTROPY):
      return ['logits', 'probs'] + tail
    if self._loss_type == LossType.L2_LOSS:
      return ['y'] + tail
    raise ValueError('invalid loss type: %s' % str(self._loss_type))

  def build_output_dict(self):
    pd = self._prediction_dict
    if 'user_emb' not in pd:
      # tf.reduce_join over the interests' as_string: a row's values joined by ',', the interests by '|'
      pd['user_emb'] = ['|'.join(','.join('%f' % v for v in row) for row in rows)
                        for rows in pd['user_interests'].detach().cpu().tolist()]
    return super(MIND, self).build_output_dict()
