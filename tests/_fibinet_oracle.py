"""OracleTrainer for backbones that hold a `FiBiNet` or `BiLinear` block (reference layers/keras/fibinet.py) and for
the input-layer block's `do_batch_norm` (layers/common_layers.py:142-191), test-side: oracle/ stays as it is.

_backbone is overridden for such backbones and defers to the parent otherwise: input-layer blocks (the per-feature
tf.layers.batch_normalization under TF's default names, counted over the graph), FiBiNet / BiLinear / SENet / MLP blocks,
concat_blocks, top_mlp.  SENet, the MLP, the dense layers and the input layer are the parent's."""
import torch

from oracle.model_oracle import OracleTrainer
from tests import _fibinet_ref as ref

_OWN = ('FiBiNet', 'BiLinear')


class FiBiNetOracle(OracleTrainer):

  def _bilinear(self, V, fields, cfg, name):
    kind = cfg.type.lower()
    params = {n: V.get(n) for n in ref.bilinear_names(name, kind, len(fields))}
    p = ref.bilinear_pairs(fields, kind, cfg.use_plus, params, name)
    return self.dense(V, p, cfg.num_output_units, name + '/output', 0.0)

  def _fibinet(self, V, fields, cfg, name, l2):
    feats = [self._keras_senet(V, fields, cfg.senet, name + '/senet')]
    if cfg.HasField('bilinear'):
      feats.append(self._bilinear(V, fields, cfg.bilinear, name + '/bilinear'))
    out = torch.cat(feats, dim=-1) if len(feats) > 1 else feats[0]
    if cfg.HasField('mlp'):
      out = self._keras_mlp(V, out, cfg.mlp, name + '/mlp', l2)
    return out

  def _backbone(self, V, batch):
    mc = self.cfg.model_config
    bb = mc.backbone
    if not any(b.WhichOneof('layer') == 'keras_layer' and b.keras_layer.class_name in _OWN for b in bb.blocks):
      return super(FiBiNetOracle, self)._backbone(V, batch)
    l2 = mc.model_params.l2_regularization
    outs, scope_id, bn_id = {}, 0, 0
    for blk in bb.blocks:
      kind = blk.WhichOneof('layer')
      if kind == 'input_layer':
        il = blk.input_layer
        scope = 'input_layer' if scope_id == 0 else 'input_layer_%d' % scope_id
        scope_id += 1
        fea, flist = self.input_layer(V, batch, blk.inputs[0].feature_group_name, scope)
        if il.do_batch_norm:
          if not il.only_output_feature_list:
            fea = self.batch_norm(V, fea, ref.bn_name(bn_id))
          flist = [self.batch_norm(V, f, ref.bn_name(bn_id + 1 + k)) for k, f in enumerate(flist)]
          bn_id += 1 + len(flist)
        outs[blk.name] = flist if il.only_output_feature_list else (
            (fea, flist) if il.output_2d_tensor_and_feature_list else fea)
        continue
      assert kind == 'keras_layer' and len(blk.inputs) == 1, 'FiBiNetOracle: block %s is not restated' % blk.name
      x = outs[blk.inputs[0].block_name]
      kl = blk.keras_layer
      if kl.class_name == 'FiBiNet':
        x = self._fibinet(V, list(x), kl.fibinet, blk.name, l2)
      elif kl.class_name == 'BiLinear':
        x = self._bilinear(V, list(x), kl.bilinear, blk.name)
      elif kl.class_name == 'SENet':
        x = self._keras_senet(V, x, kl.senet, blk.name)
      elif kl.class_name == 'MLP':
        x = self._keras_mlp(V, x, kl.mlp, blk.name, l2)
      else:
        raise NotImplementedError(kl.class_name)
      outs[blk.name] = x
    concat = list(bb.concat_blocks)
    out = torch.cat([outs[n] for n in concat], dim=-1) if len(concat) > 1 else outs[concat[0]]
    if bb.HasField('top_mlp'):
      out = self._keras_mlp(V, out, bb.top_mlp, 'backbone_top_mlp', l2)
    return out
