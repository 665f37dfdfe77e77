"""fp64 torch restatements of the two sequence combiners (TextCNN, attention pooling) and an OracleTrainer around them,
test-side: oracle/ stays as it is.

text_cnn_ref is written from the definition (windows gathered by index, an einsum per filter size), not from conv1d, so
that it does not share code with the composition it checks.  `select`: evaluate chosen outputs (b, f) under a GIVEN
selection of window positions (a weight per position, summing to 1) and a given ReLU decision instead of fp64's own
arg-max: what a test does where fp64's top two candidates lie too close for fp32 to be held to fp64's choice.

SeqCombinerOracle: the parent's input layer, DNNs, losses, regularisers and optimizer; a feature group's sequence
columns combined over time after the plain ones (reference layers/input_layer.py:309-347): sorted by column name,
tables `<scope>/<feature>_embedding/embedding_weights`, the embedding regulariser on the raw [B, L, D] embedding, then
`attention` (the variable `<scope>/<feature>_embedding/attention/kernel`, with the model's kernel regulariser) or
TextCNN (`.../<feature>_embedding_text_cnn/conv1d[_n]/kernel|bias`).  A backbone's `TextCNN` block is reached under
Dense's name (the parent's dispatch knows no TextCNN)."""
import copy

import torch

from oracle.model_oracle import OracleTrainer

MASKED_LOGIT = float(-2 ** 32 + 1)


def pad_or_truncate(x, P):
  B, L, D = x.shape
  if L >= P:
    return x[:, :P]
  return torch.cat([x, torch.zeros(B, P - L, D, dtype=x.dtype)], dim=1)


def text_cnn_pre(x, P, kernels, biases):
  """-> per filter size the pre-activations [B, P - k + 1, F]; x [B, L, D] padded / truncated to P (P <= 0: as it is)."""
  xp = pad_or_truncate(x, P) if P > 0 else x
  n_pos = xp.shape[1]
  out = []
  for w, b in zip(kernels, biases):
    k = w.shape[0]
    idx = torch.arange(n_pos - k + 1)[:, None] + torch.arange(k)[None, :]  # [np, k]
    win = xp[:, idx]  # [B, np, k, D]
    out.append(torch.einsum('bpjd,jdf->bpf', win, w) + b)
  return out


def _act(z, act):
  if act in (None, '', 'linear'):
    return z
  return {'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[act](z)


def text_cnn_ref(x, P, kernels, biases, act='relu', select=None):
  """-> y [B, sum F].  select = (override bool [B, sum F], weight [B, sum F, max positions], active bool [B, sum F]):
  where override, y = active * sum_p weight_p pre_p (the gradient reaches exactly the given positions, through the
  ReLU only where `active`)."""
  pres = text_cnn_pre(x, P, kernels, biases)
  ys, c0 = [], 0
  for pre in pres:
    y = _act(pre, act).amax(dim=1)  # [B, F]
    F, n_pos = pre.shape[2], pre.shape[1]
    if select is not None:
      over, weight, active = select
      w = weight[:, c0:c0 + F, :n_pos].transpose(1, 2)  # [B, np, F]
      forced = (w * pre).sum(dim=1) * active[:, c0:c0 + F].to(pre.dtype)
      y = torch.where(over[:, c0:c0 + F], forced, y)
    ys.append(y)
    c0 += F
  return torch.cat(ys, dim=-1)


def near_ties(x, P, kernels, biases, act, tol):
  """bool [B, sum F]: outputs whose fp64 top two window values, or whose maximum and 0 under relu, lie within tol.  Under
  relu an output whose windows all lie below -tol is 0 with no gradient under any selection: not a near tie."""
  out = []
  for pre in text_cnn_pre(x, P, kernels, biases):
    if pre.shape[1] > 1:
      top = pre.topk(2, dim=1).values
      near = (top[:, 0] - top[:, 1]) <= tol
    else:
      near = torch.zeros(pre.shape[0], pre.shape[2], dtype=torch.bool)
    if act == 'relu':
      m = pre.amax(dim=1)
      near = (near | (m.abs() <= tol)) & (m >= -tol)
    out.append(near)
  return torch.cat(out, dim=-1)


def seq_attn_pool_ref(x, lens, w):
  """x [B, L, D], lens [B], w [D] or [D, 1] -> [B, D]; a masked logit is the constant (no gradient to <x_t, w> there)."""
  logits = (x * w.reshape(-1)).sum(dim=-1)
  mask = torch.arange(x.shape[1])[None, :] < lens.to(torch.int64)[:, None]
  logits = torch.where(mask, logits, torch.full_like(logits, MASKED_LOGIT))
  p = torch.softmax(logits, dim=-1)
  return (p[:, :, None] * x).sum(dim=1)


class SeqCombinerOracle(OracleTrainer):

  def __init__(self, cfg, *args, **kwargs):
    cfg = copy.deepcopy(cfg)
    self._text_cnn_blocks = {}
    for blk in cfg.model_config.backbone.blocks:
      if blk.WhichOneof('layer') == 'keras_layer' and blk.keras_layer.class_name == 'TextCNN':
        self._text_cnn_blocks[blk.name] = copy.deepcopy(blk.keras_layer.text_cnn)
        blk.keras_layer.class_name = 'Dense'
    self._conv_uid = 0
    super(SeqCombinerOracle, self).__init__(cfg, *args, **kwargs)

  def forward(self, batch):
    self._conv_uid = 0
    return super(SeqCombinerOracle, self).forward(batch)

  def _text_cnn(self, V, seq, pb, name, l2):
    sizes = [int(k) for k in pb.filter_sizes]
    ks, bs = [], []
    for _ in sizes:
      cname = 'conv1d' if self._conv_uid == 0 else 'conv1d_%d' % self._conv_uid
      self._conv_uid += 1
      ks.append(V.get('%s/%s/kernel' % (name, cname)))
      bs.append(V.get('%s/%s/bias' % (name, cname)))
    net = text_cnn_ref(seq, int(pb.pad_sequence_length), ks, bs, pb.activation)
    if pb.HasField('mlp'):
      net = self._keras_mlp(V, net, pb.mlp, name + '/mlp', l2)
    return net

  def _standard_keras(self, V, x, kl, name):
    if name in self._text_cnn_blocks:
      seq = x[0]
      seq = seq[0] if isinstance(seq, (list, tuple)) else seq
      return self._text_cnn(V, seq, self._text_cnn_blocks[name], name, self.cfg.model_config.model_params.l2_regularization)
    return super(SeqCombinerOracle, self)._standard_keras(V, x, kl, name)

  def input_layer(self, V, batch, group_name, scope, wide_dim=None, only=None):
    group = [g for g in self.cfg.model_config.feature_groups if g.group_name == group_name][0]
    seq_names = [n for n in group.feature_names
                 if n in self.fc_by_name and self.fc_by_name[n].feature_type == self.fc_by_name[n].SequenceFeature]
    if only is not None or not seq_names:
      return super(SeqCombinerOracle, self).input_layer(V, batch, group_name, scope, wide_dim, only)
    plain = [n for n in group.feature_names if n not in seq_names]
    feats = []
    if plain:
      _, feats = super(SeqCombinerOracle, self).input_layer(V, batch, group_name, scope, wide_dim, only=plain)
    mc = self.cfg.model_config
    lam = mc.embedding_regularization
    l2 = self._l2_of(mc)
    feats = list(feats)
    for n in sorted(seq_names):  # (the columns are `<name>_embedding`: their order is the names')
      fc = self.fc_by_name[n]
      var_scope = '%s/%s_embedding' % (scope, n)
      e, lens = self._seq_lookup(V, var_scope + '/embedding_weights', batch, n)
      if lam > 0:
        self._reg = self._reg + lam * 0.5 * (e * e).sum()
      kind = fc.sequence_combiner.WhichOneof('combiner')
      if kind == 'attention':
        w = V.get(var_scope + '/attention/kernel', l2=l2)
        feats.append(seq_attn_pool_ref(e, torch.as_tensor(lens), w))
      else:
        assert kind == 'text_cnn', kind
        feats.append(self._text_cnn(V, e, fc.sequence_combiner.text_cnn, '%s/%s_embedding_text_cnn' % (var_scope, n), None))
    return torch.cat(feats, dim=1), feats
