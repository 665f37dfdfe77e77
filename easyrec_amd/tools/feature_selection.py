"""Feature ranking by variational dropout from a checkpoint of this project: the arithmetic of reference
tools/feature_selection.py (`VariationalDropoutFS`), without its plots and without rewriting fg json.

  python -m easyrec_amd.tools.feature_selection --config pipeline.config --checkpoint model.ckpt-100 --topk 10 \\
      [--output_dir out]

Reads `logit_p_<group>` (`logit_p` for the group `all`; `backbone/` in front is tried second, as the reference does)
and the groups' feature widths (the `variational_dropout` entry utils/checkpoint.py writes) from the checkpoint's tensor
bundle.  Per group the features are sorted by their mean dropout probability, ascending; the first --topk of every group
are kept, the others excluded - except the keys and history sequences of target attention, which always stay.  Prints
`group,feature,dropout_p` rows and the excluded features; with --output_dir it writes feature_dropout_ratio_<group>.csv
(the reference's file name and columns) and excluded_features.txt there instead.
"""
import argparse
import csv
import json
import os
import sys
from collections import OrderedDict

from easyrec_amd.layers.variational_dropout_layer import feature_importance
from easyrec_amd.utils import config_util, tensor_bundle


def read_importance(config, checkpoint):
  """-> {group: OrderedDict(feature -> mean dropout probability, ascending)}"""
  assert config.model_config.HasField('variational_dropout'), 'variational_dropout must be in model_config'
  embedding_wise = config.model_config.variational_dropout.embedding_wise_variational_dropout
  arrays = tensor_bundle.read_bundle(checkpoint)
  assert 'variational_dropout' in arrays, '%s holds no variational_dropout entry' % checkpoint
  dims = {('all' if name == '' else name): OrderedDict((f, int(d)) for f, d in features)
          for name, features in json.loads(arrays['variational_dropout'].tobytes().decode('utf-8'))}
  out = OrderedDict()
  for group in config.model_config.feature_groups:
    name = group.group_name
    key = 'logit_p' if name == 'all' else 'logit_p_%s' % name
    if key not in arrays:
      key = 'backbone/' + key
    out[name] = feature_importance(arrays[key], dims[name], embedding_wise)
  return out


def excluded_features(config, importance, topk):
  """reference tools/feature_selection.py:153-178"""
  excluded = set()
  for ranking in importance.values():
    excluded.update(list(ranking)[topk:])
  keep = set()
  groups = [sf for g in config.model_config.feature_groups for sf in g.sequence_features]
  for sf in groups + list(config.model_config.seq_att_groups):
    for m in sf.seq_att_map:
      keep.update(m.key)
      keep.update(m.hist_seq)
  return sorted(excluded - keep)


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--config', required=True)
  ap.add_argument('--checkpoint', required=True)
  ap.add_argument('--topk', type=int, required=True)
  ap.add_argument('--output_dir', default=None)
  args = ap.parse_args(argv)
  config = config_util.get_configs_from_pipeline_file(args.config)
  importance = read_importance(config, args.checkpoint)
  excluded = excluded_features(config, importance, args.topk)
  if args.output_dir:
    os.makedirs(args.output_dir, exist_ok=True)
  for group, ranking in importance.items():
    fout = open(os.path.join(args.output_dir, 'feature_dropout_ratio_%s.csv' % group), 'w') if args.output_dir \
        else sys.stdout
    writer = csv.writer(fout)
    writer.writerow(['feature_name', 'mean_drop_p'] if args.output_dir else ['group', 'feature_name', 'mean_drop_p'])
    for feature, p in ranking.items():
      writer.writerow([feature, p] if args.output_dir else [group, feature, p])
    if args.output_dir:
      fout.close()
  if args.output_dir:
    with open(os.path.join(args.output_dir, 'excluded_features.txt'), 'w') as fout:
      fout.write(''.join(f + '\n' for f in excluded))
  else:
    print('excluded: %s' % ','.join(excluded))
  return importance, excluded


if __name__ == '__main__':
  main()
