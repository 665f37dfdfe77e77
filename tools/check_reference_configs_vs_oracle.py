"""For every config the reference ships that builds here: two training steps of the product (host code on the oracle's
stand-in kernels) against the model oracle, on the same synthetic batches - loss by loss.  Tables are capped at 2000
rows, and the dropout probabilities of the Uniter and CMBF layers are set to 0: dropout is random on both sides, the
oracle refuses it.  negative_sampler_in_memory gets its item table; no reference config with the weighted
negative_sampler builds here (their item tables are files the reference does not ship), so that branch has nothing to
pass.  Run where /root/reference exists.  usage: python tools/check_reference_configs_vs_oracle.py [/root/reference] [-v]"""
import collections
import glob
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
logging.disable(logging.CRITICAL)
REF = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith('-') else '/root/reference'


def main():
  from easyrec_amd import kernels
  from easyrec_amd.input.synthetic import SyntheticBatches
  from easyrec_amd.model.easy_rec_estimator import EasyRecEstimator
  from easyrec_amd.utils import config_util
  from oracle.kernel_ref import RefBackend
  from oracle.model_oracle import OracleTrainer
  kernels._BACKEND = RefBackend()
  files = sorted(glob.glob(REF + '/samples/model_config/*.config') + glob.glob(REF + '/examples/configs/*.config'))
  agree, differ, no_product, no_oracle = [], [], 0, collections.Counter()
  for f in files:
    name = os.path.basename(f)
    try:
      cfg = config_util.get_configs_from_pipeline_file(f)
      for fc in list(cfg.feature_config.features) + list(cfg.feature_configs):
        fc.hash_bucket_size = min(fc.hash_bucket_size, 2000) if fc.HasField('hash_bucket_size') else fc.hash_bucket_size
        if fc.num_buckets > 2000:
          fc.num_buckets = 2000
      model = cfg.model_config.WhichOneof('model')
      mc = cfg.model_config
      towers = {'uniter': [mc.uniter.config], 'cmbf': [mc.cmbf.config],
                'dbmtl': [mc.dbmtl.bottom_uniter] if mc.dbmtl.HasField('bottom_uniter') else []}.get(model, [])
      for tower in towers:
        for field in ('hidden_dropout_prob', 'attention_probs_dropout_prob', 'text_seq_emb_dropout_prob'):
          if hasattr(tower, field):
            setattr(tower, field, 0.0)
      table = None
      if cfg.data_config.WhichOneof('sampler') == 'negative_sampler_in_memory':
        from easyrec_amd.input.neg_sampler import ItemTable
        table = ItemTable.load(cfg.data_config, list(cfg.feature_configs) or list(cfg.feature_config.features))
      est = EasyRecEstimator(cfg, device='cpu', batch_size=16, seed=1, item_table=table).build()
      gen = SyntheticBatches(cfg.data_config, est.feature_configs, batch_size=16, seed=2)
      batches = [gen.next_batch() for _ in range(2)]
      state = est.state_dict()
    except BaseException:  # noqa
      no_product += 1
      continue
    try:
      orc = OracleTrainer(cfg, state, batch_size=16, item_table=table, sampler_seed=1)
      worst = 0.0
      for b in batches:
        est.train_step(b)
        capsule = getattr(est.model, '_capsule_layer', None)
        if capsule is not None:  # MIND: the oracle runs the step on the routing logits the product drew
          orc.routing_logits = capsule.last_routing_logits.detach().cpu().numpy()
        got, exp = est.loss_values(), orc.train_step(b)
        assert sorted(got) == sorted(exp), (sorted(got), sorted(exp))
        worst = max(worst, max(abs(got[k] - exp[k]) / max(1.0, abs(exp[k])) for k in exp))
      (agree if worst <= 1e-4 else differ).append((name, worst))
    except BaseException as e:  # noqa
      no_oracle['%s: %s' % (type(e).__name__, str(e).split('\n')[0][:90])] += 1
      if '-v' in sys.argv:
        print('  (oracle) %s: %s: %s' % (name, type(e).__name__, str(e).split('\n')[0][:120]))
  print('%d configs; %d do not build in the product; of the %d that do: %d agree with the oracle over 2 steps (1e-4), '
        '%d differ, %d the oracle does not restate' % (len(files), no_product, len(files) - no_product, len(agree), len(differ),
                                                       sum(no_oracle.values())))
  for name, w in differ:
    print('  DIFFER %-60s %.3g' % (name, w))
  for msg, n in no_oracle.most_common(12):
    print('  oracle: %3d  %s' % (n, msg))


if __name__ == '__main__':
  main()
