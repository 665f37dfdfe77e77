"""Uniter against the REFERENCE'S OWN run (tests/golden/uniter_vectors.npz, made by tests/golden/make_uniter_vectors.py
from the reference's layers/uniter.py, layers/multihead_cross_attention.py and model/uniter.py over the numpy stand-in):
the fp64 restatement reproduces it at 1e-9, and the product on the stand-in backend creates the reference's variables
under the reference's names and reproduces its layer output and logits."""
import numpy as np
import pytest
import torch

from easyrec_amd.core import context
from oracle import uniter_ref as ref
from tests import _uniter_cases as cases
from tests._oracle_steps import close

GOLD = cases.fixture()
CASES = sorted({k.split(':')[0] for k in GOLD.files})


def test_fixture_covers_the_cases():
  assert CASES == sorted(['all', 'image', 'text_tanh', 'nopos', 'general_hidden', 'other_plain', 'eval'])
  cfg, groups, training, inputs, var = cases.fixture_case(GOLD, 'all')
  c = cfg.model_config.uniter.config
  assert (c.hidden_size, c.num_attention_heads, c.num_hidden_layers, c.intermediate_size) == (12, 3, 2, 10)
  lens = [n.tolist() for _, n in inputs['text']]
  assert all(0 in n and 1 in n for n in lens) and 5 in lens[0] and 3 in lens[1] and len(lens[0]) == 6
  assert cases.fixture_case(GOLD, 'text_tanh')[0].model_config.uniter.config.hidden_act == 'tanh'
  assert not cases.fixture_case(GOLD, 'nopos')[0].model_config.uniter.config.use_position_embeddings
  assert 'txt_projection/kernel' not in cases.fixture_case(GOLD, 'general_hidden')[4]
  assert not any(n.startswith('other_dnn/') for n in cases.fixture_case(GOLD, 'other_plain')[4])
  assert not cases.fixture_case(GOLD, 'eval')[2]


@pytest.mark.parametrize('tag', CASES)
def test_restatement_matches_the_reference(tag):
  cfg, groups, training, inputs, var = cases.fixture_case(GOLD, tag)
  c = cfg.model_config.uniter.config
  img = inputs['image'].reshape(6, 1, -1) if 'image' in inputs else None
  gen = inputs['general'].reshape(6, 3, -1) if 'general' in inputs else None
  cls = ref.uniter_cls(var, c, img, gen, inputs.get('text', []))
  want = GOLD['%s:cls' % tag]
  assert np.abs(cls.numpy() - want).max() <= 1e-9 * np.abs(want).max(), tag


@pytest.mark.parametrize('tag', CASES)
def test_product_names_and_forward_match_the_reference(ref_backend, tag):
  """The variables the product creates are the reference's (BatchNorm's moving statistics aside: the stand-in creates
  them only where it reads them, in eval mode), in the reference's creation order; the layer output ([CLS] feature and
  `other` branch) and the logits match the reference's at 1e-5 (fp32 against fp64)."""
  cfg, groups, training, inputs, var = cases.fixture_case(GOLD, tag)
  vs, ctx, run = cases.product_fixture_forward('cpu', cfg, training, inputs, var)
  got = [n for n in vs.names() if '/moving_' not in n]
  assert got == [n for n in var if '/moving_' not in n]
  assert all(tuple(vs.state_dict()[n].shape) == tuple(var[n].shape) for n in var)
  with context.use(ctx), torch.no_grad():
    hidden, logits = run()
  close(hidden, GOLD['%s:hidden' % tag], 1e-5, (tag, 'hidden'))
  close(logits, GOLD['%s:logits' % tag], 1e-5, (tag, 'logits'))
  close(torch.sigmoid(logits), GOLD['%s:probs' % tag], 1e-5, (tag, 'probs'))
