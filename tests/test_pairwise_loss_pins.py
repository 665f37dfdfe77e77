"""The pairwise ranking losses' torch compositions (easyrec_amd/builders/pairwise_loss.py), through loss_builder.build
on the CPU in fp64, against values and central-difference gradients of the reference's own loss/pairwise_loss.py and
loss/focal_loss.py (tests/golden/pairwise_loss_vectors.npz, written by tests/golden/make_pairwise_loss_vectors.py)."""
import os

import numpy as np
import pytest
import torch

from easyrec_amd.builders import loss_builder
from easyrec_amd.protos import loss_pb2

LT = loss_pb2.LossType
VEC = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pairwise_loss_vectors.npz'))

# fixture entry -> (loss type, loss_param, per-example weights?); a session_name in the param: the fixture's session keys
CASES = {
    'pair_wise_s': (LT.PAIR_WISE_LOSS, loss_pb2.PairwiseLoss(session_name='u'), False),
    'pair_wise_s_w_mt': (LT.PAIR_WISE_LOSS, loss_pb2.PairwiseLoss(session_name='u', margin=0.25, temperature=2.0), True),
    'logistic': (LT.PAIRWISE_LOGISTIC_LOSS, None, False),
    'logistic_s_w_hinge': (LT.PAIRWISE_LOGISTIC_LOSS,
                           loss_pb2.PairwiseLogisticLoss(session_name='u', hinge_margin=0.5, temperature=0.5), True),
    'logistic_s_label_margin': (LT.PAIRWISE_LOGISTIC_LOSS,
                                loss_pb2.PairwiseLogisticLoss(session_name='u', use_label_margin=True, temperature=2.0), False),
    'logistic_ohem': (LT.PAIRWISE_LOGISTIC_LOSS, loss_pb2.PairwiseLogisticLoss(ohem_ratio=0.5), True),
    'hinge': (LT.PAIRWISE_HINGE_LOSS, None, False),
    'hinge_s_w': (LT.PAIRWISE_HINGE_LOSS, loss_pb2.PairwiseHingeLoss(session_name='u', temperature=2.0), True),
    'hinge_s_margin': (LT.PAIRWISE_HINGE_LOSS,
                       loss_pb2.PairwiseHingeLoss(session_name='u', use_label_margin=False, margin=0.75, label_is_logits=False,
                                                  temperature=0.5), False),
    'hinge_ohem': (LT.PAIRWISE_HINGE_LOSS, loss_pb2.PairwiseHingeLoss(session_name='u', ohem_ratio=0.3), False),
    'focal': (LT.PAIRWISE_FOCAL_LOSS, None, False),
    'focal_s_w': (LT.PAIRWISE_FOCAL_LOSS,
                  loss_pb2.PairwiseFocalLoss(session_name='u', gamma=1.5, alpha=0.25, temperature=2.0), True),
    'focal_s_hinge': (LT.PAIRWISE_FOCAL_LOSS, loss_pb2.PairwiseFocalLoss(session_name='u', hinge_margin=1.0, gamma=2.0), False),
    'focal_ohem': (LT.PAIRWISE_FOCAL_LOSS, loss_pb2.PairwiseFocalLoss(ohem_ratio=0.5, gamma=3.0), True),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_composition_matches_the_reference(name):
  loss_type, param, weighted = CASES[name]
  keys = torch.from_numpy(VEC['sessions']) if param is not None and param.session_name else None
  weight = torch.from_numpy(VEC['weights']) if weighted else 1.0
  loss, dz = loss_builder.build(loss_type, torch.from_numpy(VEC['labels']), torch.from_numpy(VEC['logits']), weight,
                                loss_param=param, session_ids=keys)
  assert abs(float(loss) - float(VEC[name])) <= 1e-12 * max(1.0, abs(float(VEC[name])))
  # (central differences at h = 1e-6 of an fp64 forward: ~1e-9 absolute)
  assert float(np.abs(dz.numpy() - VEC[name + '_grad']).max()) <= 1e-7


def test_scalar_weight_scales_and_exponent_hinge_is_refused():
  y, z = torch.from_numpy(VEC['labels']), torch.from_numpy(VEC['logits'])
  loss, dz = loss_builder.build(LT.PAIRWISE_FOCAL_LOSS, y, z, 2.0, loss_scale=0.5)
  assert abs(float(loss) - float(VEC['focal'])) <= 1e-12
  assert float(np.abs(dz.numpy() - VEC['focal_grad']).max()) <= 1e-7
  with pytest.raises(NotImplementedError, match='use_exponent'):
    loss_builder.build(LT.PAIRWISE_HINGE_LOSS, y, z, loss_param=loss_pb2.PairwiseHingeLoss(use_exponent=True))
