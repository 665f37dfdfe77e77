"""Closed-form replay of Adam decay-only steps (csrc/er_decay.h) against the fp32 step-by-step recurrence, both measured
against the fp64 recurrence: the deviation of each form's update in units of 2^-24 of the update, where var starts at 0.
Cases, reference and the float32 restatement are those of tests/_decay_cases.py (the pins in tests/test_decay_pins.py
assert them; this only prints).  Usage: python tools/decay_closed_form.py [dim]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _decay_cases as dc  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 16
for pair in sorted(dc.PAIRS):
  st, ref = dc.case_reference(pair, dim, dc.S_TOTAL)
  forms = {'closed': dc.restate(st.var, st.m, st.v, st.last, dc.S_TOTAL, pair),
           'fp32 steps': dc.restate_steps(st.var, st.m, st.v, st.last, dc.S_TOTAL, pair)}
  sel = (st.var == 0) & (ref['upd'] > 0)
  for k in sorted(set(st.k[st.k > 0].tolist())):
    rows = sel & (st.k == k)[:, None]
    dev = {n: float((np.abs(f['var'].astype(np.float64) - ref['var'])[rows] / ref['upd'][rows]).max() / dc.U)
           for n, f in forms.items()}
    print('%-6s K=%3d k=%4d  update deviation in U:  closed %8.3g   fp32 steps %8.3g' %
          (pair, dc.EXPECTED_K[pair], k, dev['closed'], dev['fp32 steps']))
