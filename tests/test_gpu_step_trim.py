"""GPU (-m gpu): the per-step trims of the three-slab quad-layout kernels (LKC, CWH, PK in csrc/jq_kernels.h: carried leak integrand,
hoisted shift table, packed early trace reductions) remove repeated work only -- the same
floating-point operations on the same values in the same order.  tests/golden/step_trim/ holds what the build BEFORE them returned
(scripts/record_step_trim.py, float.hex() strings); the kernels must reproduce it exactly.  3 072 samples each:
  a  cnot3 x 300 steps, perturbed ensemble: one chunk of even length
  b  cnot3 x 23 steps with chunk_steps=7: odd chunks and a remainder (leak carry and trace records across chunk boundaries, odd tail
     of the two-step loop)
  c  (a) with unperturbed samples (use_shift == 0)
  d  cnot3 without its third control (Ncoupled = 2 on the ORD kernels)
  e  one Hanti entry x 1.01: non-uniform S, the kernels without the compact S operand"""
import importlib.util
import json
import os

import numpy as np
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_step_trim", os.path.join(ROOT, "scripts", "record_step_trim.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.mark.parametrize("name", rec.CASES)
def test_results_equal_the_recorded_ones_bit_for_bit(jq, name):
    with open(os.path.join(ROOT, "tests", "golden", "step_trim", name + ".json")) as f:
        gold = json.load(f)
    res, t, plan = rec.run_case(jq, name)
    assert t["kernel_family"] == 6 and t["kernel_band"] == 7, t
    assert plan["s_uniform"] is (name != "e_nonuniform_s")
    print("%s: infidelity %s (recorded %s) leak %s (recorded %s)" % (name, res["infidelity"], gold["infidelity"], res["leak"], gold["leak"]))
    for key in ("infidelity_grad", "leak_grad"):
        diff = [i for i, (x, y) in enumerate(zip(res[key], gold[key])) if x != y]
        print("%s: %d of %d entries differ" % (key, len(diff), len(gold[key])))
    assert res["infidelity"] == gold["infidelity"] and res["leak"] == gold["leak"]
    assert res["infidelity_grad"] == gold["infidelity_grad"] and res["leak_grad"] == gold["leak_grad"]
    g = np.array([float.fromhex(x) for x in gold["infidelity_grad"]])
    assert g.size > 0 and np.all(np.isfinite(g)) and np.linalg.norm(g) > 0.0
