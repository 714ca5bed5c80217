"""GPU (-m gpu): the Horner chain of the three-slab quad-layout kernels (k_forward / k_backward<6, 7, 3, ..., SC>, horner_add in
csrc/jq_kernels.h) runs its odd product in front of the pair loop and ends in ONE final product for every m (m = 1 included, which
used to be a product of its own on the LDS operand).  That removes register copies and branches, and moves no floating-point
operation, operand or order -- nor do the other changes around the products that profiles/sweep_fetch_ab.txt measured (table entries
held in registers, other waits).  tests/golden/sweep_fetch/ holds what the build BEFORE the change returned
(scripts/record_sweep_fetch.py, float.hex() strings); the kernels must reproduce it exactly, and meet the CPU oracle
at the reference's tolerance (rtol 1e-10 / atol 1e-14).  3 072 samples each (eight distinct nodes); steps eight times as long as
cnot3's and 300 times its control amplitudes, so that every Neumann term up to the eighth changes the result.  The cases
tests/golden/step_trim/ does not reach:
  m1 ... m7     1, 2, 3, 5, 6, 7 Neumann terms: the final product alone, no pair loop, both parities in front of the pair loop
  odd_chunk     one chunk of 151 steps, m = 5
  short_chunks  41 steps in chunks of 3: shorter than the operator ring's five time points
  two_controls  cnot3 without its third control, m = 5
  no_shift      unperturbed samples (use_shift == 0), m = 3"""
import importlib.util
import json
import os

import numpy as np
import pytest
from conftest import ROOT, reference_pass

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_sweep_fetch", os.path.join(ROOT, "scripts", "record_sweep_fetch.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

KEYS = ("infidelity", "leak", "infidelity_grad", "leak_grad")


def _values(res):
    return {k: np.array([float.fromhex(x) for x in np.atleast_1d(res[k])]) for k in KEYS}


@pytest.fixture(scope="module")
def results(jq):
    """every case once on the GPU: name -> (values, timing, plan)"""
    cache = {}

    def get(name):
        if name not in cache:
            res, t, plan = rec.run_case(jq, name)
            cache[name] = (_values(res), t, plan)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(rec.CASES))
def test_results_equal_the_recorded_ones_bit_for_bit(results, name):
    with open(os.path.join(ROOT, "tests", "golden", "sweep_fetch", name + ".json")) as f:
        gold = _values(json.load(f))
    val, t, plan = results(name)
    assert t["kernel_family"] == 6 and t["kernel_band"] == 7, t
    assert plan["s_uniform"] is True
    for k in KEYS:
        print("%s %s: %d of %d entries differ, first %s (recorded %s)" % (
            name, k, int(np.sum(val[k] != gold[k])) if val[k].shape == gold[k].shape else -1, gold[k].size,
            val[k][:1].tolist(), gold[k][:1].tolist()))
    for k in KEYS:
        assert np.array_equal(val[k], gold[k]), k
    g = gold["infidelity_grad"]
    assert g.size > 0 and np.all(np.isfinite(g)) and np.linalg.norm(g) > 0.0


@pytest.mark.parametrize("name", list(rec.CASES))
def test_results_meet_the_oracle(jq, results, name):
    from oracle.oracle import Oracle
    params, pcof, nodes, weights, shift = rec.oracle_inputs(jq, name)
    ref = Oracle(params).eval_f_g_grad(pcof, nodes, weights, shift)
    val, t, plan = results(name)
    # (objFuncType 1 keeps no leak gradient: params.last_leak_grad is empty then, as in the reference)
    keys = [k for k in KEYS if val[k].size > 0]
    assert keys[:3] == list(KEYS[:3])
    for k in keys:
        r = np.atleast_1d(ref["last_" + k])
        print("%s %s: |diff| %.3e |oracle| %.3e" % (name, k, np.linalg.norm(val[k] - r), np.linalg.norm(r)))
    for k in keys:
        assert reference_pass(val[k], ref["last_" + k]), k
