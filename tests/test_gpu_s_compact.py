"""GPU (-m gpu): the compact S operand of the three-slab quad-layout kernels (k_forward / k_backward<NT, 7, 3, ..., SC>, option s_compact,
plan info s_uniform).  When every 16-row block of the S images repeats block 0 (tests/test_s_compact.py) the kernels fetch one A
register, one (c0, c1) pair and two lane-uniform coefficients per block instead of the five doubles per block and lane of the full
operand.  The values are the image entries the full operand reads, the FMAs / MFMAs and their order are the same: results must be
BIT-identical to s_compact=0 -- the criterion of the register-form fence (tests/test_gpu_forms.py)."""
import json
import os

import numpy as np
import pytest
from conftest import ROOT, reference_pass

pytestmark = pytest.mark.gpu


def _cnot3(jq, nsteps=None):
    params, info = jq.cases.cnot3()
    if nsteps:
        params.T, params.nsteps = params.T * nsteps / params.nsteps, nsteps
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "cnot3.json")))["pcof0"])
    return params, pcof


def _ensemble(jq, params, pcof, opts, ns=3072):
    nodes, weights, shift = jq.cases.cnot3_ensemble(ns)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    plan = wa.plan_info()
    jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
    t = wa.last_timing()
    assert t["kernel_family"] == 6 and t["kernel_band"] == 7, t      # (the benchmark's kernels: quad layout, three slabs per workgroup)
    res = (params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy(), params.last_leak_grad.copy())
    wa.close()
    return res, plan


def test_plan_info_reports_the_structure_and_the_option(jq):
    params, pcof = _cnot3(jq, 300)
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    plan = wa.plan_info()
    assert plan["structure"] == "t4" and plan["s_uniform"] is True and plan["s_compact"] == 1 and plan["options"] == ""
    wa.set_option("s_compact", 0)
    plan = wa.plan_info()
    assert plan["s_uniform"] is True and plan["s_compact"] == 0 and "s_compact=0" in plan["options"]
    wa.close()
    # one (i, i + 4) coupling of b - b' made row-dependent: still 4 x 4 x n, no longer uniform
    H = params.Hanti_ops[1]
    H[37, 33] *= 1.0 + 2.0 ** -30
    H[33, 37] = -H[37, 33]
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    plan = wa.plan_info()
    assert plan["structure"] == "t4" and plan["s_uniform"] is False and plan["s_compact"] == 1
    wa.close()


@pytest.mark.parametrize("nsteps", [300, None])
def test_compact_and_full_s_operands_agree_bit_for_bit(jq, nsteps):
    """cnot3 x 300 steps and the full-length workload bench.py times (32 386 steps), 3 072 perturbed samples each"""
    params, pcof = _cnot3(jq, nsteps)
    on, plan_on = _ensemble(jq, params, pcof, None)
    off, plan_off = _ensemble(jq, params, pcof, {"s_compact": 0})
    assert plan_on["s_uniform"] is True and plan_on["s_compact"] == 1 and plan_off["s_compact"] == 0
    print("s_compact=1: infidelity %.17g leak %.17g |grad| %.17g" % (on[0], on[1], np.linalg.norm(on[2])))
    print("s_compact=0: infidelity %.17g leak %.17g |grad| %.17g" % (off[0], off[1], np.linalg.norm(off[2])))
    assert on[0] == off[0] and on[1] == off[1]
    assert np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])
    assert np.all(np.isfinite(on[2])) and np.linalg.norm(on[2]) > 0.0


@pytest.mark.parametrize("which", ["diagonal block", "coupling +-4"])
def test_a_perturbed_problem_stays_on_the_full_image_and_meets_the_oracle(jq, which):
    """Hanti with one entry pair changed (the structure still fits 4 x 4 x n): s_uniform is false, the kernels with the full operand
    run -- with the option at its default -- and 3 072 copies of the unperturbed sample reproduce the oracle's single evaluation at the
    reference's tolerance (rtol 1e-10 / atol 1e-14)"""
    from oracle.oracle import Oracle
    params, pcof = _cnot3(jq, 300)
    # (entries between populated levels -- a guard-level entry such as (37, 33) changes the gradient by less than the tolerance in 300 steps,
    #  and the last assertion below could not tell that the perturbation reached the kernels)
    r, c, q = (21, 20, 0) if which == "diagonal block" else (4, 0, 1)
    H = params.Hanti_ops[q]
    assert H[r, c] != 0.0
    H[r, c] *= 1.01
    H[c, r] = -H[r, c]
    ref = Oracle(params).traceobjgrad(pcof)
    ns = 3072
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    plan = wa.plan_info()
    assert plan["structure"] == "t4" and plan["s_uniform"] is False and plan["s_compact"] == 1
    jq.eval_f_g_grad(pcof, params, wa, np.zeros(ns), np.full(ns, 1.0 / ns), True, shift=np.zeros(params.Ntot))
    t = wa.last_timing()
    assert t["kernel_family"] == 6 and t["kernel_band"] == 7, t
    wa.close()
    print("%s: infidelity %.17g (oracle %.17g), gradient rel diff %.2e" % (
        which, params.last_infidelity, ref["primaryobjf"],
        np.linalg.norm(params.last_infidelity_grad - ref["infidelgrad"]) / np.linalg.norm(ref["infidelgrad"])))
    assert reference_pass(params.last_infidelity, ref["primaryobjf"])
    assert reference_pass(params.last_infidelity_grad, ref["infidelgrad"])
    # ... and differs from the unperturbed problem's (the perturbation reached the kernels)
    base, _ = _cnot3(jq, 300)
    rb = Oracle(base).traceobjgrad(pcof)
    assert not reference_pass(params.last_infidelity_grad, rb["infidelgrad"])
