"""GPU (-m gpu): the initial-state and terminal kernels of the column-layout state files -- k_init_lane, k_init_rowlane, k_init_quad_tl and
k_terminal_cols<Map, FLAVOR> (csrc/jq_aux_kernels.h), one terminal kernel over a column map per layout (lane, row-lane, tangent-linear quad)
in three flavours (Stormer-Verlet with sv_type 1 .. 4, implicit midpoint, tangent-linear).  They replace one copy per kernel family and move no
floating-point operation, operand or order: tests/golden/endpoint_kernels/ holds what the build BEFORE the merge returned from public calls
(scripts/record_endpoint_kernels.py, float.hex() strings; its docstring lists the cases), and the calls must reproduce it exactly.  The
same outputs meet the CPU oracle at the tolerance of the existing test of each route: conftest.reference_pass (atol 1e-14 or rtol 1e-10)
for the Stormer-Verlet evaluations, batches and Hessian-vector products (tests/ensemble_hessian_reference.py), 1e-9 relative for the
implicit-midpoint kernels (test_gpu_imr._random_checks)."""
import importlib.util
import json
import os

import numpy as np
import pytest
from conftest import ROOT, reference_pass

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_endpoint_kernels", os.path.join(ROOT, "scripts", "record_endpoint_kernels.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def results(jq):
    """every case once on the GPU: name -> outputs"""
    cache = {}

    def get(name):
        if name not in cache:
            val, family, plan = rec.run_case(jq, name)
            assert family == rec.CASES[name][1], (name, family)
            if name == "hvp_lane_rounds":
                assert plan["ens_hvp"]["rounds"] == 3 and plan["ens_hvp"]["directions_per_launch"] == 2, plan["ens_hvp"]
            elif name.startswith("hvp"):
                assert plan["ens_hvp"]["rounds"] == 1 and plan["ens_hvp"]["route"] == {"l": "lane", "r": "rowlane", "q": "quad"}[name[4]], plan["ens_hvp"]
            cache[name] = val
        return cache[name]
    return get


def node_sum_eval(pcof, nodes, weights, shift):
    """evaluate(params) -> the weighted sums over the nodes' problems (ensemble_hessian_reference.node_params) of the oracle's traceobjgrad:
    the reference of the ensemble Hessian tests' gradients.  (Oracle.eval_f_g_grad leaves level 1 unshifted, as the reference does; the
    library and these cases shift every level.)"""
    import ensemble_hessian_reference as ER
    from oracle.oracle import Oracle
    keys = ("totalgrad", "infidelgrad", "leakgrad", "primaryobjf", "secondaryobjf")

    def ev(p):
        rs = [Oracle(ER.node_params(p, e, shift)).traceobjgrad(pcof) for e in nodes]
        return {k: sum(float(w) * np.asarray(r[k], dtype=np.float64) for w, r in zip(weights, rs)) for k in keys if np.size(rs[0][k])}
    return ev


def close(name, value, ref):
    value, ref = np.atleast_1d(np.asarray(value, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    print("    %-40s |diff| %.3e  |ref| %.3e" % (name, np.linalg.norm(value - ref), np.linalg.norm(ref)))
    assert reference_pass(value, ref), name


@pytest.mark.parametrize("name", list(rec.CASES))
def test_results_equal_the_recorded_ones_bit_for_bit(results, name):
    with open(os.path.join(ROOT, "tests", "golden", "endpoint_kernels", name + ".json")) as f:
        gold = {k: np.array([float.fromhex(x) for x in v["hex"]]).reshape(v["shape"], order="F") for k, v in json.load(f).items()}
    val = results(name)
    assert sorted(val) == sorted(gold)
    for k in gold:
        same = val[k].shape == gold[k].shape
        print("%s %s: %d of %d entries differ" % (name, k, int(np.sum(val[k] != gold[k])) if same else -1, gold[k].size))
    for k in gold:
        assert val[k].shape == gold[k].shape and np.array_equal(val[k], gold[k]), k
    grads = [gold[k] for k in gold if "grad" in k and gold[k].size]      # (objFuncType 1: the leak gradient is all zeros)
    assert all(np.all(np.isfinite(g)) for g in grads) and min(np.linalg.norm(gold[k]) for k in gold if k.startswith("infid")) > 0.0


# ---- Stormer-Verlet: sv_type 1 against the oracle, 2 .. 4 through the identities of test_gpu_svtype._check_ensemble -------------------------
@pytest.mark.parametrize("group,kind,svs", [("lane_np2", "ensemble", (1, 2, 3, 4)), ("lane_np8", "single", (1, 4)), ("rowlane_n3", "ensemble", (1, 4))])
def test_continuation_adjoints_meet_the_oracle(jq, results, group, kind, svs):
    from test_svtype_host import leak_part, oracle_eval, ref_polar
    which = rec.CASES[group + "_sv1"][2]
    params, pcof, opts, nodes, weights, shift = rec.primal_problem(jq, which)
    ev = node_sum_eval(pcof, nodes, weights, shift) if kind == "ensemble" else oracle_eval(pcof)
    r1, ell, polar = ev(params), leak_part(params, ev), ref_polar(params, ev, rec.dvds_of(params))
    assert params.objFuncType != 1 and np.linalg.norm(ell) > 0.0      # (nonzero leak weights)
    out = {}
    for sv in svs:
        v = results("%s_sv%d" % (group, sv))
        if kind == "ensemble":
            v = dict(primaryobjf=v["infidelity"], secondaryobjf=v["leak"], infidelgrad=v["infidelity_grad"], leakgrad=v["leak_grad"],
                     totalgrad=v["infidelity_grad"] + v["leak_grad"])
        out[sv] = v
        for k in ("primaryobjf", "secondaryobjf", "leakgrad"):      # taken against the target in every type
            close("%s type %d %s" % (group, sv, k), v[k], r1[k])
    close(group + " type 1 totalgrad", out[1]["totalgrad"], r1["totalgrad"])
    close(group + " type 1 infidelgrad", out[1]["infidelgrad"], r1["infidelgrad"])
    close(group + " type 4 totalgrad", out[4]["totalgrad"], polar + ell)
    close(group + " type 4 infidelgrad", out[4]["infidelgrad"], polar)
    if 2 in out:
        close(group + " types 2 + 3 totalgrad", out[2]["totalgrad"] + out[3]["totalgrad"], polar + 2.0 * ell)
        close(group + " types 2 + 3 infidelgrad", out[2]["infidelgrad"] + out[3]["infidelgrad"], polar)


def test_grouped_batch_meets_the_oracle(jq, results):
    from test_gpu_pcof_batch import check_oracle, column
    params, pcof, opts, nodes, weights, shift = rec.primal_problem(jq, "rl")
    b = results("rowlane_batch3")
    vecs = rec.batch_vectors(pcof)
    assert b["totalgrad"].shape == (pcof.size, 3)
    for i, v in enumerate(vecs):
        check_oracle("column %d" % i, params, v, column(b, i))


def test_implicit_midpoint_meets_the_oracle(jq, results):
    """the criteria of test_gpu_imr._random_checks"""
    from oracle.oracle import Oracle
    p, pcof, opts, nodes, weights, shift = rec.primal_problem(jq, "imr")
    v = results("rowlane_imr_n3")
    r = Oracle(p, use_sparse=False).traceobjgrad_imr(pcof, rec.IMR_ITER, rec.IMR_TOL)
    gn = np.linalg.norm(r["totalgrad"])
    print("imr: primary %.3e secondary %.3e totalgrad %.3e infidelgrad %.3e (|grad| %.3e)" % (
        abs(v["primaryobjf"] - r["primaryobjf"]), abs(v["secondaryobjf"] - r["secondaryobjf"]), np.linalg.norm(v["totalgrad"] - r["totalgrad"]),
        np.linalg.norm(v["infidelgrad"] - r["infidelgrad"]), gn))
    assert abs(v["primaryobjf"] - r["primaryobjf"]) <= 1e-9 and abs(v["secondaryobjf"] - r["secondaryobjf"]) <= 1e-9 * max(abs(r["secondaryobjf"]), 1e-3)
    assert np.linalg.norm(v["totalgrad"] - r["totalgrad"]) <= 1e-9 * gn and np.linalg.norm(v["infidelgrad"] - r["infidelgrad"]) <= 1e-9 * gn
    inf, g, H0 = 0.0, np.zeros(pcof.size), p.Hconst.copy()
    for ep, wq in zip(nodes, weights):
        p.Hconst = H0 + np.diag(ep * shift)
        rr = Oracle(p, use_sparse=False).traceobjgrad_imr(pcof, rec.IMR_ITER, rec.IMR_TOL)
        inf += wq * rr["primaryobjf"]
        g += wq * rr["infidelgrad"]
    p.Hconst = H0
    print("imr, 3 nodes: infidelity %.3e (of %.3e) gradient %.3e (of %.3e)" % (
        abs(v["ens_infidelity"] - inf), abs(inf), np.linalg.norm(v["ens_infidelity_grad"] - g), np.linalg.norm(g)))
    assert abs(v["ens_infidelity"] - inf) <= 1e-9 * abs(inf)
    assert np.linalg.norm(v["ens_infidelity_grad"] - g) <= 1e-9 * np.linalg.norm(g)


@pytest.mark.parametrize("name", [n for n in rec.CASES if n.startswith("hvp")])
def test_hessian_vector_products_meet_the_reference(jq, results, name):
    import ensemble_hessian_reference as ER
    from test_gpu_ens_hvp import _check_against_reference, _reference
    p, pcof, opts, nodes, weights, shift, D = rec.hvp_problem(jq, name)
    r = results(name)
    assert r["hv_infid"].shape == D.shape and r["hv_leak"].shape == D.shape
    _check_against_reference(r, _reference(p, pcof, D, nodes, weights, shift))
    tg, ig = ER.weighted_oracle_gradients(p, pcof, nodes, weights, shift)
    close(name + " total gradient", r["infid_grad"] + r["leak_grad"], tg)
    close(name + " infidelity gradient", r["infid_grad"], tg if p.objFuncType == 1 else ig)
    e = node_sum_eval(pcof, nodes, weights, shift)(p)
    close(name + " infidelity", r["infidelity"], e["primaryobjf"])
    close(name + " leak", r["leak"], e["secondaryobjf"])
