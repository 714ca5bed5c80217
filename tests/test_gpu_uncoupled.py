"""GPU (-m gpu): uncoupled controls (Hunc_ops, the lab-frame evaluation of a pulse) on every kernel family against the CPU oracle.  Before
this matrix a problem with Nunc > 0 ran at one shape only (cases.cnot2_lab: Ntot 9, the row-lane family).  Every cell of
tests/uncoupled_problem.py (its completeness and the discrimination of its references: tests/test_uncoupled_matrix.py) converts a problem
of the existing generators (to_uncoupled: Hunc_ops[q] = Hsym_ops[q] or Hanti_ops[q], random Rfreq) and runs it with the options of the
route: 7 time steps in one chunk and in chunks of 3 + 3 + 1 (the split cooperative-quad sweep, whose first chunk must exceed its
8-slot ring: 11 steps in one chunk and in chunks of 9 + 2), objFuncType rotating over 1 / 2 / 3,
objective, infidelity, leak and all three gradients under the reference's criterion (conftest.reference_pass; nothing else), the
per-step history at 1e-11, a ragged ensemble with a shift, and the instantiation it ran on (family / size / band / variant of
jq_last_timing; jq_plan_info "last_kernels" where the source matrix has a record).  Implicit-midpoint cells: forward evaluations against
the oracle under exception (i) of DESIGN section 2; the gradient is JQ_EUNSUPPORTED and leaves the handle as it was.  Beyond single
calls: grouped control-vector and drift batches, the embedded twin, and a re-plan after jq_update_hconst."""
import copy

import numpy as np
import pytest
from conftest import ATOL, reference_pass

import block_band_matrix as B
import uncoupled_problem as U

pytestmark = pytest.mark.gpu
WORST = {"sv": (0.0, None), "imr": (0.0, None)}


def _err(v, w):
    """the relative difference that reference_pass compares with rtol (reported also where the absolute criterion already passes)"""
    v, w = np.atleast_1d(np.asarray(v, dtype=np.float64)), np.atleast_1d(np.asarray(w, dtype=np.float64))
    d, nrm = np.linalg.norm(v - w), np.linalg.norm(w)
    return d / nrm if nrm >= ATOL else 0.0 if d < ATOL else float("inf")


def _note(kind, name, e):
    if e > WORST[kind][0]:
        WORST[kind] = (e, name)


def _check(cell, out, ref):
    r, worst = ref["single"], 0.0
    pairs = []
    for objfv, prim, sec, tg, ig, lg in out["evals"]:
        pairs += [("objective", objfv, r["objfv"]), ("infidelity", prim, r["primaryobjf"]), ("leak", sec, r["secondaryobjf"]),
                  ("totalgrad", tg, r["totalgrad"]), ("infidelgrad", ig, r["infidelgrad"])]
        if cell.oft != 1:      # (objFuncType 1 has no leak gradient: the reference returns an empty vector)
            pairs.append(("leakgrad", lg, r["leakgrad"]))
    e = ref["ensemble"]
    names = ("last_infidelity", "last_leak", "last_infidelity_grad") + (("last_leak_grad",) if cell.oft != 1 else ())
    pairs += [(n, v, e[n]) for n, v in zip(names, out["ensemble"])]
    for _, v, w in pairs:
        worst = max(worst, _err(v, w))
    print("%s kinds %s objFuncType %d timing %s: worst relative error %.2e" % (cell.name, cell.kinds, cell.oft, out["timing"], worst))
    for name, v, w in pairs:
        assert reference_pass(v, w), (cell.name, name, v, w)
    _note("sv", cell.name, worst)


@pytest.mark.parametrize("cell", U.SV_CELLS, ids=[c.name for c in U.SV_CELLS])
def test_cell_matches_oracle_on_its_instantiation(jq, cell):
    if cell.name in U.REFUSED:      # the table says the plan refuses this combination: it must, with this message
        from juqbox_jl_amd import _lib
        with pytest.raises(_lib.JuqboxHipError) as e:
            U.run_cell(jq, cell)
        assert e.value.code == _lib.JQ_EUNSUPPORTED and U.REFUSED[cell.name] in str(e.value)
        return
    out = U.run_cell(jq, cell)      # (asserts the timing record and the last_kernels record after every gradient evaluation)
    ref = U.reference(jq, cell, out["ns"])
    assert len(out["evals"]) == len(cell.chunks)
    _check(cell, out, ref)
    assert np.max(np.abs(out["history"] - ref["single"]["history"])) < U.HISTORY_ATOL
    for alt, variant in cell.alts:      # option sets that promise the same bits
        other = U.run_cell(jq, cell, opts=alt, check=False)
        assert other["timing"] == cell.timing[:3] + (variant,), (alt, other["timing"])
        a, b = B.exact(out), B.exact(other)
        assert a == b, (alt, [k for k in a if a[k] != b[k]])


@pytest.mark.parametrize("cell", U.IMR_CELLS, ids=[c.name for c in U.IMR_CELLS])
def test_implicit_midpoint_cell_serves_the_forward_evaluation_and_refuses_the_gradient(jq, cell):
    from juqbox_jl_amd import _lib
    out = U.run_imr_cell(jq, cell)      # (asserts the timing / last_kernels record and that the refusal leaves the next evaluation bit-identical)
    r = U.reference(jq, cell, U.samples(cell))["single"]
    objfv, prim, sec = out["objective"]
    # exception (i) of DESIGN section 2: both fixed-point iterations stop at tau = 1e-11; 1e-9
    errs = (abs(objfv - r["objfv"]) / abs(r["objfv"]), abs(prim - r["primaryobjf"]), abs(sec - r["secondaryobjf"]) / max(abs(r["secondaryobjf"]), 1e-3))
    print("%s kinds %s objFuncType %d: errors %s" % (cell.name, cell.kinds, cell.oft, errs))
    assert max(errs) <= 1e-9, errs
    assert np.max(np.abs(out["history"] - r["history"])) <= 1e-9
    _note("imr", cell.name, max(errs))
    assert out["refusal"] is not None and out["refusal"][0] == _lib.JQ_EUNSUPPORTED and U.IMR_REFUSAL in out["refusal"][1], out["refusal"]


def _columns(res, i):
    """column i of a batch call's result in the order of a single call's"""
    objfv, tg, prim, sec, tinf, ig, lg = res
    return (objfv[i], tg[:, i], prim[i], sec[i], tinf[i], ig[:, i]) + ((lg[:, i],) if lg.shape[0] else ())


@pytest.mark.parametrize("name,family", [("rowlane-Ntot10", 3), ("t4-cq1-ord-m3-NT2", 8)])
def test_grouped_batches_of_control_vectors_and_of_drifts(jq, name, family):
    """jq_traceobjgrad_batch (3 vectors) and jq_traceobjgrad_drifts (3 members), grouped: per column bit-identical to the single call on the
    same variant (family 8: cq3=0, one workgroup per column quad) and within the reference's criterion of the oracle"""
    from oracle.oracle import Oracle
    cell = U.BY_NAME[name]
    pr = U.problem(jq, cell)
    p, pcof = copy.copy(pr.p), pr.pcof
    rng = np.random.default_rng(cell.seed + 5)
    P = np.stack([pcof, pcof + 0.05 * rng.standard_normal(pcof.size), 0.3 * rng.standard_normal(pcof.size)], axis=1)
    H0 = p.Hconst.copy()
    drifts = [H0 + np.diag(0.05 * rng.standard_normal(p.Ntot)) for _ in range(3)]      # (diagonal: every structure stays)
    keys = ("objfv", "totalgrad", "primaryobjf", "secondaryobjf", "traceInfidelity", "infidelgrad") + (("leakgrad",) if p.objFuncType != 1 else ())
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=dict(cell.opts))
    try:
        res = jq.traceobjgrad_batch(P, p, wa)
        info = wa.plan_info()["pcof_batch"]
        assert info["mode"] == "grouped" and info["family"] == family and wa.last_timing()["kernel_family"] == family, info
        for i in range(3):
            single = jq.traceobjgrad(P[:, i], p, wa, False, True)
            assert wa.last_timing()["kernel_family"] == family
            for a, b in zip(_columns(res, i), single):
                assert np.array_equal(a, b)
            r = Oracle(p, use_sparse=U.sparse_oracle(cell)).traceobjgrad(P[:, i])
            for k, v in zip(keys, _columns(res, i)):
                assert reference_pass(v, r[k]), (i, k, v, r[k])
        res = jq.traceobjgrad_drifts(pcof, p, wa, drifts)
        info = wa.plan_info()["drift_batch"]
        assert info["mode"] == "grouped" and info["family"] == family and wa.last_timing()["kernel_family"] == family, info
        for i in range(3):
            p.Hconst = drifts[i]
            single = jq.traceobjgrad(pcof, p, wa, False, True)
            for a, b in zip(_columns(res, i), single):
                assert np.array_equal(a, b)
            r = Oracle(p, use_sparse=U.sparse_oracle(cell)).traceobjgrad(pcof)
            for k, v in zip(keys, _columns(res, i)):
                assert reference_pass(v, r[k]), (i, k, v, r[k])
    finally:
        wa.close()


def _against_oracle(jq, p, pcof, wa):
    from oracle.oracle import Oracle
    r = Oracle(p).traceobjgrad(pcof)
    objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, p, wa, False, True)
    for k, v in (("objfv", objfv), ("primaryobjf", prim), ("secondaryobjf", sec), ("totalgrad", tg), ("infidelgrad", ig)) + ((("leakgrad", lg),) if p.objFuncType != 1 else ()):
        assert reference_pass(v, r[k]), (k, v, r[k])


def test_cnot2_lab_runs_through_the_embedded_twin(jq):
    """cases.cnot2_lab is 3 x 3 levels: padded to 4 x 4 it is one 16-row block of the JQ_BW_T4 structure; embed=2 sends every batch to
    the twin, which try_embed hands the rotation frequencies (20 steps)"""
    p, info = jq.cases.cnot2_lab(Pmin=40)
    pcof = info["pcof0"]
    nfull = p.nsteps
    p.nsteps, p.T = 20, p.T * 20 / nfull
    assert p.Nunc == 2 and p.Ntot == 9
    for oft in (1, 3):
        p.objFuncType = oft
        wa = jq.Working_Arrays_HIP(p, pcof.size, options={"embed": 2})
        try:
            assert wa.plan_info()["embedded_twin_Ntot"] == 16
            _against_oracle(jq, p, pcof, wa)
            t = wa.last_timing()
            assert (t["kernel_family"], t["kernel_band"], t["kernel_size"]) == (6, 7, 1), t
        finally:
            wa.close()


def test_update_hconst_replans_an_uncoupled_handle_and_back(jq):
    """a drift outside the 4 x 4 x n structure re-plans the handle (jq_update_hconst uploads Rfreq to the new handle); the old drift
    brings the structure back: the oracle's numbers each time"""
    cell = U.BY_NAME["t4-cq1-ord-m3-NT2"]
    pr = U.problem(jq, cell)
    p, pcof = copy.copy(pr.p), pr.pcof
    H0 = p.Hconst.copy()
    D = np.random.default_rng(cell.seed + 9).standard_normal(H0.shape)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        _against_oracle(jq, p, pcof, wa)
        assert wa.plan_info()["structure"] == "t4" and wa.plan_info()["replanned"] is False and wa.last_timing()["kernel_family"] == 8
        p.Hconst = H0 + 0.02 * (D + D.T)
        _against_oracle(jq, p, pcof, wa)
        assert wa.plan_info()["replanned"] is True and wa.plan_info()["structure"] == "dense"
        p.Hconst = H0
        _against_oracle(jq, p, pcof, wa)
        assert wa.plan_info()["structure"] == "t4" and wa.last_timing()["kernel_family"] == 8      # (the plan of the first evaluation is back)
    finally:
        wa.close()


def test_no_cell_is_skipped_and_the_worst_errors_are_on_record():
    assert len(U.SV_CELLS) + len(U.IMR_CELLS) == len(U.CELLS) and not U.REFUSED
    print("uncoupled matrix: %d cells (%d implicit midpoint); worst relative error against the oracle %.2e (%s), implicit midpoint %.2e (%s)" %
          (len(U.CELLS), len(U.IMR_CELLS), WORST["sv"][0], WORST["sv"][1], WORST["imr"][0], WORST["imr"][1]))
