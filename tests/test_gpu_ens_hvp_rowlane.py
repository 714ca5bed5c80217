"""GPU (-m gpu): jq_eval_f_g_grad_hvp on the row-lane route -- Hessian-vector products of a risk-neutral ensemble at Ntot 9 .. 16 on the
tangent-linear row-lane kernels (k_init_rowlane, k_forward_rowlane_tl, k_terminal_cols<RowlaneMap, EP_TL>, k_backward_rowlane_tl; NPJ 12 / 16),
against the CPU reference of tests/ensemble_hessian_reference.py.

Random dense problems from the generator of the block-band tests at one tile row, 7 time steps, where a row-lane kernel can go wrong:
both row lengths full and zero-padded (Ntot 9, 12 on NPJ 12; 13, 16 on NPJ 16), N 2 / 3 / 4, one node (a half-empty wave), 3 nodes x
N 3 = 9 columns (three waves, samples straddle waves), 23 nodes x N 3 = 69 columns (18 waves, the last one holds one column), 1 / 2 / 4
controls, Neumann order 0 / 1 / 4, one chunk and chunks of 3 + 3 + 1 (state, both adjoints, the carries and their tangents cross chunk
boundaries), 1 and 5 directions, objFuncType 1 / 2 / 3, the default shift and a given one.  The default shift table reaches 1e12 at
Ntot 16, where the explicit K-part of the scheme is unstable with nodes of size 0.05: the default-shift cases scale their nodes by
10^-(Ntot - 4) (max |eps shift| ~ 0.06, the size of the given-shift cases), and the CPU reference alone shows that the nodes still
change hv_infid by more than 1e-6 relative, so a dropped shift cannot pass.

Criterion: the project's reference_pass (atol 1e-14 or rtol 1e-10) on every column of hv_infid and hv_leak; out2 and the gradients
against eval_f_g_grad on the same handle; a direction of a 5-direction call and directions in rounds bit-identical to the direction alone
/ one launch; jq_eval_f_g_grad and jq_traceobjgrad_hvp the same bits before and after; option lane=0 and five controls stay on the
sequential route."""
import numpy as np
import pytest
from conftest import case_inputs, reference_pass

import ensemble_hessian_reference as ER
from block_band_problem import block_band_problem
from test_gpu_ens_hvp import SAME_BITS, Case, _check_against_reference, _check_primal, _id, _options, _reference, _total_gradient
from test_gpu_hvp import _directions

pytestmark = pytest.mark.gpu

NSTEPS = 7
KF_ROWLANE, KF_COOP = 3, 1
ROWLANE_CASES = (
    Case(9, 2, 1, 4, 0, 5, 1, 1, "default"),       # NPJ 12 zero padded, one node: a half-empty wave
    Case(9, 3, 2, 0, 3, 1, 3, 3, "given"),         # 9 columns = 3 waves, samples straddle waves, no Neumann terms, chunks, unforced pass
    Case(12, 4, 4, 1, 0, 5, 2, 3, "default"),      # NPJ 12 full, four controls
    Case(12, 3, 1, 1, 3, 5, 2, 23, "given"),       # 69 columns = 18 waves, the last wave one column
    Case(13, 2, 2, 4, 0, 1, 1, 1, "given"),        # NPJ 16 zero padded
    Case(13, 4, 1, 4, 3, 5, 3, 3, "default"),      # NPJ 16 zero padded, chunks, objFuncType 3
    Case(16, 3, 2, 1, 0, 1, 1, 23, "given"),       # NPJ 16 full
    Case(16, 4, 4, 4, 3, 5, 3, 3, "given"),        # everything at once
)
EVERYTHING = (ROWLANE_CASES[2], ROWLANE_CASES[7])      # the 12- and the 16-level case with four controls and five directions


def _npj(Ntot):
    return 12 if Ntot <= 12 else 16


def _problem(jq, c):
    rng = np.random.default_rng(91000 + 1000 * c.Ntot + 100 * c.N + 10 * c.Nc + c.m)
    p, pcof = block_band_problem(jq, rng, c.Ntot, c.N, 0, [1] * c.Nc, NSTEPS, c.m, c.objFuncType)
    if c.nquad == 1:
        nodes, weights = np.zeros(1), np.ones(1)
    else:
        nodes = 0.05 * np.linspace(-1.0, 1.0, c.nquad) + 0.01 * rng.standard_normal(c.nquad)
        weights = rng.random(c.nquad) + 0.1
        weights /= weights.sum()
    shift = None if c.shift == "default" else rng.standard_normal(c.Ntot)
    if shift is None:
        nodes = nodes * 10.0 ** -(c.Ntot - 4)
    return p, pcof, rng, nodes, weights, shift


_cache = {}


def _set_up(jq, c):
    """problem, directions and CPU reference of a case, computed once and shared (never modified) by the tests that use the case"""
    if c not in _cache:
        p, pcof, rng, nodes, weights, shift = _problem(jq, c)
        D = _directions(rng, _total_gradient(p, pcof, nodes, weights, shift), pcof.size, c.ndir)
        refs = _reference(p, pcof, D, nodes, weights, shift)
        for t in refs:
            assert np.isfinite(t["hv_infid"]).all() and np.isfinite(t["hv_leak"]).all()
        _cache[c] = (p, pcof, nodes, weights, shift, D, refs)
    return _cache[c]


@pytest.mark.parametrize("c", ROWLANE_CASES, ids=[_id(c) for c in ROWLANE_CASES])
def test_rowlane_route_matches_reference(jq, c):
    p, pcof, nodes, weights, shift, D, refs = _set_up(jq, c)
    if c.nquad > 1:      # the CPU reference alone: the nodes matter (a kernel that dropped the shift would compute the eps = 0 ensemble)
        flat = ER.EnsembleHessianReference(p, np.zeros(c.nquad), weights, shift).hvp(pcof, D[:, 0])["hv_infid"]
        effect = np.linalg.norm(refs[0]["hv_infid"] - flat) / np.linalg.norm(refs[0]["hv_infid"])
        print("node effect on hv_infid[:, 0]: %.2e relative, |hv| %.2e" % (effect, np.linalg.norm(refs[0]["hv_infid"])))
        assert effect > 1e-6
    NPJ = _npj(c.Ntot)
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=_options(c))
    try:
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift)
        assert r["hv_infid"].shape == (pcof.size, c.ndir) and r["hv_leak"].shape == (pcof.size, c.ndir)
        plan = wa.plan_info()
        assert plan["ens_hvp"] == {"route": "rowlane", "directions_per_launch": c.ndir, "chunk_steps": c.chunk or NSTEPS, "rounds": 1}
        assert plan["last_kernels"]["object"] == "r_%d" % NPJ and plan["last_kernels"]["forward_object"] == "r_%d" % NPJ
        t = wa.last_timing()
        nchunks, npass = (3 if c.chunk else 1), (2 if c.objFuncType != 1 else 1)
        assert (t["kernel_family"], t["kernel_size"], t["kernel_band"]) == (KF_ROWLANE, NPJ, 0)
        assert t["n_forward_launches"] == nchunks and t["n_backward_launches"] == nchunks * npass
        _check_against_reference(r, refs)
        _check_primal(jq, r, pcof, p, wa, nodes, weights, shift)
        if c.ndir == 5:
            for j in (1, 4):      # a direction alone: the same operations in the same order
                one = jq.eval_f_g_grad_hvp(pcof, D[:, j], p, wa, nodes, weights, shift)
                assert wa.plan_info()["ens_hvp"]["directions_per_launch"] == 1
                for k in ("hv_infid", "hv_leak"):
                    assert np.array_equal(one[k][:, 0], r[k][:, j]), (k, j)
                for k in SAME_BITS:
                    assert np.array_equal(one[k], r[k]), k
    finally:
        wa.close()


def test_rounds_and_the_calls_around_are_the_same_bits(jq):
    """a stream budget that holds the primal stream and two directions: five directions run in three rounds, bit-identical to one
    launch; jq_eval_f_g_grad and jq_traceobjgrad_hvp on the same handle return the same bits before and after the calls"""
    c = ROWLANE_CASES[7]
    p, pcof, nodes, weights, shift, D, refs = _set_up(jq, c)
    stride = 16 * _npj(c.Ntot)      # doubles of a row-lane operator image
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    wb = jq.Working_Arrays_HIP(p, pcof.size, options={"stream_bytes": 8 * 3 * 2 * stride * (2 * NSTEPS + 1), "chunk_steps": NSTEPS})
    try:
        def around(w):
            jq.eval_f_g_grad(pcof, p, w, nodes, weights, True, shift=shift)
            h = jq.traceobjgrad_hvp(pcof, D[:, :2], p, w)
            return [np.array([p.last_infidelity, p.last_leak]), p.last_infidelity_grad.copy(), p.last_leak_grad.copy(), h["totalgrad"], h["hv"], h["hv_infid"]]
        before = [around(w) for w in (wa, wb)]
        a, b = [jq.eval_f_g_grad_hvp(pcof, D, p, w, nodes, weights, shift) for w in (wa, wb)]
        assert wa.plan_info()["ens_hvp"] == {"route": "rowlane", "directions_per_launch": 5, "chunk_steps": NSTEPS, "rounds": 1}
        assert wb.plan_info()["ens_hvp"] == {"route": "rowlane", "directions_per_launch": 2, "chunk_steps": NSTEPS, "rounds": 3}
        assert wb.last_timing()["n_forward_launches"] == 3 and wb.last_timing()["n_backward_launches"] == 6
        for k in SAME_BITS + ("hv_infid", "hv_leak"):
            assert np.array_equal(a[k], b[k]), k
        _check_against_reference(b, refs)
        after = [around(w) for w in (wa, wb)]
        for x, y in zip(before, after):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)
    finally:
        wa.close()
        wb.close()


@pytest.mark.parametrize("c", EVERYTHING, ids=[_id(c) for c in EVERYTHING])
def test_option_lane0_switches_back_to_the_sequential_route(jq, c):
    """option lane=0 takes the row-lane images away from the handle: the same call runs the nodes one after the other and passes the same reference"""
    p, pcof, nodes, weights, shift, D, refs = _set_up(jq, c)
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=_options(c, {"lane": 0}))
    try:
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift)
        plan = wa.plan_info()
        assert plan["ens_hvp"] == {"route": "sequential", "directions_per_launch": c.ndir, "chunk_steps": c.chunk or NSTEPS, "rounds": c.nquad}
        assert wa.last_timing()["kernel_family"] == KF_COOP
        _check_against_reference(r, refs)
        _check_primal(jq, r, pcof, p, wa, nodes, weights, shift)
    finally:
        wa.close()


def test_five_controls_stay_on_the_sequential_route(jq):
    """more than JQ_MAXNC controls run in control groups: the sequential route, as before"""
    c = Case(12, 2, 5, 1, 0, 1, 3, 3, "given")
    p, pcof, nodes, weights, shift, D, refs = _set_up(jq, c)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift)
        assert wa.plan_info()["ens_hvp"]["route"] == "sequential" and wa.last_timing()["kernel_family"] == KF_COOP
        _check_against_reference(r, refs)
    finally:
        wa.close()


def _rel(r, refs, k):
    return max(np.linalg.norm(r[k][:, j] - t[k]) / max(np.linalg.norm(t[k]), 1e-300) for j, t in enumerate(refs))


def test_full_length_cnot2(jq):
    """cnot2 (Ntot 12, N 4, objFuncType 1) at its full length of 5 985 steps over 2 nodes with a given shift of the size of
    |diag(Hconst)|, one random direction, on the row-lane route and -- option lane=0 -- on the sequential route, both against the
    ensemble reference with reference_pass.  Should the sequential route itself miss reference_pass on this input, the row-lane
    bound is 4 x the sequential route's measured relative error (both are roundings of the same exact quantity in another summation
    order).  Measured: row-lane 1.19e-14, sequential 1.33e-14 relative -- both pass reference_pass, so that is the criterion that applied.
    Then the exact-Hessian callback of setup_ipopt_problem on the same handle (its default: the one node eps = 0)."""
    p, info, pcof, _ = case_inputs("cnot2")
    assert (p.Ntot, p.N, p.nsteps) == (12, 4, 5985)
    rng = np.random.default_rng(31415)
    nodes, weights = np.array([-0.02, 0.03]), np.array([0.45, 0.55])
    shift = np.abs(np.diag(p.Hconst)).max() * rng.standard_normal(p.Ntot) / 3.0
    D = rng.standard_normal((pcof.size, 1))
    refs = _reference(p, pcof, D, nodes, weights, shift)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    ws = jq.Working_Arrays_HIP(p, pcof.size, options={"lane": 0})
    try:
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift)
        assert wa.plan_info()["ens_hvp"]["route"] == "rowlane"
        t = wa.last_timing()
        assert (t["kernel_family"], t["kernel_size"]) == (KF_ROWLANE, 12)
        q = jq.eval_f_g_grad_hvp(pcof, D, p, ws, nodes, weights, shift)
        assert ws.plan_info()["ens_hvp"]["route"] == "sequential"
        rel_r, rel_q = _rel(r, refs, "hv_infid"), _rel(q, refs, "hv_infid")
        print("cnot2 x 2 nodes, hv_infid against the reference: row-lane %.2e, sequential %.2e relative" % (rel_r, rel_q))
        if all(reference_pass(q["hv_infid"][:, j], t["hv_infid"]) for j, t in enumerate(refs)):
            _check_against_reference(r, refs)
        else:
            assert rel_r <= 4.0 * rel_q, (rel_r, rel_q)
        assert not r["hv_leak"].any()      # objFuncType 1
        _check_primal(jq, r, pcof, p, wa, nodes, weights, shift)
        n = pcof.size
        maxpar = info["maxpar"][0]
        prob = jq.setup_ipopt_problem(p, wa, n, np.full(n, -2.0 * maxpar), np.full(n, 2.0 * maxpar), maxIter=1, hessian="exact")
        hv = prob.eval_hessvec(pcof, D[:, 0])
        assert wa.plan_info()["ens_hvp"]["route"] == "rowlane" and np.isfinite(hv).all() and hv.any()
    finally:
        wa.close()
        ws.close()
