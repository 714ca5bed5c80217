"""GPU (-m gpu): jq_traceobjgrad_drifts / jq_eval_f_g_grad_drifts -- ONE control vector over an ensemble of arbitrary drift Hamiltonians in
one call.

Two criteria per member and per quantity, no others:
  (a) agreement with the CPU oracle on a copy of params whose Hconst is that member, with conftest.reference_pass (atol 1e-14 or rtol
      1e-10 in the 2-norm);
  (b) np.array_equal with the single call traceobjgrad on a SECOND handle with the same options whose params.Hconst was set to that member
      (jq_update_hconst + jq_traceobjgrad; cooperative quad: cq3=0 on both handles, the one-workgroup backward kernel a grouped launch runs).
Members: "dense" -- Hconst + 1e-2 |Hconst|_max R with a seeded random real symmetric R (plans without a structure); "pattern" -- every
stored nonzero of Hconst scaled by 1 + 1e-2 r_ij with a symmetric seeded r, plus a random diagonal (4 x 4 x n plans: the nonzero pattern off
the diagonal is unchanged, which the test checks on the CPU).  Time loops are shortened as in tests/test_gpu_pcof_batch.py."""
import copy

import numpy as np
import pytest

from conftest import case_inputs, reference_pass
from test_gpu_pcof_batch import NAMES, cnot3_short, column, same_bits
from test_gpu_random import random_problem

pytestmark = pytest.mark.gpu


def dense_members(H0, n, seed):
    rng = np.random.default_rng(seed)
    H0 = np.asarray(H0, dtype=np.float64)
    amp = 1e-2 * float(np.max(np.abs(H0)))
    out = []
    for _ in range(n):
        R = rng.standard_normal(H0.shape)
        out.append(H0 + amp * 0.5 * (R + R.T))
    return out


def pattern_members(H0, n, seed):
    rng = np.random.default_rng(seed)
    H0 = np.asarray(H0, dtype=np.float64)
    amp = 1e-2 * float(np.max(np.abs(H0)))
    off = ~np.eye(H0.shape[0], dtype=bool)
    out = []
    for _ in range(n):
        r = rng.standard_normal(H0.shape)
        M = H0 * (1.0 + 1e-2 * 0.5 * (r + r.T)) + np.diag(amp * rng.standard_normal(H0.shape[0]))
        assert np.array_equal((M != 0.0) & off, (H0 != 0.0) & off)      # the pattern off the diagonal is the handle's own
        assert np.array_equal(M, M.T)
        out.append(M)
    return out


def with_hconst(params, M):
    p = copy.copy(params)
    p.Hconst = np.array(M, dtype=np.float64)
    return p


def drifts(jq, pcof, params, wa, members):
    return dict(zip(NAMES, jq.traceobjgrad_drifts(pcof, params, wa, members, True)))


def single(jq, pcof, params, wa):
    return dict(zip(NAMES, jq.traceobjgrad(pcof, params, wa, False, True)))


class SecondHandle:
    """the single call on a second handle whose params.Hconst is set to a member (sync_params: jq_update_hconst)"""

    def __init__(self, jq, params, ncoeff, options, make=None):
        self.jq, self.params = jq, copy.copy(params)
        self.wa = (make or jq.Working_Arrays_HIP)(self.params, ncoeff, options=options)

    def __call__(self, pcof, M):
        self.params.Hconst = np.array(M, dtype=np.float64)
        return single(self.jq, pcof, self.params, self.wa)

    def close(self):
        self.wa.close()


def check_oracle(tag, params, pcof, M, col):
    from oracle.oracle import Oracle
    r = Oracle(with_hconst(params, M), use_sparse=bool(getattr(params, "use_sparse", False))).traceobjgrad(pcof)
    for k in NAMES:
        if k == "leakgrad" and params.objFuncType == 1:
            assert np.size(col[k]) == 0
            continue
        d = np.linalg.norm(np.atleast_1d(col[k]) - np.atleast_1d(r[k]))
        print("    %-28s %-16s |diff| %.3e  |ref| %.3e" % (tag, k, d, np.linalg.norm(np.atleast_1d(r[k]))))
        assert reference_pass(col[k], r[k]), (tag, k)


def check_drifts(jq, params, pcof, members, options, family, mode="grouped", oracle=True, make=None, crosstalk=True):
    """criteria (a) and (b), the handle's own drift before and after, cross-talk (member 0 again as the last one) and a permuted ensemble;
    returns the ensemble's result"""
    n = len(members)
    H_own = np.array(params.Hconst, dtype=np.float64)
    wa = (make or jq.Working_Arrays_HIP)(params, pcof.size, options=options)
    second = SecondHandle(jq, params, pcof.size, options, make)
    try:
        before = single(jq, pcof, params, wa)
        b = drifts(jq, pcof, params, wa, members)
        info = wa.plan_info()["drift_batch"]
        print("  drift_batch:", info, "family", wa.last_timing()["kernel_family"])
        assert info["mode"] == mode and info["reason"], info
        if family is not None:
            assert wa.last_timing()["kernel_family"] == family and (mode != "grouped" or info["family"] == family), (info, wa.last_timing())
        assert b["objfv"].shape == (n,) and b["totalgrad"].shape == (pcof.size, n)
        assert b["leakgrad"].shape == ((0, n) if params.objFuncType == 1 else (pcof.size, n))
        for i, M in enumerate(members):
            same_bits("member %d against the single call" % i, column(b, i), second(pcof, M))
            if oracle:
                check_oracle("member %d" % i, params, pcof, M, column(b, i))
        if crosstalk:
            c = drifts(jq, pcof, params, wa, list(members) + [members[0]])
            same_bits("first and last member", column(c, n), column(c, 0))
            for i in range(n):
                same_bits("longer ensemble, member %d" % i, column(c, i), column(b, i))
            perm = list(np.random.default_rng(n).permutation(n))
            p = drifts(jq, pcof, params, wa, [members[j] for j in perm])
            for i, j in enumerate(perm):
                same_bits("permuted ensemble, member %d" % i, column(p, i), column(b, j))
        # the handle's own drift is what it was
        assert np.array_equal(np.asarray(params.Hconst, dtype=np.float64), H_own)
        same_bits("plain traceobjgrad before and after", single(jq, pcof, params, wa), before)
        return b
    finally:
        wa.close()
        second.close()


# ---- 1 - 3. row-lane kernels (family 3) ----------------------------------------------------------------------------------------------------
def test_rowlane_swap02_full_length(jq):
    params, info, pcof, _ = case_inputs("swap02")
    check_drifts(jq, params, pcof, dense_members(params.Hconst, 5, 1101), None, 3)


def test_rowlane_two_sweeps_and_lds_constant_images(jq):
    params, info, pcof, _ = case_inputs("cnot2-leakieq")      # objFuncType 3: forced and unforced sweep; NPJ = 12
    check_drifts(jq, params, pcof, dense_members(params.Hconst, 3, 1102), None, 3)


def test_rowlane_two_members_never_share_a_wave(jq):
    rng = np.random.default_rng(1301)
    params, pcof = random_problem(jq, rng, 6, 2, 1, 1, 11, 3, 1, False)
    check_drifts(jq, params, pcof, dense_members(params.Hconst, 5, 1103), None, 3)


# ---- 4 - 7. cooperative-quad kernels (family 8) --------------------------------------------------------------------------------------------
def test_cq_cnot3_five_members(jq):
    params, pcof = cnot3_short()
    check_drifts(jq, params, pcof, pattern_members(params.Hconst, 5, 1104), {"cq3": 0}, 8)      # 5: not a multiple of the four quads of a slab


def test_cq_cnot3_chunks_hand_over_with_group_strides(jq):
    params, pcof = cnot3_short(60)
    opts = {"cq3": 0, "chunk_steps": 7, "stream_bytes": 3 << 20}      # nine chunks (the last one of four steps), five streams each
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    try:
        members = pattern_members(params.Hconst, 5, 1105)
        drifts(jq, pcof, params, wa, members)
        assert wa.last_timing()["n_forward_launches"] == 9, wa.last_timing()
    finally:
        wa.close()
    check_drifts(jq, params, pcof, members, opts, 8, crosstalk=False)


@pytest.mark.parametrize("N", [2, 8])
def test_cq_random_t4(jq, N):
    rng = np.random.default_rng(2300 + N)
    params, pcof = random_problem(jq, rng, 32, N, 2, 1, 14, 3, 2, "t4")
    check_drifts(jq, params, pcof, pattern_members(params.Hconst, 3, 1106 + N), {"cq3": 0}, 8)


def test_cq_dense_policy(jq):
    rng = np.random.default_rng(2401)
    params, pcof = random_problem(jq, rng, 24, 4, 2, 1, 12, 3, 1, False)
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    assert wa.plan_info()["structure"] != "t4"
    wa.close()
    check_drifts(jq, params, pcof, dense_members(params.Hconst, 3, 1107), {"cq3": 0}, 8)


# ---- 8. rounds --------------------------------------------------------------------------------------------------------------------------------
def test_rounds_of_two_equal_one_launch(jq):
    params, pcof = cnot3_short(100)
    members = pattern_members(params.Hconst, 5, 1108)
    w1 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    w2 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0, "pcof_batch_max": 2})
    try:
        b1, b2 = drifts(jq, pcof, params, w1, members), drifts(jq, pcof, params, w2, members)
        i1, i2 = w1.plan_info()["drift_batch"], w2.plan_info()["drift_batch"]
        assert i1["mode"] == i2["mode"] == "grouped" and i1["members_per_launch"] == 5 and i2["members_per_launch"] == 2, (i1, i2)
        assert w2.last_timing()["n_forward_launches"] == 3 * w1.last_timing()["n_forward_launches"]      # three launches
        for i in range(5):
            same_bits("rounds of two, member %d" % i, column(b2, i), column(b1, i))
    finally:
        w1.close()
        w2.close()


# ---- 9. through the embedded twin ---------------------------------------------------------------------------------------------------------
def test_grouped_through_the_embedded_twin(jq):
    from kronecker_problem import random_kronecker_problem
    params, pcof, _ = random_kronecker_problem(jq, (3, 3, 2), 4)
    assert params.Ntot == 18
    opts = {"embed": 2, "cq3": 0}      # (tests/test_gpu_batch_twin.py: every batch of the handle is evaluated by the twin)
    members = pattern_members(params.Hconst, 3, 1109)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    try:
        assert wa.plan_info()["embedded_twin_Ntot"] == 32
        drifts(jq, pcof, params, wa, members)
        assert wa.plan_info()["embedded_twin_Ntot"] == 32      # (pattern members keep the twin's structure)
    finally:
        wa.close()
    check_drifts(jq, params, pcof, members, opts, 8)


# ---- 10. routes without grouped streams: the handle's drift swapped per member -------------------------------------------------------------
def test_sequential_quad_layout(jq):
    params, pcof = cnot3_short()
    check_drifts(jq, params, pcof, pattern_members(params.Hconst, 3, 1110), {"cq": 0}, 6, mode="sequential", oracle=False)


def test_sequential_implicit_midpoint(jq):
    params, info, pcof, _ = case_inputs("swap02")
    params.Integrator_id = jq.Implicit_Midpoint
    params.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=100, tol=1e-12, nrhs=params.N)
    check_drifts(jq, params, pcof, dense_members(params.Hconst, 3, 1111), None, None, mode="sequential", oracle=False, make=jq.Working_Arrays_M_HIP)


def test_sequential_jacobi_solver(jq):
    params, info, pcof, _ = case_inputs("cnot2-jacobi")
    params.T = params.T * 200 / params.nsteps
    params.nsteps = 200
    # (pattern members: the plan of this problem is 4 x 4 x n, and a member outside it would re-plan the handle -- test 11 -- after which
    #  "before and after" are evaluations on two different plans)
    check_drifts(jq, params, pcof, pattern_members(params.Hconst, 3, 1112), None, None, mode="sequential", oracle=False)


def test_sequential_cooperative_kernels(jq):
    rng = np.random.default_rng(5101)
    params, pcof = random_problem(jq, rng, 40, 4, 2, 1, 9, 3, 2, False)
    check_drifts(jq, params, pcof, dense_members(params.Hconst, 3, 1113), None, 1, mode="sequential", oracle=False)


# ---- 11. a member outside the planned structure ---------------------------------------------------------------------------------------------
def test_member_outside_the_structure_replans_for_the_union(jq):
    """The issue places the extra nonzero at (1, 3); those two rows share a 4 x 4 diagonal block, which the 4 x 4 x n structure stores in
    full, so that entry does not leave the structure.  The entry used here, (1, 7), couples two different 4-row groups off their diagonal
    and does (checked below on the pattern)."""
    params, pcof = cnot3_short()
    members = pattern_members(params.Hconst, 3, 1114)
    assert members[1][1, 3] == 0.0 and members[1][1, 7] == 0.0
    members[1][1, 7] = members[1][7, 1] = 1e-2 * float(np.max(np.abs(params.Hconst)))
    r, c = 1, 7      # outside: other 4-row group, and neither (i, i +- 4) inside a 16-row block nor (i, i +- 16)
    assert r // 4 != c // 4 and abs(r - c) not in (4, 16)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    fresh_params = copy.copy(params)
    try:
        assert wa.plan_info()["structure"] == "t4"
        b = drifts(jq, pcof, params, wa, members)
        for i, M in enumerate(members):
            check_oracle("member %d" % i, params, pcof, M, column(b, i))
        structure = wa.plan_info()["structure"]
        assert structure != "t4"
        fresh = jq.Working_Arrays_HIP(fresh_params, pcof.size, options={"cq3": 0})      # created with the handle's drift, then given that member
        try:
            fresh_params.Hconst = members[1]
            fresh.sync_params()
            assert fresh.plan_info()["structure"] == structure, (fresh.plan_info()["structure"], structure)
        finally:
            fresh.close()
        check_oracle("the handle's own drift afterwards", params, pcof, params.Hconst, single(jq, pcof, params, wa))
    finally:
        wa.close()


# ---- 12. the reference's own ensemble through the new call ----------------------------------------------------------------------------------
def test_reference_ensemble_through_the_drifts_call(jq):
    from oracle.oracle import Oracle
    params, info, pcof, _ = case_inputs("swap02")
    nodes, weights = np.polynomial.legendre.leggauss(16)
    shift = np.asarray(params.shift_weights_reference(), dtype=np.float64)      # 0.01 * 10^(j-2), j = 2 .. Ntot (src/ipopt_interface.jl:41-44)
    H0 = np.asarray(params.Hconst, dtype=np.float64)
    members = [H0 + ep * np.diag(shift) for ep in nodes]
    r = Oracle(params).eval_f_g_grad(pcof, nodes, weights, shift)
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    try:
        b = drifts(jq, pcof, params, wa, members)
        inf, leak, member_out = jq.eval_f_g_grad_drifts(pcof, params, wa, members, weights, True, per_member=True)
        assert wa.plan_info()["drift_batch"]["mode"] == "grouped"
        got = dict(infidelity=inf, leak=leak, infid_grad=params.last_infidelity_grad, leak_grad=params.last_leak_grad)
        ref = dict(infidelity=r["last_infidelity"], leak=r["last_leak"], infid_grad=r["last_infidelity_grad"], leak_grad=r["last_leak_grad"])
        sums = dict(infidelity=b["primaryobjf"] @ weights, leak=b["secondaryobjf"] @ weights, infid_grad=b["infidelgrad"] @ weights)
        for k in ("infidelity", "leak", "infid_grad"):
            d = np.linalg.norm(np.atleast_1d(got[k]) - np.atleast_1d(ref[k]))
            print("    %-12s |diff to the oracle's loop| %.3e  |ref| %.3e" % (k, d, np.linalg.norm(np.atleast_1d(ref[k]))))
            assert reference_pass(got[k], ref[k]), k
            assert reference_pass(got[k], sums[k]), k      # (not bitwise: the host compiler may contract the sums)
        assert params.objFuncType == 1 and np.size(got["leak_grad"]) == 0
        assert inf == params.last_infidelity and leak == params.last_leak and np.array_equal(params.last_pcof, pcof)
        assert member_out.shape == (4, 16)
        for j, k in enumerate(("objfv", "primaryobjf", "secondaryobjf", "traceInfidelity")):
            assert np.array_equal(member_out[j], b[k]), k
    finally:
        wa.close()


# ---- 13. settings follow the handle ----------------------------------------------------------------------------------------------------------
def test_sv_type_4_with_random_dvds(jq):
    from test_svtype_host import random_dvds
    params, info, pcof, _ = case_inputs("swap02")
    D = random_dvds(params)
    params.dVds_r, params.dVds_i, params.sv_type = np.asfortranarray(D.real.copy()), np.asfortranarray(D.imag.copy()), 4
    members = dense_members(params.Hconst, 3, 1116)
    b = check_drifts(jq, params, pcof, members, None, 3, oracle=False)
    p1 = with_hconst(params, members[0])
    p1.sv_type = 1
    wa = jq.Working_Arrays_HIP(p1, pcof.size)
    r1 = single(jq, pcof, p1, wa)
    wa.close()
    assert b["objfv"][0] == r1["objfv"] and not np.array_equal(b["totalgrad"][:, 0], r1["totalgrad"])      # (the type was in force)


def test_full_leakage_weights_on_the_rowlane_kernels(jq):
    from test_gpu_dense_wmat import set_forbidden
    from test_gpu_svtype import RANDOM
    cfg = RANDOM[4][0]
    assert cfg[0] == 12 and RANDOM[4][3]
    rng = np.random.default_rng(4200 + cfg[0] * 31 + cfg[1])
    params, pcof = random_problem(jq, rng, *cfg)
    set_forbidden(params, rng, 3)
    check_drifts(jq, params, pcof, dense_members(params.Hconst, 3, 1117), None, 3, oracle=False)


# ---- 14. errors --------------------------------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    params, info, pcof, _ = case_inputs("swap02")
    n = pcof.size
    members = dense_members(params.Hconst, 3, 1118)
    wa = jq.Working_Arrays_HIP(params, n)
    try:
        wa.sync_params()
        H = np.ascontiguousarray(np.stack([np.asarray(M).ravel(order="F") for M in members]))
        w = np.full(3, 1.0 / 3.0)
        p = np.ascontiguousarray(pcof, dtype=np.float64)
        ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
        nan = float("nan")
        out4, out2, mo = np.full((3, 4), nan), np.full(2, nan), np.full((3, 4), nan)
        tg, ig, lg = np.full((3, n), nan), np.full((3, n), nan), np.full((3, n), nan)
        g1, g2 = np.full(n, nan), np.full(n, nan)
        o1, s1 = np.full(4, nan), np.full(n, nan)
        for ncoeff in (n - 1, 2):      # (an odd count; fewer than three coefficients per control function): the single call's codes
            rc1 = L.jq_traceobjgrad(wa.handle, ptr(p), ncoeff, 1, ptr(o1), ptr(s1), ptr(s1), ptr(s1))
            rcd = L.jq_traceobjgrad_drifts(wa.handle, ptr(p), ncoeff, ptr(H), 3, 1, ptr(out4), ptr(tg), ptr(ig), ptr(lg))
            rce = L.jq_eval_f_g_grad_drifts(wa.handle, ptr(p), ncoeff, ptr(H), ptr(w), 3, 1, ptr(out2), ptr(g1), ptr(g2), ptr(mo))
            print("    ncoeff %d: single %d, drifts %d, eval drifts %d" % (ncoeff, rc1, rcd, rce))
            assert rc1 != _lib.JQ_OK and rcd == rc1 and rce == rc1
        for nd in (0, -2):
            assert L.jq_traceobjgrad_drifts(wa.handle, ptr(p), n, ptr(H), nd, 1, ptr(out4), ptr(tg), ptr(ig), ptr(lg)) == _lib.JQ_EINVAL
            assert L.jq_eval_f_g_grad_drifts(wa.handle, ptr(p), n, ptr(H), ptr(w), nd, 1, ptr(out2), ptr(g1), ptr(g2), ptr(mo)) == _lib.JQ_EINVAL
        assert L.jq_traceobjgrad_drifts(wa.handle, ptr(p), n, None, 3, 1, ptr(out4), ptr(tg), ptr(ig), ptr(lg)) == _lib.JQ_EINVAL
        assert L.jq_traceobjgrad_drifts(wa.handle, None, n, ptr(H), 3, 1, ptr(out4), ptr(tg), ptr(ig), ptr(lg)) == _lib.JQ_EINVAL
        assert L.jq_traceobjgrad_drifts(wa.handle, ptr(p), n, ptr(H), 3, 1, None, ptr(tg), ptr(ig), ptr(lg)) == _lib.JQ_EINVAL
        assert L.jq_traceobjgrad_drifts(wa.handle, ptr(p), n, ptr(H), 3, 1, ptr(out4), ptr(tg), None, ptr(lg)) == _lib.JQ_EINVAL
        assert L.jq_eval_f_g_grad_drifts(wa.handle, ptr(p), n, None, ptr(w), 3, 1, ptr(out2), ptr(g1), ptr(g2), ptr(mo)) == _lib.JQ_EINVAL
        assert L.jq_eval_f_g_grad_drifts(wa.handle, ptr(p), n, ptr(H), None, 3, 1, ptr(out2), ptr(g1), ptr(g2), ptr(mo)) == _lib.JQ_EINVAL
        assert L.jq_eval_f_g_grad_drifts(wa.handle, ptr(p), n, ptr(H), ptr(w), 3, 1, None, ptr(g1), ptr(g2), ptr(mo)) == _lib.JQ_EINVAL
        assert L.jq_eval_f_g_grad_drifts(wa.handle, ptr(p), n, ptr(H), ptr(w), 3, 1, ptr(out2), None, ptr(g2), ptr(mo)) == _lib.JQ_EINVAL
        for a in (out4, out2, mo, tg, ig, lg, g1, g2):
            assert np.all(np.isnan(a))
        # forward only, NULL gradients
        assert L.jq_traceobjgrad_drifts(wa.handle, ptr(p), n, ptr(H), 3, 0, ptr(out4), None, None, None) == _lib.JQ_OK
        objfv, prim, sec = jq.traceobjgrad_drifts(pcof, params, wa, members, False)
        assert np.array_equal(objfv, out4[:, 0]) and np.array_equal(prim, out4[:, 1]) and np.array_equal(sec, out4[:, 2])
        assert L.jq_eval_f_g_grad_drifts(wa.handle, ptr(p), n, ptr(H), ptr(w), 3, 0, ptr(out2), None, None, None) == _lib.JQ_OK
        assert reference_pass(out2[0], prim @ w) and reference_pass(out2[1], sec @ w)
    finally:
        wa.close()


# ---- 15. multi-device handles ------------------------------------------------------------------------------------------------------------------
def test_multi_device_handle_shards_the_members(jq):
    params, pcof = cnot3_short(100)
    members = pattern_members(params.Hconst, 5, 1119)
    w1 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    wm = jq.Working_Arrays_HIP(params, pcof.size, devices=2, options={"cq3": 0, "multi_same_device": 1})
    try:
        b1, bm = drifts(jq, pcof, params, w1, members), drifts(jq, pcof, params, wm, members)
        for i in range(5):
            same_bits("multi-device handle, member %d" % i, column(bm, i), column(b1, i))
    finally:
        w1.close()
        wm.close()


# ---- 16. the optimiser over a drift ensemble ---------------------------------------------------------------------------------------------------
def test_run_optimizer_over_a_drift_ensemble(jq):
    params, info, pcof, _ = case_inputs("swap02")
    params.quiet = True
    members = dense_members(params.Hconst, 4, 1120)
    weights = np.array([0.1, 0.2, 0.3, 0.4])
    n = pcof.size
    wa = jq.Working_Arrays_HIP(params, n)
    try:
        amp = 4.0 * max(1.0, float(np.max(np.abs(pcof))))
        prob = jq.setup_ipopt_problem(params, wa, n, -amp * np.ones(n), amp * np.ones(n), maxIter=4, drifts=members, drift_weights=weights)
        f0 = prob.eval_f(pcof)
        x = jq.run_optimizer(prob, pcof)
        f1 = prob.eval_f(x)
        print("    objective %.12e -> %.12e in %d iterations (%s)" % (f0, f1, prob.n_iter, wa.plan_info()["drift_batch"]))
        assert f1 < f0
        assert wa.plan_info()["drift_batch"]["mode"] == "grouped"
        last, xl = params.last_infidelity, params.last_pcof.copy()      # (memoised: the vector within 1e-15 of x the callbacks last evaluated)
        assert np.linalg.norm(xl - x) <= 1.0e-15
        inf, leak = jq.eval_f_g_grad_drifts(xl, params, wa, members, weights, True)
        assert inf == last and params.last_infidelity == last
    finally:
        wa.close()
