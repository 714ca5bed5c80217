"""GPU (-m gpu): jq_traceobjgrad_members / jq_eval_f_g_grad_members -- ONE control vector over members that differ in a real Nc x Nc mixing
matrix C of the controls (operator l is driven by sum_k C[l, k] (p_k, q_k): amplitude miscalibration, crosstalk), in their drift, or in both.

Two criteria per member and per quantity, no others:
  (a) agreement with the CPU oracle with conftest.reference_pass (atol 1e-14 or rtol 1e-10 in the 2-norm) on a copy of params whose
      operators are the mixed ones, Hsym'_k = sum_l C[l, k] Hsym_l and Hanti'_k = sum_l C[l, k] Hanti_l, and whose Hconst is the member's
      -- the plain problem the member is by linearity; the oracle itself knows nothing of mixes;
  (b) np.array_equal with the same member evaluated ALONE (nmember == 1: the sequential route, the single evaluation with that mix) on a
      SECOND handle with the same options (cooperative quad: cq3=0 on both handles).
Mixes: "full" -- I + 0.05 R with a seeded normal R; "amplitude" -- diag(1 + 0.05 r).  Time loops are shortened as in
tests/test_gpu_drift_batch.py."""
import copy

import numpy as np
import pytest

from conftest import case_inputs, reference_pass
from test_gpu_drift_batch import dense_members, pattern_members
from test_gpu_pcof_batch import NAMES, cnot3_short, column, same_bits
from test_gpu_random import random_problem

pytestmark = pytest.mark.gpu


def ncontrols(params):
    return max(params.Ncoupled, params.Nunc)


def full_mixes(Nc, n, seed):
    rng = np.random.default_rng(seed)
    return [np.eye(Nc) + 0.05 * rng.standard_normal((Nc, Nc)) for _ in range(n)]


def amplitude_mixes(jq, Nc, n, seed):
    rng = np.random.default_rng(seed)
    C = jq.amplitude_mix(1.0 + 0.05 * rng.standard_normal((n, Nc)))
    assert C.shape == (Nc, Nc, n)
    return [C[:, :, i].copy() for i in range(n)]


def mixed_params(params, C, H=None):
    """the plain problem a member is: operators mixed with the columns of C, the member's drift"""
    p = copy.copy(params)
    C = np.asarray(C, dtype=np.float64)
    Nc = C.shape[0]
    mixed = lambda ops: [sum(C[l, k] * np.asarray(ops[l], dtype=np.float64) for l in range(Nc)) for k in range(Nc)]
    if params.Nunc:
        p.Hunc_ops = mixed(params.Hunc_ops)
    else:
        p.Hsym_ops, p.Hanti_ops = mixed(params.Hsym_ops), mixed(params.Hanti_ops)
    if H is not None:
        p.Hconst = np.array(H, dtype=np.float64)
    return p


def members(jq, pcof, params, wa, mixes, drifts=None):
    return dict(zip(NAMES, jq.traceobjgrad_members(pcof, params, wa, Hconsts=drifts, ctrl_mix=mixes, evaladjoint=True)))


def single(jq, pcof, params, wa):
    return dict(zip(NAMES, jq.traceobjgrad(pcof, params, wa, False, True)))


def check_oracle(tag, params, pcof, C, H, col):
    from juqbox_jl_amd import Implicit_Midpoint
    from oracle.oracle import Oracle
    orc = Oracle(mixed_params(params, C, H), use_sparse=bool(getattr(params, "use_sparse", False)))
    if params.Integrator_id == Implicit_Midpoint:      # (the oracle's integrators are two methods; its fixed-point solver takes the handle's settings)
        r = orc.traceobjgrad_imr(pcof, int(params.linear_solver.max_iter), float(params.linear_solver.tol))
    else:
        r = orc.traceobjgrad(pcof)
    for k in NAMES:
        if k == "leakgrad" and params.objFuncType == 1:
            assert np.size(col[k]) == 0
            continue
        d = np.linalg.norm(np.atleast_1d(col[k]) - np.atleast_1d(r[k]))
        print("    %-28s %-16s |diff| %.3e  |ref| %.3e" % (tag, k, d, np.linalg.norm(np.atleast_1d(r[k]))))
        assert reference_pass(col[k], r[k]), (tag, k)


def check_members(jq, params, pcof, mixes, options, family, drifts=None, mode="grouped", oracle=True, make=None, crosstalk=False):
    """criteria (a) and (b), the plan's report, the plain evaluation before and after; crosstalk: member 0 again as the last one and a
    permuted ensemble.  Returns the ensemble's result"""
    n = len(mixes)
    make = make or jq.Working_Arrays_HIP
    wa = make(params, pcof.size, options=options)
    p2 = copy.copy(params)
    alone = make(p2, pcof.size, options=options)
    try:
        before = single(jq, pcof, params, wa)
        b = members(jq, pcof, params, wa, mixes, drifts)
        info = wa.plan_info()["member_batch"]
        print("  member_batch:", info, "family", wa.last_timing()["kernel_family"])
        assert info["mode"] == mode and info["reason"], info
        assert info["ctrl_mix"] is True and info["drifts"] is (drifts is not None), info
        if family is not None:
            assert wa.last_timing()["kernel_family"] == family and (mode != "grouped" or info["family"] == family), (info, wa.last_timing())
        assert b["objfv"].shape == (n,) and b["totalgrad"].shape == (pcof.size, n)
        assert b["leakgrad"].shape == ((0, n) if params.objFuncType == 1 else (pcof.size, n))
        for i, C in enumerate(mixes):
            H = None if drifts is None else drifts[i]
            a = members(jq, pcof, p2, alone, [C], None if H is None else [H])
            assert alone.plan_info()["member_batch"]["mode"] == "sequential"
            same_bits("member %d against the member alone" % i, column(b, i), column(a, 0))
            if oracle:
                check_oracle("member %d" % i, params, pcof, C, H, column(b, i))
        if crosstalk:
            dl = None if drifts is None else list(drifts)
            c = members(jq, pcof, params, wa, list(mixes) + [mixes[0]], None if dl is None else dl + [dl[0]])
            same_bits("first and last member", column(c, n), column(c, 0))
            for i in range(n):
                same_bits("longer ensemble, member %d" % i, column(c, i), column(b, i))
            perm = list(np.random.default_rng(n).permutation(n))
            p = members(jq, pcof, params, wa, [mixes[j] for j in perm], None if dl is None else [dl[j] for j in perm])
            for i, j in enumerate(perm):
                same_bits("permuted ensemble, member %d" % i, column(p, i), column(b, j))
        same_bits("plain traceobjgrad before and after", single(jq, pcof, params, wa), before)
        return b
    finally:
        wa.close()
        alone.close()


# ---- 1, 2. row-lane kernels (family 3) -------------------------------------------------------------------------------------------------------
def test_rowlane_full_mixes(jq):
    rng = np.random.default_rng(1401)
    params, pcof = random_problem(jq, rng, 6, 2, 2, 2, 11, 3, 1, False)
    check_members(jq, params, pcof, full_mixes(2, 5, 2101), None, 3)


def test_rowlane_two_control_groups_accumulate_over_both_sweeps(jq):
    rng = np.random.default_rng(1402)
    params, pcof = random_problem(jq, rng, 6, 2, 5, 1, 11, 3, 3, False)      # Nc = 5: two control groups; objFuncType 3: forced + unforced
    check_members(jq, params, pcof, full_mixes(5, 3, 2102), None, 3)


# ---- 3, 4. cooperative-quad kernels (family 8) -----------------------------------------------------------------------------------------------
def test_cq_cnot3_five_members(jq):
    params, pcof = cnot3_short()
    Nc = ncontrols(params)
    mixes = amplitude_mixes(jq, Nc, 2, 2103) + full_mixes(Nc, 3, 2104)      # 5: not a multiple of the four quads of a slab
    check_members(jq, params, pcof, mixes, {"cq3": 0}, 8)


def test_cq_cnot3_chunks_hand_over_with_group_strides(jq):
    params, pcof = cnot3_short(60)
    opts = {"cq3": 0, "chunk_steps": 7, "stream_bytes": 3 << 20}      # nine chunks (the last one of four steps)
    mixes = full_mixes(ncontrols(params), 3, 2105)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    try:
        members(jq, pcof, params, wa, mixes)
        assert wa.last_timing()["n_forward_launches"] == 9, wa.last_timing()
    finally:
        wa.close()
    check_members(jq, params, pcof, mixes, opts, 8)


def test_cq_dense_policy(jq):
    rng = np.random.default_rng(2401)
    params, pcof = random_problem(jq, rng, 24, 4, 2, 1, 12, 3, 1, False)
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    assert wa.plan_info()["structure"] != "t4"
    wa.close()
    check_members(jq, params, pcof, full_mixes(2, 3, 2106), {"cq3": 0}, 8)


# ---- 5. through the embedded twin ------------------------------------------------------------------------------------------------------------
def test_grouped_through_the_embedded_twin(jq):
    from kronecker_problem import random_kronecker_problem
    params, pcof, _ = random_kronecker_problem(jq, (3, 3, 2), 4)
    opts = {"embed": 2, "cq3": 0}      # (tests/test_gpu_batch_twin.py: every batch of the handle is evaluated by the twin)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    assert wa.plan_info()["embedded_twin_Ntot"] == 32
    wa.close()
    check_members(jq, params, pcof, full_mixes(ncontrols(params), 3, 2107), opts, 8)


# ---- 6. routes without grouped streams: member after member, each with its mix -----------------------------------------------------------
def test_sequential_quad_layout(jq):
    params, pcof = cnot3_short()
    check_members(jq, params, pcof, full_mixes(ncontrols(params), 3, 2108), {"cq": 0}, 6, mode="sequential")


def test_sequential_implicit_midpoint(jq):
    params, info, pcof, _ = case_inputs("swap02")
    params.Integrator_id = jq.Implicit_Midpoint
    params.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=100, tol=1e-12, nrhs=params.N)
    check_members(jq, params, pcof, full_mixes(ncontrols(params), 3, 2109), None, None, mode="sequential", make=jq.Working_Arrays_M_HIP)


def test_sequential_jacobi_solver(jq):
    params, info, pcof, _ = case_inputs("cnot2-jacobi")
    params.T = params.T * 200 / params.nsteps
    params.nsteps = 200
    check_members(jq, params, pcof, full_mixes(ncontrols(params), 3, 2110), None, None, mode="sequential")


def test_sequential_cooperative_kernels(jq):
    rng = np.random.default_rng(5101)
    params, pcof = random_problem(jq, rng, 40, 4, 2, 1, 9, 3, 2, False)
    check_members(jq, params, pcof, full_mixes(2, 3, 2111), None, 1, mode="sequential")


# ---- 7. drifts AND mixes ---------------------------------------------------------------------------------------------------------------------
def test_drifts_and_mixes_together_on_the_rowlane_kernels(jq):
    rng = np.random.default_rng(1403)
    params, pcof = random_problem(jq, rng, 6, 2, 2, 2, 11, 3, 1, False)
    check_members(jq, params, pcof, full_mixes(2, 3, 2112), None, 3, drifts=dense_members(params.Hconst, 3, 2113))


def test_drifts_and_mixes_together_on_the_cooperative_quad_kernels(jq):
    params, pcof = cnot3_short()
    check_members(jq, params, pcof, full_mixes(ncontrols(params), 3, 2114), {"cq3": 0}, 8, drifts=pattern_members(params.Hconst, 3, 2115))


# ---- 8. C = I ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rowlane-two-groups", "cq"])
def test_identity_mixes_are_the_unmixed_evaluation_bit_for_bit(jq, case):
    if case == "cq":
        params, pcof = cnot3_short(100)
        opts, drifts = {"cq3": 0}, pattern_members(params.Hconst, 3, 2116)
    else:
        params, pcof = random_problem(jq, np.random.default_rng(1404), 6, 2, 5, 1, 11, 3, 3, False)
        opts, drifts = None, dense_members(params.Hconst, 3, 2117)
    eye = [np.eye(ncontrols(params)) for _ in range(3)]
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    try:
        before = single(jq, pcof, params, wa)
        d = dict(zip(NAMES, jq.traceobjgrad_drifts(pcof, params, wa, drifts, True)))
        b = members(jq, pcof, params, wa, eye, drifts)
        for i in range(3):
            same_bits("identity mixes with drifts, member %d" % i, column(b, i), column(d, i))
        b = members(jq, pcof, params, wa, eye)
        assert wa.plan_info()["member_batch"]["mode"] == "grouped"
        for i in range(3):
            same_bits("identity mixes, member %d" % i, column(b, i), before)
        a = members(jq, pcof, params, wa, eye[:1])      # (alone: the single evaluation with the mix)
        same_bits("one identity mix", column(a, 0), before)
        same_bits("plain traceobjgrad before and after", single(jq, pcof, params, wa), before)
    finally:
        wa.close()


# ---- 9. a zero column ----------------------------------------------------------------------------------------------------------------------
def test_zero_column_gives_an_exactly_zero_gradient_block(jq):
    rng = np.random.default_rng(1405)
    params, pcof = random_problem(jq, rng, 6, 2, 5, 1, 11, 3, 3, False)
    mixes = full_mixes(5, 3, 2118)
    k = 3
    mixes[1][:, k] = 0.0
    b = check_members(jq, params, pcof, mixes, None, 3)
    per = pcof.size // 5      # (one block of 2 Nfreq D1 coefficients per control)
    for name in ("totalgrad", "infidelgrad", "leakgrad"):
        g = b[name][:, 1]
        assert np.all(g[k * per:(k + 1) * per] == 0.0), name
        assert np.linalg.norm(g) > 0.0 and np.linalg.norm(b[name][k * per:(k + 1) * per, 0]) > 0.0, name


# ---- 10. uncoupled controls ------------------------------------------------------------------------------------------------------------------
def test_uncoupled_controls_amplitude_members(jq):
    from test_uncoupled import lab_problem
    lab, pcof = lab_problem(jq, 5, True, oft=3)      # (the second control antisymmetric; forced and unforced sweep)
    assert lab.Nunc == 2 and lab.Ncoupled == 0
    # The time loop is NOT shortened here: the lab-frame problem has GHz carriers, and with fewer than about 3 000 of its 4 250 steps the
    # Neumann iteration diverges -- NaN in the oracle and on the device alike (seen with 500 .. 2 000 steps).  At full length the device
    # takes milliseconds and an oracle evaluation 0.2 s.
    mixes = amplitude_mixes(jq, 2, 3, 2119)
    wa = jq.Working_Arrays_HIP(lab, pcof.size)
    try:
        b = members(jq, pcof, lab, wa, mixes)
        info = wa.plan_info()["member_batch"]
        print("  member_batch:", info, "family", wa.last_timing()["kernel_family"])
        assert info["mode"] == "grouped" and info["family"] == 3 and wa.last_timing()["kernel_family"] == 3, info      # (Ntot = 9: row-lane)
        for i, C in enumerate(mixes):
            check_oracle("member %d" % i, lab, pcof, C, None, column(b, i))
    finally:
        wa.close()


# ---- 11. cross-talk between members, rounds -----------------------------------------------------------------------------------------------
def test_members_do_not_talk_to_each_other(jq):
    rng = np.random.default_rng(1406)
    params, pcof = random_problem(jq, rng, 6, 2, 5, 1, 11, 3, 3, False)
    check_members(jq, params, pcof, full_mixes(5, 4, 2120), None, 3, oracle=False, crosstalk=True)
    params, pcof = cnot3_short(100)
    check_members(jq, params, pcof, full_mixes(ncontrols(params), 3, 2121), {"cq3": 0}, 8, oracle=False, crosstalk=True)


def test_rounds_of_two_equal_one_launch(jq):
    params, pcof = cnot3_short(100)
    mixes = full_mixes(ncontrols(params), 5, 2122)
    w1 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    w2 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0, "pcof_batch_max": 2})
    try:
        b1, b2 = members(jq, pcof, params, w1, mixes), members(jq, pcof, params, w2, mixes)
        i1, i2 = w1.plan_info()["member_batch"], w2.plan_info()["member_batch"]
        assert i1["mode"] == i2["mode"] == "grouped" and i1["members_per_launch"] == 5 and i2["members_per_launch"] == 2, (i1, i2)
        assert w2.last_timing()["n_forward_launches"] == 3 * w1.last_timing()["n_forward_launches"]      # three launches
        for i in range(5):
            same_bits("rounds of two, member %d" % i, column(b2, i), column(b1, i))
    finally:
        w1.close()
        w2.close()


# ---- 12. the weighted sums ---------------------------------------------------------------------------------------------------------------------
def test_eval_f_g_grad_members_forms_the_host_sums_in_member_order(jq):
    rng = np.random.default_rng(1407)
    params, pcof = random_problem(jq, rng, 6, 2, 2, 2, 11, 3, 3, False)
    mixes, w = full_mixes(2, 4, 2123), np.array([0.1, 0.2, 0.3, 0.4])
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    try:
        b = members(jq, pcof, params, wa, mixes)
        inf, leak, member_out = jq.eval_f_g_grad_members(pcof, params, wa, w, ctrl_mix=mixes, per_member=True)
        assert wa.plan_info()["member_batch"]["mode"] == "grouped"
        s_inf = s_leak = 0.0
        g_inf, g_leak = np.zeros(pcof.size), np.zeros(pcof.size)
        for i in range(4):      # (member order; products and sums rounded one by one, as the library forms them)
            s_inf, s_leak = s_inf + b["primaryobjf"][i] * w[i], s_leak + b["secondaryobjf"][i] * w[i]
            g_inf, g_leak = g_inf + w[i] * b["infidelgrad"][:, i], g_leak + w[i] * b["leakgrad"][:, i]
        for got, want, name in ((inf, s_inf, "infidelity"), (leak, s_leak, "leak"), (params.last_infidelity_grad, g_inf, "infid_grad"),
                                (params.last_leak_grad, g_leak, "leak_grad")):
            print("    %-12s max |library - host sum| %.3e" % (name, np.max(np.abs(np.asarray(got) - want))))
            assert np.array_equal(np.asarray(got), np.asarray(want)), name
        assert member_out.shape == (4, 4)
        for j, k in enumerate(("objfv", "primaryobjf", "secondaryobjf", "traceInfidelity")):
            assert np.array_equal(member_out[j], b[k]), k
        assert inf == params.last_infidelity and leak == params.last_leak and np.array_equal(params.last_pcof, pcof)
        assert params.lastTraceInfidelity == inf and params.lastLeakIntegral == leak
        inf0, leak0 = jq.eval_f_g_grad_members(pcof, params, wa, w, ctrl_mix=mixes, compute_adjoint=False)
        assert inf0 == inf and leak0 == leak and not np.any(params.last_infidelity_grad)
    finally:
        wa.close()


# ---- 13. multi-device handles ------------------------------------------------------------------------------------------------------------------
def test_multi_device_handle_shards_the_members(jq):
    params, pcof = cnot3_short(100)
    mixes = full_mixes(ncontrols(params), 5, 2124)
    w1 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    wm = jq.Working_Arrays_HIP(params, pcof.size, devices=2, options={"cq3": 0, "multi_same_device": 1})
    try:
        b1, bm = members(jq, pcof, params, w1, mixes), members(jq, pcof, params, wm, mixes)
        for i in range(5):
            same_bits("multi-device handle, member %d" % i, column(bm, i), column(b1, i))
    finally:
        w1.close()
        wm.close()


# ---- 14. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_handle_as_it_was(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(1408)
    params, pcof = random_problem(jq, rng, 6, 2, 2, 2, 11, 3, 3, False)
    n = pcof.size
    wa = jq.Working_Arrays_HIP(params, n)
    try:
        before = single(jq, pcof, params, wa)
        C = np.ascontiguousarray(np.stack([M.ravel(order="F") for M in full_mixes(2, 3, 2125)]))
        bad = C.copy()
        bad[1, 2] = float("nan")
        inf = C.copy()
        inf[2, 0] = float("inf")
        w = np.full(3, 1.0 / 3.0)
        p = np.ascontiguousarray(pcof, dtype=np.float64)
        ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
        nan = float("nan")
        out4, out2, mo = np.full((3, 4), nan), np.full(2, nan), np.full((3, 4), nan)
        tg, ig, lg = np.full((3, n), nan), np.full((3, n), nan), np.full((3, n), nan)
        g1, g2 = np.full(n, nan), np.full(n, nan)
        o1, s1 = np.full(4, nan), np.full(n, nan)
        tr = lambda pc, nco, H, M, nm: L.jq_traceobjgrad_members(wa.handle, pc, nco, H, M, nm, 1, ptr(out4), ptr(tg), ptr(ig), ptr(lg))
        ev = lambda pc, nco, H, M, nm: L.jq_eval_f_g_grad_members(wa.handle, pc, nco, H, M, ptr(w), nm, 1, ptr(out2), ptr(g1), ptr(g2), ptr(mo))
        for call in (tr, ev):
            assert call(ptr(p), n, None, None, 3) == _lib.JQ_EINVAL                  # both arrays NULL
            assert call(ptr(p), n, None, ptr(C), 0) == _lib.JQ_EINVAL                # nmember = 0
            assert call(ptr(p), n, None, ptr(C), -1) == _lib.JQ_EINVAL
            assert call(ptr(p), n, None, ptr(bad), 3) == _lib.JQ_EINVAL              # a NaN entry
            assert call(ptr(p), n, None, ptr(inf), 3) == _lib.JQ_EINVAL
            assert call(None, n, None, ptr(C), 3) == _lib.JQ_EINVAL
            for ncoeff in (n - 1, 2):      # the single call's codes
                rc1 = L.jq_traceobjgrad(wa.handle, ptr(p), ncoeff, 1, ptr(o1), ptr(s1), ptr(s1), ptr(s1))
                assert rc1 != _lib.JQ_OK and call(ptr(p), ncoeff, None, ptr(C), 3) == rc1
        assert L.jq_traceobjgrad_members(wa.handle, ptr(p), n, None, ptr(C), 3, 1, None, ptr(tg), ptr(ig), ptr(lg)) == _lib.JQ_EINVAL
        assert L.jq_traceobjgrad_members(wa.handle, ptr(p), n, None, ptr(C), 3, 1, ptr(out4), ptr(tg), None, ptr(lg)) == _lib.JQ_EINVAL
        assert L.jq_eval_f_g_grad_members(wa.handle, ptr(p), n, None, ptr(C), None, 3, 1, ptr(out2), ptr(g1), ptr(g2), ptr(mo)) == _lib.JQ_EINVAL
        for a in (out4, out2, mo, tg, ig, lg, g1, g2, o1, s1):
            assert np.all(np.isnan(a))
        same_bits("the next plain evaluation", single(jq, pcof, params, wa), before)
        # forward only, NULL gradients
        assert L.jq_traceobjgrad_members(wa.handle, ptr(p), n, None, ptr(C), 3, 0, ptr(out4), None, None, None) == _lib.JQ_OK
        objfv, prim, sec = jq.traceobjgrad_members(pcof, params, wa, ctrl_mix=C.reshape(3, 2, 2).transpose(2, 1, 0), evaladjoint=False)
        assert np.array_equal(objfv, out4[:, 0]) and np.array_equal(prim, out4[:, 1]) and np.array_equal(sec, out4[:, 2])
        with pytest.raises(ValueError):
            jq.traceobjgrad_members(pcof, params, wa)
    finally:
        wa.close()


# ---- 15. the optimiser over an amplitude ensemble ----------------------------------------------------------------------------------------------
def test_run_optimizer_over_an_amplitude_ensemble(jq):
    params, info, pcof, _ = case_inputs("swap02")
    params.quiet = True
    mixes = jq.amplitude_mix(1.0 + 0.05 * np.random.default_rng(2126).standard_normal((3, ncontrols(params))))
    weights = np.array([0.2, 0.3, 0.5])
    n = pcof.size
    wa = jq.Working_Arrays_HIP(params, n)
    try:
        amp = 4.0 * max(1.0, float(np.max(np.abs(pcof))))
        prob = jq.setup_ipopt_problem(params, wa, n, -amp * np.ones(n), amp * np.ones(n), maxIter=4, ctrl_mix=mixes, member_weights=weights)
        f0 = prob.eval_f(pcof)
        x = jq.run_optimizer(prob, pcof)
        f1 = prob.eval_f(x)
        print("    objective %.12e -> %.12e in %d iterations (%s)" % (f0, f1, prob.n_iter, wa.plan_info()["member_batch"]))
        assert f1 < f0
        assert wa.plan_info()["member_batch"]["mode"] == "grouped" and wa.plan_info()["member_batch"]["ctrl_mix"] is True
        last, xl = params.last_infidelity, params.last_pcof.copy()      # (memoised: the vector within 1e-15 of x the callbacks last evaluated)
        assert np.linalg.norm(xl - x) <= 1.0e-15
        inf, leak = jq.eval_f_g_grad_members(xl, params, wa, weights, ctrl_mix=mixes)
        assert inf == last and params.last_infidelity == last
    finally:
        wa.close()
