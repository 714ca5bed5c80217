"""GPU (-m gpu): continuation adjoints -- params.sv_type 2 / 3 and params.dVds (src/evalobjgrad.jl:312-319, :815-844, :1492-1520) and the
project's type 4 (both terms in one backward sweep) through every Stormer-Verlet terminal kernel, against the CPU oracle.

The oracle only knows type 1; tests/test_svtype_host.py derives the references from it (type 1 with substituted targets) and checks
them oracle against oracle.  Criterion everywhere: conftest.reference_pass (atol 1e-14 or rtol 1e-10 in the 2-norm), as for every
Stormer-Verlet test of the suite."""

import numpy as np
import pytest

from conftest import case_inputs, reference_pass
from test_gpu_random import random_problem
from test_svtype_host import (align, leak_part, oracle_ensemble_eval, oracle_eval, random_dvds, ref_polar, ref_type2, ref_type3,
                              target_of, with_target)

pytestmark = pytest.mark.gpu

MFMA = (0, 1, 6, 8)      # kernel families whose state file has the slab layout (k_terminal / k_terminal_parts)


def set_dvds(params, D, sv_type):
    params.dVds_r = np.asfortranarray(np.real(D).copy())
    params.dVds_i = np.asfortranarray(np.imag(D).copy())
    params.sv_type = sv_type


def run(jq, params, pcof, wa):
    objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, params, wa, False, True)
    return dict(objfv=objfv, totalgrad=tg, primaryobjf=prim, secondaryobjf=sec, traceInfidelity=tinf, infidelgrad=ig, leakgrad=lg)


def close(name, value, ref):
    value, ref = np.atleast_1d(np.asarray(value, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    print("    %-34s |diff| %.3e  |ref| %.3e" % (name, np.linalg.norm(value - ref), np.linalg.norm(ref)))
    assert reference_pass(value, ref), name


class References:
    """everything the oracle has to say about one (params, pcof): computed once, used for every kernel family"""

    def __init__(self, params, pcof, evaluate=None):
        ev = evaluate or oracle_eval(pcof)
        self.two_grads = params.objFuncType != 1
        self.D = random_dvds(params)
        self.Dp, self.rho = align(params, pcof, self.D)
        self.r1 = ev(params)
        self.r2, self.r3 = ref_type2(params, ev, self.Dp, self.rho), ref_type3(params, ev, self.rho)
        self.ell = leak_part(params, ev)
        self.polar_D, self.polar_Dp = ref_polar(params, ev, self.D), ref_polar(params, ev, self.Dp)


def check_every_type(jq, params, pcof, wa, ref, family=None):
    T = target_of(params)

    def go(D, sv_type, tag):
        set_dvds(params, D, sv_type)
        r = run(jq, params, pcof, wa)
        assert wa.plan_info()["sv_type"] == sv_type
        t = wa.last_timing()["kernel_family"]
        if family is not None:
            assert t in (family if isinstance(family, tuple) else (family,)), (tag, t, family)
        for k in ("objfv", "primaryobjf", "secondaryobjf", "traceInfidelity"):      # the objective is taken against the target in every type
            close(tag + " " + k, r[k], ref.r1[k])
        if ref.two_grads:      # the leakage gradient is that of type 1, and what separates total from infidelity gradient
            close(tag + " leakgrad", r["leakgrad"], ref.r1["leakgrad"])
        else:
            assert np.array_equal(r["infidelgrad"], r["totalgrad"]) and r["leakgrad"].size == 0
        return r

    try:
        print("  kernel family asked for: %s" % (family,))
        r2 = go(ref.Dp, 2, "type 2, aligned")
        close("type 2, aligned totalgrad", r2["totalgrad"], ref.r2["totalgrad"])
        close("type 2, aligned infidelgrad", r2["infidelgrad"], ref.r2["infidelgrad"])
        r3 = go(ref.Dp, 3, "type 3, aligned")
        close("type 3, aligned totalgrad", r3["totalgrad"], ref.r3["totalgrad"])
        close("type 3, aligned infidelgrad", r3["infidelgrad"], ref.r3["infidelgrad"])
        r4 = go(ref.Dp, 4, "type 4, aligned")
        close("type 4, aligned totalgrad", r4["totalgrad"], ref.r2["totalgrad"] + ref.r3["totalgrad"] - ref.ell)
        close("type 4, aligned polarisation", r4["totalgrad"], ref.polar_Dp + ref.ell)
        if ref.two_grads:
            close("type 4, aligned infidelgrad", r4["infidelgrad"], ref.r2["infidelgrad"] + ref.r3["infidelgrad"])
        g2, g3, g4 = go(ref.D, 2, "type 2, general"), go(ref.D, 3, "type 3, general"), go(ref.D, 4, "type 4, general")
        close("types 2 + 3, general totalgrad", g2["totalgrad"] + g3["totalgrad"], ref.polar_D + 2.0 * ref.ell)
        close("type 4, general totalgrad", g4["totalgrad"], ref.polar_D + ref.ell)
        if ref.two_grads:
            close("types 2 + 3, general infidelgrad", g2["infidelgrad"] + g3["infidelgrad"], ref.polar_D)
            close("type 4, general infidelgrad", g4["infidelgrad"], ref.polar_D)
        # back to type 1: dVds is ignored again
        params.sv_type = 1
        r1 = run(jq, params, pcof, wa)
        close("type 1 again totalgrad", r1["totalgrad"], ref.r1["totalgrad"])
    finally:
        set_dvds(params, T, 1)


# ---- 1. every Stormer-Verlet terminal kernel -------------------------------------------------------------------------------------------
def _cnot3_short():
    params, info, pcof, _ = case_inputs("cnot3")
    params.nsteps = 300
    params.T = params.T * 300 / 32386
    return params, pcof


def _inputs(case):
    if case == "cnot3x300":
        return _cnot3_short()
    params, info, pcof, _ = case_inputs(case)
    return params, pcof


@pytest.mark.parametrize("case,option_sets", [
    ("swap02", [({}, 3)]),                                                      # row-lane: k_terminal_cols<RowlaneMap, EP_SV>
    # two sweeps (objFuncType 3); lane=0: the 16-level twin problem on the MFMA kernels (k_terminal)
    ("cnot2-leakieq", [({}, 3), ({"lane": 0}, MFMA)]),
    # the embedded twin (4 x 4 x 1) for every batch, and no twin at all on the MFMA kernels
    ("cnot2", [({"embed": 2}, MFMA), ({"embed": 0, "lane": 0}, MFMA)]),
    # cooperative quad (default), quad layout, cooperative, slabs: k_terminal at KT = 6 in each launch shape
    ("cnot3x300", [({}, 8), ({"cq": 0}, 6), ({"quad": 0}, 1), ({"quad": 0, "coop_max": 0}, 0)]),
])
def test_reference_cases_on_every_terminal_kernel(jq, case, option_sets):
    params, pcof = _inputs(case)
    ref = References(params, pcof)
    for opts, family in option_sets:
        print("%s %s" % (case, opts))
        wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
        info = wa.plan_info()
        if opts.get("embed") == 2:
            assert info["embedded_twin_Ntot"] == 16
        if opts.get("embed") == 0:
            assert info["embedded_twin_Ntot"] == 0
        check_every_type(jq, params, pcof, wa, ref, family)
        wa.close()


# Ntot, N, Nc, Nfreq, nsteps, m, objFuncType, structure; options; family; full leakage weights
RANDOM = [
    ((40, 20, 2, 1, 7, 3, 3, False), {}, MFMA, False),                      # N > 16: k_terminal_parts (two slabs per sample)
    ((8, 3, 2, 2, 9, 2, 2, False), {"rowlane_max": 0}, 2, False),            # lane kernels: k_terminal_cols<LaneMap, EP_SV> at NP = 8
    ((6, 2, 1, 1, 11, 3, 1, False), {"rowlane_max": 0}, 2, False),           # ... at NP = 6, one gradient
    ((48, 4, 2, 1, 6, 3, 3, "t4"), {}, 6, True),                             # full leakage weights (jq_update_wmat; complex: quad layout)
    ((12, 4, 2, 1, 8, 2, 1, False), {}, 3, True),                            # ... on the row-lane kernels
]


@pytest.mark.parametrize("cfg,opts,family,wfull", RANDOM, ids=lambda v: None if not isinstance(v, tuple) or len(v) != 8 else "Ntot%d_N%d_o%d" % (v[0], v[1], v[6]))
def test_random_problems_parts_lane_and_full_weights(jq, cfg, opts, family, wfull):
    Ntot, N = cfg[0], cfg[1]
    rng = np.random.default_rng(4200 + Ntot * 31 + N)
    params, pcof = random_problem(jq, rng, *cfg)
    if wfull:
        from test_gpu_dense_wmat import set_forbidden
        set_forbidden(params, rng, 3)
    ref = References(params, pcof)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    check_every_type(jq, params, pcof, wa, ref, family)
    wa.close()


# ---- 2. ensembles: jq_eval_f_g_grad -----------------------------------------------------------------------------------------------------
def _ensemble(jq, params, pcof, wa, nodes, weights, shift):
    jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
    return dict(totalgrad=params.last_infidelity_grad + (params.last_leak_grad if params.last_leak_grad.size else 0.0),
                infidelgrad=params.last_infidelity_grad.copy(), leakgrad=params.last_leak_grad.copy(),
                primaryobjf=params.last_infidelity, secondaryobjf=params.last_leak)


def _check_ensemble(jq, params, pcof, nodes, weights, shift, options, family):
    """one D, many s: no per-sample alignment -- the general-D sum identity and type 4 are the checks"""
    ev = oracle_ensemble_eval(pcof, nodes, weights, shift)
    T, D = target_of(params), random_dvds(params)
    r1, ell, polar = ev(params), leak_part(params, ev), ref_polar(params, ev, D)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=options)
    try:
        out = {}
        for sv in (2, 3, 4):
            set_dvds(params, D, sv)
            out[sv] = _ensemble(jq, params, pcof, wa, nodes, weights, shift)
            assert wa.last_timing()["kernel_family"] in family, wa.last_timing()
            close("type %d infidelity" % sv, out[sv]["primaryobjf"], r1["primaryobjf"])
            close("type %d leak" % sv, out[sv]["secondaryobjf"], r1["secondaryobjf"])
        close("types 2 + 3 totalgrad", out[2]["totalgrad"] + out[3]["totalgrad"], polar + 2.0 * ell)
        close("type 4 totalgrad", out[4]["totalgrad"], polar + ell)
        # a same-device multi handle (two shards, host-side sum) against the single handle
        multi = jq.Working_Arrays_HIP(params, pcof.size, devices=2, options=dict(options or {}, multi_same_device=1))
        try:
            for sv in (2, 3):
                set_dvds(params, D, sv)
                m = _ensemble(jq, params, pcof, multi, nodes, weights, shift)
                assert multi.plan_info()["sv_type"] == sv
                close("multi handle, type %d totalgrad" % sv, m["totalgrad"], out[sv]["totalgrad"])
                close("multi handle, type %d infidelity" % sv, m["primaryobjf"], out[sv]["primaryobjf"])
        finally:
            multi.close()
    finally:
        set_dvds(params, T, 1)
        wa.close()


def test_swap02_risk_neutral_ensemble(jq):
    params, info, pcof, _ = case_inputs("swap02_rn")
    nq = 37
    x, w = np.polynomial.legendre.leggauss(nq)
    nodes, weights = x * 0.5 * 2 * np.pi * 2e-2, w * 0.5
    _check_ensemble(jq, params, pcof, nodes, weights, params.shift_weights_reference(), None, (2, 3))


def test_cnot3_ensemble_more_samples_than_a_slab_holds(jq):
    """N = 4: four samples per slab; 21 samples = several slabs, the last one ragged (sps > 1 in k_terminal)"""
    params, pcof = _cnot3_short()
    nodes, weights, shift = jq.cases.cnot3_ensemble(21)
    _check_ensemble(jq, params, pcof, nodes, weights, shift, {"cq": 0}, (6,))


# ---- 3. bit identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,opts", [("swap02", {}), ("cnot2-leakieq", {"lane": 0}), ("cnot2", {"rowlane_max": 0}), ("cnot3x300", {}),
                                       ("cnot3x300", {"quad": 0, "coop_max": 0})])
def test_dvds_equal_to_the_target_is_type_1_bit_for_bit(jq, case, opts):
    params, pcof = _inputs(case)
    T = target_of(params)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    try:
        first = run(jq, params, pcof, wa)
        for sv in (2, 3):
            set_dvds(params, T, sv)
            r = run(jq, params, pcof, wa)
            assert wa.plan_info()["sv_type"] == sv
            for k, v in first.items():
                assert np.array_equal(v, r[k]), (sv, k)
        # a real dVds, and back to 1: the first result again
        set_dvds(params, random_dvds(params), 2)
        other = run(jq, params, pcof, wa)
        assert not np.array_equal(other["totalgrad"], first["totalgrad"])
        params.sv_type = 1
        again = run(jq, params, pcof, wa)
        for k, v in first.items():
            assert np.array_equal(v, again[k]), k
    finally:
        set_dvds(params, T, 1)
        wa.close()


def test_update_target_leaves_dvds_alone(jq):
    """jq_update_target with sv_type 2: the result equals that of a fresh handle given the same (target, dVds) pair"""
    params, info, pcof, _ = case_inputs("cnot2")
    T, D = target_of(params), random_dvds(params)
    T2 = np.linalg.qr(T + 0.3 * random_dvds(params, 11))[0]
    wa = jq.Working_Arrays_HIP(params, pcof.size, options={"embed": 2})
    try:
        set_dvds(params, D, 2)
        run(jq, params, pcof, wa)
        params.Utarget_r, params.Utarget_i = np.asfortranarray(T2.real.copy()), np.asfortranarray(T2.imag.copy())      # (not change_target: plain mutation)
        moved = run(jq, params, pcof, wa)
        fresh_wa = jq.Working_Arrays_HIP(params, pcof.size, options={"embed": 2})
        fresh = run(jq, params, pcof, fresh_wa)
        fresh_wa.close()
        for k, v in fresh.items():
            assert np.array_equal(v, moved[k]), k
    finally:
        params.Utarget_r, params.Utarget_i = np.asfortranarray(T.real.copy()), np.asfortranarray(T.imag.copy())
        set_dvds(params, T, 1)
        wa.close()


# ---- 4. refusals, each provoked once ------------------------------------------------------------------------------------------------------
def test_invalid_arguments(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    params, info, pcof, _ = case_inputs("swap02")
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    h = wa.handle
    assert L.jq_get_sv_type(h) == 1
    for bad in (0, 5):
        assert L.jq_set_sv_type(h, bad) == _lib.JQ_EINVAL and b"jq_set_sv_type" in L.jq_last_error(h)
    d = np.zeros(params.Ntot * params.N)
    assert L.jq_update_dvds(h, None, d.ctypes.data_as(_lib.c_dp)) == _lib.JQ_EINVAL
    assert L.jq_update_dvds(h, d.ctypes.data_as(_lib.c_dp), None) == _lib.JQ_EINVAL
    assert L.jq_get_sv_type(h) == 1
    for ok in (4, 2, 1):
        assert L.jq_set_sv_type(h, ok) == _lib.JQ_OK and L.jq_get_sv_type(h) == ok
    wa.close()
    params.pFidType = 1
    with pytest.raises(ValueError, match="JQ_EUNSUPPORTED"):
        jq.Working_Arrays_HIP(params, pcof.size)


def test_implicit_midpoint_refuses_other_types_in_either_order(jq):
    from juqbox_jl_amd import _lib
    from oracle.oracle import Oracle
    L = _lib.load()
    params, info, pcof, _ = case_inputs("swap02")
    params.Integrator_id = jq.Implicit_Midpoint
    params.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=100, tol=1e-12, nrhs=params.N)
    r = Oracle(params).traceobjgrad_imr(pcof, 100, 1e-12)
    wa = jq.Working_Arrays_M_HIP(params, pcof.size)
    h = wa.handle
    first = run(jq, params, pcof, wa)                     # (sync_params sets the integrator)
    close("implicit midpoint totalgrad", first["totalgrad"], r["totalgrad"])
    # integrator first, type second
    assert L.jq_set_sv_type(h, 2) == _lib.JQ_EUNSUPPORTED
    assert b"implicit-midpoint" in L.jq_last_error(h) and b"sv_type" in L.jq_last_error(h)
    assert L.jq_get_sv_type(h) == 1
    # type first, integrator second
    assert L.jq_set_integrator(h, 1, 0, 0.0) == _lib.JQ_OK
    assert L.jq_set_sv_type(h, 2) == _lib.JQ_OK
    assert L.jq_set_integrator(h, 2, 100, 1e-12) == _lib.JQ_EUNSUPPORTED
    assert b"implicit-midpoint" in L.jq_last_error(h) and b"sv_type" in L.jq_last_error(h)
    # sv_type = 1: the handle evaluates as before
    assert L.jq_set_sv_type(h, 1) == _lib.JQ_OK
    assert L.jq_set_integrator(h, 2, 100, 1e-12) == _lib.JQ_OK
    again = run(jq, params, pcof, wa)
    for k, v in first.items():
        assert np.array_equal(v, again[k]), k
    # ... and through the mirror: the library's refusal surfaces as its error
    params.sv_type = 2
    with pytest.raises(_lib.JuqboxHipError) as e:
        run(jq, params, pcof, wa)
    assert e.value.code == _lib.JQ_EUNSUPPORTED
    params.sv_type = 1
    wa.close()


# ---- 5. the continuation script ------------------------------------------------------------------------------------------------------------
def test_mirrored_continuation_use(jq):
    """objparams(...; dVds = D) -> evaluate (type 2) -> set_adjoint_Sv_type(params, 3) -> evaluate -> change_target(params, T2) -> evaluate"""
    p0, info, pcof, _ = case_inputs("cnot2-leakieq")
    T = target_of(p0)
    Dp, rho = align(p0, pcof, random_dvds(p0))
    params = jq.objparams(p0.Ne, p0.Ng, p0.T, p0.nsteps, Uinit=p0.Uinit, Utarget=T, Cfreq=p0.Cfreq, Rfreq=p0.Rfreq, Hconst=p0.Hconst,
                          Hsym_ops=p0.Hsym_ops, Hanti_ops=p0.Hanti_ops, objFuncType=p0.objFuncType, leak_ubound=p0.leak_ubound,
                          linear_solver=p0.linear_solver, dVds=Dp)
    params.wmat_real = p0.wmat_real.copy()
    assert params.sv_type == 2
    ev = oracle_eval(pcof)
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    r = run(jq, params, pcof, wa)
    ref = ref_type2(p0, ev, Dp, rho)
    close("script, type 2 totalgrad", r["totalgrad"], ref["totalgrad"])
    close("script, type 2 infidelgrad", r["infidelgrad"], ref["infidelgrad"])
    jq.set_adjoint_Sv_type(params, 3)
    r = run(jq, params, pcof, wa)
    ref = ref_type3(p0, ev, rho)
    close("script, type 3 totalgrad", r["totalgrad"], ref["totalgrad"])
    close("script, type 3 infidelgrad", r["infidelgrad"], ref["infidelgrad"])
    # a new target while sv_type == 3: dVds stays (src/evalobjgrad.jl:1502-1505); the aligned construction for the NEW pair
    T2 = np.linalg.qr(T + 0.2 * random_dvds(p0, 13))[0]
    jq.change_target(params, T2)
    assert np.array_equal(params.dVds_r, Dp.real) and np.array_equal(params.Utarget_r, T2.real)
    p2 = with_target(p0, T2)
    Dq, rho2 = align(p2, pcof, Dp)
    set_dvds(params, Dq, 3)      # (the same dVds up to the phase the construction needs)
    r = run(jq, params, pcof, wa)
    ref = ref_type3(p2, ev, rho2)
    close("script, new target, type 3 totalgrad", r["totalgrad"], ref["totalgrad"])
    close("script, new target, objective", r["objfv"], ev(p2)["objfv"])
    wa.close()
