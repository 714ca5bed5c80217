"""GPU (-m gpu): jq_traceobjgrad_batch -- many control vectors of ONE problem in one call.

Two criteria, no others:
  (a) every column against the CPU oracle's traceobjgrad of that vector, per quantity, with conftest.reference_pass (atol 1e-14 or
      rtol 1e-10 in the 2-norm);
  (b) every column bit-identical (np.array_equal) to the single call traceobjgrad of that vector on a handle with the same options
      (cooperative quad: cq3=0, the one-workgroup backward kernel the grouped batch runs; row-lane: the default variant of both).
Time loops are shortened throughout (the two reference cases of the row-lane family excepted: milliseconds at full length)."""
import numpy as np
import pytest

from conftest import case_inputs, reference_pass
from test_gpu_random import random_problem

pytestmark = pytest.mark.gpu

NAMES = ("objfv", "totalgrad", "primaryobjf", "secondaryobjf", "traceInfidelity", "infidelgrad", "leakgrad")


def vectors(pcof, n, seed, scale=0.05):
    """pcof and n - 1 seeded perturbations of it"""
    rng = np.random.default_rng(seed)
    amp = scale * max(1.0, float(np.max(np.abs(pcof))))
    return [np.array(pcof, dtype=np.float64)] + [pcof + amp * rng.standard_normal(pcof.size) for _ in range(n - 1)]


def batch(jq, vecs, params, wa):
    return dict(zip(NAMES, jq.traceobjgrad_batch(vecs, params, wa, True)))


def single(jq, v, params, wa):
    return dict(zip(NAMES, jq.traceobjgrad(v, params, wa, False, True)))


def column(b, i):
    return {k: (b[k][i] if b[k].ndim == 1 else b[k][:, i]) for k in NAMES}


def same_bits(tag, col, ref):
    for k in NAMES:
        assert np.array_equal(np.asarray(col[k]), np.asarray(ref[k])), (tag, k, col[k], ref[k])


def check_oracle(tag, params, v, col):
    from oracle.oracle import Oracle
    r = Oracle(params, use_sparse=bool(getattr(params, "use_sparse", False))).traceobjgrad(v)
    for k in NAMES:
        if k == "leakgrad" and params.objFuncType == 1:
            assert np.size(col[k]) == 0
            continue
        d = np.linalg.norm(np.atleast_1d(col[k]) - np.atleast_1d(r[k]))
        print("    %-28s %-16s |diff| %.3e  |ref| %.3e" % (tag, k, d, np.linalg.norm(np.atleast_1d(r[k]))))
        assert reference_pass(col[k], r[k]), (tag, k)


def check_batch(jq, params, vecs, options, family, mode="grouped", oracle=True, single_options=None):
    """criteria (a) and (b), cross-talk (the same vector first and last) and a permuted batch; returns the batch result"""
    n = len(vecs)
    wa = jq.Working_Arrays_HIP(params, vecs[0].size, options=options)
    ws = wa if single_options is None else jq.Working_Arrays_HIP(params, vecs[0].size, options=single_options)
    try:
        b = batch(jq, vecs, params, wa)
        info = wa.plan_info()["pcof_batch"]
        print("  pcof_batch:", info, "family", wa.last_timing()["kernel_family"])
        assert info["mode"] == mode, info
        if family is not None:
            assert wa.last_timing()["kernel_family"] == family, wa.last_timing()
        assert b["objfv"].shape == (n,) and b["totalgrad"].shape == (vecs[0].size, n)
        assert b["leakgrad"].shape == ((0, n) if params.objFuncType == 1 else (vecs[0].size, n))
        for i, v in enumerate(vecs):
            same_bits("column %d against the single call" % i, column(b, i), single(jq, v, params, ws))
            if oracle:
                check_oracle("column %d" % i, params, v, column(b, i))
        # cross-talk: the first vector again behind all the others, and a permutation
        c = batch(jq, vecs + [vecs[0]], params, wa)
        same_bits("first and last column", column(c, n), column(c, 0))
        for i in range(n):
            same_bits("longer batch, column %d" % i, column(c, i), column(b, i))
        perm = list(np.random.default_rng(n).permutation(n))
        p = batch(jq, [vecs[j] for j in perm], params, wa)
        for i, j in enumerate(perm):
            same_bits("permuted batch, column %d" % i, column(p, i), column(b, j))
        return b
    finally:
        wa.close()
        if ws is not wa:
            ws.close()


def cnot3_short(nsteps=300):
    params, info, pcof, _ = case_inputs("cnot3")
    params.nsteps = nsteps
    params.T = params.T * nsteps / 32386
    return params, pcof


# ---- 1. row-lane kernels (family 3) ------------------------------------------------------------------------------------------------------
def test_rowlane_swap02_full_length(jq):
    params, info, pcof, _ = case_inputs("swap02")      # N = 3: three columns per wave in the grouped batch, four slots in the single call
    check_batch(jq, params, vectors(pcof, 5, 11), None, 3)


def test_rowlane_two_sweeps_and_lds_constant_images(jq):
    params, info, pcof, _ = case_inputs("cnot2-leakieq")      # objFuncType 3: forced and unforced sweep; NPJ = 12
    check_batch(jq, params, vectors(pcof, 3, 12), None, 3)


def test_rowlane_two_columns_never_share_a_wave(jq):
    rng = np.random.default_rng(1301)
    params, pcof = random_problem(jq, rng, 6, 2, 1, 1, 11, 3, 1, False)
    check_batch(jq, params, vectors(pcof, 5, 13), None, 3)


# ---- 2. cooperative-quad kernels (family 8) ------------------------------------------------------------------------------------------------
def test_cq_cnot3_five_vectors(jq):
    params, pcof = cnot3_short()
    check_batch(jq, params, vectors(pcof, 5, 21), {"cq3": 0}, 8)      # 5: not a multiple of the four quads of a slab


def test_cq_cnot3_chunks_hand_over_with_group_strides(jq):
    params, pcof = cnot3_short(60)
    # 7 steps per chunk in the batch as in the single call: nine chunks (the last one of four steps) with five streams each
    opts = {"cq3": 0, "chunk_steps": 7, "stream_bytes": 3 << 20}
    check_batch(jq, params, vectors(pcof, 5, 22), opts, 8)
    # ... and 40 vectors, whose streams leave the same budget two steps per chunk: shorter chunks than the single call's sum the gradient
    # (k_gradacc adds chunk by chunk) and the leak integral (the forward kernel adds its lanes' partial sums at the end of a chunk) in
    # another order, so this run is held to criterion (a); the state passes from chunk to chunk exactly, so the infidelity keeps its bits
    vecs = vectors(pcof, 40, 23)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    try:
        t = batch(jq, vecs, params, wa)
        assert wa.plan_info()["pcof_batch"]["mode"] == "grouped" and wa.last_timing()["n_forward_launches"] > (60 + 6) // 7
        for i in (0, 19, 39):
            check_oracle("short chunks, column %d" % i, params, vecs[i], column(t, i))
            r = single(jq, vecs[i], params, wa)
            for k in ("objfv", "primaryobjf", "secondaryobjf", "traceInfidelity"):
                print("    short chunks, column %d %-16s batch %.17g single call %.17g" % (i, k, t[k][i], r[k]))
            for k in ("primaryobjf", "traceInfidelity"):
                assert t[k][i] == r[k], (k, i)
    finally:
        wa.close()


@pytest.mark.parametrize("N", [2, 8])
def test_cq_random_t4_quads_per_vector(jq, N):
    """N = 2: a column quad of its own per vector (half of it padding); N = 8: two consecutive quads, trace rows summed in the single call's order"""
    rng = np.random.default_rng(2300 + N)
    params, pcof = random_problem(jq, rng, 32, N, 2, 1, 14, 3, 2, "t4")
    check_batch(jq, params, vectors(pcof, 3, 23 + N), {"cq3": 0}, 8)


def test_cq_dense_policy(jq):
    rng = np.random.default_rng(2401)
    params, pcof = random_problem(jq, rng, 24, 4, 2, 1, 12, 3, 1, False)
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    assert wa.plan_info()["structure"] != "t4"
    wa.close()
    check_batch(jq, params, vectors(pcof, 3, 24), {"cq3": 0}, 8)


# ---- 4. rounds -----------------------------------------------------------------------------------------------------------------------------
def test_rounds_of_two_equal_one_launch(jq):
    params, pcof = cnot3_short(100)
    vecs = vectors(pcof, 5, 41)
    w1 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    w2 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0, "pcof_batch_max": 2})
    try:
        b1, b2 = batch(jq, vecs, params, w1), batch(jq, vecs, params, w2)
        i1, i2 = w1.plan_info()["pcof_batch"], w2.plan_info()["pcof_batch"]
        assert i1["mode"] == i2["mode"] == "grouped" and i1["vectors_per_launch"] == 5 and i2["vectors_per_launch"] == 2
        assert w2.last_timing()["n_forward_launches"] == 3 * w1.last_timing()["n_forward_launches"]      # three launches
        for i in range(5):
            same_bits("rounds of two, column %d" % i, column(b2, i), column(b1, i))
    finally:
        w1.close()
        w2.close()


def test_one_more_vector_than_compute_units(jq):
    rng = np.random.default_rng(4201)
    params, pcof = random_problem(jq, rng, 32, 4, 2, 1, 20, 3, 1, "t4")
    wa = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    try:
        n = wa.num_compute_units + 1
        vecs = vectors(pcof, n, 42)
        b = batch(jq, vecs, params, wa)
        info = wa.plan_info()["pcof_batch"]
        assert info["mode"] == "grouped" and info["vectors_per_launch"] == n - 1 and wa.last_timing()["kernel_family"] == 8
        for i in range(n):
            same_bits("column %d" % i, column(b, i), single(jq, vecs[i], params, wa))
        for i in (0, n - 2, n - 1):      # (first launch: first and last vector; second launch: its only one)
            check_oracle("column %d" % i, params, vecs[i], column(b, i))
    finally:
        wa.close()


# ---- 5. routes without grouped streams: one vector after the other ------------------------------------------------------------------------------
def test_sequential_cooperative_kernels(jq):
    rng = np.random.default_rng(5101)
    params, pcof = random_problem(jq, rng, 40, 4, 2, 1, 9, 3, 2, False)
    check_batch(jq, params, vectors(pcof, 3, 51), None, 1, mode="sequential", oracle=False)


def test_sequential_implicit_midpoint(jq):
    params, info, pcof, _ = case_inputs("swap02")
    params.Integrator_id = jq.Implicit_Midpoint
    params.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=100, tol=1e-12, nrhs=params.N)
    vecs = vectors(pcof, 3, 52)
    wa = jq.Working_Arrays_M_HIP(params, pcof.size)
    try:
        b = batch(jq, vecs, params, wa)
        assert wa.plan_info()["pcof_batch"]["mode"] == "sequential"
        for i, v in enumerate(vecs):
            same_bits("column %d" % i, column(b, i), single(jq, v, params, wa))
    finally:
        wa.close()


def test_sequential_quad_layout(jq):
    params, pcof = cnot3_short()
    check_batch(jq, params, vectors(pcof, 3, 53), {"cq": 0}, 6, mode="sequential", oracle=False)


# ---- 6. settings follow the handle ----------------------------------------------------------------------------------------------------------
def test_sv_type_4_with_random_dvds(jq):
    from test_svtype_host import random_dvds
    params, info, pcof, _ = case_inputs("swap02")
    D = random_dvds(params)
    params.dVds_r, params.dVds_i, params.sv_type = np.asfortranarray(D.real.copy()), np.asfortranarray(D.imag.copy()), 4
    b = check_batch(jq, params, vectors(pcof, 3, 61), None, 3, oracle=False)
    params.sv_type = 1
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    r1 = single(jq, pcof, params, wa)
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
    check_batch(jq, params, vectors(pcof, 3, 62), None, 3, oracle=False)


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    params, info, pcof, _ = case_inputs("swap02")
    n = pcof.size
    vecs = vectors(pcof, 3, 71)
    wa = jq.Working_Arrays_HIP(params, n)
    try:
        wa.sync_params()
        P = np.ascontiguousarray(np.stack(vecs))
        ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
        # forward only, NULL gradients
        out = np.zeros((3, 4))
        assert L.jq_traceobjgrad_batch(wa.handle, ptr(P), n, 3, 0, ptr(out), None, None, None) == _lib.JQ_OK
        objfv, prim, sec = jq.traceobjgrad_batch(vecs, params, wa, False)
        assert np.array_equal(objfv, out[:, 0]) and np.array_equal(prim, out[:, 1]) and np.array_equal(sec, out[:, 2])
        for i, v in enumerate(vecs):
            o1 = jq.traceobjgrad(v, params, wa, False, False)
            assert (objfv[i], prim[i], sec[i]) == tuple(o1)
        # refusals: the single call's codes, nothing written
        mark = 7.25
        out[:] = mark
        tg, ig, lg = np.full((3, n), mark), np.full((3, n), mark), np.full((3, n), mark)
        o1, g1 = np.full(4, mark), np.full(n, mark)
        for ncoeff in (n - 1, 2):      # (an odd count; fewer than three coefficients per control function)
            rc1 = L.jq_traceobjgrad(wa.handle, ptr(P), ncoeff, 1, ptr(o1), ptr(g1), ptr(g1), ptr(g1))
            rcb = L.jq_traceobjgrad_batch(wa.handle, ptr(P), ncoeff, 2, 1, ptr(out), ptr(tg), ptr(ig), ptr(lg))
            print("    ncoeff %d: single %d, batch %d" % (ncoeff, rc1, rcb))
            assert rc1 != _lib.JQ_OK and rcb == rc1
        assert L.jq_traceobjgrad_batch(wa.handle, ptr(P), n, 0, 1, ptr(out), ptr(tg), ptr(ig), ptr(lg)) == _lib.JQ_EINVAL
        assert L.jq_traceobjgrad_batch(wa.handle, ptr(P), n, -3, 1, ptr(out), ptr(tg), ptr(ig), ptr(lg)) == _lib.JQ_EINVAL
        assert L.jq_traceobjgrad_batch(wa.handle, None, n, 3, 1, ptr(out), ptr(tg), ptr(ig), ptr(lg)) == _lib.JQ_EINVAL
        assert L.jq_traceobjgrad_batch(wa.handle, ptr(P), n, 3, 1, None, ptr(tg), ptr(ig), ptr(lg)) == _lib.JQ_EINVAL
        assert L.jq_traceobjgrad_batch(wa.handle, ptr(P), n, 3, 1, ptr(out), ptr(tg), None, ptr(lg)) == _lib.JQ_EINVAL
        for a in (out, tg, ig, lg):
            assert np.all(a == mark)
    finally:
        wa.close()


# ---- 8. multi-device handles ------------------------------------------------------------------------------------------------------------------
def test_multi_device_handle_shards_the_vectors(jq):
    params, pcof = cnot3_short(100)
    vecs = vectors(pcof, 5, 81)
    w1 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    wm = jq.Working_Arrays_HIP(params, pcof.size, devices=2, options={"cq3": 0, "multi_same_device": 1})
    try:
        b1, bm = batch(jq, vecs, params, w1), batch(jq, vecs, params, wm)
        for i in range(5):
            same_bits("multi-device handle, column %d" % i, column(bm, i), column(b1, i))
    finally:
        w1.close()
        wm.close()


# ---- 9. gradient_check --------------------------------------------------------------------------------------------------------------------------
def test_gradient_check_is_one_batch_of_central_differences(jq):
    params, info, pcof, _ = case_inputs("swap02")
    ks, h = [0, 5, pcof.size - 1], 1e-6
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    try:
        g, fd = jq.gradient_check(pcof, params, wa, ks, h)
        assert wa.plan_info()["pcof_batch"]["mode"] == "grouped"
        r = single(jq, pcof, params, wa)
        assert np.array_equal(g, r["totalgrad"][ks])
        for j, k in enumerate(ks):
            vp, vm = pcof.copy(), pcof.copy()
            vp[k] += h
            vm[k] -= h
            fp, fm = single(jq, vp, params, wa)["objfv"], single(jq, vm, params, wa)["objfv"]
            assert fd[j] == (fp - fm) / (2.0 * h), (k, fd[j], (fp - fm) / (2.0 * h))
            print("    k = %d: adjoint %.10e, central difference %.10e" % (k, g[j], fd[j]))
    finally:
        wa.close()
