"""GPU (-m gpu): jq_eval_f_g_grad_batch -- the risk-neutral ensemble of ONE set of nodes for many control vectors in one call.

Two criteria, no others:
  (a) per vector the infidelity sum, the leak sum and each gradient against the CPU oracle's eval_f_g_grad of that vector, with
      conftest.reference_pass (atol 1e-14 or rtol 1e-10 in the 2-norm);
  (b) every column bit-identical (np.array_equal) to the single call eval_f_g_grad of that vector, and node_out to traceobj_sweep, on a
      handle with the same options (cooperative quad: cq3=0, the one-workgroup backward kernel the grouped batch runs; row-lane: the
      default variant of both) and the same chunk length.
Nodes lie in [-1, 1]; the weights are unequal, positive and sum to 1.  Time loops are shortened throughout (the reference cases of the
row-lane family excepted: milliseconds at full length)."""
import numpy as np
import pytest

from conftest import case_inputs, reference_pass
from test_gpu_pcof_batch import cnot3_short, vectors
from test_gpu_random import random_problem

pytestmark = pytest.mark.gpu

NAMES = ("infidelity", "leak", "infid_grad", "leak_grad")


def ensemble(nq, seed):
    """nq nodes in [-1, 1], nq unequal positive weights that sum to 1"""
    rng = np.random.default_rng(seed)
    nodes = rng.uniform(-1.0, 1.0, nq)
    w = 0.25 + rng.random(nq)
    return nodes, w / w.sum()


def small_shift(params, seed):
    """a per-level factor for problems whose level count overflows the reference's 0.01 * 10^(j-2)"""
    s = 0.05 * np.random.default_rng(seed).standard_normal(params.Ntot)
    s[0] = 0.0
    return s


def batch(jq, vecs, params, wa, nodes, weights, shift, adjoint=True):
    r = jq.eval_f_g_grad_batch(vecs, params, wa, nodes, weights, adjoint, shift=shift, per_node=True)
    b = dict(zip(NAMES, r[:4]))
    b["node_out"] = r[4]
    return b


def single(jq, v, params, wa, nodes, weights, shift, adjoint=True):
    """eval_f_g_grad and traceobj_sweep of one vector (the memoised results, copied)"""
    jq.eval_f_g_grad(v, params, wa, nodes, weights, adjoint, shift=shift)
    r = dict(infidelity=params.last_infidelity, leak=params.last_leak, infid_grad=params.last_infidelity_grad.copy(),
             leak_grad=params.last_leak_grad.copy())
    r["node_out"] = jq.traceobj_sweep(v, params, wa, nodes, shift=shift).T.copy()      # [4, nquad]
    return r


def column(b, i):
    c = {k: (b[k][i] if b[k].ndim == 1 else b[k][:, i]) for k in NAMES}
    c["node_out"] = b["node_out"][:, :, i]
    return c


def same_bits(tag, col, ref, names=NAMES + ("node_out",)):
    for k in names:
        assert np.array_equal(np.asarray(col[k]), np.asarray(ref[k])), (tag, k, col[k], ref[k])


def oracle_ref(params, v, nodes, weights, shift):
    from oracle.oracle import Oracle
    sh = params.shift_weights_reference() if shift is None else shift
    r = Oracle(params, use_sparse=bool(getattr(params, "use_sparse", False))).eval_f_g_grad(v, nodes, weights, sh)
    return dict(infidelity=r["last_infidelity"], leak=r["last_leak"], infid_grad=r["last_infidelity_grad"], leak_grad=r["last_leak_grad"])


def check_oracle(tag, params, col, r):
    for k in NAMES:
        if k == "leak_grad" and params.objFuncType == 1:
            assert np.size(col[k]) == 0
            continue
        d = np.linalg.norm(np.atleast_1d(col[k]) - np.atleast_1d(r[k]))
        print("    %-28s %-12s |diff| %.3e  |ref| %.3e" % (tag, k, d, np.linalg.norm(np.atleast_1d(r[k]))))
        assert reference_pass(col[k], r[k]), (tag, k)


def check_batch(jq, params, vecs, nq, options, family, mode="grouped", oracle=True, shift=None, make=None, seed=5):
    """criteria (a) and (b), cross-talk (the same vector first and last) and a permuted batch; returns the batch result"""
    n = len(vecs)
    nodes, weights = ensemble(nq, seed)
    wa = (make or jq.Working_Arrays_HIP)(params, vecs[0].size, options=options)
    try:
        b = batch(jq, vecs, params, wa, nodes, weights, shift)
        info = wa.plan_info()["pcof_batch"]
        print("  pcof_batch:", info, "family", wa.last_timing()["kernel_family"])
        assert info["mode"] == mode and info["nodes_per_vector"] == nq, info
        if family is not None:
            assert wa.last_timing()["kernel_family"] == family, wa.last_timing()
        m = vecs[0].size
        assert b["infidelity"].shape == (n,) and b["leak"].shape == (n,) and b["infid_grad"].shape == (m, n)
        assert b["leak_grad"].shape == ((0, n) if params.objFuncType == 1 else (m, n)) and b["node_out"].shape == (4, nq, n)
        for i, v in enumerate(vecs):
            same_bits("column %d against the single calls" % i, column(b, i), single(jq, v, params, wa, nodes, weights, shift))
            if oracle:
                check_oracle("column %d" % i, params, column(b, i), oracle_ref(params, v, nodes, weights, shift))
        # cross-talk: the first vector again behind all the others, and a permutation
        c = batch(jq, vecs + [vecs[0]], params, wa, nodes, weights, shift)
        same_bits("first and last column", column(c, n), column(c, 0))
        for i in range(n):
            same_bits("longer batch, column %d" % i, column(c, i), column(b, i))
        perm = list(np.random.default_rng(n).permutation(n))
        p = batch(jq, [vecs[j] for j in perm], params, wa, nodes, weights, shift)
        for i, j in enumerate(perm):
            same_bits("permuted batch, column %d" % i, column(p, i), column(b, j))
        return b
    finally:
        wa.close()


# ---- 1 - 4. row-lane kernels (family 3) --------------------------------------------------------------------------------------------------
def test_rowlane_swap02_a_vector_is_exactly_three_waves(jq):
    params, info, pcof, _ = case_inputs("swap02")      # N = 3, Q = 4: twelve columns
    check_batch(jq, params, vectors(pcof, 3, 111), 4, None, 3)


def test_rowlane_swap02_one_padding_slot_ends_each_vector(jq):
    params, info, pcof, _ = case_inputs("swap02")      # Q = 5: fifteen columns on four waves
    check_batch(jq, params, vectors(pcof, 3, 112), 5, None, 3)


def test_rowlane_two_columns_two_padding_slots_per_vector(jq):
    rng = np.random.default_rng(1301)
    params, pcof = random_problem(jq, rng, 6, 2, 1, 1, 11, 3, 1, False)      # N = 2, Q = 5: ten columns on three waves
    check_batch(jq, params, vectors(pcof, 3, 113), 5, None, 3, shift=small_shift(params, 13))


def test_rowlane_forced_and_unforced_sweep(jq):
    params, info, pcof, _ = case_inputs("cnot2-leakieq")      # objFuncType 3
    check_batch(jq, params, vectors(pcof, 2, 114), 3, None, 3, shift=small_shift(params, 14))


# ---- 5. cooperative-quad kernels (family 8) ------------------------------------------------------------------------------------------------
def test_cq_cnot3_three_quads_per_vector(jq):
    params, pcof = cnot3_short(300)
    check_batch(jq, params, vectors(pcof, 5, 121), 3, {"cq3": 0}, 8, shift=small_shift(params, 21))


@pytest.mark.parametrize("N, nq", [(2, 3), (8, 2)])
def test_cq_random_t4(jq, N, nq):
    """N = 2, Q = 3: six columns, one padding sample ends the vector's second quad; N = 8, Q = 2: four quads"""
    rng = np.random.default_rng(2300 + N)
    params, pcof = random_problem(jq, rng, 32, N, 2, 1, 14, 3, 2, "t4")
    check_batch(jq, params, vectors(pcof, 3, 122 + N), nq, {"cq3": 0}, 8, shift=small_shift(params, 22 + N))


def test_cq_dense_policy(jq):
    rng = np.random.default_rng(2401)
    params, pcof = random_problem(jq, rng, 24, 4, 2, 1, 12, 3, 1, False)
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    assert wa.plan_info()["structure"] != "t4"
    wa.close()
    check_batch(jq, params, vectors(pcof, 3, 124), 2, {"cq3": 0}, 8, shift=small_shift(params, 24))


# ---- 6. chunk hand-over --------------------------------------------------------------------------------------------------------------------
def test_cq_chunks_hand_over_with_group_strides(jq):
    params, pcof = cnot3_short(60)
    # 7 steps per chunk in the batch as in the single calls: nine chunks (the last one of four steps) with three streams each
    opts = {"cq3": 0, "chunk_steps": 7, "stream_bytes": 3 << 20}
    vecs, shift = vectors(pcof, 3, 131), small_shift(params, 31)
    nodes, weights = ensemble(2, 5)
    check_batch(jq, params, vecs, 2, opts, 8, oracle=False, shift=shift)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    try:
        batch(jq, vecs, params, wa, nodes, weights, shift)
        nb = wa.last_timing()["n_forward_launches"]
        jq.eval_f_g_grad(vecs[0], params, wa, nodes, weights, True, shift=shift)
        assert nb == wa.last_timing()["n_forward_launches"] == (60 + 6) // 7      # (the same chunk length: criterion (b) applies)
    finally:
        wa.close()


# ---- 7. rounds -----------------------------------------------------------------------------------------------------------------------------
def test_rounds_of_two_equal_one_launch(jq):
    params, pcof = cnot3_short(100)
    vecs, shift = vectors(pcof, 5, 141), small_shift(params, 41)
    nodes, weights = ensemble(2, 6)
    w1 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    w2 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0, "pcof_batch_max": 2})
    try:
        b1, b2 = batch(jq, vecs, params, w1, nodes, weights, shift), batch(jq, vecs, params, w2, nodes, weights, shift)
        i1, i2 = w1.plan_info()["pcof_batch"], w2.plan_info()["pcof_batch"]
        print("  ", i1, i2)
        assert i1["mode"] == i2["mode"] == "grouped" and i1["vectors_per_launch"] >= 5 and i2["vectors_per_launch"] == 2
        assert i1["nodes_per_vector"] == i2["nodes_per_vector"] == 2
        assert w2.last_timing()["n_forward_launches"] == 3 * w1.last_timing()["n_forward_launches"]      # ceil(5 / 2) launches
        for i in range(5):
            same_bits("rounds of two, column %d" % i, column(b2, i), column(b1, i))
        jq.traceobjgrad_batch(vecs, params, w1, False)
        assert w1.plan_info()["pcof_batch"]["nodes_per_vector"] == 1
    finally:
        w1.close()
        w2.close()


# ---- 8. cross-talk: a node that weighs nothing (first vector repeated, permutation: check_batch) -----------------------------------------------
def test_a_node_of_weight_zero_adds_nothing_and_is_still_reported(jq):
    params, info, pcof, _ = case_inputs("swap02")
    vecs = vectors(pcof, 3, 151)
    nodes, w = ensemble(3, 7)
    w[1] = 0.0
    w /= w.sum()
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    try:
        b = batch(jq, vecs, params, wa, nodes, w, None)
        assert wa.plan_info()["pcof_batch"]["mode"] == "grouped"
        for i, v in enumerate(vecs):
            same_bits("column %d" % i, column(b, i), single(jq, v, params, wa, nodes, w, None))      # (node_out: all three nodes)
            check_oracle("column %d, without the node" % i, params, column(b, i), oracle_ref(params, v, nodes[[0, 2]], w[[0, 2]], None))
            assert b["node_out"][1, 1, i] > 0.0
    finally:
        wa.close()


# ---- 9. one node at 0 with weight 1 is jq_traceobjgrad_batch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["swap02", "cnot3"])
def test_single_node_reproduces_traceobjgrad_batch(jq, case):
    if case == "cnot3":
        params, pcof = cnot3_short(100)
        opts = {"cq3": 0}
    else:
        params, info, pcof, _ = case_inputs(case)
        opts = None
    vecs = vectors(pcof, 3, 161)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options=opts)
    try:
        b = batch(jq, vecs, params, wa, [0.0], [1.0], None)
        assert wa.plan_info()["pcof_batch"]["mode"] == "grouped"
        objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad_batch(vecs, params, wa, True)
        assert np.array_equal(b["infidelity"], prim) and np.array_equal(b["leak"], sec)
        assert np.array_equal(b["infid_grad"], ig) and np.array_equal(b["leak_grad"], lg)
        assert np.array_equal(b["node_out"][:, 0, :], np.stack([objfv, prim, sec, tinf]))
    finally:
        wa.close()


# ---- 10. custom shift, forward only ------------------------------------------------------------------------------------------------------------
def test_custom_shift_and_forward_only_with_null_gradients(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    params, info, pcof, _ = case_inputs("swap02")
    n = pcof.size
    vecs = vectors(pcof, 3, 171)
    shift = small_shift(params, 71)
    nodes, weights = ensemble(5, 8)
    b = check_batch(jq, params, vecs, 5, None, 3, shift=shift, seed=8)
    b0 = check_batch(jq, params, vecs, 5, None, 3, oracle=False, seed=8)
    assert not np.array_equal(b["infidelity"], b0["infidelity"])      # (the shift was in force)
    wa = jq.Working_Arrays_HIP(params, n)
    try:
        wa.sync_params()
        P = np.ascontiguousarray(np.stack(vecs))
        ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
        out2, node_out = np.zeros((3, 2)), np.zeros((3, 5, 4))
        assert L.jq_eval_f_g_grad_batch(wa.handle, ptr(P), n, 3, ptr(nodes), ptr(weights), 5, ptr(shift), 0, ptr(out2), None, None,
                                        ptr(node_out)) == _lib.JQ_OK
        f = batch(jq, vecs, params, wa, nodes, weights, shift, adjoint=False)
        assert np.array_equal(f["infidelity"], out2[:, 0]) and np.array_equal(f["leak"], out2[:, 1])
        assert np.array_equal(f["node_out"], node_out.transpose(2, 1, 0))
        assert np.all(f["infid_grad"] == 0.0) and f["infid_grad"].shape == (n, 3)
        for i, v in enumerate(vecs):
            same_bits("forward only, column %d" % i, column(f, i), single(jq, v, params, wa, nodes, weights, shift, adjoint=False),
                      names=("infidelity", "leak", "node_out"))
        out2[:] = 0.0      # node_out may be NULL too
        assert L.jq_eval_f_g_grad_batch(wa.handle, ptr(P), n, 3, ptr(nodes), ptr(weights), 5, ptr(shift), 0, ptr(out2), None, None,
                                        None) == _lib.JQ_OK
        assert np.array_equal(f["infidelity"], out2[:, 0]) and np.array_equal(f["leak"], out2[:, 1])
    finally:
        wa.close()


# ---- 11. routes without grouped streams: one ensemble evaluation per vector ---------------------------------------------------------------------
def test_sequential_implicit_midpoint(jq):
    params, info, pcof, _ = case_inputs("swap02")
    params.Integrator_id = jq.Implicit_Midpoint
    params.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=100, tol=1e-12, nrhs=params.N)
    check_batch(jq, params, vectors(pcof, 3, 181), 3, None, None, mode="sequential", oracle=False, make=jq.Working_Arrays_M_HIP)


def test_sequential_quad_layout(jq):
    params, pcof = cnot3_short(100)
    check_batch(jq, params, vectors(pcof, 3, 182), 2, {"cq": 0}, 6, mode="sequential", oracle=False, shift=small_shift(params, 82))


def test_sequential_jacobi_solver(jq):
    params, info, pcof, _ = case_inputs("cnot2-jacobi")
    params.T = params.T * 200 / params.nsteps
    params.nsteps = 200
    check_batch(jq, params, vectors(pcof, 2, 183), 3, None, None, mode="sequential", shift=small_shift(params, 83))


# ---- 12. settings follow the handle ----------------------------------------------------------------------------------------------------------
def test_sv_type_4_with_random_dvds(jq):
    from test_svtype_host import leak_part, oracle_ensemble_eval, random_dvds, ref_polar
    params, info, pcof, _ = case_inputs("swap02")
    assert params.objFuncType == 1      # (infid_grad stores the total gradient)
    D = random_dvds(params)
    vecs = vectors(pcof, 3, 191)
    nodes, weights = ensemble(3, 5)
    sh = params.shift_weights_reference()
    refs = []
    for v in vecs:      # the oracle knows type 1: type 4 = (g(T + D) - g(T - D)) / 2 + l (tests/test_svtype_host.py), the objective is type 1's
        ev = oracle_ensemble_eval(v, nodes, weights, sh)
        r1 = ev(params)
        refs.append(dict(infidelity=r1["primaryobjf"], leak=r1["secondaryobjf"], infid_grad=ref_polar(params, ev, D) + leak_part(params, ev)))
    params.dVds_r, params.dVds_i, params.sv_type = np.asfortranarray(D.real.copy()), np.asfortranarray(D.imag.copy()), 4
    b = check_batch(jq, params, vecs, 3, None, 3, oracle=False)
    for i in range(3):
        for k in ("infidelity", "leak", "infid_grad"):
            d = np.linalg.norm(np.atleast_1d(column(b, i)[k]) - np.atleast_1d(refs[i][k]))
            print("    sv_type 4, column %d %-12s |diff| %.3e  |ref| %.3e" % (i, k, d, np.linalg.norm(np.atleast_1d(refs[i][k]))))
            assert reference_pass(column(b, i)[k], refs[i][k]), (i, k)
    params.sv_type = 1
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    r1 = single(jq, pcof, params, wa, nodes, weights, None)
    wa.close()
    assert b["infidelity"][0] == r1["infidelity"] and not np.array_equal(b["infid_grad"][:, 0], r1["infid_grad"])      # (the type was in force)


def test_full_leakage_weights_on_the_rowlane_kernels(jq):
    from test_gpu_dense_wmat import set_forbidden
    from test_gpu_svtype import RANDOM
    cfg = RANDOM[4][0]
    assert cfg[0] == 12 and RANDOM[4][3]
    rng = np.random.default_rng(4200 + cfg[0] * 31 + cfg[1])
    params, pcof = random_problem(jq, rng, *cfg)
    set_forbidden(params, rng, 3)
    check_batch(jq, params, vectors(pcof, 3, 192), 3, None, 3, shift=small_shift(params, 92))


# ---- 13. arguments ----------------------------------------------------------------------------------------------------------------------------
def test_arguments_and_refusals(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    params, info, pcof, _ = case_inputs("swap02")
    n = pcof.size
    vecs = vectors(pcof, 3, 201)
    nodes, weights = ensemble(2, 9)
    wa = jq.Working_Arrays_HIP(params, n)
    try:
        wa.sync_params()
        P = np.ascontiguousarray(np.stack(vecs))
        ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
        mark = 7.25
        out2, ig, lg, no = np.full((3, 2), mark), np.full((3, n), mark), np.full((3, n), mark), np.full((3, 2, 4), mark)
        o1, g1 = np.full(2, mark), np.full(n, mark)
        call = lambda pc, ncoeff, npcof, nd, wt, nq, adj, o2, a, b, c: L.jq_eval_f_g_grad_batch(wa.handle, pc, ncoeff, npcof, nd, wt, nq, None, adj, o2, a, b, c)
        for ncoeff in (n - 1, 2):      # (an odd count; fewer than three coefficients per control function): the single call's codes
            rc1 = L.jq_eval_f_g_grad(wa.handle, ptr(P), ncoeff, ptr(nodes), ptr(weights), 2, None, 1, ptr(o1), ptr(g1), ptr(g1))
            rcb = call(ptr(P), ncoeff, 2, ptr(nodes), ptr(weights), 2, 1, ptr(out2), ptr(ig), ptr(lg), ptr(no))
            print("    ncoeff %d: single %d, batch %d" % (ncoeff, rc1, rcb))
            assert rc1 != _lib.JQ_OK and rcb == rc1
        E = _lib.JQ_EINVAL
        assert call(ptr(P), n, 0, ptr(nodes), ptr(weights), 2, 1, ptr(out2), ptr(ig), ptr(lg), ptr(no)) == E
        assert call(ptr(P), n, -3, ptr(nodes), ptr(weights), 2, 1, ptr(out2), ptr(ig), ptr(lg), ptr(no)) == E
        assert call(ptr(P), n, 3, ptr(nodes), ptr(weights), 0, 1, ptr(out2), ptr(ig), ptr(lg), ptr(no)) == E
        assert call(ptr(P), n, 3, ptr(nodes), ptr(weights), -1, 1, ptr(out2), ptr(ig), ptr(lg), ptr(no)) == E
        assert call(None, n, 3, ptr(nodes), ptr(weights), 2, 1, ptr(out2), ptr(ig), ptr(lg), ptr(no)) == E
        assert call(ptr(P), n, 3, None, ptr(weights), 2, 1, ptr(out2), ptr(ig), ptr(lg), ptr(no)) == E
        assert call(ptr(P), n, 3, ptr(nodes), None, 2, 1, ptr(out2), ptr(ig), ptr(lg), ptr(no)) == E
        assert call(ptr(P), n, 3, ptr(nodes), ptr(weights), 2, 1, None, ptr(ig), ptr(lg), ptr(no)) == E
        assert call(ptr(P), n, 3, ptr(nodes), ptr(weights), 2, 1, ptr(out2), None, ptr(lg), ptr(no)) == E
        assert call(ptr(P), n, 3, ptr(nodes), ptr(weights), 2, 1, ptr(out2), ptr(ig), None, ptr(no)) == E
        for a in (out2, ig, lg, no, o1, g1):
            assert np.all(a == mark)
    finally:
        wa.close()


# ---- 14. multi-device handles ------------------------------------------------------------------------------------------------------------------
def test_multi_device_handle_shards_the_vectors(jq):
    params, pcof = cnot3_short(100)
    vecs, shift = vectors(pcof, 5, 211), small_shift(params, 11)
    nodes, weights = ensemble(2, 10)
    w1 = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    wm = jq.Working_Arrays_HIP(params, pcof.size, devices=2, options={"cq3": 0, "multi_same_device": 1})
    try:
        b1, bm = batch(jq, vecs, params, w1, nodes, weights, shift), batch(jq, vecs, params, wm, nodes, weights, shift)
        for i in range(5):
            same_bits("multi-device handle, column %d" % i, column(bm, i), column(b1, i))
    finally:
        w1.close()
        wm.close()
