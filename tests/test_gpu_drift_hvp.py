"""GPU (-m gpu): jq_eval_f_g_grad_drifts_hvp -- Hessian-vector products of a drift ensemble on the tangent-linear lane, row-lane and
quad-layout kernels, where every wave reads the operator stream of its own member (PropArgs::nprimal primal streams in front of the
directions'), against the CPU reference of tests/drift_hessian_reference.py: sum_i w_i HessianReference(p with Hconst = H_i).hvp(pcof, d).

The cases are those of tests/drift_hvp_cases.py (tests/test_drift_hvp_host.py shows on the oracle alone that they discriminate): per route
the two smallest shapes at which the packing can go wrong, 3 members of unequal weights, 2 directions, 12 steps in one chunk and in
chunks of 5 + 5 + 2, objFuncType 1 and 2.  Criterion: the project's reference_pass (atol 1e-14 or rtol 1e-10) on every column of
hv_infid and hv_leak and on infidelity, leak and the two gradients against the oracle's weighted sums; the route, the kernel objects and
the launch counts of every call.  Stream addressing is held bit for bit: one-hot weights give the bits of the member alone, and the
handle's own drift as the single member gives the bits of jq_eval_f_g_grad_hvp with one node at eps 0.  A small stream budget splits
the members into two member rounds.  Option lane=0 / quad=0, Ntot 7 and a member off the 4 x 4 x n pattern take the sequential route,
which leaves the plan and the handle's drift alone; the refusals are tl_refuse's."""
import numpy as np
import pytest
from conftest import reference_pass

import drift_hessian_reference as DR
import drift_hvp_cases as C
from block_band_problem import block_band_problem
from test_gpu_hvp import REFUSALS, _refusal_handles

pytestmark = pytest.mark.gpu

KF_COOP = 1
KEYS = ("infidelity", "leak", "infid_grad", "leak_grad", "hv_infid", "hv_leak")
FIRST = {r: next(s for s in C.SHAPES if s.route == r) for r in ("lane", "rowlane", "quad")}      # the first shape of every route
LAST = {r: [s for s in C.SHAPES if s.route == r][-1] for r in ("lane", "rowlane", "quad")}       # ... and the one with the padded packing


def _check(r, p, refs, orc):
    for j, t in enumerate(refs):
        for k in ("hv_infid", "hv_leak"):
            rel = np.linalg.norm(r[k][:, j] - t[k]) / max(np.linalg.norm(t[k]), 1e-300)
            print("%s[:, %d]: relative %.2e" % (k, j, rel))
            assert reference_pass(r[k][:, j], t[k]), (k, j, rel)
    two = p.objFuncType != 1
    assert reference_pass(r["infidelity"], orc["infidelity"]) and reference_pass(r["leak"], orc["leak"]), (r["infidelity"], orc["infidelity"], r["leak"], orc["leak"])
    assert reference_pass(r["infid_grad"], orc["infidelgrad"] if two else orc["totalgrad"])
    if two:
        assert reference_pass(r["leak_grad"], orc["totalgrad"] - orc["infidelgrad"])
    else:
        assert not r["leak_grad"].any() and not r["hv_leak"].any()


def _assert_records(wa, s, objFuncType, members, dpl, cs, rounds, nsteps=C.NSTEPS):
    plan = wa.plan_info()
    assert plan["drift_hvp"] == {"route": s.route, "members_per_launch": members, "directions_per_launch": dpl, "chunk_steps": cs, "rounds": rounds}
    assert plan["last_kernels"]["object"] == C.kernel_object(s) and plan["last_kernels"]["forward_object"] == C.kernel_object(s)
    t = wa.last_timing()
    nchunks, npass = (nsteps + cs - 1) // cs, (2 if objFuncType != 1 else 1)
    assert (t["kernel_family"], t["kernel_size"]) == (C.KERNEL_FAMILY[s.route], C.kernel_size(s))
    assert t["n_forward_launches"] == rounds * nchunks and t["n_backward_launches"] == rounds * nchunks * npass


def _same_bits(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("chunk", (0, C.CHUNK), ids=("onechunk", "chunks552"))
@pytest.mark.parametrize("objFuncType", C.OBJ_TYPES)
@pytest.mark.parametrize("s", C.SHAPES, ids=[C.shape_id(s) for s in C.SHAPES])
def test_concurrent_route_matches_reference(jq, s, objFuncType, chunk):
    p, pcof, H, D, refs, _, orc = C.case(jq, s, objFuncType)
    wa = jq.Working_Arrays_HIP(p, pcof.size, options={"chunk_steps": chunk} if chunk else None)
    try:
        r = jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, H, C.WEIGHTS)
        assert r["hv_infid"].shape == (pcof.size, C.NDIR) and r["hv_leak"].shape == (pcof.size, C.NDIR)
        _assert_records(wa, s, objFuncType, 3, C.NDIR, chunk or C.NSTEPS, 1)
        assert "ens_hvp" not in wa.plan_info() and "hvp" not in wa.plan_info()
        _check(r, p, refs, orc)
    finally:
        wa.close()


@pytest.mark.parametrize("route", ("lane", "rowlane", "quad"))
def test_a_small_stream_budget_splits_the_members_into_two_rounds(jq, route):
    """a budget of four streams of 2 x 12 + 1 time points: two directions and two of the three members per launch, the third member in
    a second member round that accumulates into the same gradient blocks"""
    s = LAST[route]
    p, pcof, H, D, refs, _, orc = C.case(jq, s, 2)
    wa = jq.Working_Arrays_HIP(p, pcof.size, options={"stream_bytes": 8 * 4 * 2 * C.image_stride(s) * (2 * C.NSTEPS + 1), "chunk_steps": C.NSTEPS})
    try:
        r = jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, H, C.WEIGHTS)
        _assert_records(wa, s, 2, 2, C.NDIR, C.NSTEPS, 2)
        _check(r, p, refs, orc)
    finally:
        wa.close()


@pytest.mark.parametrize("route", ("lane", "rowlane", "quad"))
def test_one_hot_weights_are_the_bits_of_the_member_alone(jq, route):
    """w = e_i over the three members against the single member H_i with weight 1: the wave of member i reads stream i and nothing
    else, and the members of weight zero contribute exact zeros"""
    s = LAST[route]
    p, pcof, H, D, _, _, _ = C.case(jq, s, 2)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        for i in range(3):
            w = np.zeros(3)
            w[i] = 1.0
            all3 = jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, H, w)
            _assert_records(wa, s, 2, 3, C.NDIR, C.NSTEPS, 1)
            alone = jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, H[:, :, i], np.ones(1))
            _assert_records(wa, s, 2, 1, C.NDIR, C.NSTEPS, 1)
            assert np.abs(alone["hv_infid"]).max() > 0.0
            _same_bits(all3, alone)
    finally:
        wa.close()


@pytest.mark.parametrize("route", ("lane", "rowlane", "quad"))
def test_the_handles_own_drift_as_the_single_member_is_the_node_call(jq, route):
    """one member equal to the handle's Hconst, weight 1, against jq_eval_f_g_grad_hvp with one node at eps 0 on the same route: the
    member image is the handle's image 0 and one primal stream is the launch it always was"""
    s = LAST[route]
    p, pcof, _, D, _, _, _ = C.case(jq, s, 2)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        node = jq.eval_f_g_grad_hvp(pcof, D, p, wa, np.zeros(1), np.ones(1))
        assert wa.plan_info()["ens_hvp"] == {"route": s.route, "directions_per_launch": C.NDIR, "chunk_steps": C.NSTEPS, "rounds": 1}
        member = jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, np.asarray(p.Hconst, dtype=np.float64), np.ones(1))
        _assert_records(wa, s, 2, 1, C.NDIR, C.NSTEPS, 1)
        assert wa.plan_info()["ens_hvp"] == {"route": s.route, "directions_per_launch": C.NDIR, "chunk_steps": C.NSTEPS, "rounds": 1}      # (keeps its values)
        _same_bits(member, node)
    finally:
        wa.close()


def _sequential(jq, p, pcof, H, D, w, options, refs=None, orc=None):
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=options)
    try:
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        plan0 = wa.plan_info()
        r = jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, H, w)
        plan = wa.plan_info()
        assert plan.pop("drift_hvp") == {"route": "sequential", "members_per_launch": 1, "directions_per_launch": D.shape[1], "chunk_steps": p.nsteps, "rounds": len(w)}
        assert plan == plan0      # (no re-plan, "ens_hvp" / "hvp" / "drift_batch" untouched)
        assert wa.last_timing()["kernel_family"] == KF_COOP
        if refs is None:
            ref = DR.DriftHessianReference(p, H, w)
            refs, orc = [ref.hvp(pcof, D[:, j]) for j in range(D.shape[1])], DR.weighted_oracle(p, pcof, H, w)
        _check(r, p, refs, orc)
        after = jq.traceobjgrad(pcof, p, wa, False, True)
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
    finally:
        wa.close()


@pytest.mark.parametrize("route,option", (("lane", "lane"), ("rowlane", "lane"), ("quad", "quad")))
def test_a_switched_off_route_is_sequential(jq, route, option):
    p, pcof, H, D, refs, _, orc = C.case(jq, FIRST[route], 2)
    _sequential(jq, p, pcof, H, D, C.WEIGHTS, {option: 0}, refs, orc)


def test_ntot_7_is_sequential(jq):
    s = C.Shape("lane", 7, 2, 2, 1, 0)      # NP 8: no tangent-linear lane kernel
    p, pcof, H, D = C.problem(jq, s, 3)
    _sequential(jq, p, pcof, H, D, C.WEIGHTS, None)


def test_a_member_off_the_pattern_is_sequential_and_leaves_the_plan_alone(jq):
    """a quad-route problem with one member that couples two rows no 4 x 4 x n operator couples: the members run one after the other,
    correct, without a re-plan, and traceobjgrad returns the same bits before and after"""
    s = FIRST["quad"]
    p, pcof, H, D, _, _, _ = C.case(jq, s, 2)
    H = H.copy(order="F")
    H[1, 10, 1] = H[10, 1, 1] = 0.37
    from subsystem_problem import t4_structure
    assert not t4_structure(H[:, :, 1]) and t4_structure(H[:, :, 0]) and t4_structure(H[:, :, 2])
    _sequential(jq, p, pcof, H, D, C.WEIGHTS, None)


@pytest.mark.parametrize("which", range(5), ids=REFUSALS)
def test_refusals_write_nothing_and_leave_the_handle_alone(jq, which):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    name, p, pcof, WA = _refusal_handles(jq)[which]
    assert name == REFUSALS[which]
    wa = WA(p, pcof.size)
    try:
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        n, Ntot = pcof.size, int(p.Ntot)
        z = lambda k: np.zeros(k)
        out2, ig, lg, hvi, hvl, d, w = z(2), z(n), z(n), z(n), z(n), np.ones(n), np.ones(1)
        H = np.ascontiguousarray(np.asarray(p.Hconst, dtype=np.float64).T.reshape(-1))
        dp = lambda a: a.ctypes.data_as(_lib.c_dp)
        rc = L.jq_eval_f_g_grad_drifts_hvp(wa.handle, dp(np.ascontiguousarray(pcof)), n, dp(d), 1, dp(H), dp(w), 1, dp(out2), dp(ig), dp(lg), dp(hvi), dp(hvl))
        assert rc == _lib.JQ_EUNSUPPORTED, (name, rc)
        msg = L.jq_last_error(wa.handle).decode()
        assert "jq_eval_f_g_grad_drifts_hvp" in msg and len(msg) > 40
        assert not out2.any() and not ig.any() and not lg.any() and not hvi.any() and not hvl.any()
        assert "drift_hvp" not in wa.plan_info()
        with pytest.raises(_lib.JuqboxHipError) as e:
            jq.eval_f_g_grad_drifts_hvp(pcof, d, p, wa, np.asarray(p.Hconst, dtype=np.float64).reshape(Ntot, Ntot), w)
        assert e.value.code == _lib.JQ_EUNSUPPORTED
        after = jq.traceobjgrad(pcof, p, wa, False, True)
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
    finally:
        wa.close()
