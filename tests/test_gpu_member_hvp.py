"""GPU (-m gpu): jq_eval_f_g_grad_members_hvp -- Hessian-vector products of an ensemble whose members differ in a real Nc x Nc mix of the
controls and in their drift, on the tangent-linear lane, row-lane and quad-layout kernels, where every wave reads the primal stream AND
the tangent stream of its own member (PropArgs::tl_dirs_per_member), against the CPU reference of tests/member_hvp_cases.py:
sum_i w_i HessianReference(mixed_params(p, C_i, H_i)).hvp(pcof, d).

The cases are those of tests/member_hvp_cases.py (tests/test_member_hvp_host.py shows on the oracle alone that they discriminate): the
shapes, members and directions of tests/drift_hvp_cases.py with a mix per member, 12 steps in one chunk and in chunks of 5 + 5 + 2,
objFuncType 1 and 2.  Criterion: the project's reference_pass (atol 1e-14 or rtol 1e-10) on every column of hv_infid and hv_leak and on
infidelity, leak and the two gradients against the oracle's weighted sums; the route, the kernel objects and the launch counts of every
call.  Bits are held where the source promises them and nowhere else: no mix is the drift call itself, one member with the identity mix
is the drift call with that member, one-hot weights give the member alone, a direction does not depend on the others of its call, and a
column of zeros in every mix gives exactly zero blocks for that control.  (Three identity-mix members sum their traces in another order
than the drift call: not held to bits.)  A small stream budget splits the members into two member rounds.  Options lane=0 / quad=0,
Ntot 7, five controls and a member off the 4 x 4 x n pattern take the sequential route, which leaves the plan and the handle's drift
alone; the refusals are tl_refuse's and the argument rules of jq_eval_f_g_grad_members."""
import numpy as np
import pytest
from conftest import reference_pass

import member_hvp_cases as C
from test_gpu_hvp import REFUSALS, _refusal_handles

pytestmark = pytest.mark.gpu

KF_COOP = 1
KEYS = ("infidelity", "leak", "infid_grad", "leak_grad", "hv_infid", "hv_leak")
ROUTES = ("lane", "rowlane", "quad")
FIRST = {r: next(s for s in C.SHAPES if s.route == r) for r in ROUTES}      # the first shape of every route
LAST = {r: [s for s in C.SHAPES if s.route == r][-1] for r in ROUTES}       # ... and the one with the padded packing


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


def _assert_records(wa, s, objFuncType, members, dpl, cs, rounds, drifts=True, mix=True, nsteps=C.NSTEPS):
    plan = wa.plan_info()
    assert plan["member_hvp"] == {"route": s.route, "members_per_launch": members, "directions_per_launch": dpl, "chunk_steps": cs, "rounds": rounds,
                                  "drifts": drifts, "ctrl_mix": mix}
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
    p, pcof, H, Cm, D, refs, _, orc = C.case(jq, s, objFuncType)
    wa = jq.Working_Arrays_HIP(p, pcof.size, options={"chunk_steps": chunk} if chunk else None)
    try:
        r = jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, C.WEIGHTS, Hconsts=H, ctrl_mix=Cm)
        assert r["hv_infid"].shape == (pcof.size, C.NDIR) and r["hv_leak"].shape == (pcof.size, C.NDIR)
        _assert_records(wa, s, objFuncType, 3, C.NDIR, chunk or C.NSTEPS, 1)
        plan = wa.plan_info()
        assert "drift_hvp" not in plan and "ens_hvp" not in plan and "hvp" not in plan
        _check(r, p, refs, orc)
    finally:
        wa.close()


@pytest.mark.parametrize("route", ROUTES)
def test_mixes_alone_use_the_handles_drift(jq, route):
    """Hconsts=None: every member has the handle's own drift image and its own mix"""
    s = FIRST[route]
    p, pcof, H, Cm, D, refs, _, orc = C.case(jq, s, 2, drifts=False)
    assert H is None
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        r = jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, C.WEIGHTS, ctrl_mix=Cm)
        _assert_records(wa, s, 2, 3, C.NDIR, C.NSTEPS, 1, drifts=False)
        _check(r, p, refs, orc)
    finally:
        wa.close()


@pytest.mark.parametrize("route", ROUTES)
def test_a_small_stream_budget_splits_the_members_into_two_rounds(jq, route):
    """a budget of six streams of 2 x 12 + 1 time points: a member costs 1 + 2 streams, so two of the three members per launch and the
    third in a second member round whose blocks the host adds behind the first round's"""
    s = LAST[route]
    p, pcof, H, Cm, D, refs, _, orc = C.case(jq, s, 2)
    wa = jq.Working_Arrays_HIP(p, pcof.size, options={"stream_bytes": 8 * 6 * 2 * C.image_stride(s) * (2 * C.NSTEPS + 1), "chunk_steps": C.NSTEPS})
    try:
        r = jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, C.WEIGHTS, Hconsts=H, ctrl_mix=Cm)
        _assert_records(wa, s, 2, 2, C.NDIR, C.NSTEPS, 2)
        _check(r, p, refs, orc)
    finally:
        wa.close()


@pytest.mark.parametrize("route", ROUTES)
def test_without_a_mix_the_call_is_the_drift_call(jq, route):
    """ctrl_mix=None: the launches and the bits of jq_eval_f_g_grad_drifts_hvp; each call keeps its own plan record"""
    s = LAST[route]
    p, pcof, H, _, D, _, _, _ = C.case(jq, s, 2)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        drift = jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, H, C.WEIGHTS)
        record = wa.plan_info()["drift_hvp"]
        assert "member_hvp" not in wa.plan_info()
        mine = jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, C.WEIGHTS, Hconsts=H)
        _assert_records(wa, s, 2, 3, C.NDIR, C.NSTEPS, 1, mix=False)
        assert wa.plan_info()["drift_hvp"] == record
        assert np.abs(mine["hv_infid"]).max() > 0.0
        _same_bits(mine, drift)
    finally:
        wa.close()


@pytest.mark.parametrize("route", ROUTES)
def test_one_member_with_the_identity_mix_is_the_drift_call_with_that_member(jq, route):
    """k_ctrl and k_trace_reduce with C = I write the bits of the launches without a mix, and one member's block is added to zero"""
    s = LAST[route]
    p, pcof, H, _, D, _, _, _ = C.case(jq, s, 2)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        for i in (0, 2):
            drift = jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, H[:, :, i], np.ones(1))
            mine = jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, np.ones(1), Hconsts=H[:, :, i], ctrl_mix=np.eye(s.Nc))
            _assert_records(wa, s, 2, 1, C.NDIR, C.NSTEPS, 1)
            assert np.abs(mine["hv_infid"]).max() > 0.0
            _same_bits(mine, drift)
    finally:
        wa.close()


@pytest.mark.parametrize("route", ROUTES)
def test_one_hot_weights_are_the_bits_of_the_member_alone(jq, route):
    """w = e_i over the three mixed members against member i alone with weight 1: its waves read the primal stream i and the tangent
    streams i D .. i D + D - 1 and nothing else, and the members of weight zero contribute exact zeros"""
    s = LAST[route]
    p, pcof, H, Cm, D, _, _, _ = C.case(jq, s, 2)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        for i in range(3):
            w = np.zeros(3)
            w[i] = 1.0
            all3 = jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, w, Hconsts=H, ctrl_mix=Cm)
            _assert_records(wa, s, 2, 3, C.NDIR, C.NSTEPS, 1)
            alone = jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, np.ones(1), Hconsts=H[:, :, i], ctrl_mix=Cm[:, :, i])
            _assert_records(wa, s, 2, 1, C.NDIR, C.NSTEPS, 1)
            assert np.abs(alone["hv_infid"]).max() > 0.0
            _same_bits(all3, alone)
    finally:
        wa.close()


@pytest.mark.parametrize("route", ROUTES)
def test_a_direction_does_not_depend_on_the_others_of_its_call(jq, route):
    s = LAST[route]
    p, pcof, H, Cm, D, _, _, _ = C.case(jq, s, 2)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        both = jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, C.WEIGHTS, Hconsts=H, ctrl_mix=Cm)
        for j in range(C.NDIR):
            one = jq.eval_f_g_grad_members_hvp(pcof, D[:, [j]], p, wa, C.WEIGHTS, Hconsts=H, ctrl_mix=Cm)
            _assert_records(wa, s, 2, 3, 1, C.NSTEPS, 1)
            for k in ("hv_infid", "hv_leak"):
                assert np.array_equal(one[k][:, 0], both[k][:, j]), (k, j)
            for k in ("infidelity", "leak", "infid_grad", "leak_grad"):
                assert np.array_equal(one[k], both[k]), k
    finally:
        wa.close()


@pytest.mark.parametrize("route", ROUTES)
def test_a_zero_column_in_every_mix_gives_exactly_zero_blocks(jq, route):
    """control k reaches no operator of any member: its coefficients have exactly zero gradient and exactly zero rows in both products,
    the other controls' blocks are alive"""
    s = FIRST[route]
    assert s.Nc >= 2
    p, pcof, H, Cm, D, _, _, _ = C.case(jq, s, 2)
    per = pcof.size // s.Nc      # coefficients of one control: [control][frequency][p | q][D1]
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        for k in (0, s.Nc - 1):
            Z = Cm.copy(order="F")
            Z[:, k, :] = 0.0
            r = jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, C.WEIGHTS, Hconsts=H, ctrl_mix=Z)
            _assert_records(wa, s, 2, 3, C.NDIR, C.NSTEPS, 1)
            for key in ("infid_grad", "leak_grad", "hv_infid", "hv_leak"):
                assert not r[key][k * per:(k + 1) * per].any(), (key, k)
                other = np.delete(r[key], np.s_[k * per:(k + 1) * per], axis=0)
                assert np.all(np.abs(other).reshape(s.Nc - 1, -1).max(axis=1) > 0.0), (key, k)
    finally:
        wa.close()


def _sequential(jq, p, pcof, H, Cm, D, w, options, refs=None, orc=None):
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=options)
    try:
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        plan0 = wa.plan_info()
        r = jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, w, Hconsts=H, ctrl_mix=Cm)
        plan = wa.plan_info()
        assert plan.pop("member_hvp") == {"route": "sequential", "members_per_launch": 1, "directions_per_launch": D.shape[1], "chunk_steps": p.nsteps,
                                          "rounds": len(w), "drifts": True, "ctrl_mix": True}
        assert plan == plan0      # (no re-plan; "drift_hvp" / "ens_hvp" / "hvp" / "member_batch" untouched)
        assert wa.last_timing()["kernel_family"] == KF_COOP
        if refs is None:
            refs, _, orc = C.reference(p, pcof, D, Cm, H, w)
        _check(r, p, refs, orc)
        after = jq.traceobjgrad(pcof, p, wa, False, True)
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
    finally:
        wa.close()


@pytest.mark.parametrize("route,option", (("lane", "lane"), ("rowlane", "lane"), ("quad", "quad")))
def test_a_switched_off_route_is_sequential(jq, route, option):
    p, pcof, H, Cm, D, refs, _, orc = C.case(jq, FIRST[route], 2)
    _sequential(jq, p, pcof, H, Cm, D, C.WEIGHTS, {option: 0}, refs, orc)


def test_ntot_7_is_sequential(jq):
    s = C.Shape("lane", 7, 2, 2, 1, 0)      # NP 8: no tangent-linear lane kernel
    p, pcof, H, D = C.problem(jq, s, 3)
    _sequential(jq, p, pcof, H, C.member_mixes(s), D, C.WEIGHTS, None)


def test_five_controls_are_sequential_in_two_control_groups(jq):
    """more than JQ_MAXNC controls: each group's sweep reduces its operators' traces with its rows of the mix into the coefficients of ALL
    five controls (k_trace_reduce's q0)"""
    s = C.Shape("rowlane", 12, 2, 5, 1, 0)
    p, pcof, H, D = C.problem(jq, s, 3)
    _sequential(jq, p, pcof, H, C.member_mixes(s), D, C.WEIGHTS, None)


def test_a_member_off_the_pattern_is_sequential_and_leaves_the_plan_alone(jq):
    """a quad-route problem with one member drift that couples two rows no 4 x 4 x n operator couples: the members run one after the
    other with their mixes, correct, without a re-plan, and traceobjgrad returns the same bits before and after"""
    s = FIRST["quad"]
    p, pcof, H, Cm, D, _, _, _ = C.case(jq, s, 2)
    H = H.copy(order="F")
    H[1, 10, 1] = H[10, 1, 1] = 0.37
    from subsystem_problem import t4_structure
    assert not t4_structure(H[:, :, 1]) and t4_structure(H[:, :, 0]) and t4_structure(H[:, :, 2])
    _sequential(jq, p, pcof, H, Cm, D, C.WEIGHTS, None)


def _raw_call(L, _lib, wa, pcof, d, H, Cm, w, nm):
    n = pcof.size
    out = [np.zeros(2), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)]
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib.c_dp)
    rc = L.jq_eval_f_g_grad_members_hvp(wa.handle, dp(np.ascontiguousarray(pcof)), n, dp(d), 1, dp(H), dp(Cm), dp(w), nm, *[dp(o) for o in out])
    return rc, L.jq_last_error(wa.handle).decode(), out


@pytest.mark.parametrize("which", range(5), ids=REFUSALS)
def test_refusals_write_nothing_and_leave_the_handle_alone(jq, which):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    name, p, pcof, WA = _refusal_handles(jq)[which]
    assert name == REFUSALS[which]
    wa = WA(p, pcof.size)
    try:
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        Ntot, Nc = int(p.Ntot), max(p.Ncoupled, p.Nunc)
        d, w = np.ones(pcof.size), np.ones(1)
        H = np.ascontiguousarray(np.asarray(p.Hconst, dtype=np.float64).T.reshape(-1))
        Cm = np.ascontiguousarray((np.eye(Nc) + 0.05).reshape(-1))
        rc, msg, out = _raw_call(L, _lib, wa, pcof, d, H, Cm, w, 1)
        assert rc == _lib.JQ_EUNSUPPORTED, (name, rc)
        assert "jq_eval_f_g_grad_members_hvp" in msg and len(msg) > 40
        assert not any(o.any() for o in out)
        assert "member_hvp" not in wa.plan_info()
        with pytest.raises(_lib.JuqboxHipError) as e:
            jq.eval_f_g_grad_members_hvp(pcof, d, p, wa, w, Hconsts=np.asarray(p.Hconst, dtype=np.float64).reshape(Ntot, Ntot), ctrl_mix=np.eye(Nc) + 0.05)
        assert e.value.code == _lib.JQ_EUNSUPPORTED
        after = jq.traceobjgrad(pcof, p, wa, False, True)
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
    finally:
        wa.close()


@pytest.mark.parametrize("what", ("both-null", "nan-mix"))
def test_argument_errors_of_the_member_calls(jq, what):
    """jq_eval_f_g_grad_members' rules with its messages: neither drifts nor mixes is the plain problem, a mix entry must be finite"""
    from juqbox_jl_amd import _lib
    L = _lib.load()
    s = FIRST["lane"]
    p, pcof, _, D = C.problem(jq, s, 2)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        Cm = np.ascontiguousarray(np.eye(s.Nc).reshape(-1))
        if what == "nan-mix":
            Cm[1] = np.nan
        rc, msg, out = _raw_call(L, _lib, wa, pcof, np.ascontiguousarray(D[:, 0]), None, None if what == "both-null" else Cm, np.ones(1), 1)
        assert rc == _lib.JQ_EINVAL
        expect = ("jq_eval_f_g_grad_members_hvp: Hconsts and ctrl_mix are both NULL" if what == "both-null"
                  else "jq_eval_f_g_grad_members_hvp: a control mix entry is not finite")
        assert msg.startswith(expect), msg
        assert not any(o.any() for o in out)
        assert "member_hvp" not in wa.plan_info()
        after = jq.traceobjgrad(pcof, p, wa, False, True)
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
    finally:
        wa.close()
