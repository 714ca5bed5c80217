"""GPU (-m gpu): jq_eval_f_g_grad_hvp -- Hessian-vector products of a risk-neutral ensemble on the tangent-linear lane kernels
(k_forward_lane_tl, k_terminal_cols<LaneMap, EP_TL>, k_backward_lane_tl; Ntot <= 6) and on the sequential route (everything else), against the CPU
reference of tests/ensemble_hessian_reference.py: sum_i w_i HessianReference(p_i).hvp(pcof, d) over the nodes' problems.

Random dense problems from the generator of the block-band tests at one tile row, 7 time steps, where a lane kernel can go wrong: every
padded dimension full and zero-padded (Ntot 2 .. 6 on NP 2 / 4 / 6; Ntot 7, 8 have no tangent-linear lane kernel -- it would spill --
and must take the sequential route), N 2 / 3 / 4, one node (eps 0), 3 nodes, 23 nodes x N 3 = 69 columns (a second wave that is partly
padding, a column count that is no multiple of 16), 1 / 2 / 4 controls, Neumann order 0 / 1 / 4, one chunk and chunks of 3 + 3 + 1
(state, both adjoints, the carries and their tangents cross chunk boundaries), 1 and 5 directions (e_k, g/|g|, random), objFuncType
1 / 2 / 3, the default shift and a given one.  Criterion: the project's reference_pass (atol 1e-14 or rtol 1e-10) on every column of
hv_infid and hv_leak; out2 and the gradients against eval_f_g_grad on the same handle; a direction of a 5-direction call and directions
in rounds bit-identical to the direction alone / one launch; jq_eval_f_g_grad and jq_traceobjgrad_hvp the same bits before and after."""
import collections

import numpy as np
import pytest
from conftest import case_inputs, reference_pass

import ensemble_hessian_reference as ER
from block_band_problem import block_band_problem
from test_gpu_hvp import REFUSALS, _directions, _refusal_handles

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "Ntot N Nc m chunk ndir objFuncType nquad shift")
NSTEPS = 7
KF_LANE, KF_COOP = 2, 1
LANE_CASES = (
    Case(2, 2, 1, 4, 0, 5, 1, 1, "default"),       # NP 2 full, no guard level, one node
    Case(3, 2, 2, 0, 3, 1, 3, 3, "given"),         # NP 4 zero padded, no Neumann terms, chunks, unforced pass
    Case(4, 3, 4, 1, 0, 5, 2, 3, "default"),       # NP 4 full, four controls
    Case(3, 3, 1, 1, 3, 5, 2, 23, "default"),      # 69 columns: two waves, the second mostly padding
    Case(4, 2, 2, 4, 0, 1, 1, 1, "given"),
    Case(5, 4, 1, 4, 3, 5, 3, 3, "given"),         # NP 6 zero padded
    Case(6, 3, 2, 1, 0, 1, 1, 23, "given"),        # NP 6 full, 69 columns
    Case(6, 2, 4, 4, 3, 5, 3, 3, "given"),         # NP 6, four controls, everything at once
)
SEQ_CASES = (      # (case, options)
    (Case(7, 2, 2, 1, 0, 5, 3, 3, "given"), None),                 # NP 8: no tangent-linear lane kernel
    (Case(8, 4, 1, 4, 3, 1, 1, 3, "given"), None),
    (Case(3, 2, 2, 0, 3, 1, 3, 3, "given"), {"lane": 0}),          # the lane problems with the lane kernels disabled
    (Case(5, 4, 1, 4, 3, 5, 3, 3, "given"), {"lane": 0}),
    (Case(4, 2, 5, 1, 0, 1, 3, 3, "default"), None),               # five controls: two control groups
    (Case(17, 3, 2, 1, 3, 5, 3, 3, "given"), None),                # a second tile row
)


def _id(c):
    return "Ntot%d-N%d-Nc%d-m%d-%s-ndir%d-type%d-nq%d-%s" % (c.Ntot, c.N, c.Nc, c.m, "chunks331" if c.chunk else "onechunk", c.ndir, c.objFuncType, c.nquad, c.shift)


def _problem(jq, c):
    rng = np.random.default_rng(83000 + 1000 * c.Ntot + 100 * c.N + 10 * c.Nc + c.m)
    p, pcof = block_band_problem(jq, rng, c.Ntot, c.N, (c.Ntot - 1) // 16, [1] * c.Nc, NSTEPS, c.m, c.objFuncType)
    if c.nquad == 1:
        nodes, weights = np.zeros(1), np.ones(1)
    else:
        nodes = 0.05 * np.linspace(-1.0, 1.0, c.nquad) + 0.01 * rng.standard_normal(c.nquad)
        weights = rng.random(c.nquad) + 0.1
        weights /= weights.sum()
    shift = None if c.shift == "default" else rng.standard_normal(c.Ntot)
    return p, pcof, rng, nodes, weights, shift


def _options(c, extra=None):
    o = dict(extra or {})
    if c.chunk:
        o["chunk_steps"] = c.chunk
    return o or None


def _reference(p, pcof, D, nodes, weights, shift):
    ref = ER.EnsembleHessianReference(p, nodes, weights, shift)
    return [ref.hvp(pcof, D[:, j]) for j in range(D.shape[1])]


def _check_against_reference(r, refs):
    for j, t in enumerate(refs):
        for k in ("hv_infid", "hv_leak"):
            rel = np.linalg.norm(r[k][:, j] - t[k]) / max(np.linalg.norm(t[k]), 1e-300)
            print("%s[:, %d]: relative %.2e" % (k, j, rel))
            assert reference_pass(r[k][:, j], t[k]), (k, j, rel)


def _check_primal(jq, r, pcof, p, wa, nodes, weights, shift):
    inf, leak = jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
    assert reference_pass(r["infidelity"], inf) and reference_pass(r["leak"], leak), (r["infidelity"], inf, r["leak"], leak)
    assert reference_pass(r["infid_grad"], p.last_infidelity_grad)
    if p.objFuncType != 1:
        assert reference_pass(r["leak_grad"], p.last_leak_grad)
    else:
        assert not r["leak_grad"].any() and not r["hv_leak"].any()


def _total_gradient(p, pcof, nodes, weights, shift):
    return ER.weighted_oracle_gradients(p, pcof, nodes, weights, shift)[0]


SAME_BITS = ("infidelity", "leak", "infid_grad", "leak_grad")


@pytest.mark.parametrize("c", LANE_CASES, ids=[_id(c) for c in LANE_CASES])
def test_lane_route_matches_reference(jq, c):
    p, pcof, rng, nodes, weights, shift = _problem(jq, c)
    D = _directions(rng, _total_gradient(p, pcof, nodes, weights, shift), pcof.size, c.ndir)
    refs = _reference(p, pcof, D, nodes, weights, shift)
    NP = 2 * ((c.Ntot + 1) // 2)
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=_options(c))
    try:
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift)
        assert r["hv_infid"].shape == (pcof.size, c.ndir) and r["hv_leak"].shape == (pcof.size, c.ndir)
        plan = wa.plan_info()
        assert plan["ens_hvp"] == {"route": "lane", "directions_per_launch": c.ndir, "chunk_steps": c.chunk or NSTEPS, "rounds": 1}
        assert plan["last_kernels"]["object"] == "l_%d" % NP and plan["last_kernels"]["forward_object"] == "l_%d" % NP
        t = wa.last_timing()
        nchunks, npass = (3 if c.chunk else 1), (2 if c.objFuncType != 1 else 1)
        assert (t["kernel_family"], t["kernel_size"], t["kernel_band"]) == (KF_LANE, NP, 0)
        assert t["n_forward_launches"] == nchunks and t["n_backward_launches"] == nchunks * npass
        _check_against_reference(r, refs)
        _check_primal(jq, r, pcof, p, wa, nodes, weights, shift)
        if c.ndir > 1:
            for j in (1, c.ndir - 1):      # a direction alone: the same operations in the same order
                one = jq.eval_f_g_grad_hvp(pcof, D[:, j], p, wa, nodes, weights, shift)
                assert wa.plan_info()["ens_hvp"]["directions_per_launch"] == 1
                for k in ("hv_infid", "hv_leak"):
                    assert np.array_equal(one[k][:, 0], r[k][:, j]), (k, j)
                for k in SAME_BITS:
                    assert np.array_equal(one[k], r[k]), k
    finally:
        wa.close()


@pytest.mark.parametrize("c,opts", SEQ_CASES, ids=[_id(c) + ("-lane0" if o else "") for c, o in SEQ_CASES])
def test_sequential_route_matches_reference(jq, c, opts):
    p, pcof, rng, nodes, weights, shift = _problem(jq, c)
    D = _directions(rng, _total_gradient(p, pcof, nodes, weights, shift), pcof.size, c.ndir)
    refs = _reference(p, pcof, D, nodes, weights, shift)
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=_options(c, opts))
    try:
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift)
        plan = wa.plan_info()
        assert plan["ens_hvp"] == {"route": "sequential", "directions_per_launch": c.ndir, "chunk_steps": c.chunk or NSTEPS, "rounds": c.nquad}
        assert "hvp" not in plan      # (that record stays jq_traceobjgrad_hvp's)
        assert wa.last_timing()["kernel_family"] == KF_COOP
        _check_against_reference(r, refs)
        _check_primal(jq, r, pcof, p, wa, nodes, weights, shift)
    finally:
        wa.close()


def test_rounds_and_the_calls_around_are_the_same_bits(jq):
    """a stream budget that holds the primal stream and two directions: five directions run in three rounds, bit-identical to one
    launch; jq_eval_f_g_grad and jq_traceobjgrad_hvp on the same handle return the same bits before and after the calls"""
    c = Case(6, 2, 4, 4, 0, 5, 3, 3, "given")
    p, pcof, rng, nodes, weights, shift = _problem(jq, c)
    D = _directions(rng, _total_gradient(p, pcof, nodes, weights, shift), pcof.size, 5)
    stride = 48      # doubles of a lane operator image at NP = 6 (36 padded to a multiple of 16)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    wb = jq.Working_Arrays_HIP(p, pcof.size, options={"stream_bytes": 8 * 3 * 2 * stride * (2 * NSTEPS + 1), "chunk_steps": NSTEPS})
    try:
        def around(w):
            jq.eval_f_g_grad(pcof, p, w, nodes, weights, True, shift=shift)
            h = jq.traceobjgrad_hvp(pcof, D[:, :2], p, w)
            return [np.array([p.last_infidelity, p.last_leak]), p.last_infidelity_grad.copy(), p.last_leak_grad.copy(), h["totalgrad"], h["hv"], h["hv_infid"]]
        before = [around(w) for w in (wa, wb)]
        a, b = [jq.eval_f_g_grad_hvp(pcof, D, p, w, nodes, weights, shift) for w in (wa, wb)]
        assert wa.plan_info()["ens_hvp"] == {"route": "lane", "directions_per_launch": 5, "chunk_steps": NSTEPS, "rounds": 1}
        assert wb.plan_info()["ens_hvp"] == {"route": "lane", "directions_per_launch": 2, "chunk_steps": NSTEPS, "rounds": 3}
        assert wb.last_timing()["n_forward_launches"] == 3 and wb.last_timing()["n_backward_launches"] == 6
        for k in SAME_BITS + ("hv_infid", "hv_leak"):
            assert np.array_equal(a[k], b[k]), k
        after = [around(w) for w in (wa, wb)]
        for x, y in zip(before, after):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)
    finally:
        wa.close()
        wb.close()


@pytest.mark.parametrize("which", range(5), ids=REFUSALS)
def test_refusals_write_nothing_and_leave_the_handle_alone(jq, which):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    name, p, pcof, WA = _refusal_handles(jq)[which]
    wa = WA(p, pcof.size)
    try:
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        n = pcof.size
        z = lambda k: np.zeros(k)
        out2, ig, lg, hvi, hvl, d, nodes, w = z(2), z(n), z(n), z(n), z(n), np.ones(n), np.array([0.01]), np.ones(1)
        dp = lambda a: a.ctypes.data_as(_lib.c_dp)
        rc = L.jq_eval_f_g_grad_hvp(wa.handle, dp(np.ascontiguousarray(pcof)), n, dp(d), 1, dp(nodes), dp(w), 1, None, dp(out2), dp(ig), dp(lg), dp(hvi), dp(hvl))
        assert rc == _lib.JQ_EUNSUPPORTED, (name, rc)
        msg = L.jq_last_error(wa.handle).decode()
        assert "jq_eval_f_g_grad_hvp" in msg and len(msg) > 40
        assert not out2.any() and not ig.any() and not lg.any() and not hvi.any() and not hvl.any()
        assert "ens_hvp" not in wa.plan_info()
        with pytest.raises(_lib.JuqboxHipError) as e:
            jq.eval_f_g_grad_hvp(pcof, d, p, wa, nodes, w)
        assert e.value.code == _lib.JQ_EUNSUPPORTED
        after = jq.traceobjgrad(pcof, p, wa, False, True)
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
    finally:
        wa.close()


def test_argument_codes(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    c = LANE_CASES[1]
    p, pcof, rng, nodes, weights, shift = _problem(jq, c)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        wa.sync_params()
        n = pcof.size
        z = lambda k: np.zeros(k)
        out2, ig, lg, hvi, hvl, d = z(2), z(n), z(n), z(n), z(n), np.ones(n)
        dp = lambda a: a.ctypes.data_as(_lib.c_dp)
        good = [wa.handle, dp(np.ascontiguousarray(pcof)), n, dp(d), 1, dp(nodes), dp(weights), nodes.size, None, dp(out2), dp(ig), dp(lg), dp(hvi), dp(hvl)]
        f = L.jq_eval_f_g_grad_hvp
        for k in (1, 3, 5, 6, 9, 10, 11, 12, 13):      # every required pointer
            bad = list(good)
            bad[k] = None
            assert f(*bad) == _lib.JQ_EINVAL, k
        for k in (4, 7):      # ndir, nquad
            bad = list(good)
            bad[k] = 0
            assert f(*bad) == _lib.JQ_EINVAL, k
        bad = list(good)
        bad[2] = n - 1
        assert f(*bad) in (_lib.JQ_EINVAL, _lib.JQ_EDIM)
        assert not out2.any() and not ig.any() and not hvi.any() and not hvl.any()
        assert "ens_hvp" not in wa.plan_info()
        assert f(*good) == _lib.JQ_OK
        assert out2[0] != 0.0 and ig.any() and hvi.any() and hvl.any()
    finally:
        wa.close()


def test_full_length_swap02(jq):
    """swap02 at its full length of 7 915 steps over 3 nodes along g/|g| and one random direction"""
    p, info, pcof, _ = case_inputs("swap02")
    assert p.nsteps == 7915
    nodes, weights = np.array([-0.02, 0.0, 0.03]), np.array([0.3, 0.4, 0.3])
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True)
        g = p.last_infidelity_grad + (p.last_leak_grad if p.objFuncType != 1 else 0.0)
        rng = np.random.default_rng(2718)
        D = np.stack([g / np.linalg.norm(g), rng.standard_normal(pcof.size)], axis=1)
        refs = _reference(p, pcof, D, nodes, weights, None)
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights)
        assert wa.plan_info()["ens_hvp"]["route"] == "lane" and wa.last_timing()["kernel_family"] == KF_LANE
        _check_against_reference(r, refs)
        _check_primal(jq, r, pcof, p, wa, nodes, weights, None)
    finally:
        wa.close()


def test_run_optimizer_with_the_exact_hessian(jq):
    """rabi from a perturbed start, a handful of trust-region iterations on exact Hessian-vector products: the objective decreases and
    the bounds hold"""
    p, info, pcof, _ = case_inputs("rabi")
    rng = np.random.default_rng(99)
    n = pcof.size
    maxpar = info["maxpar"][0]
    lo, hi = np.full(n, -2.0 * maxpar), np.full(n, 2.0 * maxpar)
    x0 = np.clip(pcof + 0.4 * maxpar * rng.standard_normal(n), lo, hi)
    wa = jq.Working_Arrays_HIP(p, n)
    try:
        prob = jq.setup_ipopt_problem(p, wa, n, lo, hi, maxIter=6, hessian="exact")
        assert prob.eval_hessvec is not None and prob.m == 0
        f0 = prob.eval_f(x0)
        d = rng.standard_normal(n)
        hv = prob.eval_hessvec(x0, d)
        assert wa.plan_info()["ens_hvp"]["route"] == "lane"
        eps = 1e-5      # (a sanity check of the callback's sign and Tikhonov term: central difference of the gradient callback, 1e-6 relative)
        fd = (prob.eval_grad_f(x0 + eps * d) - prob.eval_grad_f(x0 - eps * d)) / (2.0 * eps)
        assert np.linalg.norm(hv - fd) < 1e-6 * np.linalg.norm(fd)
        x = jq.run_optimizer(prob, x0)
        print("rabi, exact Hessian: objective %.6e -> %.6e in %d iterations (%s)" % (f0, prob.obj_val, prob.n_iter, prob.status))
        assert prob.obj_val < f0
        assert np.all(x >= lo - 1e-12) and np.all(x <= hi + 1e-12)
        assert jq.setup_ipopt_problem(p, wa, n, lo, hi, maxIter=6).eval_hessvec is None      # the default changes nothing
    finally:
        wa.close()
