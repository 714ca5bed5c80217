"""GPU (-m gpu): jq_eval_f_g_grad_samples_hvp -- Hessian-vector products in SAMPLE space on every route of the tangent-linear drivers
(lane, row-lane NPJ 12 and 16, quad, sequential with one and with two control groups), against the CPU reference of
tests/sampled_hessian_reference.py: the unchanged oracle behind B = d pq / d pcof of full row rank (one carrier frequency,
D1 = 2 nsteps + 3), Hs V = lstsq(B', EnsembleHessianReference.hvp(x, d)) with B x = S, B d = V.

The tables are NOT the handle's splines: every control function a different asymmetric piecewise-constant pulse; the directions are
dense random tables, three per call.  Every cell runs with one node (0, weight 1) and with five random nodes, weights and a given shift.
The cells are the smallest shapes where each piece can go wrong: 1 step (one chunk of three time points), 2 steps in chunks of 1 (a
boundary point that gets its halves from two launches), 7 steps in one chunk and in 3 + 3 + 1, 8 steps in 3 + 3 + 2, N = 5 columns that
straddle waves, five controls in two control groups (the q0 columns of the assembly), objFuncType 1 / 2 / 3.

Criterion everywhere: the project's reference_pass (atol 1e-14 or rtol 1e-10) per direction on hv_infid and hv_leak and on both gradients,
compared in sample space; the achieved relative errors are printed."""
import collections
import copy

import numpy as np
import pytest
from conftest import case_inputs, reference_pass

import sampled_hessian_reference as SR
from block_band_problem import block_band_problem
from subsystem_problem import subsystem_problem
from test_gpu_hvp import REFUSALS, _refusal_handles
from test_gpu_random import random_problem

pytestmark = pytest.mark.gpu

# kernel_family codes of jq_timing (include/juqbox_hip.h)
KF_COOP, KF_LANE, KF_ROWLANE, KF_QUAD = 1, 2, 3, 6
NDIR = 3

Cell = collections.namedtuple("Cell", "name build route family size nsteps chunks objFuncType Nc")
# build(jq, rng, nsteps) -> params; chunks: option chunk_steps per run (0: one chunk); size: kernel_size of jq_last_timing
CELLS = (
    Cell("lane-Ntot5-2steps", lambda jq, rng, n: random_problem(jq, rng, 5, 2, 2, 1, n, 0, 2, False)[0], "lane", KF_LANE, 6, 2, (1,), 2, 2),
    Cell("lane-Ntot5-1step", lambda jq, rng, n: random_problem(jq, rng, 5, 2, 2, 1, n, 0, 2, False)[0], "lane", KF_LANE, 6, 1, (0,), 2, 2),
    Cell("rowlane12-Ntot12", lambda jq, rng, n: random_problem(jq, rng, 12, 3, 2, 1, n, 3, 1, False)[0], "rowlane", KF_ROWLANE, 12, 7, (0, 3), 1, 2),
    Cell("rowlane16-Ntot13-N5", lambda jq, rng, n: random_problem(jq, rng, 13, 5, 4, 1, n, 1, 3, False)[0], "rowlane", KF_ROWLANE, 16, 8, (3,), 3, 4),
    Cell("quad-Ntot32", lambda jq, rng, n: subsystem_problem(jq, rng, 2, 32, 4, 3, 1, "varied", n, 2)[0], "quad", KF_QUAD, 2, 7, (0, 3), 2, 3),
    Cell("sequential-Ntot7", lambda jq, rng, n: random_problem(jq, rng, 7, 2, 2, 1, n, 2, 3, False)[0], "sequential", KF_COOP, 1, 2, (1,), 3, 2),
    Cell("sequential-Ntot29-five-controls", lambda jq, rng, n: block_band_problem(jq, rng, 29, 3, 1, [1, 0, 2, 1, 1], n, 3, 3)[0],
         "sequential", KF_COOP, 2, 2, (0,), 3, 5),
)
BY_NAME = {c.name: c for c in CELLS}
ENSEMBLES = ("one-node", "five-nodes")


def test_the_cells_cover_what_the_feature_touches():
    assert {c.route for c in CELLS} == {"lane", "rowlane", "quad", "sequential"}
    assert {(c.route, c.size) for c in CELLS} >= {("rowlane", 12), ("rowlane", 16)}
    assert {c.objFuncType for c in CELLS} == {1, 2, 3}
    assert {(c.nsteps, ch) for c in CELLS for ch in c.chunks} >= {(1, 0), (2, 0), (2, 1), (7, 0), (7, 3), (8, 3)}
    assert any(c.Nc > 4 for c in CELLS) and any(c.Nc == 4 for c in CELLS)      # (two control groups; a full group)
    for c in CELLS:
        if c.route == "sequential":
            assert c.family == KF_COOP      # (the run-time-size kernels report themselves as cooperative)


def one_frequency(p):
    """the generators of the 4 x 4 x n and block-band problems draw two carrier frequencies; the rank condition of the reference is stated
    for one, and a table does not know of carriers"""
    p.Cfreq = np.asfortranarray(np.asarray(p.Cfreq)[:, :1].copy())
    p.Nfreq = 1
    return p


Problem = collections.namedtuple("Problem", "p S V ens")
_problems = {}


def problem(jq, cell):
    """the problem of a cell, its table, its direction tables, and per ensemble (nodes, weights, shift, CPU gradients, CPU products)
    -- computed once, shared by the tests that use the cell and never modified"""
    if cell.name not in _problems:
        rng = np.random.default_rng(61000 + 17 * CELLS.index(cell))
        p = one_frequency(cell.build(jq, rng, cell.nsteps))
        assert p.nsteps == cell.nsteps and p.objFuncType == cell.objFuncType and p.Ncoupled == cell.Nc and p.Nfreq == 1
        nf, nt = 2 * p.Ncoupled, 2 * p.nsteps + 1
        S = SR.piecewise_constant_table(rng, nf, nt)
        V = rng.standard_normal((nf, nt, NDIR))
        shift = 0.05 * rng.standard_normal(p.Ntot)
        shift[0] = 0.0
        ens = {}
        for name, nodes, weights in (("one-node", np.zeros(1), np.ones(1)), ("five-nodes", 0.1 * rng.standard_normal(5), rng.random(5))):
            ref = SR.SampledHessianReference(jq, p, nodes, weights, shift)
            x = ref.coefficients(S)
            hv = [ref.hvp(S, V[:, :, j], x) for j in range(NDIR)]
            ens[name] = dict(nodes=nodes, weights=weights, shift=shift, ref=ref, grads=ref.gradients(S, x), hv=hv)
            assert ref.residual <= 1e-13, ref.residual
        _problems[cell.name] = Problem(p, S, V, ens)
    return _problems[cell.name]


def handle(jq, p, chunk, extra=None):
    opts = dict(extra or {})
    if chunk:
        opts["chunk_steps"] = chunk
    ncoeff = 2 * p.Ncoupled * p.Nfreq * (2 * p.nsteps + 3)      # (the coefficient count of the spline calls around; a table call does not read it)
    return jq.Working_Arrays_HIP(p, ncoeff, options=opts or None)


def check_route(cell, wa, nq, chunk, rounds=None):
    info = wa.plan_info()["sampled_hvp"]
    assert info["route"] == cell.route, (cell.name, info)
    assert info["time_points"] == 2 * cell.nsteps + 1 and info["nodes"] == nq and info["chunk_steps"] == (chunk or cell.nsteps), info
    assert set(info) == {"route", "directions_per_launch", "chunk_steps", "rounds", "time_points", "nodes"}
    if rounds is not None:
        assert info["rounds"] == rounds, info
    t = wa.last_timing()
    assert t["kernel_family"] == cell.family and t["kernel_size"] == cell.size, (cell.name, t["kernel_family"], t["kernel_size"])
    assert t["n_forward_launches"] > 0 and t["n_backward_launches"] == t["n_forward_launches"] * (2 if cell.objFuncType != 1 else 1) * (2 if cell.Nc > 4 else 1)


def check_against_reference(tag, r, e, two):
    for k in ("infid_grad", "leak_grad"):
        rel = np.linalg.norm(r[k] - e["grads"][k]) / max(np.linalg.norm(e["grads"][k]), 1e-300)
        print("%s %s: relative %.2e (|reference| %.3e)" % (tag, k, rel, np.linalg.norm(e["grads"][k])))
    for j, t in enumerate(e["hv"]):
        for k in ("hv_infid", "hv_leak"):
            rel = np.linalg.norm(r[k][:, :, j] - t[k]) / max(np.linalg.norm(t[k]), 1e-300)
            print("%s %s[:, :, %d]: relative %.2e (|reference| %.3e)" % (tag, k, j, rel, np.linalg.norm(t[k])))
    for k in ("infid_grad", "leak_grad"):
        assert reference_pass(r[k], e["grads"][k]), (tag, k)
    for j, t in enumerate(e["hv"]):
        for k in ("hv_infid", "hv_leak"):
            assert reference_pass(r[k][:, :, j], t[k]), (tag, k, j)
    if not two:
        assert not r["leak_grad"].any() and not r["hv_leak"].any()
    assert np.all(np.any(r["hv_infid"] != 0.0, axis=0))      # (every time point of every direction carries a product)


@pytest.mark.parametrize("which", ENSEMBLES)
@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_products_and_gradients_against_the_cpu_reference(jq, cell, which):
    pr = problem(jq, cell)
    p, e = pr.p, pr.ens[which]
    nf, nt = pr.S.shape
    runs = []
    for chunk in cell.chunks:
        wa = handle(jq, p, chunk)
        try:
            assert "sampled_hvp" not in wa.plan_info()
            r = jq.eval_f_g_grad_samples_hvp(pr.S, pr.V, p, wa, e["nodes"], e["weights"], e["shift"])
            check_route(cell, wa, e["nodes"].size, chunk)
            assert "ens_hvp" not in wa.plan_info() and "hvp" not in wa.plan_info()      # (those records stay the coefficient calls')
            assert r["infid_grad"].shape == r["leak_grad"].shape == (nf, nt) and r["hv_infid"].shape == r["hv_leak"].shape == (nf, nt, NDIR)
            check_against_reference("%s %s chunk %d" % (cell.name, which, chunk), r, e, p.objFuncType != 1)
            # objective and gradients: the sampled-controls call on the same handle
            s = jq.eval_f_g_grad_samples(pr.S, p, wa, e["nodes"], e["weights"], e["shift"])
            for k in ("infidelity", "leak", "infid_grad", "leak_grad"):
                assert reference_pass(r[k], s[k]), (cell.name, k)
            if which == "one-node":      # the one-node wrapper: the same call
                t = jq.traceobjgrad_samples_hvp(pr.S, pr.V, p, wa)
                assert t["objfv"] == r["infidelity"] + r["leak"] and np.array_equal(t["hv_infid"], r["hv_infid"])
                assert np.array_equal(t["hv"], r["hv_infid"] + r["hv_leak"]) and np.array_equal(t["totalgrad"], r["infid_grad"] + r["leak_grad"])
            runs.append(r)
        finally:
            wa.close()
    if len(runs) > 1:      # across chunk lengths: equal to rounding (bit-identity is not promised)
        for k in ("infid_grad", "hv_infid"):
            assert reference_pass(runs[1][k], runs[0][k]), (cell.name, k)


CROSS = ("lane-Ntot5-2steps", "rowlane12-Ntot12", "quad-Ntot32", "sequential-Ntot7")


@pytest.mark.parametrize("name", CROSS)
def test_cross_check_against_the_coefficient_call_on_the_device(jq, name):
    """S = control_samples(pcof), V = B d: B' hv is eval_f_g_grad_hvp(pcof, d) on the same handle, the routes are equal, and the primal
    gradients are eval_f_g_grad_samples'"""
    cell = BY_NAME[name]
    pr = problem(jq, cell)
    p, e = pr.p, pr.ens["five-nodes"]
    rng = np.random.default_rng(5 + CELLS.index(cell))
    wa = handle(jq, p, cell.chunks[-1])
    try:
        ncoeff = int(wa.nCoeff)
        pcof, d = 0.3 * rng.standard_normal(ncoeff), rng.standard_normal((ncoeff, NDIR))
        B = jq.spline_sample_matrix(p, ncoeff, jq.control_sample_times(p, wa))
        S = jq.control_samples(pcof, p, wa)
        V = (B @ d).reshape(S.shape + (NDIR,), order="F")
        c = jq.eval_f_g_grad_hvp(pcof, d, p, wa, e["nodes"], e["weights"], e["shift"])
        kernels = wa.plan_info()["last_kernels"]
        r = jq.eval_f_g_grad_samples_hvp(S, V, p, wa, e["nodes"], e["weights"], e["shift"])
        plan = wa.plan_info()
        assert plan["sampled_hvp"]["route"] == plan["ens_hvp"]["route"] == cell.route
        assert plan["last_kernels"] == kernels      # (the same propagator objects)
        for k in ("directions_per_launch", "chunk_steps", "rounds"):
            assert plan["sampled_hvp"][k] == plan["ens_hvp"][k], k
        for k in ("hv_infid", "hv_leak"):
            for j in range(NDIR):
                folded = B.T @ r[k][:, :, j].ravel(order="F")
                rel = np.linalg.norm(folded - c[k][:, j]) / max(np.linalg.norm(c[k][:, j]), 1e-300)
                print("%s B' %s[:, :, %d] against the coefficient call: relative %.2e" % (name, k, j, rel))
                assert reference_pass(folded, c[k][:, j]), (k, j, rel)
        assert reference_pass(r["infidelity"], c["infidelity"]) and reference_pass(r["leak"], c["leak"])
        s = jq.eval_f_g_grad_samples(S, p, wa, e["nodes"], e["weights"], e["shift"])
        for k in ("infid_grad", "leak_grad"):
            assert reference_pass(r[k], s[k]), k
            assert reference_pass(B.T @ r[k].ravel(order="F"), c[k]), k
    finally:
        wa.close()


def test_directions_alone_among_three_and_in_rounds_are_the_same_bits(jq):
    """a direction's product does not depend on the launch it rides in: alone, among three, and -- under a stream budget that holds the
    primal stream and ONE direction (the option of test_rounds_and_the_calls_around_are_the_same_bits) -- in three rounds; an all-zero
    direction returns exact zeros; two identical calls give identical bits; traceobjgrad, traceobjgrad_samples and eval_f_g_grad_hvp on
    the same handle return the same bits before and after"""
    cell = BY_NAME["rowlane12-Ntot12"]
    pr = problem(jq, cell)
    p, e = pr.p, pr.ens["five-nodes"]
    args = (e["nodes"], e["weights"], e["shift"])
    stride = 16 * 12      # doubles of a row-lane operator image at NPJ 12
    wa = handle(jq, p, 0)
    wb = handle(jq, p, cell.nsteps, {"stream_bytes": 8 * 2 * 2 * stride * (2 * cell.nsteps + 1)})
    rng = np.random.default_rng(12)
    try:
        pcof, d = 0.3 * rng.standard_normal(int(wa.nCoeff)), rng.standard_normal((int(wa.nCoeff), 2))

        def around(w):
            a = jq.traceobjgrad(pcof, p, w, False, True)
            b = jq.traceobjgrad_samples(pr.S, p, w, True)
            c = jq.eval_f_g_grad_hvp(pcof, d, p, w, *args)
            return [np.asarray(v) for v in a] + [np.asarray(v) for v in b] + [np.asarray(c[k]) for k in sorted(c)], w.plan_info()["ens_hvp"]

        before = [around(w) for w in (wa, wb)]
        a, b = [jq.eval_f_g_grad_samples_hvp(pr.S, pr.V, p, w, *args) for w in (wa, wb)]
        check_route(cell, wa, 5, 0, rounds=1)
        check_route(cell, wb, 5, 0, rounds=3)
        assert wa.plan_info()["sampled_hvp"]["directions_per_launch"] == 3 and wb.plan_info()["sampled_hvp"]["directions_per_launch"] == 1
        for w, ens_before in ((wa, before[0][1]), (wb, before[1][1])):
            assert w.plan_info()["ens_hvp"] == ens_before and "hvp" not in w.plan_info()
        again = jq.eval_f_g_grad_samples_hvp(pr.S, pr.V, p, wa, *args)
        for k in a:
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], again[k]), k
        for j in range(NDIR):
            one = jq.eval_f_g_grad_samples_hvp(pr.S, pr.V[:, :, j], p, wa, *args)
            assert wa.plan_info()["sampled_hvp"]["directions_per_launch"] == 1
            for k in ("hv_infid", "hv_leak"):
                assert np.array_equal(one[k][:, :, 0], a[k][:, :, j]), (k, j)
            for k in ("infidelity", "leak", "infid_grad", "leak_grad"):
                assert np.array_equal(one[k], a[k]), k
        Vz = pr.V.copy()
        Vz[:, :, 1] = 0.0
        z = jq.eval_f_g_grad_samples_hvp(pr.S, Vz, p, wa, *args)
        assert np.all(z["hv_infid"][:, :, 1] == 0.0) and np.all(z["hv_leak"][:, :, 1] == 0.0)
        for j in (0, 2):
            assert np.array_equal(z["hv_infid"][:, :, j], a["hv_infid"][:, :, j])
        after = [around(w) for w in (wa, wb)]
        for (x, _), (y, _) in zip(before, after):
            assert len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y))
    finally:
        wa.close()
        wb.close()


def test_zero_directions_and_determinism_on_a_two_pass_route(jq):
    """objFuncType 2 on the lane route in chunks of one step: hv_leak = forced - unforced of an all-zero direction is an exact zero too"""
    cell = BY_NAME["lane-Ntot5-2steps"]
    pr = problem(jq, cell)
    p, e = pr.p, pr.ens["five-nodes"]
    wa = handle(jq, p, 1)
    try:
        z = jq.eval_f_g_grad_samples_hvp(pr.S, np.zeros_like(pr.S), p, wa, e["nodes"], e["weights"], e["shift"])
        assert z["hv_infid"].shape == pr.S.shape + (1,) and np.all(z["hv_infid"] == 0.0) and np.all(z["hv_leak"] == 0.0)
        assert z["infid_grad"].any() and z["leak_grad"].any()
        a = jq.eval_f_g_grad_samples_hvp(pr.S, pr.V, p, wa, e["nodes"], e["weights"], e["shift"])
        b = jq.eval_f_g_grad_samples_hvp(pr.S, pr.V, p, wa, e["nodes"], e["weights"], e["shift"])
        assert all(np.array_equal(a[k], b[k]) for k in a)
    finally:
        wa.close()


SENT = -7.25


def _call(L, lib, h, tab, nt, dirs, ndir, nodes, weights, nq, outs, null=()):
    dp = lambda a: a.ctypes.data_as(lib.c_dp)
    args = [h, dp(tab), nt, dp(dirs), ndir, dp(nodes), dp(weights), nq, None] + [dp(o) for o in outs]
    for k in null:
        args[k] = None
    return L.jq_eval_f_g_grad_samples_hvp(*args)


@pytest.mark.parametrize("which", range(5), ids=REFUSALS)
def test_refusals_write_nothing_and_leave_the_handle_alone(jq, which):
    """everything tl_refuse(..., true) refuses -- the uncoupled handle is what samples_refuse refuses as well -- on a handle per cause"""
    from juqbox_jl_amd import _lib
    L = _lib.load()
    name, p, pcof, WA = _refusal_handles(jq)[which]
    assert name == REFUSALS[which]
    wa = WA(p, pcof.size)
    try:
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        nt, nf = 2 * p.nsteps + 1, 2 * max(int(p.Ncoupled), int(getattr(p, "Nunc", 0)))
        n = nf * nt
        tab, dirs = np.zeros(n), np.ones(n)
        outs = [np.full(k, SENT) for k in (2, n, n, n, n)]
        rc = _call(L, _lib, wa.handle, tab, nt, dirs, 1, np.zeros(1), np.ones(1), 1, outs)
        assert rc == _lib.JQ_EUNSUPPORTED, (name, rc)
        msg = L.jq_last_error(wa.handle).decode()
        assert "jq_eval_f_g_grad_samples_hvp" in msg and len(msg) > 40
        assert all(np.all(o == SENT) for o in outs)
        assert "sampled_hvp" not in wa.plan_info()
        if name != "uncoupled":      # (the Python layer sizes a table by Ncoupled)
            with pytest.raises(_lib.JuqboxHipError) as e:
                jq.eval_f_g_grad_samples_hvp(tab.reshape((nf, nt), order="F"), dirs.reshape((nf, nt), order="F"), p, wa)
            assert e.value.code == _lib.JQ_EUNSUPPORTED
        after = jq.traceobjgrad(pcof, p, wa, False, True)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
    finally:
        wa.close()


def test_argument_codes_write_nothing_and_leave_the_handle_alone(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    cell = BY_NAME["lane-Ntot5-2steps"]
    pr = problem(jq, cell)
    p = pr.p
    nf, nt = pr.S.shape
    n = nf * nt
    wa = handle(jq, p, 0)
    try:
        pcof = 0.3 * np.random.default_rng(3).standard_normal(int(wa.nCoeff))
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        good, dirs = SR.flat(pr.S), np.concatenate([SR.flat(pr.V[:, :, j]) for j in range(2)])
        nodes, weights = np.zeros(1), np.ones(1)
        outs = [np.full(k, SENT) for k in (2, n, n, 2 * n, 2 * n)]
        call = lambda tab=good, nt_=nt, d=dirs, nd=2, nq=1, null=(): _call(L, _lib, wa.handle, tab, nt_, d, nd, nodes, weights, nq, outs, null)
        for k in (1, 3, 5, 6, 9, 10, 11, 12, 13):      # every required pointer
            assert call(null=(k,)) == _lib.JQ_EINVAL, k
        for nt_ in (nt - 1, nt + 1, 0):
            assert call(nt_=nt_) == _lib.JQ_EINVAL, nt_
        assert call(nd=0) == _lib.JQ_EINVAL and call(nd=-1) == _lib.JQ_EINVAL and call(nq=0) == _lib.JQ_EINVAL
        for bad_value in (np.nan, np.inf):
            bad = good.copy()
            bad[nf + 1] = bad_value
            assert call(tab=bad) == _lib.JQ_EINVAL
            bad = dirs.copy()
            bad[-1] = bad_value      # (the last entry of the SECOND table)
            assert call(d=bad) == _lib.JQ_EINVAL
            assert len(L.jq_last_error(wa.handle)) > 0
        assert all(np.all(o == SENT) for o in outs)
        assert "sampled_hvp" not in wa.plan_info()
        after = jq.traceobjgrad(pcof, p, wa, False, True)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        assert call() == _lib.JQ_OK
        assert all(np.all(o != SENT) for o in outs) and outs[3].any() and outs[4].any()
        r = jq.eval_f_g_grad_samples_hvp(pr.S, pr.V[:, :, :2], p, wa)
        assert np.array_equal(SR.flat(r["hv_infid"][:, :, 1]), outs[3][n:]) and np.array_equal(SR.flat(r["leak_grad"]), outs[2])
    finally:
        wa.close()


def test_sampled_hessvec_with_the_spline_matrix_is_the_coefficient_product(jq):
    import torch
    from juqbox_jl_amd.torch_controls import sampled_hessvec
    cell = BY_NAME["rowlane12-Ntot12"]
    pr = problem(jq, cell)
    p, e = pr.p, pr.ens["five-nodes"]
    nf, nt = pr.S.shape
    rng = np.random.default_rng(77)
    wa = handle(jq, p, 3)
    try:
        ncoeff = int(wa.nCoeff)
        pcof, d = 0.3 * rng.standard_normal(ncoeff), rng.standard_normal(ncoeff)
        B = torch.from_numpy(jq.spline_sample_matrix(p, ncoeff, jq.control_sample_times(p, wa)))
        fn = lambda x: (B @ x).reshape(nt, nf).T
        for ens in ((), (e["nodes"], e["weights"], e["shift"])):
            got = sampled_hessvec(fn, torch.from_numpy(pcof), torch.from_numpy(d), p, wa, *ens).numpy()
            assert wa.plan_info()["sampled_hvp"]["route"] == "rowlane"
            c = jq.eval_f_g_grad_hvp(pcof, d, p, wa, *ens)
            want = (c["hv_infid"] + c["hv_leak"])[:, 0]
            rel = np.linalg.norm(got - want) / np.linalg.norm(want)
            print("sampled_hessvec(B) against eval_f_g_grad_hvp, %d node(s): relative %.2e" % (len(ens[0]) if ens else 1, rel))
            assert got.shape == (ncoeff,) and reference_pass(got, want)
    finally:
        wa.close()


def test_sampled_hessvec_with_tanh_saturated_segment_amplitudes(jq):
    """a non-linear parameterisation: 2 Nc x 4 amplitudes, saturated by amp tanh(.), each held for a quarter of the time points
    (repeat_interleave).  Reference in numpy: Jfn' (Hs (Jfn v)) from the CPU reference's product along the table Jfn v, plus the curvature
    term fn''(theta) v . (the oracle's sample gradient summed over the segment)."""
    import torch
    from juqbox_jl_amd.torch_controls import sampled_hessvec
    cell = BY_NAME["rowlane12-Ntot12"]
    pr = problem(jq, cell)
    p, e = pr.p, pr.ens["five-nodes"]
    nf, nt = pr.S.shape
    nseg, rep, amp = 4, (nt + 3) // 4, 0.5
    rng = np.random.default_rng(78)
    theta, v = rng.standard_normal((nf, nseg)), rng.standard_normal((nf, nseg))
    fn = lambda th: (amp * torch.tanh(th)).repeat_interleave(rep, dim=1)[:, :nt]
    seg = np.arange(nt) // rep
    th1, th2 = amp * (1.0 - np.tanh(theta) ** 2), -2.0 * amp * np.tanh(theta) * (1.0 - np.tanh(theta) ** 2)
    S, U = (amp * np.tanh(theta))[:, seg], (th1 * v)[:, seg]
    ref = e["ref"]
    x = ref.coefficients(S)
    g = ref.gradients(S, x)["totalgrad"]
    Hu = ref.hvp(S, U, x)["hv"]
    want = np.stack([th1[:, k] * Hu[:, seg == k].sum(axis=1) + th2[:, k] * v[:, k] * g[:, seg == k].sum(axis=1) for k in range(nseg)], axis=1)
    curvature = np.stack([th2[:, k] * v[:, k] * g[:, seg == k].sum(axis=1) for k in range(nseg)], axis=1)
    assert np.linalg.norm(curvature) > 1e-3 * np.linalg.norm(want)      # (the second term is not negligible here)
    wa = handle(jq, p, 3)
    try:
        got = sampled_hessvec(fn, torch.from_numpy(theta), torch.from_numpy(v), p, wa, e["nodes"], e["weights"], e["shift"]).numpy()
        assert wa.plan_info()["sampled_hvp"] == {"route": "rowlane", "directions_per_launch": 1, "chunk_steps": 3, "rounds": 1, "time_points": nt, "nodes": 5}
    finally:
        wa.close()
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("sampled_hessvec(tanh segments) against the CPU reference: relative %.2e (curvature term %.1e of it)"
          % (rel, np.linalg.norm(curvature) / np.linalg.norm(want)))
    assert got.shape == theta.shape and reference_pass(got, want)
