"""GPU (-m gpu): controls given as samples on the time grid (jq_traceobjgrad_samples, jq_eval_f_g_grad_samples, jq_control_samples,
jq_sample_times; torch_controls.SampledObjective) on every kernel family.

The reference is the CPU oracle, which knows spline coefficients only.  With D1 = 2 nsteps + 3 coefficients per spline the matrix
B = d pq / d pcof (spline_sample_matrix, pinned against the oracle in tests/test_sampled_controls_host.py) has full ROW rank: every sample
table is B pcof for some pcof, and no component of a sample gradient G is invisible in B' G, which the oracle's coefficient gradient checks.

One small problem per place the new code can go wrong (CELLS): the seven kernel families, asserted from jq_last_timing; objFuncType
1 / 2 / 3; Neumann order 0 and 3; the Jacobi solver; the implicit-midpoint integrator; five controls (two control groups); rank-2 full
leakage weights; time loops of 1 step, 2 steps in (2) and (1, 1), 7 steps in one chunk and in 3 + 3 + 1, 8 steps in 3 + 3 + 2 -- every
boundary point, both parities, boundaries shared by two launches."""
import collections
import copy
import ctypes

import numpy as np
import pytest
from conftest import case_inputs, reference_pass

from block_band_problem import block_band_problem
from subsystem_problem import subsystem_problem
from test_gpu_random import random_problem
from uncoupled_problem import FD_NEUMANN_TERMS

pytestmark = pytest.mark.gpu

# kernel_family codes of jq_timing (include/juqbox_hip.h)
SLAB, COOP, LANE, ROWLANE, ROWLANE_IMR, QUAD, CQ = 0, 1, 2, 3, 4, 6, 8
DENSE_POLICY_BAND = 10

Cell = collections.namedtuple("Cell", "name build options family nsteps chunks kind")
# build(jq, rng, nsteps) -> params; options: of the handle; chunks: option chunk_steps per run (0: one chunk); kind: neumann / jacobi / imr


def _short_swap02(jq, rng, nsteps):
    p, info = jq.cases.swap02()
    p.T = p.T * nsteps / p.nsteps
    p.nsteps = nsteps
    return p


def _swap02_full_weights(jq, rng, nsteps):
    from test_gpu_dense_wmat import set_forbidden
    p = _short_swap02(jq, rng, nsteps)
    set_forbidden(p, rng, 2)
    return p


def _swap02_imr(jq, rng, nsteps):
    p = _short_swap02(jq, rng, nsteps)
    p.Integrator_id = jq.Implicit_Midpoint
    p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=60, tol=1e-11, nrhs=p.N)
    p.wmat = p.wmat_real.copy()
    return p


def _band29_jacobi(jq, rng, nsteps):
    p = block_band_problem(jq, rng, 29, 3, 1, [1, 0, 2], nsteps, 3, 2)[0]
    p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER, max_iter=80, tol=1e-12, nrhs=p.N)
    return p


CELLS = (
    Cell("rowlane-swap02", _short_swap02, {}, ROWLANE, 7, (0, 3), "neumann"),
    Cell("rowlane-fullweights", _swap02_full_weights, {}, ROWLANE, 2, (0,), "neumann"),
    Cell("rowlane-imr", _swap02_imr, {}, ROWLANE_IMR, 7, (0, 3), "imr"),
    Cell("rowlane-random4", lambda jq, rng, n: random_problem(jq, rng, 4, 3, 2, 1, n, 3, 1, False)[0], {}, ROWLANE, 7, (0, 3), "neumann"),
    Cell("lane-Ntot5", lambda jq, rng, n: random_problem(jq, rng, 5, 2, 2, 1, n, 0, 2, False)[0], {"rowlane_max": 0}, LANE, 2, (1,), "neumann"),
    Cell("cq-dense-Ntot29", lambda jq, rng, n: random_problem(jq, rng, 29, 3, 2, 1, n, 3, 3, False)[0], {}, CQ, 8, (3,), "neumann"),
    Cell("cq-Ntot32", lambda jq, rng, n: subsystem_problem(jq, rng, 2, 32, 4, 3, 3, "varied", n, 1)[0], {}, CQ, 7, (0, 3), "neumann"),
    Cell("quad-Ntot32", lambda jq, rng, n: subsystem_problem(jq, rng, 2, 32, 4, 3, 0, "varied", n, 2)[0], {"cq": 0}, QUAD, 1, (0,), "neumann"),
    Cell("coop-Ntot29-five-controls", lambda jq, rng, n: block_band_problem(jq, rng, 29, 3, 1, [1, 0, 2, 1, 1], n, 3, 3)[0],
         {"cq": 0, "dq": 0}, COOP, 2, (0,), "neumann"),
    Cell("slab-Ntot29-jacobi", _band29_jacobi, {"cq": 0, "dq": 0, "coop_max": 0}, SLAB, 8, (3,), "jacobi"),
)
BY_NAME = {c.name: c for c in CELLS}


def test_the_cells_cover_what_the_feature_touches():
    assert {c.family for c in CELLS} >= {SLAB, COOP, LANE, ROWLANE, QUAD, CQ}
    assert {c.kind for c in CELLS} == {"neumann", "jacobi", "imr"}
    assert {(c.nsteps, ch) for c in CELLS for ch in c.chunks} >= {(1, 0), (2, 0), (2, 1), (7, 0), (7, 3), (8, 3)}


Problem = collections.namedtuple("Problem", "p pcof nodes weights shift ref")
_problems = {}


def problem(jq, cell):
    """the problem of a cell with a coefficient vector of D1 = 2 nsteps + 3, its ensemble and the ORACLE's results, computed once"""
    if cell.name not in _problems:
        from oracle.oracle import Oracle
        rng = np.random.default_rng(77000 + 13 * CELLS.index(cell))
        p = cell.build(jq, rng, cell.nsteps)
        assert p.nsteps == cell.nsteps
        D1 = 2 * cell.nsteps + 3
        pcof = 0.3 * rng.standard_normal(2 * p.Ncoupled * p.Nfreq * D1)
        if cell.name.startswith("rowlane-swap02") or "imr" in cell.name or "fullweights" in cell.name:
            pcof *= 0.05      # (swap02's controls are bounded by maxpar = 0.02)
        nodes, weights = 0.1 * rng.standard_normal(5), rng.random(5)
        shift = 0.05 * rng.standard_normal(p.Ntot)
        shift[0] = 0.0
        o = Oracle(p, use_sparse=False)
        ref = o.traceobjgrad_imr(pcof, 60, 1e-11) if cell.kind == "imr" else o.traceobjgrad(pcof)
        _problems[cell.name] = Problem(p, pcof, nodes, weights, shift, ref)
    return _problems[cell.name]


def handle(jq, cell, p, ncoeff, chunk):
    opts = dict(cell.options)
    if chunk:
        opts["chunk_steps"] = chunk
    WA = jq.Working_Arrays_M_HIP if cell.kind == "imr" else jq.Working_Arrays_HIP
    return WA(p, ncoeff, options=opts)


def fold(B, G):
    return B.T @ np.asarray(G).ravel(order="F")


def check_family(cell, wa):
    t = wa.last_timing()
    assert t["kernel_family"] == cell.family, (cell.name, t["kernel_family"], t["kernel_band"])
    if cell.name.startswith("cq-dense"):
        assert t["kernel_band"] == DENSE_POLICY_BAND, t


def run_cell(jq, cell):
    """every chunking of a cell: [(chunk, out4 forward-only, out4 with the adjoint, totalgrad, infidelgrad, leakgrad samples gradients, B, the
    library's own spline results, ensemble figures)]"""
    pr = problem(jq, cell)
    p, pcof = pr.p, pr.pcof
    runs = []
    for chunk in cell.chunks:
        wa = handle(jq, cell, p, pcof.size, chunk)
        try:
            times = jq.control_sample_times(p, wa)
            B = jq.spline_sample_matrix(p, pcof.size, times)
            pq = jq.control_samples(pcof, p, wa)
            own = jq.traceobjgrad(pcof, p, wa, False, True)
            own_fwd = jq.traceobjgrad(pcof, p, wa, False, False)
            fwd = jq.traceobjgrad_samples(pq, p, wa, False)
            check_family(cell, wa)
            adj = jq.traceobjgrad_samples(pq, p, wa, True)
            check_family(cell, wa)
            again = jq.traceobjgrad_samples(pq, p, wa, True)
            info = wa.plan_info()["sampled_controls"]
            ens = []
            for nq in (1, 5):
                jq.eval_f_g_grad(pcof, p, wa, pr.nodes[:nq], pr.weights[:nq], True, shift=pr.shift)
                spline = (p.last_infidelity, p.last_leak, p.last_infidelity_grad.copy(), p.last_leak_grad.copy())
                ens.append((spline, jq.eval_f_g_grad_samples(pq, p, wa, pr.nodes[:nq], pr.weights[:nq], pr.shift)))
            runs.append(dict(chunk=chunk, times=times, B=B, pq=pq, own=own, own_fwd=own_fwd, fwd=fwd, adj=adj, again=again, info=info, ens=ens))
        finally:
            wa.close()
    return runs


_runs = {}


def runs_of(jq, cell):
    if cell.name not in _runs:
        _runs[cell.name] = run_cell(jq, cell)
    return _runs[cell.name]


def grad_ok(cell, value, ref, scale):
    """the reference's criterion (test/evalGrad.jl: atol 1e-14 or rtol 1e-10); implicit midpoint: the project's stated 1e-9 of the total
    gradient's norm (exception (i)), as tests/test_gpu_block_band.py; Jacobi at tol 1e-12: the reference's criterion"""
    if cell.kind == "imr":
        return np.linalg.norm(value - ref) <= 1e-9 * scale
    return reference_pass(value, ref)


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_forward_bits_and_gradient_against_the_oracle(jq, cell):
    pr = problem(jq, cell)
    p, ref = pr.p, pr.ref
    nt = 2 * cell.nsteps + 1
    for r in runs_of(jq, cell):
        assert r["times"].shape == (nt,) and r["times"][0] == 0.0 and np.all(np.diff(r["times"]) > 0) and abs(r["times"][-1] - p.T) <= 1e-12 * p.T
        assert r["pq"].shape == (2 * p.Ncoupled, nt)
        assert r["info"] == {"time_points": nt, "nodes": 1, "chunk_steps": r["info"]["chunk_steps"]}
        if r["chunk"]:
            assert r["info"]["chunk_steps"] == r["chunk"]
        # the library's controls are the oracle's at those times (another order of operations)
        from oracle.oracle import Oracle
        o = Oracle(p, use_sparse=False)
        for J in (0, 1, nt // 2, nt - 2, nt - 1):
            assert np.allclose(r["pq"][:, J], o.controls(pr.pcof, r["times"][J]), rtol=0, atol=1e-12)
        # 1. forward bit-identity: the objective of the handle's own controls, forward-only and with the adjoint
        objfv, tg, prim, sec, tinf, ig, lg = r["own"]
        assert r["fwd"] == r["own_fwd"] == (objfv, prim, sec)
        a_objfv, G, a_prim, a_sec, a_tinf, Gi, Gl = r["adj"]
        assert (a_objfv, a_prim, a_sec, a_tinf) == (objfv, prim, sec, tinf)
        for (s_inf, s_leak, s_ig, s_lg), e in r["ens"]:
            assert (e["infidelity"], e["leak"]) == (s_inf, s_leak)
        # 4. deterministic
        assert all(np.array_equal(x, y) for x, y in zip(r["adj"], r["again"]))
        # 2. B' G against the ORACLE's coefficient gradients
        B = r["B"]
        scale = np.linalg.norm(ref["totalgrad"])
        got = {"totalgrad": fold(B, G), "infidelgrad": fold(B, Gi)}
        assert G.shape == Gi.shape == (2 * p.Ncoupled, nt)
        if p.objFuncType != 1:
            got["leakgrad"] = fold(B, Gl)
            assert np.array_equal(Gl, G - Gi)
        else:
            assert Gl.size == 0 and np.array_equal(G, Gi)
        for name, v in got.items():
            d_or = np.linalg.norm(v - ref[name]) / max(np.linalg.norm(ref[name]), 1e-300)
            d_own = np.linalg.norm(v - {"totalgrad": tg, "infidelgrad": ig, "leakgrad": lg}[name]) / max(np.linalg.norm(ref[name]), 1e-300)
            print("%s chunk %d %s: |B'G - oracle| / |oracle| = %.2e, |B'G - traceobjgrad| / |oracle| = %.2e (|oracle| %.3e)"
                  % (cell.name, r["chunk"], name, d_or, d_own, np.linalg.norm(ref[name])))
        for name, v in got.items():
            if cell.kind == "imr" and name == "leakgrad":
                continue
            assert grad_ok(cell, v, ref[name], scale), (cell.name, r["chunk"], name)
        # the ensemble's gradients fold to the spline call's (the oracle pins that call in tests/test_gpu_random.py, at 1e-10 of the
        # infidelity gradient's norm for both gradients; implicit midpoint 1e-9): the same sweeps, so the same bound
        for (s_inf, s_leak, s_ig, s_lg), e in r["ens"]:
            bound = (1e-9 if cell.kind == "imr" else 1e-10) * np.linalg.norm(s_ig)
            assert np.linalg.norm(fold(B, e["infid_grad"]) - s_ig) <= bound
            if p.objFuncType != 1:
                assert np.linalg.norm(fold(B, e["leak_grad"]) - s_lg) <= bound
            else:
                assert s_lg.size == 0 and np.all(e["leak_grad"] == 0.0)
        # 4. implicit midpoint reads the half points only: exact zeros at the integer points
        if cell.kind == "imr":
            assert np.all(G[:, 0::2] == 0.0) and np.all(Gi[:, 0::2] == 0.0) and np.any(G[:, 1::2] != 0.0)
        else:
            assert np.all(np.any(G != 0.0, axis=0))      # (every time point carries gradient)
    # 4. across chunk lengths: equal to rounding (bit-identity is not promised)
    rs = runs_of(jq, cell)
    if len(rs) > 1:
        for k in (1, 5):
            assert reference_pass(rs[1]["adj"][k], rs[0]["adj"][k]), (cell.name, k)


def richardson(f, x, d, h, levels=3):
    """central differences of f along d at steps h, h / 2, ...: extrapolated to O(h^(2 levels)) (tests/test_uncoupled_matrix.py)"""
    T = [[(f(x + (h / 2 ** i) * d) - f(x - (h / 2 ** i) * d)) / (2 * h / 2 ** i)] for i in range(levels)]
    for i in range(1, levels):
        for k in range(1, i + 1):
            T[i].append(T[i][k - 1] + (T[i][k - 1] - T[i - 1][k - 1]) / (4 ** k - 1))
    return T[-1][-1]


def test_index_maps_with_an_asymmetric_piecewise_constant_pulse(jq):
    """Samples that are NOT the handle's splines: every control function a different random piecewise-constant pulse, asymmetric in time.
    B has full row rank, so the table is B x for x = pinv(B) pq and the ORACLE evaluates it; its objective's Richardson-extrapolated
    central differences along single coefficients at the start, in the middle and at the end of the time interval -- B d is non-zero at a
    few neighbouring time points only -- must equal (B d)' G.  A reversed or shifted index map fails at order one.  Neumann order 24, where
    the adjoint gradient is the derivative of the objective (pattern and bound of tests/test_uncoupled_matrix.py); 7 steps in 3 + 3 + 1."""
    from oracle.oracle import Oracle
    cell = BY_NAME["rowlane-random4"]
    p = copy.copy(problem(jq, cell).p)
    p.linear_solver = jq.lsolver_object(max_iter=FD_NEUMANN_TERMS)
    assert p.linear_solver.max_iter >= 20
    rng = np.random.default_rng(4711)
    nt, nf, D1 = 2 * p.nsteps + 1, 2 * p.Ncoupled, 2 * p.nsteps + 3
    ncoeff = nf * p.Nfreq * D1
    pq = np.zeros((nf, nt))
    for f in range(nf):      # 3 .. 5 segments with random break points and levels
        cuts = np.sort(rng.choice(np.arange(1, nt), size=int(rng.integers(2, 5)), replace=False))
        for lo, hi in zip(np.r_[0, cuts], np.r_[cuts, nt]):
            pq[f, lo:hi] = 0.4 * rng.standard_normal()
    assert not np.allclose(pq, pq[:, ::-1])
    wa = handle(jq, cell, p, ncoeff, 3)
    try:
        times = jq.control_sample_times(p, wa)
        objfv, G = jq.traceobjgrad_samples(pq, p, wa, True)[:2]
        assert wa.last_timing()["kernel_family"] == ROWLANE
    finally:
        wa.close()
    B = jq.spline_sample_matrix(p, ncoeff, times)
    x = np.linalg.lstsq(B, pq.ravel(order="F"), rcond=None)[0]
    assert np.abs(B @ x - pq.ravel(order="F")).max() <= 1e-13
    o = Oracle(p, use_sparse=False)
    f = lambda v: o.traceobjgrad(v, evaladjoint=False)["objfv"]
    assert abs(f(x) - objfv) <= 1e-12      # (the same table to 1e-13 per sample)
    gnorm = np.linalg.norm(fold(B, G))
    # single coefficients whose knot window lies at the start, in the middle, at the end: the first block of control 0 and the last block of the last control
    picks = [(blk * D1 + k, where) for blk in (0, nf * p.Nfreq - 1) for k, where in ((0, "start"), (D1 // 2, "middle"), (D1 - 1, "end"))]
    for k, where in picks:
        d = np.zeros(ncoeff)
        d[k] = 1.0
        touched = np.unique(np.nonzero((B @ d).reshape((nf, nt), order="F"))[1])
        assert touched.size <= 4 and touched.max() - touched.min() <= 3
        assert {"start": touched.min() == 0, "end": touched.max() == nt - 1, "middle": 0 < touched.min() and touched.max() < nt - 1}[where]
        gd = fold(B, G) @ d
        fd = richardson(f, x, d, 2e-2)
        print("coefficient %d (%s, time points %s): (B d)' G = %.12e, Richardson %.12e, relative difference %.2e (|B' G| %.3e)"
              % (k, where, touched.tolist(), gd, fd, abs(fd - gd) / abs(gd), gnorm))
        assert abs(fd - gd) <= 1e-9 * abs(gd)


def test_refusals_write_nothing_and_leave_the_handle_alone(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
    SENT = -7.25

    def refused(wa, p, pcof, calls):
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        for call, code in calls:
            outs = [np.full(n, SENT) for n in call[1]]
            assert call[0](*[ptr(a) for a in outs]) == code, (call, L.jq_last_error(wa.handle))
            assert all(np.all(a == SENT) for a in outs)
            assert len(L.jq_last_error(wa.handle)) > 0
        after = jq.traceobjgrad(pcof, p, wa, False, True)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))

    # uncoupled controls: ft is a function of both slots
    p, info, pcof, _ = case_inputs("cnot2_lab")
    p.T = p.T * 6 / p.nsteps
    p.nsteps = 6
    nt, nf = 13, 2 * p.Nunc
    tab = np.zeros(nf * nt)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        h = wa.handle
        refused(wa, p, pcof, [
            ((lambda o4, g0, g1, g2: L.jq_traceobjgrad_samples(h, ptr(tab), nt, 1, o4, g0, g1, g2), (4, tab.size, tab.size, tab.size)), _lib.JQ_EUNSUPPORTED),
            ((lambda o2, g0, g1: L.jq_eval_f_g_grad_samples(h, ptr(tab), nt, ptr(np.zeros(1)), ptr(np.ones(1)), 1, None, 1, o2, g0, g1), (2, tab.size, tab.size)), _lib.JQ_EUNSUPPORTED),
            ((lambda out: L.jq_control_samples(h, ptr(pcof), pcof.size, out), (tab.size,)), _lib.JQ_EUNSUPPORTED),
        ])
        t = np.zeros(nt)
        assert L.jq_sample_times(h, ptr(t), nt) == _lib.JQ_OK and t[-1] > 0      # (the grid itself is no control)
    finally:
        wa.close()
    # a wrong number of time points, a sample that is not finite, NULL outputs
    cell = BY_NAME["rowlane-random4"]
    pr = problem(jq, cell)
    p, pcof = pr.p, pr.pcof
    nt, nf = 2 * p.nsteps + 1, 2 * p.Ncoupled
    wa = handle(jq, cell, p, pcof.size, 0)
    try:
        h = wa.handle
        good = np.ascontiguousarray(jq.control_samples(pcof, p, wa).ravel(order="F"))
        bad = good.copy()
        bad[nf * 4 + 1] = np.nan
        inf = good.copy()
        inf[-1] = np.inf
        n = good.size
        calls = []
        for tab_, nt_ in ((good, nt - 1), (good, nt + 1), (good, 0), (bad, nt), (inf, nt)):
            calls.append(((lambda o4, g0, g1, g2, tab_=tab_, nt_=nt_: L.jq_traceobjgrad_samples(h, ptr(tab_), nt_, 1, o4, g0, g1, g2), (4, n, n, n)), _lib.JQ_EINVAL))
            calls.append(((lambda o2, g0, g1, tab_=tab_, nt_=nt_: L.jq_eval_f_g_grad_samples(h, ptr(tab_), nt_, ptr(np.zeros(1)), ptr(np.ones(1)), 1, None, 1, o2, g0, g1), (2, n, n)),
                          _lib.JQ_EINVAL))
        calls.append(((lambda o4: L.jq_traceobjgrad_samples(h, ptr(good), nt, 1, o4, None, None, None), (4,)), _lib.JQ_EINVAL))
        calls.append(((lambda o4: L.jq_traceobjgrad_samples(h, None, nt, 0, o4, None, None, None), (4,)), _lib.JQ_EINVAL))
        calls.append(((lambda o2, g0, g1: L.jq_eval_f_g_grad_samples(h, ptr(good), nt, ptr(np.zeros(1)), ptr(np.ones(1)), 0, None, 1, o2, g0, g1), (2, n, n)), _lib.JQ_EINVAL))
        calls.append(((lambda t: L.jq_sample_times(h, t, nt - 1), (nt,)), _lib.JQ_EINVAL))
        refused(wa, p, pcof, calls)
        # the Python layer refuses shapes and entries that are not finite before the library sees them
        for tab_ in (bad.reshape((nf, nt), order="F"), np.zeros((nf, nt - 1))):
            with pytest.raises(ValueError):
                jq.traceobjgrad_samples(tab_, p, wa)
            with pytest.raises(ValueError):
                jq.eval_f_g_grad_samples(tab_, p, wa, pr.nodes, pr.weights)
    finally:
        wa.close()


def test_autograd_through_the_spline_matrix_and_a_piecewise_constant_pulse(jq):
    import torch
    from juqbox_jl_amd.torch_controls import SampledObjective
    cell = BY_NAME["rowlane-random4"]
    pr = problem(jq, cell)
    p, pcof = pr.p, pr.pcof
    nt, nf = 2 * p.nsteps + 1, 2 * p.Ncoupled
    wa = handle(jq, cell, p, pcof.size, 0)
    try:
        B = torch.from_numpy(jq.spline_sample_matrix(p, pcof.size, jq.control_sample_times(p, wa)))
        x = torch.tensor(pcof, dtype=torch.float64, requires_grad=True)
        J = SampledObjective.apply((B @ x).reshape(nt, nf).T, p, wa)
        J.backward()
        assert J.dtype == torch.float64 and J.dim() == 0
        assert reference_pass(J.item(), pr.ref["objfv"]) and reference_pass(x.grad.numpy(), pr.ref["totalgrad"])
        # ... and the risk-neutral objective: infidelity + leak over the nodes, its gradient that of the spline call
        x2 = torch.tensor(pcof, dtype=torch.float64, requires_grad=True)
        Jr = SampledObjective.apply((B @ x2).reshape(nt, nf).T, p, wa, pr.nodes, pr.weights, pr.shift)
        Jr.backward()
        jq.eval_f_g_grad(pcof, p, wa, pr.nodes, pr.weights, True, shift=pr.shift)
        assert reference_pass(Jr.item(), p.last_infidelity + p.last_leak)
        assert p.objFuncType == 1 and p.last_leak_grad.size == 0      # (infid_grad carries the total gradient)
        assert reference_pass(x2.grad.numpy(), p.last_infidelity_grad)
        # without a gradient request no adjoint sweep runs
        with torch.no_grad():
            assert SampledObjective.apply((B @ x).reshape(nt, nf).T, p, wa).item() == J.item()
        assert wa.last_timing()["n_backward_launches"] == 0
        # ten Adam steps on a piecewise-constant parameterisation: 2 Nc x 4 values, each held for a quarter of the time points
        theta = torch.tensor(0.2 * np.random.default_rng(5).standard_normal((nf, 4)), dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([theta], lr=0.02)
        hist = []
        for _ in range(10):
            opt.zero_grad()
            Jk = SampledObjective.apply(theta.repeat_interleave((nt + 3) // 4, dim=1)[:, :nt], p, wa)
            Jk.backward()
            hist.append(Jk.item())
            opt.step()
        hist.append(SampledObjective.apply(theta.detach().repeat_interleave((nt + 3) // 4, dim=1)[:, :nt], p, wa).item())
        print("objective over ten Adam steps:", " ".join("%.6f" % v for v in hist))
        assert hist[-1] < hist[0]
        with pytest.raises(TypeError):
            SampledObjective.apply(torch.zeros(nf, nt, dtype=torch.float32), p, wa)
    finally:
        wa.close()
