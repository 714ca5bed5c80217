"""GPU (-m gpu): sample tables over member ensembles and in batches (jq_traceobjgrad_samples_batch, jq_traceobjgrad_samples_members,
jq_eval_f_g_grad_samples_members; torch_controls.SampledMembersObjective / SampledBatchObjective).

The reference is the CPU oracle on a member's MIXED OPERATORS (mixed_params) at the coefficients whose samples are the table: with
D1 = 2 nsteps + 3 the matrix B = d pq / d pcof has full row rank (tests/test_sampled_controls_host.py), so B' G_g is checked by the
oracle's coefficient gradient without a blind component; tests/test_sampled_members_host.py pins that reference against the oracle on
the mixed TABLE.

One small problem per place the new code can go wrong (CELLS): both grouped kernel families (the cooperative-quad one with the 4 x 4 x n structure and on the dense policy), six sequential routes, chunk boundaries of
both parities, members that differ in their drift, in their mix and in both, one and two gradient passes, more than JQ_MAXNC controls."""
import collections
import copy

import numpy as np
import pytest
from conftest import case_inputs, reference_pass

from block_band_problem import block_band_problem
from subsystem_problem import subsystem_problem
from test_gpu_drift_batch import dense_members, pattern_members
from test_gpu_member_batch import amplitude_mixes, full_mixes, mixed_params
from test_gpu_random import random_problem
from test_gpu_sampled_controls import (COOP, CQ, DENSE_POLICY_BAND, QUAD, ROWLANE, ROWLANE_IMR, SLAB, _band29_jacobi, _swap02_imr, fold,
                                       grad_ok, richardson)
from uncoupled_problem import FD_NEUMANN_TERMS

pytestmark = pytest.mark.gpu
JQ_MAXNC = 4      # controls per backward sweep (include/juqbox_hip.h: more run in control groups)

Cell = collections.namedtuple("Cell", "name build options family mode nsteps chunks kind nmember drifts mixes")
# build(jq, rng, nsteps) -> params; options: of the handle; mode: the route plan_info must report; chunks: option chunk_steps per run (0: one
# chunk); kind: neumann / jacobi / imr; drifts: None | "dense" | "pattern"; mixes: None | "full" | "amplitude"

_rowlane4 = lambda jq, rng, n: random_problem(jq, rng, 4, 3, 2, 1, n, 3, 1, False)[0]
_cq32 = lambda jq, rng, n: subsystem_problem(jq, rng, 2, 32, 4, 3, 3, "varied", n, 1)[0]

CELLS = (
    Cell("rowlane", _rowlane4, {}, ROWLANE, "grouped", 7, (0, 3), "neumann", 3, "dense", "full"),
    Cell("rowlane-two-passes", lambda jq, rng, n: random_problem(jq, rng, 4, 3, 2, 1, n, 3, 2, False)[0], {}, ROWLANE, "grouped", 2, (1,), "neumann", 3,
         None, "amplitude"),
    Cell("cq-Ntot32", _cq32, {}, CQ, "grouped", 7, (0, 3), "neumann", 3, "pattern", "full"),
    # (three columns per sample straddle the column quads of the dense policy: the spline batch's column-count rule sends N = 3 down the
    #  sequential route, N = 4 shares launches)
    Cell("cq-dense-Ntot29", lambda jq, rng, n: random_problem(jq, rng, 29, 3, 2, 1, n, 3, 3, False)[0], {}, CQ, "sequential", 8, (3,), "neumann", 2, "dense", None),
    Cell("cq-dense-Ntot29-N4", lambda jq, rng, n: random_problem(jq, rng, 29, 4, 2, 1, n, 3, 3, False)[0], {}, CQ, "grouped", 8, (3,), "neumann", 2, "dense", None),
    Cell("quad-Ntot32", _cq32, {"cq": 0}, QUAD, "sequential", 1, (0,), "neumann", 2, "pattern", "full"),
    Cell("coop-Ntot29-five-controls", lambda jq, rng, n: block_band_problem(jq, rng, 29, 3, 1, [1, 0, 2, 1, 1], n, 3, 3)[0], {"cq": 0, "dq": 0}, COOP,
         "sequential", 2, (0,), "neumann", 2, None, "full"),
    Cell("slab-Ntot29-jacobi", _band29_jacobi, {"cq": 0, "dq": 0, "coop_max": 0}, SLAB, "sequential", 8, (3,), "jacobi", 2, "pattern", "full"),
    Cell("rowlane-imr", _swap02_imr, {}, ROWLANE_IMR, "sequential", 7, (0,), "imr", 2, "pattern", "amplitude"),
    Cell("rowlane-sequential-by-option", _rowlane4, {"pcof_batch_max": 0}, ROWLANE, "sequential", 7, (0,), "neumann", 3, "dense", "full"),
)
BY_NAME = {c.name: c for c in CELLS}


def test_the_cells_cover_what_the_feature_touches(jq):
    grouped = [c for c in CELLS if c.mode == "grouped"]
    assert {c.family for c in grouped} == {ROWLANE, CQ} and any(c.name.startswith("cq-dense") for c in grouped)
    assert len({c.family for c in CELLS if c.mode == "sequential"}) >= 4
    # chunk boundaries at even and at odd steps (a boundary after step n is shared by the launches of two chunks), and none
    assert {(c.nsteps, ch) for c in CELLS for ch in c.chunks} >= {(7, 0), (7, 3), (8, 3), (2, 1)}
    assert {(c.drifts is not None, c.mixes is not None) for c in CELLS} == {(True, False), (False, True), (True, True)}
    types = {problem(jq, c).p.objFuncType for c in CELLS}
    assert 1 in types and types & {2, 3}
    assert any(problem(jq, c).p.Ncoupled > JQ_MAXNC for c in CELLS)
    assert {c.kind for c in CELLS} == {"neumann", "jacobi", "imr"}


Problem = collections.namedtuple("Problem", "p pcof H C w ref")
_problems = {}


def make_members(jq, cell, p, n, seed):
    H = {None: None, "dense": dense_members, "pattern": pattern_members}[cell.drifts]
    H = H(p.Hconst, n, seed) if H else None
    if cell.mixes == "full":
        C = full_mixes(p.Ncoupled, n, seed + 1)
    elif cell.mixes == "amplitude":
        C = amplitude_mixes(jq, p.Ncoupled, n, seed + 1)
    else:
        C = None
    return H, C


def oracle_member(cell, p, pcof, H, C):
    """the ORACLE on the plain problem a member is, at the coefficients whose samples are the shared table"""
    from oracle.oracle import Oracle
    o = Oracle(mixed_params(p, C if C is not None else np.eye(p.Ncoupled), H), use_sparse=False)
    return o.traceobjgrad_imr(pcof, 60, 1e-11) if cell.kind == "imr" else o.traceobjgrad(pcof)


def problem(jq, cell):
    """the problem of a cell with a coefficient vector of D1 = 2 nsteps + 3, its members with their weights and the ORACLE's result per
    member, computed once"""
    if cell.name not in _problems:
        rng = np.random.default_rng(88000 + 17 * CELLS.index(cell))
        p = cell.build(jq, rng, cell.nsteps)
        assert p.nsteps == cell.nsteps
        D1 = 2 * cell.nsteps + 3
        pcof = 0.3 * rng.standard_normal(2 * p.Ncoupled * p.Nfreq * D1)
        if "imr" in cell.name:
            pcof *= 0.05      # (swap02's controls are bounded by maxpar = 0.02)
        H, C = make_members(jq, cell, p, cell.nmember, 5100 + CELLS.index(cell))
        w = 0.2 + rng.random(cell.nmember)
        ref = [oracle_member(cell, p, pcof, H[g] if H else None, C[g] if C else None) for g in range(cell.nmember)]
        _problems[cell.name] = Problem(p, pcof, H, C, w, ref)
    return _problems[cell.name]


def handle(jq, cell, p, ncoeff, chunk, **more):
    opts = dict(cell.options)
    opts.update(more)
    if chunk:
        opts["chunk_steps"] = chunk
    WA = jq.Working_Arrays_M_HIP if cell.kind == "imr" else jq.Working_Arrays_HIP
    return WA(p, ncoeff, options=opts)


SNAMES = ("objfv", "totalgrad", "primaryobjf", "secondaryobjf", "traceInfidelity", "infidelgrad", "leakgrad")
RECORD = ("objfv", "primaryobjf", "secondaryobjf", "traceInfidelity")


def smembers(jq, pq, p, wa, H, C):
    return dict(zip(SNAMES, jq.traceobjgrad_samples_members(pq, p, wa, Hconsts=H, ctrl_mix=C, evaladjoint=True)))


def member(b, g):
    return {k: b[k][g] if np.size(b[k]) else np.zeros((0, 0)) for k in SNAMES}      # (objFuncType 1: the empty leak gradient of the single call)


def same_bits(tag, a, b, names=SNAMES):
    for k in names:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (tag, k)


def check_route(cell, wa, kind, per_launch=None):
    t = wa.last_timing()
    assert t["kernel_family"] == cell.family, (cell.name, t["kernel_family"], t["kernel_band"])
    if cell.name.startswith("cq-dense"):
        assert t["kernel_band"] == DENSE_POLICY_BAND, t
    info = wa.plan_info()["sampled_batch"]
    assert info["kind"] == kind and info["mode"] == cell.mode, (cell.name, info)
    assert info["family"] == cell.family and info["time_points"] == 2 * cell.nsteps + 1 and len(info["why"]) > 0, info
    if kind == "members":
        assert info["drifts"] == (cell.drifts is not None) and info["mixes"] == (cell.mixes is not None), info
    if cell.mode == "sequential":
        assert info["per_launch"] == 1
    elif per_launch:
        assert info["per_launch"] == per_launch, info
    return info


def weighted(b, w, p):
    """sum_g w_g of the per-member outputs, in member order"""
    out = dict(infidelity=0.0, leak=0.0, infid_grad=0.0, leak_grad=0.0)
    for g in range(len(w)):
        out["infidelity"] += w[g] * b["primaryobjf"][g]
        out["leak"] += w[g] * b["secondaryobjf"][g]
        out["infid_grad"] = out["infid_grad"] + w[g] * b["infidelgrad"][g]
        if p.objFuncType != 1:
            out["leak_grad"] = out["leak_grad"] + w[g] * b["leakgrad"][g]
    if p.objFuncType == 1:
        out["leak_grad"] = np.zeros_like(out["infid_grad"])
    return out


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_members_against_the_oracle_the_spline_call_and_the_ensemble(jq, cell):
    pr = problem(jq, cell)
    p, pcof, H, C, w = pr.p, pr.pcof, pr.H, pr.C, pr.w
    n, nt = cell.nmember, 2 * cell.nsteps + 1
    for chunk in cell.chunks:
        wa = handle(jq, cell, p, pcof.size, chunk)
        try:
            B = jq.spline_sample_matrix(p, pcof.size, jq.control_sample_times(p, wa))
            pq = jq.control_samples(pcof, p, wa)
            b = smembers(jq, pq, p, wa, H, C)
            info = check_route(cell, wa, "members", n if cell.mode == "grouped" else None)
            if chunk:
                assert info["chunk_steps"] == chunk
            assert wa.plan_info()["sampled_controls"]["time_points"] == nt
            again = smembers(jq, pq, p, wa, H, C)
            fwd = jq.traceobjgrad_samples_members(pq, p, wa, Hconsts=H, ctrl_mix=C, evaladjoint=False)
            spline = jq.traceobjgrad_members(pcof, p, wa, Hconsts=H, ctrl_mix=C, evaladjoint=True)
            ens = jq.eval_f_g_grad_samples_members(pq, p, wa, w, Hconsts=H, ctrl_mix=C, per_member=True)
            check_route(cell, wa, "members")
            ens_again = jq.eval_f_g_grad_samples_members(pq, p, wa, w, Hconsts=H, ctrl_mix=C, per_member=True)
            ens_fwd = jq.eval_f_g_grad_samples_members(pq, p, wa, w, Hconsts=H, ctrl_mix=C, compute_adjoint=False)
        finally:
            wa.close()
        assert b["totalgrad"].shape == b["infidelgrad"].shape == (n, 2 * p.Ncoupled, nt)
        # 4. deterministic; the forward-only call returns the same records
        same_bits("repeat", b, again)
        assert all(np.array_equal(x, b[k]) for x, k in zip(fwd, ("objfv", "primaryobjf", "secondaryobjf")))
        for k in ("infidelity", "leak", "infid_grad", "leak_grad", "members"):
            assert np.array_equal(ens[k], ens_again[k]), k
        assert (ens_fwd["infidelity"], ens_fwd["leak"]) == (ens["infidelity"], ens["leak"]) and "infid_grad" not in ens_fwd
        sp = dict(zip(SNAMES, spline))
        for g in range(n):
            m, ref = member(b, g), pr.ref[g]
            scale = np.linalg.norm(ref["totalgrad"])
            # 1. against the ORACLE: the record, and B' G_g against its coefficient gradients
            for k in RECORD:
                assert reference_pass(m[k], ref[k]), (cell.name, chunk, g, k, m[k], ref[k])
            got = {"totalgrad": fold(B, m["totalgrad"]), "infidelgrad": fold(B, m["infidelgrad"])}
            if p.objFuncType != 1:
                got["leakgrad"] = fold(B, m["leakgrad"])
                assert np.array_equal(m["leakgrad"], m["totalgrad"] - m["infidelgrad"])
            else:
                assert np.size(b["leakgrad"]) == 0 and np.array_equal(m["totalgrad"], m["infidelgrad"])
            for name, v in got.items():
                d = np.linalg.norm(v - ref[name]) / max(np.linalg.norm(ref[name]), 1e-300)
                print("%s chunk %d member %d %s: |B'G - oracle| / |oracle| = %.2e (|oracle| %.3e)" % (cell.name, chunk, g, name, d, np.linalg.norm(ref[name])))
            for name, v in got.items():
                if cell.kind == "imr" and name == "leakgrad":
                    continue
                assert grad_ok(cell, v, ref[name], scale), (cell.name, chunk, g, name)
            # 2. against the spline call on the same members: the record, bit for bit where the table's bits are k_ctrl's
            rec_s = {k: sp[k][g] for k in RECORD}
            if cell.mixes is None:
                same_bits("record of the spline call, member %d" % g, m, rec_s, RECORD)
            else:
                print("%s chunk %d member %d record: samples %r, splines %r" % (cell.name, chunk, g, [float(m[k]).hex() for k in RECORD],
                                                                               [float(rec_s[k]).hex() for k in RECORD]))
                for k in RECORD:
                    assert reference_pass(m[k], rec_s[k]), (cell.name, chunk, g, k)
            # 3. the members' records of the ensemble call are those bits
            assert np.array_equal(ens["members"][:, g], [m[k] for k in RECORD])
        # 3. the ensemble against the weighted sums of the per-member outputs
        ws = weighted(b, w, p)
        for k in ("infidelity", "leak", "infid_grad", "leak_grad"):
            if k == "leak_grad" and p.objFuncType == 1:
                assert np.all(ens[k] == 0.0)
                continue
            d = np.linalg.norm(np.atleast_1d(ens[k] - ws[k])) / max(np.linalg.norm(np.atleast_1d(ws[k])), 1e-300)
            print("%s chunk %d ensemble %s: relative difference to the host sum %.2e" % (cell.name, chunk, k, d))
            assert reference_pass(ens[k], ws[k]), (cell.name, chunk, k)
        assert ens["infid_grad"].shape == (2 * p.Ncoupled, nt)


# ---- once, on the first row-lane cell --------------------------------------------------------------------------------------------------
def rowlane(jq):
    cell = CELLS[0]
    return cell, problem(jq, cell)


@pytest.mark.parametrize("chunk", [0, 3])
def test_identity_members_are_the_single_call_bit_for_bit(jq, chunk):
    cell, pr = rowlane(jq)
    p, pcof = pr.p, pr.pcof
    wa = handle(jq, cell, p, pcof.size, chunk)
    try:
        pq = jq.control_samples(pcof, p, wa)
        one = dict(zip(SNAMES, jq.traceobjgrad_samples(pq, p, wa, True)))
        b = smembers(jq, pq, p, wa, None, [np.eye(p.Ncoupled)] * 3)
        assert check_route(cell._replace(drifts=None), wa, "members", 3)["chunk_steps"] == wa.plan_info()["sampled_controls"]["chunk_steps"]
        if chunk:
            assert wa.plan_info()["sampled_controls"]["chunk_steps"] == chunk
    finally:
        wa.close()
    for g in range(3):
        same_bits("identity member %d" % g, member(b, g), one)


def test_a_zero_column_of_the_mix_gives_exactly_zero_gradient_rows(jq):
    cell, pr = rowlane(jq)
    p, pcof = pr.p, pr.pcof
    C = [c.copy() for c in pr.C]
    C[1][:, 1] = 0.0
    wa = handle(jq, cell, p, pcof.size, 3)
    try:
        b = smembers(jq, jq.control_samples(pcof, p, wa), p, wa, pr.H, C)
    finally:
        wa.close()
    for k in ("totalgrad", "infidelgrad"):
        assert np.all(b[k][1][2:4, :] == 0.0) and np.all(np.any(b[k][1][0:2, :] != 0.0, axis=0))
        assert np.all(np.any(b[k][0][2:4, :] != 0.0, axis=0))      # (the other members' rows are not)


def test_members_do_not_talk_to_each_other(jq):
    cell, pr = rowlane(jq)
    p, pcof = pr.p, pr.pcof
    perm = [2, 0, 1]
    wa = handle(jq, cell, p, pcof.size, 3)
    try:
        pq = jq.control_samples(pcof, p, wa)
        b = smembers(jq, pq, p, wa, pr.H, pr.C)
        bp = smembers(jq, pq, p, wa, [pr.H[i] for i in perm], [pr.C[i] for i in perm])
    finally:
        wa.close()
    for g, i in enumerate(perm):
        same_bits("permuted member %d" % g, member(bp, g), member(b, i))


def test_rounds_of_two_equal_one_launch(jq):
    """five members in rounds 2 + 2 + 1 and in one launch, at a chunk length that puts boundaries inside the time loop: the per-member
    outputs and the ensemble gradient -- summed on the device in member order from whole member gradients -- are the same bits"""
    cell, pr = rowlane(jq)
    p, pcof = pr.p, pr.pcof
    H, C = make_members(jq, cell, p, 5, 6200)
    w = 0.2 + np.random.default_rng(6201).random(5)
    out = []
    for more, per in (({"pcof_batch_max": 2}, 2), ({}, 5)):
        wa = handle(jq, cell, p, pcof.size, 3, **more)
        try:
            pq = jq.control_samples(pcof, p, wa)
            b = smembers(jq, pq, p, wa, H, C)
            assert check_route(cell, wa, "members", per)["chunk_steps"] == 3
            e = jq.eval_f_g_grad_samples_members(pq, p, wa, w, Hconsts=H, ctrl_mix=C, per_member=True)
            assert check_route(cell, wa, "members", per)["chunk_steps"] == 3
            out.append((b, e))
        finally:
            wa.close()
    same_bits("rounds", out[0][0], out[1][0])
    for k in ("infidelity", "leak", "infid_grad", "leak_grad", "members"):
        assert np.array_equal(out[0][1][k], out[1][1][k]), k


def test_the_grouped_and_the_sequential_route_agree(jq):
    cell, pr = rowlane(jq)
    seq = BY_NAME["rowlane-sequential-by-option"]
    p, pcof = pr.p, pr.pcof
    out = []
    for c in (cell, seq):
        wa = handle(jq, c, p, pcof.size, 0)
        try:
            pq = jq.control_samples(pcof, p, wa)
            b = smembers(jq, pq, p, wa, pr.H, pr.C)
            check_route(c, wa, "members")
            out.append((b, jq.eval_f_g_grad_samples_members(pq, p, wa, pr.w, Hconsts=pr.H, ctrl_mix=pr.C)))
        finally:
            wa.close()
    for k in SNAMES:
        if np.size(out[0][0][k]):
            assert reference_pass(out[0][0][k], out[1][0][k]), k
    for k in ("infidelity", "leak", "infid_grad"):
        assert reference_pass(out[0][1][k], out[1][1][k]), k


def test_index_maps_under_a_mix_with_an_asymmetric_piecewise_constant_pulse(jq):
    """The pulse and the Richardson differences of test_index_maps_with_an_asymmetric_piecewise_constant_pulse
    (tests/test_gpu_sampled_controls.py), applied to the weighted ensemble objective of three members with full mixes and dense drifts,
    which the ORACLE evaluates on each member's mixed operators at x = pinv(B) pq.  Neumann order FD_NEUMANN_TERMS, 7 steps in 3 + 3 + 1;
    (B d)' G_ens must equal the extrapolated difference to that test's 1e-9 relative."""
    from oracle.oracle import Oracle
    cell, pr = rowlane(jq)
    p = copy.copy(pr.p)
    p.linear_solver = jq.lsolver_object(max_iter=FD_NEUMANN_TERMS)
    assert p.linear_solver.max_iter >= 20
    rng = np.random.default_rng(4712)
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
        e = jq.eval_f_g_grad_samples_members(pq, p, wa, pr.w, Hconsts=pr.H, ctrl_mix=pr.C)
        assert check_route(cell, wa, "members", 3)["chunk_steps"] == 3
    finally:
        wa.close()
    assert p.objFuncType == 1      # (infid_grad carries the total gradient, infidelity + leak is the weighted objfv)
    G = e["infid_grad"] + e["leak_grad"]
    B = jq.spline_sample_matrix(p, ncoeff, times)
    x = np.linalg.lstsq(B, pq.ravel(order="F"), rcond=None)[0]
    assert np.abs(B @ x - pq.ravel(order="F")).max() <= 1e-13
    oracles = [Oracle(mixed_params(p, C, H), use_sparse=False) for H, C in zip(pr.H, pr.C)]
    f = lambda v: sum(wg * o.traceobjgrad(v, evaladjoint=False)["objfv"] for wg, o in zip(pr.w, oracles))
    assert abs(f(x) - (e["infidelity"] + e["leak"])) <= 1e-12 * float(np.sum(pr.w))
    picks = [(blk * D1 + k, where) for blk in (0, nf * p.Nfreq - 1) for k, where in ((0, "start"), (D1 // 2, "middle"), (D1 - 1, "end"))]
    for k, where in picks:
        d = np.zeros(ncoeff)
        d[k] = 1.0
        touched = np.unique(np.nonzero((B @ d).reshape((nf, nt), order="F"))[1])
        assert {"start": touched.min() == 0, "end": touched.max() == nt - 1, "middle": 0 < touched.min() and touched.max() < nt - 1}[where]
        gd = fold(B, G) @ d
        fd = richardson(f, x, d, 2e-2)
        print("coefficient %d (%s, time points %s): (B d)' G_ens = %.12e, Richardson %.12e, relative difference %.2e"
              % (k, where, touched.tolist(), gd, fd, abs(fd - gd) / abs(gd)))
        assert abs(fd - gd) <= 1e-9 * abs(gd)


def four_tables(jq, p, pcof, wa, seed):
    """the handle's splines and three random piecewise-constant tables"""
    rng = np.random.default_rng(seed)
    nt, nf = 2 * p.nsteps + 1, 2 * p.Ncoupled
    tabs = [jq.control_samples(pcof, p, wa)]
    for _ in range(3):
        t = np.zeros((nf, nt))
        for f in range(nf):
            cuts = np.sort(rng.choice(np.arange(1, nt), size=min(2, nt - 1), replace=False))
            for lo, hi in zip(np.r_[0, cuts], np.r_[cuts, nt]):
                t[f, lo:hi] = 0.3 * rng.standard_normal()
        tabs.append(t)
    return tabs


@pytest.mark.parametrize("name,chunk", [("rowlane", 0), ("rowlane", 3), ("quad-Ntot32", 0)])
def test_a_batch_of_tables_is_the_single_call_per_table(jq, name, chunk):
    cell = BY_NAME[name]
    pr = problem(jq, cell)
    p, pcof = pr.p, pr.pcof
    wa = handle(jq, cell, p, pcof.size, chunk)
    try:
        tabs = four_tables(jq, p, pcof, wa, 31)
        singles = [dict(zip(SNAMES, jq.traceobjgrad_samples(t, p, wa, True))) for t in tabs]
        cs = wa.plan_info()["sampled_controls"]["chunk_steps"]
        b = dict(zip(SNAMES, jq.traceobjgrad_samples_batch(np.stack(tabs), p, wa, True)))
        info = check_route(cell, wa, "tables", 4 if cell.mode == "grouped" else None)
        assert info["chunk_steps"] == cs and info["drifts"] is False and info["mixes"] is False
        fwd = jq.traceobjgrad_samples_batch(tabs, p, wa, False)
        one = dict(zip(SNAMES, jq.traceobjgrad_samples_batch(tabs[2:3], p, wa, True)))
        assert wa.plan_info()["sampled_batch"]["mode"] == "sequential"      # (one table: the single call)
    finally:
        wa.close()
    assert len({s["objfv"] for s in singles}) == 4
    for i in range(4):
        same_bits("table %d" % i, member(b, i), singles[i], SNAMES)      # (record and gradients: the same sweeps, the same assembly)
    assert all(np.array_equal(x, b[k]) for x, k in zip(fwd, ("objfv", "primaryobjf", "secondaryobjf")))
    same_bits("a batch of one", member(one, 0), singles[2])


def test_refusals_write_nothing_and_leave_the_handle_alone(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
    SENT = -7.25

    def refused(before_after, h, calls):
        before = before_after()
        for i, (call, sizes, code) in enumerate(calls):
            outs = [np.full(n, SENT) for n in sizes]
            assert call(*[ptr(a) for a in outs]) == code, (i, L.jq_last_error(h))
            assert all(np.all(a == SENT) for a in outs), i
            assert len(L.jq_last_error(h)) > 0
        after = before_after()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))

    def three(h, tab, tabs2, nt, n, mix, w):
        """(batch of two tables, members, ensemble) with these arguments"""
        sz = tab.size
        return [
            (lambda o4, g0, g1, g2: L.jq_traceobjgrad_samples_batch(h, ptr(tabs2), nt, 2, 1, o4, g0, g1, g2), (8, 2 * sz, 2 * sz, 2 * sz)),
            (lambda o4, g0, g1, g2: L.jq_traceobjgrad_samples_members(h, ptr(tab), nt, None, ptr(mix) if mix is not None else None, n, 1, o4, g0, g1, g2),
             (4 * max(n, 1), max(n, 1) * sz, max(n, 1) * sz, max(n, 1) * sz)),
            (lambda o2, g0, g1, mo: L.jq_eval_f_g_grad_samples_members(h, ptr(tab), nt, None, ptr(mix) if mix is not None else None, ptr(w), n, 1, o2, g0, g1, mo),
             (2, sz, sz, 4 * max(n, 1))),
        ]

    # an uncoupled-controls handle
    p, info, pcof, _ = case_inputs("cnot2_lab")
    p.T = p.T * 6 / p.nsteps
    p.nsteps = 6
    nt, nf, Nc = 13, 2 * p.Nunc, p.Nunc
    tab, mix, w = np.zeros(nf * nt), np.stack([np.eye(Nc).ravel()] * 2), np.full(2, 0.5)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        h = wa.handle
        refused(lambda: jq.traceobjgrad(pcof, p, wa, False, True), h,
                [(c, s, _lib.JQ_EUNSUPPORTED) for c, s in three(h, tab, np.zeros(2 * tab.size), nt, 2, mix, w)])
    finally:
        wa.close()
    cell, pr = rowlane(jq)
    p, pcof = pr.p, pr.pcof
    nt, nf, Nc = 2 * p.nsteps + 1, 2 * p.Ncoupled, p.Ncoupled
    wa = handle(jq, cell, p, pcof.size, 0)
    try:
        h = wa.handle
        pq = jq.control_samples(pcof, p, wa)
        good = np.ascontiguousarray(pq.ravel(order="F"))
        two = np.concatenate([good, 0.5 * good])
        nan2 = two.copy()
        nan2[good.size + nf * 4 + 1] = np.nan      # (a sample of the SECOND table)
        nan1 = good.copy()
        nan1[3] = np.nan
        mix = np.stack([np.eye(Nc).ravel()] * 2)
        nanmix = mix.copy()
        nanmix[1, 2] = np.nan
        w = np.full(2, 0.5)
        calls = []
        for nt_ in (nt - 1, nt + 1):      # nt off by one
            calls += [(c, s, _lib.JQ_EINVAL) for c, s in three(h, good, two, nt_, 2, mix, w)]
        calls.append(three(h, good, nan2, nt, 2, mix, w)[0] + (_lib.JQ_EINVAL,))      # a NaN sample in the second table
        calls += [(c, s, _lib.JQ_EINVAL) for c, s in three(h, nan1, two, nt, 2, mix, w)[1:]]
        calls += [(c, s, _lib.JQ_EINVAL) for c, s in three(h, good, two, nt, 2, nanmix, w)[1:]]      # a NaN mix entry
        calls += [(c, s, _lib.JQ_EINVAL) for c, s in three(h, good, two, nt, 2, None, w)[1:]]      # both member arrays NULL
        calls += [(c, s, _lib.JQ_EINVAL) for c, s in three(h, good, two, nt, 0, mix, w)[1:]]      # nmember = 0
        sz = good.size
        calls.append((lambda o4, g0, g1, g2: L.jq_traceobjgrad_samples_batch(h, ptr(two), nt, 0, 1, o4, g0, g1, g2), (4, sz, sz, sz), _lib.JQ_EINVAL))      # ntab = 0
        calls.append((lambda o4: L.jq_traceobjgrad_samples_batch(h, ptr(two), nt, 2, 1, o4, None, None, None), (8,), _lib.JQ_EINVAL))
        calls.append((lambda o2: L.jq_eval_f_g_grad_samples_members(h, ptr(good), nt, None, ptr(mix), None, 2, 0, o2, None, None, None), (2,), _lib.JQ_EINVAL))
        refused(lambda: jq.traceobjgrad_samples(pq, p, wa, True), h, calls)
    finally:
        wa.close()


def test_multi_device_handle_runs_on_its_first_device(jq):
    cell, pr = rowlane(jq)
    p, pcof = pr.p, pr.pcof
    w1 = handle(jq, cell, p, pcof.size, 3)
    wm = jq.Working_Arrays_HIP(p, pcof.size, devices=2, options={"chunk_steps": 3, "multi_same_device": 1})
    try:
        pq = jq.control_samples(pcof, p, w1)
        tabs = four_tables(jq, p, pcof, w1, 32)
        out = [(smembers(jq, pq, p, wa, pr.H, pr.C), jq.eval_f_g_grad_samples_members(pq, p, wa, pr.w, Hconsts=pr.H, ctrl_mix=pr.C, per_member=True),
                dict(zip(SNAMES, jq.traceobjgrad_samples_batch(tabs, p, wa, True)))) for wa in (w1, wm)]
        assert wm.plan_info()["devices"] == 2 and wm.plan_info()["sampled_batch"]["kind"] == "tables"
    finally:
        w1.close()
        wm.close()
    same_bits("members", out[1][0], out[0][0])
    for k in ("infidelity", "leak", "infid_grad", "leak_grad", "members"):
        assert np.array_equal(out[1][1][k], out[0][1][k]), k
    same_bits("tables", out[1][2], out[0][2])


def test_autograd_over_members_and_over_a_batch_of_tables(jq):
    import torch
    from juqbox_jl_amd.torch_controls import SampledBatchObjective, SampledMembersObjective
    cell, pr = rowlane(jq)
    p, pcof = pr.p, pr.pcof
    nt, nf = 2 * p.nsteps + 1, 2 * p.Ncoupled
    H, C = np.stack(pr.H, axis=2), np.stack(pr.C, axis=2)
    wa = handle(jq, cell, p, pcof.size, 0)
    try:
        # a piecewise-constant pulse: 2 Nc x 4 values, each held for a quarter of the time points
        seg = (nt + 3) // 4
        theta = torch.tensor(0.2 * np.random.default_rng(6).standard_normal((nf, 4)), dtype=torch.float64, requires_grad=True)
        J = SampledMembersObjective.apply(theta.repeat_interleave(seg, dim=1)[:, :nt], p, wa, pr.w, H, C)
        J.backward()
        assert J.dtype == torch.float64 and J.dim() == 0
        table = theta.detach().numpy().repeat(seg, axis=1)[:, :nt]
        e = jq.eval_f_g_grad_samples_members(table, p, wa, pr.w, Hconsts=H, ctrl_mix=C)
        assert J.item() == e["infidelity"] + e["leak"]
        G = e["infid_grad"] + e["leak_grad"]
        chain = np.stack([G[:, s * seg:min((s + 1) * seg, nt)].sum(axis=1) for s in range(4)], axis=1)
        assert reference_pass(theta.grad.numpy(), chain)
        with torch.no_grad():
            assert SampledMembersObjective.apply(torch.from_numpy(table), p, wa, pr.w, H, C).item() == J.item()
        assert wa.last_timing()["n_backward_launches"] == 0
        # a batch of tables with a random grad_output
        pqs = torch.tensor(np.stack(four_tables(jq, p, pcof, wa, 33)), dtype=torch.float64, requires_grad=True)
        out = SampledBatchObjective.apply(pqs, p, wa)
        go = torch.tensor(np.random.default_rng(7).standard_normal(4), dtype=torch.float64)
        out.backward(go)
        b = jq.traceobjgrad_samples_batch(pqs.detach().numpy(), p, wa, True)
        assert out.shape == (4,) and np.array_equal(out.detach().numpy(), b[0])
        assert np.array_equal(pqs.grad.numpy(), go.numpy()[:, None, None] * b[1])
        with pytest.raises(TypeError):
            SampledBatchObjective.apply(torch.zeros(4, nf, nt, dtype=torch.float32), p, wa)
    finally:
        wa.close()
