"""GPU (-m gpu): jq_traceobjgrad_hvp -- the tangent of the adjoint sweep (k_forward_tl, k_terminal_hvp, k_backward_tl) against the CPU
reference of tests/hessian_reference.py (three runs of the unchanged oracle on the 2 Ntot problem with 3 Nc controls).

Random dense problems from the generator of the block-band tests, 7 time steps, at the sizes where a run-time-size dense-tile kernel
can go wrong: one partly filled tile row (Ntot 3), one full tile row (16), a second tile row with one live row (17), six tile rows with
padding (93), two slabs per direction (N = 17), 17 tile rows so that a wave owns two (260).  Over them: Neumann order 0 / 1 / 4, one /
two / five controls (five: two control groups), one chunk and chunks of 3 + 3 + 1 (the carries and their tangents cross chunk
boundaries), 1 and 5 directions (e_k, g/|g|, random), objFuncType 1 / 2 / 3.  Criterion: the project's reference_pass (atol 1e-14 or
rtol 1e-10) for every hv[:, j] and hv_infid[:, j]; the primal record against jq_traceobjgrad, totalgrad against the oracle; a
direction of a 5-direction call, and directions in rounds, bit-identical to the direction alone / to one launch; jq_traceobj_jvp on
the same handle the same bits before and after."""
import collections
import copy

import numpy as np
import pytest
from conftest import case_inputs, reference_pass

import block_band_matrix as M
import hessian_reference as HR
from block_band_problem import block_band_problem, tile_rows

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "Ntot N Nc m chunk ndir objFuncType")
NSTEPS = 7
CASES = (
    Case(3, 2, 1, 4, 0, 5, 1),        # one partly filled tile row, 15 idle waves
    Case(3, 2, 2, 0, 3, 1, 3),
    Case(16, 4, 2, 1, 3, 5, 3),       # one full tile row
    Case(17, 3, 5, 0, 0, 5, 1),       # second tile row with one live row; five controls = two control groups, no Neumann terms
    Case(17, 3, 5, 1, 3, 1, 3),       # ... control groups, chunks and the unforced pass together
    Case(17, 3, 1, 1, 3, 1, 2),
    Case(17, 3, 2, 4, 0, 5, 3),
    Case(93, 3, 2, 4, 3, 5, 3),       # six tile rows, padding
    Case(93, 3, 1, 1, 0, 1, 1),
    Case(29, 17, 2, 4, 3, 5, 3),      # two slabs per direction
    Case(29, 17, 1, 0, 0, 1, 1),
    Case(260, 2, 1, 4, 3, 1, 3),      # 17 tile rows: a wave owns two (the one slow reference: 520 levels)
)


def _id(c):
    return "Ntot%d-N%d-Nc%d-m%d-%s-ndir%d-type%d" % (c.Ntot, c.N, c.Nc, c.m, "chunks331" if c.chunk else "onechunk", c.ndir, c.objFuncType)


def _problem(jq, c):
    rng = np.random.default_rng(52000 + 1000 * c.Ntot + 100 * c.N + 10 * c.Nc + c.m)
    NT = tile_rows(c.Ntot)
    modes = ([1, 0, 2, 1, 1] if NT >= 2 else [1] * 5)[:c.Nc]
    p, pcof = block_band_problem(jq, rng, c.Ntot, c.N, NT - 1, modes, NSTEPS, c.m, c.objFuncType)
    return p, pcof, rng


def _directions(rng, g, ncoeff, ndir):
    """ndir 5: e_k, g/|g|, three random directions; ndir 1: one random direction"""
    rnd = [rng.standard_normal(ncoeff) for _ in range(3)]
    if ndir == 1:
        return np.stack([rnd[0]], axis=1)
    e = np.zeros(ncoeff)
    e[int(rng.integers(ncoeff))] = 1.0
    return np.stack([e, g / np.linalg.norm(g)] + rnd, axis=1)


def _check_against_reference(r, refs, two):
    for j, t in enumerate(refs):
        assert reference_pass(r["hv"][:, j], t["hv"]), ("hv", j, np.linalg.norm(r["hv"][:, j] - t["hv"]) / np.linalg.norm(t["hv"]))
        if two:
            assert reference_pass(r["hv_infid"][:, j], t["hv_infid"]), ("hv_infid", j, np.linalg.norm(r["hv_infid"][:, j] - t["hv_infid"]) / np.linalg.norm(t["hv_infid"]))
            assert np.array_equal(r["hv_leak"][:, j], r["hv"][:, j] - r["hv_infid"][:, j])
    if not two:
        assert "hv_infid" not in r and "hv_leak" not in r


def _check_primal(jq, r, pcof, p, wa, oracle_grad):
    objfv, prim, sec = jq.traceobjgrad(pcof, p, wa, False, False)
    for name, v, w in (("objfv", r["objfv"], objfv), ("primaryobjf", r["primaryobjf"], prim), ("secondaryobjf", r["secondaryobjf"], sec)):
        assert reference_pass(v, w), (name, v, w)
    assert reference_pass(r["totalgrad"], oracle_grad), np.linalg.norm(r["totalgrad"] - oracle_grad) / np.linalg.norm(oracle_grad)


SAME_BITS = ("objfv", "primaryobjf", "secondaryobjf", "totalgrad")


@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_hvp_matches_reference(jq, c):
    from oracle.oracle import Oracle
    p, pcof, rng = _problem(jq, c)
    g = Oracle(p).traceobjgrad(pcof)["totalgrad"]
    D = _directions(rng, g, pcof.size, c.ndir)
    ref = HR.HessianReference(p)
    refs = [ref.hvp(pcof, D[:, j]) for j in range(c.ndir)]
    two = c.objFuncType != 1
    wa = jq.Working_Arrays_HIP(p, pcof.size, options={"chunk_steps": c.chunk} if c.chunk else None)
    try:
        r = jq.traceobjgrad_hvp(pcof, D, p, wa)
        assert r["hv"].shape == (pcof.size, c.ndir)
        assert wa.plan_info()["hvp"] == {"directions_per_launch": c.ndir, "chunk_steps": c.chunk or NSTEPS, "rounds": 1}
        t = wa.last_timing()
        nchunks, nsweeps = (3 if c.chunk else 1), (2 if two else 1) * (2 if c.Nc > 4 else 1)
        assert (t["kernel_family"], t["kernel_size"], t["kernel_band"]) == (1, tile_rows(c.Ntot), 15)
        assert t["n_forward_launches"] == nchunks and t["n_backward_launches"] == nchunks * nsweeps
        assert t["mfma_executed"] > t["mfma_backward"] > 0
        _check_against_reference(r, refs, two)
        _check_primal(jq, r, pcof, p, wa, g)
        if c.ndir > 1:
            for j in (1, c.ndir - 1):      # a direction alone: the same operations in the same order
                one = jq.traceobjgrad_hvp(pcof, D[:, j], p, wa)
                assert wa.plan_info()["hvp"]["directions_per_launch"] == 1
                assert np.array_equal(one["hv"][:, 0], r["hv"][:, j]), j
                if two:
                    assert np.array_equal(one["hv_infid"][:, 0], r["hv_infid"][:, j]), j
                for k in SAME_BITS:
                    assert np.array_equal(one[k], r[k]), k
    finally:
        wa.close()


def test_directions_in_rounds_and_the_jvp_around_the_call_are_the_same_bits(jq):
    """a stream budget that holds the primal stream and two directions: five directions run in three rounds, bit-identical to one
    launch; jq_traceobj_jvp on the same handle returns the same bits before and after the calls"""
    c = Case(17, 3, 2, 4, 0, 5, 3)
    from oracle.oracle import Oracle
    p, pcof, rng = _problem(jq, c)
    D = _directions(rng, Oracle(p).traceobjgrad(pcof)["totalgrad"], pcof.size, 5)
    stride = 2 * 8 * 64      # doubles of a dense operator image at two tile rows
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    wb = jq.Working_Arrays_HIP(p, pcof.size, options={"stream_bytes": 8 * 3 * 2 * stride * (2 * NSTEPS + 1)})
    try:
        jvp0 = [jq.traceobj_jvp(pcof, D, p, w) for w in (wa, wb)]
        a, b = jq.traceobjgrad_hvp(pcof, D, p, wa), jq.traceobjgrad_hvp(pcof, D, p, wb)
        assert wa.plan_info()["hvp"] == {"directions_per_launch": 5, "chunk_steps": NSTEPS, "rounds": 1}
        assert wb.plan_info()["hvp"] == {"directions_per_launch": 2, "chunk_steps": NSTEPS, "rounds": 3}
        t = wb.last_timing()      # the launch timer over rounds: one chunk, three rounds, two sweeps (objFuncType 3: forced and unforced)
        nchunks, rounds, nsweeps = 1, 3, 2
        assert t["n_forward_launches"] == nchunks * rounds and t["n_backward_launches"] == nchunks * rounds * nsweeps
        assert t["ms_generate"] >= 0 and t["ms_total"] >= t["ms_propagate"]
        for k in SAME_BITS + ("hv", "hv_infid", "hv_leak"):
            assert np.array_equal(a[k], b[k]), k
        jvp1 = [jq.traceobj_jvp(pcof, D, p, w) for w in (wa, wb)]
        for x, y in zip(jvp0, jvp1):
            for k in ("objfv", "d_objfv", "d_primary", "d_secondary", "W"):
                assert np.array_equal(x[k], y[k]), k
    finally:
        wa.close()
        wb.close()


def test_hessian_is_every_unit_direction(jq):
    """hessian(): column j = hv along e_j (the same bits as that direction alone), symmetrize = (J + J')/2"""
    c = Case(3, 2, 1, 4, 0, 1, 1)
    p, pcof, _ = _problem(jq, c)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        J = jq.hessian(pcof, p, wa)
        assert J.shape == (pcof.size, pcof.size)
        e = np.zeros(pcof.size)
        e[3] = 1.0
        assert np.array_equal(J[:, 3], jq.traceobjgrad_hvp(pcof, e, p, wa)["hv"][:, 0])
        assert reference_pass(J[:, 3], HR.hvp(p, pcof, e)["hv"])
        assert np.array_equal(jq.hessian(pcof, p, wa, symmetrize=True), 0.5 * (J + J.T))
    finally:
        wa.close()


def test_full_length_swap02(jq):
    """swap02 at its full length of 7 915 steps along g/|g| and one random direction"""
    p, info, pcof, _ = case_inputs("swap02")
    assert p.nsteps == 7915
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        g = jq.traceobjgrad(pcof, p, wa, False, True)[1]
        rng = np.random.default_rng(2718)
        D = np.stack([g / np.linalg.norm(g), rng.standard_normal(pcof.size)], axis=1)
        ref = HR.HessianReference(p)
        refs = [ref.hvp(pcof, D[:, j]) for j in range(2)]
        r = jq.traceobjgrad_hvp(pcof, D, p, wa)
        for j, t in enumerate(refs):
            print("swap02 direction %d: hv relative %.2e" % (j, np.linalg.norm(r["hv"][:, j] - t["hv"]) / np.linalg.norm(t["hv"])))
        _check_against_reference(r, refs, p.objFuncType != 1)
        assert reference_pass(r["totalgrad"], g)
    finally:
        wa.close()


def _refusal_handles(jq):
    """(name, params, pcof, working-array type) of the five handles the entry point refuses"""
    rng = np.random.default_rng(4242)
    p, pcof = block_band_problem(jq, rng, 17, 3, 1, [1, 1], NSTEPS, 3, 3)
    pw = copy.copy(p)
    A = rng.standard_normal((17, 17))
    pw.wmat_real = np.asfortranarray(A @ A.T / 17.0)
    pw.wmat_imag = np.zeros((17, 17), order="F")
    ps = copy.copy(p)
    Dv = rng.standard_normal((17, 3)) + 1j * rng.standard_normal((17, 3))
    ps.dVds_r, ps.dVds_i, ps.sv_type = np.asfortranarray(Dv.real.copy()), np.asfortranarray(Dv.imag.copy()), 2
    pu, _, pcofu, _ = case_inputs("cnot2_lab")      # uncoupled controls (Hunc_ops), shortened to 20 steps
    pu.T, pu.nsteps = pu.T * 20 / pu.nsteps, 20
    return (("implicit-midpoint", M.with_solver(jq, p, "imr"), pcof, jq.Working_Arrays_M_HIP),
            ("jacobi", M.with_solver(jq, p, "jacobi"), pcof, jq.Working_Arrays_HIP),
            ("full-weights", pw, pcof, jq.Working_Arrays_HIP),
            ("sv_type", ps, pcof, jq.Working_Arrays_HIP),
            ("uncoupled", pu, pcofu, jq.Working_Arrays_HIP))


REFUSALS = ["implicit-midpoint", "jacobi", "full-weights", "sv_type", "uncoupled"]


@pytest.mark.parametrize("which", range(5), ids=REFUSALS)
def test_refusals_write_nothing_and_leave_the_handle_alone(jq, which):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    name, p, pcof, WA = _refusal_handles(jq)[which]
    assert name == REFUSALS[which]
    wa = WA(p, pcof.size)
    try:
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        n = pcof.size
        out4, grad, hv, hvi, d = np.zeros(4), np.zeros(n), np.zeros(n), np.zeros(n), np.ones(n)
        dp = lambda a: a.ctypes.data_as(_lib.c_dp)
        rc = L.jq_traceobjgrad_hvp(wa.handle, dp(np.ascontiguousarray(pcof)), n, dp(d), 1, dp(out4), dp(grad), dp(hv), dp(hvi))
        assert rc == _lib.JQ_EUNSUPPORTED, (name, rc)
        msg = L.jq_last_error(wa.handle).decode()
        assert "jq_traceobjgrad_hvp" in msg and len(msg) > 40
        assert not out4.any() and not grad.any() and not hv.any() and not hvi.any()
        assert "hvp" not in wa.plan_info()
        with pytest.raises(_lib.JuqboxHipError) as e:
            jq.traceobjgrad_hvp(pcof, d, p, wa)
        assert e.value.code == _lib.JQ_EUNSUPPORTED
        after = jq.traceobjgrad(pcof, p, wa, False, True)
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
    finally:
        wa.close()


def test_argument_codes(jq):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    c = CASES[1]
    p, pcof, rng = _problem(jq, c)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        wa.sync_params()
        n = pcof.size
        out4, grad, hv, d = np.zeros(4), np.zeros(n), np.zeros(n), np.ones(n)
        dp = lambda a: a.ctypes.data_as(_lib.c_dp)
        pc = np.ascontiguousarray(pcof)
        f = L.jq_traceobjgrad_hvp
        assert f(wa.handle, None, n, dp(d), 1, dp(out4), dp(grad), dp(hv), None) == _lib.JQ_EINVAL
        assert f(wa.handle, dp(pc), n, None, 1, dp(out4), dp(grad), dp(hv), None) == _lib.JQ_EINVAL
        assert f(wa.handle, dp(pc), n, dp(d), 0, dp(out4), dp(grad), dp(hv), None) == _lib.JQ_EINVAL
        assert f(wa.handle, dp(pc), n, dp(d), 1, None, dp(grad), dp(hv), None) == _lib.JQ_EINVAL
        assert f(wa.handle, dp(pc), n, dp(d), 1, dp(out4), None, dp(hv), None) == _lib.JQ_EINVAL
        assert f(wa.handle, dp(pc), n, dp(d), 1, dp(out4), dp(grad), None, None) == _lib.JQ_EINVAL
        assert f(wa.handle, dp(pc), n - 1, dp(d), 1, dp(out4), dp(grad), dp(hv), None) in (_lib.JQ_EINVAL, _lib.JQ_EDIM)
        assert not out4.any() and not grad.any() and not hv.any()
        assert f(wa.handle, dp(pc), n, dp(d), 1, dp(out4), dp(grad), dp(hv), None) == _lib.JQ_OK
        assert out4[0] != 0.0 and grad.any() and hv.any()
    finally:
        wa.close()
