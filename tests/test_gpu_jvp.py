"""GPU (-m gpu): jq_traceobj_jvp -- the tangent-linear Stormer-Verlet sweep (k_forward_tl) against the CPU reference of
tests/tangent_reference.py (the unchanged oracle on the block-triangular 2 Ntot problem).

Random dense problems from the generator of the block-band tests, 7 time steps, at the sizes where a run-time-size dense-tile kernel
can go wrong: one partly filled tile row (Ntot 3), one full tile row (16), a second tile row with one live row (17), six tile rows with
padding (93), 17 tile rows so that a wave owns two (260), two slabs per direction (N = 17).  Over them: Neumann order 0 / 1 / 4, one /
two / five controls, one chunk and chunks of 3 + 3 + 1, 1 and 5 directions (e_k, g/|g|, random), directions in rounds, uncoupled
controls.  Criterion: the project's reference_pass (atol 1e-14 or rtol 1e-10) for the vector of d_primary, the vector of d_secondary and
every final tangent; the primal against jq_traceobjgrad; a direction of a 5-direction call bit-identical to the same direction alone."""
import collections
import copy

import numpy as np
import pytest
from conftest import case_inputs, reference_pass

import block_band_matrix as M
import tangent_reference as TR
from block_band_problem import block_band_problem, tile_rows

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "Ntot N Nc m chunk ndir objFuncType")
NSTEPS = 7
CASES = (
    Case(3, 2, 1, 4, 0, 5, 1),        # one partly filled tile row, 15 idle waves
    Case(3, 2, 2, 0, 3, 1, 3),
    Case(16, 4, 2, 1, 3, 5, 3),       # one full tile row
    Case(17, 3, 5, 0, 0, 5, 1),       # second tile row with one live row; five controls, no Neumann terms
    Case(17, 3, 1, 1, 3, 1, 2),
    Case(17, 3, 2, 4, 0, 5, 3),
    Case(93, 3, 2, 4, 3, 5, 3),       # six tile rows, padding
    Case(93, 3, 1, 1, 0, 1, 1),
    Case(29, 17, 2, 4, 3, 5, 3),      # two slabs per direction
    Case(29, 17, 1, 0, 0, 1, 1),
    Case(260, 2, 1, 4, 3, 1, 3),      # 17 tile rows: a wave owns two (the one slow reference: 520 levels)
)


def _id(c):
    return "Ntot%d-N%d-Nc%d-m%d-%s-ndir%d" % (c.Ntot, c.N, c.Nc, c.m, "chunks331" if c.chunk else "onechunk", c.ndir)


def _problem(jq, c):
    rng = np.random.default_rng(31000 + 1000 * c.Ntot + 100 * c.N + 10 * c.Nc + c.m)
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


def _check_against_reference(r, refs):
    assert reference_pass(r["d_primary"], [t["d_primary"] for t in refs]), (r["d_primary"], [t["d_primary"] for t in refs])
    assert reference_pass(r["d_secondary"], [t["d_secondary"] for t in refs]), (r["d_secondary"], [t["d_secondary"] for t in refs])
    assert np.array_equal(r["d_objfv"], r["d_primary"] + r["d_secondary"])
    for j, t in enumerate(refs):
        W = r["W"][:, :, j]
        assert reference_pass(np.concatenate([W.real.ravel(), W.imag.ravel()]), np.concatenate([t["W"].real.ravel(), t["W"].imag.ravel()])), j


def _check_primal(jq, r, pcof, p, wa):
    objfv, prim, sec = jq.traceobjgrad(pcof, p, wa, False, False)
    for name, v, w in (("objfv", r["objfv"], objfv), ("primaryobjf", r["primaryobjf"], prim), ("secondaryobjf", r["secondaryobjf"], sec)):
        assert reference_pass(v, w), (name, v, w)


@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_tangent_matches_reference(jq, c):
    from oracle.oracle import Oracle
    p, pcof, rng = _problem(jq, c)
    g = Oracle(p).traceobjgrad(pcof)["totalgrad"] if c.ndir > 1 else None
    D = _directions(rng, g, pcof.size, c.ndir)
    ref = TR.TangentReference(p)
    refs = [ref.tangent(pcof, D[:, j]) for j in range(c.ndir)]
    wa = jq.Working_Arrays_HIP(p, pcof.size, options={"chunk_steps": c.chunk} if c.chunk else None)
    try:
        r = jq.traceobj_jvp(pcof, D, p, wa)
        assert wa.plan_info()["jvp"] == {"directions_per_launch": c.ndir, "chunk_steps": c.chunk or NSTEPS, "rounds": 1}
        t = wa.last_timing()
        assert (t["kernel_family"], t["kernel_size"], t["kernel_band"]) == (1, tile_rows(c.Ntot), 15) and t["n_backward_launches"] == 0
        assert t["n_forward_launches"] == (3 if c.chunk else 1) and t["mfma_executed"] > 0
        _check_against_reference(r, refs)
        _check_primal(jq, r, pcof, p, wa)
        if c.ndir > 1:
            for j in (1, c.ndir - 1):      # a direction alone: the same operations in the same order
                one = jq.traceobj_jvp(pcof, D[:, j], p, wa)
                assert wa.plan_info()["jvp"]["directions_per_launch"] == 1
                for k in ("d_objfv", "d_primary", "d_secondary"):
                    assert np.array_equal(one[k], r[k][j:j + 1]), (j, k)
                assert np.array_equal(one["W"][:, :, 0], r["W"][:, :, j])
                assert one["objfv"] == r["objfv"]
            nofinal = jq.traceobj_jvp(pcof, D, p, wa, final=False)
            assert "W" not in nofinal and np.array_equal(nofinal["d_objfv"], r["d_objfv"])
    finally:
        wa.close()


def test_directions_in_rounds_are_the_same_bits(jq):
    """a stream budget that holds the primal stream and two directions: five directions run in three rounds, bit-identical to one launch"""
    c = Case(17, 3, 2, 4, 0, 5, 3)
    from oracle.oracle import Oracle
    p, pcof, rng = _problem(jq, c)
    D = _directions(rng, Oracle(p).traceobjgrad(pcof)["totalgrad"], pcof.size, 5)
    stride = 2 * 8 * 64      # doubles of a dense operator image at two tile rows
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    wb = jq.Working_Arrays_HIP(p, pcof.size, options={"stream_bytes": 8 * 3 * 2 * stride * (2 * NSTEPS + 1)})
    try:
        a, b = jq.traceobj_jvp(pcof, D, p, wa), jq.traceobj_jvp(pcof, D, p, wb)
        assert wa.plan_info()["jvp"] == {"directions_per_launch": 5, "chunk_steps": NSTEPS, "rounds": 1}
        assert wb.plan_info()["jvp"] == {"directions_per_launch": 2, "chunk_steps": NSTEPS, "rounds": 3}
        for k in ("objfv", "d_objfv", "d_primary", "d_secondary", "W"):
            assert np.array_equal(a[k], b[k]), k
    finally:
        wa.close()
        wb.close()


def test_uncoupled_controls(jq):
    """cases.cnot2_lab (Hunc_ops, lab frame) shortened to 20 steps: ft is linear in the coefficients too"""
    p, info, pcof, _ = case_inputs("cnot2_lab")
    nfull = p.nsteps
    p.nsteps = 20
    p.T = p.T * 20 / nfull
    rng = np.random.default_rng(99)
    e = np.zeros(pcof.size)
    e[5] = 1.0
    D = np.stack([e, rng.standard_normal(pcof.size)], axis=1)
    ref = TR.TangentReference(p)
    refs = [ref.tangent(pcof, D[:, j]) for j in range(2)]
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        r = jq.traceobj_jvp(pcof, D, p, wa)
        assert wa.plan_info()["jvp"] == {"directions_per_launch": 2, "chunk_steps": 20, "rounds": 1}
        _check_against_reference(r, refs)
        _check_primal(jq, r, pcof, p, wa)
    finally:
        wa.close()


def test_mirrored_call_on_swap02(jq):
    """traceobjgrad(pcof, params, wa, True, True) at full length: the reference's 6-tuple along e_kpar"""
    p, info, pcof, _ = case_inputs("swap02")
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        tg0 = jq.traceobjgrad(pcof, p, wa, False, True)[1]
        objfv0, hist0, fid0 = jq.traceobjgrad(pcof, p, wa, True, False)
        gn = np.linalg.norm(tg0)
        for n, kpar in enumerate((1, 7, pcof.size)):
            p.kpar = kpar
            objfv, tg, hist, fid, dfdp, wfinal = jq.traceobjgrad(pcof, p, wa, True, True)
            assert np.array_equal(tg, tg0) and np.array_equal(hist, hist0) and fid == fid0
            assert wfinal.shape == (p.Ntot, p.N) and np.iscomplexobj(wfinal)
            print("swap02 kpar %d: dfdp %.15e adjoint %.15e, relative to |g| %.2e" % (kpar, dfdp, tg0[kpar - 1], abs(dfdp - tg0[kpar - 1]) / gn))
            assert abs(dfdp - tg0[kpar - 1]) / gn < 1e-10
            if n == 0:
                e = np.zeros(pcof.size)
                e[kpar - 1] = 1.0
                W = TR.tangent(p, pcof, e)["W"]
                assert reference_pass(np.concatenate([wfinal.real.ravel(), wfinal.imag.ravel()]), np.concatenate([W.real.ravel(), W.imag.ravel()]))
    finally:
        wa.close()


def _refusal_handles(jq):
    """(name, params, pcof, working-array type) of the three handles the entry point refuses"""
    rng = np.random.default_rng(4242)
    p, pcof = block_band_problem(jq, rng, 17, 3, 1, [1, 1], NSTEPS, 3, 3)
    pw = copy.copy(p)
    A = rng.standard_normal((17, 17))
    pw.wmat_real = np.asfortranarray(A @ A.T / 17.0)
    pw.wmat_imag = np.zeros((17, 17), order="F")
    return (("implicit-midpoint", M.with_solver(jq, p, "imr"), pcof, jq.Working_Arrays_M_HIP),
            ("jacobi", M.with_solver(jq, p, "jacobi"), pcof, jq.Working_Arrays_HIP),
            ("full-weights", pw, pcof, jq.Working_Arrays_HIP))


@pytest.mark.parametrize("which", [0, 1, 2], ids=["implicit-midpoint", "jacobi", "full-weights"])
def test_refusals_write_nothing_and_leave_the_handle_alone(jq, which):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    name, p, pcof, WA = _refusal_handles(jq)[which]
    wa = WA(p, pcof.size)
    try:
        before = jq.traceobjgrad(pcof, p, wa, False, True)
        out4, dout, d = np.zeros(4), np.zeros(3), np.ones(pcof.size)
        wr, wi = np.zeros(p.Ntot * p.N), np.zeros(p.Ntot * p.N)
        dp = lambda a: a.ctypes.data_as(_lib.c_dp)
        rc = L.jq_traceobj_jvp(wa.handle, dp(np.ascontiguousarray(pcof)), pcof.size, dp(d), 1, dp(out4), dp(dout), dp(wr), dp(wi))
        assert rc == _lib.JQ_EUNSUPPORTED, (name, rc)
        assert len(L.jq_last_error(wa.handle).decode()) > 20
        assert not out4.any() and not dout.any() and not wr.any() and not wi.any()
        assert "jvp" not in wa.plan_info()
        with pytest.raises(_lib.JuqboxHipError) as e:
            jq.traceobj_jvp(pcof, d, p, wa)
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
        out4, dout, d, w = np.zeros(4), np.zeros(3), np.ones(pcof.size), np.zeros(p.Ntot * p.N)
        dp = lambda a: a.ctypes.data_as(_lib.c_dp)
        pc = np.ascontiguousarray(pcof)
        assert L.jq_traceobj_jvp(wa.handle, None, pcof.size, dp(d), 1, dp(out4), dp(dout), None, None) == _lib.JQ_EINVAL
        assert L.jq_traceobj_jvp(wa.handle, dp(pc), pcof.size, None, 1, dp(out4), dp(dout), None, None) == _lib.JQ_EINVAL
        assert L.jq_traceobj_jvp(wa.handle, dp(pc), pcof.size, dp(d), 0, dp(out4), dp(dout), None, None) == _lib.JQ_EINVAL
        assert L.jq_traceobj_jvp(wa.handle, dp(pc), pcof.size, dp(d), 1, dp(out4), dp(dout), dp(w), None) == _lib.JQ_EINVAL
        assert L.jq_traceobj_jvp(wa.handle, dp(pc), pcof.size, dp(d), 1, dp(out4), None, None, None) == _lib.JQ_EINVAL
        assert L.jq_traceobj_jvp(wa.handle, dp(pc), pcof.size - 1, dp(d), 1, dp(out4), dp(dout), None, None) in (_lib.JQ_EINVAL, _lib.JQ_EDIM)
        assert L.jq_traceobj_jvp(wa.handle, dp(pc), pcof.size, dp(d), 1, dp(out4), dp(dout), None, None) == _lib.JQ_OK
        assert out4[0] != 0.0 and dout[0] != 0.0 and not w.any()
    finally:
        wa.close()
