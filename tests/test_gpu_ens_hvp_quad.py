"""GPU (-m gpu): jq_eval_f_g_grad_hvp on the quad route -- Hessian-vector products of a risk-neutral ensemble at Ntot > 16 with the
4 x 4 x n structure on the tangent-linear quad-layout kernels (k_init_quad_tl, k_forward_quad_tl, k_terminal_cols<QuadMap, EP_TL>,
k_backward_quad_tl; objects t_<NT>_7), against the CPU reference of tests/ensemble_hessian_reference.py.

Random 4 x 4 x n problems from tests/subsystem_problem.py (control q on subsystem q only: every T4 mode of the trace products), 7 time
steps, at the smallest shapes where a quad-layout kernel can go wrong: NT 2 zero padded and full (Ntot 29, 32: only the mt > 0 and the
mt + 1 < NT coupling edges), NT 3 (Ntot 48: an interior block with both +- 16 neighbours), NT 6 zero padded and full (Ntot 93, 96:
cnot3's size and its register pressure); N 4 (one quad per node), N 3 (one node: a padding column; three nodes: 9 columns, nodes straddle
quads), N 2 x 3 nodes (two nodes in one quad, the last quad half empty), 13 nodes x N 4 (13 quads: workgroups of 4 + 4 + 4 + 1 waves);
one node at eps 0; 1 / 2 / 3 controls and, from a generator of this file, 4 (the fourth fills all three parts of the image); Neumann
order 0 / 1 / 4; objFuncType 1 / 2 / 3; one chunk and chunks of 3 + 3 + 1; 1 and 5 directions; the default shift and a given one; one
case of 40 steps in chunks of 16 + 16 + 8.  The default shift table is 0.01 x 10^(i-1): as in tests/test_gpu_ens_hvp_rowlane.py the
default-shift cases scale their nodes by 10^-(Ntot - 4) (max |eps shift| ~ 0.05, the size of the given-shift cases), and the CPU
reference alone shows that the nodes still change hv_infid by more than 1e-6 relative, so a dropped shift cannot pass.

Criterion: the project's reference_pass (atol 1e-14 or rtol 1e-10) on every column of hv_infid and hv_leak; out2 and the gradients
against eval_f_g_grad on the same handle; a direction of a 5-direction call and directions in rounds bit-identical to the direction
alone / one launch; option quad=0, five controls, an unstructured problem and an embedded structure stay on the sequential route; the
refusals are tl_refuse's; the exact-Hessian callback of setup_ipopt_problem runs on the route; the t_ objects ship in the VGPR register
form, so the NT 6 case runs through the default-form twin of the library too and must give the same bits."""
import collections
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import reference_pass

import block_band_matrix as M
import ensemble_hessian_reference as ER
from block_band_problem import block_band_problem
from kronecker_problem import random_kronecker_problem
from subsystem_problem import PARTS, _part, subsystem_problem, t4_structure
from test_gpu_ens_hvp import SAME_BITS, _check_against_reference, _check_primal, _reference, _total_gradient
from test_gpu_hvp import REFUSALS, _directions, _refusal_handles

pytestmark = pytest.mark.gpu

QCase = collections.namedtuple("QCase", "n Ntot N Nc m chunk ndir objFuncType nquad shift flavour nsteps")
NSTEPS = 7
KF_QUAD, KF_COOP = 6, 1
QUAD_CASES = (
    QCase(2, 29, 4, 1, 4, 0, 5, 1, 1, "default", "varied", NSTEPS),      # NT 2 zero padded, one quad, one node at eps 0
    QCase(2, 32, 3, 2, 0, 3, 1, 3, 3, "given", "uniform", NSTEPS),       # NT 2 full, 9 columns = 3 quads, no Neumann terms, chunks, unforced pass
    QCase(3, 48, 2, 3, 1, 0, 5, 2, 3, "default", "varied", NSTEPS),      # NT 3, 6 columns: two nodes in one quad, the last quad half empty
    QCase(2, 29, 4, 3, 1, 3, 1, 2, 13, "given", "varied", NSTEPS),       # 13 quads per direction: workgroups of 4 + 4 + 4 + 1 waves
    QCase(6, 93, 3, 3, 4, 0, 1, 1, 1, "given", "varied", NSTEPS),        # NT 6 zero padded, one node of N 3: a padding column
    QCase(6, 96, 4, 3, 4, 3, 1, 3, 3, "given", "uniform", NSTEPS),       # NT 6 full (cnot3's size), everything at once
    QCase(2, 32, 4, 4, 1, 0, 1, 3, 3, "default", "varied", NSTEPS),      # four controls, the fourth with all three parts
    QCase(2, 29, 2, 2, 1, 16, 1, 2, 3, "given", "varied", 40),           # 40 steps in chunks of 16 + 16 + 8: the carries cross chunks
)


def _id(c):
    return "NT%d-Ntot%d-N%d-Nc%d-m%d-%s-ndir%d-type%d-nq%d-%s-%s-%dsteps" % (c.n, c.Ntot, c.N, c.Nc, c.m, "chunks%d" % c.chunk if c.chunk else "onechunk",
                                                                            c.ndir, c.objFuncType, c.nquad, c.shift, c.flavour, c.nsteps)


def many_control_problem(jq, rng, n, Ntot, N, Nc, m, nsteps, objFuncType):
    """subsystem_problem with more than three controls: control q < 3 fills part PARTS[q] of the T4 image, every further one all three
    parts with independent entries (what the library multiplies with the full product)"""
    assert 16 * (n - 1) < Ntot <= 16 * n and n > 1 and Nc > 3
    def op(q, anti):
        return _part(rng, n, Ntot, PARTS[q], anti, "varied") if q < 3 else sum(_part(rng, n, Ntot, part, anti, "varied") for part in PARTS)
    T, Nfreq = 1.0 + rng.random(), 2
    Hs, Ha = [op(q, False) for q in range(Nc)], [op(q, True) for q in range(Nc)]
    H0 = sum(_part(rng, n, Ntot, part, False, "varied") for part in PARTS)
    for h in Hs + Ha + [H0]:
        assert t4_structure(h)
    scale = 2.0 / max(1.0, max(np.abs(np.linalg.eigvalsh(h)).max() for h in Hs + [H0]))
    U0 = np.linalg.qr(rng.standard_normal((Ntot, N)))[0]
    Ut = np.linalg.qr(rng.standard_normal((Ntot, N)) + 1j * rng.standard_normal((Ntot, N)))[0]
    p = jq.objparams([N], [Ntot - N], T, nsteps, Uinit=U0, Utarget=Ut, Cfreq=rng.standard_normal((Nc, Nfreq)), Rfreq=np.zeros(Nc), Hconst=H0 * scale,
                     Hsym_ops=[h * scale for h in Hs], Hanti_ops=[h * scale for h in Ha], objFuncType=objFuncType, linear_solver=jq.lsolver_object(max_iter=m))
    p.wmat_real = rng.random(Ntot) * (np.arange(Ntot) >= N)
    pcof = 0.3 * rng.standard_normal(2 * Nc * Nfreq * int(rng.integers(3, 7)))
    return p, pcof


def _problem(jq, c):
    rng = np.random.default_rng(97000 + 1000 * c.Ntot + 100 * c.N + 10 * c.Nc + c.m)
    if c.Nc <= 3:
        p, pcof = subsystem_problem(jq, rng, c.n, c.Ntot, c.N, c.Nc, c.m, c.flavour, c.nsteps, c.objFuncType)
    else:
        p, pcof = many_control_problem(jq, rng, c.n, c.Ntot, c.N, c.Nc, c.m, c.nsteps, c.objFuncType)
    if c.nquad == 1:
        nodes, weights = np.zeros(1), np.ones(1)
    else:
        nodes = 0.05 * np.linspace(-1.0, 1.0, c.nquad) + 0.01 * rng.standard_normal(c.nquad)
        weights = rng.random(c.nquad) + 0.1
        weights /= weights.sum()
    shift = None if c.shift == "default" else rng.standard_normal(c.Ntot)
    if shift is None:
        nodes = nodes * 10.0 ** -(c.Ntot - 4)
    return p, pcof, rng, nodes, weights, shift


def _options(c, extra=None):
    o = dict(extra or {})
    if c.chunk:
        o["chunk_steps"] = c.chunk
    return o or None


_cache = {}


def _set_up(jq, c):
    """problem, directions and CPU reference of a case, computed once and shared (never modified) by the tests that use the case"""
    if c not in _cache:
        p, pcof, rng, nodes, weights, shift = _problem(jq, c)
        D = _directions(rng, _total_gradient(p, pcof, nodes, weights, shift), pcof.size, c.ndir)
        refs = _reference(p, pcof, D, nodes, weights, shift)
        for t in refs:
            assert np.isfinite(t["hv_infid"]).all() and np.isfinite(t["hv_leak"]).all()
        _cache[c] = (p, pcof, nodes, weights, shift, D, refs)
    return _cache[c]


def _nchunks(c):
    cs = c.chunk or c.nsteps
    return (c.nsteps + cs - 1) // cs


def _assert_quad_records(wa, c, dpl, rounds):
    plan = wa.plan_info()
    assert plan["ens_hvp"] == {"route": "quad", "directions_per_launch": dpl, "chunk_steps": c.chunk or c.nsteps, "rounds": rounds}
    assert plan["last_kernels"]["object"] == "t_%d_7" % c.n and plan["last_kernels"]["forward_object"] == "t_%d_7" % c.n
    t = wa.last_timing()
    npass = 2 if c.objFuncType != 1 else 1
    assert (t["kernel_family"], t["kernel_size"], t["kernel_band"]) == (KF_QUAD, c.n, 7)
    assert t["n_forward_launches"] == rounds * _nchunks(c) and t["n_backward_launches"] == rounds * _nchunks(c) * npass


@pytest.mark.parametrize("c", QUAD_CASES, ids=[_id(c) for c in QUAD_CASES])
def test_quad_route_matches_reference(jq, c):
    p, pcof, nodes, weights, shift, D, refs = _set_up(jq, c)
    if c.nquad > 1 and c.Ntot <= 48:      # the CPU reference alone: the nodes matter (a kernel that dropped the shift would compute the eps = 0 ensemble)
        flat = ER.EnsembleHessianReference(p, np.zeros(c.nquad), weights, shift).hvp(pcof, D[:, 0])["hv_infid"]
        effect = np.linalg.norm(refs[0]["hv_infid"] - flat) / np.linalg.norm(refs[0]["hv_infid"])
        print("node effect on hv_infid[:, 0]: %.2e relative, |hv| %.2e" % (effect, np.linalg.norm(refs[0]["hv_infid"])))
        assert effect > 1e-6
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=_options(c))
    try:
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift)
        assert r["hv_infid"].shape == (pcof.size, c.ndir) and r["hv_leak"].shape == (pcof.size, c.ndir)
        _assert_quad_records(wa, c, c.ndir, 1)
        _check_against_reference(r, refs)
        _check_primal(jq, r, pcof, p, wa, nodes, weights, shift)
        if c.ndir == 5:
            for j in (1, 4):      # a direction alone: the same operations in the same order
                one = jq.eval_f_g_grad_hvp(pcof, D[:, j], p, wa, nodes, weights, shift)
                assert wa.plan_info()["ens_hvp"]["directions_per_launch"] == 1
                for k in ("hv_infid", "hv_leak"):
                    assert np.array_equal(one[k][:, 0], r[k][:, j]), (k, j)
                for k in SAME_BITS:
                    assert np.array_equal(one[k], r[k]), k
    finally:
        wa.close()


def test_directions_in_rounds_are_the_same_bits(jq):
    """a stream budget that holds the primal stream and two directions: five directions run in three rounds (2 + 2 + 1), bit-identical to
    one launch"""
    c = QUAD_CASES[2]
    p, pcof, nodes, weights, shift, D, refs = _set_up(jq, c)
    stride = 128 * c.n      # doubles of a T4 operator image
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    wb = jq.Working_Arrays_HIP(p, pcof.size, options={"stream_bytes": 8 * 3 * 2 * stride * (2 * NSTEPS + 1), "chunk_steps": NSTEPS})
    try:
        a, b = [jq.eval_f_g_grad_hvp(pcof, D, p, w, nodes, weights, shift) for w in (wa, wb)]
        _assert_quad_records(wa, c, 5, 1)
        _assert_quad_records(wb, c, 2, 3)
        for k in SAME_BITS + ("hv_infid", "hv_leak"):
            assert np.array_equal(a[k], b[k]), k
        _check_against_reference(b, refs)
    finally:
        wa.close()
        wb.close()


@pytest.mark.parametrize("c", (QUAD_CASES[3], QUAD_CASES[6]), ids=[_id(QUAD_CASES[3]), _id(QUAD_CASES[6])])
def test_option_quad0_switches_back_to_the_sequential_route(jq, c):
    """option quad=0 takes the quad-layout kernels away from the handle: the same call runs the nodes one after the other and passes the
    same reference"""
    p, pcof, nodes, weights, shift, D, refs = _set_up(jq, c)
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=_options(c, {"quad": 0}))
    try:
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift)
        plan = wa.plan_info()
        assert plan["ens_hvp"] == {"route": "sequential", "directions_per_launch": c.ndir, "chunk_steps": c.chunk or NSTEPS, "rounds": c.nquad}
        assert wa.last_timing()["kernel_family"] == KF_COOP
        _check_against_reference(r, refs)
        _check_primal(jq, r, pcof, p, wa, nodes, weights, shift)
    finally:
        wa.close()


def _sequential(jq, p, pcof, nodes, weights, shift, options=None):
    rng = np.random.default_rng(5)
    D = rng.standard_normal((pcof.size, 1))
    refs = _reference(p, pcof, D, nodes, weights, shift)
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=options)
    try:
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift)
        plan = wa.plan_info()
        assert plan["ens_hvp"]["route"] == "sequential" and wa.last_timing()["kernel_family"] == KF_COOP
        _check_against_reference(r, refs)
        return plan
    finally:
        wa.close()


def test_five_controls_stay_on_the_sequential_route(jq):
    """more than JQ_MAXNC controls run in control groups: the sequential route, as before"""
    rng = np.random.default_rng(97555)
    p, pcof = many_control_problem(jq, rng, 2, 29, 2, 5, 1, NSTEPS, 3)
    _sequential(jq, p, pcof, np.array([-0.03, 0.04]), np.array([0.4, 0.6]), rng.standard_normal(29))


def test_an_unstructured_problem_stays_on_the_sequential_route(jq):
    rng = np.random.default_rng(97529)
    p, pcof = block_band_problem(jq, rng, 29, 3, 1, [1, 1], NSTEPS, 1, 3)
    _sequential(jq, p, pcof, np.array([-0.03, 0.04]), np.array([0.4, 0.6]), rng.standard_normal(29))


def test_an_embedded_structure_stays_on_the_sequential_route(jq):
    """3 x 3 x 2 levels reach the 4 x 4 x n kernels through the embedded twin only: the handle's own plan has no such structure"""
    p, pcof, rng = random_kronecker_problem(jq, (3, 3, 2), 4)
    plan = _sequential(jq, p, pcof, np.array([-0.03, 0.04]), np.array([0.4, 0.6]), rng.standard_normal(18), {"embed": 2})
    assert plan["embedded_twin_Ntot"] == 32


def _quad_refusal_handles(jq):
    """the handles of tests/test_gpu_hvp.py REFUSALS on a problem that would take the quad route (the uncoupled one is that file's)"""
    rng = np.random.default_rng(97042)
    p, pcof = subsystem_problem(jq, rng, 2, 29, 3, 2, 3, "varied", NSTEPS, 3)
    pw = copy.copy(p)
    A = rng.standard_normal((29, 29))
    pw.wmat_real = np.asfortranarray(A @ A.T / 29.0)
    pw.wmat_imag = np.zeros((29, 29), order="F")
    ps = copy.copy(p)
    Dv = rng.standard_normal((29, 3)) + 1j * rng.standard_normal((29, 3))
    ps.dVds_r, ps.dVds_i, ps.sv_type = np.asfortranarray(Dv.real.copy()), np.asfortranarray(Dv.imag.copy()), 2
    return (("implicit-midpoint", M.with_solver(jq, p, "imr"), pcof, jq.Working_Arrays_M_HIP), ("jacobi", M.with_solver(jq, p, "jacobi"), pcof, jq.Working_Arrays_HIP),
            ("full-weights", pw, pcof, jq.Working_Arrays_HIP), ("sv_type", ps, pcof, jq.Working_Arrays_HIP), _refusal_handles(jq)[4])


@pytest.mark.parametrize("which", range(5), ids=REFUSALS)
def test_refusals_write_nothing_and_leave_the_handle_alone(jq, which):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    name, p, pcof, WA = _quad_refusal_handles(jq)[which]
    assert name == REFUSALS[which]
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


def test_the_exact_hessian_callback_runs_on_the_route(jq):
    """setup_ipopt_problem(hessian="exact") on an NT 2 problem: the callback's product is eval_f_g_grad_hvp's (plus the Tikhonov term)"""
    from juqbox_jl_amd import ipopt_interface as ip
    c = QUAD_CASES[0]
    p, pcof, nodes, weights, shift, D, refs = _set_up(jq, c)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    try:
        n = pcof.size
        prob = jq.setup_ipopt_problem(p, wa, n, np.full(n, -5.0), np.full(n, 5.0), maxIter=1, hessian="exact")
        hv = prob.eval_hessvec(pcof, D[:, 0])
        _assert_quad_records(wa, c._replace(chunk=0), 1, 1)
        r = jq.eval_f_g_grad_hvp(pcof, D[:, 0], p, wa)
        assert np.array_equal(hv, r["hv_infid"][:, 0] + r["hv_leak"][:, 0] + ip.tikhonov_hessvec(D[:, 0], p.tik0))
        assert reference_pass(r["hv_infid"][:, 0], refs[0]["hv_infid"])
    finally:
        wa.close()


def test_the_vgpr_form_objects_equal_their_default_form_twins_bit_for_bit():
    """the t_ objects are built with -amdgpu-mfma-vgpr-form=1 (csrc/Makefile): the NT 6 case with two directions through the shipped
    library and through libjuqbox_hip_df.so, a fresh process each (JQ_LIB is read when the library is loaded)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import check_forms
    root, tests = os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import numpy as np; import juqbox_jl_amd as jq; import test_gpu_ens_hvp_quad as T;"
            "c = T.QUAD_CASES[5]; p, pcof, rng, nodes, weights, shift = T._problem(jq, c);"
            "D = np.random.default_rng(1).standard_normal((pcof.size, 2));"
            "wa = jq.Working_Arrays_HIP(p, pcof.size, options=T._options(c)); r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift);"
            "print(wa.plan_info()['ens_hvp']['route'], ''.join(r[k].tobytes().hex() for k in ('hv_infid', 'hv_leak', 'infid_grad', 'leak_grad')));"
            "wa.close()" % (root, tests))
    outs = []
    for lib in (check_forms.MAIN, check_forms.DF):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, JQ_LIB=lib), capture_output=True, text=True, cwd=root)
        assert r.returncode == 0, r.stderr[-1000:]
        outs.append(r.stdout.strip().splitlines()[-1].split())
    assert outs[0][0] == outs[1][0] == "quad" and len(outs[0][1]) > 1000
    assert outs[0][1] == outs[1][1]
