"""CPU: Hessian-vector products in sample space (jq_eval_f_g_grad_samples_hvp) through the layers that need no GPU -- the entry point in
the header, the library, the ctypes table, the Python exports and the Julia binding; the CPU reference of
tests/sampled_hessian_reference.py (the unchanged oracle behind B = d pq / d pcof of full row rank) against null-space moves of its
coefficient vectors and against Richardson-extrapolated central differences of the oracle's gradient; the argument errors of the Python
surfaces, raised before the library is loaded; and the chain rule of torch_controls.sampled_hessvec on a synthetic objective with a
NON-symmetric second derivative."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, reference_pass
from test_julia_shim import CTYPE, header, julia

import ensemble_hessian_reference as ER
import sampled_hessian_reference as SR
from test_gpu_random import random_problem

NAME = "jq_eval_f_g_grad_samples_hvp"
ARGS = ["jq_handle *", "const double *", "int32_t", "const double *", "int32_t", "const double *", "const double *", "int32_t",
        "const double *", "double *", "double *", "double *", "double *", "double *"]


def test_header_symbol_table_library_export_and_julia_agree():
    from juqbox_jl_amd import _lib
    _, protos = header()
    assert NAME in protos, NAME + ": not declared in include/juqbox_hip.h"
    ret, args = protos[NAME]
    assert ret == "int" and args == ARGS
    assert NAME in _lib.SYMBOLS, NAME + ": not in the binding table of juqbox.jl_amd/_lib.py"
    restype, argtypes = _lib.SYMBOLS[NAME]
    d, i = _lib.c_dp, _lib.c_i32
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, d, i, d, i, d, d, i, d, d, d, d, d, d]
    assert getattr(ctypes.CDLL(_lib.LIB_PATH), NAME) is not None      # (AttributeError: not exported)
    L = _lib.load()
    assert L.jq_abi_version() == 6      # a new symbol, no layout change: the version stays
    assert "JQ_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "juqbox_hip.h")).read()
    _, calls = julia()
    mine = [c for c in calls if c[0] == NAME]
    assert len(mine) == 1, NAME + ": no ccall in julia/hip_backend.jl"
    _, jret, jargs = mine[0]
    assert jret in CTYPE[ret] and len(jargs) == len(args)
    for ct, jt in zip(args, jargs):
        assert jt in CTYPE[ct], (ct, jt)
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "hip_backend.jl")).read())
    assert re.search(r"function eval_f_g_grad_samples_hvp\(pq::Matrix\{Float64\}, dirs::Union\{Matrix\{Float64\}, Array\{Float64, 3\}\}, params::objparams,", txt)


def test_null_handle_is_einval_and_writes_nothing():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    z = lambda n: np.zeros(n)
    out2, ig, lg, hvi, hvl, tab, d, nodes, w = z(2), z(12), z(12), z(12), z(12), z(12), np.ones(12), z(1), np.ones(1)
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)
    assert L.jq_eval_f_g_grad_samples_hvp(None, dp(tab), 3, dp(d), 1, dp(nodes), dp(w), 1, None, dp(out2), dp(ig), dp(lg), dp(hvi), dp(hvl)) == _lib.JQ_EINVAL
    assert not out2.any() and not ig.any() and not hvi.any() and not hvl.any()


def test_python_exports_and_documents_name_the_call(jq):
    assert callable(jq.eval_f_g_grad_samples_hvp) and callable(jq.traceobjgrad_samples_hvp)
    from juqbox_jl_amd import torch_controls
    assert callable(torch_controls.sampled_hessvec)
    assert "torch_controls" not in open(os.path.join(ROOT, "juqbox.jl_amd", "__init__.py")).read()      # (importing the package does not import torch)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert NAME in design and "k_ctrl_samples_grouped" in design and "k_gradsamples_grouped" in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert "eval_f_g_grad_samples_hvp" in open(os.path.join(ROOT, doc)).read(), doc


# ---- the reference helper on three CPU problems ----------------------------------------------------------------------------------------
#            Ntot N  nsteps m objFuncType nodes
PROBLEMS = ((5, 2, 2, 0, 2, 1),
            (12, 3, 7, 3, 1, 3),
            (4, 3, 1, 2, 3, 2))


def _setup(jq, Ntot, N, nsteps, m, typ, nq):
    rng = np.random.default_rng(9100 + 100 * Ntot + nsteps)
    p = random_problem(jq, rng, Ntot, N, 2, 1, nsteps, m, typ, False)[0]
    nodes = np.zeros(1) if nq == 1 else 0.1 * rng.standard_normal(nq)
    weights = np.ones(1) if nq == 1 else rng.random(nq) + 0.1
    shift = 0.3 * rng.standard_normal(Ntot)
    shift[0] = 0.0
    nf, nt = 2 * p.Ncoupled, 2 * nsteps + 1
    S = SR.piecewise_constant_table(rng, nf, nt)
    V = rng.standard_normal((nf, nt))
    return rng, p, nodes, weights, shift, S, V


def richardson(f, x, d, h, levels=3):
    """central differences of f along d at steps h, h / 2, ...: extrapolated to O(h^(2 levels)) (tests/test_uncoupled_matrix.py)"""
    T = [[(f(x + (h / 2 ** i) * d) - f(x - (h / 2 ** i) * d)) / (2 * h / 2 ** i)] for i in range(levels)]
    for i in range(1, levels):
        for k in range(1, i + 1):
            T[i].append(T[i][k - 1] + (T[i][k - 1] - T[i - 1][k - 1]) / (4 ** k - 1))
    return T[-1][-1]


@pytest.mark.parametrize("Ntot,N,nsteps,m,typ,nq", PROBLEMS, ids=["Ntot%d-N%d-steps%d-m%d-type%d-nq%d" % c for c in PROBLEMS])
def test_reference_is_null_space_invariant_and_matches_richardson_differences(jq, Ntot, N, nsteps, m, typ, nq):
    """S = B x and V = B d with x, d from lstsq: the reference does not change when x and d move by O(1) null-space vectors of B
    (<= 1e-12 relative), and it equals the Richardson-extrapolated central differences (h = 1e-2, three levels) of the oracle's weighted
    gradients, unfolded to sample space, within the project's reference_pass."""
    rng, p, nodes, weights, shift, S, V = _setup(jq, Ntot, N, nsteps, m, typ, nq)
    ref = SR.SampledHessianReference(jq, p, nodes, weights, shift)
    B = ref.B
    sv = np.linalg.svd(B, compute_uv=False)
    assert sv.size == B.shape[0] and sv[0] / sv[-1] <= 1.0 / 0.35      # (full row rank, tests/test_sampled_controls_host.py)
    x, d = ref.coefficients(S), ref.coefficients(V)
    r = ref.hvp(S, V, x, d)
    g = ref.gradients(S, x)
    # null space of B: the trailing right singular vectors
    null = np.linalg.svd(B)[2][B.shape[0]:].T
    assert null.shape[1] == B.shape[1] - B.shape[0] > 0 and np.abs(B @ null).max() <= 1e-14
    xn, dn = x + null @ rng.standard_normal(null.shape[1]), d + null @ rng.standard_normal(null.shape[1])
    rn, gn = ref.hvp(S, V, xn, dn), ref.gradients(S, xn)
    for k in ("hv_infid", "hv_leak", "hv"):
        rel = np.linalg.norm(rn[k] - r[k]) / max(np.linalg.norm(r[k]), 1e-300)
        print("%s: relative change under null-space moves %.2e" % (k, rel))
        assert rel <= 1e-12, k
    for k in ("infid_grad", "leak_grad"):
        assert np.linalg.norm(gn[k] - g[k]) <= 1e-12 * max(np.linalg.norm(g[k]), 1e-300), k
    # Richardson differences of the oracle's weighted gradients (totalgrad, infidelgrad) along d in coefficient space = B' Hs V
    def grads(v):
        return np.concatenate(ER.weighted_oracle_gradients(p, v, nodes, weights, shift))
    rich = richardson(grads, x, d, 1e-2)
    n = x.size
    want = {"hv": ref.unfold(rich[:n]), "hv_infid": ref.unfold(rich[n:] if typ != 1 else rich[:n])}
    for k, w in want.items():
        rel = np.linalg.norm(r[k] - w) / np.linalg.norm(w)
        print("%s: reference vs Richardson differences, relative %.2e (|.| %.3e)" % (k, rel, np.linalg.norm(w)))
        assert reference_pass(r[k], w), (k, rel)
    if typ == 1:
        assert not r["hv_leak"].any() and np.array_equal(r["hv"], r["hv_infid"])
    else:
        assert np.allclose(r["hv_leak"], r["hv"] - r["hv_infid"], rtol=0, atol=1e-13 * np.abs(r["hv"]).max())
    print("lstsq residuals <= %.1e, cond(B) = %.2f" % (ref.residual, sv[0] / sv[-1]))
    assert ref.residual <= 1e-13
    # (the direction matters: another table gives another product)
    other = ref.hvp(S, V[:, ::-1])
    assert np.linalg.norm(other["hv"] - r["hv"]) > 1e-6 * np.linalg.norm(r["hv"])


# ---- the Python surfaces: argument errors before any library call ---------------------------------------------------------------------
class _NoLibrary:
    def __call__(self):
        raise AssertionError("the library was loaded before the arguments were checked")


class _Params:
    Ntot, N, objFuncType, Ncoupled, nsteps = 4, 2, 3, 2, 3


@pytest.fixture
def fake_wa(monkeypatch):
    import juqbox_jl_amd as jq
    from juqbox_jl_amd import _lib, evalobjgrad
    monkeypatch.setattr(_lib, "load", _NoLibrary())
    wa = object.__new__(evalobjgrad.Working_Arrays_HIP)
    wa.handle = None
    wa.nCoeff = 20
    wa.params = _Params()
    return jq, wa


OK = np.zeros((4, 7))
BAD_TABLES = [np.zeros((4, 6)), np.zeros((7, 4)), np.zeros(28), np.full((4, 7), np.nan), np.full((4, 7), np.inf), "table"]
BAD_DIRS = BAD_TABLES + [np.zeros((4, 7, 0)), np.zeros((3, 4, 7)), np.zeros((4, 7, 2, 1)), np.dstack([OK, np.full((4, 7), np.nan)])]


@pytest.mark.parametrize("which", range(len(BAD_TABLES)))
def test_table_errors_come_before_any_library_call(fake_wa, which):
    jq, wa = fake_wa
    with pytest.raises(ValueError, match="eval_f_g_grad_samples_hvp"):
        jq.eval_f_g_grad_samples_hvp(BAD_TABLES[which], OK, wa.params, wa)
    with pytest.raises(ValueError, match="traceobjgrad_samples_hvp"):
        jq.traceobjgrad_samples_hvp(BAD_TABLES[which], OK, wa.params, wa)


@pytest.mark.parametrize("which", range(len(BAD_DIRS)))
def test_direction_errors_come_before_any_library_call(fake_wa, which):
    jq, wa = fake_wa
    with pytest.raises(ValueError, match="eval_f_g_grad_samples_hvp: dirs"):
        jq.eval_f_g_grad_samples_hvp(OK, BAD_DIRS[which], wa.params, wa)
    with pytest.raises(ValueError, match="traceobjgrad_samples_hvp: dirs"):
        jq.traceobjgrad_samples_hvp(OK, BAD_DIRS[which], wa.params, wa)


def test_other_argument_errors_come_before_any_library_call(fake_wa):
    jq, wa = fake_wa
    f = jq.eval_f_g_grad_samples_hvp
    with pytest.raises(ValueError, match="nodes and weights"):
        f(OK, OK, wa.params, wa, nodes=[0.0, 0.1], weights=[1.0])
    with pytest.raises(ValueError, match="nodes and weights"):
        f(OK, OK, wa.params, wa, nodes=[[0.0]], weights=[[1.0]])
    with pytest.raises(ValueError, match="at least one node"):
        f(OK, OK, wa.params, wa, nodes=[], weights=[])
    with pytest.raises(ValueError, match="shift"):
        f(OK, OK, wa.params, wa, shift=np.zeros(3))
    with pytest.raises(ValueError):
        f(OK, OK, _Params(), wa)      # another objparams
    with pytest.raises(TypeError):
        f(OK, OK, wa.params, object())
    from juqbox_jl_amd.evalobjgrad import _direction_tables
    one, n1 = _direction_tables(OK + 1.0, wa.params, "t")
    stack, n3 = _direction_tables(np.dstack([OK, OK + 1.0, OK + 2.0]), wa.params, "t")
    assert (one.size, n1, stack.size, n3) == (28, 1, 84, 3)
    assert np.array_equal(stack[28:56], one)      # (one table after the other, each column-major)


# ---- sampled_hessvec: the chain rule around the library call --------------------------------------------------------------------------
def test_sampled_hessvec_chain_rule_on_a_synthetic_objective(monkeypatch):
    """J(s) = c's + s'A s / 2 + sum(s^3) / 6 with a NON-symmetric A stands in for the library: its "gradient" G = c + A s + s^2 / 2 and
    "product" Hs u = A u + s u are what the library returns (the derivative of G, not of a symmetrised one).  For fn(theta) = tanh-saturated
    segment amplitudes through repeat_interleave the result must be Jfn'(Hs (Jfn v)) + (d Jfn / d theta . v)' G, here in closed form; a
    transposed A (what double backward through autograd would need) is another vector."""
    import torch
    from juqbox_jl_amd import torch_controls as tc
    rng = np.random.default_rng(31)
    nf, nt, nseg, rep = 4, 7, 4, 2
    A, c = rng.standard_normal((nf * nt, nf * nt)), rng.standard_normal(nf * nt)
    calls = []

    def fake(pq, dirs, params, wa, nodes=(0.0,), weights=(1.0,), shift=None, _who=""):
        s, u = np.asarray(pq).ravel(order="F"), np.asarray(dirs).ravel(order="F")
        calls.append((nodes, weights, shift))
        G, Hu = c + A @ s + 0.5 * s * s, A @ u + s * u
        sh = (nf, nt)
        return dict(infidelity=0.0, leak=0.0, infid_grad=0.25 * G.reshape(sh, order="F"), leak_grad=0.75 * G.reshape(sh, order="F"),
                    hv_infid=0.25 * Hu.reshape(sh + (1,), order="F"), hv_leak=0.75 * Hu.reshape(sh + (1,), order="F"))

    monkeypatch.setattr(tc, "eval_f_g_grad_samples_hvp", fake)
    amp = 0.7
    fn = lambda th: (amp * torch.tanh(th)).repeat_interleave(rep, dim=1)[:, :nt]
    theta, v = rng.standard_normal((nf, nseg)), rng.standard_normal((nf, nseg))
    got = tc.sampled_hessvec(fn, torch.from_numpy(theta), torch.from_numpy(v), None, None).numpy()
    # closed form: sample (f, J) depends on theta[f, J // rep] only
    seg = np.arange(nt) // rep
    t1, t2 = amp * (1.0 - np.tanh(theta) ** 2), -2.0 * amp * np.tanh(theta) * (1.0 - np.tanh(theta) ** 2)      # fn', fn'' per amplitude
    s = (amp * np.tanh(theta))[:, seg]
    u = (t1 * v)[:, seg]
    G = (c + A @ s.ravel(order="F") + 0.5 * s.ravel(order="F") ** 2).reshape((nf, nt), order="F")
    Hu = (A @ u.ravel(order="F") + s.ravel(order="F") * u.ravel(order="F")).reshape((nf, nt), order="F")
    want, wrong = np.zeros((nf, nseg)), np.zeros((nf, nseg))
    HuT = (A.T @ u.ravel(order="F") + s.ravel(order="F") * u.ravel(order="F")).reshape((nf, nt), order="F")
    for k in range(nseg):
        want[:, k] = t1[:, k] * Hu[:, seg == k].sum(axis=1) + t2[:, k] * v[:, k] * G[:, seg == k].sum(axis=1)
        wrong[:, k] = t1[:, k] * HuT[:, seg == k].sum(axis=1) + t2[:, k] * v[:, k] * G[:, seg == k].sum(axis=1)
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("sampled_hessvec against the closed form: relative %.2e" % rel)
    assert reference_pass(got, want)
    assert np.linalg.norm(got - wrong) > 1e-3 * np.linalg.norm(want)
    assert len(calls) == 1 and calls[0] == ((0.0,), (1.0,), None)
    # a linear fn: no curvature term; nodes and weights reach the library call
    M = torch.from_numpy(rng.standard_normal((nf * nt, 5)))
    lin = lambda th: (M @ th).reshape(nt, nf).T
    th, vv = rng.standard_normal(5), rng.standard_normal(5)
    got = tc.sampled_hessvec(lin, torch.from_numpy(th), torch.from_numpy(vv), None, None, [0.1, 0.2], [0.5, 0.5], None).numpy()
    sl = M.numpy() @ th
    assert reference_pass(got, M.numpy().T @ (A @ (M.numpy() @ vv) + sl * (M.numpy() @ vv)))
    assert calls[-1][0] == [0.1, 0.2]
    with pytest.raises(TypeError):
        tc.sampled_hessvec(lin, torch.zeros(5, dtype=torch.float32), torch.zeros(5, dtype=torch.float32), None, None)
    with pytest.raises(ValueError):
        tc.sampled_hessvec(lin, torch.from_numpy(th), torch.from_numpy(vv), None, None, nodes=[0.0])
