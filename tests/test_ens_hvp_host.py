"""CPU: Hessian-vector products of a risk-neutral ensemble (jq_eval_f_g_grad_hvp) through the layers that need no GPU -- the ensemble
reference (tests/ensemble_hessian_reference.py) against Richardson-extrapolated central differences of the oracle's weighted gradient,
the header / ctypes table / library export / Julia binding of the entry point, the argument errors of the Python surfaces (raised
before the library is loaded), the Tikhonov term of eval_hessvec_par and the refusals of setup_ipopt_problem(hessian="exact")."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
from test_julia_shim import CTYPE, header, julia

import ensemble_hessian_reference as ER
from block_band_problem import block_band_problem

NSTEPS = 7


def test_ensemble_reference_matches_richardson_differences(jq):
    """3 nodes, Ntot 3, objFuncType 3: hv_infid and hv_infid + hv_leak against (4 cd(h/2) - cd(h))/3 of the oracle's weighted gradients,
    h = 1e-3/|d|; the bound of tests/test_hvp_host.py for the same comparison (1.2e-10)"""
    rng = np.random.default_rng(7301)
    p, pcof = block_band_problem(jq, rng, 3, 2, 0, [1, 1], NSTEPS, 4, 3)
    nodes, weights = np.array([-0.7, 0.0, 0.4]), np.array([0.25, 0.5, 0.25])
    shift = np.array([0.0, 0.3, -0.2])
    d = rng.standard_normal(pcof.size)
    h = 1e-3 / np.linalg.norm(d)

    def cd(step):
        a, b = ER.weighted_oracle_gradients(p, pcof + step * d, nodes, weights, shift), ER.weighted_oracle_gradients(p, pcof - step * d, nodes, weights, shift)
        return [(x - y) / (2.0 * step) for x, y in zip(a, b)]

    r = ER.EnsembleHessianReference(p, nodes, weights, shift).hvp(pcof, d)
    rich = [(4.0 * x - y) / 3.0 for x, y in zip(cd(0.5 * h), cd(h))]
    for name, mine, want in (("totalgrad", r["hv_infid"] + r["hv_leak"], rich[0]), ("infidelgrad", r["hv_infid"], rich[1])):
        rel = np.linalg.norm(mine - want) / np.linalg.norm(want)
        print("d(%s): ensemble reference vs Richardson differences, relative %.2e" % (name, rel))
        assert rel < 1.2e-10
    # (the nodes matter: the unperturbed problem alone is another vector)
    one = ER.EnsembleHessianReference(p, [0.0], [1.0], shift).hvp(pcof, d)
    assert np.linalg.norm(one["hv_infid"] - r["hv_infid"]) > 1e-6 * np.linalg.norm(r["hv_infid"])


ENS_ARGS = ["jq_handle *", "const double *", "int32_t", "const double *", "int32_t", "const double *", "const double *", "int32_t",
            "const double *", "double *", "double *", "double *", "double *", "double *"]


def test_header_symbol_table_and_library_export_agree():
    from juqbox_jl_amd import _lib
    _, protos = header()
    assert "jq_eval_f_g_grad_hvp" in protos
    ret, args = protos["jq_eval_f_g_grad_hvp"]
    assert ret == "int" and args == ENS_ARGS
    restype, argtypes = _lib.SYMBOLS["jq_eval_f_g_grad_hvp"]
    assert restype is ctypes.c_int
    d, i = _lib.c_dp, _lib.c_i32
    assert argtypes == [ctypes.c_void_p, d, i, d, i, d, d, i, d, d, d, d, d, d]
    L = _lib.load()
    assert L.jq_eval_f_g_grad_hvp is not None
    assert L.jq_abi_version() == 6      # a new symbol, no layout change: the version stays
    assert "JQ_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "juqbox_hip.h")).read()


def test_null_handle_is_einval():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    z = lambda n: np.zeros(n)
    out2, ig, lg, hvi, hvl, pc, d, nodes, w = z(2), z(12), z(12), z(12), z(12), z(12), np.ones(12), z(1), np.ones(1)
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)
    assert L.jq_eval_f_g_grad_hvp(None, dp(pc), 12, dp(d), 1, dp(nodes), dp(w), 1, None, dp(out2), dp(ig), dp(lg), dp(hvi), dp(hvl)) == _lib.JQ_EINVAL
    assert not out2.any() and not ig.any() and not hvi.any() and not hvl.any()


def test_julia_wrapper_and_its_ccall_match_the_header():
    _, protos = header()
    _, calls = julia()
    mine = [c for c in calls if c[0] == "jq_eval_f_g_grad_hvp"]
    assert len(mine) == 1
    _, ret, args = mine[0]
    cret, cargs = protos["jq_eval_f_g_grad_hvp"]
    assert ret in CTYPE[cret]
    assert len(args) == len(cargs)
    for ct, jt in zip(cargs, args):
        assert jt in CTYPE[ct], (ct, jt)
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "hip_backend.jl")).read())
    assert re.search(r"function eval_f_g_grad_hvp\(pcof::Vector\{Float64\}, dirs::VecOrMat\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP,", txt)


def test_documents_and_exports_name_the_call():
    import juqbox_jl_amd as jq
    assert callable(jq.eval_f_g_grad_hvp) and callable(jq.eval_hessvec_par)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "jq_eval_f_g_grad_hvp" in design and "k_backward_lane_tl" in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert "eval_f_g_grad_hvp" in open(os.path.join(ROOT, doc)).read(), doc


# ---- the Python surfaces: argument errors before any library call ---------------------------------------------------------------------
class _NoLibrary:
    def __call__(self):
        raise AssertionError("the library was loaded before the arguments were checked")


class _Params:
    Ntot, N, objFuncType = 4, 2, 3


@pytest.fixture
def fake_wa(monkeypatch):
    import juqbox_jl_amd as jq
    from juqbox_jl_amd import _lib, evalobjgrad
    monkeypatch.setattr(_lib, "load", _NoLibrary())
    wa = object.__new__(evalobjgrad.Working_Arrays_HIP)
    wa.handle = None
    wa.nCoeff = 12
    wa.params = _Params()
    return jq, wa


@pytest.mark.parametrize("bad", [np.zeros(11), np.zeros((11, 3)), np.zeros((12, 0)), np.zeros((12, 2, 2)), np.full(12, np.nan), "direction"],
                         ids=["1d-wrong-length", "2d-wrong-rows", "zero-columns", "3d", "nan", "string"])
def test_direction_errors_come_before_any_library_call(fake_wa, bad):
    jq, wa = fake_wa
    with pytest.raises(ValueError, match="eval_f_g_grad_hvp"):
        jq.eval_f_g_grad_hvp(np.zeros(12), bad, wa.params, wa)


def test_other_shape_errors_come_before_any_library_call(fake_wa):
    jq, wa = fake_wa
    ok = np.zeros(12)
    with pytest.raises(ValueError, match="pcof"):
        jq.eval_f_g_grad_hvp(np.zeros(11), ok, wa.params, wa)
    with pytest.raises(ValueError, match="nodes and weights"):
        jq.eval_f_g_grad_hvp(ok, ok, wa.params, wa, nodes=[0.0, 0.1], weights=[1.0])
    with pytest.raises(ValueError, match="nodes and weights"):
        jq.eval_f_g_grad_hvp(ok, ok, wa.params, wa, nodes=[[0.0]], weights=[[1.0]])
    with pytest.raises(ValueError, match="at least one node"):
        jq.eval_f_g_grad_hvp(ok, ok, wa.params, wa, nodes=[], weights=[])
    with pytest.raises(ValueError, match="shift"):
        jq.eval_f_g_grad_hvp(ok, ok, wa.params, wa, shift=np.zeros(3))
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_hvp(ok, ok, _Params(), wa)      # another objparams
    with pytest.raises(TypeError):
        jq.eval_f_g_grad_hvp(ok, ok, wa.params, object())
    with pytest.raises(ValueError, match="eval_f_g_grad_hvp"):
        jq.eval_hessvec_par(ok, np.zeros(11), wa.params, wa)


def test_tikhonov_term_of_the_hessvec_is_the_difference_of_tikhonov_grad(monkeypatch):
    """tikhonov_grad is affine in pcof: its derivative along d is the difference of two gradients, with or without prior coefficients;
    eval_hessvec_par adds exactly that to the library's products (objFuncType 1: hv_infid + hv_leak, else hv_infid)"""
    from juqbox_jl_amd import ipopt_interface as ip
    from juqbox_jl_amd.setup_utils import tikhonov_grad
    rng = np.random.default_rng(5)
    pcof, d, prior = rng.standard_normal(12), rng.standard_normal(12), rng.standard_normal(12)
    tik0 = 0.37
    for pr in (None, prior):
        diff = tikhonov_grad(pcof + d, tik0, pr) - tikhonov_grad(pcof, tik0, pr)
        assert np.allclose(ip.tikhonov_hessvec(d, tik0), diff, rtol=1e-13, atol=1e-15)
    hvi, hvl = rng.standard_normal((12, 1)), rng.standard_normal((12, 1))
    monkeypatch.setattr(ip, "eval_f_g_grad_hvp", lambda *a, **k: dict(hv_infid=hvi, hv_leak=hvl))
    for typ, lib in ((1, hvi[:, 0] + hvl[:, 0]), (2, hvi[:, 0])):
        par = types.SimpleNamespace(objFuncType=typ, tik0=tik0, usingPriorCoeffs=True, priorCoeffs=prior)
        got = ip.eval_hessvec_par(pcof, d, par, None)
        assert np.array_equal(got, lib + tikhonov_grad(d, tik0, None))
        assert np.allclose(got - lib, tikhonov_grad(pcof + d, tik0, prior) - tikhonov_grad(pcof, tik0, prior), rtol=1e-13, atol=1e-15)


def test_exact_hessian_refusals_of_setup_ipopt_problem():
    import juqbox_jl_amd as jq
    lo, hi = -np.ones(12), np.ones(12)
    with pytest.raises(ValueError, match="objFuncType == 3"):
        jq.setup_ipopt_problem(types.SimpleNamespace(objFuncType=3), None, 12, lo, hi, hessian="exact")
    p = types.SimpleNamespace(objFuncType=1, Ntot=4)
    with pytest.raises(ValueError, match="drifts or ctrl_mix"):
        jq.setup_ipopt_problem(p, None, 12, lo, hi, hessian="exact", drifts=[np.eye(4)], drift_weights=[1.0])
    with pytest.raises(ValueError, match="drifts or ctrl_mix"):
        jq.setup_ipopt_problem(p, None, 12, lo, hi, hessian="exact", ctrl_mix=[np.eye(2)], member_weights=[1.0])
    with pytest.raises(ValueError, match="hessian must be"):
        jq.setup_ipopt_problem(p, None, 12, lo, hi, hessian="bfgs")
