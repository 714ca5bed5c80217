"""CPU: the tangent (Jacobian-vector product) of the forward map through the layers that need no GPU -- the construction of the CPU
reference (tests/tangent_reference.py: the unchanged oracle on the block-triangular 2 Ntot problem) against central differences and
against the oracle's adjoint gradient, the header / ctypes table / library export of jq_traceobj_jvp, the Julia wrapper, and the
argument errors of the Python surfaces, which are raised before the library is loaded."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, case_inputs
from test_julia_shim import CTYPE, header, julia

import tangent_reference as TR

CASES = ("swap02", "cnot2")
_cache = {}


def _setup(case):
    """per case, computed once: params, pcof, the doubled oracle, the plain oracle's adjoint evaluation, the directions g/|g| and random"""
    if case not in _cache:
        from oracle.oracle import Oracle
        params, info, pcof, _ = case_inputs(case)
        orc = Oracle(params)
        adj = orc.traceobjgrad(pcof, evaladjoint=True)
        g = adj["totalgrad"]
        rng = np.random.default_rng(2718)
        rnd = rng.standard_normal(pcof.size)
        dirs = [g / np.linalg.norm(g), rnd / np.linalg.norm(rnd)]
        ref = TR.TangentReference(params)
        _cache[case] = dict(params=params, pcof=pcof, orc=orc, adj=adj, dirs=dirs, tan=[ref.tangent(pcof, d) for d in dirs])
    return _cache[case]


@pytest.mark.parametrize("case", CASES)
def test_construction_matches_central_differences(case):
    """a sanity bound on the construction (1e-5 = 20 x the largest value measured, 4.4e-7), not a kernel tolerance"""
    s = _setup(case)
    h = 1e-5
    for d, t in zip(s["dirs"], s["tan"]):
        fs = [s["orc"].traceobjgrad(s["pcof"] + sg * h * d, evaladjoint=False, final_state=True)["final_state"] for sg in (1.0, -1.0)]
        U = [f[:, :, 0] - 1j * f[:, :, 1] for f in fs]
        fd = (U[0] - U[1]) / (2.0 * h)
        rel = np.linalg.norm(t["W"] - fd) / np.linalg.norm(fd)
        print("%s: tangent vs central differences, relative %.2e" % (case, rel))
        assert rel < 1e-5
    # ... and the primal half of the doubled sweep is the plain sweep
    f0 = s["orc"].traceobjgrad(s["pcof"], evaladjoint=False, final_state=True)["final_state"]
    assert np.linalg.norm(s["tan"][0]["V"] - (f0[:, :, 0] - 1j * f0[:, :, 1])) < 1e-12 * np.linalg.norm(f0[:, :, :2])


@pytest.mark.parametrize("case", CASES)
def test_construction_matches_adjoint_gradient(case):
    """d(objfv) along g/|g| and a random direction against totalgrad . d at the case's own step count and weights: the project's rtol
    1e-10 over the vector of directions (measured 1.4e-12 on swap02, 5.0e-12 on cnot2)"""
    s = _setup(case)
    got = np.array([t["d_primary"] + t["d_secondary"] for t in s["tan"]])
    want = np.array([s["adj"]["totalgrad"] @ d for d in s["dirs"]])
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("%s: tangent vs adjoint, relative %.2e" % (case, rel))
    assert rel < 1e-10
    assert abs(s["tan"][0]["primaryobjf"] - s["adj"]["primaryobjf"]) < 1e-12


# ---- the C entry point -------------------------------------------------------------------------------------------------------------
JVP_ARGS = ["jq_handle *", "const double *", "int32_t", "const double *", "int32_t", "double *", "double *", "double *", "double *"]


def test_header_symbol_table_and_library_export_agree():
    from juqbox_jl_amd import _lib
    _, protos = header()
    assert "jq_traceobj_jvp" in protos
    ret, args = protos["jq_traceobj_jvp"]
    assert ret == "int" and args == JVP_ARGS
    restype, argtypes = _lib.SYMBOLS["jq_traceobj_jvp"]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, _lib.c_dp, _lib.c_i32, _lib.c_dp, _lib.c_i32, _lib.c_dp, _lib.c_dp, _lib.c_dp, _lib.c_dp]
    L = _lib.load()
    assert L.jq_traceobj_jvp is not None
    assert L.jq_abi_version() == 6      # no layout change, no change of an existing entry point: the version stays


def test_null_handle_is_einval():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    out4, dout, pc, d = np.zeros(4), np.zeros(3), np.zeros(12), np.ones(12)
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)
    assert L.jq_traceobj_jvp(None, dp(pc), 12, dp(d), 1, dp(out4), dp(dout), None, None) == _lib.JQ_EINVAL
    assert np.all(out4 == 0.0) and np.all(dout == 0.0)


def test_julia_wrapper_and_its_ccall_match_the_header():
    _, protos = header()
    _, calls = julia()
    mine = [c for c in calls if c[0] == "jq_traceobj_jvp"]
    assert len(mine) == 1
    _, ret, args = mine[0]
    cret, cargs = protos["jq_traceobj_jvp"]
    assert ret in CTYPE[cret]
    assert len(args) == len(cargs)
    for ct, jt in zip(cargs, args):
        assert jt in CTYPE[ct], (ct, jt)
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "hip_backend.jl")).read())
    assert re.search(r"function traceobj_jvp\(pcof::Vector\{Float64\}, dirs::VecOrMat\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP", txt)
    assert "is not accelerated" not in txt      # the verbose && evaladjoint method no longer calls error


# ---- the Python surfaces: argument errors before any library call ---------------------------------------------------------------------
class _NoLibrary:
    def __call__(self):
        raise AssertionError("the library was loaded before the arguments were checked")


class _Params:
    Ntot, N, kpar, sv_type = 4, 2, 1, 1


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


@pytest.mark.parametrize("bad", [
    np.zeros(11),                          # one direction of the wrong length
    np.zeros((11, 3)),                     # columns of the wrong length
    np.zeros((12, 0)),                     # no direction
    np.zeros((12, 2, 2)),                  # not a matrix
    [np.zeros(12), np.zeros(11)],          # ragged
    np.full(12, np.nan),                   # not finite
    "direction",                           # not numbers
], ids=["1d-wrong-length", "2d-wrong-rows", "zero-columns", "3d", "ragged", "nan", "string"])
def test_jvp_direction_errors_come_before_any_library_call(fake_wa, bad):
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.traceobj_jvp(np.zeros(12), bad, wa.params, wa)


def test_jvp_pcof_and_handle_errors_come_before_any_library_call(fake_wa):
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.traceobj_jvp(np.zeros(11), np.zeros(12), wa.params, wa)
    with pytest.raises(ValueError):
        jq.traceobj_jvp(np.zeros(12), np.zeros(12), _Params(), wa)      # another objparams
    with pytest.raises(TypeError):
        jq.traceobj_jvp(np.zeros(12), np.zeros(12), wa.params, object())


def test_directions_accept_a_vector_and_columns_alike():
    from juqbox_jl_amd.evalobjgrad import _directions
    rng = np.random.default_rng(7)
    M = rng.standard_normal((12, 3))
    a = _directions(M, 12)
    assert a.shape == (3, 12) and a.flags["C_CONTIGUOUS"] and np.array_equal(a, M.T)
    assert np.array_equal(_directions(np.asfortranarray(M), 12), a)
    assert np.array_equal(_directions(M[:, 1], 12), M[:, 1:2].T)
    assert np.array_equal(_directions(list(M[:, 2]), 12), M[:, 2:3].T)


@pytest.mark.parametrize("kpar", [0, 13, -1, 1.5])
def test_mirrored_call_kpar_errors_come_before_any_library_call(fake_wa, kpar):
    jq, wa = fake_wa
    wa.params.kpar = kpar
    with pytest.raises(ValueError, match="kpar"):
        jq.traceobjgrad(np.zeros(12), wa.params, wa, True, True)


@pytest.mark.parametrize("sv", [2, 3, 4])
def test_mirrored_call_sv_type_error_comes_before_any_library_call(fake_wa, sv):
    jq, wa = fake_wa
    wa.params.sv_type = sv
    with pytest.raises(ValueError, match="sv_type"):
        jq.traceobjgrad(np.zeros(12), wa.params, wa, True, True)


def test_docstrings_no_longer_say_the_branch_is_refused():
    import juqbox_jl_amd as jq
    assert "out of scope" not in jq.traceobjgrad.__doc__ and "traceobj_jvp" in jq.traceobjgrad.__doc__
    assert "refuses" not in jq.gradient_check.__doc__
    hdr = open(os.path.join(ROOT, "include", "juqbox_hip.h")).read()
    assert "jq_traceobj_jvp" in hdr and "JQ_ABI_VERSION 6" in hdr
