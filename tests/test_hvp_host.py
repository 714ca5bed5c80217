"""CPU: the derivative of the gradient (Hessian-vector products) through the layers that need no GPU -- the construction of the CPU
reference (tests/hessian_reference.py: three runs of the unchanged oracle on the 2 Ntot problem with 3 Nc controls) against
Richardson-extrapolated central differences of the oracle's gradient, its symmetry at a high Neumann order, the header / ctypes table /
library export of jq_traceobjgrad_hvp, the Julia wrapper, and the argument errors of the Python surfaces, which are raised before the
library is loaded."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_julia_shim import CTYPE, header, julia

import hessian_reference as HR
from block_band_problem import block_band_problem, tile_rows

Case = collections.namedtuple("Case", "Ntot N Nc m objFuncType")
NSTEPS = 7
CASES = (Case(3, 2, 1, 4, 1), Case(3, 2, 2, 0, 3), Case(17, 3, 2, 1, 3), Case(29, 17, 2, 4, 3))


def _problem(jq, c):
    rng = np.random.default_rng(52000 + 1000 * c.Ntot + 100 * c.N + 10 * c.Nc + c.m)
    NT = tile_rows(c.Ntot)
    modes = ([1, 0, 2, 1, 1] if NT >= 2 else [1] * 5)[:c.Nc]
    p, pcof = block_band_problem(jq, rng, c.Ntot, c.N, NT - 1, modes, NSTEPS, c.m, c.objFuncType)
    return p, pcof, rng


@pytest.mark.parametrize("c", CASES, ids=["Ntot%d-N%d-Nc%d-m%d-type%d" % c for c in CASES])
def test_construction_matches_richardson_differences(jq, c):
    """a sanity bound on the construction (1.2e-10 = 20 x the largest value measured when it was written, 5.8e-12, the floor of the
    differences themselves), not a kernel tolerance: hv and hv_infid against (4 cd(h/2) - cd(h))/3 of the oracle's gradients,
    h = 1e-3/|d|"""
    from oracle.oracle import Oracle
    p, pcof, rng = _problem(jq, c)
    d = rng.standard_normal(pcof.size)
    orc = Oracle(p)
    h = 1e-3 / np.linalg.norm(d)

    def cd(step, key):
        return (orc.traceobjgrad(pcof + step * d)[key] - orc.traceobjgrad(pcof - step * d)[key]) / (2.0 * step)

    r = HR.hvp(p, pcof, d)
    for key, mine in (("totalgrad", r["hv"]), ("infidelgrad", r["hv_infid"])):
        rich = (4.0 * cd(0.5 * h, key) - cd(h, key)) / 3.0
        rel = np.linalg.norm(mine - rich) / np.linalg.norm(rich)
        print("%s d(%s): construction vs Richardson differences, relative %.2e" % (c, key, rel))
        assert rel < 1.2e-10


def test_symmetric_at_high_neumann_order(jq):
    """with 20 Neumann terms the linear solves are exact to rounding, the adjoint is the transpose of the forward scheme and the
    Jacobian of the gradient is the Hessian: |e.Jd - d.Je| <= 1e-12 |e.Jd| (measured 1.1e-15)"""
    rng = np.random.default_rng(1)
    p, pcof = block_band_problem(jq, rng, 17, 3, 0, [1], 7, 20, 1)
    d, e = rng.standard_normal(pcof.size), rng.standard_normal(pcof.size)
    ref = HR.HessianReference(p)
    eJd, dJe = e @ ref.hvp(pcof, d)["hv"], d @ ref.hvp(pcof, e)["hv"]
    print("e.Jd %.15e d.Je %.15e asymmetry %.2e" % (eJd, dJe, abs(eJd - dJe) / abs(eJd)))
    assert abs(eJd - dJe) <= 1e-12 * abs(eJd)


# ---- the C entry point -------------------------------------------------------------------------------------------------------------
HVP_ARGS = ["jq_handle *", "const double *", "int32_t", "const double *", "int32_t", "double *", "double *", "double *", "double *"]


def test_header_symbol_table_and_library_export_agree():
    from juqbox_jl_amd import _lib
    _, protos = header()
    assert "jq_traceobjgrad_hvp" in protos
    ret, args = protos["jq_traceobjgrad_hvp"]
    assert ret == "int" and args == HVP_ARGS
    restype, argtypes = _lib.SYMBOLS["jq_traceobjgrad_hvp"]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, _lib.c_dp, _lib.c_i32, _lib.c_dp, _lib.c_i32, _lib.c_dp, _lib.c_dp, _lib.c_dp, _lib.c_dp]
    L = _lib.load()
    assert L.jq_traceobjgrad_hvp is not None
    assert L.jq_abi_version() == 6      # no layout change, no change of an existing entry point: the version stays


def test_null_handle_is_einval():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    out4, grad, hv, pc, d = np.zeros(4), np.zeros(12), np.zeros(12), np.zeros(12), np.ones(12)
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)
    assert L.jq_traceobjgrad_hvp(None, dp(pc), 12, dp(d), 1, dp(out4), dp(grad), dp(hv), None) == _lib.JQ_EINVAL
    assert not out4.any() and not grad.any() and not hv.any()


def test_julia_wrapper_and_its_ccall_match_the_header():
    _, protos = header()
    _, calls = julia()
    mine = [c for c in calls if c[0] == "jq_traceobjgrad_hvp"]
    assert len(mine) == 1
    _, ret, args = mine[0]
    cret, cargs = protos["jq_traceobjgrad_hvp"]
    assert ret in CTYPE[cret]
    assert len(args) == len(cargs)
    for ct, jt in zip(cargs, args):
        assert jt in CTYPE[ct], (ct, jt)
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "hip_backend.jl")).read())
    assert re.search(r"function traceobjgrad_hvp\(pcof::Vector\{Float64\}, dirs::VecOrMat\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP\)", txt)
    assert re.search(r"function hessian\(pcof::Vector\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP, symmetrize::Bool = false\)", txt)


def test_documents_name_the_call_and_its_definition():
    hdr = open(os.path.join(ROOT, "include", "juqbox_hip.h")).read()
    assert "jq_traceobjgrad_hvp" in hdr and "JQ_ABI_VERSION 6" in hdr and "does not symmetrise silently" in hdr
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "jq_traceobjgrad_hvp" in design and "k_backward_tl" in design
    for doc in ("README.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        assert "hvp" in open(os.path.join(ROOT, doc)).read(), doc


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


@pytest.mark.parametrize("bad", [
    np.zeros(11),                          # one direction of the wrong length
    np.zeros((11, 3)),                     # columns of the wrong length
    np.zeros((12, 0)),                     # no direction
    np.zeros((12, 2, 2)),                  # not a matrix
    [np.zeros(12), np.zeros(11)],          # ragged
    np.full(12, np.nan),                   # not finite
    "direction",                           # not numbers
], ids=["1d-wrong-length", "2d-wrong-rows", "zero-columns", "3d", "ragged", "nan", "string"])
def test_hvp_direction_errors_come_before_any_library_call(fake_wa, bad):
    jq, wa = fake_wa
    with pytest.raises(ValueError, match="traceobjgrad_hvp"):
        jq.traceobjgrad_hvp(np.zeros(12), bad, wa.params, wa)


def test_hvp_pcof_and_handle_errors_come_before_any_library_call(fake_wa):
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.traceobjgrad_hvp(np.zeros(11), np.zeros(12), wa.params, wa)
    with pytest.raises(ValueError):
        jq.traceobjgrad_hvp(np.zeros(12), np.zeros(12), _Params(), wa)      # another objparams
    with pytest.raises(TypeError):
        jq.traceobjgrad_hvp(np.zeros(12), np.zeros(12), wa.params, object())
    with pytest.raises(ValueError):
        jq.hessian(np.zeros(11), wa.params, wa)
    with pytest.raises(ValueError):
        jq.hessian(np.zeros(12), _Params(), wa)
    with pytest.raises(TypeError):
        jq.hessian(np.zeros(12), wa.params, object())
