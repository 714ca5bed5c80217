"""CPU: Hessian-vector products of a drift ensemble (jq_eval_f_g_grad_drifts_hvp) through the layers that need no GPU -- the CPU
reference (tests/drift_hessian_reference.py) against Richardson-extrapolated central differences of the oracle's weighted gradient, the
proof on the oracle alone that the device cases of tests/drift_hvp_cases.py discriminate (every member carries a visible share of the
ensemble's product, and the ensemble is not the handle's own drift), the header / ctypes table / library export, the Julia wrapper,
and the argument errors of the Python surfaces, which are raised before the library is loaded."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_julia_shim import CTYPE, header, julia

import drift_hessian_reference as DR
import drift_hvp_cases as C
import hessian_reference as HR
from block_band_problem import block_band_problem

NAME = "jq_eval_f_g_grad_drifts_hvp"


@pytest.mark.parametrize("objFuncType", (1, 3))
def test_reference_matches_richardson_differences_of_the_weighted_oracle_gradient(jq, objFuncType):
    """Neumann order 24: the truncated series is converged, the gradient is smooth to rounding and the extrapolated differences
    (4 cd(h/2) - cd(h))/3, h = 1e-3/|d|, carry an error of O(h^4) plus rounding / h: the helper must agree to 1e-9 relative (the
    bound tests/test_hvp_host.py sets for its reference at the orders it uses is 1.2e-10; measured here: printed)."""
    rng = np.random.default_rng(7301 + objFuncType)
    s = C.Shape("rowlane", 10, 3, 2, 24, 0)
    p, pcof = block_band_problem(jq, rng, s.Ntot, s.N, 0, [1] * s.Nc, 7, s.m, objFuncType)
    H = C.member_drifts(rng, s, np.asarray(p.Hconst, dtype=np.float64), 3)
    w = np.array([0.45, 0.35, 0.2])
    d = rng.standard_normal(pcof.size)
    h = 1e-3 / np.linalg.norm(d)

    def cd(step):
        a, b = DR.weighted_oracle_gradients(p, pcof + step * d, H, w), DR.weighted_oracle_gradients(p, pcof - step * d, H, w)
        return [(x - y) / (2.0 * step) for x, y in zip(a, b)]

    r = DR.DriftHessianReference(p, H, w).hvp(pcof, d)
    half, full = cd(0.5 * h), cd(h)
    for name, mine, k in (("totalgrad", r["hv"], 0), ("infidelgrad", r["hv_infid"] if objFuncType != 1 else r["hv"], 1 if objFuncType != 1 else 0)):
        rich = (4.0 * half[k] - full[k]) / 3.0
        rel = np.linalg.norm(mine - rich) / np.linalg.norm(rich)
        print("type %d d(%s): helper vs Richardson differences, relative %.2e" % (objFuncType, name, rel))
        assert rel < 1e-9
    if objFuncType != 1:
        assert np.array_equal(r["hv_leak"], r["hv"] - r["hv_infid"])
    else:
        assert not r["hv_leak"].any() and np.array_equal(r["hv_infid"], r["hv"])


@pytest.mark.parametrize("objFuncType", C.OBJ_TYPES)
@pytest.mark.parametrize("s", C.SHAPES, ids=[C.shape_id(s) for s in C.SHAPES])
def test_device_cases_discriminate_on_the_oracle(jq, s, objFuncType):
    """what a wrong stream address would change is visible at the tolerance of the device tests: every member's w_i hv_i carries at
    least 0.01 of the norm of the ensemble's hv_infid, and the ensemble's product differs from the product of the problem's own drift
    alone by at least 1e-3 relative"""
    p, pcof, H, D, refs, members, _ = C.case(jq, s, objFuncType)
    own = HR.HessianReference(p)
    key = "hv_infid" if objFuncType != 1 else "hv"
    for j in range(C.NDIR):
        total = np.linalg.norm(refs[j]["hv_infid"])
        assert total > 0.0
        for i, (w, r) in enumerate(zip(C.WEIGHTS, members[j])):
            share = np.linalg.norm(w * r[key]) / total
            print("%s type %d direction %d member %d: |w hv| / |ensemble hv_infid| = %.3f" % (C.shape_id(s), objFuncType, j, i, share))
            assert share >= 0.01
        alone = own.hvp(pcof, D[:, j])[key]
        diff = np.linalg.norm(refs[j]["hv_infid"] - alone) / np.linalg.norm(alone)
        print("%s type %d direction %d: ensemble vs own drift alone, relative %.3e" % (C.shape_id(s), objFuncType, j, diff))
        assert diff >= 1e-3
    for i in range(H.shape[2]):      # (and the members are what the routes take: symmetric, inside the pattern -- member_drifts asserts the pattern)
        assert np.array_equal(H[:, :, i], H[:, :, i].T)


# ---- the C entry point -------------------------------------------------------------------------------------------------------------
ARGS = ["jq_handle *", "const double *", "int32_t", "const double *", "int32_t", "const double *", "const double *", "int32_t", "double *", "double *",
        "double *", "double *", "double *"]


def test_header_symbol_table_and_library_export_agree():
    from juqbox_jl_amd import _lib
    _, protos = header()
    assert NAME in protos
    ret, args = protos[NAME]
    assert ret == "int" and args == ARGS
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is ctypes.c_int
    dp, i32 = _lib.c_dp, _lib.c_i32
    assert argtypes == [ctypes.c_void_p, dp, i32, dp, i32, dp, dp, i32, dp, dp, dp, dp, dp]
    L = _lib.load()
    assert getattr(L, NAME) is not None
    assert L.jq_abi_version() == 6      # no layout change, no change of an existing entry point: the version stays


def test_null_handle_is_einval():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    z = lambda k: np.zeros(k)
    out2, ig, lg, hvi, hvl, pc, d, H, w = z(2), z(12), z(12), z(12), z(12), z(12), np.ones(12), z(16), np.ones(1)
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)
    assert L.jq_eval_f_g_grad_drifts_hvp(None, dp(pc), 12, dp(d), 1, dp(H), dp(w), 1, dp(out2), dp(ig), dp(lg), dp(hvi), dp(hvl)) == _lib.JQ_EINVAL
    assert not out2.any() and not ig.any() and not lg.any() and not hvi.any() and not hvl.any()


def test_julia_wrapper_and_its_ccall_match_the_header():
    _, protos = header()
    _, calls = julia()
    mine = [c for c in calls if c[0] == NAME]
    assert len(mine) == 1
    _, ret, args = mine[0]
    cret, cargs = protos[NAME]
    assert ret in CTYPE[cret]
    assert len(args) == len(cargs)
    for ct, jt in zip(cargs, args):
        assert jt in CTYPE[ct], (ct, jt)
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "hip_backend.jl")).read())
    assert re.search(r"function eval_f_g_grad_drifts_hvp\(pcof::Vector\{Float64\}, dirs::VecOrMat\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP,\s*"
                     r"Hconsts::Array\{Float64, 3\}, weights::Vector\{Float64\}\)", txt)


def test_documents_name_the_call():
    hdr = open(os.path.join(ROOT, "include", "juqbox_hip.h")).read()
    assert NAME in hdr and "JQ_ABI_VERSION 6" in hdr and '"drift_hvp"' in hdr
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc


# ---- the Python surfaces: argument errors before any library call ---------------------------------------------------------------------
class _NoLibrary:
    def __call__(self):
        raise AssertionError("the library was loaded before the arguments were checked")


class _Params:
    Ntot, N, objFuncType, tik0 = 4, 2, 3, 0.0


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


GOOD_H, GOOD_W = np.zeros((4, 4, 2)), np.ones(2)


@pytest.mark.parametrize("bad", [
    np.zeros(11), np.zeros((11, 3)), np.zeros((12, 0)), np.zeros((12, 2, 2)), [np.zeros(12), np.zeros(11)], np.full(12, np.nan), "direction",
], ids=["1d-wrong-length", "2d-wrong-rows", "zero-columns", "3d", "ragged", "nan", "string"])
def test_direction_errors_come_before_any_library_call(fake_wa, bad):
    jq, wa = fake_wa
    with pytest.raises(ValueError, match="eval_f_g_grad_drifts_hvp"):
        jq.eval_f_g_grad_drifts_hvp(np.zeros(12), bad, wa.params, wa, GOOD_H, GOOD_W)


@pytest.mark.parametrize("H,w", [
    (np.zeros((3, 4, 2)), np.ones(2)),         # members of the wrong shape
    (np.zeros((4, 4, 2, 1)), np.ones(2)),      # not a stack of matrices
    ([], np.ones(0)),                          # no member
    ([np.zeros((4, 4)), np.zeros((4, 3))], np.ones(2)),
    ("drifts", np.ones(1)),
    (np.zeros((4, 4, 2)), np.ones(3)),         # one weight per member
    (np.zeros((4, 4, 2)), np.ones((2, 1))),
    (np.zeros((4, 4, 2)), "weights"),
], ids=["wrong-shape", "4d", "empty", "ragged", "string", "weights-length", "weights-2d", "weights-string"])
def test_member_errors_come_before_any_library_call(fake_wa, H, w):
    jq, wa = fake_wa
    with pytest.raises(ValueError, match="eval_f_g_grad_drifts_hvp"):
        jq.eval_f_g_grad_drifts_hvp(np.zeros(12), np.zeros(12), wa.params, wa, H, w)
    with pytest.raises(ValueError, match="eval_f_g_grad_drifts_hvp"):
        jq.eval_hessvec_drifts(np.zeros(12), np.zeros(12), wa.params, wa, H, w)


def test_pcof_and_handle_errors_come_before_any_library_call(fake_wa):
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_drifts_hvp(np.zeros(11), np.zeros(12), wa.params, wa, GOOD_H, GOOD_W)
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_drifts_hvp("pcof", np.zeros(12), wa.params, wa, GOOD_H, GOOD_W)
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_drifts_hvp(np.zeros(12), np.zeros(12), _Params(), wa, GOOD_H, GOOD_W)      # another objparams
    with pytest.raises(TypeError):
        jq.eval_f_g_grad_drifts_hvp(np.zeros(12), np.zeros(12), wa.params, object(), GOOD_H, GOOD_W)
    with pytest.raises(TypeError):
        jq.eval_hessvec_drifts(np.zeros(12), np.zeros(12), wa.params, object(), GOOD_H, GOOD_W)
