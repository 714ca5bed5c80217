"""CPU: Hessian-vector products of a member ensemble with control mixes (jq_eval_f_g_grad_members_hvp) through the layers that need no
GPU -- the CPU reference (tests/member_hvp_cases.py: the mixed problems through tests/hessian_reference.py) against Richardson-
extrapolated central differences of the oracle's weighted gradient, the proof on the oracle alone that the device cases discriminate
(every member carries a visible share, the mixes are visible against identity mixes, a mix belongs to its member and is not its
transpose), the header / ctypes table / library export, the Julia wrapper, and the argument errors of the Python surfaces, which are
raised before the library is loaded."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_julia_shim import CTYPE, header, julia

import drift_hvp_cases as DC
import member_hvp_cases as C
from block_band_problem import block_band_problem

NAME = "jq_eval_f_g_grad_members_hvp"


@pytest.mark.parametrize("objFuncType", (1, 3))
def test_reference_matches_richardson_differences_of_the_weighted_oracle_gradient(jq, objFuncType):
    """Neumann order 24: the truncated series is converged, the gradient is smooth to rounding and the extrapolated differences
    (4 cd(h/2) - cd(h))/3, h = 1e-3/|d|, carry an error of O(h^4) plus rounding / h: the reference must agree to 1e-9 relative, the
    bound of tests/test_drift_hvp_host.py (measured here: printed)."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(7401 + objFuncType)
    s = C.Shape("rowlane", 10, 3, 2, 24, 0)
    p, pcof = block_band_problem(jq, rng, s.Ntot, s.N, 0, [1] * s.Nc, 7, s.m, objFuncType)
    H = C.member_drifts(rng, s, np.asarray(p.Hconst, dtype=np.float64), 3)
    Cm = C.member_mixes(s)
    w = np.array([0.45, 0.35, 0.2])
    d = rng.standard_normal(pcof.size)
    h = 1e-3 / np.linalg.norm(d)
    probs = [C.mixed_params(p, Cm[:, :, i], H[:, :, i]) for i in range(3)]

    def grads(x):
        rs = [Oracle(q).traceobjgrad(x) for q in probs]
        return [sum(wi * r[k] for wi, r in zip(w, rs)) for k in ("totalgrad", "infidelgrad")]

    def cd(step):
        return [(x - y) / (2.0 * step) for x, y in zip(grads(pcof + step * d), grads(pcof - step * d))]

    refs, _, _ = C.reference(p, pcof, d[:, None], Cm, H, w)
    r = refs[0]
    half, full = cd(0.5 * h), cd(h)
    for name, mine, k in (("totalgrad", r["hv"], 0), ("infidelgrad", r["hv_infid"] if objFuncType != 1 else r["hv"], 1 if objFuncType != 1 else 0)):
        rich = (4.0 * half[k] - full[k]) / 3.0
        rel = np.linalg.norm(mine - rich) / np.linalg.norm(rich)
        print("type %d d(%s): reference vs Richardson differences, relative %.2e" % (objFuncType, name, rel))
        assert rel < 1e-9
    if objFuncType != 1:
        assert np.array_equal(r["hv_leak"], r["hv"] - r["hv_infid"])
    else:
        assert not r["hv_leak"].any() and np.array_equal(r["hv_infid"], r["hv"])


@pytest.mark.parametrize("objFuncType", C.OBJ_TYPES)
@pytest.mark.parametrize("s", C.SHAPES, ids=[C.shape_id(s) for s in C.SHAPES])
def test_device_cases_discriminate_on_the_oracle(jq, s, objFuncType):
    """what a wrong stream, a wrong mix table entry or a transposed mix would change is visible at the tolerance of the device tests:
    every member's w_i hv_i carries at least 0.01 of the norm of the ensemble's product, and the product differs by at least 1e-3
    relative from that of the same ensemble with identity mixes, with the mixes of members 0 and 1 swapped, and (Nc >= 2) with every
    mix transposed"""
    p, pcof, H, Cm, D, refs, members, _ = C.case(jq, s, objFuncType)
    key = "hv_infid" if objFuncType != 1 else "hv"
    identity = DC.case(jq, s, objFuncType)[4]      # (the drift ensemble of tests/drift_hvp_cases.py: the same members without mixes)
    swapped, _, _ = C.reference(p, pcof, D, np.asfortranarray(Cm[:, :, [1, 0, 2]]), H, C.WEIGHTS)
    variants = [("identity mixes", identity), ("mixes of members 0 and 1 swapped", swapped)]
    if s.Nc >= 2:
        variants.append(("every mix transposed", C.reference(p, pcof, D, np.asfortranarray(Cm.transpose(1, 0, 2)), H, C.WEIGHTS)[0]))
    for j in range(C.NDIR):
        total = np.linalg.norm(refs[j]["hv_infid"])
        assert total > 0.0
        for i, (w, r) in enumerate(zip(C.WEIGHTS, members[j])):
            share = np.linalg.norm(w * r[key]) / total
            print("%s type %d direction %d member %d: |w hv| / |ensemble hv_infid| = %.3f" % (C.shape_id(s), objFuncType, j, i, share))
            assert share >= 0.01
        for what, other in variants:
            diff = np.linalg.norm(refs[j]["hv_infid"] - other[j]["hv_infid"]) / np.linalg.norm(other[j]["hv_infid"])
            print("%s type %d direction %d: ensemble vs %s, relative %.3e" % (C.shape_id(s), objFuncType, j, what, diff))
            assert diff >= 1e-3


def test_the_mixes_are_the_stated_draws():
    for s in C.SHAPES:
        Cm = C.member_mixes(s)
        rng = np.random.default_rng(71000 + 1000 * s.Ntot + 100 * s.N + 10 * s.Nc + s.m)
        assert Cm.shape == (s.Nc, s.Nc, 3)
        for i in range(3):
            assert np.array_equal(Cm[:, :, i], np.eye(s.Nc) + 0.05 * rng.standard_normal((s.Nc, s.Nc)))


# ---- the C entry point -------------------------------------------------------------------------------------------------------------
ARGS = ["jq_handle *", "const double *", "int32_t", "const double *", "int32_t", "const double *", "const double *", "const double *", "int32_t",
        "double *", "double *", "double *", "double *", "double *"]


def test_header_symbol_table_and_library_export_agree():
    from juqbox_jl_amd import _lib
    _, protos = header()
    assert NAME in protos
    ret, args = protos[NAME]
    assert ret == "int" and args == ARGS
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is ctypes.c_int
    dp, i32 = _lib.c_dp, _lib.c_i32
    assert argtypes == [ctypes.c_void_p, dp, i32, dp, i32, dp, dp, dp, i32, dp, dp, dp, dp, dp]
    L = _lib.load()
    assert getattr(L, NAME) is not None
    assert L.jq_abi_version() == 6      # a new symbol only: the version stays


def test_null_handle_is_einval():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    z = lambda k: np.zeros(k)
    out2, ig, lg, hvi, hvl, pc, d, H, Cm, w = z(2), z(12), z(12), z(12), z(12), z(12), np.ones(12), z(16), np.ones(1), np.ones(1)
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)
    rc = L.jq_eval_f_g_grad_members_hvp(None, dp(pc), 12, dp(d), 1, dp(H), dp(Cm), dp(w), 1, dp(out2), dp(ig), dp(lg), dp(hvi), dp(hvl))
    assert rc == _lib.JQ_EINVAL
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
    assert re.search(r"function eval_f_g_grad_members_hvp\(pcof::Vector\{Float64\}, dirs::VecOrMat\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP,\s*"
                     r"Hconsts::Union\{Nothing,Array\{Float64,3\}\}, ctrl_mix::Union\{Nothing,Array\{Float64,3\}\}, weights::Vector\{Float64\}\)", txt)


def test_documents_name_the_call_and_its_plan_record():
    hdr = open(os.path.join(ROOT, "include", "juqbox_hip.h")).read()
    assert NAME in hdr and "JQ_ABI_VERSION 6" in hdr and '"member_hvp"' in hdr
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc


# ---- the Python surfaces: argument errors before any library call ---------------------------------------------------------------------
class _NoLibrary:
    def __call__(self):
        raise AssertionError("the library was loaded before the arguments were checked")


class _Params:
    Ntot, N, objFuncType, tik0, Ncoupled, Nunc = 4, 2, 3, 0.0, 2, 0


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


GOOD_H, GOOD_C, GOOD_W = np.zeros((4, 4, 2)), np.stack([np.eye(2)] * 2, axis=2), np.ones(2)


@pytest.mark.parametrize("bad", [
    np.zeros(11), np.zeros((11, 3)), np.zeros((12, 0)), np.zeros((12, 2, 2)), [np.zeros(12), np.zeros(11)], np.full(12, np.nan), "direction",
], ids=["1d-wrong-length", "2d-wrong-rows", "zero-columns", "3d", "ragged", "nan", "string"])
def test_direction_errors_come_before_any_library_call(fake_wa, bad):
    jq, wa = fake_wa
    with pytest.raises(ValueError, match="eval_f_g_grad_members_hvp"):
        jq.eval_f_g_grad_members_hvp(np.zeros(12), bad, wa.params, wa, GOOD_W, GOOD_H, GOOD_C)


@pytest.mark.parametrize("H,Cm,w", [
    (None, None, np.ones(2)),                                      # neither drifts nor mixes: the plain problem
    (np.zeros((3, 4, 2)), GOOD_C, np.ones(2)),                     # drifts of the wrong shape
    (np.zeros((4, 4, 2, 1)), None, np.ones(2)),
    ([], None, np.ones(0)),                                        # no member
    (GOOD_H, np.zeros((3, 3, 2)), np.ones(2)),                     # mixes of the wrong shape
    (None, np.zeros((2, 2, 2, 1)), np.ones(2)),
    (None, [np.eye(2), np.zeros((2, 3))], np.ones(2)),
    (None, "mixes", np.ones(1)),
    (np.zeros((4, 4, 3)), GOOD_C, np.ones(3)),                     # three drifts, two mixes
    (GOOD_H, GOOD_C, np.ones(3)),                                  # one weight per member
    (None, GOOD_C, np.ones((2, 1))),
    (GOOD_H, None, "weights"),
], ids=["neither", "drift-shape", "drift-4d", "empty", "mix-shape", "mix-4d", "mix-ragged", "mix-string", "counts-differ", "weights-length",
        "weights-2d", "weights-string"])
def test_member_errors_come_before_any_library_call(fake_wa, H, Cm, w):
    jq, wa = fake_wa
    with pytest.raises(ValueError, match="eval_f_g_grad_members_hvp"):
        jq.eval_f_g_grad_members_hvp(np.zeros(12), np.zeros(12), wa.params, wa, w, Hconsts=H, ctrl_mix=Cm)
    with pytest.raises(ValueError, match="eval_f_g_grad_members_hvp"):
        jq.eval_hessvec_members(np.zeros(12), np.zeros(12), wa.params, wa, w, Hconsts=H, ctrl_mix=Cm)


def test_pcof_and_handle_errors_come_before_any_library_call(fake_wa):
    jq, wa = fake_wa
    with pytest.raises(ValueError, match="eval_f_g_grad_members_hvp"):
        jq.eval_f_g_grad_members_hvp(np.zeros(11), np.zeros(12), wa.params, wa, GOOD_W, GOOD_H, GOOD_C)
    with pytest.raises(ValueError, match="eval_f_g_grad_members_hvp"):
        jq.eval_f_g_grad_members_hvp("pcof", np.zeros(12), wa.params, wa, GOOD_W, GOOD_H, GOOD_C)
    with pytest.raises(ValueError, match="eval_f_g_grad_members_hvp"):
        jq.eval_f_g_grad_members_hvp(np.zeros(12), np.zeros(12), _Params(), wa, GOOD_W, GOOD_H, GOOD_C)      # another objparams
    with pytest.raises(TypeError):
        jq.eval_f_g_grad_members_hvp(np.zeros(12), np.zeros(12), wa.params, object(), GOOD_W, GOOD_H, GOOD_C)
    with pytest.raises(TypeError):
        jq.eval_hessvec_members(np.zeros(12), np.zeros(12), wa.params, object(), GOOD_W, GOOD_H, GOOD_C)
