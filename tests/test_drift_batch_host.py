"""CPU: jq_traceobjgrad_drifts / jq_eval_f_g_grad_drifts (one control vector over an ensemble of drift Hamiltonians in one call) through the
layers that need no GPU -- header, ctypes table and library export, the Julia methods, the Python wrappers' shape checks (raised before
the library is loaded), the documents."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_julia_shim import CTYPE, header, julia

NAMES = ("jq_traceobjgrad_drifts", "jq_eval_f_g_grad_drifts")


def test_header_symbol_table_and_library_export_agree():
    from juqbox_jl_amd import _lib
    _, protos = header()
    dp, i32 = _lib.c_dp, _lib.c_i32
    want = {
        "jq_traceobjgrad_drifts": (["jq_handle *", "const double *", "int32_t", "const double *", "int32_t", "int32_t", "double *", "double *", "double *", "double *"],
                                   [ctypes.c_void_p, dp, i32, dp, i32, i32, dp, dp, dp, dp]),
        "jq_eval_f_g_grad_drifts": (["jq_handle *", "const double *", "int32_t", "const double *", "const double *", "int32_t", "int32_t", "double *", "double *", "double *", "double *"],
                                    [ctypes.c_void_p, dp, i32, dp, dp, i32, i32, dp, dp, dp, dp]),
    }
    L = _lib.load()      # (every declared symbol must resolve: the exports exist)
    for name in NAMES:
        assert name in protos and name in _lib.SYMBOLS
        ret, args = protos[name]
        assert ret == "int" and args == want[name][0], (name, args)
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is ctypes.c_int and argtypes == want[name][1], name
        assert getattr(L, name) is not None
    assert L.jq_abi_version() == 6      # added like the two batch calls: no layout change, the version stays


def test_null_handle_is_einval():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
    out4, out2, pc, H, w = np.zeros(4), np.zeros(2), np.zeros(12), np.zeros(16), np.ones(1)
    assert L.jq_traceobjgrad_drifts(None, ptr(pc), 12, ptr(H), 1, 0, ptr(out4), None, None, None) == _lib.JQ_EINVAL
    assert L.jq_eval_f_g_grad_drifts(None, ptr(pc), 12, ptr(H), ptr(w), 1, 0, ptr(out2), None, None, None) == _lib.JQ_EINVAL
    assert np.all(out4 == 0.0) and np.all(out2 == 0.0)


def test_julia_methods_and_their_ccalls_match_the_header():
    _, protos = header()
    _, calls = julia()
    for name in NAMES:
        mine = [c for c in calls if c[0] == name]
        assert len(mine) == 1, name
        _, ret, args = mine[0]
        cret, cargs = protos[name]
        assert ret in CTYPE[cret]
        assert len(args) == len(cargs)
        for ct, jt in zip(cargs, args):
            assert jt in CTYPE[ct], (name, ct, jt)
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "hip_backend.jl")).read())
    assert re.search(r"function traceobjgrad_drifts\(pcof::Vector\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP, Hconsts::Array\{Float64,3\},\s*evaladjoint::Bool = true\)", txt)
    assert re.search(r"function eval_f_g_grad_drifts!\(pcof::Vector\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP, Hconsts::Array\{Float64,3\},\s*"
                     r"weights::AbstractArray, compute_adjoint::Bool = true; per_member::Bool = false\)", txt)
    assert re.search(r"const JQ_ABI_VERSION = 6\b", txt)


class _NoLibrary:
    """stands in for juqbox_jl_amd._lib.load while the wrappers' argument checks run: any library call fails the test"""

    def __call__(self):
        raise AssertionError("the library was loaded before the shapes were checked")


class _Params:
    Ntot = 4
    objFuncType = 1


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


BAD_MEMBERS = [
    ([np.zeros((4, 3)), np.zeros((4, 3))], "non-square"),
    (np.zeros((4, 3, 2)), "non-square-array"),
    ([np.zeros((5, 5))], "wrong-Ntot"),
    (np.zeros((5, 5, 2)), "wrong-Ntot-array"),
    ([], "empty-list"),
    (np.zeros((4, 4, 0)), "empty-array"),
    ([np.zeros((4, 4)), np.zeros((4, 5))], "ragged"),
    (np.zeros((4, 4, 2, 2)), "4d"),
]


@pytest.mark.parametrize("bad", [b for b, _ in BAD_MEMBERS], ids=[i for _, i in BAD_MEMBERS])
def test_wrapper_shape_errors_come_before_any_library_call(fake_wa, bad):
    jq, wa = fake_wa
    n = len(bad) if isinstance(bad, list) else (bad.shape[2] if bad.ndim >= 3 else 1)
    with pytest.raises(ValueError):
        jq.traceobjgrad_drifts(np.zeros(12), wa.params, wa, bad, True)
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_drifts(np.zeros(12), wa.params, wa, bad, np.ones(max(n, 1)) / max(n, 1), True)
    with pytest.raises(ValueError):
        jq.setup_ipopt_problem(wa.params, wa, 12, -np.ones(12), np.ones(12), drifts=bad, drift_weights=np.ones(max(n, 1)) / max(n, 1))


@pytest.mark.parametrize("weights", [np.ones(2), np.ones(4), np.ones((3, 1)), []], ids=["short", "long", "2d", "empty"])
def test_weights_length_must_be_the_member_count(fake_wa, weights):
    jq, wa = fake_wa
    members = np.zeros((4, 4, 3))
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_drifts(np.zeros(12), wa.params, wa, members, weights, True)
    with pytest.raises(ValueError):
        jq.setup_ipopt_problem(wa.params, wa, 12, -np.ones(12), np.ones(12), drifts=members, drift_weights=weights)


def test_setup_needs_both_or_neither(fake_wa):
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.setup_ipopt_problem(wa.params, wa, 12, -np.ones(12), np.ones(12), drifts=np.zeros((4, 4, 2)))
    with pytest.raises(ValueError):
        jq.setup_ipopt_problem(wa.params, wa, 12, -np.ones(12), np.ones(12), drift_weights=np.ones(2))


def test_wrong_coefficient_count_is_a_value_error(fake_wa):
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.traceobjgrad_drifts(np.zeros(11), wa.params, wa, np.zeros((4, 4, 2)), True)
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_drifts(np.zeros(11), wa.params, wa, np.zeros((4, 4, 2)), np.ones(2), True)


def test_wrapper_accepts_arrays_and_sequences_alike():
    from juqbox_jl_amd.evalobjgrad import _drift_members
    rng = np.random.default_rng(7)
    A = rng.standard_normal((4, 4, 3))
    a = _drift_members(A, 4, "t")
    b = _drift_members([A[:, :, i].copy() for i in range(3)], 4, "t")
    c = _drift_members(np.asfortranarray(A), 4, "t")
    assert a.shape == (3, 16) and a.flags["C_CONTIGUOUS"]
    for i in range(3):
        assert np.array_equal(a[i], A[:, :, i].ravel(order="F"))      # member i column-major: the C ABI's Ntot x Ntot x ndrift
    assert np.array_equal(b, a) and np.array_equal(c, a)
    assert np.array_equal(_drift_members(A[:, :, 0], 4, "t"), a[:1])


def test_documents_name_the_calls():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        txt = open(os.path.join(ROOT, doc)).read()
        assert "jq_traceobjgrad_drifts" in txt, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "drift_batch" in design and "union" in design
