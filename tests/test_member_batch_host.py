"""CPU: jq_traceobjgrad_members / jq_eval_f_g_grad_members (one control vector over members that differ in a real mixing matrix of the
controls, in their drift, or in both) through the layers that need no GPU -- header, ctypes table and library export, the Julia methods, the
Python wrappers' shape checks (raised before the library is loaded), amplitude_mix, setup_ipopt_problem's keyword rules, the documents."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_julia_shim import CTYPE, header, julia

NAMES = ("jq_traceobjgrad_members", "jq_eval_f_g_grad_members")


def test_header_symbol_table_and_library_export_agree():
    from juqbox_jl_amd import _lib
    _, protos = header()
    dp, i32 = _lib.c_dp, _lib.c_i32
    want = {
        "jq_traceobjgrad_members": (["jq_handle *", "const double *", "int32_t", "const double *", "const double *", "int32_t", "int32_t", "double *", "double *", "double *",
                                     "double *"], [ctypes.c_void_p, dp, i32, dp, dp, i32, i32, dp, dp, dp, dp]),
        "jq_eval_f_g_grad_members": (["jq_handle *", "const double *", "int32_t", "const double *", "const double *", "const double *", "int32_t", "int32_t", "double *",
                                      "double *", "double *", "double *"], [ctypes.c_void_p, dp, i32, dp, dp, dp, i32, i32, dp, dp, dp, dp]),
    }
    L = _lib.load()      # (every declared symbol must resolve: the exports exist)
    for name in NAMES:
        assert name in protos and name in _lib.SYMBOLS
        ret, args = protos[name]
        assert ret == "int" and args == want[name][0], (name, args)
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is ctypes.c_int and argtypes == want[name][1], name
        assert getattr(L, name) is not None
    assert L.jq_abi_version() == 6      # symbols only: no layout change, the version stays


def test_null_handle_is_einval():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    ptr = lambda a: a.ctypes.data_as(_lib.c_dp)
    out4, out2, pc, C, w = np.zeros(4), np.zeros(2), np.zeros(12), np.ones(1), np.ones(1)
    assert L.jq_traceobjgrad_members(None, ptr(pc), 12, None, ptr(C), 1, 0, ptr(out4), None, None, None) == _lib.JQ_EINVAL
    assert L.jq_eval_f_g_grad_members(None, ptr(pc), 12, None, ptr(C), ptr(w), 1, 0, ptr(out2), None, None, None) == _lib.JQ_EINVAL
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
    mats = r"Hconsts::Union\{Nothing,Array\{Float64,3\}\}, ctrl_mix::Union\{Nothing,Array\{Float64,3\}\}"
    assert re.search(r"function traceobjgrad_members\(pcof::Vector\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP,\s*" + mats +
                     r",\s*evaladjoint::Bool = true\)", txt)
    assert re.search(r"function eval_f_g_grad_members!\(pcof::Vector\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP,\s*" + mats +
                     r",\s*weights::AbstractArray, compute_adjoint::Bool = true; per_member::Bool = false\)", txt)
    assert re.search(r"const JQ_ABI_VERSION = 6\b", txt)


class _NoLibrary:
    """stands in for juqbox_jl_amd._lib.load while the wrappers' argument checks run: any library call fails the test"""

    def __call__(self):
        raise AssertionError("the library was loaded before the shapes were checked")


class _Params:
    Ntot = 4
    Ncoupled = 2
    Nunc = 0
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


BAD_MIXES = [
    ([np.zeros((2, 3)), np.zeros((2, 3))], "non-square"),
    (np.zeros((2, 3, 2)), "non-square-array"),
    ([np.eye(3)], "wrong-Nc"),
    (np.zeros((3, 3, 2)), "wrong-Nc-array"),
    ([], "empty-list"),
    (np.zeros((2, 2, 0)), "empty-array"),
    ([np.eye(2), np.zeros((2, 3))], "ragged"),
    (np.zeros((2, 2, 2, 2)), "4d"),
    ([np.array([[1.0, float("nan")], [0.0, 1.0]])], "nan"),
    ([np.array([[1.0, 0.0], [float("inf"), 1.0]])], "inf"),
    ([np.eye(2) * (1.0 + 0.1j)], "complex"),
]


@pytest.mark.parametrize("bad", [b for b, _ in BAD_MIXES], ids=[i for _, i in BAD_MIXES])
def test_wrapper_shape_errors_come_before_any_library_call(fake_wa, bad):
    jq, wa = fake_wa
    n = len(bad) if isinstance(bad, list) else (bad.shape[2] if bad.ndim >= 3 else 1)
    w = np.ones(max(n, 1)) / max(n, 1)
    with pytest.raises(ValueError):
        jq.traceobjgrad_members(np.zeros(12), wa.params, wa, ctrl_mix=bad)
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_members(np.zeros(12), wa.params, wa, w, ctrl_mix=bad)
    with pytest.raises(ValueError):
        jq.setup_ipopt_problem(wa.params, wa, 12, -np.ones(12), np.ones(12), ctrl_mix=bad, member_weights=w)


def test_neither_drifts_nor_mixes_and_unequal_counts_are_value_errors(fake_wa):
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.traceobjgrad_members(np.zeros(12), wa.params, wa)
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_members(np.zeros(12), wa.params, wa, np.ones(1))
    mixes, drifts = np.zeros((2, 2, 3)), np.zeros((4, 4, 2))
    with pytest.raises(ValueError):
        jq.traceobjgrad_members(np.zeros(12), wa.params, wa, Hconsts=drifts, ctrl_mix=mixes)
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_members(np.zeros(12), wa.params, wa, np.ones(3), Hconsts=drifts, ctrl_mix=mixes)
    with pytest.raises(ValueError):      # (a member drift of the wrong size)
        jq.traceobjgrad_members(np.zeros(12), wa.params, wa, Hconsts=np.zeros((5, 5, 3)), ctrl_mix=mixes)


@pytest.mark.parametrize("weights", [np.ones(2), np.ones(4), np.ones((3, 1)), []], ids=["short", "long", "2d", "empty"])
def test_weights_length_must_be_the_member_count(fake_wa, weights):
    jq, wa = fake_wa
    mixes = np.zeros((2, 2, 3))
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_members(np.zeros(12), wa.params, wa, weights, ctrl_mix=mixes)
    with pytest.raises(ValueError):
        jq.setup_ipopt_problem(wa.params, wa, 12, -np.ones(12), np.ones(12), ctrl_mix=mixes, member_weights=weights)


def test_wrong_coefficient_count_is_a_value_error(fake_wa):
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.traceobjgrad_members(np.zeros(11), wa.params, wa, ctrl_mix=np.zeros((2, 2, 2)))
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_members(np.zeros(11), wa.params, wa, np.ones(2), ctrl_mix=np.zeros((2, 2, 2)))


def test_setup_keyword_rules(fake_wa):
    jq, wa = fake_wa
    setup = lambda **kw: jq.setup_ipopt_problem(wa.params, wa, 12, -np.ones(12), np.ones(12), **kw)
    mixes, drifts, w = np.stack([np.eye(2)] * 3, axis=2), np.zeros((4, 4, 3)), np.ones(3) / 3
    with pytest.raises(ValueError):      # both weight keywords
        setup(ctrl_mix=mixes, member_weights=w, drift_weights=w)
    with pytest.raises(ValueError):
        setup(drifts=drifts, ctrl_mix=mixes, member_weights=w, drift_weights=w)
    with pytest.raises(ValueError):      # mixes without weights, weights without members
        setup(ctrl_mix=mixes)
    with pytest.raises(ValueError):
        setup(member_weights=w)
    with pytest.raises(ValueError):      # drifts and mixes of different member counts
        setup(drifts=np.zeros((4, 4, 2)), ctrl_mix=mixes, member_weights=w)
    wa.params.quiet = True
    # accepted: mixes alone, drifts and mixes with ONE weight vector under either keyword, drifts as before (with either keyword)
    for kw in (dict(ctrl_mix=mixes, member_weights=w), dict(drifts=drifts, ctrl_mix=mixes, member_weights=w),
               dict(drifts=drifts, ctrl_mix=mixes, drift_weights=w), dict(drifts=drifts, drift_weights=w), dict(drifts=drifts, member_weights=w)):
        prob = setup(**kw)
        assert prob.nCoeff == 12


def test_amplitude_mix_shapes():
    import juqbox_jl_amd as jq
    s = 1.0 + 0.05 * np.random.default_rng(3).standard_normal((4, 3))
    C = jq.amplitude_mix(s)
    assert C.shape == (3, 3, 4)
    for i in range(4):
        assert np.array_equal(C[:, :, i], np.diag(s[i]))
    one = jq.amplitude_mix([1.0, 0.9])
    assert one.shape == (2, 2, 1) and np.array_equal(one[:, :, 0], np.diag([1.0, 0.9]))
    for bad in (np.zeros((2, 2, 2)), np.zeros((0, 3)), np.zeros((3, 0)), 1.0, "x"):
        with pytest.raises(ValueError):
            jq.amplitude_mix(bad)


def test_wrapper_accepts_arrays_and_sequences_alike():
    from juqbox_jl_amd.evalobjgrad import _mix_members
    rng = np.random.default_rng(7)
    A = rng.standard_normal((2, 2, 3))
    a = _mix_members(A, 2, "t")
    b = _mix_members([A[:, :, i].copy() for i in range(3)], 2, "t")
    c = _mix_members(np.asfortranarray(A), 2, "t")
    assert a.shape == (3, 4) and a.flags["C_CONTIGUOUS"]
    for i in range(3):
        assert np.array_equal(a[i], A[:, :, i].ravel(order="F"))      # element (l, k) of member i at l + Nc k: the C ABI's Nc x Nc x nmember
    assert np.array_equal(b, a) and np.array_equal(c, a)
    assert np.array_equal(_mix_members(A[:, :, 0], 2, "t"), a[:1])


def test_documents_name_the_calls():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        txt = open(os.path.join(ROOT, doc)).read()
        assert "jq_traceobjgrad_members" in txt, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "member_batch" in design and "crosstalk" in design and "amplitude" in design
    hdr = open(os.path.join(ROOT, "include", "juqbox_hip.h")).read()
    assert "ctrl_mix" in hdr and "member_batch" in hdr
