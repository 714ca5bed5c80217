"""CPU: jq_traceobjgrad_batch (many control vectors of one problem in one call) through the layers that need no GPU -- header, ctypes
table and library export, the Julia method, the Python wrapper's shape checks (raised before the library is loaded), the option row."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_julia_shim import CTYPE, header, julia


def test_header_symbol_table_and_library_export_agree():
    from juqbox_jl_amd import _lib
    _, protos = header()
    assert "jq_traceobjgrad_batch" in protos
    ret, args = protos["jq_traceobjgrad_batch"]
    assert ret == "int"
    assert args == ["jq_handle *", "const double *", "int32_t", "int32_t", "int32_t", "double *", "double *", "double *", "double *"]
    restype, argtypes = _lib.SYMBOLS["jq_traceobjgrad_batch"]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, _lib.c_dp, _lib.c_i32, _lib.c_i32, _lib.c_i32, _lib.c_dp, _lib.c_dp, _lib.c_dp, _lib.c_dp]
    L = _lib.load()      # (every declared symbol must resolve: the export exists)
    assert L.jq_traceobjgrad_batch is not None
    assert L.jq_abi_version() == 6      # added like jq_s_uniform: no layout change, the version stays


def test_null_handle_is_einval():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    out4 = np.zeros(4)
    pc = np.zeros(12)
    assert L.jq_traceobjgrad_batch(None, pc.ctypes.data_as(_lib.c_dp), 12, 1, 0, out4.ctypes.data_as(_lib.c_dp), None, None, None) == _lib.JQ_EINVAL
    assert np.all(out4 == 0.0)


def test_julia_method_and_its_ccall_match_the_header():
    _, protos = header()
    _, calls = julia()
    mine = [c for c in calls if c[0] == "jq_traceobjgrad_batch"]
    assert len(mine) == 1
    _, ret, args = mine[0]
    cret, cargs = protos["jq_traceobjgrad_batch"]
    assert ret in CTYPE[cret]
    assert len(args) == len(cargs)
    for ct, jt in zip(cargs, args):
        assert jt in CTYPE[ct], (ct, jt)
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "hip_backend.jl")).read())
    assert re.search(r"function traceobjgrad_batch\(pcofs::Matrix\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP,\s*evaladjoint::Bool = true\)", txt)


class _NoLibrary:
    """stands in for juqbox_jl_amd._lib.load while the wrapper's argument checks run: any library call fails the test"""

    def __call__(self):
        raise AssertionError("the library was loaded before the shapes were checked")


@pytest.fixture
def fake_wa(monkeypatch):
    import juqbox_jl_amd as jq
    from juqbox_jl_amd import _lib, evalobjgrad
    monkeypatch.setattr(_lib, "load", _NoLibrary())
    wa = object.__new__(evalobjgrad.Working_Arrays_HIP)
    wa.handle = None
    wa.nCoeff = 12
    wa.params = object()
    return jq, wa


@pytest.mark.parametrize("bad", [
    [np.zeros(12), np.zeros(11)],          # ragged list
    [[0.0] * 12, [0.0] * 13],              # ... of plain lists
    np.zeros(11),                          # one vector of the wrong length
    np.zeros((11, 3)),                     # columns of the wrong length
    np.zeros((12, 0)),                     # zero vectors
    [],                                    # ... as a sequence
    np.zeros((12, 2, 2)),                  # not a matrix
], ids=["ragged", "ragged-lists", "1d-wrong-length", "2d-wrong-rows", "zero-columns", "empty-list", "3d"])
def test_wrapper_shape_errors_come_before_any_library_call(fake_wa, bad):
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.traceobjgrad_batch(bad, wa.params, wa, True)


def test_gradient_check_argument_errors_come_before_any_library_call(fake_wa):
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.gradient_check(np.zeros(11), wa.params, wa, [0])
    with pytest.raises(ValueError):
        jq.gradient_check(np.zeros(12), wa.params, wa, [12])


def test_wrapper_accepts_columns_and_sequences_alike():
    from juqbox_jl_amd.evalobjgrad import _pcof_columns
    rng = np.random.default_rng(5)
    M = rng.standard_normal((12, 3))
    a = _pcof_columns(M, 12)
    b = _pcof_columns([M[:, i].copy() for i in range(3)], 12)
    c = _pcof_columns(np.asfortranarray(M), 12)
    assert a.shape == (3, 12) and a.flags["C_CONTIGUOUS"]
    assert np.array_equal(a, M.T) and np.array_equal(b, a) and np.array_equal(c, a)
    assert np.array_equal(_pcof_columns(M[:, 0], 12), M[:, :1].T)


def test_the_refused_self_check_names_its_stand_in():
    import juqbox_jl_amd as jq
    assert "gradient_check" in jq.traceobjgrad.__doc__
    assert "verbose" in jq.gradient_check.__doc__


def test_option_row_in_integration_md():
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"^\| `pcof_batch_max` \| not set \| per evaluation \| .*control vectors per launch", txt, flags=re.M)
    assert "jq_traceobjgrad_batch" in txt
