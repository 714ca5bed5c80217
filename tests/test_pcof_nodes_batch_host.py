"""CPU: jq_eval_f_g_grad_batch (control vectors x the nodes of one ensemble in one call) through the layers that need no GPU -- header,
ctypes table and library export, the Julia method, the Python wrapper's shape checks (raised before the library is loaded), the documents."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_julia_shim import CTYPE, header, julia
from test_pcof_batch_host import fake_wa  # noqa: F401  (fixture: a Working_Arrays_HIP without a library behind it)

NAME = "jq_eval_f_g_grad_batch"


def test_header_symbol_table_and_library_export_agree():
    from juqbox_jl_amd import _lib
    _, protos = header()
    assert NAME in protos
    ret, args = protos[NAME]
    assert ret == "int"
    assert args == ["jq_handle *", "const double *", "int32_t", "int32_t", "const double *", "const double *", "int32_t", "const double *",
                    "int32_t", "double *", "double *", "double *", "double *"]
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is ctypes.c_int
    d, i = _lib.c_dp, _lib.c_i32
    assert argtypes == [ctypes.c_void_p, d, i, i, d, d, i, d, i, d, d, d, d]
    L = _lib.load()      # (every declared symbol must resolve: the export exists)
    assert getattr(L, NAME) is not None


def test_abi_version_stays_6():
    from juqbox_jl_amd import _lib
    assert _lib.load().jq_abi_version() == 6      # added like jq_traceobjgrad_batch: no layout change


def test_null_handle_is_einval():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    p = lambda a: a.ctypes.data_as(_lib.c_dp)
    out2, pc, nd, wt = np.zeros(2), np.zeros(12), np.zeros(1), np.ones(1)
    assert L.jq_eval_f_g_grad_batch(None, p(pc), 12, 1, p(nd), p(wt), 1, None, 0, p(out2), None, None, None) == _lib.JQ_EINVAL
    assert np.all(out2 == 0.0)


def test_julia_method_and_its_ccall_match_the_header():
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
    assert re.search(r"function eval_f_g_grad_batch\(pcofs::Matrix\{Float64\}, params::objparams, wa::AbstractWorkingArraysHIP,\s*nodes::AbstractArray,"
                     r"\s*weights::AbstractArray, compute_adjoint::Bool = true; shift = nothing, per_node::Bool = false\)", txt)


@pytest.mark.parametrize("pcofs, nodes, weights", [
    (np.zeros((12, 2)), [0.0, 0.1], [1.0]),                 # nodes and weights of different lengths
    (np.zeros((12, 2)), [0.0, 0.1], [0.2, 0.3, 0.5]),
    (np.zeros((12, 2)), [], []),                            # no node at all
    (np.zeros((12, 2)), np.zeros((2, 2)), np.zeros((2, 2))),    # not vectors
    (np.zeros((12, 0)), [0.0], [1.0]),                      # an empty pcofs
    ([], [0.0], [1.0]),                                     # ... as a sequence
    (np.zeros((11, 2)), [0.0], [1.0]),                      # columns of the wrong length
    ([np.zeros(12), np.zeros(11)], [0.0], [1.0]),           # ragged
], ids=["fewer-weights", "more-weights", "no-nodes", "2d-nodes", "zero-columns", "empty-list", "wrong-rows", "ragged"])
def test_wrapper_shape_errors_come_before_any_library_call(fake_wa, pcofs, nodes, weights):  # noqa: F811
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_batch(pcofs, wa.params, wa, nodes, weights)
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_batch(pcofs, wa.params, wa, nodes, weights, False, per_node=True)


def test_wrapper_refuses_foreign_working_arrays(fake_wa):  # noqa: F811
    jq, wa = fake_wa
    with pytest.raises(ValueError):
        jq.eval_f_g_grad_batch(np.zeros((12, 2)), object(), wa, [0.0], [1.0])
    with pytest.raises(TypeError):
        jq.eval_f_g_grad_batch(np.zeros((12, 2)), wa.params, object(), [0.0], [1.0])


def test_exported_next_to_traceobjgrad_batch_and_leaves_the_memo_alone():
    import juqbox_jl_amd as jq
    assert callable(jq.eval_f_g_grad_batch) and callable(jq.traceobjgrad_batch)
    assert "last_" in jq.eval_f_g_grad_batch.__doc__


def test_documents_name_the_entry():
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        txt = open(os.path.join(ROOT, doc)).read()
        assert "eval_f_g_grad_batch" in txt, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "in one call do not exist" not in design
    assert "nodes_per_vector" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
