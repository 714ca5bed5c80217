"""CPU: sample tables over member ensembles and in batches (jq_traceobjgrad_samples_batch, jq_traceobjgrad_samples_members,
jq_eval_f_g_grad_samples_members) -- what can be held without a device.  The three entry points are named by the header, the library, the
Python binding and the Julia shim; the Python wrappers refuse wrong shapes and entries that are not finite before any library call; and
the two references tests/test_gpu_sampled_members.py uses are pinned against each other: the oracle on a member's MIXED OPERATORS at the
caller's coefficients (reference A), and the oracle on the plain operators at coefficients whose samples are the MIXED TABLE (reference B)."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT, reference_pass

from test_gpu_drift_batch import dense_members, with_hconst
from test_gpu_member_batch import full_mixes, mixed_params
from test_gpu_random import random_problem
from test_sampled_controls_host import _grid

SYMBOLS = ("jq_traceobjgrad_samples_batch", "jq_traceobjgrad_samples_members", "jq_eval_f_g_grad_samples_members")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_library_python_and_julia_name_the_three_entry_points(jq):
    from juqbox_jl_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", _read("include", "juqbox_hip.h"), flags=re.S)
    julia = re.sub(r"#.*", "", _read("julia", "hip_backend.jl"))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name + ": not declared in include/juqbox_hip.h"
        assert getattr(L, name) is not None      # (AttributeError: not exported)
        assert name in _lib.SYMBOLS, name + ": not in the binding table of juqbox.jl_amd/_lib.py"
        assert "ccall((:%s, libjq)" % name in julia, name + ": no ccall in julia/hip_backend.jl"
    # symbols only: the ABI version did not move
    assert int(re.search(r"#define JQ_ABI_VERSION (\d+)", header).group(1)) == 6 == _lib.JQ_ABI_VERSION
    assert _lib.load().jq_abi_version() == 6
    for name in ("traceobjgrad_samples_batch", "traceobjgrad_samples_members", "eval_f_g_grad_samples_members"):
        assert callable(getattr(jq, name)), name
    assert "torch_controls" not in _read("juqbox.jl_amd", "__init__.py")
    for name in ("SampledMembersObjective", "SampledBatchObjective"):
        assert re.search(r"^class %s\(torch\.autograd\.Function\)" % name, _read("juqbox.jl_amd", "torch_controls.py"), flags=re.M), name
    L = _lib.load()
    assert L.jq_traceobjgrad_samples_batch(None, None, 0, 0, 0, None, None, None, None) == _lib.JQ_EINVAL
    assert L.jq_traceobjgrad_samples_members(None, None, 0, None, None, 0, 0, None, None, None, None) == _lib.JQ_EINVAL
    assert L.jq_eval_f_g_grad_samples_members(None, None, 0, None, None, None, 0, 0, None, None, None, None) == _lib.JQ_EINVAL


class _NoLibrary:
    """stands where the handle would: a wrapper that reaches for it made a library call"""

    def __get__(self, obj, owner=None):
        raise AssertionError("the wrapper reached for the handle before it refused its arguments")


def test_the_wrappers_refuse_their_arguments_before_any_library_call(jq):
    from juqbox_jl_amd.evalobjgrad import Working_Arrays_HIP

    class Stub(Working_Arrays_HIP):      # (no handle is ever created: __init__ does not run)
        handle = _NoLibrary()

        def sync_params(self):
            raise AssertionError("the wrapper synchronised the handle before it refused its arguments")

        def close(self):
            pass

    p = random_problem(jq, np.random.default_rng(3), 4, 3, 2, 1, 3, 3, 1, False)[0]
    wa = Stub.__new__(Stub)
    wa.params = p
    nf, nt, Nc = 2 * p.Ncoupled, 2 * p.nsteps + 1, p.Ncoupled
    ok = np.zeros((nf, nt))
    nan = ok.copy()
    nan[1, 2] = np.nan
    mix = np.stack([np.eye(Nc)] * 2, axis=2)
    badmix = mix.copy()
    badmix[0, 1, 1] = np.inf
    calls = [
        lambda: jq.traceobjgrad_samples_batch(np.zeros((2, nf, nt - 1)), p, wa),      # a wrong table shape
        lambda: jq.traceobjgrad_samples_batch(np.zeros((nf, nt)), p, wa),
        lambda: jq.traceobjgrad_samples_batch([ok, np.zeros((nt, nf))], p, wa),
        lambda: jq.traceobjgrad_samples_batch([], p, wa),
        lambda: jq.traceobjgrad_samples_batch([ok, nan], p, wa),      # a sample that is not finite, in the second table
        lambda: jq.traceobjgrad_samples_members(np.zeros((nf, nt + 1)), p, wa, ctrl_mix=mix),
        lambda: jq.traceobjgrad_samples_members(nan, p, wa, ctrl_mix=mix),
        lambda: jq.traceobjgrad_samples_members(ok, p, wa, ctrl_mix=badmix),      # a mix entry that is not finite
        lambda: jq.traceobjgrad_samples_members(ok, p, wa),      # Hconsts and ctrl_mix both None
        lambda: jq.traceobjgrad_samples_members(ok, p, wa, Hconsts=[p.Hconst] * 3, ctrl_mix=mix),      # 3 drifts, 2 mixes
        lambda: jq.traceobjgrad_samples_members(ok, p, wa, ctrl_mix=np.zeros((Nc + 1, Nc + 1, 2))),
        lambda: jq.eval_f_g_grad_samples_members(np.zeros((nf, nt - 1)), p, wa, [0.5, 0.5], ctrl_mix=mix),
        lambda: jq.eval_f_g_grad_samples_members(nan, p, wa, [0.5, 0.5], ctrl_mix=mix),
        lambda: jq.eval_f_g_grad_samples_members(ok, p, wa, [0.5, 0.5], ctrl_mix=badmix),
        lambda: jq.eval_f_g_grad_samples_members(ok, p, wa, [0.5, 0.5]),
        lambda: jq.eval_f_g_grad_samples_members(ok, p, wa, [0.5, 0.25, 0.25], ctrl_mix=mix),      # a weight count that is not the member count
        lambda: jq.eval_f_g_grad_samples_members(ok, p, wa, [0.5], Hconsts=[p.Hconst] * 2),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            print("call %d" % i)
            call()
    with pytest.raises(TypeError):
        jq.traceobjgrad_samples_members(ok, p, object(), ctrl_mix=mix)
    # ... and well-formed arguments do reach the library
    with pytest.raises(AssertionError):
        jq.traceobjgrad_samples_members(ok, p, wa, ctrl_mix=mix)


def mix_matrix(C, nt):
    """the mix as a matrix on flat tables (column-major [2 Nc x nt]): per time point C (x) I_2, row 2 l + s = sum_k C[l, k] row 2 k + s"""
    return np.kron(np.eye(nt), np.kron(np.asarray(C, dtype=np.float64), np.eye(2)))


def test_the_two_references_of_the_gpu_tests_agree(jq):
    """The 7-step row-lane problem of tests/test_gpu_sampled_controls.py with D1 = 2 nsteps + 3, three members with a dense drift and a
    full mix.  A: the oracle on mixed_params(p, C_g, H_g) at pcof.  B: the oracle on p with Hconst = H_g at x = lstsq(B, M_g B pcof), M_g
    the mix on tables -- the same table to rounding, so the objectives agree to 1e-12 (the bound of
    test_index_maps_with_an_asymmetric_piecewise_constant_pulse for the same construction); and A's coefficient gradient is
    B' M_g' G, with G the sample gradient that B's coefficient gradient B' G determines (B has full row rank)."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(77000 + 13 * 3)
    nsteps = 7
    p = random_problem(jq, rng, 4, 3, 2, 1, nsteps, 3, 1, False)[0]
    nt, nf, D1 = 2 * nsteps + 1, 2 * p.Ncoupled, 2 * nsteps + 3
    ncoeff = nf * p.Nfreq * D1
    pcof = 0.3 * rng.standard_normal(ncoeff)
    Bm = jq.spline_sample_matrix(p, ncoeff, _grid(p))
    assert Bm.shape == (nf * nt, ncoeff)
    drifts, mixes = dense_members(p.Hconst, 3, 911), full_mixes(p.Ncoupled, 3, 912)
    for g, (H, C) in enumerate(zip(drifts, mixes)):
        M = mix_matrix(C, nt)
        a = Oracle(mixed_params(p, C, H), use_sparse=False).traceobjgrad(pcof)
        x = np.linalg.lstsq(Bm, M @ (Bm @ pcof), rcond=None)[0]
        assert np.abs(Bm @ x - M @ (Bm @ pcof)).max() <= 1e-13
        b = Oracle(with_hconst(p, H), use_sparse=False).traceobjgrad(x)
        print("member %d: objfv A %.15e, B %.15e, difference %.2e" % (g, a["objfv"], b["objfv"], abs(a["objfv"] - b["objfv"])))
        assert abs(a["objfv"] - b["objfv"]) <= 1e-12
        for name in ("totalgrad", "infidelgrad"):
            G, res = np.linalg.lstsq(Bm.T, b[name], rcond=None)[:2]
            assert np.abs(Bm.T @ G - b[name]).max() <= 1e-12 * max(1.0, np.abs(b[name]).max())      # (b's gradient IS B' G for a table gradient G)
            back = Bm.T @ (M.T @ G)
            d = np.linalg.norm(back - a[name]) / np.linalg.norm(a[name])
            print("member %d %s: |B' M' G - A| / |A| = %.2e (|A| %.3e)" % (g, name, d, np.linalg.norm(a[name])))
            assert reference_pass(back, a[name]), (g, name)
