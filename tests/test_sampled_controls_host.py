"""CPU: controls given as samples on the time grid (jq_traceobjgrad_samples and its siblings) -- what can be held without a device.
The four entry points are named by the header, the library, the Python binding and the Julia shim; spline_sample_matrix, the dense
B = d pq / d pcof the GPU tests fold sample gradients with, is pinned by the ORACLE's control evaluation; and the rank condition those tests
rely on holds: with one carrier frequency and D1 = 2 nsteps + 3 coefficients per spline, B has full ROW rank with a bounded condition, so
no component of a sample gradient G is invisible in B' G."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

SYMBOLS = ("jq_sample_times", "jq_control_samples", "jq_traceobjgrad_samples", "jq_eval_f_g_grad_samples")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_library_python_and_julia_name_the_four_entry_points():
    from juqbox_jl_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", _read("include", "juqbox_hip.h"), flags=re.S)
    julia = re.sub(r"#.*", "", _read("julia", "hip_backend.jl"))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name + ": not declared in include/juqbox_hip.h"
        assert getattr(L, name) is not None      # (AttributeError: not exported)
        assert name in _lib.SYMBOLS, name + ": not in the binding table of juqbox.jl_amd/_lib.py"
        assert "ccall((:%s, libjq)" % name in julia, name + ": no ccall in julia/hip_backend.jl"
    # additive: the ABI version did not move
    assert int(re.search(r"#define JQ_ABI_VERSION (\d+)", header).group(1)) == 6 == _lib.JQ_ABI_VERSION


def test_python_surface(jq):
    for name in ("control_sample_times", "control_samples", "traceobjgrad_samples", "eval_f_g_grad_samples", "spline_sample_matrix"):
        assert callable(getattr(jq, name)), name
    # importing the package does not import torch: torch_controls is the one module with a module-level import of it (ipopt_interface
    # imports torch.distributed inside the functions that need it)
    for f in os.listdir(os.path.join(ROOT, "juqbox.jl_amd")):
        if f.endswith(".py") and f != "torch_controls.py":
            assert not re.search(r"^(import|from)\s+torch\b", _read("juqbox.jl_amd", f), flags=re.M), f
    assert "torch_controls" not in _read("juqbox.jl_amd", "__init__.py")


def test_argument_rules_that_need_no_device():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    t = np.zeros(3)
    assert L.jq_sample_times(None, t.ctypes.data_as(_lib.c_dp), 3) == _lib.JQ_EINVAL
    assert L.jq_control_samples(None, None, 0, None) == _lib.JQ_EINVAL
    assert L.jq_traceobjgrad_samples(None, None, 0, 0, None, None, None, None) == _lib.JQ_EINVAL
    assert L.jq_eval_f_g_grad_samples(None, None, 0, None, None, 0, None, 0, None, None, None) == _lib.JQ_EINVAL


def _params(jq, rng, Nc, Nfreq, nsteps):
    """a problem as far as the controls go (the operators do not enter B)"""
    Ntot, N = 3, 2
    z = np.zeros((Ntot, Ntot))
    return jq.objparams([N], [Ntot - N], 1.0 + rng.random(), nsteps, Uinit=np.eye(Ntot)[:, :N], Utarget=np.eye(Ntot)[:, :N] + 0j,
                        Cfreq=rng.standard_normal((Nc, Nfreq)), Rfreq=np.zeros(Nc), Hconst=z, Hsym_ops=[z + np.eye(Ntot)] * Nc,
                        Hanti_ops=[z] * Nc)


def _grid(p):
    """the times of jq_sample_times restated: t accumulated like the forward sweep's table, half points t + dt / 2"""
    dt = p.T / p.nsteps
    t, out = 0.0, []
    for n in range(p.nsteps + 1):
        out.append(t)
        if n < p.nsteps:
            out.append(t + 0.5 * dt)
        t = t + dt
    return np.array(out)


@pytest.mark.parametrize("Nc,Nfreq,nsteps,D1", [(1, 1, 2, 7), (2, 2, 7, 17), (3, 1, 5, 4), (2, 3, 3, 3)])
def test_spline_sample_matrix_against_the_oracles_controls(jq, Nc, Nfreq, nsteps, D1):
    """Column k of B is the central difference of the oracle's control evaluation along e_k with step 1 -- exact, the controls are linear
    in pcof -- at every time of the grid, t = 0 and t = T (the clamped knot indices) included; and B pcof is the oracle's controls."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(100 * Nc + 10 * Nfreq + nsteps)
    p = _params(jq, rng, Nc, Nfreq, nsteps)
    ncoeff = 2 * Nc * Nfreq * D1
    times = _grid(p)
    assert times.size == 2 * nsteps + 1 and times[0] == 0.0 and abs(times[-1] - p.T) < 1e-14
    B = jq.spline_sample_matrix(p, ncoeff, times)
    assert B.shape == (2 * Nc * times.size, ncoeff)
    o = Oracle(p)
    ref = np.zeros_like(B)
    for k in range(ncoeff):
        e = np.zeros(ncoeff)
        e[k] = 1.0
        for J, t in enumerate(times):
            ref[2 * Nc * J:2 * Nc * (J + 1), k] = 0.5 * (o.controls(e, t) - o.controls(-e, t))
    err = np.abs(B - ref).max()
    print("Nc %d Nfreq %d nsteps %d D1 %d: max |B - oracle| = %.2e (max |B| %.2f)" % (Nc, Nfreq, nsteps, D1, err, np.abs(B).max()))
    # the same formulas, possibly in another order of operations: an entry is a quadratic in tau with terms below 4.5 (ulp 8.9e-16) times a
    # sine or cosine -- fewer than ten roundings of that size
    assert err <= 1e-14
    assert np.count_nonzero(ref) > 0 and np.all(np.count_nonzero(ref, axis=1) <= 6 * Nfreq)      # (three knots, two blocks per frequency)
    pcof = rng.standard_normal(ncoeff)
    pq = (B @ pcof).reshape((2 * Nc, times.size), order="F")
    for J, t in enumerate(times):
        assert np.allclose(pq[:, J], o.controls(pcof, t), rtol=0, atol=1e-13)


# sigma_min / sigma_max of the spline collocation block (knot spacing T / (2 nsteps + 1) against a grid of spacing T / (2 nsteps)), which the
# carrier rotation -- orthogonal per time point -- leaves unchanged: computed 0.83, 0.66, 0.42, 0.40, 0.35
@pytest.mark.parametrize("nsteps", [1, 2, 7, 8, 11])
def test_full_row_rank_with_one_frequency_and_two_nsteps_plus_three_coefficients(jq, nsteps):
    rng = np.random.default_rng(nsteps)
    Nc = 2
    p = _params(jq, rng, Nc, 1, nsteps)
    D1 = 2 * nsteps + 3
    B = jq.spline_sample_matrix(p, 2 * Nc * D1, _grid(p))
    assert B.shape == (2 * Nc * (2 * nsteps + 1), 2 * Nc * D1) and B.shape[0] < B.shape[1]
    sv = np.linalg.svd(B, compute_uv=False)
    print("nsteps %d: B %r, sigma_min / sigma_max = %.3f" % (nsteps, B.shape, sv[-1] / sv[0]))
    assert sv.size == B.shape[0] and sv[-1] / sv[0] >= 0.2


def test_sample_table_shapes_are_refused_before_any_library_call(jq):
    from juqbox_jl_amd.evalobjgrad import _sample_table
    p = _params(jq, np.random.default_rng(0), 2, 1, 3)
    ok = np.zeros((4, 7))
    tab, shape = _sample_table(ok, p, "t")
    assert tab.size == 28 and shape == (4, 7)
    for bad in (np.zeros((4, 6)), np.zeros((7, 4)), np.zeros(28), np.full((4, 7), np.nan), np.full((4, 7), np.inf)):
        with pytest.raises(ValueError):
            _sample_table(bad, p, "t")
    with pytest.raises(ValueError):
        jq.spline_sample_matrix(p, 10, [0.0])
