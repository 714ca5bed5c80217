"""CPU: the structure test behind the compact S operand of the three-slab quad-layout kernels (jq_s_uniform = plan info "s_uniform";
csrc/jq_host_images.h s_image_uniform).  With Hanti_k = a_k - a_k' on a 4 x 4 x n space every 16-row block of S(t) = sum_k q_k(t) Hanti_k
repeats block 0: the same 4 x 4 diagonal blocks, the same (i, i +- 4) couplings, one (i, i +- 16) coupling per pair of blocks.  The
kernels read block 0 only when -- and only when -- that holds for the problem at hand."""
import os
import re

import numpy as np
import pytest
from conftest import ROOT


def s_uniform(hanti):
    from juqbox_jl_amd import _lib
    L = _lib.load()
    ops = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.float64).ravel(order="F") for h in hanti]))
    return L.jq_s_uniform(ops.ctypes.data_as(_lib.c_dp), hanti[0].shape[0], len(hanti))


def test_cnot3_has_uniform_s_images(jq):
    params, _ = jq.cases.cnot3()
    assert params.Ntot == 96 and s_uniform(params.Hanti_ops) == 1
    # ... every operator on its own, and the same set-up with another number of cavity levels (4 x 4 x 4)
    assert all(s_uniform([h]) == 1 for h in params.Hanti_ops)
    small, _ = jq.cases.cnot3(Ng3=3)
    assert small.Ntot == 64 and s_uniform(small.Hanti_ops) == 1


def _perturbed(jq, which):
    """cnot3 with one entry pair of one Hanti changed; the nonzero pattern -- and with it the 4 x 4 x n structure -- stays"""
    params, _ = jq.cases.cnot3()
    H = [h.copy() for h in params.Hanti_ops]
    if which == "diagonal block":          # the 4 x 4 block of row group 5 (rows 20 .. 23) of a - a'
        r, c, q = 21, 20, 0
    elif which == "coupling +-4":          # one (i, i + 4) pair of b - b': the coefficient now depends on the row, not only on b
        r, c, q = 37, 33, 1
    elif which == "coupling +-4, block 0":
        r, c, q = 6, 2, 1
    else:                                  # one (i, i + 16) pair of c - c': no longer one number per pair of blocks
        r, c, q = 50, 34, 2
    assert H[q][r, c] != 0.0 and H[q][c, r] == -H[q][r, c]
    H[q][r, c] *= 1.0 + 2.0 ** -30
    H[q][c, r] = -H[q][r, c]
    return params, H


@pytest.mark.parametrize("which", ["diagonal block", "coupling +-4", "coupling +-4, block 0", "coupling +-16"])
def test_a_perturbed_entry_switches_it_off(jq, which):
    params, H = _perturbed(jq, which)
    assert s_uniform(H) == 0, which
    assert s_uniform(params.Hanti_ops) == 1


def test_the_comparison_is_bit_by_bit(jq):
    """+0.0 and -0.0 compare equal and are different operands: the record must hold the bits the full image holds"""
    params, _ = jq.cases.cnot3()
    H = [h.copy() for h in params.Hanti_ops]
    assert H[0][40, 43] == 0.0
    H[0][40, 43] = -0.0            # (inside the diagonal 4 x 4 block of row group 10)
    assert s_uniform(H) == 0


def test_operators_outside_the_structure_and_bad_sizes(jq):
    params, _ = jq.cases.cnot3()
    H = [h.copy() for h in params.Hanti_ops]
    H[1][0, 9], H[1][9, 0] = 0.5, -0.5      # neither a diagonal-block entry nor a +-4 / +-16 coupling
    assert s_uniform(H) == 0
    assert s_uniform([np.zeros((12, 12))]) < 0      # (JQ_EINVAL: not a multiple of 16)


def test_the_option_is_documented():
    table = open(os.path.join(ROOT, "juqbox.jl_amd", "csrc", "jq_options.h")).read()
    assert re.search(r'\{"s_compact", 1, 0,', table), "s_compact: a per-evaluation option, default on"
    assert "s_compact" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hdr = open(os.path.join(ROOT, "include", "juqbox_hip.h")).read()
    assert "jq_s_uniform" in hdr
