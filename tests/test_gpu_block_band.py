"""GPU (-m gpu): every block-band kernel object against the CPU oracle on operators that FILL their 16 x 16 tiles.  The random problems
of the other tests reach the band kernels with one entry (a ladder operator) or a diagonal per off-diagonal block, never with block band 2
below dense and never with block band 0 on two or more tile rows; here every (tile rows, band code, route) cell of
tests/block_band_matrix.py -- the completeness of the table is checked by tests/test_block_band_matrix.py -- runs a problem of
tests/block_band_problem.py with a ragged last tile (Ntot = 16 NT - 3; NT = 4, 6, 16: also full tiles), three controls with the trace
layouts 1 / 0 / 2 (full band, block diagonal, band without diagonal blocks), 7 time steps in one chunk and in chunks of 3 + 3 + 1, the
per-step history and a 7-sample ensemble (21 columns: two slabs, the last one ragged), and is asserted to have run on the object the
table names.  The NT <= 6 cells, whose slab and cooperative objects ship in the VGPR register form, also go through the
default-register-form build of the same sources: every number must be bit-identical."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import reference_pass

import block_band_matrix as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_reference_tolerance(out, ref):
    """Stormer-Verlet, Neumann and Jacobi (tol 1e-12: an iteration more or less moves the gradient by < 1e-12 relative): the reference's
    own criterion (test/evalGrad.jl: rtol 1e-10 / atol 1e-14) per quantity"""
    r = ref["single"]
    for objfv, prim, sec, tg, ig, lg in out["evals"]:
        for name, v, w in (("objective", objfv, r["objfv"]), ("infidelity", prim, r["primaryobjf"]), ("leak", sec, r["secondaryobjf"]),
                           ("totalgrad", tg, r["totalgrad"]), ("infidelgrad", ig, r["infidelgrad"]), ("leakgrad", lg, r["leakgrad"])):
            assert reference_pass(v, w), (name, v, w)
    e = ref["ensemble"]
    for name, v in zip(("last_infidelity", "last_leak", "last_infidelity_grad", "last_leak_grad"), out["ensemble"]):
        assert reference_pass(v, e[name]), (name, v, e[name])


def _check_imr_tolerance(out, ref):
    """implicit midpoint: the project's stated 1e-9 (exception (i)), as tests/test_gpu_imr.py _random_checks"""
    r = ref["single"]
    gn = np.linalg.norm(r["totalgrad"])
    for objfv, prim, sec, tg, ig, lg in out["evals"]:
        assert abs(prim - r["primaryobjf"]) <= 1e-9 and abs(sec - r["secondaryobjf"]) <= 1e-9 * max(abs(r["secondaryobjf"]), 1e-3)
        assert np.linalg.norm(tg - r["totalgrad"]) <= 1e-9 * gn and np.linalg.norm(ig - r["infidelgrad"]) <= 1e-9 * gn
    inf, g = ref["ensemble"]["last_infidelity"], ref["ensemble"]["last_infidelity_grad"]
    assert abs(out["ensemble"][0] - inf) <= 1e-9 * abs(inf)
    assert np.linalg.norm(out["ensemble"][2] - g) <= 1e-9 * np.linalg.norm(g)


@pytest.mark.parametrize("cell,Ntot", M.CASES, ids=[M.cell_id(c, nt) for c, nt in M.CASES])
def test_cell_matches_oracle_on_its_object(jq, cell, Ntot):
    if cell.tag is None:      # the table says the plan refuses this combination: it must, and say why
        from juqbox_jl_amd import _lib
        with pytest.raises(_lib.JuqboxHipError) as e:
            M.run_cell(jq, cell, Ntot)
        assert e.value.code == _lib.JQ_EUNSUPPORTED
        return
    out = M.run_cell(jq, cell, Ntot)
    assert out["tag"] == cell.tag
    if out["objects"] is not None:      # (the build manifest is linked in)
        assert cell.tag in out["objects"], out["objects"]
    ref = M.reference(jq, cell, Ntot)
    assert len(out["evals"]) == len(M.CHUNKS)
    (_check_imr_tolerance if M.kind_of(cell.route) == "imr" else _check_reference_tolerance)(out, ref)
    assert np.max(np.abs(out["history"] - ref["single"]["history"])) < 1e-10


def test_small_cells_are_bit_identical_in_both_register_forms(tmp_path):
    """The NT <= 6 objects (k_*, c_*) ship in VGPR form: a fresh process per library (JQ_LIB, as scripts/check_forms.py) runs their
    cells; objectives, gradients, histories and ensembles must agree in every bit, and both must have run the same objects."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_forms
    dumps = []
    for name, lib in (("main", check_forms.MAIN), ("df", check_forms.DF)):
        assert os.path.exists(lib), lib
        path = str(tmp_path / (name + ".json"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "block_band_matrix.py"), path], env=dict(os.environ, JQ_LIB=lib),
                           cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        dumps.append(json.load(open(path)))
    a, b = dumps
    want = {M.cell_id(c, nt): c.tag for c, nt in M.CASES if c.NT <= 6 and c.tag is not None}
    assert set(a) == set(b) == set(want) and len(want) >= 5 * 17
    assert all(a[k]["tag"] == want[k] for k in want)
    differ = [k for k in sorted(want) if a[k] != b[k]]
    assert not differ, differ[:10]
