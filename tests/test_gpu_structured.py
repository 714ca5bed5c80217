"""GPU (-m gpu): every kernel object behind the structure codes 7, 8, 9 and every specialised instantiation inside them (UNI / ORD / SC
of the three-slab quad kernels, ORD / RIDE of the split quad backward sweep, ORD x MODD x WLR of the cooperative-quad kernels on one, two
and three workgroups per column quad) against the CPU oracle on problems whose control q acts on subsystem q only
(tests/subsystem_problem.py) -- the condition under which the library selects them, which no other random problem of the suite meets.
Every cell of tests/structured_matrix.py (its completeness is checked by tests/test_structured_matrix.py) runs at Ntot = 16 NT - 3 or
16 NT with 7 time steps in one chunk and in chunks of 3 + 3 + 1 (the split latency kernels: 11 steps in one chunk), the per-step
history and a 13-sample ensemble (four slabs: a full three-slab workgroup and a ragged one), and is asserted to have run the
instantiation the table names: jq_plan_info "last_kernels" (object, slabs / quads per workgroup, workgroups per quad, flags), the
build manifest's object list, family / size / band of jq_last_timing.  Where the source promises bit-identity between two variants
(s_compact, cq_fwd2, cq3, imr_cq2, the split quad sweep at four quads per workgroup against the one-wave kernel) the cell runs its
partner and every number must agree in every bit; specialised against generic trace products (no_ord, no_uni, cq_generic_traces,
RIDE) is promised nowhere: both sides meet the oracle.  The cells whose object ships in the VGPR register form also go through the
default-register-form build of the same sources, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import structured_matrix as M
from test_gpu_block_band import _check_imr_tolerance, _check_reference_tolerance

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cell", M.CELLS, ids=[c.name for c in M.CELLS])
def test_cell_matches_oracle_on_its_instantiation(jq, cell):
    if cell.name in M.REFUSED:      # the table says the plan refuses this combination: it must, with this message
        from juqbox_jl_amd import _lib
        with pytest.raises(_lib.JuqboxHipError) as e:
            M.run_cell(jq, cell)
        assert e.value.code == _lib.JQ_EUNSUPPORTED and M.REFUSED[cell.name] in str(e.value)
        return
    out = M.run_cell(jq, cell)      # (asserts the last_kernels record, the manifest and the timing record after every gradient evaluation)
    ref = M.reference(jq, cell, out["ns"])
    assert len(out["evals"]) == len(cell.chunks)
    (_check_imr_tolerance if cell.kind == "imr" else _check_reference_tolerance)(out, ref)
    assert np.max(np.abs(out["history"] - ref["single"]["history"])) < 1e-10
    if cell.partner is not None:      # the variant the source promises to be bit-identical
        a, b = M.B.exact(out), M.B.exact(M.run_cell(jq, cell, opts=cell.partner, check=False))
        assert a == b, [k for k in a if a[k] != b[k]]


def test_a_single_block_never_runs_the_cooperative_quad_families(jq):
    """u_1_7 and v_1_7 are built but unreachable (structured_matrix.UNREACHABLE): an NT = 1 problem with every option at its default --
    but lane=0, without which Ntot <= 16 stays on the row-lane kernels -- runs the quad-layout families 6 / 7, never 8 / 9"""
    assert set(M.UNREACHABLE) == {"u_1_7", "v_1_7"}
    cell = M.BY_NAME["quad1-generic-NT1"]
    p0, pcof = M.base_problem(jq, cell.prob)
    for kind, WA, family in (("neumann", jq.Working_Arrays_HIP, 6), ("imr", jq.Working_Arrays_M_HIP, 7)):
        p = M.with_solver(jq, p0, kind, 0)
        wa = WA(p, pcof.size, options={"lane": 0})
        try:
            jq.traceobjgrad(pcof, p, wa, False, True)
            t, k = wa.last_timing(), wa.plan_info()["last_kernels"]
            assert t["kernel_family"] == family and t["kernel_size"] == 1 and k["object"][0] in "spq" and k["forward_object"][0] in "sq", (t, k)
        finally:
            wa.close()


def test_vgpr_form_cells_are_bit_identical_in_both_register_forms(tmp_path):
    """The s_ / p_ / q_ objects, k_N_8, k_N_9 and c_N_9 ship in VGPR form: a fresh process per library (JQ_LIB, as scripts/check_forms.py)
    runs their cells; objectives, gradients, histories and ensembles must agree in every bit."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_forms
    dumps = []
    for name, lib in (("main", check_forms.MAIN), ("df", check_forms.DF)):
        assert os.path.exists(lib), lib
        path = str(tmp_path / (name + ".json"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "structured_matrix.py"), path], env=dict(os.environ, JQ_LIB=lib),
                           cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        dumps.append(json.load(open(path)))
    a, b = dumps
    want = {c.name: c.expect["object"] for c in M.VGPR_CELLS if c.name not in M.REFUSED}
    assert set(a) == set(b) == set(want) and len(want) >= 87      # s_ 16, p_ 37, q_ 16, k_N_8 8, k_N_9 5, c_N_9 5
    assert all(a[k]["tag"] == want[k] for k in want)
    differ = [k for k in sorted(want) if a[k] != b[k]]
    assert not differ, differ[:10]
