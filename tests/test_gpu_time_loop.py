"""GPU (-m gpu): the time loop crossed with every kernel object.  The block-band, the structured and the uncoupled matrix pin every object
on its instantiation, and all run the same loop: 7 steps in one chunk and in chunks of 3 + 3 + 1 at one Neumann order per cell.  The
one wrong-number bug in this project's record that came from the compiler (csrc/Makefile: w_6_5 in VGPR form) showed only on a chunk of
ODD length with Neumann terms, on one separately compiled object -- so here every cell of tests/time_loop_matrix.py (the two matrices'
cells, the small systems -- lane, row-lane, their implicit-midpoint kernels, the NT = 1 slab and cooperative objects -- and the weighted
objects w_* / x_*; completeness and coverage are checked by tests/test_time_loop_matrix.py) runs problems of 1, 2, 2, 9, 8 and 11 steps in chunks of (1), (2), (1, 1),
(2, 2, 2, 2, 1), (3, 3, 2) and (4, 4, 3) steps at the source cell's own step size, with Neumann orders 0 .. 6 rotating over the cells
of a route, and the cells of the split latency kernels three more of 9, 20 and 21 steps in chunks of (9), (9, 9, 2) and (10, 10, 1),
the only ones on which those kernels are taken.  Every run (a handle per step count; the two 2-step runs share one, the chunking changed
through jq_set_option and the order through params.linear_solver) asserts the six quantities of the gradient
evaluation, the forward-only objective and the per-step history against the CPU oracle (the 8-step run also the source cell's
ensemble), the object and instantiation it ran on -- the source matrix's record with `modd` and the workgroups of the split kernels
recomputed for the run -- and that the forward sweep took one launch per chunk.  Three sweeps on one representative per kernel
template follow -- the step count, the Neumann order 0 .. 12, a trace budget that shortens the chunks of a gradient evaluation -- and the
tangent-linear sweeps (JVP, HVP, ensemble and drift-ensemble HVP) over the runs A1 and A4 .. A6."""
import numpy as np
import pytest
from conftest import reference_pass

import time_loop_matrix as T
from test_gpu_block_band import _check_imr_tolerance, _check_reference_tolerance

pytestmark = pytest.mark.gpu
_NO_ENSEMBLE = ({"last_infidelity": 1.0, "last_leak": 0.0, "last_infidelity_grad": np.ones(1), "last_leak_grad": np.zeros(1)},
                (1.0, 0.0, np.ones(1), np.zeros(1)))      # (a run without an ensemble: the criteria's ensemble part compares these two)


def check_numbers(cell, run, out, ref):
    """the criteria of tests/test_gpu_block_band.py on one run: the gradient evaluation (and the ensemble, where the run has one),
    the forward-only objective under the same criterion, the history under that file's bound"""
    r = ref["single"]
    o = {"evals": [out["eval"]], "ensemble": out.get("ensemble", _NO_ENSEMBLE[1])}
    rr = {"single": r, "ensemble": ref["ensemble"] if "ensemble" in out else _NO_ENSEMBLE[0]}
    objfv, prim, sec = out["forward"]
    if cell.kind == "imr":
        _check_imr_tolerance(o, rr)
        assert abs(prim - r["primaryobjf"]) <= 1e-9 and abs(sec - r["secondaryobjf"]) <= 1e-9 * max(abs(r["secondaryobjf"]), 1e-3)
        assert abs(objfv - r["objfv"]) <= 1e-9 * max(abs(r["objfv"]), 1.0)
    else:
        _check_reference_tolerance(o, rr)
        for name, v, w in (("objective", objfv, r["objfv"]), ("infidelity", prim, r["primaryobjf"]), ("leak", sec, r["secondaryobjf"])):
            assert reference_pass(v, w), ("forward only", name, v, w)
    assert out["history"].shape == r["history"].shape == (out["history"].shape[0], out["history"].shape[1], run.nsteps + 1)
    assert np.max(np.abs(out["history"] - r["history"])) < 1e-10


@pytest.mark.parametrize("cell", T.CELLS, ids=[c.name for c in T.CELLS])
def test_cell_matches_oracle_on_its_object_on_every_run(jq, cell):
    outs = T.run_all(jq, cell)
    assert [run for run, _ in outs] == list(T.runs_of(cell))
    for run, out in outs:
        _checked(cell, run, out, T.reference(jq, cell, run, out.get("ns", 0)))


def _checked(cell, run, out, ref):
    T.check_object(cell, run, out)
    try:
        check_numbers(cell, run, out, ref)
    except AssertionError as e:
        raise AssertionError("%s %s (chunks %s, m %s): %s" % (cell.name, run.name, T.chunks(run), T.m_run(cell, run), e)) from e


@pytest.mark.parametrize("cell", T.SWEEP_CELLS, ids=[c.name for c in T.SWEEP_CELLS])
def test_step_sweep_on_a_representative_of_every_template(jq, cell):
    """one chunk of 1 .. 12, 16, 17 steps at the cell's own Neumann order (the split latency kernels: 9 .. 12, 16, 17, 24, 25): every
    ring of time points at depth - 1, depth, depth + 1 and on its second wrap"""
    runs = T.step_runs(cell)
    refs = T.sweep_references(jq, cell, runs)
    for run, ref in zip(runs, refs):
        _checked(cell, run, T.run_one(jq, cell, run), ref)


@pytest.mark.parametrize("name", T.SV_REPRESENTATIVES)
def test_neumann_sweep_on_a_representative_of_every_template(jq, name):
    """m = 0 .. 12 on one handle, 5 steps in chunks of 2 + 2 + 1, at the amplitude factor at which the oracle sees every term"""
    cell = T.BY_NAME[name]
    refs = T.sweep_references(jq, cell, T.neumann_runs(cell), T.SWEEP_AMPLITUDE[name])
    outs = T.run_neumann_sweep(jq, cell)
    assert [run.mslot for run, _ in outs] == list(T.NEUMANN_SWEEP)
    for (run, out), ref in zip(outs, refs):
        _checked(cell, run, out, ref)


@pytest.mark.parametrize("cell", T.SWEEP_CELLS, ids=[c.name for c in T.SWEEP_CELLS])
def test_trace_budget_shortens_both_sweeps_of_a_gradient_evaluation(jq, cell):
    """9 steps, chunk_steps unset, trace_bytes=1: nine backward chunks of one step.  The library keeps one chunk length per evaluation
    (jq_host_plan.h plan_batch), so the forward sweep of the gradient evaluation is launched in the same nine chunks and the forward-only
    evaluation of the handle in one: 9 and 9 x sweeps x control groups launches, then (1, 0) (check_object)"""
    run = T.BACKWARD_ONLY
    out = T.run_one(jq, cell, run)
    assert out["forward_launches"] == (1, 0) and out["launches"][0] == 9 and out["launches"][1] == 9 * (2 if out["objFuncType"] != 1 else 1) * out["plan"]["control_groups"]
    _checked(cell, run, out, T.sweep_reference(jq, cell, run))


@pytest.mark.parametrize("cell", T.TL_CELLS, ids=[c.name for c in T.TL_CELLS])
def test_tangent_linear_sweeps_over_the_chunkings(jq, cell):
    """jq_traceobj_jvp, jq_traceobjgrad_hvp, jq_eval_f_g_grad_hvp (lane, row-lane, quad route) and jq_eval_f_g_grad_drifts_hvp over the
    runs A1 and A4 .. A6: the tangents cross chunk boundaries of even and odd length at every Neumann class.  References and criteria
    are the source tests' own; the plan record must report the run's chunk length, the timing record one launch per chunk"""
    import test_gpu_drift_hvp as GD
    import test_gpu_ens_hvp as GE
    import test_gpu_hvp as GH
    import test_gpu_jvp as GJ
    refs = T.tl_references(jq, cell)
    src = T.tl_source(jq, cell)
    for run, ref in zip(T.TL_RUNS, refs):
        out = T.tl_run(jq, cell, run)
        wa, r, p, pcof = out["wa"], out["r"], out["p"], out["pcof"]
        try:
            T.tl_check_records(cell, run, out)
            if cell.api == "jvp":
                GJ._check_against_reference(r, ref)
                GJ._check_primal(jq, r, pcof, p, wa)
            elif cell.api == "hvp":
                GH._check_against_reference(r, ref[0], p.objFuncType != 1)
                GH._check_primal(jq, r, pcof, p, wa, ref[1])
            elif cell.api == "ens":
                GE._check_against_reference(r, ref)
                GE._check_primal(jq, r, pcof, p, wa, src["nodes"], src["weights"], src["shift"])
            else:
                GD._check(r, p, ref[0], ref[1])
        except AssertionError as e:
            raise AssertionError("%s %s (chunks %s, m %d): %s" % (cell.name, run.name, T.chunks(run), T.tl_m(cell, run), e)) from e
        finally:
            wa.close()
