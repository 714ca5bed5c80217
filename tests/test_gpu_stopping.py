"""GPU (-m gpu): every stopping rule against the CPU oracle where stopping decides the result.  The four kernel-object matrices run their
Jacobi and implicit-midpoint cells at tol 1e-12 / 1e-11 with a cap that is never reached, where one iteration more or less moves the
gradient by less than their criteria.  Here every cell of tests/stopping_matrix.py -- completeness, and the conditions that make a run
decisive, mixed and discriminating, are checked by tests/test_stopping_matrix.py on the oracle's iteration record -- runs on ONE handle
at tol 1e-4 and 1e-6 (exit by tolerance after 2 .. 8 iterations), at caps of 1, 2, 3 (and 0, Jacobi) with a tolerance that is never
met, at the median count of the cell as cap (both exits in one evaluation) and at last at the source cell's own settings; the settings
change through params.linear_solver.  Every run asserts the gradient evaluation and the forward-only objective, the 1e-4 run also the
per-step history, the 1e-4 and the mixed run also an ensemble whose samples share slabs and stop at different counts -- and after every
evaluation the object the source table names.

Criterion: conftest.reference_pass (atol 1e-14 or rtol 1e-10) per quantity for BOTH solvers, the history < 1e-10 absolute.  On these
runs no stopping comparison of the oracle is within 1e-6 relative of its tolerance, so both sides execute the same iterations and what
remains is rounding; exception (i) of DESIGN.md section 2 (implicit midpoint at 1e-9) is for tolerances at which the comparison itself
sits in the rounding noise and applies to the last run only, which keeps its source table's criterion."""
import json
import os

import numpy as np
import pytest
from conftest import ATOL, RTOL, reference_pass

import stopping_matrix as S
from test_gpu_block_band import _check_imr_tolerance, _check_reference_tolerance
from test_gpu_time_loop import _NO_ENSEMBLE

pytestmark = pytest.mark.gpu
HISTORY_ATOL = 1e-10


def source_criterion(kind, ev, ref_single):
    """the source tables' criterion on one gradient evaluation (tests/test_gpu_block_band.py): reference_pass per quantity, implicit
    midpoint 1e-9 (exception (i))"""
    o, rr = {"evals": [ev], "ensemble": _NO_ENSEMBLE[1]}, {"single": ref_single, "ensemble": _NO_ENSEMBLE[0]}
    (_check_imr_tolerance if kind == "imr" else _check_reference_tolerance)(o, rr)


def miss(value, ref):
    """(error, factor): the error reference_pass looks at (relative 2-norm; absolute where the reference is below atol) and the factor by
    which it misses the criterion (< 1: passes)"""
    value, ref = np.atleast_1d(np.asarray(value, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    d, nrm = np.linalg.norm(value - ref), np.linalg.norm(ref)
    if nrm < ATOL:
        return d, d / ATOL
    return d / nrm, min(d / ATOL, d / nrm / RTOL)


def quantities(run, out, ref):
    """[(name, value, reference)] of a run: what reference_pass is asked about"""
    r = ref["single"]
    q = [("grad-eval " + n, v, r[n]) for n, v in zip(S.SINGLE, out["eval"])]
    q += [("forward-only " + n, v, r[n]) for n, v in zip(S.SINGLE[:3], out["forward"])]
    if run.ensemble:
        q += [("ensemble " + n, v, ref["ensemble"][n]) for n, v in zip(S.ENSEMBLE, out["ensemble"])]
    return q


def _report(cell, worst):
    path = os.environ.get("JQ_STOPPING_REPORT")      # (a measuring run keeps every figure: one JSON line per cell)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"cell": cell.name, "family": S.family_of(cell), "worst": worst}) + "\n")


@pytest.mark.parametrize("cell", S.CELLS, ids=[c.name for c in S.CELLS])
def test_cell_stops_where_the_oracle_stops_on_its_object(jq, cell):
    refs = S.references(jq, cell)
    outs = S.run_cell(jq, cell, refs)
    assert [run for run, _ in outs] == list(S.runs_of(cell))
    failed, worst = [], {}
    for run, out in outs:
        S.check_object(cell, out)
        ref = refs[run.name]
        if run.name == "OWN":      # the handle is what it was: the source table's criterion at the source table's settings
            source_criterion(cell.kind, out["eval"], ref["single"])
        errs = []
        for name, v, w in quantities(run, out, ref):
            err, factor = miss(v, w)
            errs.append(err)
            print("%s %s %s: error %.3e (%.3g x the criterion)" % (cell.name, run.name, name, err, factor))
            if run.name != "OWN" and not reference_pass(v, w):
                failed.append((run.name, name, err))
        if run.history:
            assert out["history"].shape == ref["single"]["history"].shape
            h = float(np.max(np.abs(out["history"] - ref["single"]["history"])))
            print("%s %s history: max abs error %.3e" % (cell.name, run.name, h))
            if not h < HISTORY_ATOL:
                failed.append((run.name, "history", h))
        worst[run.name] = max(errs)
    _report(cell, worst)
    assert not failed, (cell.name, failed)
    opts = S.partner_options(cell)
    if opts is not None:      # the source promises a second set of options to be BIT-identical: at every run
        twin = S.run_cell(jq, cell, refs, opts)
        for (run, a), (_, b) in zip(outs, twin):
            for key in ("eval", "forward", "history", "ensemble"):
                if key in a:
                    va, vb = np.atleast_1d(a[key]) if key == "history" else a[key], np.atleast_1d(b[key]) if key == "history" else b[key]
                    assert all(np.array_equal(x, y) for x, y in zip(va, vb)), (cell.name, run.name, key, opts)
