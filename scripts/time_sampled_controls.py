#!/usr/bin/env python3
"""Times jq_traceobjgrad_samples against jq_traceobjgrad on the SAME handle and build, swap02 and cnot3 at full length: the sample table is
the handle's own controls (jq_control_samples of the stored coefficients), so both calls run the same sweeps on the same plan.  The
spline call is the code path of every earlier build: its kernels are untouched.  Per call: the median wall time of the Python call over
REPS calls after a warm-up call, next to the library's own event times (ms_total, ms_generate: control evaluation, tile streams, trace
reduction and gradient assembly; the sample call's upload and download of 2 Nc nt doubles lie outside the events, inside the wall time).
Also printed: that the objectives agree bit for bit and how far B' G is from the spline gradient.  Arguments: the problems (default
swap02 cnot3).  Prints the body of profiles/sampled_controls.txt.  Needs a GPU; one process."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import juqbox_jl_amd as jq  # noqa: E402
from juqbox_jl_amd import _lib  # noqa: E402

REPS = 7


def timed(fn):
    """(median wall ms of REPS calls after a warm-up call, all of them, the last result, the library's events of the last call)"""
    fn()
    walls = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        r = fn()
        walls.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(walls), walls, r


def run(name):
    p, info = getattr(jq.cases, name)()
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))["pcof0"])
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    nt = 2 * p.nsteps + 1
    print("%s: Ntot %d, N %d, %d controls, %d time steps (%d time points, table of %.2f MB), %d coefficients, objFuncType %d" % (
        name, p.Ntot, p.N, p.Ncoupled, p.nsteps, nt, 8e-6 * 2 * p.Ncoupled * nt, pcof.size, p.objFuncType))
    pq = jq.control_samples(pcof, p, wa)
    fmt = lambda ev: "events: total %.2f ms, generate %.2f ms, forward %.2f ms in %d launches, backward %.2f ms in %d launches" % (
        ev["ms_total"], ev["ms_generate"], ev["ms_forward"], ev["n_forward_launches"], ev["ms_backward"], ev["n_backward_launches"])
    ts, ws, rs = timed(lambda: jq.traceobjgrad(pcof, p, wa, False, True))
    evs = wa.last_timing()
    tq, wq, rq = timed(lambda: jq.traceobjgrad_samples(pq, p, wa, True))
    evq, plan = wa.last_timing(), wa.plan_info()
    # the spline call once more, after the sample calls: the spread of the sweeps between two blocks of calls
    ts2, ws2, _ = timed(lambda: jq.traceobjgrad(pcof, p, wa, False, True))
    print("  jq_traceobjgrad          median %.2f ms wall (%s); %s" % (ts, " ".join("%.2f" % w for w in ws), fmt(evs)))
    print("  jq_traceobjgrad_samples  median %.2f ms wall (%s); %s" % (tq, " ".join("%.2f" % w for w in wq), fmt(evq)))
    print("  jq_traceobjgrad again    median %.2f ms wall (%s)" % (ts2, " ".join("%.2f" % w for w in ws2)))
    print("  kernel family %d <%d, %d>, kernels %s, plan %s" % (evq["kernel_family"], evq["kernel_size"], evq["kernel_band"], plan["last_kernels"]["object"],
                                                                json.dumps(plan["sampled_controls"])))
    times, fold = jq.control_sample_times(p, wa), np.zeros(pcof.size)
    for j0 in range(0, nt, 2048):      # B' G in blocks of time points (the dense B of cnot3 would take gigabytes)
        fold += jq.spline_sample_matrix(p, pcof.size, times[j0:j0 + 2048]).T @ rq[1][:, j0:j0 + 2048].ravel(order="F")
    print("  samples / spline wall time %.3f; events total %.3f, generate %.3f; objective bit-identical: %s; |B' G - totalgrad| / |totalgrad| = %.2e" % (
        tq / ts, evq["ms_total"] / evs["ms_total"], evq["ms_generate"] / evs["ms_generate"], rq[0] == rs[0] and rq[2] == rs[2] and rq[3] == rs[3],
        np.linalg.norm(fold - rs[1]) / np.linalg.norm(rs[1])))
    wa.close()


if __name__ == "__main__":
    print(_lib.load().jq_version().decode())
    for name in (sys.argv[1:] or ["swap02", "cnot3"]):
        run(name)
        print()
