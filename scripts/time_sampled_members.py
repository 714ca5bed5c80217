#!/usr/bin/env python3
"""Times jq_eval_f_g_grad_samples_members on swap02, cnot2 (row-lane kernels) and cnot3 (cooperative-quad kernels) at full length, 8 members
with amplitude mixes AND member drifts, the table = control_samples(pcof), against three things:
  (a) loop     what a caller writes without the call, on the same handle: per member params.Hconst = H_i (jq_update_hconst), the table
               mixed on the host, jq_traceobjgrad_samples, the gradient folded back with C_i' and the weighted sum on the host;
  (b) splines  jq_eval_f_g_grad_members on the same members with pcof: the same sweeps, so what tables cost shows in ms_generate and in
               the host time outside the library's events, which are printed apart;
  (c) fetch    jq_traceobjgrad_samples_members and the weighted sum of its nmember gradient tables on the host, against the sum on the
               device (the ensemble call).
Members: the drifts of scripts/time_drift_hvp.py (Hconst + eps_i diag(0.01 j), eps_i the 8 Gauss-Legendre nodes on [-0.05, 0.05], with
their weights) and the amplitude mixes diag(1 + 0.05 r_i), r_i standard normal from default_rng(16).  Wall-clock times of the Python calls
after a warm-up call of each: the median of 3 calls, the candidates taking turns (call, loop, splines, fetch, call, ...), with the
spread (min .. max) next to it; the library's own event times of the last call next to them.  Arguments: the problems to run (default:
swap02 cnot2 cnot3).  Prints the body of profiles/sampled_members_timing.txt.  Needs a GPU."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import juqbox_jl_amd as jq  # noqa: E402
from time_drift_hvp import NMEMBER, members  # noqa: E402


def alternating(calls, runs=3):
    """{name: (median ms, min, max, last result, the library's timing record of the last call)} of the calls taking turns, after one
    warm-up call each"""
    for name, (call, wa) in calls.items():
        call()
    times = {name: [] for name in calls}
    last = {}
    for _ in range(runs):
        for name, (call, wa) in calls.items():
            t0 = time.perf_counter()
            r = call()
            times[name].append(1e3 * (time.perf_counter() - t0))
            last[name] = (r, wa.last_timing())
    return {name: (float(np.median(t)), min(t), max(t)) + last[name] for name, t in times.items()}


def run(name):
    p, info = getattr(jq.cases, name)()
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))["pcof0"])
    H, w = members(p)
    Nc = p.Ncoupled
    Cm = jq.amplitude_mix(1.0 + 0.05 * np.random.default_rng(16).standard_normal((NMEMBER, Nc)))
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    pq = jq.control_samples(pcof, p, wa)
    nt = pq.shape[1]
    print("%s: Ntot %d, N %d, %d controls, %d time steps, Neumann order %d, objFuncType %d; %d members; a table has %d x %d samples (%.2f MB per gradient)" % (
        name, p.Ntot, p.N, Nc, p.nsteps, p.linear_solver.max_iter, p.objFuncType, NMEMBER, pq.shape[0], nt, pq.size * 8 / 1e6))
    own = np.array(p.Hconst, dtype=np.float64, order="F", copy=True)
    two = p.objFuncType != 1

    def call():
        return jq.eval_f_g_grad_samples_members(pq, p, wa, w, Hconsts=H, ctrl_mix=Cm)

    def loop():
        inf = leak = 0.0
        ig, lg = np.zeros_like(pq), np.zeros_like(pq)
        try:
            for i in range(NMEMBER):
                C = Cm[:, :, i]
                p.Hconst = H[:, :, i]
                M = np.kron(C, np.eye(2))      # (row 2 l + s of the mixed table = sum_k C[l, k] row 2 k + s)
                r = jq.traceobjgrad_samples(M @ pq, p, wa, True)
                inf, leak = inf + w[i] * r[2], leak + w[i] * r[3]
                ig += w[i] * (M.T @ r[5])
                if two:
                    lg += w[i] * (M.T @ r[6])
        finally:
            p.Hconst = own
        return dict(infidelity=inf, leak=leak, infid_grad=ig, leak_grad=lg)

    def splines():
        return jq.eval_f_g_grad_members(pcof, p, wa, w, Hconsts=H, ctrl_mix=Cm)

    def fetch():
        r = jq.traceobjgrad_samples_members(pq, p, wa, Hconsts=H, ctrl_mix=Cm)
        return dict(infid_grad=np.tensordot(w, r[5], axes=1), leak_grad=np.tensordot(w, r[6], axes=1) if two else None)

    res = alternating({"call": (call, wa), "loop": (loop, wa), "splines": (splines, wa), "fetch": (fetch, wa)})
    plan = wa.plan_info()
    fmt = lambda k: "%.2f ms wall (%.2f .. %.2f)" % res[k][:3]
    ev = lambda k: "the library's events %.2f ms (generate %.2f, forward %.2f in %d launches, backward %.2f in %d launches), outside them %.2f ms" % (
        res[k][4]["ms_total"], res[k][4]["ms_generate"], res[k][4]["ms_forward"], res[k][4]["n_forward_launches"], res[k][4]["ms_backward"],
        res[k][4]["n_backward_launches"], res[k][0] - res[k][4]["ms_total"])
    print("  the call: %s; %s; plan %s, kernels %s" % (fmt("call"), ev("call"), json.dumps(plan["sampled_batch"]), plan["last_kernels"]["object"]))
    print("  (a) the caller's loop over the members on the same handle: %s (its last member: %s)" % (fmt("loop"), ev("loop")))
    print("  (b) jq_eval_f_g_grad_members with pcof, the same members: %s; %s" % (fmt("splines"), ev("splines")))
    print("  (c) jq_traceobjgrad_samples_members + the weighted sum of %d tables on the host: %s; %s" % (NMEMBER, fmt("fetch"), ev("fetch")))
    c, l = res["call"][3], res["loop"][3]
    print("  the call is %.2f x faster than (a), takes %.2f x the time of (b), and is %.2f x faster than (c)" % (
        res["loop"][0] / res["call"][0], res["call"][0] / res["splines"][0], res["fetch"][0] / res["call"][0]))
    print("  |infid_grad - (a)'s| / |infid_grad| = %.2e, - (c)'s %.2e; infidelity %.15e, (a)'s %.15e" % (
        np.linalg.norm(c["infid_grad"] - l["infid_grad"]) / np.linalg.norm(c["infid_grad"]),
        np.linalg.norm(c["infid_grad"] - res["fetch"][3]["infid_grad"]) / np.linalg.norm(c["infid_grad"]), c["infidelity"], l["infidelity"]))
    wa.close()


if __name__ == "__main__":
    for arg in (sys.argv[1:] or ["swap02", "cnot2", "cnot3"]):
        run(arg)
        print()
