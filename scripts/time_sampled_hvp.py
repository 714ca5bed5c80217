#!/usr/bin/env python3
"""Times jq_eval_f_g_grad_samples_hvp at full length on swap02 (lane route), cnot2 (row-lane) and cnot3 (quad), one node, 1 and 16
directions, in ONE process on the same handle and build, against two things:
  (a) coefficients  jq_eval_f_g_grad_hvp with S = control_samples(pcof) and V = B d: the same sweeps on the same propagator kernels; what
                    differs is the upload of 2 Nc nt doubles per table instead of ncoeff, the generation of the streams from tables and the
                    assembly without a basis (ms_generate of both is printed).  The two calls ALTERNATE, REPS times each after a warm-up
                    call of each; medians and all wall times are printed, and how far B' hv is from the coefficient call's product.
  (b) differences   what a sample-space user has without the call: central differences of two jq_eval_f_g_grad_samples gradients per
                    direction (2 ndir gradient calls; step 1e-6 |S| / |V_j|), timed once after a warm-up call, with its distance from
                    the product.
Wall-clock times are of the Python calls (they end in a stream synchronise inside the library); the library's HIP-event times are
next to them.  Arguments: the problems (default swap02 cnot2 cnot3).  Prints the body of profiles/sampled_hvp_timing.txt.  Needs a GPU."""
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

REPS = 3
BLOCK = 2048      # time points per block of B (the dense B of cnot3 would take gigabytes)


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def fmt(ev):
    return "events: total %.2f ms, generate %.2f ms, forward %.2f ms in %d launches, backward %.2f ms in %d launches" % (
        ev["ms_total"], ev["ms_generate"], ev["ms_forward"], ev["n_forward_launches"], ev["ms_backward"], ev["n_backward_launches"])


def run(name):
    p, info = getattr(jq.cases, name)()
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))["pcof0"])
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    nf, nt = 2 * p.Ncoupled, 2 * p.nsteps + 1
    print("%s: Ntot %d, N %d, %d controls, %d time steps (%d time points, %.2f MB per table), Neumann order %d, %d coefficients, objFuncType %d; one node" % (
        name, p.Ntot, p.N, p.Ncoupled, p.nsteps, nt, 8e-6 * nf * nt, p.linear_solver.max_iter, pcof.size, p.objFuncType))
    S = jq.control_samples(pcof, p, wa)
    times = jq.control_sample_times(p, wa)
    g = jq.traceobjgrad(pcof, p, wa, False, True)[1]
    rng = np.random.default_rng(21)
    jq.eval_f_g_grad_samples(S, p, wa)      # warm-up
    tg = statistics.median([wall(lambda: jq.eval_f_g_grad_samples(S, p, wa))[0] for _ in range(REPS)])
    print("  one jq_eval_f_g_grad_samples (objective and gradient): median %.2f ms wall" % tg)
    for ndir in (1, 16):
        d = np.stack([g / np.linalg.norm(g)] + [rng.standard_normal(pcof.size) for _ in range(ndir - 1)], axis=1)
        V = np.zeros((nf, nt, ndir))
        for j0 in range(0, nt, BLOCK):
            B = jq.spline_sample_matrix(p, pcof.size, times[j0:j0 + BLOCK])
            V[:, j0:j0 + BLOCK, :] = (B @ d).reshape((nf, -1, ndir), order="F")
        coeff = lambda: jq.eval_f_g_grad_hvp(pcof, d, p, wa)
        samp = lambda: jq.eval_f_g_grad_samples_hvp(S, V, p, wa)
        coeff(), samp()      # warm-up of both
        wc, ws = [], []
        for _ in range(REPS):      # alternating
            t, rc = wall(coeff)
            wc.append(t)
            evc, planc = wa.last_timing(), wa.plan_info()
            t, rs = wall(samp)
            ws.append(t)
            evs, plans = wa.last_timing(), wa.plan_info()
        tc, ts = statistics.median(wc), statistics.median(ws)
        fold = np.zeros((pcof.size, ndir))
        for j0 in range(0, nt, BLOCK):
            B = jq.spline_sample_matrix(p, pcof.size, times[j0:j0 + BLOCK])
            fold += B.T @ rs["hv_infid"][:, j0:j0 + BLOCK, :].reshape((-1, ndir), order="F")
        agree = max(np.linalg.norm(fold[:, j] - rc["hv_infid"][:, j]) / np.linalg.norm(rc["hv_infid"][:, j]) for j in range(ndir))
        print("  ndir %2d jq_eval_f_g_grad_hvp          median %.2f ms wall (%s); %s; plan %s" % (
            ndir, tc, " ".join("%.2f" % w for w in wc), fmt(evc), json.dumps(planc["ens_hvp"])))
        print("  ndir %2d jq_eval_f_g_grad_samples_hvp  median %.2f ms wall (%s); %s; plan %s, kernels %s" % (
            ndir, ts, " ".join("%.2f" % w for w in ws), fmt(evs), json.dumps(plans["sampled_hvp"]), plans["last_kernels"]["object"]))
        print("  ndir %2d samples / coefficients: wall %.3f, events total %.3f, generate %.2f ms against %.2f ms; max_j |B' hv_j - coefficient hv_j| / |.| = %.2e" % (
            ndir, ts / tc, evs["ms_total"] / evc["ms_total"], evs["ms_generate"], evc["ms_generate"], agree))

        def differences():
            out = np.zeros((nf, nt, ndir))
            for j in range(ndir):
                h = 1e-6 * np.linalg.norm(S) / np.linalg.norm(V[:, :, j])
                a = jq.eval_f_g_grad_samples(S + h * V[:, :, j], p, wa)
                b = jq.eval_f_g_grad_samples(S - h * V[:, :, j], p, wa)
                out[:, :, j] = (a["infid_grad"] - b["infid_grad"]) / (2.0 * h)
            return out
        if ndir == 1:
            differences()      # warm-up
        tf, fd = wall(differences)
        err = max(np.linalg.norm(fd[:, :, j] - rs["hv_infid"][:, :, j]) / np.linalg.norm(rs["hv_infid"][:, :, j]) for j in range(ndir))
        print("  ndir %2d central differences of jq_eval_f_g_grad_samples gradients (%d calls): %.2f ms wall = %.2f x the call; max_j |difference quotient - hv_j| / |hv_j| = %.1e" % (
            ndir, 2 * ndir, tf, tf / ts, err))
    wa.close()


if __name__ == "__main__":
    print(_lib.load().jq_version().decode())
    for name in (sys.argv[1:] or ["swap02", "cnot2", "cnot3"]):
        run(name)
        print()
