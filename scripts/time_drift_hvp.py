#!/usr/bin/env python3
"""Times jq_eval_f_g_grad_drifts_hvp on swap02, cnot2 and cnot3 at full length, 8 members, 1 and 16 directions, three ways:
  concurrent  the call on a default handle (lane / row-lane / quad route: every wave reads its own member's operator stream);
  sequential  the same call on a handle with option lane=0 (swap02, cnot2) / quad=0 (cnot3): the members one after the other;
  loop        what a caller writes without the call: per member params.Hconst = H_i (jq_update_hconst) and jq_traceobjgrad_hvp, on a
              default handle, the handle's own drift put back at the end.
Members: Hconst + eps_i diag(0.01 j), eps_i the 8 Gauss-Legendre nodes on [-0.05, 0.05], with their weights -- inside every plan's
pattern.  Wall-clock times of the Python calls (the loop has host work between its launches that HIP events of one call do not see),
after a warm-up call: the best of two calls (concurrent), one call (sequential, loop; cnot3:loop1: no warm-up, a call takes 20 s); the
library's own event time of the concurrent call next to it.  Arguments: the problems to run (default: swap02 cnot2 cnot3);
"cnot3:loop1" times the cnot3 loop and the sequential route with ONE member and reports 8 x that figure, marked as such (the members
of both run one after the other and do not interact; 8 members of either take minutes per call).
Prints the body of profiles/drift_hvp_timing.txt.  Needs a GPU."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import juqbox_jl_amd as jq  # noqa: E402

NMEMBER = 8


def members(p, n=NMEMBER):
    x, w = np.polynomial.legendre.leggauss(n)
    H0 = np.asarray(p.Hconst, dtype=np.float64)
    H = np.stack([H0 + np.diag(0.05 * e * 0.01 * np.arange(p.Ntot)) for e in x], axis=2)
    return np.asfortranarray(H), 0.5 * w


def best(call, runs, warm=True):
    if warm:
        call()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r = call()
        out.append((1e3 * (time.perf_counter() - t0), r))
    return min(out, key=lambda x: x[0])


def run(name, short):
    p, info = getattr(jq.cases, name)()
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))["pcof0"])
    H, w = members(p)
    own = np.array(p.Hconst, dtype=np.float64, order="F", copy=True)
    off = {"quad": 0} if p.Ntot > 16 else {"lane": 0}
    print("%s: Ntot %d, N %d, %d time steps, Neumann order %d, %d coefficients, objFuncType %d; %d members" % (
        name, p.Ntot, p.N, p.nsteps, p.linear_solver.max_iter, pcof.size, p.objFuncType, NMEMBER))
    wa, ws = jq.Working_Arrays_HIP(p, pcof.size), jq.Working_Arrays_HIP(p, pcof.size, options=off)
    g = jq.traceobjgrad(pcof, p, wa, False, True)[1]
    rng = np.random.default_rng(15)
    nm = 1 if short else NMEMBER
    for ndir in (1, 16):
        D = np.stack([g / np.linalg.norm(g)] + [rng.standard_normal(pcof.size) for _ in range(ndir - 1)], axis=1)
        tc, rc = best(lambda: jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, H, w), 2)
        plan, ev = wa.plan_info(), wa.last_timing()
        ts, rs = best(lambda: jq.eval_f_g_grad_drifts_hvp(pcof, D, p, ws, H[:, :, :nm], w[:nm]), 1, not short)
        plans = ws.plan_info()

        def loop():
            hv = np.zeros((pcof.size, ndir))
            for i in range(nm):
                p.Hconst = H[:, :, i]
                r = jq.traceobjgrad_hvp(pcof, D, p, wa)
                hv += w[i] * (r["hv_infid"] if p.objFuncType != 1 else r["hv"])
            p.Hconst = own
            wa.sync_params()
            return hv
        tl, hl = best(loop, 1, not short)
        scale = NMEMBER / nm
        mark = " (8 x the time of ONE member)" if short else ""
        print("  ndir %2d concurrent: %.2f ms wall, %.2f ms by the library's events (forward %.2f ms in %d launches, backward %.2f ms in %d launches); plan %s, kernels %s" % (
            ndir, tc, ev["ms_total"], ev["ms_forward"], ev["n_forward_launches"], ev["ms_backward"], ev["n_backward_launches"], json.dumps(plan["drift_hvp"]),
            plan["last_kernels"]["object"]))
        print("  ndir %2d sequential (options %s): %.2f ms wall%s; plan %s" % (ndir, json.dumps(off), ts * scale, mark, json.dumps(plans["drift_hvp"])))
        print("  ndir %2d loop of jq_update_hconst + jq_traceobjgrad_hvp: %.2f ms wall%s" % (ndir, tl * scale, mark))
        print("  ndir %2d: concurrent route %.1f x faster than the loop, %.1f x faster than the sequential route" % (ndir, tl * scale / tc, ts * scale / tc))
        if not short:
            print("           |hv_infid - the loop's| / |hv_infid| = %.2e, against the sequential route %.2e" % (
                np.linalg.norm(rc["hv_infid"] - hl) / np.linalg.norm(hl), np.linalg.norm(rc["hv_infid"] - rs["hv_infid"]) / np.linalg.norm(rs["hv_infid"])))
    wa.close()
    ws.close()


if __name__ == "__main__":
    for arg in (sys.argv[1:] or ["swap02", "cnot2", "cnot3"]):
        name, _, mode = arg.partition(":")
        run(name, mode == "loop1")
        print()
