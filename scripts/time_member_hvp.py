#!/usr/bin/env python3
"""Times jq_eval_f_g_grad_members_hvp on swap02, cnot2 and cnot3 at full length, 8 members with amplitude mixes AND member drifts, 1 and
16 directions, against three things:
  (a) sequential  the same call on a handle with option lane=0 (swap02, cnot2) / quad=0 (cnot3): the members one after the other;
  (b) drifts      jq_eval_f_g_grad_drifts_hvp with the same drifts and no mixes on the same handle: what P dpl tangent streams instead
                  of dpl cost (ms_generate, chunk length and rounds of both calls are printed);
  (c) handles     what a caller writes without the call: one handle per member, created on the member's mixed operators
                  Hsym'_k = sum_l C[l, k] Hsym_l, Hanti'_k likewise, and its drift, then jq_eval_f_g_grad_hvp with one node at eps 0 on
                  each (the concurrent route of ONE member) and the weighted sum on the host.  The handles are created before the clock
                  starts; their creation is timed apart.
Members: the drifts of scripts/time_drift_hvp.py (Hconst + eps_i diag(0.01 j), eps_i the 8 Gauss-Legendre nodes on [-0.05, 0.05], with
their weights) and the amplitude mixes diag(1 + 0.05 r_i), r_i standard normal from default_rng(16).  Wall-clock times of the Python
calls after a warm-up call: the best of two calls (the call, drifts, handles), one call (sequential); the library's own event times next
to them.  Arguments: the problems to run (default: swap02 cnot2 cnot3); "cnot3:seq1" times the sequential route with ONE member
without a warm-up call and reports 8 x that figure, marked as such (its members run one after the other and do not interact; 8 members
take minutes per call).  Prints the body of profiles/member_hvp_timing.txt.  Needs a GPU."""
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import juqbox_jl_amd as jq  # noqa: E402
from time_drift_hvp import NMEMBER, best, members  # noqa: E402


def mixed_params(p, C, H):
    """the plain problem a member is: operators mixed with the columns of C, the member's drift"""
    q = copy.copy(p)
    Nc = C.shape[0]
    mixed = lambda ops: [sum(C[l, k] * np.asarray(ops[l], dtype=np.float64) for l in range(Nc)) for k in range(Nc)]
    q.Hsym_ops, q.Hanti_ops = mixed(p.Hsym_ops), mixed(p.Hanti_ops)
    q.Hconst = np.array(H, dtype=np.float64, order="F", copy=True)
    return q


def run(name, short):
    p, info = getattr(jq.cases, name)()
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))["pcof0"])
    H, w = members(p)
    Nc = max(p.Ncoupled, p.Nunc)
    Cm = jq.amplitude_mix(1.0 + 0.05 * np.random.default_rng(16).standard_normal((NMEMBER, Nc)))
    off = {"quad": 0} if p.Ntot > 16 else {"lane": 0}
    print("%s: Ntot %d, N %d, %d controls, %d time steps, Neumann order %d, %d coefficients, objFuncType %d; %d members" % (
        name, p.Ntot, p.N, Nc, p.nsteps, p.linear_solver.max_iter, pcof.size, p.objFuncType, NMEMBER))
    wa, ws = jq.Working_Arrays_HIP(p, pcof.size), jq.Working_Arrays_HIP(p, pcof.size, options=off)
    g = jq.traceobjgrad(pcof, p, wa, False, True)[1]
    tcreate, made = best(lambda: [(q, jq.Working_Arrays_HIP(q, pcof.size)) for q in (mixed_params(p, Cm[:, :, i], H[:, :, i]) for i in range(NMEMBER))], 1, False)
    rng = np.random.default_rng(15)
    nm = 1 if short else NMEMBER
    key = "hv_infid"
    fmt = lambda ev: "%.2f ms by the library's events (generate %.2f ms, forward %.2f ms in %d launches, backward %.2f ms in %d launches)" % (
        ev["ms_total"], ev["ms_generate"], ev["ms_forward"], ev["n_forward_launches"], ev["ms_backward"], ev["n_backward_launches"])
    for ndir in (1, 16):
        D = np.stack([g / np.linalg.norm(g)] + [rng.standard_normal(pcof.size) for _ in range(ndir - 1)], axis=1)
        tc, rc = best(lambda: jq.eval_f_g_grad_members_hvp(pcof, D, p, wa, w, Hconsts=H, ctrl_mix=Cm), 2)
        plan, ev = wa.plan_info(), wa.last_timing()
        td, _ = best(lambda: jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, H, w), 2)
        pland, evd = wa.plan_info(), wa.last_timing()
        ts, rs = best(lambda: jq.eval_f_g_grad_members_hvp(pcof, D, p, ws, w[:nm], Hconsts=H[:, :, :nm], ctrl_mix=Cm[:, :, :nm]), 1, not short)
        plans = ws.plan_info()

        def handles():
            hv = np.zeros((pcof.size, ndir))
            for wi, (q, wq) in zip(w, made):
                hv += wi * jq.eval_f_g_grad_hvp(pcof, D, q, wq)[key]
            return hv
        th, hh = best(handles, 2)
        scale = NMEMBER / nm
        mark = " (8 x the time of ONE member)" if short else ""
        print("  ndir %2d the call: %.2f ms wall, %s; plan %s, kernels %s" % (ndir, tc, fmt(ev), json.dumps(plan["member_hvp"]), plan["last_kernels"]["object"]))
        print("  ndir %2d (a) sequential (options %s): %.2f ms wall%s; plan %s" % (ndir, json.dumps(off), ts * scale, mark, json.dumps(plans["member_hvp"])))
        print("  ndir %2d (b) jq_eval_f_g_grad_drifts_hvp, the same drifts, no mixes: %.2f ms wall, %s; plan %s" % (ndir, td, fmt(evd), json.dumps(pland["drift_hvp"])))
        print("  ndir %2d (c) one handle per member on the mixed operators + jq_eval_f_g_grad_hvp with one node: %.2f ms wall (the 8 handles took %.2f ms to create)" % (
            ndir, th, tcreate))
        print("  ndir %2d: the call is %.1f x faster than (a), takes %.2f x the time of (b), and is %.2f x faster than (c)" % (ndir, ts * scale / tc, tc / td, th / tc))
        print("           |hv_infid - (c)'s| / |hv_infid| = %.2e%s" % (
            np.linalg.norm(rc[key] - hh) / np.linalg.norm(hh),
            "" if short else ", against the sequential route %.2e" % (np.linalg.norm(rc[key] - rs[key]) / np.linalg.norm(rs[key]))))
    for _, wq in made:
        wq.close()
    wa.close()
    ws.close()


if __name__ == "__main__":
    for arg in (sys.argv[1:] or ["swap02", "cnot2", "cnot3"]):
        name, _, mode = arg.partition(":")
        run(name, mode == "seq1")
        print()
