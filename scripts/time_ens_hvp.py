#!/usr/bin/env python3
"""Times jq_eval_f_g_grad_hvp with the library's own HIP events (jq_last_timing), two calls after a warm-up each:
  (a) swap02 at full length, one node, 1 and 16 directions, against jq_traceobjgrad_hvp on the same handle in the same process;
  (b) the SWAP-02 risk-neutral configuration (cases.swap02_rn, 512 nodes), 1 and 16 directions, against jq_eval_f_g_grad on the same
      handle;
  (c) cnot2 (Ntot 12: the row-lane route) at full length with 1 and with 3 nodes, 1 and 16 directions, on a default handle and on one with
      option lane=0 (the sequential route) -- run with JQ_LIB=<the parent commit's library> the same calls give the baseline;
  (d) cnot2 over 512 nodes (the ensemble scripts/time_rl_ens.py times: Gauss-Legendre nodes on [-0.05, 0.05], shift 0.01 j), 1 and 16
      directions, against jq_eval_f_g_grad on the same handle.
  (e) cnot3 (Ntot 96 = 4 x 4 x 6: the quad route) at full length, one node, 1 and 16 directions, on a default handle and on one with
      option quad=0 (the sequential route, which is the parent commit's route for this problem), the relative difference of hv_infid /
      hv_leak between the two, and the multiple of one jq_eval_f_g_grad on the same handle;
  (f) cnot3 over the nodes of cases.cnot3_ensemble (32: 32 column quads per direction), 1 and 16 directions, against jq_eval_f_g_grad on
      the same handle.
Prints the body of profiles/ens_hvp_timing.txt (a, b), of profiles/ens_hvp_rowlane_timing.txt (c, d, kernels) and of
profiles/ens_hvp_quad_timing.txt (e, f, qkernels).  Sections are chosen by letter on the command line (default: a b).  Needs a GPU,
except `kernels` / `qkernels`, which read the build manifest."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import juqbox_jl_amd as jq  # noqa: E402


def timed(call, wa, runs=2):
    call()      # warm-up
    out = []
    for _ in range(runs):
        r = call()
        out.append((wa.last_timing(), r))
    return out


def line(tag, t):
    return "  %s: total %.2f ms, forward %.2f ms in %d launches, backward %.2f ms in %d launches, generate %.2f ms" % (
        tag, t["ms_total"], t["ms_forward"], t["n_forward_launches"], t["ms_backward"], t["n_backward_launches"], t["ms_generate"])


def directions(g, n, ndir, seed):
    rng = np.random.default_rng(seed)
    return np.stack([g / np.linalg.norm(g)] + [rng.standard_normal(n) for _ in range(ndir - 1)], axis=1)


def part_a():
    p, info = jq.cases.swap02()
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "swap02.json")))["pcof0"])
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    g = jq.traceobjgrad(pcof, p, wa, False, True)[1]
    tg = wa.last_timing()
    print("(a) swap02: Ntot %d, N %d, %d time steps, Neumann order %d, %d coefficients, objFuncType %d; one node (eps 0)" % (
        p.Ntot, p.N, p.nsteps, p.linear_solver.max_iter, pcof.size, p.objFuncType))
    print(line("plain adjoint evaluation (family %d)" % tg["kernel_family"], tg))
    for ndir in (1, 16):
        D = directions(g, pcof.size, ndir, 11)
        old = timed(lambda: jq.traceobjgrad_hvp(pcof, D, p, wa), wa)
        new = timed(lambda: jq.eval_f_g_grad_hvp(pcof, D, p, wa), wa)
        plan = wa.plan_info()
        for k, (t, _) in enumerate(old):
            print(line("ndir %2d jq_traceobjgrad_hvp  run %d" % (ndir, k), t))
        for k, (t, _) in enumerate(new):
            print(line("ndir %2d jq_eval_f_g_grad_hvp run %d" % (ndir, k), t))
        bo, bn = min(t["ms_total"] for t, _ in old), min(t["ms_total"] for t, _ in new)
        ro, rn = old[-1][1], new[-1][1]
        hv_new = rn["hv_infid"] + rn["hv_leak"]
        print("ndir %2d: plan %s, kernels %s; %.1f x faster than jq_traceobjgrad_hvp (best of 2: %.2f against %.2f ms); %.2f us per time step and "
              "direction; %.1f x one jq_traceobjgrad" % (ndir, json.dumps(plan["ens_hvp"]), plan["last_kernels"]["object"], bo / bn, bn, bo,
                                                         1e3 * bn / p.nsteps / ndir, bn / tg["ms_total"]))
        print("         |hv - hv of jq_traceobjgrad_hvp| / |hv| = %.2e" % (np.linalg.norm(hv_new - ro["hv"]) / np.linalg.norm(ro["hv"])))
    wa.close()


def part_b():
    p, info = jq.cases.swap02_rn()
    pcof, nodes, weights = np.asarray(info["pcof0"]), info["nodes"], info["weights"]
    wa = jq.Working_Arrays_HIP(p, pcof.size)

    def grad():
        jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True)
        return p.last_infidelity_grad.copy()
    gr = timed(grad, wa)
    g = gr[-1][1]
    bg = min(t["ms_total"] for t, _ in gr)
    print("(b) SWAP-02 risk-neutral: Ntot %d, N %d, %d time steps, Neumann order %d, %d coefficients, objFuncType %d; %d nodes = %d columns" % (
        p.Ntot, p.N, p.nsteps, p.linear_solver.max_iter, pcof.size, p.objFuncType, nodes.size, nodes.size * p.N))
    for k, (t, _) in enumerate(gr):
        print(line("jq_eval_f_g_grad (family %d) run %d" % (t["kernel_family"], k), t))
    for ndir in (1, 16):
        D = directions(g, pcof.size, ndir, 12)
        new = timed(lambda: jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights), wa)
        plan = wa.plan_info()
        for k, (t, _) in enumerate(new):
            print(line("ndir %2d jq_eval_f_g_grad_hvp run %d" % (ndir, k), t))
        bn = min(t["ms_total"] for t, _ in new)
        tb = min(new, key=lambda x: x[0]["ms_total"])[0]
        print("ndir %2d: plan %s; %.1f x one jq_eval_f_g_grad for the call, %.2f x per direction (best of 2: %.2f against %.2f ms); forward %.2f, "
              "backward %.2f us per time step" % (ndir, json.dumps(plan["ens_hvp"]), bn / bg, bn / bg / ndir, bn, bg,
                                                  1e3 * tb["ms_forward"] / p.nsteps, 1e3 * tb["ms_backward"] / p.nsteps))
        r = new[-1][1]
        print("         |infid_grad - eval_f_g_grad's| / |g| = %.2e" % (np.linalg.norm(r["infid_grad"] - g) / np.linalg.norm(g)))
    wa.close()


def cnot2_problem():
    p, info = jq.cases.cnot2()
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "cnot2.json")))["pcof0"])
    return p, pcof, 0.01 * np.arange(p.Ntot)


def gl_nodes(nquad):
    if nquad == 1:
        return np.zeros(1), np.ones(1)
    x, w = np.polynomial.legendre.leggauss(nquad)
    return 0.05 * x, 0.5 * w


def part_c():
    p, pcof, shift = cnot2_problem()
    print("(c) cnot2: Ntot %d, N %d, %d time steps, Neumann order %d, %d coefficients, objFuncType %d; library %s" % (
        p.Ntot, p.N, p.nsteps, p.linear_solver.max_iter, pcof.size, p.objFuncType, os.environ.get("JQ_LIB", "(this build)")))
    for opts in (None, {"lane": 0}):
        wa = jq.Working_Arrays_HIP(p, pcof.size, options=opts)
        for nquad in (1, 3):
            nodes, weights = gl_nodes(nquad)
            jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
            g = p.last_infidelity_grad.copy()
            for ndir in (1, 16):
                D = directions(g, pcof.size, ndir, 13)
                new = timed(lambda: jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift), wa)
                plan = wa.plan_info()
                tag = "options %s, %d node(s), ndir %2d" % (json.dumps(opts), nquad, ndir)
                for k, (t, _) in enumerate(new):
                    print(line("%s run %d" % (tag, k), t))
                tb = min(new, key=lambda x: x[0]["ms_total"])[0]
                nb = max(tb["n_backward_launches"] // max(tb["n_forward_launches"], 1), 1)
                print("%s: plan %s, kernels %s, family %d; best of 2: %.2f ms; forward %.2f, backward %.2f us per time step and pass" % (
                    tag, json.dumps(plan["ens_hvp"]), plan["last_kernels"]["object"], tb["kernel_family"], tb["ms_total"],
                    1e3 * tb["ms_forward"] / p.nsteps, 1e3 * tb["ms_backward"] / p.nsteps / nb))
        wa.close()


def part_d():
    p, pcof, shift = cnot2_problem()
    nodes, weights = gl_nodes(512)
    wa = jq.Working_Arrays_HIP(p, pcof.size)

    def grad():
        jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
        return p.last_infidelity_grad.copy()
    gr = timed(grad, wa)
    g = gr[-1][1]
    bg = min(t["ms_total"] for t, _ in gr)
    print("(d) cnot2 x %d nodes = %d columns (%d waves per direction)" % (nodes.size, nodes.size * p.N, (nodes.size * p.N + 3) // 4))
    for k, (t, _) in enumerate(gr):
        print(line("jq_eval_f_g_grad (family %d) run %d" % (t["kernel_family"], k), t))
    for ndir in (1, 16):
        D = directions(g, pcof.size, ndir, 14)
        new = timed(lambda: jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift), wa)
        plan = wa.plan_info()
        for k, (t, _) in enumerate(new):
            print(line("ndir %2d jq_eval_f_g_grad_hvp run %d" % (ndir, k), t))
        bn = min(t["ms_total"] for t, _ in new)
        tb = min(new, key=lambda x: x[0]["ms_total"])[0]
        print("ndir %2d: plan %s; %.1f x one jq_eval_f_g_grad for the call, %.2f x per direction (best of 2: %.2f against %.2f ms); forward %.2f, "
              "backward %.2f us per time step" % (ndir, json.dumps(plan["ens_hvp"]), bn / bg, bn / bg / ndir, bn, bg,
                                                  1e3 * tb["ms_forward"] / p.nsteps, 1e3 * tb["ms_backward"] / p.nsteps))
        r = new[-1][1]
        print("         |infid_grad - eval_f_g_grad's| / |g| = %.2e" % (np.linalg.norm(r["infid_grad"] - g) / np.linalg.norm(g)))
    wa.close()


def part_kernels():
    """registers, AGPRs, LDS and scratch of the tangent-linear row-lane kernels from the build manifest (dynamic LDS: the host's figures)"""
    m = json.load(open(os.path.join(ROOT, "juqbox.jl_amd", "csrc", "build", "manifest.json")))
    print("kernels (build manifest; LDS is dynamic: 2 rings of 1 536 NPJ bytes, the backward sweep adds 2 Nc images of 128 NPJ bytes):")
    for obj in ("r_12", "r_16"):
        for k in m["objects"][obj]["kernels"]:
            if "rowlane_tl" in k["name"]:
                print("  %s %s: %d VGPRs, %d AGPRs, %d SGPRs, scratch %d bytes, static LDS %d bytes, occupancy %d" % (
                    obj, k["name"], k["vgprs"], k["agprs"], k["sgprs"], k["scratch_bytes"], k["lds_bytes"], k["occupancy"]))


def cnot3_problem():
    p, info = jq.cases.cnot3()
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "cnot3.json")))["pcof0"])
    return p, pcof


def per_step(tb, p):
    nb = max(tb["n_backward_launches"] // max(tb["n_forward_launches"], 1), 1)
    return 1e3 * tb["ms_forward"] / p.nsteps, 1e3 * tb["ms_backward"] / p.nsteps / nb


def part_e():
    p, pcof = cnot3_problem()
    nodes, weights, shift = np.zeros(1), np.ones(1), np.zeros(p.Ntot)
    print("(e) cnot3: Ntot %d, N %d, %d time steps, Neumann order %d, %d coefficients, objFuncType %d; one node (eps 0)" % (
        p.Ntot, p.N, p.nsteps, p.linear_solver.max_iter, pcof.size, p.objFuncType))
    results = {}
    for opts in (None, {"quad": 0}):
        wa = jq.Working_Arrays_HIP(p, pcof.size, options=opts)

        def grad():
            jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
            return p.last_infidelity_grad.copy()
        gr = timed(grad, wa)
        g = gr[-1][1]
        bg = min(t["ms_total"] for t, _ in gr)
        print(line("options %s, jq_eval_f_g_grad (family %d), best of 2" % (json.dumps(opts), gr[-1][0]["kernel_family"]), min(gr, key=lambda x: x[0]["ms_total"])[0]))
        for ndir in (1, 16):
            D = directions(g, pcof.size, ndir, 15)
            new = timed(lambda: jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift), wa, runs=2 if opts is None else 1)
            plan = wa.plan_info()
            tag = "options %s, ndir %2d" % (json.dumps(opts), ndir)
            for k, (t, _) in enumerate(new):
                print(line("%s run %d" % (tag, k), t))
            tb = min(new, key=lambda x: x[0]["ms_total"])[0]
            f, b = per_step(tb, p)
            print("%s: plan %s, kernels %s, family %d; best: %.2f ms = %.1f x one jq_eval_f_g_grad (%.2f ms), %.2f x per direction; forward %.2f, "
                  "backward %.2f us per time step and pass" % (tag, json.dumps(plan["ens_hvp"]), plan["last_kernels"]["object"], tb["kernel_family"],
                                                               tb["ms_total"], tb["ms_total"] / bg, bg, tb["ms_total"] / bg / ndir, f, b))
            results[(opts is None, ndir)] = (tb["ms_total"], new[-1][1])
        wa.close()
    for ndir in (1, 16):
        (tq, rq), (ts, rs) = results[(True, ndir)], results[(False, ndir)]
        rel = lambda k: np.linalg.norm(rq[k] - rs[k]) / max(np.linalg.norm(rs[k]), 1e-300)
        print("ndir %2d: quad route %.2f ms against %.2f ms on the sequential route = %.1f x faster; |hv_infid difference| / |hv_infid| = %.2e, "
              "hv_leak %.2e" % (ndir, tq, ts, ts / tq, rel("hv_infid"), rel("hv_leak")))


def part_f(nquad=32):
    p, pcof = cnot3_problem()
    nodes, weights, shift = jq.cases.cnot3_ensemble(nquad)
    wa = jq.Working_Arrays_HIP(p, pcof.size)

    def grad():
        jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
        return p.last_infidelity_grad.copy()
    gr = timed(grad, wa)
    g = gr[-1][1]
    bg = min(t["ms_total"] for t, _ in gr)
    print("(f) cnot3 x %d nodes (cases.cnot3_ensemble) = %d columns (%d quads per direction)" % (nodes.size, nodes.size * p.N, (nodes.size * p.N + 3) // 4))
    for k, (t, _) in enumerate(gr):
        print(line("jq_eval_f_g_grad (family %d) run %d" % (t["kernel_family"], k), t))
    for ndir in (1, 16):
        D = directions(g, pcof.size, ndir, 16)
        new = timed(lambda: jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift), wa)
        plan = wa.plan_info()
        for k, (t, _) in enumerate(new):
            print(line("ndir %2d jq_eval_f_g_grad_hvp run %d" % (ndir, k), t))
        tb = min(new, key=lambda x: x[0]["ms_total"])[0]
        f, b = per_step(tb, p)
        print("ndir %2d: plan %s; %.1f x one jq_eval_f_g_grad for the call, %.2f x per direction (best of 2: %.2f against %.2f ms); forward %.2f, "
              "backward %.2f us per time step and pass" % (ndir, json.dumps(plan["ens_hvp"]), tb["ms_total"] / bg, tb["ms_total"] / bg / ndir, tb["ms_total"], bg, f, b))
        r = new[-1][1]
        print("         |infid_grad - eval_f_g_grad's| / |g| = %.2e" % (np.linalg.norm(r["infid_grad"] - g) / np.linalg.norm(g)))
    wa.close()


def part_qkernels():
    """registers, AGPRs, LDS and scratch of the tangent-linear quad-layout kernels from the build manifest (dynamic LDS: the host's figures)"""
    m = json.load(open(os.path.join(ROOT, "juqbox.jl_amd", "csrc", "build", "manifest.json")))
    print("kernels (build manifest; LDS is dynamic: 2 rings of 3 time points x (K, S) = 12 images of NT KiB, the backward sweep adds 2 Nc images):")
    for nt in (2, 3, 4, 5, 6):
        for k in m["objects"]["t_%d_7" % nt]["kernels"]:
            print("  t_%d_7 %s: %d VGPRs, %d AGPRs, %d SGPRs, scratch %d bytes, static LDS %d bytes, occupancy %d" % (
                nt, k["name"], k["vgprs"], k["agprs"], k["sgprs"], k["scratch_bytes"], k["lds_bytes"], k["occupancy"]))


if __name__ == "__main__":
    parts = {"a": part_a, "b": part_b, "c": part_c, "d": part_d, "kernels": part_kernels, "e": part_e, "f": part_f, "qkernels": part_qkernels}
    for k, name in enumerate(sys.argv[1:] or ["a", "b"]):
        if k:
            print()
        parts[name]()
