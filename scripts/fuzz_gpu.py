"""Randomised GPU-vs-oracle stress (development aid, not part of the test-suite): draws problem sizes, structures,
kernel-family overrides, chunkings and ensemble sizes and compares objective / gradient with the CPU oracle.
usage: fuzz_gpu.py [n_cases] [seed]      (FUZZ_FOCUS=imr_cq: only the cooperative-quad implicit-midpoint kernels;
FUZZ_FOCUS=wfull_cq: only the 4 x 4 x n structure with full leakage weights that fit the four slots of the cooperative-quad kernels --
real rank <= 4, complex rank <= 2 -- and ensembles of 1 .. 140 samples: three / two / one workgroup per quad, the quad-layout fallback;
FUZZ_DUMP=<file.json>: DIFFERENTIAL mode -- no oracle; every draw's results are written to the file (exact decimal representations), to be
compared with the same run of ANOTHER BUILD of the library (JQ_LIB; scripts/cmp_fuzz_dumps.py): what found nothing in round 5, after
the oracle-based run had found an object that hipcc miscompiles in one register form;
FUZZ_FOCUS=slab: every draw forced onto the slab kernels (family 0: no cooperative, quad-layout, lane or row-lane kernels) -- the
objects k_*, j_*, w_* of every size and band, which small ensembles otherwise rarely reach; FUZZ_FOCUS=wfull: full weights in every
Stormer-Verlet draw;
FUZZ_UNCOUPLED=<share>: the share of the Stormer-Verlet draws that are converted to UNCOUPLED controls (tests/uncoupled_problem.py
to_uncoupled: Hunc_ops[q] = Hsym_ops[q] or Hanti_ops[q] -- all symmetric, all antisymmetric or mixed, a third each -- and Rfreq with
0.2 <= |Rfreq| <= 2); default 0.15.  The conversion draws from a generator of its own, seeded by (seed, draw), so the other 85 % of a
seed's draws -- and everything else about the converted ones -- are what they were before uncoupled draws existed)"""
import os, sys, time
import numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import juqbox_jl_amd as jq
from oracle.oracle import Oracle
from test_gpu_random import random_problem
from uncoupled_problem import to_uncoupled


RTOL, ATOL = 1e-10, 1e-14      # the reference's tolerances (test/evalGrad.jl:4-5): the ONLY ones this script and tests/test_gpu_fuzz.py use
UNCOUPLED_SHARE = 0.15         # of the Stormer-Verlet draws (implicit midpoint: the gradient with uncoupled controls is refused); FUZZ_UNCOUPLED overrides
IMR_TOL = 1e-12                # fixed-point solver of the implicit-midpoint draws: the reference's own test setting (test/runtests.jl:69-70)


def ref_err(value, ref):
    """0 when the pair passes the reference's ABSOLUTE criterion (norm of the difference below atol), else the relative difference:
    a draw passes iff every quantity's ref_err is below RTOL -- exactly reference_pass of tests/conftest.py.
    (Rounds 3 - 5 divided the error of the LEAK gradient by the norm of the INFIDELITY gradient and floored the leak at 1e-3: the one
    draw above 1e-10 on record -- profiles/r05_fuzz_wfull_600.txt:529, 1.8e-10 -- was that ratio, a leak gradient of O(1) with a
    relative error of 1e-16 next to an infidelity gradient of 2e-6; profiles/r06_fuzz_draw528.txt.)"""
    value, ref = np.atleast_1d(np.asarray(value, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    d, nrm = np.linalg.norm(value - ref), np.linalg.norm(ref)
    if d < ATOL:
        return 0.0
    return d / nrm if nrm >= ATOL else float("inf")


def _diag(p, pcof, wa, nodes, weights, shift, oft):
    """FUZZ_DIAG=1 with FUZZ_ONLY: where does the error of a replayed draw sit, and how well conditioned is the draw itself?  Per sample:
    GPU against oracle; the oracle against ITSELF after a one-ulp perturbation of pcof (what rounding alone does to this problem); the
    growth of the state norm (a truncated Neumann series is not unitary: growth amplifies every rounding difference)."""
    rng = np.random.default_rng(7)
    H0 = p.Hconst.copy()
    pert = pcof * (1.0 + 2.0 ** -52 * rng.choice([-1.0, 1.0], pcof.size))
    rows = []
    for k, (ep, wq) in enumerate(zip(nodes, weights)):
        if wq == 0.0 or k >= int(os.environ.get("FUZZ_DIAG_MAX", "6")):
            continue
        p.Hconst = H0 + np.diag(ep * shift)
        o = Oracle(p, use_sparse=False)
        r = o.traceobjgrad(pcof, final_state=True)
        r2 = o.traceobjgrad(pert)
        r3 = Oracle(p, use_sparse=True).traceobjgrad(pcof)
        fs = r["final_state"]
        growth = float(np.max(np.sqrt(np.sum(fs[:, :, 0] ** 2 + fs[:, :, 1] ** 2, axis=0))))
        p.Hconst = H0
        one = np.zeros(len(nodes)); one[k] = 1.0
        jq.eval_f_g_grad(pcof, p, wa, nodes, one, True, shift=shift)
        gn = max(np.linalg.norm(r["infidelgrad"]), 1e-300)
        rows.append((k, abs(p.last_infidelity - r["primaryobjf"]) / abs(r["primaryobjf"]), abs(p.last_leak - r["secondaryobjf"]) / max(abs(r["secondaryobjf"]), 1e-3),
                     np.linalg.norm(p.last_infidelity_grad - r["infidelgrad"]) / gn,
                     np.linalg.norm(r2["infidelgrad"] - r["infidelgrad"]) / gn, np.linalg.norm(r3["infidelgrad"] - r["infidelgrad"]) / gn, growth,
                     r["primaryobjf"], r["secondaryobjf"], gn))
    print("   sample | GPU-oracle: infid, leak, grad | oracle one-ulp pcof: grad | oracle sparse-order: grad | max column norm at T | infid leak |grad|")
    for row in rows:
        print("   %5d  | %.2e %.2e %.2e | %.2e | %.2e | %.3e | %.4e %.4e %.3e" % row, flush=True)


def run(n_cases=50, seed=1, verbose=True):
    """Returns (worst relative error, number of cases really compared with the oracle -- combinations without kernels
    (JQ_EUNSUPPORTED) are skipped and NOT counted)."""
    nonlocal_print = print if verbose else (lambda *a, **k: None)
    rng = np.random.default_rng(seed)
    worst = 0.0
    compared = 0
    n_unconv = 0
    t0 = time.time()
    case = -1
    while compared < n_cases and case + 1 < 2 * n_cases:     # draws without kernels (JQ_EUNSUPPORTED) are replaced, not counted
        case += 1
        Ntot = int(rng.choice([2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 14, 16, 17, 20, 31, 32, 33, 40, 48, 50, 63, 64, 65, 80, 81, 95, 96, 100, 112, 128, 150, 200, 200, 270, 300]))      # (round 6: beyond 256 -- the run-time-size kernels)
        N = int(rng.integers(1, min(Ntot, 16) + 1))
        if Ntot >= 17 and rng.random() < 0.12:      # (round 4: more than 16 columns per evaluation, both integrators)
            N = int(rng.integers(17, min(Ntot, 32) + 1))
        Nc = int(rng.integers(1, 5)) if rng.random() < 0.75 else int(rng.integers(5, 10))      # (round 3: control groups)
        Nfreq = int(rng.integers(1, 4))
        nsteps = int(rng.integers(3, 24))
        m = int(rng.integers(0, 8))
        oft = int(rng.integers(1, 4))
        structure = rng.choice([False, True, "od", "t4", "t4"]) if Ntot > 16 else rng.choice([False, True, "t4"])
        structure = structure if isinstance(structure, str) else bool(structure)
        imr = bool(rng.random() < 0.3) and (Ntot <= 16 or structure is not False)
        if Ntot > 96:      # 4 x 4 x 7 / 4 x 4 x 8 on the NT = 7, 8 instantiations (N = 1, 2, 4); anything else at this size: cooperative kernels
            imr = imr and (structure != "t4" or N in (1, 2, 4) or N > 16)
        if Ntot > 256:     # (the implicit-midpoint path is implemented up to Ntot = 256; a small batch: the CPU oracle pays Ntot^2 per product and column)
            imr = False
            N = min(N, 6)
        if os.environ.get("FUZZ_FOCUS") == "imr_cq":      # the cooperative-quad implicit-midpoint kernels: 4 x 4 x n structure, N = 4
            Ntot, N, structure, imr = int(rng.choice([32, 48, 64, 80, 96])), 4, "t4", True
        focus_w = os.environ.get("FUZZ_FOCUS") == "wfull_cq"
        if focus_w:
            Ntot, N, structure, imr = int(rng.choice([16, 32, 48, 64, 80, 96, 112])), int(rng.choice([1, 2, 3, 4, 4, 4, 8])), "t4", False
            Nc = int(rng.integers(1, 5))
        env = {}
        if rng.random() < 0.5:
            env["JQ_CHUNK_STEPS"] = str(int(rng.integers(1, nsteps + 1)))
        mode = rng.choice(["auto", "JQ_COOP_MAX=0", "JQ_LANE=0", "JQ_ROWLANE_MAX=0", "JQ_OD=0", "JQ_QUAD=0", "JQ_WINDOW=0", "JQ_T4=0"])
        if os.environ.get("FUZZ_FOCUS") in ("imr_cq", "wfull_cq"):
            mode = "auto"
        elif structure == "t4" and rng.random() < 0.5:      # the JQ_BW_T4 slab kernels instead of the quad-layout / cooperative ones
            env["JQ_QUAD"] = "0"
            env["JQ_COOP_MAX"] = "0"
            env["JQ_LANE"] = "0"
        if os.environ.get("FUZZ_FOCUS") == "slab":
            imr = False
            mode = "auto"
            env.update({"JQ_COOP_MAX": "0", "JQ_QUAD": "0", "JQ_CQ": "0", "JQ_DQ": "0", "JQ_LANE": "0", "JQ_ROWLANE_MAX": "0"})
        if imr and mode == "JQ_COOP_MAX=0":
            mode = "auto"           # (the cooperative kernels are the only implicit-midpoint path for Ntot > 16)
        if mode != "auto":
            k, v = mode.split("=")
            env[k] = v
        p, pcof = random_problem(jq, rng, Ntot, N, Nc, Nfreq, nsteps, m, oft, structure)
        unc_rng = np.random.default_rng([seed, case, 0x756E63])      # (its own stream: the main one draws what it always drew)
        kinds = None
        if not imr and unc_rng.random() < float(os.environ.get("FUZZ_UNCOUPLED", UNCOUPLED_SHARE)):
            kinds = ("s" * Nc, "a" * Nc, "".join(unc_rng.choice(["s", "a"], Nc)))[int(unc_rng.integers(0, 3))]
            p = to_uncoupled(jq, p, kinds, unc_rng)
        jac = (not imr) and N <= 16 and rng.random() < 0.15      # (round 3: the Jacobi solver with a loose tolerance -- per-sample convergence;
        #                                                             N > 16 converges per 16-column part: O(tol), tests/test_gpu_round4.py)
        if focus_w:
            jac = False
        if os.environ.get("FUZZ_FOCUS") == "wfull":
            jac = False
        # (round 6: full weights also with the Jacobi solver, and ranks beyond 16)
        wfull = (not imr) and (focus_w or os.environ.get("FUZZ_FOCUS") == "wfull" or rng.random() < (0.3 if os.environ.get("FUZZ_FOCUS") == "slab" else 0.12))      # (round 4: full / complex leakage weights, rank 1 .. 4)
        if wfull:
            nf = int(rng.integers(1, 5))
            if not focus_w and Ntot >= 20 and rng.random() < 0.12:
                nf = int(rng.integers(17, min(Ntot, 24) + 1))
            cplx_w = rng.random() < (0.5 if focus_w else 0.7)
            if focus_w and cplx_w:
                nf = int(rng.integers(1, 3))
            fs = rng.standard_normal((Ntot, nf)) + (1j * rng.standard_normal((Ntot, nf)) if cplx_w else 0)
            fs = fs / np.linalg.norm(fs, axis=0)
            Wf = sum((0.5 + rng.random()) * np.outer(fs[:, k], np.conj(fs[:, k])) for k in range(nf))
            if not os.environ.get("FUZZ_NOWEIGHTS"):
                p.wmat_real, p.wmat_imag = np.asfortranarray(Wf.real.copy()), np.asfortranarray(Wf.imag.copy())
            if os.environ.get("FUZZ_ONLY") and not os.environ.get("FUZZ_DRY"):
                print("   weights: %d states, complex %s" % (nf, cplx_w if focus_w else "?"), flush=True)
        jtol = float(10.0 ** rng.integers(-12, -4))
        if imr:
            p.Integrator_id = jq.Implicit_Midpoint
            p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=80, tol=IMR_TOL, nrhs=N)
            p.wmat = p.wmat_real.copy()
        elif jac:
            p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER, max_iter=60, tol=jtol, nrhs=N)
        replan = rng.random() < 0.1                  # (round 3: a drift outside the planned structure before the evaluation)
        only = os.environ.get("FUZZ_ONLY")           # replay ONE case of a run (same n_cases and seed): the others only draw
        if only and os.environ.get("FUZZ_DRY") and case in [int(x) for x in only.split(",")]:
            print("%d Ntot=%d N=%d Nc=%d Nf=%d steps=%d m=%d oft=%d %s imr=%s mode=%s env=%s replan=%s uncoupled=%s" % (
                case, Ntot, N, Nc, Nfreq, nsteps, m, oft, structure, imr, mode, env, replan, kinds), flush=True)
        if only and (os.environ.get("FUZZ_DRY") or case not in [int(x) for x in only.split(",")]):
            if replan:
                rng.standard_normal((Ntot, Ntot))
            nq = int(rng.choice([1, 2, 5, 17, 70, 100, 140])) if focus_w else int(rng.choice([1, 2, 5, 17, 70]))
            nq = min(nq, 2) if Ntot > 256 else min(nq, 5) if Ntot >= 128 else nq      # (the CPU oracle pays Ntot^2 per product, column and node)
            rng.standard_normal(nq), rng.random(nq)
            if focus_w and nq > 20:
                rng.choice(nq, 4, replace=False)
            rng.standard_normal(Ntot)
            compared += 1        # (a replay of a run without unsupported draws; with them the indices shift)
            continue
        if os.environ.get("FUZZ_NOCHUNK"):      # (bisection aids for a replayed case)
            env.pop("JQ_CHUNK_STEPS", None)
        wa = (jq.Working_Arrays_M_HIP if imr else jq.Working_Arrays_HIP)(p, pcof.size, options=env)      # (historic spelling: {"JQ_QUAD": "0"} = option quad=0)
        if replan:
            D = rng.standard_normal((Ntot, Ntot))
            if not os.environ.get("FUZZ_NOREPLAN"):
                p.Hconst = p.Hconst + 0.02 * (D + D.T)
            if os.environ.get("FUZZ_REPLAN_FIRST"):      # (the same drift, but known to the handle before the weights are pushed again)
                wa.close()
                wa = jq.Working_Arrays_HIP(p, pcof.size, options=env)
        nq = int(rng.choice([1, 2, 5, 17, 70, 100, 140])) if focus_w else int(rng.choice([1, 2, 5, 17, 70]))
        nq = min(nq, 2) if Ntot > 256 else min(nq, 5) if Ntot >= 128 else nq      # (the CPU oracle pays Ntot^2 per product, column and node)
        nodes, weights = 0.05 * rng.standard_normal(nq), rng.random(nq)
        if focus_w and nq > 20:      # (the oracle loops over the samples: a few one-hot weights)
            hot = rng.choice(nq, 4, replace=False)
            w0 = weights.copy()
            weights[:] = 0.0
            weights[hot] = w0[hot]
        shift = 0.05 * rng.standard_normal(Ntot); shift[0] = 0.0
        dump_path = os.environ.get("FUZZ_DUMP")
        if dump_path:      # differential mode: this build's numbers only
            try:
                jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
                rec = [repr(float(p.last_infidelity)), repr(float(p.last_leak)), [repr(float(x)) for x in p.last_infidelity_grad],
                       [repr(float(x)) for x in p.last_leak_grad] if oft != 1 else [], int(wa.last_timing()["kernel_family"])]
            except RuntimeError as e:
                rec = ["unsupported" if "error -3" in str(e) else "error: " + str(e)[-80:]]
            dumped = globals().setdefault("_dumped", {})
            dumped[str(case)] = rec
            compared += 1
            wa.close()
            if compared == n_cases or only:      # (a replayed draw: written at once)
                import json
                json.dump(dumped, open(dump_path, "w"))
                nonlocal_print("%d draws written to %s in %.0f s" % (compared, dump_path, time.time() - t0))
            continue
        orc = Oracle(p, use_sparse=False)
        inf = leak = 0.0
        gi, gl = np.zeros(pcof.size), np.zeros(pcof.size)
        H0 = p.Hconst.copy()
        for ep, wq in zip(nodes, weights):
            if wq == 0.0:
                continue
            p.Hconst = H0 + np.diag(ep * shift)
            o2 = Oracle(p, use_sparse=False)
            r = o2.traceobjgrad_imr(pcof, 80, IMR_TOL) if imr else o2.traceobjgrad(pcof)
            inf += wq * r["primaryobjf"]; leak += wq * r["secondaryobjf"]; gi += wq * r["infidelgrad"]; gl += wq * r["leakgrad"]
        p.Hconst = H0
        # implicit midpoint: a draw whose fixed-point iteration does not converge within its 80 iterations (large dt ||H||: every
        # iteration amplifies rounding differences) is reported but not held to the tolerance
        # (advisor, round 3: such a draw was never flagged whatever its error -- a genuinely wrong result would have passed.  It is
        #  now held to a LOOSE bound: 1e-4, or 100 x the oracle's own change between 79 and 80 iterations, whichever is larger.)
        unconv, loose = False, 0.0
        if imr:
            ra, rb = orc.traceobjgrad_imr(pcof, 80, IMR_TOL), orc.traceobjgrad_imr(pcof, 79, IMR_TOL)
            own = abs(ra["primaryobjf"] - rb["primaryobjf"]) / max(1.0, abs(ra["primaryobjf"]))
            unconv = own > 1e-10
            loose = max(1e-4, 100.0 * own)
        try:
            jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
        except RuntimeError as e:
            if "error -3" in str(e):     # JQ_EUNSUPPORTED: a combination (usually forced by the env override) without kernels
                nonlocal_print("%3d Ntot=%2d N=%2d %s %-18s unsupported: %s" % (case, Ntot, N, "IMR" if imr else "SV ", mode, str(e)[-70:]), flush=True)
                wa.close()
                continue
            raise
        fam = wa.last_timing()["kernel_family"]
        # the reference's own criterion (test/evalGrad.jl:43-67), per quantity: |x - ref| < atol = 1e-14, or |x - ref| / |ref| < rtol = 1e-10
        e1, e2, e3 = ref_err(p.last_infidelity, inf), ref_err(p.last_leak, leak), ref_err(p.last_infidelity_grad, gi)
        e4 = ref_err(p.last_leak_grad, gl) if oft != 1 else 0.0
        err = max(e1, e2, e3, e4)
        if os.environ.get("FUZZ_ONLY"):
            print("   infidelity %.3e leak %.3e (values %.6e / %.6e) grad %.3e leak grad %.3e" % (e1, e2, p.last_leak, leak, e3, e4), flush=True)
            if os.environ.get("FUZZ_DIAG") and not imr:
                _diag(p, pcof, wa, nodes, weights, shift, oft)
        if not unconv:
            worst = max(worst, err)
        else:
            n_unconv += 1
            if err >= loose:
                worst = max(worst, err)      # above even the loose bound: a genuine mismatch
        compared += 1
        flag = (("   (fixed-point iteration not converged: loose bound %.0e)" % loose) if err < loose else "   <<<<<< MISMATCH (unconverged draw, above its loose bound)") \
            if unconv else ("" if err < RTOL else "   <<<<<< MISMATCH")
        nonlocal_print("%3d Ntot=%2d N=%2d Nc=%d Nf=%d steps=%2d m=%d oft=%d %-5s %s nq=%2d fam=%d %-18s env=%s%s%s%s err=%.1e%s" % (
            case, Ntot, N, Nc, Nfreq, nsteps, m, oft, structure, "IMR" if imr else ("JAC" if jac else ("SVW" if wfull else "SV ")), nq, fam, mode,
            env.get("JQ_CHUNK_STEPS", "-"), " replan" if replan else "", (" tol=%.0e" % jtol) if jac else "", (" Hunc=" + kinds) if kinds else "", err, flag), flush=True)
        wa.close()
    nonlocal_print("worst relative error %.2e over %d compared cases (of %d drawn; %d implicit-midpoint draws with an unconverged fixed-point "
                   "iteration held to their loose bound only) in %.0f s" % (worst, compared, n_cases, n_unconv, time.time() - t0))

    return worst, compared


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 50, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
