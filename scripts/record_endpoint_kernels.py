"""Records what public calls return on the column-layout state files (lane, row-lane and tangent-linear quad kernels) for the cases
of tests/test_gpu_endpoint_kernels.py: every output as float.hex() strings, one JSON file per case.

    python3 scripts/record_endpoint_kernels.py [DIR]   (default: tests/golden/endpoint_kernels; needs a GPU; library: JQ_LIB or the built one)

The committed files were written by the build of the commit BEFORE the initial-state and terminal kernels of these layouts became
k_init_lane / k_init_rowlane / k_init_quad_tl and k_terminal_cols<Map, FLAVOR> (csrc/jq_aux_kernels.h).  The merge keeps every
floating-point operation, its operands and its order, so the calls must reproduce these files bit for bit.

The problems are those of the case tables of the existing tests of each route (their generators, their seeds), at most 16 time steps:
  lane_np2_sv1 .. 4   lane kernels at NP = 2 (no guard level: leak weights on both levels), N = 2, 37 nodes = 74 columns, sv_type 1 .. 4
  lane_np8_sv1, 4     lane kernels at NP = 8 (the size the tangent-linear list does not have), one evaluation, N = 3
  rowlane_n3_sv1, 4   row-lane kernels, N = 3, 7 nodes = 21 columns: samples straddle waves, the sixth wave holds one column
  rowlane_batch3      jq_traceobjgrad_batch, three control vectors of N = 3 columns: cpw = 3, a wave per vector
  rowlane_imr_n3      implicit midpoint on the row-lane kernels, N = 3 (sample-aligned packing, cpw = 3): one evaluation and 3 nodes
  hvp_lane_np2        jq_eval_f_g_grad_hvp, lane route, NP = 2, three nodes, two directions, objFuncType 1
  hvp_lane_np6        ... NP = 6, objFuncType 3 (second, unforced pass)
  hvp_lane_rounds     ... NP = 6, five directions, two per launch: three rounds, each re-runs the initial state
  hvp_rowlane_npj12   row-lane route, Ntot 9, N = 3, three nodes: nine columns, the third wave holds one
  hvp_rowlane_npj16   ... Ntot 16
  hvp_quad_nt2        quad route, NT = 2, N = 3, three nodes: the third quad holds one column, nodes share quads"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

LANE_OPTS = {"rowlane_max": 0}
KF_LANE, KF_ROWLANE, KF_ROWLANE_IMR, KF_QUAD = 2, 3, 4, 6
# name: (kind, kernel family, ...)
CASES = {}
for sv in (1, 2, 3, 4):
    CASES["lane_np2_sv%d" % sv] = ("ensemble", KF_LANE, "np2", sv)
for sv in (1, 4):
    CASES["lane_np8_sv%d" % sv] = ("single", KF_LANE, "np8", sv)
    CASES["rowlane_n3_sv%d" % sv] = ("ensemble", KF_ROWLANE, "rl", sv)
CASES["rowlane_batch3"] = ("batch", KF_ROWLANE, "rl", 1)
CASES["rowlane_imr_n3"] = ("imr", KF_ROWLANE_IMR, "imr", 1)
for name in ("hvp_lane_np2", "hvp_lane_np6", "hvp_lane_rounds", "hvp_rowlane_npj12", "hvp_rowlane_npj16", "hvp_quad_nt2"):
    CASES[name] = ("hvp", {"l": KF_LANE, "r": KF_ROWLANE, "q": KF_QUAD}[name[4]], name, 1)
NAMES = ("objfv", "totalgrad", "primaryobjf", "secondaryobjf", "traceInfidelity", "infidelgrad", "leakgrad")
HVP_KEYS = ("infidelity", "leak", "infid_grad", "leak_grad", "hv_infid", "hv_leak")
IMR_ITER, IMR_TOL = 60, 1e-11


def primal_problem(jq, which):
    """(params, pcof, options, nodes, weights, shift) of the Stormer-Verlet and implicit-midpoint cases"""
    from test_gpu_random import random_problem
    if which == "np2":       # (no row of test_gpu_svtype.RANDOM has NP = 2: its lane rows, at the smallest padded size)
        rng = np.random.default_rng(4200 + 2 * 31 + 2)
        p, pcof = random_problem(jq, rng, 2, 2, 1, 1, 11, 3, 2, False)
        p.wmat_real = rng.random(2) + 0.1
        nq = 37                                                          # (test_gpu_svtype.test_swap02_risk_neutral_ensemble)
        x, w = np.polynomial.legendre.leggauss(nq)
        return p, pcof, LANE_OPTS, x * 0.05, w * 0.5, rng.standard_normal(2)
    if which == "np8":       # test_gpu_svtype.RANDOM[1]
        rng = np.random.default_rng(4200 + 8 * 31 + 3)
        p, pcof = random_problem(jq, rng, 8, 3, 2, 2, 9, 2, 2, False)
        return p, pcof, LANE_OPTS, None, None, None
    if which == "rl":        # test_gpu_random.CASES: Ntot 10, N 3 (NPJ 12, objFuncType 3)
        rng = np.random.default_rng(4200 + 10 * 31 + 3)
        p, pcof = random_problem(jq, rng, 10, 3, 2, 2, 15, 3, 3, False)
        nodes = 0.05 * np.linspace(-1.0, 1.0, 7) + 0.01 * rng.standard_normal(7)
        return p, pcof, None, nodes, rng.random(7) + 0.1, rng.standard_normal(10)
    assert which == "imr"    # test_gpu_imr.test_imr_random_problems_match_oracle: (5, 3, 2, 2, 14, 3)
    rng = np.random.default_rng(77 + 5)
    p, pcof = random_problem(jq, rng, 5, 3, 2, 2, 14, 3, 3, False)
    p.Integrator_id = jq.Implicit_Midpoint
    p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=IMR_ITER, tol=IMR_TOL, nrhs=3)
    p.wmat = p.wmat_real.copy()
    shift = 0.05 * rng.standard_normal(5)
    shift[0] = 0.0
    return p, pcof, None, 0.05 * rng.standard_normal(3), rng.random(3), shift


def dvds_of(params):
    from test_svtype_host import random_dvds
    return random_dvds(params)


def set_sv_type(params, sv):
    """sv_type with the random dVds of the svtype tests (sv = 1: the target, as those tests leave it)"""
    from test_svtype_host import target_of
    D = dvds_of(params) if sv != 1 else target_of(params)
    params.dVds_r, params.dVds_i = np.asfortranarray(np.real(D).copy()), np.asfortranarray(np.imag(D).copy())
    params.sv_type = sv


def batch_vectors(pcof):
    from test_gpu_pcof_batch import vectors
    return vectors(pcof, 3, 13)


def hvp_problem(jq, name):
    """(params, pcof, options, nodes, weights, shift, directions) of the jq_eval_f_g_grad_hvp cases"""
    import test_gpu_ens_hvp as L
    import test_gpu_ens_hvp_quad as Q
    import test_gpu_ens_hvp_rowlane as R
    mod, c, extra, ndir = {
        "hvp_lane_np2": (L, L.Case(2, 2, 1, 4, 0, 5, 1, 3, "default"), None, 2),
        "hvp_lane_np6": (L, L.Case(6, 2, 4, 4, 0, 5, 3, 3, "given"), None, 2),
        # (the stream budget of test_gpu_ens_hvp.test_rounds_and_the_calls_around_are_the_same_bits: the primal stream and two directions)
        "hvp_lane_rounds": (L, L.Case(6, 2, 4, 4, 0, 5, 3, 3, "given"), {"stream_bytes": 8 * 3 * 2 * 48 * (2 * L.NSTEPS + 1), "chunk_steps": L.NSTEPS}, 5),
        "hvp_rowlane_npj12": (R, R.ROWLANE_CASES[1], None, 2),
        "hvp_rowlane_npj16": (R, L.Case(16, 3, 2, 1, 0, 5, 1, 3, "given"), None, 2),
        "hvp_quad_nt2": (Q, Q.QUAD_CASES[1], None, 2),
    }[name]
    p, pcof, rng, nodes, weights, shift = mod._problem(jq, c)
    assert p.N in (2, 3) and nodes.size == 3
    return p, pcof, mod._options(c, extra), nodes, weights, shift, rng.standard_normal((pcof.size, ndir))


def _hex(x):
    return [float(v).hex() for v in np.atleast_1d(np.asarray(x, dtype=np.float64)).ravel(order="F")]


def _ensemble(jq, pcof, params, wa, nodes, weights, shift):
    jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
    return {"infidelity": params.last_infidelity, "leak": params.last_leak, "infidelity_grad": params.last_infidelity_grad.copy(),
            "leak_grad": params.last_leak_grad.copy()}


def run_case(jq, name):
    """the case on the GPU: (outputs as arrays, kernel family of the last launch, plan_info)"""
    kind, family, which, sv = CASES[name]
    if kind == "hvp":
        p, pcof, opts, nodes, weights, shift, D = hvp_problem(jq, name)
        wa = jq.Working_Arrays_HIP(p, pcof.size, options=opts)
        r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, nodes, weights, shift)
        out = {k: r[k] for k in HVP_KEYS}
    else:
        p, pcof, opts, nodes, weights, shift = primal_problem(jq, which)
        wa = (jq.Working_Arrays_M_HIP if kind == "imr" else jq.Working_Arrays_HIP)(p, pcof.size, options=opts)
        if kind != "imr":
            set_sv_type(p, sv)
        if kind == "ensemble":
            out = _ensemble(jq, pcof, p, wa, nodes, weights, shift)
        elif kind == "batch":
            out = dict(zip(NAMES, jq.traceobjgrad_batch(batch_vectors(pcof), p, wa, True)))
        else:
            out = dict(zip(NAMES, jq.traceobjgrad(pcof, p, wa, False, True)))
        if kind == "imr":
            fam1 = wa.last_timing()["kernel_family"]
            assert fam1 == family, (name, fam1)
            out.update({"ens_" + k: v for k, v in _ensemble(jq, pcof, p, wa, nodes, weights, shift).items()})
    t, plan = wa.last_timing(), wa.plan_info()
    wa.close()
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}, t["kernel_family"], plan


def main():
    import juqbox_jl_amd as jq
    from juqbox_jl_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "endpoint_kernels")
    os.makedirs(out, exist_ok=True)
    print("library:", _lib.load().jq_version().decode())
    for name in CASES:
        res, family, plan = run_case(jq, name)
        assert family == CASES[name][1], (name, family)
        if "ens_hvp" in plan:
            print("  ", plan["ens_hvp"])
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump({k: {"shape": list(v.shape), "hex": _hex(v)} for k, v in res.items()}, f, indent=0)
            f.write("\n")
        print("%s: family %d, %s" % (name, family, ", ".join("%s %d" % (k, v.size) for k, v in res.items())))


if __name__ == "__main__":
    main()
