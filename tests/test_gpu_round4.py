"""GPU (-m gpu), round 4:
 (1) bench.py --single-process --gpus K in the same-device TEST MODE (JQ_MULTI_SAME_DEVICE=1): the reporting code of the one-process /
     K-device path -- per-shard min / max, in-library all-reduce time, both strong-scaling points, CPU baseline -- runs on a one-GPU box;
 (2) jq_update_hconst after a re-plan: the handle keeps its plan while the drifts fit it (no re-creation per call) and plans again
     when a drift regains a better structure;
 (3) build manifest: the kernels the bench path runs were built in VGPR form and within their scratch budget."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [2, 4])
def test_bench_single_process_same_device(K):
    env = dict(os.environ, JQ_OPTIONS="multi_same_device=1", JQ_BENCH_SAMPLES="128")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--single-process", "--gpus", str(K), "--steps", "1", "--warmup", "1",
           "--strong-samples", "512", "--strong-small-samples", "256", "--full", "--quick-extras"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "per_rank_ms", "allreduce_ms", "strong_scaling", "strong_scaling_small"):
        assert k in j, k
    assert j["n_gpus"] == K and j["config"]["devices_behind_handle"] == K and j["config"]["rccl_world_size"] == 0      # (test mode: no communicator)
    assert j["config"]["launcher"].startswith("TEST MODE same-device") and "not a multi-GPU measurement" in j["config"]["launcher"]
    assert j["config"]["samples_per_gpu"] == 128 and j["value"] > 0
    assert 0.0 < j["per_rank_ms"]["min"] <= j["per_rank_ms"]["max"] and j["allreduce_ms"] >= 0.0
    for key, total in (("strong_scaling", 512), ("strong_scaling_small", 256)):
        sp = j[key]
        assert sp["total_samples"] == total and sp["samples_per_gpu"] == total // K and sp["evals_per_s"] > 0
        assert 0.0 < sp["per_rank_ms"]["min"] <= sp["per_rank_ms"]["max"] and sp["allreduce_ms"] >= 0.0
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["cores"] == 1 and j["cpu_baseline"]["kind"] == "port"
    # without the test mode the same request is refused on a box with fewer GPUs
    from juqbox_jl_amd import _lib
    if _lib.load().jq_device_count() < K:
        env.pop("JQ_OPTIONS")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode != 0 and "GPU(s) are visible" in r.stderr and not any(ln.startswith("{") for ln in r.stdout.splitlines())


def test_replanned_handle_keeps_its_plan_while_the_drift_fits(jq):
    """advisor, round 3: after one out-of-structure drift every later jq_update_hconst re-created the whole handle (streams,
    allocations, uploads, the embedded twin) -- per call, on every device -- even when the new drift fitted the current plan.  A script
    that mutates params.Hconst per iteration (eval_f_g_grad!'s own loop does) must only pay for an upload."""
    from oracle.oracle import Oracle
    from test_gpu_random import random_problem
    rng = np.random.default_rng(12)
    p, pcof = random_problem(jq, rng, 64, 4, 2, 1, 8, 3, 1, "t4")
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    H0 = p.Hconst.copy()
    D = rng.standard_normal((64, 64))
    p.Hconst = H0 + 0.02 * (D + D.T)
    jq.traceobjgrad(pcof, p, wa, False, True)
    info = wa.plan_info()
    assert info["replanned"] is True and info["structure"] == "dense"
    times = []
    for k in range(6):                                   # six more dense drifts: the plan stays, each update is an upload
        p.Hconst = H0 + (0.02 + 0.001 * k) * (D + D.T)
        t0 = time.perf_counter()
        wa.sync_params()
        times.append(time.perf_counter() - t0)
        assert wa.plan_info() == info
    r = Oracle(p, use_sparse=False).traceobjgrad(pcof)
    objfv, tg = jq.traceobjgrad(pcof, p, wa, False, True)[:2]
    assert abs(objfv - r["objfv"]) <= 1e-10 * abs(r["objfv"]) and np.linalg.norm(tg - r["totalgrad"]) <= 1e-10 * np.linalg.norm(r["totalgrad"])
    p.Hconst = H0 * 1.01                                 # the 4 x 4 x n structure is back: planned again, fast family in use
    jq.traceobjgrad(pcof, p, wa, False, True)
    assert wa.plan_info()["structure"] == "t4" and wa.last_timing()["kernel_family"] in (6, 8)
    t0 = time.perf_counter()
    p.Hconst = H0 + 0.02 * (D + D.T)
    wa.sync_params()                                     # (a genuine re-plan, for scale)
    t_replan = time.perf_counter() - t0
    assert max(times) < 0.5 * t_replan, (times, t_replan)
    wa.close()


def test_manifest_of_the_bench_path_kernels():
    """verdict, round 3: Makefile silently rebuilt an object without -amdgpu-mfma-vgpr-form=1 when hipcc crashed, and nothing said
    which.  The build now writes csrc/build/manifest.json (flags, fallback, registers, scratch per kernel); jq_plan_info quotes it
    for the kernels a handle selects.  The objects of the bench path must be in VGPR form and within their scratch budget."""
    import juqbox_jl_amd as jq
    p, info = jq.cases.cnot3()
    wa = jq.Working_Arrays_HIP(p, info["nCoeff"])
    pi = wa.plan_info()
    wa.close()
    bk = pi["build"]
    assert bk["manifest"] is True
    # (round 6, csrc/Makefile: VGPR form only where it was measured to pay -- s_6_7 yes; k_6_7, u_6_7 no difference: default form)
    for obj, vf in (("k_6_7", False), ("s_6_7", True), ("u_6_7", False), ("p_6_7", True)):
        e = bk["objects"][obj]
        assert e["vgpr_form"] is vf and e["fallback"] is False, (obj, e)
    assert bk["objects"]["k_6_7"]["max_scratch_bytes"] <= 160
    assert bk["objects"]["s_6_7"]["max_scratch_bytes"] <= 64


@pytest.mark.parametrize("Ntot,N,tol,exact", [(40, 20, 1e-9, True), (64, 40, 1e-7, True), (80, 64, 1e-8, True), (130, 24, 1e-8, False), (90, 70, 1e-8, False)])
def test_jacobi_solver_with_more_than_16_columns(jq, Ntot, N, tol, exact):
    """JACOBI_SOLVER tests convergence per evaluation like the reference (norm(T - X) over the whole Ntot x N block,
    src/linear_solvers.jl:121).  With N > 16 the columns of an evaluation take ceil(N / 16) slabs.  Round 5: up to four slabs are the
    waves of ONE workgroup of the slab kernels, which adds their residual norms before it decides -- the reference's rule: 1e-10 against
    the oracle at any tolerance (`exact`; N = 20, 40, 64: two, three, four parts, the last one ragged).  More than four parts, or the
    cooperative kernels of Ntot > 96 (a slab per workgroup): every 16-column part is tested on its own, parts may stop at different
    iterations and the result differs by O(tol) (documented in include/juqbox_hip.h) -- held to 1e3 * tol; with a tolerance below the
    rounding level every part runs to max_iter like the reference and the agreement is 1e-10 again.  JQ_JAC_WG=0 (the per-part rule on
    the slab kernels too) must show that the exact cases are not exact by accident."""
    from oracle.oracle import Oracle
    from test_gpu_random import random_problem
    rng = np.random.default_rng(5 + Ntot)
    p, pcof = random_problem(jq, rng, Ntot, N, 2, 1, 12, 3, 1, False)
    for t, bound in ((tol, 1e-10 if exact else 1e3 * tol), (1e-30, 1e-10)):
        p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER, max_iter=40, tol=t, nrhs=N)
        wa = jq.Working_Arrays_HIP(p, pcof.size)
        r = Oracle(p, use_sparse=False).traceobjgrad(pcof)
        objfv, tg = jq.traceobjgrad(pcof, p, wa, False, True)[:2]
        assert abs(objfv - r["objfv"]) <= bound * abs(r["objfv"]), (t, objfv, r["objfv"])
        assert np.linalg.norm(tg - r["totalgrad"]) <= bound * np.linalg.norm(r["totalgrad"]), t
        # an ensemble too (several workgroups, one per sample)
        nodes, weights = 0.02 * rng.standard_normal(5), rng.random(5)
        shift = 0.05 * np.arange(p.Ntot)
        ref = Oracle(p, use_sparse=False).eval_f_g_grad(pcof, nodes, weights, shift)
        jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
        assert abs(p.last_infidelity - ref["last_infidelity"]) <= bound * abs(ref["last_infidelity"]), t
        assert np.linalg.norm(p.last_infidelity_grad - ref["last_infidelity_grad"]) <= bound * np.linalg.norm(ref["last_infidelity_grad"]), t
        wa.close()


@pytest.mark.parametrize("cfg", [
    # Ntot, N, Nc, Nfreq, nsteps, objFuncType, structure
    (40, 20, 2, 1, 10, 1, False), (48, 17, 1, 2, 8, 3, True), (96, 33, 2, 1, 6, 2, False), (64, 20, 3, 1, 7, 1, "t4"),
    (80, 32, 2, 1, 6, 3, "od"), (130, 24, 2, 1, 5, 1, True), (200, 40, 1, 1, 4, 2, False),
], ids=lambda c: "Ntot%d_N%d_%s" % (c[0], c[1], c[6] if isinstance(c[6], str) else ("band" if c[6] else "dense")))
def test_implicit_midpoint_with_more_than_16_columns(jq, cfg):
    """Round 3 refused the implicit-midpoint path for N > 16 (the fixed-point solver stops on the residual norm of the WHOLE
    evaluation, src/linear_solvers.jl:156-270, and an evaluation's 16-column parts ran in different workgroups).  Now one cooperative
    workgroup per evaluation walks over its parts: objective, gradients (leak split included), a ragged weighted ensemble and the
    state history against the oracle -- block-banded, dense 96 x 96 (images from L2), 4 x 4 x n, JQ_BW_OD, Ntot > 96."""
    from oracle.oracle import Oracle
    from test_gpu_random import random_problem
    Ntot, N, Nc, Nfreq, nsteps, oft, structure = cfg
    rng = np.random.default_rng(600 + Ntot + N)
    p, pcof = random_problem(jq, rng, Ntot, N, Nc, Nfreq, nsteps, 3, oft, structure)
    p.Integrator_id = jq.Implicit_Midpoint
    p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=80, tol=1e-12, nrhs=N)
    p.wmat = p.wmat_real.copy()
    wa = jq.Working_Arrays_M_HIP(p, pcof.size)
    orc = Oracle(p, use_sparse=False)
    r = orc.traceobjgrad_imr(pcof, 80, 1e-12, history=True)
    objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, p, wa, False, True)
    assert wa.last_timing()["kernel_family"] == 5
    gn = np.linalg.norm(r["totalgrad"])
    tol = 1e-9      # (implicit midpoint: bounded by the fixed-point solver's tolerance 1e-12 per step, see tests/test_gpu_round3.py)
    assert abs(prim - r["primaryobjf"]) <= tol and abs(sec - r["secondaryobjf"]) <= tol * max(abs(r["secondaryobjf"]), 1e-3)
    assert np.linalg.norm(tg - r["totalgrad"]) <= tol * gn and np.linalg.norm(ig - r["infidelgrad"]) <= tol * gn
    if oft != 1:
        assert np.linalg.norm(lg - r["leakgrad"]) <= tol * gn
    _, hist, _ = jq.traceobjgrad(pcof, p, wa, True, False)
    assert np.max(np.abs(hist - r["history"])) < 1e-9
    nq = 3
    nodes, weights = 0.05 * rng.standard_normal(nq), rng.random(nq)
    shift = rng.standard_normal(Ntot) * 0.05
    shift[0] = 0.0
    inf = leak = 0.0
    gi = np.zeros(pcof.size)
    H0 = p.Hconst.copy()
    for ep, wq in zip(nodes, weights):
        p.Hconst = H0 + np.diag(ep * shift)
        rr = Oracle(p, use_sparse=False).traceobjgrad_imr(pcof, 80, 1e-12)
        inf += wq * rr["primaryobjf"]
        leak += wq * rr["secondaryobjf"]
        gi += wq * rr["infidelgrad"]
    p.Hconst = H0
    jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
    assert abs(p.last_infidelity - inf) <= tol * abs(inf) and abs(p.last_leak - leak) <= tol * max(abs(leak), 1e-3)
    assert np.linalg.norm(p.last_infidelity_grad - gi) <= tol * np.linalg.norm(gi)
    wa.close()


def test_uni_and_ord_variants_of_the_throughput_kernel_agree(jq):
    """Round 4: the twelve-wave backward kernel has a one-sample-per-wave variant (UNI: the sample's shift folded into the MFMA's A
    operand, weight after the reduction, fused state-step stages) and, on top, one for controls that act on one subsystem each (ORD:
    compile-time trace modes, Hsym_1 lambda_i rides along with K05 lambda_i).  They reorder floating-point operations only: against
    the generic kernel (JQ_NO_UNI=1) and against each other the ensemble results agree to 1e-12; the default is the ORD kernel, which
    tests/test_gpu_round2.py pins against the oracle at full length."""
    params, info = jq.cases.cnot3()
    params.T, params.nsteps = params.T * 600 / params.nsteps, 600
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "cnot3.json")))["pcof0"])
    nodes, weights, shift = jq.cases.cnot3_ensemble(3072)
    res = {}
    for tag, env in (("ord", {}), ("uni", {"JQ_NO_ORD": "1"}), ("generic", {"JQ_NO_UNI": "1"})):
        with jq.options(**env):
            wa = jq.Working_Arrays_HIP(params, pcof.size)
            jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
            t = wa.last_timing()
            assert t["kernel_family"] == 6 and t["kernel_band"] == 7
            res[tag] = (params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy())
            wa.close()
    g = np.linalg.norm(res["generic"][2])
    for tag in ("ord", "uni"):
        assert abs(res[tag][0] - res["generic"][0]) <= 1e-13 * abs(res["generic"][0])
        assert abs(res[tag][1] - res["generic"][1]) <= 1e-12 * abs(res["generic"][1])
        assert np.linalg.norm(res[tag][2] - res["generic"][2]) <= 1e-12 * g
    assert not np.array_equal(res["ord"][2], res["generic"][2])      # (different kernels did run)


@pytest.mark.gpu
@pytest.mark.parametrize("nsamples", [0, 5])
def test_two_set_cooperative_quad_implicit_midpoint_kernel_is_the_one_set_kernel(jq, nsamples):
    """Round 4: k_backward_cq_imr2 runs the state chain of time step k and the adjoint chain of step k - 1 on two sets of waves
    (a pipeline of depth one inside a chunk, prologue and epilogue super-steps, odd chunk lengths); k_backward_cq_imr3 (the default for
    single evaluations and small ensembles) gives each chain and the trace products a workgroup of their own (three CUs, a ring in
    global memory).  Each chain performs the operations of the one-set kernel (JQ_CQ3=0 JQ_IMR_CQ2=0) in the same order:
    bit-identical results -- for one evaluation and for a small ensemble with shifts, with a step count that is odd and leaves a
    ragged last chunk."""
    params, info = jq.cases.cnot3()
    params.T, params.nsteps = params.T * 1501 / params.nsteps, 1501
    params.Integrator_id = jq.Implicit_Midpoint
    params.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=100, tol=1e-12, nrhs=params.N)
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "cnot3.json")))["pcof0"])
    res = {}
    for tag, env in (("three", {"JQ_CHUNK_STEPS": "400"}), ("two", {"JQ_CQ3": "0", "JQ_CHUNK_STEPS": "400"}),
                     ("one", {"JQ_CQ3": "0", "JQ_IMR_CQ2": "0", "JQ_CHUNK_STEPS": "400"}), ("three_whole", {})):
        with jq.options(**env):
            wa = jq.Working_Arrays_M_HIP(params, pcof.size)
            if nsamples:
                nodes, weights, shift = jq.cases.cnot3_ensemble(nsamples)
                jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
                res[tag] = (params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy())
            else:
                f, g, *_ = jq.traceobjgrad(pcof, params, wa, False, True)
                res[tag] = (f, 0.0, np.array(g))
            t = wa.last_timing()
            assert t["kernel_family"] == 9 and t["kernel_variant"] == (3 if tag.startswith("three") else 0)
            wa.close()
    for tag in ("two", "one"):
        assert res["three"][0] == res[tag][0] and res["three"][1] == res[tag][1]
        assert np.array_equal(res["three"][2], res[tag][2])
    # (one chunk instead of four: the gradient's partial sums are grouped differently)
    assert abs(res["three"][0] - res["three_whole"][0]) <= 1e-13 * abs(res["three"][0])
    assert np.linalg.norm(res["three"][2] - res["three_whole"][2]) <= 1e-12 * np.linalg.norm(res["three"][2])


@pytest.mark.gpu
@pytest.mark.parametrize("nsamples", [2, 5, 300])
def test_forward_cooperative_quad_kernel_with_two_quads_per_workgroup(jq, nsamples):
    """Round 4: with more column quads than CUs the forward cooperative-quad kernel takes two quads per workgroup (k_forward_cq<.., 2>:
    every array a pair of doubles per lane, the second quad in channel 1 of the exchange image).  Each quad sees the operations of
    the one-quad kernel in the same order: bit-identical results, also with an odd number of quads (a half-empty last pair) and
    several chunks; 300 samples take that kernel by themselves (more quads than CUs)."""
    params, info = jq.cases.cnot3()
    params.T, params.nsteps = params.T * 901 / params.nsteps, 901
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "cnot3.json")))["pcof0"])
    nodes, weights, shift = jq.cases.cnot3_ensemble(nsamples)
    res = {}
    for tag, env in (("two", {"JQ_CQ_FWD2": "1", "JQ_CHUNK_STEPS": "250"}), ("one", {"JQ_CQ_FWD2": "0", "JQ_CHUNK_STEPS": "250"}), ("auto", {"JQ_CHUNK_STEPS": "250"})):
        with jq.options(**env):
            wa = jq.Working_Arrays_HIP(params, pcof.size)
            jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
            assert wa.last_timing()["kernel_family"] == 8
            res[tag] = (params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy())
            wa.close()
    for tag in ("one", "auto"):
        assert res["two"][0] == res[tag][0] and res["two"][1] == res[tag][1]
        assert np.array_equal(res["two"][2], res[tag][2])


@pytest.mark.gpu
@pytest.mark.parametrize("case,nquad,K", [("swap02_rn", 13, 4), ("cnot2-leakieq", 7, 3)])
def test_multi_handle_against_the_oracle_loop(jq, case, nquad, K):
    """The K-sub-handle tests of round 3 compare the multi-device handle with the single handle (which the oracle pins elsewhere);
    here the sharded evaluation itself -- ragged shards, host threads, packing, the host-order sum that stands in for the all-reduce in
    the same-device mode -- is held against the oracle's loop over the samples (src/ipopt_interface.jl:38-65) at the 1e-10 of every
    Stormer-Verlet comparison."""
    from conftest import case_inputs
    from oracle.oracle import Oracle
    params, info, pcof, _ = case_inputs(case)
    x, w = np.polynomial.legendre.leggauss(nquad)
    nodes, weights = x * 0.5 * (2 * np.pi * 2e-2), w * 0.5
    shift = params.shift_weights_reference() if params.Ntot <= 4 else 0.05 * np.arange(params.Ntot)
    ref = Oracle(params).eval_f_g_grad(pcof, nodes, weights, shift)
    wam = jq.Working_Arrays_HIP(params, pcof.size, devices=K, options={"multi_same_device": 1})
    assert wam.num_devices == K and wam.rccl_world_size == 0      # (test mode: no communicator)
    jq.eval_f_g_grad(pcof, params, wam, nodes, weights, True, shift=shift if params.Ntot > 4 else None)
    wam.close()
    gn = np.linalg.norm(ref["last_infidelity_grad"])
    assert abs(params.last_infidelity - ref["last_infidelity"]) <= 1e-10 * abs(ref["last_infidelity"])
    assert abs(params.last_leak - ref["last_leak"]) <= 1e-10 * abs(ref["last_leak"])
    assert np.linalg.norm(params.last_infidelity_grad - ref["last_infidelity_grad"]) <= 1e-10 * gn
    if params.objFuncType != 1:
        assert np.linalg.norm(params.last_leak_grad - ref["last_leak_grad"]) <= 1e-10 * gn


def _cq3_problem(jq, kind):
    """cnot3 shortened (4 x 4 x 6, NT = 6, even m), or random 4 x 4 x n problems with N = 4 (NT = 3 / 7; objFuncType 3: two backward passes)"""
    if kind == "cnot3":
        params, info = jq.cases.cnot3()
        params.T, params.nsteps = params.T * 1101 / params.nsteps, 1101
        pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "cnot3.json")))["pcof0"])
        return params, pcof
    from test_gpu_random import random_problem
    Ntot, m = {"t4x3": (48, 5), "t4x7": (112, 4)}[kind]
    rng = np.random.default_rng(5 + Ntot)
    params, pcof = random_problem(jq, rng, Ntot, 4, 3, 2, 57, m, 3, "t4")
    return params, pcof


@pytest.mark.gpu
@pytest.mark.parametrize("kind,nsamples", [("cnot3", 1), ("cnot3", 5), ("cnot3", 21), ("t4x3", 3), ("t4x7", 2)])
def test_backward_sweep_on_three_workgroups_per_quad_is_the_one_workgroup_kernel(jq, kind, nsamples):
    """Round 4: k_backward_cq3 runs the state re-integration, the adjoint step and the trace products of a column quad on three
    workgroups (CUs) that hand their per-step arrays on through a ring in global memory.  Every chain and every trace sum performs the
    operations of k_backward_cq (JQ_CQ3=0) in the same order: bit-identical results -- single evaluation and small ensembles (groups
    of 8 quads with idle ones), several chunks with odd lengths, odd / even numbers of Neumann terms, NT = 3, 6, 7, objFuncType 3
    (a second, unforced backward pass), and run to run."""
    params, pcof = _cq3_problem(jq, kind)
    rng = np.random.default_rng(3)
    nodes, weights = 0.02 * rng.standard_normal(nsamples), rng.random(nsamples)
    shift = 0.01 * np.arange(params.Ntot)
    res = {}
    for tag, env in (("three", {"JQ_CHUNK_STEPS": "300" if kind == "cnot3" else "20"}), ("one", {"JQ_CQ3": "0", "JQ_CHUNK_STEPS": "300" if kind == "cnot3" else "20"}),
                     ("three_again", {})):
        with jq.options(**env):
            wa = jq.Working_Arrays_HIP(params, pcof.size)
            jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
            t = wa.last_timing()
            assert t["kernel_family"] == 8 and t["kernel_variant"] == (0 if tag == "one" else 3), t
            res[tag] = (params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy(),
                        params.last_leak_grad.copy() if params.objFuncType != 1 else np.zeros(1))
            wa.close()
    a, b, c = res["three"], res["one"], res["three_again"]
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    # (one chunk instead of several: the gradient's partial sums are grouped differently)
    assert abs(a[0] - c[0]) <= 1e-13 * abs(a[0]) and np.linalg.norm(a[2] - c[2]) <= 1e-12 * np.linalg.norm(a[2])


@pytest.mark.gpu
def test_three_workgroup_kernel_falls_back_when_it_reports_a_dead_wait(jq):
    """k_backward_cq3 raises an error word when a wait between its workgroups is abandoned or when they do not share an XCD.  The word is
    read after the FIRST backward launch (round 5), the evaluation is repeated with k_backward_cq, and the handle leaves the split alone
    for a while (4, 8, 16 ... evaluations per fault, for good after six faults) instead of for ever (JQ_CQ3_FAULT=1 simulates the report).
    jq_plan_info says what was decided and why."""
    params, pcof = _cq3_problem(jq, "cnot3")
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    f0, g0, *_ = jq.traceobjgrad(pcof, params, wa, False, True)
    assert wa.last_timing()["kernel_variant"] == 3
    ls = wa.plan_info()["latency_split"]
    assert ls["last_decision"].startswith("taken") and ls["faults"] == 0 and ls["off"] is False
    wa.set_option("cq3_fault", 1)
    try:
        f1, g1, *_ = jq.traceobjgrad(pcof, params, wa, False, True)
    finally:
        wa.set_option("cq3_fault", None)
    assert wa.last_timing()["kernel_variant"] == 0 and f1 == f0 and np.array_equal(g1, g0)
    ls = wa.plan_info()["latency_split"]
    assert ls["last_decision"] == "not taken: cooling down after a fault" and ls["faults"] == 1 and ls["cooling_down"] == 3
    for k in range(3):      # (the handle stays on the one-workgroup kernel while it cools down)
        f2, g2, *_ = jq.traceobjgrad(pcof, params, wa, False, True)
        assert wa.last_timing()["kernel_variant"] == 0 and f2 == f0 and np.array_equal(g2, g0)
    f3, g3, *_ = jq.traceobjgrad(pcof, params, wa, False, True)      # ... and tries the split again afterwards
    assert wa.last_timing()["kernel_variant"] == 3 and f3 == f0 and np.array_equal(g3, g0)
    wa.close()


@pytest.mark.gpu
def test_three_workgroup_kernels_across_changing_ensemble_sizes(jq):
    """One handle, ensemble sizes that move in and out of the three-workgroup regime (its hand-off buffer grows, the one-workgroup
    kernel takes over beyond 80 samples and hands back): every result equals the one of a handle that never uses the split."""
    params, pcof = _cq3_problem(jq, "cnot3")
    wb = jq.Working_Arrays_HIP(params, pcof.size, options={"cq3": 0})
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    for ns in (1, 80, 9, 81, 2, 33, 300, 5):
        nodes, weights, shift = jq.cases.cnot3_ensemble(ns)
        jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
        a = (params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy())
        # (more column quads than CUs: the backward sweep of both handles is k_backward_qsplit with two quads per workgroup, round 5)
        # (round 5: 81 .. 128 samples on two workgroups per quad)
        assert wa.last_timing()["kernel_variant"] == (3 if ns <= 80 else 2 if ns <= 128 else 22 if ns > 256 else 0), ns
        jq.eval_f_g_grad(pcof, params, wb, nodes, weights, True, shift=shift)
        assert wb.last_timing()["kernel_variant"] == (22 if ns > 256 else 0)
        assert a[0] == params.last_infidelity and a[1] == params.last_leak and np.array_equal(a[2], params.last_infidelity_grad), ns
    wa.close()
    wb.close()
