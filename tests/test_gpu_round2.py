"""GPU (-m gpu): the parity gaps of the round-1 verdict and the multi-GPU entry points.

 (1) the EXACT path bench.py times -- cnot3 at full length (32 386 steps), 3 072 PERTURBED samples (use_shift = 1),
     quad-layout kernels with three slabs per workgroup -- against the CPU oracle: one-hot ensemble weights select
     single samples, whose infidelity / leak / gradient are compared with oracle evaluations of the same perturbed
     Hamiltonian; the forward-only sweep entry gives the per-sample objectives of ALL samples;
 (2) SWAP-02 risk-neutral at BASELINE's 512 nodes against the oracle's serial ensemble loop;
 (3) the cnot3 state history against the oracle at sampled steps;
 (4) chunking rules (trace-record budget, gridDim.y cap at nsteps > 32 767);
 (5) multi-GPU: a one-device multi-device handle (RCCL inside the library), a one-rank nccl process group through
     torch.distributed (the device-resident packed result), bench.py's launcher.
Tolerance: 1e-10 relative (north_star: "within a stated fp64 tolerance"; the reference's own rtol, test/evalGrad.jl:4)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT, case_inputs
from kronecker_problem import random_kronecker_problem

pytestmark = pytest.mark.gpu

TOL = 1e-10


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def hip(jq):
    from juqbox_jl_amd import _lib
    assert _lib.load().jq_device_count() >= 1, "no HIP device: the hot path has no CPU fallback"
    return jq


def oracle_sample(params, pcof, ep, shift, **kw):
    """oracle evaluation of ONE ensemble sample: Hconst + ep * diag(shift) (src/ipopt_interface.jl:41-44)"""
    from oracle.oracle import Oracle
    H0 = params.Hconst.copy()
    params.Hconst = H0 + np.diag(ep * shift)
    try:
        return Oracle(params).traceobjgrad(pcof, **kw)
    finally:
        params.Hconst = H0


def test_bench_path_full_length_perturbed_samples_match_the_oracle(hip):
    jq = hip
    params, info, pcof, _ = case_inputs("cnot3")
    ns = 3072
    nodes, weights, shift = jq.cases.cnot3_ensemble(ns)          # bench.py's ensemble: nonzero nodes
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    picks = [0, 1537, 3071]          # first / middle / last sample: different slabs, waves and workgroups
    refs = {i: oracle_sample(params, pcof, nodes[i], shift) for i in picks}
    for i in picks:
        w = np.zeros(ns)
        w[i] = 1.0
        jq.eval_f_g_grad(pcof, params, wa, nodes, w, True, shift=shift)
        t = wa.last_timing()
        assert t["kernel_family"] == 6 and t["kernel_band"] == 7 and t["kernel_size"] == 6      # bench.py's kernels
        r = refs[i]
        assert abs(params.last_infidelity - r["primaryobjf"]) <= TOL * abs(r["primaryobjf"]), i
        assert abs(params.last_leak - r["secondaryobjf"]) <= TOL * abs(r["secondaryobjf"]), i
        assert rel(params.last_infidelity_grad, r["totalgrad"]) < TOL, i
    # the perturbation matters at this tolerance (the test would not notice a dropped shift otherwise)
    assert abs(refs[0]["primaryobjf"] - refs[1537]["primaryobjf"]) > 1e-7 * abs(refs[1537]["primaryobjf"])
    # per-sample objectives of the whole ensemble from the forward-only sweep entry
    sw = jq.traceobj_sweep(pcof, params, wa, nodes, shift)
    for i in picks:
        assert abs(sw[i, 1] - refs[i]["primaryobjf"]) <= TOL * abs(refs[i]["primaryobjf"])
        assert abs(sw[i, 2] - refs[i]["secondaryobjf"]) <= TOL * abs(refs[i]["secondaryobjf"])
    # the quadrature nodes are symmetric and the detuning enters the objective smoothly: the sweep is a smooth curve
    assert np.all(np.isfinite(sw)) and np.max(np.abs(np.diff(sw[:, 1]))) < 1e-3
    # the full weighted ensemble equals the weighted sum of the sweep (linearity of eval_f_g_grad! in the weights)
    jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
    assert abs(params.last_infidelity - np.dot(weights, sw[:, 1])) <= 1e-12
    assert abs(params.last_leak - np.dot(weights, sw[:, 2])) <= 1e-15
    wa.close()


def test_swap02_risk_neutral_512_nodes_matches_the_oracle_loop(hip):
    """BASELINE configs[4]: examples/Risk_Neutral/swap-02-risk-neutral.jl with 512 Gauss-Legendre nodes and the reference's
    own perturbation 0.01 ep 10^(j-2)."""
    from oracle.oracle import Oracle
    jq = hip
    params, info, pcof, _ = case_inputs("swap02_rn")
    nodes, weights = info["nodes"], info["weights"]
    assert nodes.size == 512
    ref = Oracle(params).eval_f_g_grad(pcof, nodes, weights, params.shift_weights_reference())
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True)
    assert abs(params.last_infidelity - ref["last_infidelity"]) <= TOL * abs(ref["last_infidelity"])
    assert abs(params.last_leak - ref["last_leak"]) <= TOL * abs(ref["last_leak"])
    assert rel(params.last_infidelity_grad, ref["last_infidelity_grad"]) < TOL
    wa.close()


def test_cnot3_state_history_matches_the_oracle_at_sampled_steps(hip):
    from oracle.oracle import Oracle
    jq = hip
    params, info, pcof, _ = case_inputs("cnot3")
    r = Oracle(params).traceobjgrad(pcof, evaladjoint=False, history=True)
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    objfv, hist, fid = jq.traceobjgrad(pcof, params, wa, True, False)      # ONE forward sweep: history + objective
    steps = np.unique(np.concatenate([np.arange(0, params.nsteps + 1, 97), [1, 2, params.nsteps - 1, params.nsteps]]))
    assert steps.size > 300
    assert np.max(np.abs(hist[:, :, steps] - r["history"][:, :, steps])) < 1e-11
    assert abs(objfv - r["objfv"]) <= TOL * abs(r["objfv"])
    # the device-side consumers (jq_state_populations) against numpy on the ORACLE's history: level populations at every
    # 500th step, third-subsystem marginals, maxima over all columns and steps
    p2 = np.abs(r["history"]) ** 2
    pop, maxpop = jq.state_populations(pcof, params, wa, every=500)
    assert np.max(np.abs(pop - p2[:, :, ::500])) < 1e-11
    assert np.max(np.abs(maxpop - p2.max(axis=(1, 2)))) < 1e-11
    m3 = jq.marginalize3_device(pcof, params, wa, every=500)
    grp = jq.plotstatectrl._subsystem_indices(params)[2]
    ref3 = np.zeros_like(m3)
    for row in range(params.Ntot):
        ref3[grp[row]] += p2[row, :, ::500]
    assert np.max(np.abs(m3 - ref3)) < 1e-11
    wa.close()


def test_trace_record_budget_only_changes_the_chunking(hip):
    """JQ_TRACE_BYTES bounds the per-step trace records of a backward chunk: a tiny budget forces many short chunks and
    must give the same result (cnot3 shortened to 240 steps, 40 perturbed samples)."""
    jq = hip
    params, info, pcof, _ = case_inputs("cnot3")
    params.nsteps = 240
    params.T = params.T * 240 / 32386
    nodes, weights, shift = jq.cases.cnot3_ensemble(40)
    res = []
    for budget in (None, "20000"):
        wa = jq.Working_Arrays_HIP(params, pcof.size, options={"trace_bytes": budget} if budget else None)
        jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
        res.append((params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy(),
                    wa.last_timing()["n_backward_launches"]))
        wa.close()
    assert res[1][3] > res[0][3]
    assert abs(res[0][0] - res[1][0]) <= 1e-13 and abs(res[0][1] - res[1][1]) <= 1e-16
    assert rel(res[1][2], res[0][2]) < 1e-12


def test_more_than_32767_steps_per_evaluation(hip):
    """k_ctrl / k_stream index the time points of a chunk with gridDim.y: chunks are capped at 32 767 steps, so longer
    gates take more than one chunk (rabi with 40 000 steps vs the oracle)."""
    from oracle.oracle import Oracle
    jq = hip
    params, info, pcof, _ = case_inputs("rabi")
    params.nsteps = 40000
    r = Oracle(params).traceobjgrad(pcof)
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    objfv, tg, *_ = jq.traceobjgrad(pcof, params, wa, False, True)
    assert wa.last_timing()["n_forward_launches"] >= 2
    # (rabi's objective is the cancellation 1 - |s|^2 + leak ~ 1e-13 at this step size: absolute floor = rounding of 40 000 steps)
    assert abs(objfv - r["objfv"]) <= max(TOL * abs(r["objfv"]), 1e-12)
    assert np.linalg.norm(tg - r["totalgrad"]) <= max(TOL * np.linalg.norm(r["totalgrad"]), 1e-12)
    wa.close()


# ---- multi-GPU entry points ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,nquad", [("swap02_rn", 64), ("cnot2-leakieq", 5)])
def test_multi_device_handle_with_one_device_matches_the_single_device_handle(hip, case, nquad):
    """jq_create_multi on the one GPU of this box: sharding, per-device packing and the ncclAllReduce (1-rank communicator
    from ncclCommInitAll) run for real; results must equal the single-device handle's, which the oracle pins."""
    jq = hip
    params, info, pcof, _ = case_inputs(case)
    x, w = np.polynomial.legendre.leggauss(nquad)
    nodes, weights = x * 0.5 * (2 * np.pi * 2e-2), w * 0.5
    shift = None if params.Ntot <= 4 else 0.05 * np.arange(params.Ntot)
    wa1 = jq.Working_Arrays_HIP(params, pcof.size)
    jq.eval_f_g_grad(pcof, params, wa1, nodes, weights, True, shift=shift)
    a = (params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy(), params.last_leak_grad.copy())
    sw1 = jq.traceobj_sweep(pcof, params, wa1, nodes, shift)
    t1 = jq.traceobjgrad(pcof, params, wa1, False, True)
    wa1.close()
    wam = jq.Working_Arrays_HIP(params, pcof.size, devices=[0])
    assert wam.num_devices == 1
    jq.eval_f_g_grad(pcof, params, wam, nodes, weights, True, shift=shift)
    assert abs(params.last_infidelity - a[0]) <= 1e-13 * abs(a[0]) and abs(params.last_leak - a[1]) <= 1e-13 * abs(a[1])
    assert rel(params.last_infidelity_grad, a[2]) < 1e-13
    if params.objFuncType != 1:
        assert np.linalg.norm(params.last_leak_grad - a[3]) <= 1e-13 * np.linalg.norm(a[2])
    assert wam.last_timing()["svts"] == nquad * params.N * params.nsteps
    assert np.array_equal(jq.traceobj_sweep(pcof, params, wam, nodes, shift), sw1)
    tm = jq.traceobjgrad(pcof, params, wam, False, True)
    assert tm[0] == t1[0] and np.array_equal(tm[1], t1[1])
    params.linear_solver.max_iter += 1                           # mutations reach every device handle
    jq.eval_f_g_grad(pcof, params, wam, nodes, weights, True, shift=shift)
    assert params.last_infidelity != a[0]
    wam.close()


def test_multi_device_handle_rejects_more_devices_than_visible(hip):
    from juqbox_jl_amd import _lib
    jq = hip
    params, info, pcof, _ = case_inputs("swap02")
    n = _lib.load().jq_device_count()
    with pytest.raises(_lib.JuqboxHipError) as e:
        jq.Working_Arrays_HIP(params, pcof.size, devices=n + 1)
    assert e.value.code == _lib.JQ_EINVAL
    with pytest.raises(_lib.JuqboxHipError):
        jq.Working_Arrays_HIP(params, pcof.size, devices=[0, 0])


_NCCL_WORKER = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import torch, torch.distributed as dist
import juqbox_jl_amd as jq
from conftest import case_inputs
torch.cuda.set_device(0)
params, info, pcof, _ = case_inputs("swap02_rn")
nodes, weights = info["nodes"][:96], info["weights"][:96]
wa = jq.Working_Arrays_HIP(params, pcof.size)
jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True)                       # no process group: host path
a = [params.last_infidelity, params.last_leak] + params.last_infidelity_grad.tolist()
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True)                       # device-resident packed result + all_reduce
b = [params.last_infidelity, params.last_leak] + params.last_infidelity_grad.tolist()
jq.eval_f_g_grad(pcof, params, wa, nodes, weights, False)
c = [params.last_infidelity, params.last_leak, float(np.abs(params.last_infidelity_grad).max())]
dist.barrier(); dist.destroy_process_group(); wa.close()
print("RESULT " + json.dumps(dict(a=a, b=b, c=c, backend="nccl")))
"""


def test_one_rank_nccl_process_group_uses_the_device_resident_result(hip):
    """eval_f_g_grad under an initialised nccl (= RCCL) process group with ONE rank: jq_eval_f_g_grad_dev leaves the packed
    sums on the GPU, torch.distributed all-reduces them there.  Fresh process: the group must not leak into other tests."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29600 + os.getpid() % 300),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", _NCCL_WORKER.format(root=ROOT)], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    a, b, c = np.array(res["a"]), np.array(res["b"]), res["c"]
    assert abs(a[0] - b[0]) <= 1e-13 * abs(a[0]) and abs(a[1] - b[1]) <= 1e-13 * abs(a[1])
    assert rel(b[2:], a[2:]) < 1e-13
    assert abs(c[0] - a[0]) <= 1e-13 * abs(a[0]) and c[2] == 0.0      # compute_adjoint = false: gradients reset to zero


def test_bench_refuses_more_gpus_than_visible(hip):
    from juqbox_jl_amd import _lib
    n = _lib.load().jq_device_count()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n + 1)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "GPU(s) are visible" in r.stderr
    assert not any(ln.startswith("{") for ln in r.stdout.splitlines())       # and no JSON line that could be mistaken for a result


# ---- sizes beyond the round-1 kernel limits (Ntot <= 96, N <= 16) --------------------------------------------------------
@pytest.mark.parametrize("Ntot,N,Nc,nsteps,m,oft,structure,nq", [
    (112, 4, 2, 9, 3, 1, False, 1),          # NT = 7, dense
    (128, 16, 1, 7, 2, 3, False, 3),         # NT = 8, dense, full slab, objFuncType 3 (two backward passes), ensemble
    (160, 5, 3, 6, 4, 1, True, 2),           # NT = 10, nearest-level couplings: block band 1
    (200, 3, 2, 5, 1, 2, False, 1),          # NT = 13 (Ntot not a multiple of 16), dense
    (256, 8, 1, 4, 2, 1, True, 1),           # NT = 16: 1024-thread workgroups
    (40, 24, 2, 11, 3, 1, False, 2),         # N > 16: two slabs per sample, slab kernels (NT = 3)
    (20, 20, 1, 9, 2, 3, False, 3),          # N = Ntot (no guard levels), 3 samples
    (96, 40, 2, 6, 2, 1, "t4", 1),           # N > 16 on the quad-layout / JQ_BW_T4 kernels
    (130, 33, 1, 5, 2, 1, True, 2),          # both: big cooperative kernels with three slabs per sample
])
def test_sizes_beyond_the_round1_limits_match_the_oracle(hip, Ntot, N, Nc, nsteps, m, oft, structure, nq):
    """Ntot up to 256 (cooperative kernels with 7..16 waves per slab, operator tiles read from HBM) and N up to Ntot
    (a sample's columns spread over ceil(N/16) slabs; the trace fidelity couples them in k_terminal_parts): objective,
    gradients, ensemble sums and the state history against the oracle."""
    from oracle.oracle import Oracle
    from test_gpu_random import random_problem
    jq = hip
    rng = np.random.default_rng(1000 + Ntot + N)
    p, pcof = random_problem(jq, rng, Ntot, N, Nc, 2, nsteps, m, oft, structure)
    nodes, weights = 0.05 * rng.standard_normal(nq), rng.random(nq)
    shift = 0.05 * rng.standard_normal(Ntot)
    inf = leak = 0.0
    gi, gl = np.zeros(pcof.size), np.zeros(pcof.size)
    for ep, wq in zip(nodes, weights):
        r = oracle_sample(p, pcof, ep, shift)
        inf += wq * r["primaryobjf"]
        leak += wq * r["secondaryobjf"]
        gi += wq * r["infidelgrad"]
        gl += wq * r["leakgrad"]
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
    from conftest import reference_pass      # (the reference's criterion, rtol 1e-10 / atol 1e-14 per quantity: rounds 2 - 5 asserted 1e-9 here)
    assert reference_pass(p.last_infidelity, inf) and reference_pass(p.last_leak, leak) and reference_pass(p.last_infidelity_grad, gi)
    if oft != 1:
        assert reference_pass(p.last_leak_grad, gl)
    r0 = Oracle(p, use_sparse=False).traceobjgrad(pcof, evaladjoint=False, history=True)
    objfv, hist, fid = jq.traceobjgrad(pcof, p, wa, True, False)
    assert hist.shape == (Ntot, N, nsteps + 1)
    assert np.max(np.abs(hist - r0["history"])) < 1e-11
    assert reference_pass(objfv, r0["objfv"])
    wa.close()


# ---- structure embedding: d1 x d2 x d3 Hilbert spaces on the 4 x 4 x n (JQ_BW_T4 / quad-layout) kernels --------------------
@pytest.mark.parametrize("case", ["cnot2", "cnot2-leakieq"])
def test_cnot2_goldens_on_the_quad_layout_kernels_through_the_embedding(hip, case):
    """cnot2 is 3 x 4 levels: padded to 4 x 4 it is ONE 16-row block of the JQ_BW_T4 structure.  JQ_EMBED=2 sends every batch to
    the embedded twin: the reference's goldens must come out of the quad-layout kernels (kernel family 6)."""
    from test_gpu_parity import gpu_eval_like_evalGrad
    from conftest import reference_pass
    jq = hip
    params, info, pcof, golden = case_inputs(case)
    wa = jq.Working_Arrays_HIP(params, pcof.size, options={"embed": 2})
    obj, grad = gpu_eval_like_evalGrad(jq, params, wa, pcof)
    t = wa.last_timing()
    assert (t["kernel_family"], t["kernel_band"], t["kernel_size"]) == (6, 7, 1)
    assert reference_pass(obj, golden["obj0"]), (obj, golden["obj0"])
    assert reference_pass(grad, golden["grad0"])
    # mutations reach the twin: target, weights, Neumann terms, drift
    from oracle.oracle import Oracle
    params.linear_solver.max_iter = 3
    params.wmat_real = jq.setup_utils.wmatsetup(params.Ne, params.Ng)
    params.Utarget_r, params.Utarget_i = params.Utarget_i.copy(), -params.Utarget_r.copy()
    params.Hconst[np.diag_indices(params.Ntot)] += 1e-3 * np.arange(params.Ntot)
    r = Oracle(params).traceobjgrad(pcof)
    objfv, tg, *_ = jq.traceobjgrad(pcof, params, wa, False, True)
    assert wa.last_timing()["kernel_family"] == 6
    assert abs(objfv - r["objfv"]) <= TOL * abs(r["objfv"]) and rel(tg, r["totalgrad"]) < TOL
    wa.close()


@pytest.mark.parametrize("dims,N,nq", [((3, 4, 1), 4, 700), ((2, 2, 3), 3, 5), ((3, 3, 5), 4, 40), ((4, 2, 6), 2, 9), ((2, 4, 2), 16, 3),
                                       ((3, 4, 7), 4, 9), ((3, 3, 8), 2, 5)])
def test_random_kronecker_problems_take_the_embedded_kernels(hip, dims, N, nq):
    """Random d1 x d2 x d3 problems (dense blocks on the fastest factor, diagonal couplings of the other two): large batches
    go to the embedded twin by default (family 6 or 0 with band 7 / 8), results against the oracle; with JQ_EMBED=0 the same
    problem runs on the generic kernels and must agree."""
    jq = hip
    p, pcof, rng = random_kronecker_problem(jq, dims, N)
    nodes, weights = 0.05 * rng.standard_normal(nq), rng.random(nq)
    shift = 0.05 * rng.standard_normal(p.Ntot)
    out = {}
    for mode in ("2", "0"):
        # (a space that has the structure natively, 2 x 2 x 3, must use it too: no lane kernels)
        wa = jq.Working_Arrays_HIP(p, pcof.size, options=dict({"embed": mode}, **({"lane": 0} if mode == "2" else {})))
        jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
        t = wa.last_timing()
        out[mode] = (p.last_infidelity, p.last_leak, p.last_infidelity_grad.copy(), p.last_leak_grad.copy(), t["kernel_family"], t["kernel_band"])
        wa.close()
    a, b = out["2"], out["0"]
    assert a[5] in (7, 8) and (b[5] not in (7, 8) or dims == (2, 2, 3))
    assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-11 * abs(b[1])
    assert rel(a[2], b[2]) < 1e-11 and np.linalg.norm(a[3] - b[3]) <= 1e-11 * np.linalg.norm(b[2])
    # and against the oracle (small ensembles only: CPU time)
    if nq <= 40:
        inf = leak = 0.0
        gi = np.zeros(pcof.size)
        for ep, wq in zip(nodes, weights):
            r = oracle_sample(p, pcof, ep, shift)
            inf += wq * r["primaryobjf"]; leak += wq * r["secondaryobjf"]; gi += wq * r["infidelgrad"]
        from conftest import reference_pass
        assert reference_pass(a[0], inf) and reference_pass(a[1], leak) and reference_pass(a[2], gi)


# ---- split batches (ensembles that do not fill their last round of the three-slab quad-layout kernels) -------------------
def test_split_batches_give_the_results_of_the_unsplit_batch(hip):
    """3 x #CU x 4 + 131 cnot3 samples (60 time steps): run_eval evaluates the full round(s) on the three-slab quad-layout
    kernels and the remainder on the cooperative-quad kernels (two batches); JQ_NOSPLIT=1 evaluates one batch.  Same ensemble
    sums (host outputs and the device-resident packed vector), same per-sample objectives, and the remainder's samples
    against the oracle."""
    import ctypes
    from juqbox_jl_amd import _lib
    from juqbox_jl_amd.evalobjgrad import _f64, _ptr
    jq = hip
    params, info = jq.cases.cnot3()
    params.nsteps = 60
    params.T = params.T * 60 / 32386
    pcof = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "cnot3.json")))["pcof0"])
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    L = _lib.load()
    hiprt = L      # (device memory for the packed result from the HIP runtime the library itself is bound to: dlsym on its handle
                   #  searches its dependencies -- a second copy of the runtime, e.g. PyTorch's, may not see the device here)
    npk = 2 + 2 * pcof.size
    d_packed = ctypes.c_void_p()
    hiprt.hipMalloc.restype = hiprt.hipMemcpy.restype = hiprt.hipFree.restype = ctypes.c_int
    assert hiprt.hipMalloc(ctypes.byref(d_packed), ctypes.c_size_t(8 * npk)) == 0
    ncu = L.jq_num_compute_units(wa.handle)     # (256 on MI355X: one round of the three-slab kernels = 3 ncu slabs)
    ns = 3 * ncu * 4 + 131
    nodes, weights, shift = jq.cases.cnot3_ensemble(ns)
    weights = weights * (1.0 + 0.3 * np.cos(np.arange(ns)))      # (not uniform: a mix-up of the two parts' weights would show)
    res = {}
    for tag in ("split", "nosplit"):
        wa.set_option("nosplit", 1 if tag == "nosplit" else None)
        try:
            jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
            t = wa.last_timing()
            _lib.check(L.jq_eval_f_g_grad_dev(wa.handle, _ptr(_f64(pcof)), pcof.size, _ptr(_f64(nodes)), _ptr(_f64(weights)), ns,
                                              _ptr(_f64(shift)), 1, d_packed), wa.handle)
            packed = np.zeros(npk)
            assert hiprt.hipMemcpy(packed.ctypes.data_as(ctypes.c_void_p), d_packed, ctypes.c_size_t(8 * npk), 2) == 0      # DeviceToHost
            sweep = jq.traceobj_sweep(pcof, params, wa, nodes, shift=shift)
        finally:
            wa.set_option("nosplit", None)
        res[tag] = (params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy(), packed, np.asarray(sweep),
                    t["n_forward_launches"], t["svts"])
    a, b = res["split"], res["nosplit"]
    assert a[5] == 2 * b[5] and a[6] == b[6] == ns * 4 * 60       # two batches, every column counted once
    assert abs(a[0] - b[0]) <= 1e-13 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-13 * abs(b[1])
    assert rel(a[2], b[2]) < 1e-12
    assert rel(a[3], b[3]) < 1e-12
    assert abs(a[3][0] - a[0]) <= 1e-13 * abs(a[0]) and rel(a[3][2:2 + pcof.size], a[2]) < 1e-12
    assert np.max(np.abs(a[4] - b[4])) < 1e-12
    # the first and the last sample of the remainder against the oracle
    for j in (ns - 131, ns - 1):
        r = oracle_sample(params, pcof, nodes[j], shift, evaladjoint=False)
        assert abs(a[4][j, 0] - r["objfv"]) <= 1e-10 * abs(r["objfv"])
    hiprt.hipFree(d_packed)
    wa.close()


@pytest.mark.parametrize("Ntot,N,structure", [(112, 4, False), (160, 5, True)])
def test_jacobi_solver_beyond_96_levels_matches_the_oracle(hip, Ntot, N, structure):
    """JACOBI_SOLVER (src/linear_solvers.jl:110-153) on the cooperative kernels with 7 .. 16 waves per slab: early exit,
    iteration cap, a three-node ensemble with loose tolerances (convergence is tested per sample like the reference: 1e-10)."""
    from oracle.oracle import Oracle
    from test_gpu_random import random_problem
    jq = hip
    rng = np.random.default_rng(77 + Ntot)
    p, pcof = random_problem(jq, rng, Ntot, N, 2, 1, 6, 4, 1, structure)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    for max_iter, tol in ((40, 1e-13), (3, 1e-30), (40, 1e-6)):
        p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER, max_iter=max_iter, tol=tol, nrhs=1)
        r = Oracle(p, use_sparse=False).traceobjgrad(pcof)
        objfv, tg, *_ = jq.traceobjgrad(pcof, p, wa, False, True)
        assert wa.last_timing()["kernel_family"] == 1
        assert abs(objfv - r["objfv"]) <= 1e-10 * abs(r["objfv"])      # (per-sample convergence test: irrespective of tol)
        assert rel(tg, r["totalgrad"]) < 1e-10
    nodes, weights, shift = 0.3 * rng.standard_normal(3), rng.random(3), 0.3 * rng.standard_normal(Ntot)
    shift[0] = 0.0      # (the reference shifts the levels j >= 2 only, src/ipopt_interface.jl:41-44)
    for tol in (1e-13, 1e-6, 1e-4):      # loose tolerances: the samples of the slab stop after different iteration counts
        p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER, max_iter=40, tol=tol, nrhs=1)
        ref = Oracle(p, use_sparse=False).eval_f_g_grad(pcof, nodes, weights, shift)
        jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
        assert abs(p.last_infidelity - ref["last_infidelity"]) <= 1e-10 * abs(ref["last_infidelity"])
        assert rel(p.last_infidelity_grad, ref["last_infidelity_grad"]) < 1e-10
    wa.close()


@pytest.mark.parametrize("Ng3,oft", [(1, 1), (2, 3), (5, 2)])
def test_cooperative_quad_kernels_with_single_subsystem_controls_match_the_oracle(hip, Ng3, oft):
    """cnot3-type problems (control q acts on subsystem q only: the trace products of the cooperative-quad backward sweep use one
    part of the product each) against the oracle, and against the same kernels with the branch-free full trace products
    (JQ_CQ_GENERIC_TRACES=1); Ntot = 32 / 48 / 96, 7 time steps, objFuncType 1 / 3 / 2, a five-node ensemble."""
    from oracle.oracle import Oracle
    jq = hip
    params, info = jq.cases.cnot3(Ng3=Ng3)
    params.nsteps = 7
    params.T = params.T * 7 / 32386
    params.objFuncType = oft
    rng = np.random.default_rng(Ng3)
    pcof = 0.02 * rng.standard_normal(info["nCoeff"])
    r = Oracle(params).traceobjgrad(pcof)
    res = []
    for env in ({}, {"JQ_CQ_GENERIC_TRACES": "1"}):
        with jq.options(**env):
            wa = jq.Working_Arrays_HIP(params, pcof.size)
            objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, params, wa, False, True)
            assert wa.last_timing()["kernel_family"] == 8
            nodes, weights, shift = jq.cases.cnot3_ensemble(5)
            jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=np.arange(params.Ntot) * 1.0)
            res.append((objfv, tg, ig, params.last_infidelity, params.last_infidelity_grad.copy()))
            wa.close()
        gn = np.linalg.norm(r["totalgrad"])
        assert abs(objfv - r["objfv"]) <= 1e-10 * abs(r["objfv"])
        assert np.linalg.norm(tg - r["totalgrad"]) <= 1e-10 * gn and np.linalg.norm(ig - r["infidelgrad"]) <= 1e-10 * gn
    a, b = res
    assert abs(a[0] - b[0]) <= 1e-13 * abs(b[0]) and rel(a[1], b[1]) < 1e-12 and rel(a[4], b[4]) < 1e-12
    assert abs(a[3] - b[3]) <= 1e-13 * abs(b[3])


@pytest.mark.gpu
def test_handles_release_their_device_memory(hip):
    """jq_destroy gives back everything a handle allocated (operators, state batches, the split-batch buffers, the ensemble
    results): 30 create / evaluate / destroy cycles over the kernel families leave the device's free memory where it was."""
    import ctypes
    import gc
    from juqbox_jl_amd import _lib
    jq = hip
    L = _lib.load()
    L.hipMemGetInfo.restype = ctypes.c_int

    def free_bytes():
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        assert L.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value

    def cycle(case, nsamples):
        params, info = getattr(jq.cases, case)()
        params.T = params.T * 40 / params.nsteps
        params.nsteps = 40
        pcof = 0.01 * np.cos(np.arange(info["nCoeff"]) + 1.0)
        wa = jq.Working_Arrays_HIP(params, pcof.size)
        jq.traceobjgrad(pcof, params, wa, False, True)
        nodes = np.linspace(-1e-4, 1e-4, nsamples)
        weights = np.full(nsamples, 1.0 / nsamples)
        shift = np.arange(params.Ntot, dtype=np.float64) % 3
        shift[0] = 0.0
        jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
        assert np.isfinite(params.last_infidelity)
        wa.close()

    cycle("cnot3", 1100)                  # (first use: module load, RCCL-free single device, allocator pools)
    gc.collect()
    before = free_bytes()
    for k in range(10):
        cycle("cnot3", 1100 + 7 * k)      # split batches (full round + remainder) on the quad-layout kernels
        cycle("cnot2", 300)
        cycle("rabi", 64)
    gc.collect()
    after = free_bytes()
    assert abs(before - after) <= 8 << 20, "device memory not returned: %d bytes" % (before - after)
