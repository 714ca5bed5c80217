"""GPU (-m gpu): what the round-2 verdict asked for first.

 (1) the ndev > 1 code of a multi-device handle -- host threads, one stream per sub-handle, sharding (jq_shard_bounds), per-device
     packing, the sum over the devices -- EXECUTED on this one-GPU box through the test mode JQ_MULTI_SAME_DEVICE=1 (K sub-handles
     on one physical GPU, the ncclAllReduce replaced by a host-side sum in device order; everything else is the production code):
     results against the single-device handle (which the oracle pins) for ragged shards, shards without samples, objFuncType 3,
     the embedded / quad-layout families, sweeps, mutations; looped to shake out threading problems;
 (2) bitwise run-to-run reproducibility of EVERY kernel family as the race detector ("deterministic
     reduction order + bitwise run-to-run check"): the same evaluation three times on one handle and once on a fresh handle must
     agree bit for bit -- objective, gradients, ensemble sums, sampled state history -- including the path bench.py times;
 (3) a librccl that cannot be loaded is an error code, not a crash (advisor finding of round 2);
 (4) bench.py in the driver's launcher form (python -m torch.distributed.run --nproc-per-node 1 ... bench.py --gpus 1)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT, case_inputs

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def hip(jq):
    from juqbox_jl_amd import _lib
    assert _lib.load().jq_device_count() >= 1, "no HIP device: the hot path has no CPU fallback"
    return jq


@pytest.fixture()
def same_device(jq):
    with jq.options(multi_same_device=1):      # (option of the multi-device handles created inside: jq_create_multi_opts)
        yield


def _ensemble(params, nquad, seed=0):
    rng = np.random.default_rng(seed)
    x, w = np.polynomial.legendre.leggauss(max(nquad, 1))
    nodes, weights = x[:nquad] * 0.5 * (2 * np.pi * 2e-2), w[:nquad] * 0.5 + 0.01 * rng.random(nquad)
    shift = None if params.Ntot <= 4 else 0.05 * np.arange(params.Ntot)
    return nodes, weights, shift


def _short_cnot3(jq, nsteps=120):
    params, info, pcof, _ = case_inputs("cnot3")
    params.T = params.T * nsteps / params.nsteps
    params.nsteps = nsteps
    return params, pcof


# ---- (1) multi-device handle with K > 1 sub-handles ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,nquad,K", [("swap02_rn", 64, 2), ("swap02_rn", 13, 4), ("swap02_rn", 3, 8), ("cnot2-leakieq", 5, 2),
                                          ("cnot2-leakieq", 11, 3), ("cnot3-short", 9, 4), ("cnot3-short", 70, 3)])
def test_multi_handle_with_K_subhandles_matches_the_single_handle(hip, same_device, case, nquad, K):
    """K sub-handles (host threads, own streams) on one GPU: ragged shards (13 over 4, 11 over 3), shards WITHOUT samples
    (3 nodes over 8 devices), objFuncType 3 (two backward passes, leak gradient), cnot3 on the cooperative-quad / quad-layout
    kernels.  The single-device result is pinned by the oracle elsewhere; agreement to 1e-13 (the order of the sum over the
    samples differs), per-sample sweep outputs bit for bit."""
    jq = hip
    if case == "cnot3-short":
        params, pcof = _short_cnot3(jq)
    else:
        params, info, pcof, _ = case_inputs(case)
    nodes, weights, shift = _ensemble(params, nquad)
    wa1 = jq.Working_Arrays_HIP(params, pcof.size)
    jq.eval_f_g_grad(pcof, params, wa1, nodes, weights, True, shift=shift)
    a = (params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy(), params.last_leak_grad.copy())
    sw1 = jq.traceobj_sweep(pcof, params, wa1, nodes, shift)
    t1 = jq.traceobjgrad(pcof, params, wa1, False, True)
    wam = jq.Working_Arrays_HIP(params, pcof.size, devices=K)
    assert wam.num_devices == K
    for rep in range(3):
        jq.eval_f_g_grad(pcof, params, wam, nodes, weights, True, shift=shift)
        assert abs(params.last_infidelity - a[0]) <= 1e-13 * abs(a[0])
        assert abs(params.last_leak - a[1]) <= 1e-13 * max(abs(a[1]), 1e-6)
        assert rel(params.last_infidelity_grad, a[2]) < 1e-13
        if params.objFuncType != 1:
            assert np.linalg.norm(params.last_leak_grad - a[3]) <= 1e-13 * np.linalg.norm(a[2])
    t = wam.last_timing()
    assert t["svts"] == nquad * params.N * params.nsteps          # work of all shards
    assert 0.0 < t["ms_shard_min"] <= t["ms_shard_max"] and t["ms_allreduce"] >= 0.0
    assert np.array_equal(jq.traceobj_sweep(pcof, params, wam, nodes, shift), sw1)      # independent outputs: bit for bit
    tm = jq.traceobjgrad(pcof, params, wam, False, True)                                # single evaluation: first device
    assert tm[0] == t1[0] and np.array_equal(tm[1], t1[1])
    # forward-only ensemble (compute_adjoint = false) and a mutation that must reach every sub-handle
    jq.eval_f_g_grad(pcof, params, wam, nodes, weights, False, shift=shift)
    assert abs(params.last_infidelity - a[0]) <= 1e-13 * abs(a[0]) and not params.last_infidelity_grad.any()
    params.linear_solver.max_iter = 1          # (far from converged: the result must change)
    jq.eval_f_g_grad(pcof, params, wam, nodes, weights, True, shift=shift)
    b = (params.last_infidelity, params.last_infidelity_grad.copy())
    jq.eval_f_g_grad(pcof, params, wa1, nodes, weights, True, shift=shift)
    assert b[0] != a[0] and abs(b[0] - params.last_infidelity) <= 1e-13 * abs(b[0]) and rel(b[1], params.last_infidelity_grad) < 1e-13
    wam.close()
    wa1.close()


def test_multi_handle_threads_twenty_rounds(hip, same_device):
    """20 rounds with changing pcof, ensemble size and shard pattern on ONE 4-sub-handle object next to a single-device handle:
    shared state between the host threads (error strings, capacities, timing) would show up as a mismatch or a crash."""
    jq = hip
    params, info, pcof, _ = case_inputs("swap02_rn")
    rng = np.random.default_rng(11)
    wa1 = jq.Working_Arrays_HIP(params, pcof.size)
    wam = jq.Working_Arrays_HIP(params, pcof.size, devices=4)
    for rnd in range(20):
        nquad = int(rng.integers(1, 40))
        pc = pcof * (1.0 + 0.05 * rng.standard_normal(pcof.size))
        nodes, weights, shift = _ensemble(params, nquad, seed=rnd)
        jq.eval_f_g_grad(pc, params, wa1, nodes, weights, True, shift=shift)
        a = (params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy())
        jq.eval_f_g_grad(pc, params, wam, nodes, weights, True, shift=shift)
        assert abs(params.last_infidelity - a[0]) <= 1e-13 * abs(a[0]), rnd
        assert abs(params.last_leak - a[1]) <= 1e-13 * max(abs(a[1]), 1e-6), rnd
        assert rel(params.last_infidelity_grad, a[2]) < 1e-13, rnd
    wam.close()
    wa1.close()


def test_multi_handle_reports_errors_of_a_sub_handle(hip, same_device):
    """a failing shard (wrong pcof length -> the reference's DimensionMismatch) comes back as the error of the multi handle"""
    from juqbox_jl_amd import _lib
    jq = hip
    params, info, pcof, _ = case_inputs("swap02_rn")
    wam = jq.Working_Arrays_HIP(params, pcof.size, devices=3)
    nodes, weights, shift = _ensemble(params, 7)
    with pytest.raises(_lib.JuqboxHipError) as e:
        jq.eval_f_g_grad(pcof[:-1], params, wam, nodes, weights, True, shift=shift)
    assert e.value.code in (_lib.JQ_EINVAL, _lib.JQ_EDIM)
    jq.eval_f_g_grad(pcof, params, wam, nodes, weights, True, shift=shift)          # and the handle still works
    assert np.isfinite(params.last_infidelity)
    wam.close()


def test_same_device_mode_is_off_by_default(hip):
    from juqbox_jl_amd import _lib
    jq = hip
    assert "multi_same_device" not in os.environ.get("JQ_OPTIONS", "")
    params, info, pcof, _ = case_inputs("swap02")
    with pytest.raises(_lib.JuqboxHipError):
        jq.Working_Arrays_HIP(params, pcof.size, devices=[0, 0])


_RCCL_FAIL = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
os.environ["JQ_RCCL_LIB"] = "/nonexistent/librccl.so.1"
import juqbox_jl_amd as jq
from juqbox_jl_amd import _lib
from conftest import case_inputs
params, info, pcof, _ = case_inputs("swap02")
try:
    jq.Working_Arrays_HIP(params, pcof.size, devices=[0])
    print("RESULT created")
except _lib.JuqboxHipError as e:
    print("RESULT code=%d msg=%s" % (e.code, e))
"""


def test_unloadable_rccl_is_an_error_code_not_a_crash(hip):
    """jq_create_multi with a librccl that cannot be loaded returns JQ_EUNSUPPORTED with the loader's message (round 2 built the
    message from TWO dlerror() calls: the second returns NULL -> std::string(NULL) -> SIGSEGV of the host process)."""
    r = subprocess.run([sys.executable, "-c", _RCCL_FAIL.format(root=ROOT)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-1500:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    assert "code=-3" in line and "cannot load librccl" in line, line


# ---- (2) bitwise reproducibility -----------------------------------------------------------------------------------------
def _bitwise_rounds(jq, p, pcof, env, family, imr=False, nq=None, history=True):
    """three evaluations on one handle + one on a fresh handle: objective, gradients, a ragged weighted ensemble and the state
    history must be bit-identical; returns the kernel family that ran"""
    rng = np.random.default_rng(5)
    sps = max(1, 16 // p.N)
    nq = nq or 2 * sps + 1
    nodes, weights = 0.05 * rng.standard_normal(nq), rng.random(nq)
    shift = 0.05 * rng.standard_normal(p.Ntot)
    shift[0] = 0.0
    runs = []
    fam = None
    with jq.options(**env):      # (some knobs are read at jq_create, some per evaluation: set for the whole test)
        for handle in range(2):
            wa = (jq.Working_Arrays_M_HIP if imr else jq.Working_Arrays_HIP)(p, pcof.size)
            for rep in range(3 if handle == 0 else 1):
                o = jq.traceobjgrad(pcof, p, wa, False, True)
                fam = wa.last_timing()["kernel_family"]
                jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
                e = (p.last_infidelity, p.last_leak, p.last_infidelity_grad.copy(), p.last_leak_grad.copy())
                hist = jq.traceobjgrad(pcof, p, wa, True, False)[1][:, :, ::max(1, p.nsteps // 7)] if history else None
                runs.append((o, e, hist))
            wa.close()
    o0, e0, h0 = runs[0]
    for o, e, hist in runs[1:]:
        assert o[0] == o0[0] and o[2] == o0[2] and o[3] == o0[3]
        for k in (1, 5, 6):
            assert np.array_equal(o[k], o0[k])
        assert e[0] == e0[0] and e[1] == e0[1] and np.array_equal(e[2], e0[2]) and np.array_equal(e[3], e0[3])
        if history:
            assert np.array_equal(hist, h0)
    if family is not None:
        assert fam == family, (fam, family)
    return fam


_SV_FAMILIES = [
    # (id, random-problem config (Ntot, N, Nc, Nfreq, nsteps, m, objFuncType, structure), environment, expected kernel family)
    ("rowlane", (12, 4, 2, 2, 40, 5, 3, False), {}, 3),
    ("lane", (8, 3, 3, 2, 40, 2, 1, False), {"JQ_ROWLANE_MAX": "0"}, 2),
    ("slab-dense", (47, 3, 4, 1, 30, 2, 3, False), {"JQ_COOP_MAX": "0", "JQ_LANE": "0", "JQ_QUAD": "0"}, 0),
    ("slab-t4", (96, 4, 3, 1, 30, 6, 1, "t4"), {"JQ_COOP_MAX": "0", "JQ_LANE": "0", "JQ_QUAD": "0"}, 0),
    ("slab-od", (80, 5, 3, 1, 30, 4, 2, "od"), {"JQ_COOP_MAX": "0", "JQ_LANE": "0", "JQ_QUAD": "0"}, 0),
    ("coop", (64, 4, 3, 2, 30, 3, 3, False), {}, 1),
    ("coop-big", (130, 4, 2, 1, 12, 3, 1, True), {}, 1),
    ("quad4", (96, 4, 3, 1, 30, 6, 2, "t4"), {"JQ_CQ": "0"}, 6),
    ("quad8", (96, 4, 3, 1, 30, 6, 1, "t4"), {"JQ_QUAD8": "1"}, 6),
    ("quad12", (96, 4, 3, 1, 30, 6, 3, "t4"), {"JQ_QUAD8": "2"}, 6),
    ("cq", (96, 4, 3, 1, 30, 6, 3, "t4"), {}, 8),
    ("cq-odd-m", (64, 2, 2, 1, 31, 3, 1, "t4"), {}, 8),
]


@pytest.mark.parametrize("name,cfg,env,family", _SV_FAMILIES, ids=[f[0] for f in _SV_FAMILIES])
def test_bitwise_reproducible_stormer_verlet_families(hip, name, cfg, env, family):
    from test_gpu_random import random_problem
    Ntot, N, Nc, Nfreq, nsteps, m, oft, banded = cfg
    p, pcof = random_problem(hip, np.random.default_rng(77 + Ntot), Ntot, N, Nc, Nfreq, nsteps, m, oft, banded)
    _bitwise_rounds(hip, p, pcof, env, family)


_IMR_FAMILIES = [
    ("imr-rowlane", (12, 4, 2, 2, 30, 3, 3, False), {}, 4),
    ("imr-coop", (48, 4, 3, 1, 20, 2, 2, False), {}, 5),
    ("imr-quad", (96, 4, 3, 1, 20, 3, 1, "t4"), {"JQ_IMR_CQ": "0"}, 7),
    ("imr-cq", (96, 4, 3, 1, 20, 3, 3, "t4"), {}, 9),
]


@pytest.mark.parametrize("name,cfg,env,family", _IMR_FAMILIES, ids=[f[0] for f in _IMR_FAMILIES])
def test_bitwise_reproducible_implicit_midpoint_families(hip, name, cfg, env, family):
    from test_gpu_random import random_problem
    jq = hip
    Ntot, N, Nc, Nfreq, nsteps, m, oft, banded = cfg
    p, pcof = random_problem(jq, np.random.default_rng(99 + Ntot), Ntot, N, Nc, Nfreq, nsteps, m, oft, banded)
    p.Integrator_id = jq.Implicit_Midpoint
    p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=60, tol=1e-11, nrhs=N)
    p.wmat = p.wmat_real.copy()
    _bitwise_rounds(jq, p, pcof, env, family, imr=True)


def test_bitwise_reproducible_jacobi_solver(hip):
    """the Stormer-Verlet path with the Jacobi solver (data-dependent iteration counts; slab kernels and, beyond Ntot 96, the
    cooperative ones)"""
    from test_gpu_random import random_problem
    jq = hip
    for Ntot, N, fam in ((40, 3, 0), (112, 4, 1)):
        p, pcof = random_problem(jq, np.random.default_rng(5 + Ntot), Ntot, N, 2, 1, 25, 3, 1, True)
        p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER, max_iter=40, tol=1e-11, nrhs=N)
        _bitwise_rounds(jq, p, pcof, {}, fam, history=False)


def test_bitwise_reproducible_bench_path(hip):
    """the path bench.py times -- cnot3, 3 072 perturbed samples, quad-layout kernels with three slabs per workgroup (12 waves,
    window staging, per-workgroup trace records, fixed-order reductions) -- at 2 000 time steps: the ensemble sums and gradient
    of three evaluations on one handle and one on a fresh handle agree bit for bit; so does a split batch (3 072 + 128)."""
    jq = hip
    params, pcof = _short_cnot3(jq, 2000)
    for ns in (3072, 3200):
        nodes, weights, shift = jq.cases.cnot3_ensemble(ns)
        runs = []
        for handle in range(2):
            wa = jq.Working_Arrays_HIP(params, pcof.size)
            for rep in range(3 if handle == 0 else 1):
                jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
                runs.append((params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy()))
                t = wa.last_timing()
                assert t["kernel_family"] == 6 and t["kernel_band"] == 7
            sw = jq.traceobj_sweep(pcof, params, wa, nodes[:700], shift)
            runs[-1] = runs[-1] + (sw,)
            wa.close()
        for r in runs[1:]:
            assert r[0] == runs[0][0] and r[1] == runs[0][1] and np.array_equal(r[2], runs[0][2])
        assert np.array_equal(runs[2][3], runs[3][3])


# ---- (4) the driver's launcher form -----------------------------------------------------------------------------------------
def test_bench_under_torch_distributed_run_one_rank(hip):
    """`python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port P bench.py --gpus 1
    --steps 1 --warmup 1` (the form the driver uses for N > 1, here with the one GPU of the box): RANK / WORLD_SIZE come from the
    launcher, an nccl process group is initialised, the packed result stays on the device for the all-reduce.  The JSON line
    must carry the contract's keys plus the per-rank and all-reduce timings and the CPU baseline (bounded sample)."""
    port = 29700 + os.getpid() % 250
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", JQ_BENCH_SAMPLES="256")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
           "--strong-samples", "512", "--full", "--quick-extras"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 1 and j["config"]["rccl_world_size"] == 1 and "nccl" in j["config"]["launcher"]
    assert j["value"] > 0 and 0.0 < j["roofline"]["frac"] <= 1.0
    assert j["per_rank_ms"]["min"] <= j["per_rank_ms"]["max"] and j["allreduce_ms"] >= 0.0
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["cores"] == 1
    assert j["strong_scaling"]["total_samples"] == 512 and "strong_scaling_small" in j


def test_plain_bench_run_and_its_dumped_outputs(hip, tmp_path):
    """`bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR`: the line of a plain run carries no side measurement (those
    need --full), and DIR holds what the last timed step returned -- the same numbers as one evaluation of the same inputs here."""
    jq = hip
    ns = 256
    env = dict(os.environ, JQ_BENCH_SAMPLES=str(ns))
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0 and j["dtype"] == "f64"
    for k in ("strong_scaling", "cpu_baseline", "single_evaluation", "dense_operator", "baseline_configs"):
        assert k not in j, k
    assert "issue_bound" not in j["roofline"]
    dumped = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert set(dumped) == {"infidelity", "leak", "infidelity_grad"}, sorted(dumped)
    assert all(a.dtype == np.float64 for a in dumped.values())
    assert dumped["infidelity"][0] == j["ensemble_infidelity"]
    params, info, pcof, _ = case_inputs("cnot3")
    nodes, weights, shift = jq.cases.cnot3_ensemble(ns)
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
    wa.close()
    assert rel(dumped["infidelity"], params.last_infidelity) < 1e-12 and rel(dumped["leak"], params.last_leak) < 1e-12
    assert rel(dumped["infidelity_grad"], params.last_infidelity_grad) < 1e-12


# ---- (5) more than four control Hamiltonians, drift updates outside the planned structure -------------------------------------
_MANY_CONTROLS = [
    # id, (Ntot, N, Nc, Nfreq, nsteps, m, objFuncType, structure), environment, implicit midpoint
    ("rowlane-5", (12, 4, 5, 1, 25, 3, 1, False), {}, False),
    ("lane-7", (8, 3, 7, 1, 20, 2, 3, False), {"JQ_ROWLANE_MAX": "0"}, False),
    ("slab-dense-6", (40, 3, 6, 1, 12, 2, 2, False), {"JQ_COOP_MAX": "0", "JQ_LANE": "0", "JQ_QUAD": "0"}, False),
    ("coop-8", (64, 4, 8, 1, 10, 3, 1, False), {}, False),
    ("coop-big-5", (130, 2, 5, 1, 8, 2, 3, True), {}, False),
    ("cq-6", (96, 4, 6, 1, 12, 6, 3, "t4"), {}, False),
    ("quad12-5", (96, 4, 5, 2, 10, 5, 1, "t4"), {"JQ_QUAD8": "2"}, False),
    ("slab-t4-7", (48, 4, 7, 1, 10, 3, 2, "t4"), {"JQ_COOP_MAX": "0", "JQ_LANE": "0", "JQ_QUAD": "0"}, False),
    ("slab-od-5", (80, 5, 5, 1, 8, 4, 1, "od"), {"JQ_COOP_MAX": "0", "JQ_LANE": "0", "JQ_QUAD": "0"}, False),
    ("imr-rowlane-5", (12, 4, 5, 1, 15, 3, 3, False), {}, True),
    ("imr-coop-6", (48, 4, 6, 1, 8, 2, 1, False), {}, True),
    ("imr-cq-5", (96, 4, 5, 1, 8, 3, 2, "t4"), {}, True),
    ("imr-quad-7", (64, 2, 7, 1, 8, 3, 1, "t4"), {"JQ_IMR_CQ": "0"}, True),
]


@pytest.mark.parametrize("name,cfg,env,imr", _MANY_CONTROLS, ids=[c[0] for c in _MANY_CONTROLS])
def test_more_than_four_controls_match_the_oracle(hip, name, cfg, env, imr):
    """objparams has no limit on the number of control Hamiltonians (src/evalobjgrad.jl:152-343); the kernels' trace / carry
    bookkeeping holds four, so the backward sweep runs once per group of at most four controls (5 .. 8 controls: two sweeps,
    each with its own trace images; K(t), S(t) always contain every control).  Objective, all three gradients and a weighted
    ensemble against the oracle on every kernel family, both integrators."""
    from oracle.oracle import Oracle
    from test_gpu_random import random_problem
    jq = hip
    Ntot, N, Nc, Nfreq, nsteps, m, oft, banded = cfg
    rng = np.random.default_rng(300 + Ntot + Nc)
    p, pcof = random_problem(jq, rng, Ntot, N, Nc, Nfreq, nsteps, m, oft, banded)
    if imr:
        p.Integrator_id = jq.Implicit_Midpoint
        p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=80, tol=1e-12, nrhs=N)
        p.wmat = p.wmat_real.copy()
    with jq.options(**env):
        wa = (jq.Working_Arrays_M_HIP if imr else jq.Working_Arrays_HIP)(p, pcof.size)
        orc = Oracle(p, use_sparse=False)
        r = orc.traceobjgrad_imr(pcof, 80, 1e-12) if imr else orc.traceobjgrad(pcof)
        objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, p, wa, False, True)
        gn = np.linalg.norm(r["totalgrad"])
        # Stormer-Verlet: the reference's own tolerance; implicit midpoint: the fixed-point solver stops at ITS tolerance (1e-12 per
        # evaluation and step, accumulated over the steps and amplified by the random problem's conditioning): 1e-9
        tol = 1e-9 if imr else 1e-10
        assert abs(prim - r["primaryobjf"]) <= tol and abs(sec - r["secondaryobjf"]) <= tol * max(abs(r["secondaryobjf"]), 1e-3)
        assert np.linalg.norm(tg - r["totalgrad"]) <= tol * gn
        assert np.linalg.norm(ig - r["infidelgrad"]) <= tol * gn
        if oft != 1:
            assert np.linalg.norm(lg - r["leakgrad"]) <= tol * gn
        # every control's block of the gradient is non-trivial and right (a group that was skipped would leave zeros)
        per = pcof.size // Nc
        for q in range(Nc):
            blk = slice(q * per, (q + 1) * per)
            assert np.linalg.norm(r["totalgrad"][blk]) > 0
            assert np.linalg.norm(tg[blk] - r["totalgrad"][blk]) <= tol * gn
        if not imr:
            nq = 2 * max(1, 16 // N) + 1
            nodes, weights = 0.1 * rng.standard_normal(nq), rng.random(nq)
            shift = rng.standard_normal(Ntot) * 0.05
            shift[0] = 0.0
            ref = orc.eval_f_g_grad(pcof, nodes, weights, shift)
            jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
            gref = ref["last_infidelity_grad"]
            assert abs(p.last_infidelity - ref["last_infidelity"]) <= tol * abs(ref["last_infidelity"])
            assert np.linalg.norm(p.last_infidelity_grad - gref) <= tol * np.linalg.norm(gref)
            if oft != 1:
                assert np.linalg.norm(p.last_leak_grad - ref["last_leak_grad"]) <= tol * np.linalg.norm(gref)
        wa.close()


# (round 6: more than 16 controls are no longer refused -- tests/test_gpu_round6.py test_more_than_16_control_hamiltonians)


@pytest.mark.parametrize("structure,Ntot,imr", [("t4", 96, False), ("od", 80, False), (True, 50, False), ("t4", 64, True)])
def test_hconst_update_outside_the_planned_structure_replans(hip, structure, Ntot, imr):
    """Scripts mutate params.Hconst arbitrarily (src/ipopt_interface.jl:41-44, run_all.jl:13-15).  A new drift with entries outside
    the structure the kernels were chosen for (4 x 4 x n Kronecker structure, diagonal off-diagonal blocks, block band) re-plans
    the handle in place (round 2: JQ_EUNSUPPORTED): results against the oracle with the dense drift, then back with the structured
    one -- where the fast kernel family must be in use again."""
    from oracle.oracle import Oracle
    from test_gpu_random import random_problem
    jq = hip
    rng = np.random.default_rng(41 + Ntot)
    p, pcof = random_problem(jq, rng, Ntot, 4, 3, 1, 10, 3, 3, structure)
    if imr:
        p.Integrator_id = jq.Implicit_Midpoint
        p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=80, tol=1e-12, nrhs=4)
        p.wmat = p.wmat_real.copy()
    wa = (jq.Working_Arrays_M_HIP if imr else jq.Working_Arrays_HIP)(p, pcof.size)
    p.linear_solver.max_iter += 0
    H0 = p.Hconst.copy()

    def check():
        orc = Oracle(p, use_sparse=False)
        r = orc.traceobjgrad_imr(pcof, 80, 1e-12) if imr else orc.traceobjgrad(pcof)
        objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, p, wa, False, True)
        gn = np.linalg.norm(r["totalgrad"])
        tol = 1e-9 if imr else 1e-10      # (implicit midpoint: bounded by the fixed-point solver's own tolerance, see above)
        assert abs(prim - r["primaryobjf"]) <= tol and np.linalg.norm(tg - r["totalgrad"]) <= tol * gn
        assert np.linalg.norm(lg - r["leakgrad"]) <= tol * gn
        return wa.last_timing()
    t0 = check()
    D = rng.standard_normal((Ntot, Ntot))
    p.Hconst = H0 + 0.05 * (D + D.T)                    # dense: outside every structure
    t1 = check()
    assert (t1["kernel_family"], t1["kernel_band"]) != (t0["kernel_family"], t0["kernel_band"])
    p.Hconst = H0 * 1.01                                # structured again: the plan comes back
    t2 = check()
    assert (t2["kernel_family"], t2["kernel_band"]) == (t0["kernel_family"], t0["kernel_band"])
    wa.close()


@pytest.mark.parametrize("Ntot", [120, 130, 150])
def test_dense_operators_beyond_96_levels_whose_band_equals_a_structure_code(hip, Ntot):
    """Dense operators with NT = 8, 9, 10 tile rows: their block band NT - 1 = 7, 8, 9 equals the codes of the quad-layout /
    JQ_BW_T4 / JQ_BW_OD structures.  Round 2 mistook such handles for structured ones: kernel families that do not exist at this
    size (JQ_EUNSUPPORTED at NT = 9) and, at NT = 10, the JQ_BW_OD product for a dense matrix (WRONG results, Ntot 145 .. 160).
    Dense is band code 15 at every NT > 6 now; both integrators against the oracle."""
    from oracle.oracle import Oracle
    from test_gpu_random import random_problem
    jq = hip
    p, pcof = random_problem(jq, np.random.default_rng(900 + Ntot), Ntot, 3, 2, 1, 4, 2, 3, False)
    wa = jq.Working_Arrays_HIP(p, pcof.size)
    r = Oracle(p, use_sparse=False).traceobjgrad(pcof)
    objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, p, wa, False, True)
    assert wa.last_timing()["kernel_family"] == 1 and wa.last_timing()["kernel_band"] == 15      # (dense at this size: band code 15)
    gn = np.linalg.norm(r["totalgrad"])
    assert abs(prim - r["primaryobjf"]) <= 1e-10 and np.linalg.norm(tg - r["totalgrad"]) <= 1e-10 * gn
    assert np.linalg.norm(lg - r["leakgrad"]) <= 1e-10 * gn
    wa.close()
    p.Integrator_id = jq.Implicit_Midpoint
    p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=60, tol=1e-11, nrhs=3)
    p.wmat = p.wmat_real.copy()
    wm = jq.Working_Arrays_M_HIP(p, pcof.size)
    r = Oracle(p, use_sparse=False).traceobjgrad_imr(pcof, 60, 1e-11)
    objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, p, wm, False, True)
    assert wm.last_timing()["kernel_family"] == 5
    gn = np.linalg.norm(r["totalgrad"])
    # (implicit midpoint with tol = 1e-11 per step: the solver's tolerance bounds the agreement, not the arithmetic)
    assert abs(prim - r["primaryobjf"]) <= 1e-9 and np.linalg.norm(tg - r["totalgrad"]) <= 1e-9 * gn, "implicit midpoint: solver tolerance 1e-11"
    wm.close()


@pytest.mark.parametrize("case", ["swap02", "cnot2-leakieq", "flux"])
def test_rowlane_backward_sweep_on_two_and_three_waves_equals_the_one_wave_kernel(hip, case):
    """k_backward_rowlane3 (state chain | adjoint chain | traces on three waves: the default for small batches since round 6) and
    k_backward_rowlane2 (state chain | adjoint chain + traces, option rl_split=2) against k_backward_rowlane (rl_split=0): each
    quantity's arithmetic is the same instruction sequence, so objective and gradients agree to the last bits; single evaluations
    and a ragged ensemble; the golden through the default kernel."""
    jq = hip
    params, info, pcof, golden = case_inputs(case)
    res = {}
    for tag, opt, variant in (("three", None, 33), ("two", {"rl_split": 2}, 32), ("one", {"rl_split": 0}, 0)):
        wa = jq.Working_Arrays_HIP(params, pcof.size, options=opt)
        o = jq.traceobjgrad(pcof, params, wa, False, True)
        assert wa.last_timing()["kernel_family"] == 3 and wa.last_timing()["kernel_variant"] == variant
        nodes, weights, shift = _ensemble(params, 7, seed=3)
        jq.eval_f_g_grad(pcof, params, wa, nodes, weights, True, shift=shift)
        res[tag] = (o, params.last_infidelity, params.last_leak, params.last_infidelity_grad.copy(), params.last_leak_grad.copy())
        wa.close()
    b = res["one"]
    for tag in ("three", "two"):
        a = res[tag]
        assert a[0][0] == b[0][0]                                  # (the forward sweep is the same kernel)
        for k in (1, 5, 6):
            assert rel(a[0][k], b[0][k]) < 1e-14 or not np.any(b[0][k])
        assert a[1] == b[1] and a[2] == b[2] and rel(a[3], b[3]) < 1e-14
    for k in (1, 5, 6):                                            # two and three waves: the same sums in the same order -- bit for bit
        assert np.array_equal(res["three"][0][k], res["two"][0][k])
    assert np.array_equal(res["three"][3], res["two"][3]) and np.array_equal(res["three"][4], res["two"][4])


def test_plan_info_describes_the_handle(hip):
    """jq_plan_info: structure found in the operators, control groups and the batch-size thresholds of the kernel families -- one
    place where a caller (and a reviewer) can read what the ~30 JQ_* knobs and the plan constants amount to for a problem."""
    jq = hip
    params, info, pcof, _ = case_inputs("cnot3")
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    p = wa.plan_info()
    assert p["Ntot"] == 96 and p["N"] == 4 and p["tile_rows"] == 6 and p["structure"] == "t4" and p["controls"] == 3 and p["control_groups"] == 1
    fams = {f["family"]: f for f in p["families"]}
    assert 8 in fams and fams[8]["max_quads"] == 2 * p["compute_units"] and 6 in fams and 0 in fams and 3 not in fams
    wa.close()
    params, info, pcof, _ = case_inputs("cnot2")                       # 3 x 4 levels: row-lane kernels + the embedded 4 x 4 x 1 twin
    wa = jq.Working_Arrays_HIP(params, pcof.size)
    p = wa.plan_info()
    assert p["embedded_twin_Ntot"] == 16 and p["families"][0]["family"] == 3 and p["families"][0]["max_columns"] == 32 * p["compute_units"]
    wa.close()
