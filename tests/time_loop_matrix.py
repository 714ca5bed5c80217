"""The time-loop matrix (tests/test_time_loop_matrix.py, tests/test_gpu_time_loop.py): the cells of the block-band matrix
(tests/block_band_matrix.py, at Ntot = 16 NT - 3), of the structured matrix (tests/structured_matrix.py) and of a table of small systems
(Ntot <= 16: lane, row-lane, their implicit-midpoint kernels and the NT = 1 slab / cooperative objects) and of the objects with the
low-rank terms of full leakage weights (w_*, x_*) crossed with the time loop --
problems of 1, 2, 8, 9 and 11 steps in one chunk and in chunks of 1, 2, 3 and 4 steps, with the Neumann order rotating over 0 .. 6.
The three matrices it draws on run 7 steps in one chunk and in chunks of 3 + 3 + 1 at one Neumann order per cell: no chunk of even
length, no problem shorter than its rings, m = 2 nowhere.

A run is (cell, nsteps, chunk_steps, m).  Its problem is the source cell's with T = h * nsteps at the source's own step size
h = T / nsteps (a 1-step problem over the whole horizon would test the divergence of the Jacobi iterations, not the loop); there is one
handle per (cell, step count): the two 2-step runs share theirs, the chunking changed through jq_set_option.  The problems, the options, the solver settings and the expected objects / last_kernels records are the source
matrices'; what the time loop changes in a record is recomputed here: `modd` of the cooperative-quad objects follows the run's m, the
split latency kernels take three workgroups only while the first backward chunk exceeds their 8-step ring (jq_host_plan.h
JQ_CQ3_RING), so runs A1 .. A6 expect the one-workgroup kernel on those cells and the runs A7 .. A9 exist for them alone.

Below the matrix: three sweeps on one representative per kernel template of csrc/jq_inst_list.h (TEMPLATES) -- the step count 1 .. 17 in
one chunk, the Neumann order 0 .. 12 on one handle, a trace budget that shortens the chunks of a gradient evaluation -- and the cells of
the tangent-linear sweeps (TL_CELLS: JVP, HVP, ensemble and drift-ensemble HVP over the runs A1 and A4 .. A6)."""
import collections
import threading
import zlib

import numpy as np

import block_band_matrix as B
import structured_matrix as M

# chunk 0: one chunk; mslot: "r0" / "r1" / "r2" rotate, "zero", "odd", "even", "own" (the source cell's order) or the order itself;
# bwd: steps of a chunk of a GRADIENT evaluation where the trace budget (option trace_bytes) makes it shorter than chunk_steps (0: it does not)
Run = collections.namedtuple("Run", "name nsteps chunk mslot bwd", defaults=(0,))
RUNS = (Run("A1", 1, 0, "r0"), Run("A2", 2, 0, "r1"), Run("A3", 2, 1, "r2"), Run("A4", 9, 2, "zero"), Run("A5", 8, 3, "odd"), Run("A6", 11, 4, "even"))
# the cells of the split latency kernels only: a first chunk longer than the ring (9: the shortest that splits), last chunks of 2 and 1
SPLIT_RUNS = (Run("A7", 9, 0, "r0"), Run("A8", 20, 9, "r1"), Run("A9", 21, 10, "r2"))
ENSEMBLE_RUN = "A5"
RING = 8      # jq_host_plan.h JQ_CQ3_RING
ODD, EVEN = (1, 3, 5), (2, 4, 6)


def chunks(run):
    """the chunk lengths of a run, first to last"""
    cs = run.chunk or run.nsteps
    return [cs] * (run.nsteps // cs) + ([run.nsteps % cs] if run.nsteps % cs else [])


def first_backward_chunk(run):
    return run.bwd or chunks(run)[0]


def m_of(index, run):
    """the Neumann order of a run on the index-th Neumann cell of a route: A4 none, A5 odd, A6 even, rotating with the cell; A1 .. A3
    (A7 .. A9) take the three classes none / odd / even in an order that rotates with the cell, with values one and two places ahead of
    A5's and A6's -- three consecutive cells of a route see every class on every run and every order 0 .. 6"""
    if run.mslot == "zero":
        return 0
    if run.mslot == "odd":
        return ODD[index % 3]
    if run.mslot == "even":
        return EVEN[index % 3]
    cls = (index + int(run.mslot[1])) % 3
    return (0, ODD[(index + 1) % 3], EVEN[(index + 2) % 3])[cls]


# ---- the small systems (Ntot <= 16): test_gpu_random.random_problem, dense, Nc = 2, Nfreq = 2, objFuncType 3 ---------------------------------
# timing: (kernel_family, kernel_size, kernel_band, kernel_variant) of jq_last_timing; forb: real forbidden states (full weights of that rank)
# split: default options on the dense cooperative-quad policy -- the split latency kernels (variant 3) once the first backward chunk exceeds their ring
# gen: (Nc, Nfreq, banded) of random_problem; cplx: complex forbidden states
Small = collections.namedtuple("Small", "name tag Ntot N kind opts timing forb split gen cplx", defaults=(False, (2, 2, False), False))
LANE_NP, ROWLANE_NPJ = (2, 4, 6, 8), (2, 4, 6, 8, 12, 16)      # csrc/Makefile LANE, ROWLANE
SLAB_OPTS = {"coop_max": 0, "lane": 0, "dq": 0, "quad": 0}      # (block_band_matrix.options of a slab route)


def padded(Ntot, sizes):
    return min(s for s in sizes if s >= Ntot)


def _small():
    out = []

    def add(name, tag, Ntot, kind, opts, timing, N=None, forb=0):
        out.append(Small(name, tag, Ntot, N or (2 if Ntot == 2 else 3), kind, dict(opts), tuple(timing), forb))

    for Ntot in (2, 3, 5, 7):
        NP = padded(Ntot, LANE_NP)
        add("lane-Ntot%d" % Ntot, "l_%d" % NP, Ntot, "neumann", {"rowlane_max": 0}, (2, NP, 0, 0))
    for Ntot in (2, 3, 5, 7, 9, 13, 16):
        NPJ = padded(Ntot, ROWLANE_NPJ)
        add("rowlane-three-Ntot%d" % Ntot, "r_%d" % NPJ, Ntot, "neumann", {}, (3, NPJ, 0, 33))
    for Ntot in (5, 9, 13):
        NPJ = padded(Ntot, ROWLANE_NPJ)
        add("rowlane-two-Ntot%d" % Ntot, "r_%d" % NPJ, Ntot, "neumann", {"rl_split": 2}, (3, NPJ, 0, 32))
        add("rowlane-one-Ntot%d" % Ntot, "r_%d" % NPJ, Ntot, "neumann", {"rl_split": 0}, (3, NPJ, 0, 0))
    for Ntot in (5, 13):      # full weights (WF, HIST instantiations): one wave
        NPJ = padded(Ntot, ROWLANE_NPJ)
        add("rowlane-wlr-Ntot%d" % Ntot, "r_%d" % NPJ, Ntot, "neumann", {}, (3, NPJ, 0, 0), forb=2)
    for Ntot in (2, 3, 5, 7, 9, 13):
        NPJ = padded(Ntot, ROWLANE_NPJ)
        add("rowlane-imr-two-Ntot%d" % Ntot, "m_%d" % NPJ, Ntot, "imr", {}, (4, NPJ, 0, 32))
    for Ntot in (5, 9, 13):
        NPJ = padded(Ntot, ROWLANE_NPJ)
        add("rowlane-imr-one-Ntot%d" % Ntot, "m_%d" % NPJ, Ntot, "imr", {"rl_split": 0}, (4, NPJ, 0, 0))
    add("coop-imr-Ntot13", "i_1_0", 13, "imr", {}, (5, 1, 0, 0), N=6)
    add("slab-neumann-Ntot13", "k_1_0", 13, "neumann", SLAB_OPTS, (0, 1, 0, 0))
    add("slab-jacobi-Ntot13", "j_1_0", 13, "jacobi", SLAB_OPTS, (0, 1, 0, 0))
    # ---- the objects with the low-rank terms of full leakage weights, on the problems and options of tests/test_gpu_round6.py (2), (6) and
    #      tests/test_gpu_dense_wmat.py: quad layout (five complex forbidden states, so that the cooperative-quad kernels do not take them),
    #      the one-tile-row slab object, the dense 96 x 96 slab object; x_: the same with the Jacobi solver
    for NT in range(1, 9):
        out.append(Small("weighted-quad-NT%d" % NT, "w_%d_7" % NT, 16 * NT, 4, "neumann", {"lane": 0} if NT == 1 else {}, (6, NT, 7, 0), 5, False, (2, 1, "t4"), True))
    dense96 = {"force_dense": 1, "embed": 0, "coop_max": 0}
    out.append(Small("weighted-slab-Ntot12", "w_1_0", 12, 3, "neumann", {"lane": 0, "embed": 0}, (0, 1, 0, 0), 3, False, (2, 1, False), True))
    out.append(Small("weighted-slab-Ntot96", "w_6_5", 96, 4, "neumann", dense96, (0, 6, 5, 0), 2, False, (2, 1, False), True))
    out.append(Small("weighted-jacobi-Ntot12", "x_1_0", 12, 3, "jacobi", {}, (0, 1, 0, 0), 2, False, (1, 1, False), False))
    out.append(Small("weighted-jacobi-Ntot96", "x_6_5", 96, 4, "jacobi", dense96, (0, 6, 5, 0), 2, False, (2, 1, False), True))
    return tuple(out)


SMALL = _small()
SMALL_BY_NAME = {s.name: s for s in SMALL}
SMALL_NSTEPS, SMALL_M, SMALL_ENS = 7, 3, 7
# seeds of small problems (default: the CRC of the name).  lane-Ntot5: with the default the Neumann sweep's terms show at factor 16 only, where
# one ulp in the coefficients moves the oracle's gradient by 2.8e-12 relative (tests/test_time_loop_matrix.py asks for <= 1e-12)
SMALL_SEEDS = {"lane-Ntot5": 1}

# ---- the cells ---------------------------------------------------------------------------------------------------------------------------
# source "band": key (block_band_matrix.Cell, Ntot); "structured": key structured_matrix.Cell; "small": key Small.
# route: the cells a Neumann order rotates over; index: the cell's place among the Neumann cells of its route (None: Jacobi / implicit midpoint)
Cell = collections.namedtuple("Cell", "name source key route kind index")


def _cells():
    out, turn = [], collections.Counter()

    def add(name, source, key, route, kind):
        index = None
        if kind == "neumann":
            index, turn[route] = turn[route], turn[route] + 1
        out.append(Cell(name, source, key, route, kind, index))

    for bc in B.CELLS:
        if bc.tag is not None:
            Ntot = 16 * bc.NT - 3
            add("band-" + B.cell_id(bc, Ntot), "band", (bc, Ntot), "band-" + bc.route, B.kind_of(bc.route))
    for sc in M.CELLS:
        if sc.name not in M.REFUSED:
            add("t4-" + sc.name, "structured", sc, "t4-" + sc.route, sc.kind)
    for s in SMALL:
        route = {"l": "lane", "r": "rowlane", "m": "rowlane-imr", "i": "band-coop-imr", "k": "band-slab-neumann", "j": "band-slab-jacobi",
                 "w": "weighted", "x": "weighted-jacobi"}[s.tag[0]]
        add("small-" + s.name, "small", s, route, s.kind)
    return tuple(out)


CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
assert len(BY_NAME) == len(CELLS)
# propagator objects of csrc/Makefile that no cell of this table runs, and why
UNREACHABLE = dict(M.UNREACHABLE, t_1_7="holds no kernel: the tangent-linear quad-layout kernels exist for NT = 2 .. 6 (jq_inst_list.h JQ_INST_T, JQ_SIZES_QUAD_TL)")


def splits(cell):
    """cells whose backward sweep goes to the split latency kernels once its first chunk exceeds their ring: default options on the
    cooperative-quad plan (cq-split, cq-wlr-three, the implicit-midpoint cooperative-quad cells)"""
    if cell.source != "structured":
        return cell.source == "small" and cell.key.split
    sc = cell.key
    return sc.expect["backward_workgroups"] == 3 or (sc.route == "imr" and sc.variant.startswith("cq"))


def runs_of(cell):
    return RUNS + (SPLIT_RUNS if splits(cell) else ())


def m_run(cell, run):
    """the Neumann order of a run (None: the cell is no Neumann cell and keeps its source's solver settings)"""
    if cell.kind != "neumann":
        return None
    if run.mslot == "own":
        return B.NEUMANN_TERMS if cell.source == "band" else cell.key.prob.m if cell.source == "structured" else SMALL_M
    return run.mslot if isinstance(run.mslot, int) else m_of(cell.index, run)


def objects_of(cell):
    """the objects of csrc/Makefile the cell's kernels come from"""
    if cell.source == "band":
        return {cell.key[0].tag}
    if cell.source == "structured":
        return {cell.key.expect["object"], cell.key.expect["forward_object"]}
    return {cell.key.tag}


def expected_record(cell, run, ensemble=False):
    """the last_kernels record of a structured cell after a run (ensemble: after the run's ensemble), None for the other sources"""
    if cell.source != "structured":
        return None
    sc = cell.key
    e = dict(sc.expect)
    if sc.kind == "neumann" and e["forward_object"][0] == "u":
        e["modd"] = m_run(cell, run) % 2 == 1
    if splits(cell):
        taken = first_backward_chunk(run) > RING
        if sc.kind == "imr":      # three workgroups take the place of the two sets of waves (jq_host_plan.h imr_cq3 / imr_cq2)
            e["backward_workgroups"], e["imr_two_sets"] = (3, False) if taken else (1, sc.expect["imr_two_sets"])
        else:
            e["backward_workgroups"] = (dict(e, **sc.expect_ens)["backward_workgroups"] if ensemble else 3) if taken else 1
    return e


def expected_decision(cell, run):
    """the start of jq_plan_info "latency_split" "last_decision" after a run of a split cell"""
    return "taken: three workgroups per column quad" if first_backward_chunk(run) > RING else "not taken: the first chunk of the sweep is not longer than the hand-off ring"


def expected_timing(cell, run):
    """(kernel_family, kernel_size, kernel_band[, kernel_variant]) of jq_last_timing"""
    if cell.source == "small":
        return cell.key.timing[:3] + ((3,) if cell.key.split and first_backward_chunk(run) > RING else cell.key.timing[3:])
    if cell.source == "structured":
        return M.family_of(cell.key) + (cell.key.NT,)      # (family, band, size): as structured_matrix.run_cell compares them
    bc = cell.key[0]
    return ({"k": 0, "j": 0, "c": 1, "i": 5}[bc.tag[0]], bc.NT, bc.code)


def options(cell, run):
    o = dict(B.options(cell.key[0], 0) if cell.source == "band" else cell.key.opts)
    if run.chunk:
        o["chunk_steps"] = run.chunk
    if run.bwd:
        assert run.bwd == 1
        o["trace_bytes"] = 1      # (a trace record of one byte holds no step: the backward sweep falls to its smallest chunk, one step)
    return o


# ---- problems ----------------------------------------------------------------------------------------------------------------------------
_small_problems, _lock = {}, threading.Lock()


def small_problem(jq, s):
    """(params, pcof) of a small cell, built once (objFuncType 3, so that the backward sweep runs twice)"""
    from test_gpu_dense_wmat import set_forbidden
    from test_gpu_random import random_problem
    with _lock:
        if s.name not in _small_problems:
            rng = np.random.default_rng(SMALL_SEEDS.get(s.name, zlib.crc32(s.name.encode())))
            p, pcof = random_problem(jq, rng, s.Ntot, s.N, s.gen[0], s.gen[1], SMALL_NSTEPS, SMALL_M, 3, s.gen[2])
            if s.forb:
                set_forbidden(p, rng, s.forb, complex_states=s.cplx)
            _small_problems[s.name] = (p, pcof)
        return _small_problems[s.name]


def source_problem(jq, cell):
    """(params, pcof) of the source cell: shared with its matrix, never modified"""
    if cell.source == "band":
        bc, Ntot = cell.key
        pr = B.problem(jq, bc.NT, bc.code, Ntot)
        return pr.p, pr.pcof
    if cell.source == "structured":
        return M.base_problem(jq, cell.key.prob)
    return small_problem(jq, cell.key)


def problem_key(cell):
    """cells with equal keys share their source problem (and, at equal solver settings, their references)"""
    if cell.source == "band":
        return ("band", cell.key[0].code, cell.key[1])
    if cell.source == "structured":
        return ("structured",) + tuple(cell.key.prob)
    return ("small", cell.key.name)


# At the source's control amplitudes the Neumann terms beyond the fourth are below what a comparison at rtol 1e-10 can see on most
# problems (the oracle's gradient moves by 1e-12 .. 1e-8 relative from order 5 to 6): a kernel that dropped the last term would pass.
# The Neumann cells of these problems scale their coefficient vector by the first factor of 1, 2, 4, 8, 16 at which every order a run
# of theirs uses moves the oracle's gradient by >= 1e-7 relative against the order below (tests/test_time_loop_matrix.py recomputes
# the choice on the oracle and checks that the reference stays well conditioned there).  Keys: amplitude_key; factor 1 where not listed.
_AMPLITUDE = {
    2: "b0_61 b1_93 b2_109 b2_125 b2_157 b1_173 b2_173 b2_189 b1_205 b2_205 b2_221 b1_237 b2_237 b15_253 s46242 s49454 s62442 s65444 s62438 "
       "s62242 s65454 s62452 s62412 s78442 s81444 s78438 s78242 s78443 s78453 s1078442 s1078453 s94442 s97444 s97454 s94443 s1094442 s1094453 "
       "s110442 s110242 s113454 s110443 s126438 s129440 s126242 s1126449 s142434 s145436 s142234 s145440 rowlane-three-Ntot3 "
       "lane-Ntot5 rowlane-three-Ntot13 rowlane-three-Ntot16 rowlane-two-Ntot5 rowlane-one-Ntot5 rowlane-one-Ntot13 slab-neumann-Ntot13 "
       "weighted-quad-NT1 weighted-quad-NT3 weighted-quad-NT5 weighted-quad-NT8 weighted-slab-Ntot12 weighted-slab-Ntot96",
    4: "b0_29 s30238 s46442 s49444 s46438 s46443 s46453 s1046453 s62443 s62453 s1062453 s94242 s113444 s110438 s110453 s1110442 s129454 "
       "s126443 s126453 lane-Ntot2 lane-Ntot3 rowlane-three-Ntot2 rowlane-two-Ntot9 rowlane-wlr-Ntot5 "
       "weighted-quad-NT4 weighted-quad-NT6 weighted-quad-NT7",
    8: "s1062442 s1110453 s126442"}
AMPLITUDE = {k: f for f, keys in _AMPLITUDE.items() for k in keys.split()}
FACTORS = (1, 2, 4, 8, 16)


def amplitude_key(cell):
    """the source problem of a cell in AMPLITUDE: b<band code>_<Ntot>, s<seed of the structured problem>, the small cell's name"""
    if cell.source == "band":
        return "b%d_%d" % (cell.key[0].code, cell.key[1])
    if cell.source == "structured":
        return "s%d" % M.seed_of(cell.key.prob)
    return cell.key.name


def amplitude(cell):
    return AMPLITUDE.get(amplitude_key(cell), 1) if cell.kind == "neumann" else 1


def run_problem(jq, cell, run, m=None, scale=None):
    """(params, pcof) of a run: a copy of the source's parameters with the source's step size, the run's step count and Neumann order
    (m: another order than the run's), the coefficients times the problem's amplitude factor (scale: another factor)"""
    p0, pcof = source_problem(jq, cell)
    p = B.with_solver(jq, p0, cell.kind)
    p.nsteps, p.T = run.nsteps, (p0.T / p0.nsteps) * run.nsteps
    if cell.kind == "neumann":
        p.linear_solver = jq.lsolver_object(max_iter=m_run(cell, run) if m is None else m)
    return p, pcof * (amplitude(cell) if scale is None else scale)


def ensemble(jq, cell, ns):
    """(nodes, weights, shift) of the source cell's ensemble"""
    if cell.source == "band":
        pr = B.problem(jq, cell.key[0].NT, cell.key[0].code, cell.key[1])
        return pr.nodes, pr.weights, pr.shift
    if cell.source == "structured":
        e = M.ensemble(jq, cell.key.prob, ns)
        return e.nodes, e.weights, e.shift
    rng = np.random.default_rng([zlib.crc32(cell.key.name.encode()), ns])
    shift = 0.05 * rng.standard_normal(cell.key.Ntot)
    shift[0] = 0.0
    return 0.1 * rng.standard_normal(ns), rng.random(ns), shift


def samples(cell, compute_units=M.MI355X_CUS):
    if cell.source == "band":
        return B.NQUAD
    if cell.source == "structured":
        return cell.key.ens or M.two_wg_samples(compute_units, cell.key.prob.N)
    return SMALL_ENS


def sparse_oracle(cell):
    """(storage only: the oracle multiplies over the nonzero pattern in both forms)"""
    return cell.source == "structured" or (cell.source == "band" and B.generator_band(cell.key[0].NT, cell.key[0].code) < cell.key[0].NT - 1)


# ---- the CPU oracle's side: one reference per (problem, solver, step count, Neumann order), shared by the cells and runs that need it ------------
def reference_key(cell, run, ns):
    return problem_key(cell) + (cell.kind, run.nsteps, m_run(cell, run), ns if run.name == ENSEMBLE_RUN else 0)


def _reference(jq, name, run, ns):
    from oracle.oracle import Oracle
    cell = BY_NAME[name]
    p, pcof = run_problem(jq, cell, run)
    if run.name == ENSEMBLE_RUN:
        return B.oracle_reference(jq, B.Problem(p, pcof, *ensemble(jq, cell, ns)), cell.kind, sparse_oracle(cell))
    orc = Oracle(p, use_sparse=sparse_oracle(cell))
    return {"single": orc.traceobjgrad_imr(pcof, 60, 1e-11, history=True) if cell.kind == "imr" else orc.traceobjgrad(pcof, history=True)}


_pool, _by_key = None, {}


def reference(jq, cell, run, ns):
    global _pool
    if _pool is None:
        def jobs():
            out = []
            for c in CELLS:
                for r in runs_of(c):
                    key = reference_key(c, r, samples(c))
                    _by_key.setdefault(key, (c.name, r, samples(c)))
                    out.append((key, _reference, (jq,) + _by_key[key]))
            return out
        _pool = B.ReferencePool(jobs, missing=lambda key: (_reference, jq) + _by_key[key])
    key = reference_key(cell, run, ns)
    _by_key.setdefault(key, (cell.name, run, ns))
    return _pool.result(key)


# ---- the GPU's side ----------------------------------------------------------------------------------------------------------------------
def run_one(jq, cell, run):
    """One run on the GPU, on a handle of its own: the gradient evaluation, the forward-only objective, the per-step history and, on
    the ensemble run, the source cell's ensemble.  Nothing is asserted here: what the library reports comes back next to the numbers.
    -> {"eval": (objfv, infidelity, leak, totalgrad, infidelgrad, leakgrad), "forward": (objfv, infidelity, leak), "history",
        "timing", "launches", "plan", "ensemble", "ns", "ens_plan", "ens_timing"}"""
    p, pcof = run_problem(jq, cell, run)
    WA = jq.Working_Arrays_M_HIP if cell.kind == "imr" else jq.Working_Arrays_HIP
    wa = WA(p, pcof.size, options=options(cell, run))
    try:
        return evaluate(jq, cell, run, p, pcof, wa)
    finally:
        wa.close()


def run_all(jq, cell):
    """every run of a cell -> [(run, out of run_one)].  Runs of equal step count (the two 2-step runs) share a handle: the chunking is
    changed through jq_set_option, the Neumann order through params.linear_solver; every other run has a handle of its own"""
    groups = []
    for run in runs_of(cell):      # (consecutive runs only: the 9-step runs A4 and A7 of a split cell keep their own handles)
        if groups and groups[-1][-1].nsteps == run.nsteps:
            groups[-1].append(run)
        else:
            groups.append([run])
    WA = jq.Working_Arrays_M_HIP if cell.kind == "imr" else jq.Working_Arrays_HIP
    outs = []
    for runs in groups:
        p, pcof = run_problem(jq, cell, runs[0])
        wa = WA(p, pcof.size, options=options(cell, runs[0]))
        try:
            for i, run in enumerate(runs):
                if i:
                    assert options(cell, run) == dict(options(cell, runs[0]), chunk_steps=run.chunk), (cell.name, run.name)
                    wa.set_option("chunk_steps", run.chunk)
                    if cell.kind == "neumann":
                        p.linear_solver = jq.lsolver_object(max_iter=m_run(cell, run))
                outs.append((run, evaluate(jq, cell, run, p, pcof, wa)))
        finally:
            wa.close()
    return outs


def evaluate(jq, cell, run, p, pcof, wa):
    """the evaluations of run_one on a live handle"""
    out = {}
    objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, p, wa, False, True)
    out["eval"] = (objfv, prim, sec, tg.copy(), ig.copy(), lg.copy())
    t = out["timing"] = wa.last_timing()
    out["launches"] = (t["n_forward_launches"], t["n_backward_launches"])
    out["plan"], out["objFuncType"] = wa.plan_info(), p.objFuncType
    if cell.source == "band":
        out["ran_on"] = B.ran_on(wa)
    out["forward"] = tuple(jq.traceobjgrad(pcof, p, wa, False, False))
    t = wa.last_timing()
    out["forward_launches"] = (t["n_forward_launches"], t["n_backward_launches"])
    out["history"] = jq.traceobjgrad(pcof, p, wa, True, False)[1]
    if run.name == ENSEMBLE_RUN:
        ns = out["ns"] = samples(cell, out["plan"]["compute_units"])
        nodes, weights, shift = ensemble(jq, cell, ns)
        jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
        out["ensemble"] = (p.last_infidelity, p.last_leak, p.last_infidelity_grad.copy(), p.last_leak_grad.copy())
        out["ens_plan"], out["ens_timing"] = wa.plan_info(), wa.last_timing()
    return out


def check_object(cell, run, out):
    """the run ran on the object, the instantiation and the chunking the table names"""
    t, plan = out["timing"], out["plan"]
    want = expected_timing(cell, run)
    if cell.source == "band":
        tag, objects = out["ran_on"]
        assert tag == cell.key[0].tag and (t["kernel_family"], t["kernel_size"], t["kernel_band"]) == want, (cell.name, run.name, tag, t)
        assert objects is None or tag in objects, objects
    elif cell.source == "small":
        got = (t["kernel_family"], t["kernel_size"], t["kernel_band"], t["kernel_variant"])
        assert got == want and plan["full_weight_rank"] == cell.key.forb, (cell.name, run.name, got, want, plan["full_weight_rank"])
        if cell.kind != "imr":      # the solver tells x_* from w_* and j_1_0 from k_1_0
            assert plan["integrator"] != "implicit_midpoint" and (plan["linear_solver"] == "jacobi") == (cell.kind == "jacobi"), (cell.name, plan["linear_solver"])
        listed = set(plan["build"]["objects"]) if plan["build"]["manifest"] else None
        if cell.key.tag[0] in "wx" and got[0] == 6:      # the quad-layout objects with the low-rank terms: named by the record and listed
            assert plan["last_kernels"]["object"] == cell.key.tag, (cell.name, run.name, plan["last_kernels"])
            assert listed is None or cell.key.tag in listed, sorted(listed)
        elif cell.key.tag[0] in "wx":
            # the slab objects w_<NT>_<BW> / x_<NT>_<BW>: the plan lists the slab plan's k_ / j_ pair only (jq_host_info.h), so the object is
            # pinned by family 0 at the tag's <NT, BW>, a full-weight rank > 0 (select_slab_kernels: wlr = wrank > 0) and the solver
            assert got[:3] == (0,) + tuple(int(v) for v in cell.key.tag.split("_")[1:]) and plan["full_weight_rank"] > 0
            assert listed is None or "kj"["wx".index(cell.key.tag[0])] + cell.key.tag[1:] in listed, sorted(listed)
        elif cell.key in SMALL:
            assert listed is None or cell.key.tag in listed, sorted(listed)
    else:
        sc = cell.key
        for ens, pl, tm in ((False, plan, t),) + (((True, out["ens_plan"], out["ens_timing"]),) if "ens_plan" in out else ()):
            rec = expected_record(cell, run, ens)
            assert pl["last_kernels"] == rec, (cell.name, run.name, ens, pl["last_kernels"], rec, pl["latency_split"])
            assert (tm["kernel_family"], tm["kernel_band"], tm["kernel_size"]) == want and pl["tile_rows"] == sc.NT, (cell.name, run.name, tm)
            assert pl["structure"] == ("od" if sc.route == "od" else "t4") and pl["full_weight_rank"] == sc.prob.forb
            assert pl["s_uniform"] == (sc.route != "od" and M.plan_uniform(sc.prob))
            if pl["build"]["manifest"]:
                assert {rec["object"], rec["forward_object"]} <= set(pl["build"]["objects"]), sorted(pl["build"]["objects"])
        if splits(cell):
            assert plan["latency_split"]["last_decision"].startswith(expected_decision(cell, run)), (cell.name, run.name, plan["latency_split"])
    # One forward launch per chunk; one backward launch per chunk, sweep (two where objFuncType != 1) and control group.  An evaluation
    # with a gradient has ONE chunk length for both sweeps (jq_host_plan.h: p->cs = adjoint ? backward_chunk_steps(...) : h->chunk_steps), so
    # where the trace budget shortens the backward chunks the forward sweep of THAT evaluation is launched in the same chunks; the
    # forward-only evaluation of the same handle keeps the forward chunking
    nfwd = len(chunks(run))
    nchunks = (run.nsteps + run.bwd - 1) // run.bwd if run.bwd else nfwd
    want = (nchunks, nchunks * (2 if out["objFuncType"] != 1 else 1) * plan["control_groups"])
    assert out["launches"] == want and out["forward_launches"] == (nfwd, 0), (cell.name, run.name, out["launches"], want, out["forward_launches"])
    assert plan["chunk_steps"] == (run.chunk or plan["chunk_steps"]) >= 1, (cell.name, run.name, plan["chunk_steps"])


# ---- sweeps on one representative per kernel template ----------------------------------------------------------------------------------------
# two more problems of test_gpu_random.random_problem for templates the cells above do not reach: the run-time-size kernels (Ntot > 256:
# one workgroup of 16 waves per slab) and the dense policy of the cooperative-quad kernels (17 .. 32 levels without the structure)
SWEEP_EXTRA = (Small("huge-Ntot257", "c_run_time", 257, 2, "neumann", {}, (1, 17, 15, 0), 0),
               Small("dense-cq-Ntot29", "u_dense", 29, 3, "neumann", {}, (8, 2, 10, 0), 0, True),
               # ... implicit midpoint: more than 16 columns (the parts kernels) and the dense policy of the cooperative-quad kernels (N = 4)
               Small("imr-parts-Ntot20", "i_parts", 20, 18, "imr", {}, (5, 2, 1, 0), 0),
               Small("imr-dense-cq-Ntot29", "v_dense", 29, 4, "imr", {}, (9, 2, 10, 0), 0, True))
SWEEP_EXTRA_CELLS = tuple(Cell("sweep-" + x.name, "small", x, "sweep", x.kind, i if x.kind == "neumann" else None) for i, x in enumerate(SWEEP_EXTRA))
# Stormer-Verlet with the Neumann solver: all three sweeps
SV_REPRESENTATIVES = ("band-k_3_1-slab-neumann-Ntot45", "band-k_6_5-slab-neumann-Ntot93", "small-weighted-slab-Ntot96", "t4-t4-neumann-NT3", "t4-od-slab-neumann-NT3",
                      "band-c_3_1-coop-neumann-Ntot45", "t4-od-coop-neumann-NT3", "band-c_7_15-coop-neumann-Ntot109", "sweep-huge-Ntot257",
                      "t4-quad3-ord+sc-NT3", "t4-quad3-generic-NT3", "t4-quad1-generic-NT3", "t4-qsplit4-ord-NT3", "t4-qsplit2-ride-NT3",
                      "t4-cq1-ord-m3-NT3", "t4-cq-split-three-NT3", "t4-cq-wlr-one-NT3", "sweep-dense-cq-Ntot29", "small-lane-Ntot5",
                      "small-rowlane-three-Ntot5", "small-rowlane-three-Ntot9", "small-rowlane-two-Ntot9", "small-rowlane-one-Ntot9")
# Jacobi and implicit midpoint: the step sweep and the backward-only chunking
ITERATIVE_REPRESENTATIVES = ("band-j_3_1-slab-jacobi-Ntot45", "band-c_7_15-coop-jacobi-Ntot109", "band-i_3_1-coop-imr-Ntot45",
                             "band-i_6_5-coop-imr-Ntot93", "t4-imr-quad-n4-NT3", "t4-imr-cq-NT3", "t4-imr-cq-one-set-NT3",
                             "small-rowlane-imr-two-Ntot9", "small-rowlane-imr-one-Ntot9", "small-coop-imr-Ntot13", "sweep-imr-parts-Ntot20",
                             "sweep-imr-dense-cq-Ntot29")
# the kernel templates of csrc/jq_inst_list.h -> representatives that run them (the tangent-linear templates: the cells of TL_CELLS)
TEMPLATES = {
    "k_forward": ("band-k_3_1-slab-neumann-Ntot45", "band-k_6_5-slab-neumann-Ntot93", "small-weighted-slab-Ntot96", "t4-t4-neumann-NT3", "t4-od-slab-neumann-NT3", "t4-quad3-ord+sc-NT3",
                  "t4-quad3-generic-NT3", "t4-quad1-generic-NT3", "t4-qsplit4-ord-NT3", "band-j_3_1-slab-jacobi-Ntot45"),
    "k_backward": ("band-k_3_1-slab-neumann-Ntot45", "band-k_6_5-slab-neumann-Ntot93", "small-weighted-slab-Ntot96", "t4-t4-neumann-NT3", "t4-od-slab-neumann-NT3", "t4-quad3-ord+sc-NT3",
                   "t4-quad3-generic-NT3", "t4-quad1-generic-NT3", "band-j_3_1-slab-jacobi-Ntot45"),
    "k_forward_coop": ("band-c_3_1-coop-neumann-Ntot45", "t4-od-coop-neumann-NT3", "band-c_7_15-coop-neumann-Ntot109", "band-c_7_15-coop-jacobi-Ntot109"),
    "k_backward_coop": ("band-c_3_1-coop-neumann-Ntot45", "t4-od-coop-neumann-NT3", "band-c_7_15-coop-neumann-Ntot109", "band-c_7_15-coop-jacobi-Ntot109"),
    "k_forward_cq": ("t4-cq1-ord-m3-NT3", "t4-cq-wlr-one-NT3", "t4-qsplit2-ride-NT3", "t4-cq-split-three-NT3", "sweep-dense-cq-Ntot29"),
    "k_backward_cq": ("t4-cq1-ord-m3-NT3", "t4-cq-wlr-one-NT3", "sweep-dense-cq-Ntot29"),
    "k_backward_cq3": ("t4-cq-split-three-NT3", "sweep-dense-cq-Ntot29"),
    "k_backward_qsplit": ("t4-qsplit4-ord-NT3", "t4-qsplit2-ride-NT3"),
    "k_forward_lane": ("small-lane-Ntot5",), "k_backward_lane": ("small-lane-Ntot5",),
    "k_forward_rowlane": ("small-rowlane-three-Ntot5", "small-rowlane-three-Ntot9", "small-rowlane-two-Ntot9", "small-rowlane-one-Ntot9"),
    "k_backward_rowlane": ("small-rowlane-one-Ntot9",), "k_backward_rowlane2": ("small-rowlane-two-Ntot9",),
    "k_backward_rowlane3": ("small-rowlane-three-Ntot5", "small-rowlane-three-Ntot9"),
    "k_forward_rowlane_imr": ("small-rowlane-imr-two-Ntot9", "small-rowlane-imr-one-Ntot9"),
    "k_backward_rowlane_imr": ("small-rowlane-imr-one-Ntot9",), "k_backward_rowlane_imr2": ("small-rowlane-imr-two-Ntot9",),
    "k_forward_coop_imr": ("band-i_3_1-coop-imr-Ntot45", "band-i_6_5-coop-imr-Ntot93", "small-coop-imr-Ntot13"),
    "k_backward_coop_imr": ("band-i_3_1-coop-imr-Ntot45", "band-i_6_5-coop-imr-Ntot93", "small-coop-imr-Ntot13"),
    "k_forward_coop_imr_parts": ("sweep-imr-parts-Ntot20",), "k_backward_coop_imr_parts": ("sweep-imr-parts-Ntot20",),
    "k_forward_cq_imr": ("t4-imr-cq-NT3", "t4-imr-cq-one-set-NT3", "sweep-imr-dense-cq-Ntot29"),
    "k_backward_cq_imr": ("t4-imr-cq-one-set-NT3",), "k_backward_cq_imr2": ("t4-imr-cq-NT3",),
    "k_backward_cq_imr3": ("t4-imr-cq-NT3", "sweep-imr-dense-cq-Ntot29"),      # (from the tenth step of the step sweep on)
    "k_forward_quad_imr": ("t4-imr-quad-n4-NT3",), "k_backward_quad_imr": ("t4-imr-quad-n4-NT3",),
}      # (the tangent-linear templates: TL_CELLS below)
BY_NAME.update({c.name: c for c in SWEEP_EXTRA_CELLS})
SWEEP_CELLS = tuple(BY_NAME[n] for n in SV_REPRESENTATIVES + ITERATIVE_REPRESENTATIVES)
STEP_SWEEP = tuple(range(1, 13)) + (16, 17)      # every ring (5 time points, 7, 8 steps, AHEAD + 2 slots) at depth - 1, depth, depth + 1 and a second wrap
SPLIT_STEP_SWEEP = (9, 10, 11, 12, 16, 17, 24, 25)      # the split latency kernels exist above their 8-step ring only
NEUMANN_SWEEP = tuple(range(13))      # RlTerms<2 .. 10> and the run-time loop on both sides, both MODD parities, the odd / pair structure of the Horner chains
BACKWARD_ONLY = Run("B9", 9, 0, "own", 1)      # one forward chunk of 9 steps, nine backward chunks of one


def always_split(cell):
    """cells whose source runs the split latency kernels by definition (their record names three workgroups)"""
    return cell.source == "structured" and cell.key.expect["backward_workgroups"] == 3


def step_runs(cell):
    return tuple(Run("S%d" % n, n, 0, "own") for n in (SPLIT_STEP_SWEEP if always_split(cell) else STEP_SWEEP))


def neumann_runs(cell):
    return tuple(Run("N%d" % m, 5, 2, m) for m in NEUMANN_SWEEP)


# the Neumann sweep's amplitude factors: the first of FACTORS at which EVERY term up to the twelfth moves the oracle's gradient by >= 1e-7
# relative at 5 steps (tests/test_time_loop_matrix.py recomputes the choice; at factor 1 the terms beyond the seventh are invisible)
SWEEP_AMPLITUDE = dict({name: 4 for name in SV_REPRESENTATIVES}, **{"t4-cq-split-three-NT3": 8, "band-c_7_15-coop-neumann-Ntot109": 16,
                                                                  "t4-cq-wlr-one-NT3": 16, "small-lane-Ntot5": 8, "small-rowlane-two-Ntot9": 16})


def sweep_reference(jq, cell, run, scale=None):
    """the oracle's single evaluation of a sweep's run (computed where it is asked for: the sweeps' problems are few and short)"""
    from oracle.oracle import Oracle
    p, pcof = run_problem(jq, cell, run, scale=scale)
    orc = Oracle(p, use_sparse=sparse_oracle(cell))
    return {"single": orc.traceobjgrad_imr(pcof, 60, 1e-11, history=True) if cell.kind == "imr" else orc.traceobjgrad(pcof, history=True)}


def run_neumann_sweep(jq, cell):
    """the Neumann sweep on ONE handle (5 steps in chunks of 2 + 2 + 1), the order changed through params.linear_solver -> [(run, out)]"""
    runs = neumann_runs(cell)
    p, pcof = run_problem(jq, cell, runs[0], scale=SWEEP_AMPLITUDE[cell.name])
    wa = jq.Working_Arrays_HIP(p, pcof.size, options=options(cell, runs[0]))
    outs = []
    try:
        for run in runs:
            p.linear_solver = jq.lsolver_object(max_iter=run.mslot)
            outs.append((run, evaluate(jq, cell, run, p, pcof, wa)))
    finally:
        wa.close()
    return outs


def sweep_references(jq, cell, runs, scale=None):
    """[sweep_reference] of the runs, on a few threads (the 257-level problem takes a second per evaluation of 7 steps)"""
    import concurrent.futures
    from oracle import oracle
    oracle.lib()      # (loaded before the threads start)
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(lambda r: sweep_reference(jq, cell, r, scale), runs))


# ---- the tangent-linear sweeps: jq_traceobj_jvp, jq_traceobjgrad_hvp, jq_eval_f_g_grad_hvp, jq_eval_f_g_grad_drifts_hvp ---------------------
# The tangents are carried over chunk boundaries next to the primal carries; their own tests run one chunk and chunk_steps=3 (the drift
# ensemble: 5).  Here the runs A1 and A4 .. A6 with the matrix's rotation of the Neumann order, on the cases, references and criteria of
# tests/test_gpu_jvp.py, test_gpu_hvp.py, test_gpu_ens_hvp.py, test_gpu_ens_hvp_rowlane.py, test_gpu_ens_hvp_quad.py, test_gpu_drift_hvp.py.
TL_RUNS = (RUNS[0], RUNS[3], RUNS[4], RUNS[5])
TL_NDIR = 2
# api: "jvp" / "hvp" / "ens" / "drift"; route: what the plan record names ("coop": the dense-tile kernels k_forward_tl / k_backward_tl);
# case: the Case / QCase / Shape of the source test; expect: (kernel_family, kernel_size, kernel_band or None, object or None)
TLCell = collections.namedtuple("TLCell", "name api route case index expect objects")


def _tl_cells():
    import drift_hvp_cases as DC
    import test_gpu_ens_hvp as E
    import test_gpu_ens_hvp_quad as Q
    import test_gpu_ens_hvp_rowlane as R
    import test_gpu_hvp as H
    from block_band_problem import tile_rows
    out = []

    def add(api, route, case, ident, expect, objects):
        index = sum(1 for c in out if (c.api, c.route) == (api, route))
        out.append(TLCell("tl-%s-%s-%s" % (api, route, ident), api, route, case, index, expect, objects))

    # Ntot 17 (a second tile row with one live row): two, one and five controls (five: two control groups), objFuncType 3 / 2 / 1
    for c in (H.Case(17, 3, 2, 4, 0, 5, 3), H.Case(17, 3, 1, 1, 3, 1, 2), H.Case(17, 3, 5, 0, 0, 5, 1)):
        for api in ("jvp", "hvp"):
            add(api, "coop", c, "Ntot17-Nc%d" % c.Nc, (1, tile_rows(c.Ntot), 15, None), ("k_forward_tl", "k_backward_tl")[:1 if api == "jvp" else 2])
    for c in (E.LANE_CASES[0], E.LANE_CASES[2], E.LANE_CASES[7]):      # NP 2, 4, 6
        NP = 2 * ((c.Ntot + 1) // 2)
        add("ens", "lane", c, "Ntot%d" % c.Ntot, (2, NP, 0, "l_%d" % NP), ("k_forward_lane_tl", "k_backward_lane_tl"))
    for c in (R.ROWLANE_CASES[1], R.ROWLANE_CASES[2], R.ROWLANE_CASES[7]):      # NPJ 12, 12, 16
        add("ens", "rowlane", c, "Ntot%d" % c.Ntot, (3, R._npj(c.Ntot), 0, "r_%d" % R._npj(c.Ntot)), ("k_forward_rowlane_tl", "k_backward_rowlane_tl"))
    quads = (Q.QUAD_CASES[1], Q.QUAD_CASES[2], Q.QCase(4, 61, 4, 3, 1, 0, 1, 3, 3, "given", "varied", Q.NSTEPS),
             Q.QCase(5, 77, 3, 2, 4, 0, 1, 2, 3, "given", "varied", Q.NSTEPS), Q.QUAD_CASES[5])      # NT 2 .. 6
    for c in quads:
        add("ens", "quad", c, "NT%d" % c.n, (6, c.n, 7, "t_%d_7" % c.n), ("k_forward_quad_tl", "k_backward_quad_tl"))
    for route in ("lane", "rowlane", "quad"):      # the first shape of every route, objFuncType 2
        s = next(x for x in DC.SHAPES if x.route == route)
        add("drift", route, s, DC.shape_id(s), (DC.KERNEL_FAMILY[route], DC.kernel_size(s), None, DC.kernel_object(s)),
            {"lane": ("k_forward_lane_tl", "k_backward_lane_tl"), "rowlane": ("k_forward_rowlane_tl", "k_backward_rowlane_tl"),
             "quad": ("k_forward_quad_tl", "k_backward_quad_tl")}[route])
    return tuple(out)


TL_CELLS = _tl_cells()
TL_BY_NAME = {c.name: c for c in TL_CELLS}
assert len(TL_BY_NAME) == len(TL_CELLS)
DRIFT_OBJ_TYPE = 2
# amplitude factors of the tangent-linear cells, chosen like AMPLITUDE (the first factor at which every order a run uses moves the oracle's
# gradient by >= 1e-7 relative; tests/test_time_loop_matrix.py recomputes the choice); factor 1 where not listed
TL_AMPLITUDE = {"tl-jvp-coop-Ntot17-Nc1": 2, "tl-ens-quad-NT4": 2}
for _c in TL_CELLS:
    for _t in _c.objects:
        TEMPLATES[_t] = TEMPLATES.get(_t, ()) + (_c.name,)
_tl_sources = {}


def tl_m(cell, run):
    return m_of(cell.index, run)


def tl_source(jq, cell):
    """the source test's problem of a cell, built once and never modified: dict p, pcof, D [ncoeff, <= 2] and, by api, nodes / weights /
    shift (ens) or H, weights (drift)"""
    import test_gpu_hvp as H
    with _lock:
        if cell.name in _tl_sources:
            return _tl_sources[cell.name]
    from oracle.oracle import Oracle
    c = cell.case
    if cell.api in ("jvp", "hvp"):
        import test_gpu_jvp as J
        p, pcof, rng = (J if cell.api == "jvp" else H)._problem(jq, c)
        src = dict(p=p, pcof=pcof, D=H._directions(rng, Oracle(p).traceobjgrad(pcof)["totalgrad"], pcof.size, 5)[:, :TL_NDIR])
    elif cell.api == "ens":
        import test_gpu_ens_hvp as E
        import test_gpu_ens_hvp_quad as Q
        import test_gpu_ens_hvp_rowlane as R
        p, pcof, rng, nodes, weights, shift = {"lane": E, "rowlane": R, "quad": Q}[cell.route]._problem(jq, c)
        D = H._directions(rng, E._total_gradient(p, pcof, nodes, weights, shift), pcof.size, c.ndir)[:, :TL_NDIR]
        src = dict(p=p, pcof=pcof, D=D, nodes=nodes, weights=weights, shift=shift)
    else:
        import drift_hvp_cases as DC
        p, pcof, Hm, D = DC.problem(jq, c, DRIFT_OBJ_TYPE)
        src = dict(p=p, pcof=pcof, D=D, H=Hm, weights=DC.WEIGHTS)
    with _lock:
        return _tl_sources.setdefault(cell.name, src)


def tl_problem(jq, cell, run, m=None, scale=None):
    """(params, pcof) of a run: the source's step size, the run's step count and Neumann order, the coefficients times the cell's factor"""
    import copy
    src = tl_source(jq, cell)
    p = copy.copy(src["p"])
    p.nsteps, p.T = run.nsteps, (src["p"].T / src["p"].nsteps) * run.nsteps
    p.linear_solver = jq.lsolver_object(max_iter=tl_m(cell, run) if m is None else m)
    return p, src["pcof"] * (TL_AMPLITUDE.get(cell.name, 1) if scale is None else scale)


def tl_reference(jq, cell, run):
    """the CPU reference of a run, by the source test's own reference: a list per direction (drift: (refs, weighted oracle sums))"""
    src = tl_source(jq, cell)
    p, pcof = tl_problem(jq, cell, run)
    D = src["D"]
    if cell.api == "jvp":
        import tangent_reference as TR
        ref = TR.TangentReference(p)
        return [ref.tangent(pcof, D[:, j]) for j in range(D.shape[1])]
    if cell.api == "hvp":
        import hessian_reference as HR
        from oracle.oracle import Oracle
        ref = HR.HessianReference(p)
        return [ref.hvp(pcof, D[:, j]) for j in range(D.shape[1])], Oracle(p).traceobjgrad(pcof)["totalgrad"]
    if cell.api == "ens":
        import test_gpu_ens_hvp as E
        return E._reference(p, pcof, D, src["nodes"], src["weights"], src["shift"])
    import drift_hessian_reference as DR
    W = src["weights"]
    ref = DR.DriftHessianReference(p, src["H"], W)
    refs = []
    for j in range(D.shape[1]):      # (as drift_hvp_cases.case)
        mem = ref.member_hvps(pcof, D[:, j])
        hv, hvi = sum(w * r["hv"] for w, r in zip(W, mem)), sum(w * r["hv_infid"] for w, r in zip(W, mem))
        refs.append(dict(hv=hv, hv_infid=hvi, hv_leak=hv - hvi) if p.objFuncType != 1 else dict(hv=hv, hv_infid=hv, hv_leak=np.zeros(pcof.size)))
    return refs, DR.weighted_oracle(p, pcof, src["H"], W)


def tl_references(jq, cell):
    import concurrent.futures
    from oracle import oracle
    oracle.lib()
    tl_source(jq, cell)
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(TL_RUNS)) as pool:
        return list(pool.map(lambda r: tl_reference(jq, cell, r), TL_RUNS))


PLAN_KEY = {"jvp": "jvp", "hvp": "hvp", "ens": "ens_hvp", "drift": "drift_hvp"}


def tl_run(jq, cell, run):
    """One run on the GPU on a handle of its own -> {"r": the call's result, "plan", "timing", "p", "pcof", and the primal checks' inputs}"""
    src = tl_source(jq, cell)
    p, pcof = tl_problem(jq, cell, run)
    D = src["D"]
    wa = jq.Working_Arrays_HIP(p, pcof.size, options={"chunk_steps": run.chunk} if run.chunk else None)
    try:
        if cell.api == "jvp":
            r = jq.traceobj_jvp(pcof, D, p, wa)
        elif cell.api == "hvp":
            r = jq.traceobjgrad_hvp(pcof, D, p, wa)
        elif cell.api == "ens":
            r = jq.eval_f_g_grad_hvp(pcof, D, p, wa, src["nodes"], src["weights"], src["shift"])
        else:
            r = jq.eval_f_g_grad_drifts_hvp(pcof, D, p, wa, src["H"], src["weights"])
        out = dict(r=r, plan=wa.plan_info(), timing=wa.last_timing(), p=p, pcof=pcof, wa=wa)
        return out
    except Exception:
        wa.close()
        raise


def tl_check_records(cell, run, out):
    """the plan record reports the route, the directions (members) of one launch and the chunk length of the run; one forward launch per
    chunk, one backward launch per chunk, pass and control group (the tangent alone: none); family, size, band and object of the cell"""
    plan, t, p = out["plan"], out["timing"], out["p"]
    ndir = tl_source_ndir(cell)
    cs = run.chunk or run.nsteps
    want = {"directions_per_launch": ndir, "chunk_steps": cs, "rounds": 1}
    if cell.api in ("ens", "drift"):
        want["route"] = cell.route
    if cell.api == "drift":
        want["members_per_launch"] = 3
    assert plan[PLAN_KEY[cell.api]] == want, (cell.name, run.name, plan[PLAN_KEY[cell.api]], want)
    family, size, band, obj = cell.expect
    assert (t["kernel_family"], t["kernel_size"]) == (family, size) and (band is None or t["kernel_band"] == band), (cell.name, run.name, t)
    if obj is not None:
        assert plan["last_kernels"]["object"] == obj and plan["last_kernels"]["forward_object"] == obj, (cell.name, plan["last_kernels"])
    nchunks = len(chunks(run))
    npass = 0 if cell.api == "jvp" else (2 if p.objFuncType != 1 else 1) * (plan["control_groups"] if cell.api == "hvp" else 1)
    assert (t["n_forward_launches"], t["n_backward_launches"]) == (nchunks, nchunks * npass), (cell.name, run.name, t["n_forward_launches"], t["n_backward_launches"], nchunks, npass)


def tl_source_ndir(cell):
    return _tl_sources[cell.name]["D"].shape[1]
