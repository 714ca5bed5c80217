"""The stopping-rule matrix (tests/test_stopping_matrix.py, tests/test_gpu_stopping.py): the Jacobi and implicit-midpoint cells of the
block-band matrix (tests/block_band_matrix.py, at Ntot = 16 NT - 3), of the structured matrix (tests/structured_matrix.py) and of the
small systems of tests/time_loop_matrix.py, and six extra cells for stopping rules that no table reaches, crossed with solver settings
at which the place where an iteration stops decides the result.

The source matrices run their iterative cells at tol = 1e-12 (Jacobi) and 1e-11 (implicit midpoint) with a cap that is never reached:
one iteration more or less moves their gradients by 1e-13 .. 4e-12 relative, below the criteria, so an off-by-one in a stopping rule,
a test on the sum of the two norms, a sample that iterates until its wave-mate converges or a wrong iterate kept at the cap all pass.
Here the tolerances are 1e-4 and 1e-6 and the cap is 0 .. 3 or the median count of the cell, where the same errors are 1e-8 .. 1e-4.

A run is (max_iter, tol).  Every cell has ONE handle, the source cell's problem (7 steps in one chunk), options and expected object /
last_kernels record; the settings change through params.linear_solver (jq_set_linear_solver / jq_set_integrator).  The CPU oracle
computes every run with its iteration record on (oracle/oracle.py Oracle.instrument): tests/test_stopping_matrix.py checks on the
record that no stopping comparison of a run is close enough to its tolerance for rounding to decide it, that samples sharing a slab
stop at different counts, and -- with the oracle's test-only bias -- that one iteration more or less in ONE solve misses the criterion
by two orders of magnitude here while the same bias in EVERY solve passes at the source cell's settings.

Out of scope (and where they are covered):
  Jacobi with the per-part rule -- N > 64, or N > 16 on the cooperative or run-time-size kernels: exception (ii) of DESIGN.md section 2,
  "the 2-norm of ITS columns' update, not the sample's": O(tol) by design, so there is no count to agree on; tests/test_gpu_round4.py.
  The forward-only implicit-midpoint cells of the uncoupled matrix (tests/test_uncoupled_matrix.py): the same kernels as the cells here,
  launched without a backward sweep; the forward-only objective of every run here covers their loop.
  The three-workgroup backward kernels of the cooperative-quad implicit-midpoint family (k_backward_cq_imr3) are taken only when the
  first backward chunk exceeds their 8-step ring: no 7-step run reaches them (tests/time_loop_matrix.py A7 .. A9 do, at tight tolerance)."""
import collections
import copy
import zlib

import numpy as np

import block_band_matrix as B
import structured_matrix as M
import time_loop_matrix as T

NSTEPS = 7
BASE = T.Run("S7", NSTEPS, 0, "own")      # the time loop of every run: the source cells' 7 steps in one chunk

# max_iter None: MIX takes the median count of the cell's L4 record, OWN the source cell's settings
Run = collections.namedtuple("Run", "name max_iter tol history ensemble")
RUNS = (Run("L4", 80, 1e-4, True, True),        # exit by tolerance, counts of 2 .. 5
        Run("L6", 80, 1e-6, False, False),      # exit by tolerance, longer counts, both register sets
        Run("C1", 1, 1e-30, False, False), Run("C2", 2, 1e-30, False, False), Run("C3", 3, 1e-30, False, False),      # the cap alone, odd and even
        Run("C0", 0, 1e-30, False, False),      # Jacobi only: jacobi_add's max_iter <= 0 branch
        Run("MIX", None, 1e-4, False, True),    # both exits inside one evaluation
        Run("OWN", None, None, False, False))   # the handle is what it was
RUN_BY_NAME = {r.name: r for r in RUNS}


def runs_of(cell):
    return tuple(r for r in RUNS if r.name != "C0" or cell.kind == "jacobi")


# ---- the cells ---------------------------------------------------------------------------------------------------------------------------
DENSE96 = {"force_dense": 1, "embed": 0}
# extras, one cell each (T.Small: name tag Ntot N kind opts timing forb split gen); the problems are test_gpu_random.random_problem's, dense
EXTRA = (
    T.SWEEP_EXTRA[0]._replace(kind="jacobi"),      # run-time-size Jacobi loop: Ntot = 257, N = 2, the problem of sweep-huge-Ntot257
    T.Small("imr-dense-cq-Ntot25", "v_dense", 25, 4, "imr", {}, (9, 2, 10, 0), 0, True),      # dense policy of the cooperative-quad kernels
    T.Small("imr-hbm-Ntot96", "i_6_5", 96, 3, "imr", DENSE96, (5, 6, 5, 0), 0),               # dense 96 x 96: images read from HBM
    T.Small("imr-parts-lds-Ntot40", "i_parts", 40, 20, "imr", {}, (5, 3, 2, 0), 0),           # _parts walkers, images in LDS
    T.Small("imr-parts-hbm-Ntot109", "i_parts", 109, 20, "imr", {}, (5, 7, 15, 0), 0),        # _parts walkers, images in HBM
    T.Small("jacobi-wgsum-Ntot40", "j_3_2", 40, 20, "jacobi", T.SLAB_OPTS, (0, 3, 2, 0), 0),   # workgroup-sum rule of the slab kernels
)
EXTRA_CELLS = tuple(T.Cell("extra-" + x.name, "small", x, "extra", x.kind, None) for x in EXTRA)
SMALL_TAGS = ("i_1_0", "j_1_0", "x_1_0", "x_6_5")


def _cells():
    out = []
    for c in T.CELLS:
        if c.kind not in ("jacobi", "imr"):
            continue
        if c.source == "band":
            bc = c.key[0]
            if bc.route in ("slab-jacobi", "coop-imr") or (bc.route == "coop-jacobi" and bc.NT >= 7):      # (NT <= 6: coop-jacobi IS slab-jacobi's object)
                out.append(c)
        elif c.source == "structured":
            out.append(c)
        elif c.key.tag.startswith("m_") or c.key.tag in SMALL_TAGS:
            out.append(c)
    return tuple(out) + EXTRA_CELLS


CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
assert len(BY_NAME) == len(CELLS)

# objects with an iterative solver that no cell here runs, and why
UNREACHABLE = {"v_1_7": M.UNREACHABLE["v_1_7"]}

def N_of(cell):
    return B.N if cell.source == "band" else cell.key.prob.N if cell.source == "structured" else cell.key.N


def Ntot_of(cell):
    return cell.key[1] if cell.source == "band" else cell.key.prob.Ntot if cell.source == "structured" else cell.key.Ntot


def _prefix(c):
    return {t[0] for t in T.objects_of(c)}


def _variant(c, *variants):
    return c.source == "structured" and c.key.route == "imr" and c.key.variant in variants


def _rowlane(c):
    return c.source == "small" and c.key.tag.startswith("m_")


# Every implementation of a stopping rule (kernel header: what) -> the cells that run it
RULES = {
    "jq_kernels.h: jacobi_add, per sample": lambda c: c.kind == "jacobi" and bool(_prefix(c) & {"j", "x"}) and N_of(c) <= 16,
    "jq_kernels.h: jacobi_add, workgroup sum": lambda c: c.name == "extra-jacobi-wgsum-Ntot40",
    "jq_coop_kernels.h: coop_horner": lambda c: c.source == "band" and c.key[0].route == "coop-jacobi",
    "jq_huge_kernels.h: run-time-size Jacobi loop": lambda c: c.name == "extra-huge-Ntot257",
    "jq_quad_imr_kernels.h: QuadImr::step4": lambda c: _variant(c, "quad-n4"),
    "jq_quad_imr_kernels.h: QuadImr::step": lambda c: _variant(c, "quad-n2"),
    "jq_coop_imr_kernels.h: forward and backward loops": lambda c: c.kind == "imr" and _prefix(c) == {"i"} and N_of(c) <= 16,
    "jq_coop_imr_kernels.h: _parts walkers": lambda c: c.name.startswith("extra-imr-parts-"),
    "jq_cq_imr_kernels.h: reducer wave, two sets of waves (imr2)": lambda c: _variant(c, "cq") and c.key.expect["imr_two_sets"],
    "jq_cq_imr_kernels.h: reducer wave, one set of waves": lambda c: _variant(c, "cq", "cq-one-set") and not c.key.expect["imr_two_sets"],
    "jq_cq_imr_kernels.h: reducer wave, dense policy": lambda c: c.name == "extra-imr-dense-cq-Ntot25",
    "jq_rowlane_imr_kernels.h: one wave": lambda c: _rowlane(c) and c.key.opts.get("rl_split", 1) == 0,
    "jq_rowlane_imr_kernels.h: two waves": lambda c: _rowlane(c) and c.key.opts.get("rl_split", 1) != 0,
}


def rule_cells(rule):
    return tuple(c for c in CELLS if RULES[rule](c))


# ---- problems, settings, ensembles -----------------------------------------------------------------------------------------------------------
def problem(jq, cell):
    """(params with the source cell's own solver settings, pcof): a copy, 7 steps at the source's step size"""
    return T.run_problem(jq, cell, BASE)


def own_solver(jq, cell):
    return problem(jq, cell)[0].linear_solver


def solver(jq, cell, run, mix_cap=None):
    """the lsolver_object of a run (Jacobi: tol times sqrt(N) like every Jacobi handle of the tables, src/linear_solvers.jl:40)"""
    if run.name == "OWN":
        return own_solver(jq, cell)
    max_iter = mix_cap if run.name == "MIX" else run.max_iter
    assert max_iter is not None
    return jq.lsolver_object(solver=jq.JACOBI_SOLVER if cell.kind == "jacobi" else jq.JACOBI_SOLVER_M, max_iter=max_iter, tol=run.tol, nrhs=N_of(cell))


def mix_cap(l4_record):
    """the cap of MIX: the median iteration count of the L4 gradient evaluation's solves"""
    return int(np.median(l4_record["count"]))


def samples(cell):
    ns = T.samples(cell)
    assert ns in (7, 13)
    return ns


# Nodes 0.3 randn and shift 0.5 randn (shift[0] = 0), as tests/test_gpu_parity.py, are the starting point: on the matrices' problems,
# whose operators are far larger than cnot2's, they move few counts, and the median count of a cell is often its largest, which no cap
# exit can share an evaluation with.  Much wider nodes take Stormer-Verlet past its stability limit (h |K| > 2): samples grow to 1e7
# and one ulp in the coefficients moves the oracle's own gradient by 1e-4.  NODE_FACTOR widens the nodes for every cell; a cell whose
# ensemble still misses a condition of tests/test_stopping_matrix.py (slab-mates that differ in a count at L4 and MIX, both exits in the
# MIX ensemble, every margin > 1e-6, no cap exit at L4, one ulp in every coefficient moves the ensemble's results by <= 1e-12 relative)
# gets (node factor, seed) here -- the first of the grid SEEDS x FACTORS that meets them all; the conditions are never relaxed.
# Keys: ensemble_key.
NODE_SCALE, SHIFT_SCALE, NODE_FACTOR = 0.3, 0.5, 3
FACTORS, SEEDS = (3, 10, 5, 2, 1, 30), (0, 1, 2)
_OVERRIDES = {
    (2, 0): "weighted-jacobi-Ntot12:jacobi",
    (5, 0): "b0_45:jacobi b1_125:jacobi b1_237:jacobi",
    (5, 2): "b2_253:jacobi",
    (10, 0): "b0_29:jacobi b1_45:imr b0_61:jacobi b0_61:imr b3_61:jacobi b1_77:jacobi b1_93:imr b15_109:imr b2_141:jacobi "
            "b2_173:jacobi b1_205:jacobi b1_205:imr b15_205:jacobi b2_237:jacobi s81444:jacobi s81444:imr s110442:imr s142242:imr "
            "rowlane-imr-two-Ntot2:imr",
    (10, 1): "b2_157:jacobi",
    (10, 2): "b2_189:jacobi",
    (30, 0): "s46442:jacobi",
    (30, 1): "rowlane-imr-two-Ntot3:imr",
}
ENSEMBLE_OVERRIDES = {k: v for v, keys in _OVERRIDES.items() for k in keys.split()}


# The discrimination check of tests/test_stopping_matrix.py biases single solves of the L4 gradient evaluation.  Node override: where a
# solve of the unperturbed problem is too well conditioned for one iteration to move any quantity by 100 x the criterion, the check runs
# at the node of this sample of the cell's ensemble (which the GPU side compares as part of that ensemble).  b2_205:jacobi: one more
# iteration in the very first solve moves the history by 3.2e-9 (32 x) at the unperturbed problem, by 1.25e-8 at sample 4.
DISCRIMINATION_NODES = {"b2_205:jacobi": 4}


def problem_key(cell):
    return T.problem_key(cell) + (cell.kind,)


def ensemble_key(cell):
    """the problem and solver kind of a cell in ENSEMBLE_OVERRIDES: time_loop_matrix.amplitude_key and the kind"""
    return "%s:%s" % (T.amplitude_key(cell), cell.kind)


def ensemble(cell, override=None):
    """(nodes, weights, shift) of the cell's L4 / MIX ensemble: by the problem, so cells of one problem share their references"""
    key, ns, Ntot = ensemble_key(cell), samples(cell), Ntot_of(cell)
    factor, seed = override or ENSEMBLE_OVERRIDES.get(key, (NODE_FACTOR, 0))
    rng = np.random.default_rng([zlib.crc32(key.encode()), seed])
    shift = SHIFT_SCALE * rng.standard_normal(Ntot)
    shift[0] = 0.0
    return factor * NODE_SCALE * rng.standard_normal(ns), rng.random(ns), shift


def one_ulp_moves(a, b, names):
    """the largest relative change of the named quantities between two oracle results (coefficients one ulp apart): the conditioning of
    the reference, as tests/test_time_loop_matrix.py measures it"""
    return max(float(np.linalg.norm(np.atleast_1d(a[k] - b[k])) / max(np.linalg.norm(np.atleast_1d(a[k])), 1e-300)) for k in names)


def slab_mates(cell):
    """pairs of samples that share a 16-column slab (a wave of the row-lane kernels, a workgroup of the others)"""
    sps = 16 // N_of(cell)
    return [(s, s + 1) for s in range(samples(cell) - 1) if sps >= 2 and s // sps == (s + 1) // sps]


# ---- the CPU oracle's side -----------------------------------------------------------------------------------------------------------------
SINGLE = ("objfv", "primaryobjf", "secondaryobjf", "totalgrad", "infidelgrad", "leakgrad")
ENSEMBLE = ("last_infidelity", "last_leak", "last_infidelity_grad", "last_leak_grad")


def oracle_single(jq, cell, ls, history=False, record=True, bias=0, solve=-1, Hconst=None, pcof=None):
    """the oracle's gradient evaluation under the settings `ls` -> (results, iteration record or None); pcof: other coefficients than the cell's"""
    from oracle.oracle import Oracle
    p0, pcof = problem(jq, cell)[0], (problem(jq, cell)[1] if pcof is None else pcof)
    p = copy.copy(p0)
    p.linear_solver = ls
    if Hconst is not None:
        p.Hconst = Hconst
    orc = Oracle(p, use_sparse=T.sparse_oracle(cell))
    if record or bias:
        orc.instrument(record=record, bias=bias, solve=solve)
    r = orc.traceobjgrad_imr(pcof, ls.max_iter, ls.tol, history=history) if cell.kind == "imr" else orc.traceobjgrad(pcof, history=history)
    return r, (orc.iteration_record() if record else None)


def oracle_ensemble(jq, cell, ls, override=None, pcof=None):
    """the weighted sum over the cell's ensemble -> ({last_*}, record with the sample of every solve)"""
    from oracle.oracle import Oracle
    nodes, weights, shift = ensemble(cell, override)
    p0, pcof = problem(jq, cell)[0], (problem(jq, cell)[1] if pcof is None else pcof)
    if cell.kind == "jacobi":
        p = copy.copy(p0)
        p.linear_solver = ls
        orc = Oracle(p, use_sparse=T.sparse_oracle(cell))
        orc.instrument(record=True)
        return orc.eval_f_g_grad(pcof, nodes, weights, shift), orc.iteration_record()
    e = {"last_infidelity": 0.0, "last_leak": 0.0, "last_infidelity_grad": np.zeros(pcof.size), "last_leak_grad": np.zeros(pcof.size)}
    recs = []
    for s, (ep, wq) in enumerate(zip(nodes, weights)):      # (as block_band_matrix.oracle_reference)
        r, rec = oracle_single(jq, cell, ls, Hconst=p0.Hconst + np.diag(ep * shift), pcof=pcof)
        e["last_infidelity"] += wq * r["primaryobjf"]
        e["last_leak"] += wq * r["secondaryobjf"]
        e["last_infidelity_grad"] += wq * r["infidelgrad"]
        e["last_leak_grad"] += wq * r["leakgrad"]
        rec["sample"][:] = s
        recs.append(rec)
    rec = {k: np.concatenate([r[k] for r in recs]) for k in ("count", "by_cap", "sample", "margin")}
    return e, rec


def _references(jq, name):
    """{run name: {"solver", "single", "record"[, "ensemble", "ens_record"]}} of a cell, every run of RUNS its kind has"""
    cell, out = BY_NAME[name], {}
    for run in runs_of(cell):
        ls = solver(jq, cell, run, mix_cap(out["L4"]["record"]) if run.name == "MIX" else None)
        r, rec = oracle_single(jq, cell, ls, history=run.history)
        out[run.name] = {"solver": (ls.max_iter, ls.tol), "single": r, "record": rec}
        if run.ensemble:
            out[run.name]["ensemble"], out[run.name]["ens_record"] = oracle_ensemble(jq, cell, ls)
    return out


_pool, _first = None, {}
for _c in CELLS:
    _first.setdefault(problem_key(_c), _c.name)


def references(jq, cell):
    """the oracle's runs of a cell; computed once per problem and solver kind on a few threads (block_band_matrix.ReferencePool)"""
    global _pool
    if _pool is None:
        _pool = B.ReferencePool(lambda: [(problem_key(c), _references, (jq, _first[problem_key(c)])) for c in CELLS])
    return _pool.result(problem_key(cell))


# ---- the GPU's side --------------------------------------------------------------------------------------------------------------------------
def evaluate(jq, cell, run, p, pcof, wa):
    """the evaluations of a run on a live handle (the keys of time_loop_matrix.evaluate, so that its check_object applies):
    the gradient evaluation, the forward-only objective, on L4 the per-step history, on L4 and MIX the ensemble.  "ran": (family, size,
    band) of jq_last_timing after EVERY evaluation."""
    out = {"ran": []}

    def ran():
        t = wa.last_timing()
        out["ran"].append((t["kernel_family"], t["kernel_size"], t["kernel_band"]))
        return t

    objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, p, wa, False, True)
    out["eval"] = (objfv, prim, sec, tg.copy(), ig.copy(), lg.copy())
    t = out["timing"] = ran()
    out["launches"] = (t["n_forward_launches"], t["n_backward_launches"])
    out["plan"], out["objFuncType"] = wa.plan_info(), p.objFuncType
    if cell.source == "band":
        out["ran_on"] = B.ran_on(wa)
    out["forward"] = tuple(jq.traceobjgrad(pcof, p, wa, False, False))
    t = ran()
    out["forward_launches"] = (t["n_forward_launches"], t["n_backward_launches"])
    if run.history:
        out["history"] = jq.traceobjgrad(pcof, p, wa, True, False)[1]
        ran()
    if run.ensemble:
        nodes, weights, shift = ensemble(cell)
        out["ns"] = len(nodes)
        jq.eval_f_g_grad(pcof, p, wa, nodes, weights, True, shift=shift)
        out["ensemble"] = (p.last_infidelity, p.last_leak, p.last_infidelity_grad.copy(), p.last_leak_grad.copy())
        out["ens_plan"], out["ens_timing"] = wa.plan_info(), ran()
    return out


def run_cell(jq, cell, refs, opts=None):
    """every run of a cell on ONE handle (opts: the options of its bit-identical partner instead of the cell's) -> [(run, out of evaluate)]"""
    p, pcof = problem(jq, cell)
    WA = jq.Working_Arrays_M_HIP if cell.kind == "imr" else jq.Working_Arrays_HIP
    wa = WA(p, pcof.size, options=T.options(cell, BASE) if opts is None else dict(opts))
    outs = []
    try:
        for run in runs_of(cell):
            p.linear_solver = solver(jq, cell, run, mix_cap(refs["L4"]["record"]) if run.name == "MIX" else None)
            assert (p.linear_solver.max_iter, p.linear_solver.tol) == refs[run.name]["solver"]
            outs.append((run, evaluate(jq, cell, run, p, pcof, wa)))
    finally:
        wa.close()
    return outs


def check_object(cell, out):
    """the run ran on the object the source table names (time_loop_matrix.check_object: last_kernels, family / size / band of
    jq_last_timing, the manifest, the launches of a single chunk) -- after every evaluation of the run"""
    T.check_object(cell, BASE, out)
    want = T.expected_timing(cell, BASE)
    want = (want[0], want[2], want[1]) if cell.source == "structured" else want[:3]      # (structured: family, band, size)
    assert all(r == want for r in out["ran"]), (cell.name, out["ran"], want)


def partner_options(cell):
    """options of the second handle that the source promises to be bit-identical (structured cells with a partner), or None"""
    return dict(cell.key.partner) if cell.source == "structured" and cell.key.partner is not None else None


def family_of(cell):
    """the kernel family a cell's errors are reported under (profiles/stopping_matrix.txt)"""
    if cell.source == "small" and cell.key in EXTRA:
        return "extra " + cell.key.name
    return "%s %s" % (cell.source, cell.route if cell.source != "structured" else cell.key.route + " " + cell.key.variant)
