"""Uncoupled controls (Hunc_ops, the lab-frame evaluation of a pulse: KS! src/evalobjgrad.jl:2373-2387) on every kernel family
(tests/test_uncoupled_matrix.py, tests/test_gpu_uncoupled.py): the generator and the table of cells.

to_uncoupled turns a coupled problem of the existing generators (test_gpu_random.random_problem, block_band_problem,
subsystem_problem, random_kronecker_problem) into an uncoupled one: Hunc_ops[q] is the problem's Hsym_ops[q] (kind "s") or Hanti_ops[q]
(kind "a"), Rfreq is random with several radians over T, everything else is kept.  jq_create then fills ONE slot of control pair q and
leaves the other image zero, k_ctrl feeds both slots with ft = 2 (p cos(2 pi Rfreq t) - q sin(2 pi Rfreq t)), and k_gradacc folds the
traces of both slots (B = P + Q) before it applies the rotation again -- on every family the zero image's traces must be EXACT zeros.

The cells reuse the option sets and the expected records of the two existing matrices (tests/block_band_matrix.py ROUTES,
tests/structured_matrix.py CELLS) instead of restating them, and add the routes those matrices do not have (lane, row-lane, the dense
cooperative-quad policy, run-time sizes, N > 16, control groups, the row-lane implicit-midpoint kernels).  The kind patterns rotate over
the cells of a family (all symmetric: S(t) = 0; all antisymmetric: K = Hconst; mixed), objFuncType over 1 / 2 / 3."""
import collections
import copy
import threading
import zlib

import numpy as np

import block_band_matrix as B
import structured_matrix as M

NSTEPS, NQUAD_BAND = B.NSTEPS, B.NQUAD
CHUNKS = (0, 3)      # chunk_steps 3: chunks of 3 + 3 + 1 steps
# the split cooperative-quad sweep (11 steps) is taken only when the first chunk exceeds its 8-slot ring (jq_host_plan.h): chunks of 3
# would run the one-workgroup kernel, so those cells run one chunk and chunks of 9 + 2 -- the second one shorter than the ring
SPLIT_CHUNKS = (0, 9)
HISTORY_ATOL = 1e-11      # per-step histories
MIN_SHARE = 0.01          # every control's block of a gradient, of that gradient's norm, on the oracle
FD_NEUMANN_TERMS = 24     # finite-difference checks: at order 3 the adjoint differs from the objective's derivative by the truncation
IMR_REFUSAL = "uncoupled controls (Hunc_ops): gradients with the Stormer-Verlet integrator only"      # jq_host_plan.h plan_batch
# cell names that the plan refuses with JQ_EUNSUPPORTED -> the library's message: none
REFUSED = {}


def to_uncoupled(jq, p, kinds, rng, Rfreq=None):
    """the uncoupled twin of the coupled problem p: Hunc_ops[q] = Hsym_ops[q] (kinds[q] == "s") or Hanti_ops[q] ("a"); Rfreq[q] random
    with 0.2 <= |Rfreq[q]| <= 2 (T >= 1: at least 1.2 rad, up to 25) unless given.  Levels, T, steps, Uinit / Utarget, Cfreq, drift,
    weights (Diagonal or full), objFuncType, solver and integrator are kept."""
    assert p.Nunc == 0 and len(kinds) == p.Ncoupled and set(kinds) <= {"s", "a"}, kinds
    ops = [(p.Hsym_ops if k == "s" else p.Hanti_ops)[q] for q, k in enumerate(kinds)]
    if Rfreq is None:
        Rfreq = rng.choice([-1.0, 1.0], len(kinds)) * (0.2 + 1.8 * rng.random(len(kinds)))
    u = jq.objparams(p.Ne, p.Ng, p.T, p.nsteps, Uinit=p.Uinit, Utarget=p.Utarget_r + 1j * p.Utarget_i, Cfreq=p.Cfreq, Rfreq=np.asarray(Rfreq, dtype=np.float64),
                     Hconst=p.Hconst, Hunc_ops=ops, objFuncType=p.objFuncType, linear_solver=copy.copy(p.linear_solver), Integrator=p.Integrator_id,
                     use_sparse=p.use_sparse, leak_ubound=p.leak_ubound)
    # (an operator that is ZERO -- a random "t4" control on a part its size does not have -- counts as symmetric whatever it was taken from)
    assert all(sym == (k == "s") or not h.any() for sym, k, h in zip(u.isSymm, kinds, u.Hunc_ops)), (u.isSymm, kinds)
    for name in ("wmat", "wmat_real", "wmat_imag", "forb_states", "forb_weights"):
        setattr(u, name, copy.copy(getattr(p, name)))
    return u


def coupled_twin_without_rotation(jq, u):
    """Rfreq = 0 and symmetric operators: ft = 2 p, so the uncoupled problem IS the coupled problem Hsym = 2 Hunc, Hanti = 0"""
    assert all(u.isSymm)
    z = [np.zeros_like(h) for h in u.Hunc_ops]
    c = jq.objparams(u.Ne, u.Ng, u.T, u.nsteps, Uinit=u.Uinit, Utarget=u.Utarget_r + 1j * u.Utarget_i, Cfreq=u.Cfreq, Rfreq=np.zeros(u.Nunc),
                     Hconst=u.Hconst, Hsym_ops=[2.0 * h for h in u.Hunc_ops], Hanti_ops=z, objFuncType=u.objFuncType,
                     linear_solver=copy.copy(u.linear_solver))
    c.wmat_real = copy.copy(u.wmat_real)
    return c


def hanti_images(u):
    """the antisymmetric slots jq_create fills (zeros where Hunc_ops[q] is symmetric)"""
    return [np.zeros_like(h) if sym else h for h, sym in zip(u.Hunc_ops, u.isSymm)]


# ---- the cells ---------------------------------------------------------------------------------------------------------------------------
# source: "structured" (key: a structured_matrix cell name), "band" (key: (NT, code, route, Ntot) of block_band_matrix), "random" (key:
# the arguments of test_gpu_random.random_problem behind rng and before objFuncType: Ntot N Nc Nfreq nsteps m banded), "kron" (dims, N)
# timing: (kernel_family, kernel_size, kernel_band, kernel_variant) of jq_last_timing after a single evaluation, ens_timing after the ensemble
# record / ens_record: jq_plan_info "last_kernels" where the source matrix has one (else None)
# alts: (options, kernel_variant) of runs that the option text promises to be bit-identical to the cell's own
Cell = collections.namedtuple("Cell", "name source key kinds oft kind opts chunks ens timing ens_timing record ens_record alts seed")
PATTERNS = ("s", "a", "sa", "as")      # all symmetric, all antisymmetric, mixed starting with either


def pattern(i, Nc):
    """kind pattern i of Nc controls; one control has no mixed pattern"""
    base = PATTERNS[i % (4 if Nc > 1 else 2)]
    return (base * Nc)[:Nc]


def classify(kinds):
    return "s" if set(kinds) == {"s"} else "a" if set(kinds) == {"a"} else "mixed"


def plan_uniform(scell, kinds):
    """plan info s_uniform of a 4 x 4 x n plan for the CONVERTED operators: jq_create tests the antisymmetric slots, and an all-symmetric
    set leaves every one of them zero -- S(t) = 0 is uniform whatever the size; a symmetric control takes its operator out of the test"""
    pr = scell.prob
    return pr.n == 1 or "a" not in kinds or (pr.flavour == "uniform" and pr.Ntot % 16 == 0)


def variant_of(record):
    """kernel_variant of jq_last_timing for a last_kernels record (jq_host_plan.h): workgroups per column quad of the split latency
    kernels, 20 + quads per workgroup of the split quad sweep, else 0"""
    return record["backward_workgroups"] if record["backward_workgroups"] in (2, 3) else 20 + record["quads_per_workgroup"] if record["quads_per_workgroup"] else 0


SLAB_OPTS = {"coop_max": 0, "lane": 0, "dq": 0, "quad": 0}
STRUCTURED_EXTRA = ("cq1-ord-m3-NT3", "quad3-ord-NT3", "imr-quad-n2-NT3", "imr-cq-NT3")      # an interior 16-row block; a third cell for families 7 / 9


def _cells():
    out, turn, count = [], collections.Counter(), [0]

    def add(name, source, key, Nc, kind, opts, timing, chunks=CHUNKS, ens=7, ens_timing=None, record=None, ens_record=None, alts=(), kinds=None):
        family = timing[0]
        if kinds is None:      # the patterns rotate over the cells of a family
            kinds = pattern(turn[family], Nc)
            turn[family] += 1
        oft = count[0] % 3 + 1
        count[0] += 1
        if kind == "imr":      # forward only: one chunking, no gradient
            chunks = (0,)
        seed = SEEDS.get(name, zlib.crc32(name.encode()))
        out.append(Cell(name, source, key, kinds, oft, kind, dict(opts), chunks, ens, tuple(timing), tuple(ens_timing or timing), record, ens_record, tuple(alts), seed))

    # ---- lane kernels (family 2): Ntot <= 8, forced by rowlane_max=0; NP = 6, 8
    for Ntot, kinds in ((5, "ss"), (5, "sa"), (8, "aa"), (8, "as")):
        add("lane-Ntot%d-%s" % (Ntot, kinds), "random", (Ntot, 2, 2, 2, NSTEPS, 3, False), 2, "neumann", {"rowlane_max": 0}, (2, 6 if Ntot == 5 else 8, 0, 0),
            ens=33, kinds=kinds)      # 66 columns: two waves of 64 lanes, the second nearly empty
    # ---- row-lane kernels (family 3): NPJ = 12, 16; rl_split 0 / 2 / 3: one / two / three waves, the same bits (jq_options.h)
    for Ntot, NPJ in ((10, 12), (13, 16)):
        add("rowlane-Ntot%d" % Ntot, "random", (Ntot, 3, 2, 2, NSTEPS, 3, False), 2, "neumann", {}, (3, NPJ, 0, 33),
            alts=(({"rl_split": 0}, 0), ({"rl_split": 2}, 32), ({"rl_split": 3}, 33)))
    add("rowlane-5ctrl", "random", (10, 3, 5, 2, NSTEPS, 3, False), 5, "neumann", {}, (3, 12, 0, 33), kinds="sasas")
    # ---- ... and their implicit-midpoint kernels (family 4): the two chains on two waves
    for i in range(3):
        add("rowlane-imr-Ntot10-%d" % i, "random", (10, 3, 2, 2, NSTEPS, 0, False), 2, "imr", {}, (4, 12, 0, 32))
    # ---- slab / cooperative band kernels: the ROUTES of block_band_matrix at NT = 2 (band codes 0, 1) and the HBM-operand cooperative
    #      kernels at NT = 7, band 15 (Ntot 109 = 16 * 7 - 3)
    for bc in B.CELLS:
        if (bc.NT == 2 or (bc.NT, bc.code) == (7, 15)) and bc.tag is not None:
            Ntot = 16 * bc.NT - 3
            family = {"k": 0, "j": 0, "c": 1, "i": 5}[bc.tag[0]]
            add("band-%s" % B.cell_id(bc, Ntot), "band", (bc.NT, bc.code, bc.route, Ntot), len(B.modes(bc.NT, bc.code)), B.kind_of(bc.route),
                B.options(bc, 0), (family, bc.NT, bc.code, 0), ens=NQUAD_BAND)
    # ---- the dense policy of the cooperative-quad kernels (family 8, band 10): 17 .. 32 levels without the structure, default options
    for i in range(3):
        add("dense-cq-Ntot29-%d" % i, "random", (29, 3, 2, 2, NSTEPS, 3, False), 2, "neumann", {}, (8, 2, 10, 0))
    # ---- 4 x 4 x n: every structured_matrix cell with NT = 2, and an interior block for cq1 / quad3 ORD
    for sc in M.CELLS:
        if (sc.NT == 2 or sc.name in STRUCTURED_EXTRA) and sc.name not in M.REFUSED:
            family, band = M.family_of(sc)
            out_kinds = pattern(turn[family], sc.prob.Nc)
            rec, ens_rec = dict(sc.expect), dict(sc.expect, **sc.expect_ens)
            if sc.route == "quad3":      # SC follows the converted operators: an all-symmetric set turns it on
                sc_on = plan_uniform(sc, out_kinds) and sc.opts.get("s_compact", 1) == 1
                for r in (rec, ens_rec):
                    r["sc_forward"], r["sc_backward"] = sc_on, sc_on and r["ord"]
            chunks = sc.chunks
            if chunks == (0,) and sc.kind != "imr":      # the source matrix runs the split sweep in one chunk only
                assert sc.prob.nsteps == M.SPLIT_STEPS and rec["backward_workgroups"] == 3
                chunks = SPLIT_CHUNKS
            add("t4-" + sc.name, "structured", sc.name, sc.prob.Nc, sc.kind, sc.opts, (family, sc.NT, band, variant_of(rec)), chunks=chunks, ens=sc.ens,
                ens_timing=(family, sc.NT, band, variant_of(ens_rec)), record=rec, ens_record=ens_rec)
    # ---- a Kronecker problem whose control 0 fills all three parts (no ORD): 4 x 4 x 2 on the cooperative-quad kernels
    add("kron-4x4x2", "kron", ((4, 4, 2), 4), 3, "neumann", {"cq3": 0}, (8, 2, 7, 0), ens=13)
    # ---- run-time sizes (Ntot > 256): one workgroup of 16 waves per slab, dense windows
    add("huge-Ntot257", "random", (257, 2, 2, 1, NSTEPS, 3, False), 2, "neumann", {}, (1, 17, 15, 0), ens=3, kinds="sa")
    # ---- more than 16 columns per evaluation (two 16-column parts), slab and cooperative
    add("n17-slab", "random", (20, 17, 2, 2, NSTEPS, 3, False), 2, "neumann", SLAB_OPTS, (0, 2, 1, 0), ens=2)
    add("n17-coop", "random", (20, 17, 2, 2, NSTEPS, 3, False), 2, "neumann", {"dq": 0}, (1, 2, 1, 0), ens=2)
    # ---- five controls: two control groups (JQ_MAXNC = 4), k_gradacc with q0 > 0
    add("slab-5ctrl", "random", (29, 3, 5, 2, NSTEPS, 3, False), 5, "neumann", SLAB_OPTS, (0, 2, 1, 0), kinds="sasas")
    add("quad-5ctrl", "random", (29, 4, 5, 2, NSTEPS, 3, "t4"), 5, "neumann", {"quad8": 2}, (6, 2, 7, 0), ens=13, kinds="sasas")
    return tuple(out)


# seeds of cells whose default (the CRC of the name) gives a control a share of a gradient below MIN_SHARE (tests/test_uncoupled_matrix.py)
SEEDS = {"t4-quad3-s_compact0-NT2": 3, "t4-quad2-generic-NT2": 3, "t4-imr-cq-one-set-NT2": 3}      # (share 0.003 with the default)
CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
assert len(BY_NAME) == len(CELLS)
SV_CELLS = tuple(c for c in CELLS if c.kind != "imr")
IMR_CELLS = tuple(c for c in CELLS if c.kind == "imr")

# ---- problems ----------------------------------------------------------------------------------------------------------------------------
Problem = collections.namedtuple("Problem", "p pcof nodes weights shift coupled")
_problems, _lock = {}, threading.Lock()
MI355X_CUS = 256


def samples(cell, compute_units=MI355X_CUS):
    if cell.ens:
        return cell.ens
    return M.two_wg_samples(compute_units, M.BY_NAME[cell.key].prob.N)


def _coupled(jq, cell, rng):
    """(params, pcof) of the coupled source problem (never modified: the matrices it comes from share it)"""
    if cell.source == "structured":
        return M.base_problem(jq, M.BY_NAME[cell.key].prob)
    if cell.source == "band":
        NT, code, route, Ntot = cell.key
        pr = B.problem(jq, NT, code, Ntot)
        return pr.p, pr.pcof
    if cell.source == "kron":
        from kronecker_problem import random_kronecker_problem
        p, pcof, _ = random_kronecker_problem(jq, *cell.key)
        p.nsteps = NSTEPS
        return p, pcof
    from test_gpu_random import random_problem
    Ntot, N, Nc, Nfreq, nsteps, m, banded = cell.key
    return random_problem(jq, rng, Ntot, N, Nc, Nfreq, nsteps, m, cell.oft, banded)


def problem(jq, cell, ns=None):
    """the cell's uncoupled problem (solver settings of a Neumann cell: B.with_solver adds the others) and its ensemble of ns samples"""
    ns = samples(cell) if ns is None else ns
    with _lock:
        if (cell.name, ns) not in _problems:
            rng = np.random.default_rng(cell.seed)
            p0, pcof = _coupled(jq, cell, rng)
            u = to_uncoupled(jq, p0, cell.kinds, rng)
            u.objFuncType = cell.oft
            erng = np.random.default_rng([cell.seed, ns])
            shift = 0.05 * erng.standard_normal(u.Ntot)
            shift[0] = 0.0
            _problems[cell.name, ns] = Problem(u, pcof, 0.1 * erng.standard_normal(ns), erng.random(ns), shift, p0)
        return _problems[cell.name, ns]


def sparse_oracle(cell):
    """(storage only: the oracle multiplies over the nonzero pattern in both forms)"""
    return cell.source in ("structured", "kron") or (cell.source == "band" and B.generator_band(cell.key[0], cell.key[1]) < cell.key[0] - 1)


# ---- the CPU oracle's side: one reference per (problem, solver, ensemble), shared -----------------------------------------------------------
def _reference(jq, name, ns):
    from oracle.oracle import Oracle
    cell = BY_NAME[name]
    prob = problem(jq, cell, ns)
    if cell.kind != "imr":
        return B.oracle_reference(jq, prob, cell.kind, sparse_oracle(cell))
    p = B.with_solver(jq, prob.p, "imr")      # forward only: the implicit-midpoint adjoint has no term for uncoupled controls
    return {"single": Oracle(p, use_sparse=sparse_oracle(cell)).traceobjgrad_imr(prob.pcof, 60, 1e-11, evaladjoint=False, history=True)}


_pool = None


def reference(jq, cell, ns):
    global _pool
    if _pool is None:
        _pool = B.ReferencePool(lambda: [((c.name, samples(c)), _reference, (jq, c.name, samples(c))) for c in CELLS if c.name not in REFUSED],
                                missing=lambda key: (_reference, jq) + key)
    return _pool.result((cell.name, ns))


# ---- the GPU's side ----------------------------------------------------------------------------------------------------------------------
def _verify(wa, cell, timing, record):
    plan, t = wa.plan_info(), wa.last_timing()
    got = (t["kernel_family"], t["kernel_size"], t["kernel_band"], t["kernel_variant"])
    assert got == timing, (cell.name, got, timing, plan["last_kernels"])
    if cell.source == "band":
        assert B.ran_on(wa)[0] == "%s_%d_%d" % ({(0, "neumann"): "k", (0, "jacobi"): "j", (1, "neumann"): "c", (1, "jacobi"): "c", (5, "imr"): "i"}[timing[0], cell.kind],
                                                 timing[1], timing[2])
    if record is not None:
        sc = M.BY_NAME[cell.key]
        assert plan["last_kernels"] == record, (cell.name, plan["last_kernels"], record, plan["latency_split"])
        assert plan["structure"] == ("od" if sc.route == "od" else "t4") and plan["full_weight_rank"] == sc.prob.forb and plan["tile_rows"] == sc.NT
        assert plan["s_uniform"] == (sc.route != "od" and plan_uniform(sc, cell.kinds)), (cell.name, plan["s_uniform"])
        if plan["build"]["manifest"]:
            assert {record["object"], record["forward_object"]} <= set(plan["build"]["objects"]), sorted(plan["build"]["objects"])
    return plan["last_kernels"]


def run_cell(jq, cell, opts=None, check=True):
    """A Stormer-Verlet cell on the GPU with its options (opts: a bit-identical alternative's): one gradient evaluation per chunking, then
    the per-step history and the ragged ensemble on the last handle; after every evaluation with a gradient the timing record, and where
    the source matrix has one the last_kernels record, are asserted.
    -> {"tag", "evals": [(objfv, infidelity, leak, totalgrad, infidelgrad, leakgrad) per chunking], "history", "ensemble", "ns"}"""
    assert cell.kind != "imr"
    out = {"evals": [], "tag": cell.name}
    p = pcof = None
    for chunk in cell.chunks:
        o = dict(cell.opts if opts is None else dict(cell.opts, **opts))
        if chunk:
            o["chunk_steps"] = chunk
        if p is None:
            pr0 = problem(jq, cell)
            p, pcof = B.with_solver(jq, pr0.p, cell.kind), pr0.pcof
        wa = jq.Working_Arrays_HIP(p, pcof.size, options=o)
        try:
            assert wa.plan_info()["last_kernels"] is None
            objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, p, wa, False, True)
            out["evals"].append((objfv, prim, sec, tg.copy(), ig.copy(), lg.copy() if p.objFuncType != 1 else tg - ig))
            t = wa.last_timing()
            out["timing"] = (t["kernel_family"], t["kernel_size"], t["kernel_band"], t["kernel_variant"])
            if check:
                _verify(wa, cell, cell.timing, cell.record)
            if chunk == cell.chunks[-1]:
                out["history"] = jq.traceobjgrad(pcof, p, wa, True, False)[1]
                ns = out["ns"] = samples(cell, wa.plan_info()["compute_units"])
                e = problem(jq, cell, ns)
                jq.eval_f_g_grad(pcof, p, wa, e.nodes, e.weights, True, shift=e.shift)
                if check:
                    _verify(wa, cell, cell.ens_timing, cell.ens_record)
                out["ensemble"] = (p.last_infidelity, p.last_leak, p.last_infidelity_grad.copy(),
                                   p.last_leak_grad.copy() if p.objFuncType != 1 else np.zeros(pcof.size))
        finally:
            wa.close()
    return out


def run_imr_cell(jq, cell):
    """An implicit-midpoint cell: forward evaluations are served (objective, history), the gradient is refused with the library's message
    and leaves the handle's next forward evaluation bit-identical.  -> {"objective": (objfv, infidelity, leak), "history", "refusal"}"""
    from juqbox_jl_amd import _lib
    assert cell.kind == "imr"
    pr0 = problem(jq, cell)
    p, pcof = B.with_solver(jq, pr0.p, "imr"), pr0.pcof
    wa = jq.Working_Arrays_M_HIP(p, pcof.size, options=dict(cell.opts))
    try:
        first = jq.traceobjgrad(pcof, p, wa, False, False)
        _verify(wa, cell, cell.timing, cell.record)
        try:
            jq.traceobjgrad(pcof, p, wa, False, True)
            refusal = None
        except _lib.JuqboxHipError as e:
            refusal = (e.code, str(e))
        again = jq.traceobjgrad(pcof, p, wa, False, False)
        assert [float(x).hex() for x in first] == [float(x).hex() for x in again], (first, again)
        history = jq.traceobjgrad(pcof, p, wa, True, False)[1]
    finally:
        wa.close()
    return {"objective": first, "history": history, "refusal": refusal}
