"""The block-band matrix (tests/test_block_band_matrix.py, tests/test_gpu_block_band.py): one cell per (tile rows NT, band code, route)
with the kernel object it must run on, the problems of a cell (tests/block_band_problem.py: operators that fill their tiles), the CPU
oracle's results for them (computed once per problem and solver, shared by the cells) and the run of a cell on the GPU.

As a program -- python tests/block_band_matrix.py OUT.json -- it runs every NT <= 6 cell through the library named by JQ_LIB and
writes every number in exact form: the register-form fence of tests/test_gpu_block_band.py compares two such dumps bit for bit."""
import atexit
import collections
import concurrent.futures
import copy
import os
import sys
import threading

import numpy as np

from block_band_problem import block_band_problem

ROUTES = ("slab-neumann", "slab-jacobi", "coop-neumann", "coop-jacobi", "coop-imr")
# band codes of the instantiations (csrc/Makefile INST / COOP; the last one of a row is "dense" = NT - 1) ...
SMALL_BANDS = {2: (0, 1), 3: (0, 1, 2), 4: (0, 1, 2, 3), 5: (0, 1, 2, 4), 6: (0, 1, 2, 5)}
# ... and of the Ntot > 96 cooperative kernels (BIG; 15 = dense for every NT), which are the only family at that size
BIG_NT = tuple(range(7, 17))
BIG_BANDS = (1, 2, 15)
BIG_ROUTES = ROUTES[2:]
# (NT, band code, route) that the plan refuses with JQ_EUNSUPPORTED instead of running it: none
REFUSED = frozenset()

Cell = collections.namedtuple("Cell", "NT code route tag")      # tag None: refused


def _tag(NT, code, route):
    if (NT, code, route) in REFUSED:
        return None
    # The Jacobi solver with Diagonal weights has cooperative kernels only above 96 levels (jq_host_plan.h plan_batch): with the default
    # options a Jacobi handle of NT <= 6 runs on the slab kernels' Jacobi object as well
    prefix = {"slab-neumann": "k", "slab-jacobi": "j", "coop-neumann": "c", "coop-jacobi": "j" if NT <= 6 else "c", "coop-imr": "i"}[route]
    return "%s_%d_%d" % (prefix, NT, code)


CELLS = tuple(Cell(NT, code, route, _tag(NT, code, route)) for NT, codes in SMALL_BANDS.items() for code in codes for route in ROUTES) + \
        tuple(Cell(NT, code, route, _tag(NT, code, route)) for NT in BIG_NT for code in BIG_BANDS for route in BIG_ROUTES)

N, NSTEPS, NEUMANN_TERMS, OBJ_FUNC_TYPE, NQUAD = 3, 7, 3, 3, 7
CHUNKS = (0, 3)      # chunk_steps 3: chunks of 3 + 3 + 1 steps


def sizes(NT):
    """Hilbert dimensions of a cell: a ragged last tile row and column, and full tiles where NT is 4, 6 or 16"""
    return (16 * NT - 3,) + ((16 * NT,) if NT in (4, 6, 16) else ())


def generator_band(NT, code):
    return NT - 1 if code == 15 else code


def modes(NT, code):
    """trace layouts of the controls: full band, block diagonal, band without the diagonal blocks; one control where the band is 0"""
    return [1, 0, 2] if generator_band(NT, code) >= 1 else [1]


def cell_id(cell, Ntot):
    return "%s-%s-Ntot%d" % (cell.tag or "refused_%d_%d" % (cell.NT, cell.code), cell.route, Ntot)


CASES = tuple((cell, Ntot) for cell in CELLS for Ntot in sizes(cell.NT))

Problem = collections.namedtuple("Problem", "p pcof nodes weights shift")
_problems, _problems_lock = {}, threading.Lock()


def problem(jq, NT, code, Ntot):
    """the problem of (NT, code, Ntot) and its ensemble (random nodes, weights and shift), built once"""
    with _problems_lock:
        if (code, Ntot) not in _problems:
            rng = np.random.default_rng(16000 + 100 * Ntot + code)
            p, pcof = block_band_problem(jq, rng, Ntot, N, generator_band(NT, code), modes(NT, code), NSTEPS, NEUMANN_TERMS, OBJ_FUNC_TYPE)
            shift = 0.05 * rng.standard_normal(Ntot)
            shift[0] = 0.0
            _problems[code, Ntot] = Problem(p, pcof, 0.1 * rng.standard_normal(NQUAD), rng.random(NQUAD), shift)
        return _problems[code, Ntot]


def with_solver(jq, p, kind):
    """a copy of the parameters with the solver settings of a route"""
    p = copy.copy(p)
    if kind == "jacobi":
        p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER, max_iter=80, tol=1e-12, nrhs=N)
    elif kind == "imr":
        p.Integrator_id = jq.Implicit_Midpoint
        p.linear_solver = jq.lsolver_object(solver=jq.JACOBI_SOLVER_M, max_iter=60, tol=1e-11, nrhs=N)
        p.wmat = p.wmat_real.copy()
    return p


def kind_of(route):
    return route.split("-")[1]


# ---- the CPU oracle's side: one reference per (problem, solver), shared by the cells that need it ------------------------------------------
def oracle_reference(jq, prob, kind, sparse):
    """{"single", "ensemble"} of a Problem under the solver settings of `kind` (shared with tests/structured_matrix.py)"""
    from oracle.oracle import Oracle
    p = with_solver(jq, prob.p, kind)
    orc = Oracle(p, use_sparse=sparse)
    if kind != "imr":
        return {"single": orc.traceobjgrad(prob.pcof, history=True),
                "ensemble": orc.eval_f_g_grad(prob.pcof, prob.nodes, prob.weights, prob.shift)}
    # implicit midpoint: the weighted sum of the samples' evaluations, as tests/test_gpu_imr.py _random_checks
    inf, g, H0 = 0.0, np.zeros(prob.pcof.size), p.Hconst
    for ep, wq in zip(prob.nodes, prob.weights):
        p.Hconst = H0 + np.diag(ep * prob.shift)
        rr = Oracle(p, use_sparse=sparse).traceobjgrad_imr(prob.pcof, 60, 1e-11)
        inf += wq * rr["primaryobjf"]
        g += wq * rr["infidelgrad"]
    return {"single": orc.traceobjgrad_imr(prob.pcof, 60, 1e-11, history=True), "ensemble": {"last_infidelity": inf, "last_infidelity_grad": g}}


def _reference(jq, NT, code, Ntot, kind):
    # (sparse is storage only: the oracle multiplies over the nonzero pattern in both forms)
    return oracle_reference(jq, problem(jq, NT, code, Ntot), kind, generator_band(NT, code) < NT - 1)


class ReferencePool:
    """The first request starts every reference of a matrix on a few threads (the oracle is C behind ctypes and holds no global
    state; the largest problems take seconds each); every cell then waits for its own only.  jobs(): (key, function, arguments) in the
    order the cells run; a key asked for that jobs() did not name is computed on the spot by missing(key)."""
    def __init__(self, jobs, missing=None):
        self.jobs, self.missing, self.pool, self.futures = jobs, missing, None, {}

    def result(self, key):
        if self.pool is None:
            from oracle import oracle
            oracle.lib()      # (loaded before the threads start)
            pool = self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(12, (os.cpu_count() or 2) - 1)))
            atexit.register(lambda: pool.shutdown(wait=False, cancel_futures=True))
            for k, fn, args in self.jobs():
                if k not in self.futures:
                    self.futures[k] = pool.submit(fn, *args)
        if key not in self.futures:
            self.futures[key] = self.pool.submit(*self.missing(key))
        return self.futures[key].result()


_pool = None


def reference(jq, cell, Ntot):
    global _pool
    if _pool is None:
        _pool = ReferencePool(lambda: [((c.code, nt, kind_of(c.route)), _reference, (jq, c.NT, c.code, nt, kind_of(c.route)))
                                       for c, nt in CASES if c.tag is not None])
    return _pool.result((cell.code, Ntot, kind_of(cell.route)))


# ---- the GPU's side ----------------------------------------------------------------------------------------------------------------------
def options(cell, chunk):
    opts = {"coop_max": 0, "lane": 0, "dq": 0, "quad": 0} if cell.route.startswith("slab") else ({"dq": 0} if cell.NT == 2 else {})
    if chunk:
        opts["chunk_steps"] = chunk
    return opts


def ran_on(wa):
    """the object tag of the last evaluation, from jq_last_timing and jq_plan_info (and the objects the manifest lists, or None)"""
    t, plan = wa.last_timing(), wa.plan_info()
    imr, jacobi = plan["integrator"] == "implicit_midpoint", plan["linear_solver"] == "jacobi"
    prefix = {(0, False): "j" if jacobi else "k", (1, False): "c", (5, True): "i"}.get((t["kernel_family"], imr), "family%d" % t["kernel_family"])
    assert t["kernel_size"] == plan["tile_rows"] and t["kernel_band"] == plan["block_band"], (t, plan)
    assert plan["full_weight_rank"] == 0      # (family 0 with full weights would be the w_ / x_ objects)
    return "%s_%d_%d" % (prefix, t["kernel_size"], t["kernel_band"]), (sorted(plan["build"]["objects"]) if plan["build"]["manifest"] else None)


def run_cell(jq, cell, Ntot, chunks=CHUNKS):
    """A cell on the GPU: one gradient evaluation per chunking, then the per-step history and the ensemble on the last handle.
    -> {"tag", "objects", "evals": [(objfv, infidelity, leak, totalgrad, infidelgrad, leakgrad) per chunking], "history", "ensemble"}"""
    prob = problem(jq, cell.NT, cell.code, Ntot)
    kind = kind_of(cell.route)
    p = with_solver(jq, prob.p, kind)
    WA = jq.Working_Arrays_M_HIP if kind == "imr" else jq.Working_Arrays_HIP
    out = {"evals": []}
    for chunk in chunks:
        wa = WA(p, prob.pcof.size, options=options(cell, chunk))
        try:
            objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(prob.pcof, p, wa, False, True)
            out["evals"].append((objfv, prim, sec, tg.copy(), ig.copy(), lg.copy()))
            tag, objects = ran_on(wa)
            assert out.setdefault("tag", tag) == tag, (out["tag"], tag)
            out["objects"] = objects
            if chunk == chunks[-1]:
                out["history"] = jq.traceobjgrad(prob.pcof, p, wa, True, False)[1]
                jq.eval_f_g_grad(prob.pcof, p, wa, prob.nodes, prob.weights, True, shift=prob.shift)
                assert ran_on(wa)[0] == tag
                out["ensemble"] = (p.last_infidelity, p.last_leak, p.last_infidelity_grad.copy(), p.last_leak_grad.copy())
        finally:
            wa.close()
    return out


def exact(out):
    """every number of run_cell's result in exact (hexadecimal) form"""
    def hx(v):
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(v)))
        return [float(x).hex() for x in (a.view(np.float64) if np.iscomplexobj(a) else a.astype(np.float64)).ravel()]
    return {"tag": out["tag"], "evals": [[hx(v) for v in e] for e in out["evals"]], "history": hx(out["history"]),
            "ensemble": [hx(v) for v in out["ensemble"]]}


def dump_main(runs):
    """python tests/<matrix>.py OUT.json: runs() -> (id, result of run_cell) through the library named by JQ_LIB, every number in exact form"""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import juqbox_jl_amd
    dump = {k: exact(out) for k, out in runs(juqbox_jl_amd)}
    with open(sys.argv[1], "w") as f:
        json.dump(dump, f)


if __name__ == "__main__":
    dump_main(lambda jq: ((cell_id(c, nt), run_cell(jq, c, nt)) for c, nt in CASES if c.NT <= 6 and c.tag is not None))
