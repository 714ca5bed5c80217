"""The structured matrix (tests/test_structured_matrix.py, tests/test_gpu_structured.py): one cell per (tile rows NT, route, variant) of
the kernels behind the structure codes 7, 8, 9 (JQ_BW_T4Q, JQ_BW_T4, JQ_BW_OD) -- the options that force the route, the problem
(tests/subsystem_problem.py: control q acts on subsystem q only, which is what selects the ORD / RIDE / SC specialisations) and the
record jq_plan_info "last_kernels" must show after the cell's evaluations: object, slabs / quads per workgroup, workgroups per column
quad and the compile-time flags.  Built like tests/block_band_matrix.py, whose reference pool, exact() dump and dumper it shares.

As a program -- python tests/structured_matrix.py OUT.json -- it runs every cell whose object ships in the VGPR register form through
the library named by JQ_LIB and writes every number in exact form (the register-form fence of tests/test_gpu_structured.py).

Routes and what limits them (jq_host_plan.h plan_batch, jq_host_create.h; LDS of a CU: 160 KiB):
  quad3    quad8=2: quad layout, three slabs per workgroup, k_N_7.  The window staging grows with the control count: three slabs fit
           with three controls up to NT = 6, with two at NT = 7, with ONE at NT = 8 -- so ORD (two or three controls) does not exist at
           NT = 8 and the three-control ORD / SC variants do not exist at NT = 7; those cells use the largest control count that fits.
  quad1/2  cq=0 qsplit=0 / quad8=1: one / two slabs per workgroup, s_N_7 (no specialisation; two slabs at NT = 8: two controls).
  qsplit4  cq=0: backward sweep k_backward_qsplit<.., 4>, p_N_7 behind the s_N_7 forward kernel (NT <= 6).
  qsplit2  qsplit=2 cq3=0: k_backward_qsplit<.., 2>, p_N_7 behind the u_N_7 forward kernel (NT = 2 .. 6).
  cq1      cq3=0: cooperative quad, one workgroup per column quad, u_N_7 (NT = 2 .. 7).
  cq-split default options, 11 steps in one chunk (the first chunk must exceed the 8-slot ring): three workgroups per quad; two for the
           smallest ensemble with 3 nq_pad > compute units >= 2 nq_pad.
  cq-wlr   real full weights of rank 2 (two real forbidden states): the WLR instantiations of u_N_7, one and three workgroups
           (NT = 7: two controls -- the partial dots of the weights do not fit next to three).
  t4       coop_max=0 lane=0 dq=0 quad=0: JQ_BW_T4 slab kernels, k_N_8 / j_N_8.
  od       t4=0: JQ_BW_OD slab (k_ / j_N_9), cooperative (c_N_9) and cooperative implicit-midpoint (i_N_9) kernels.
  imr      implicit midpoint on the structure: q_N_7 (N = 2; N = 4 with imr_cq=0), v_N_7 (N = 4; two sets of waves up to NT = 6).
NT = 1 (Ntot <= 16) needs lane=0 on every route, has no +- 16 couplings (two controls), no cooperative-quad kernels, and its one block
makes every S image uniform: the three-slab cells run the SC kernels unless s_compact=0."""
import collections
import threading

import numpy as np

import block_band_matrix as B
from subsystem_problem import subsystem_problem

N, NSTEPS, SPLIT_STEPS, OBJ_FUNC_TYPE, NQUAD = 4, 7, 11, 3, 13
CHUNKS = (0, 3)      # chunk_steps 3: chunks of 3 + 3 + 1 steps
FLAGS = ("uni", "ord", "sc_forward", "sc_backward", "ride", "modd", "fwd2", "wlr", "imr_two_sets")
# objects csrc/Makefile builds that no plan reaches: cq_max_quads (jq_host_create.h) needs NT >= 2 -- a single 16-row block has no
# neighbour to split the work with -- so an NT = 1 problem never runs the cooperative-quad families 8 / 9
UNREACHABLE = {"u_1_7": "cooperative-quad kernels need NT >= 2 (jq_host_create.h cq_max_quads)",
               "v_1_7": "cooperative-quad implicit-midpoint kernels need NT >= 2 (jq_host_create.h cq_max_quads)"}
# objects with structure code 7 that are not this matrix's: full leakage weights on the quad-layout / slab kernels (tests/test_gpu_dense_wmat.py)
OUT_OF_SCOPE = ("w_*_7", "w_1_0", "w_6_5", "x_*")
# cell names that the plan refuses with JQ_EUNSUPPORTED -> the library's message: none
REFUSED = {}

# n Ntot N Nc m flavour nsteps forb (real forbidden states: full weights of that rank)
Prob = collections.namedtuple("Prob", "n Ntot N Nc m flavour nsteps forb")
# ens: samples of the ensemble (0: by the compute units, two_wg_samples); expect_ens: what differs in the record after the ensemble;
# partner: options of a second run of the same problem that the source promises to be BIT-identical
Cell = collections.namedtuple("Cell", "name NT route variant prob kind opts expect expect_ens chunks ens partner")


def rec(obj, fwd=None, spw=0, qw=0, wgs=0, **flags):
    assert set(flags) <= set(FLAGS), flags
    r = {"object": obj, "forward_object": fwd or obj, "slabs_per_workgroup": spw, "quads_per_workgroup": qw, "backward_workgroups": wgs}
    r.update({f: bool(flags.get(f, False)) for f in FLAGS})
    return r


def prob(NT, Nc=3, full=False, uniform=False, m=3, N=N, nsteps=NSTEPS, forb=0):
    return Prob(NT, 16 * NT if full else 16 * NT - 3, N, min(Nc, 2) if NT == 1 else Nc, m, "uniform" if uniform else "varied", nsteps, forb)


def _cells():
    out = []

    def add(NT, route, variant, pr, expect, opts=None, kind="neumann", expect_ens=None, chunks=CHUNKS, ens=NQUAD, partner=None):
        opts, partner = dict(opts or {}), (dict(partner) if partner is not None else None)
        if NT == 1:
            opts["lane"] = 0
            if partner is not None:
                partner["lane"] = 0
            if route == "quad3" and opts.get("s_compact", 1) == 1:      # a single 16-row block is uniform whatever its entries: SC is taken
                expect = dict(expect, sc_forward=True, sc_backward=expect["ord"])
        out.append(Cell("%s-%s-NT%d" % (route, variant, NT), NT, route, variant, pr, kind, opts, expect, expect_ens or {}, chunks, ens, partner))

    for NT in range(1, 9):
        k, s, p, u, q, v = ("%s_%d_7" % (c, NT) for c in "kspuqv")
        nc3 = {1: 2, 7: 2, 8: 1}.get(NT, 3)      # controls next to which three slabs per workgroup fit the LDS
        base, full = prob(NT, min(nc3, 3) if NT != 8 else 2), prob(NT, nc3 if NT != 8 else 2, full=True, uniform=True)
        # ---- quad layout, three slabs per workgroup
        o3 = {"quad8": 2}
        if nc3 >= 2:
            ragged, whole = prob(NT, nc3), prob(NT, nc3, full=True, uniform=True)
            add(NT, "quad3", "ord", ragged, rec(k, spw=3, uni=True, ord=True), o3)
            add(NT, "quad3", "ord+sc", whole, rec(k, spw=3, uni=True, ord=True, sc_forward=True, sc_backward=True), o3, partner=dict(o3, s_compact=0))
            add(NT, "quad3", "s_compact0", whole, rec(k, spw=3, uni=True, ord=True), dict(o3, s_compact=0))
            add(NT, "quad3", "uni", ragged, rec(k, spw=3, uni=True), dict(o3, no_ord=1))
            add(NT, "quad3", "generic", ragged, rec(k, spw=3), dict(o3, no_uni=1))
            if nc3 == 3:
                add(NT, "quad3", "ord-nc2", prob(NT, 2), rec(k, spw=3, uni=True, ord=True), o3)
        else:      # NT = 8: one control, so no ORD and no SC backward kernel
            ragged, whole = prob(NT, 1), prob(NT, 1, full=True, uniform=True)
            add(NT, "quad3", "uni", ragged, rec(k, spw=3, uni=True), o3)
            add(NT, "quad3", "uni+scfwd", whole, rec(k, spw=3, uni=True, sc_forward=True), o3, partner=dict(o3, s_compact=0))
            add(NT, "quad3", "generic", ragged, rec(k, spw=3), dict(o3, no_uni=1))
        add(NT, "quad3", "generic-n2", prob(NT, nc3, N=2), rec(k, spw=3), o3)      # (uni needs N % 4 == 0)
        # ---- quad layout, one / two slabs per workgroup: no specialisation
        add(NT, "quad1", "generic", base, rec(s, spw=1), {"cq": 0, "qsplit": 0})
        add(NT, "quad2", "generic", full, rec(s, spw=2), {"quad8": 1})
        # ---- split quad backward sweep behind the one-slab forward kernel
        if NT <= 6:
            add(NT, "qsplit4", "ord", base, rec(p, s, spw=1, qw=4, ord=True), {"cq": 0}, partner={"cq": 0, "qsplit": 0})
            if NT >= 2:
                add(NT, "qsplit4", "ride", full, rec(p, s, spw=1, qw=4, ord=True, ride=True), {"cq": 0, "qs_ride": 1})
            add(NT, "qsplit4", "generic", base, rec(p, s, spw=1, qw=4), {"cq": 0, "no_ord": 1})
        # ---- ... and behind the cooperative-quad forward kernel (m = 3: MODD forward kernel)
        if 2 <= NT <= 6:
            o2 = {"qsplit": 2, "cq3": 0}
            add(NT, "qsplit2", "ride", base, rec(p, u, qw=2, ord=True, ride=True, modd=True), o2)
            add(NT, "qsplit2", "ord", full, rec(p, u, qw=2, ord=True, modd=True), dict(o2, qs_ride=0))
            add(NT, "qsplit2", "ord-nc2", prob(NT, 2), rec(p, u, qw=2, ord=True, modd=True), o2)
            add(NT, "qsplit2", "generic", base, rec(p, u, qw=2, modd=True), dict(o2, no_ord=1))
        # ---- cooperative quad
        if 2 <= NT <= 7:
            o1 = {"cq3": 0}
            m4, m4full = prob(NT, m=4), prob(NT, full=True, uniform=True, m=4)
            add(NT, "cq1", "ord-m3", base if base.Nc == 3 else prob(NT), rec(u, wgs=1, ord=True, modd=True), o1)
            add(NT, "cq1", "generic-m3", base if base.Nc == 3 else prob(NT), rec(u, wgs=1, modd=True), dict(o1, cq_generic_traces=1))
            add(NT, "cq1", "ord-m4", m4full, rec(u, wgs=1, ord=True), o1)
            add(NT, "cq1", "generic-m4", m4full, rec(u, wgs=1), dict(o1, cq_generic_traces=1))
            add(NT, "cq1", "ord-n2", prob(NT, N=2), rec(u, wgs=1, ord=True, modd=True), o1)      # (two samples per column quad)
            add(NT, "cq1", "fwd2", m4, rec(u, wgs=1, ord=True, fwd2=True), dict(o1, cq_fwd2=1), partner=dict(o1, cq_fwd2=0))
            if NT == 3:
                add(NT, "cq1", "ord-m0", prob(NT, m=0), rec(u, wgs=1, ord=True), o1)
                add(NT, "cq1", "ord-m1", prob(NT, m=1), rec(u, wgs=1, ord=True, modd=True), o1)
            # the split backward sweep: default options only, one chunk of 11 steps
            s3, s4 = prob(NT, nsteps=SPLIT_STEPS), prob(NT, m=4, nsteps=SPLIT_STEPS)
            add(NT, "cq-split", "three", s3, rec(u, wgs=3, ord=True, modd=True), {}, chunks=(0,), partner={"cq3": 0})
            add(NT, "cq-split", "two", s4, rec(u, wgs=3, ord=True), {}, expect_ens={"backward_workgroups": 2}, chunks=(0,), ens=0, partner={"cq3": 0})
            ncw = 2 if NT == 7 else 3
            add(NT, "cq-wlr", "one", prob(NT, ncw, forb=2), rec(u, wgs=1, ord=True, modd=True, wlr=True), o1)
            add(NT, "cq-wlr", "three", prob(NT, ncw, m=4, nsteps=SPLIT_STEPS, forb=2), rec(u, wgs=3, ord=True, wlr=True), {}, chunks=(0,), partner={"cq3": 0})
        # ---- JQ_BW_T4 slab kernels
        ot = {"coop_max": 0, "lane": 0, "dq": 0, "quad": 0}
        add(NT, "t4", "neumann", base, rec("k_%d_8" % NT), ot)
        add(NT, "t4", "jacobi", base, rec("j_%d_8" % NT), ot, kind="jacobi")
        # ---- JQ_BW_OD
        if 2 <= NT <= 6:
            od = prob(NT, full=(NT == 4), uniform=(NT == 4))
            add(NT, "od", "slab-neumann", od, rec("k_%d_9" % NT), dict(ot, t4=0))
            add(NT, "od", "slab-jacobi", od, rec("j_%d_9" % NT), dict(ot, t4=0), kind="jacobi")
            add(NT, "od", "coop-neumann", od, rec("c_%d_9" % NT), {"t4": 0, "dq": 0} if NT == 2 else {"t4": 0})
            add(NT, "od", "coop-imr", od, rec("i_%d_9" % NT), {"t4": 0, "dq": 0} if NT == 2 else {"t4": 0}, kind="imr")
        # ---- implicit midpoint on the structure
        add(NT, "imr", "quad-n2", prob(NT, N=2), rec(q, spw=1), {}, kind="imr")
        add(NT, "imr", "quad-n4", base, rec(q, spw=1), {} if NT in (1, 8) else {"imr_cq": 0}, kind="imr")
        if 2 <= NT <= 7:
            two = NT <= 6
            add(NT, "imr", "cq", base if base.Nc == 3 else prob(NT), rec(v, wgs=1, imr_two_sets=two), {}, kind="imr", partner={"imr_cq2": 0} if two else None)
            if two:
                add(NT, "imr", "cq-one-set", full, rec(v, wgs=1), {"imr_cq2": 0}, kind="imr")
    return tuple(out)


CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
assert len(BY_NAME) == len(CELLS)
# objects that ship in the VGPR register form (csrc/Makefile KCC): their cells go through the default-form twin as well
VGPR_PREFIXES = ("s_", "p_", "q_")


def in_vgpr_form(tag):
    nt = int(tag.split("_")[1])
    return tag.startswith(VGPR_PREFIXES) or (tag.startswith("k_") and tag.endswith(("_8", "_9"))) or (tag.startswith("c_") and tag.endswith("_9") and nt <= 6)


VGPR_CELLS = tuple(c for c in CELLS if in_vgpr_form(c.expect["object"]) or in_vgpr_form(c.expect["forward_object"]))


def plan_uniform(pr):
    """plan info s_uniform of a 4 x 4 x n plan: true Kronecker products on full blocks -- and every problem of ONE 16-row block (nothing to repeat)"""
    return pr.n == 1 or (pr.flavour == "uniform" and pr.Ntot % 16 == 0)


def family_of(cell):
    """(kernel_family, kernel_band) of jq_last_timing for the cell's object"""
    tag = cell.expect["object"]
    pre, band = tag[0], int(tag.split("_")[2])
    if pre == "p" and cell.expect["forward_object"][0] == "u":      # the split quad sweep behind the cooperative-quad plan
        return 8, band
    return {"k": 6 if band == 7 else 0, "s": 6, "p": 6, "u": 8, "v": 9, "q": 7, "j": 0, "c": 1, "i": 5}[pre], band


def two_wg_samples(cu, Nq=N):
    """the smallest ensemble whose backward sweep takes two workgroups per column quad: 3 nq_pad > compute units >= 2 nq_pad"""
    for nslabs in range(1, cu):
        nq_pad = (4 * nslabs + 7) // 8 * 8
        if 3 * nq_pad > cu:
            assert 2 * nq_pad <= cu, (cu, nq_pad)
            return (16 // Nq) * (nslabs - 1) + 1
    raise AssertionError(cu)


Problem = collections.namedtuple("Problem", "p pcof nodes weights shift")
_problems, _lock = {}, threading.Lock()


def seed_of(pr):
    return 17000 + 1000 * pr.Ntot + 100 * pr.N + 10 * pr.m + 4 * pr.Nc + 2 * (pr.flavour == "uniform") + (pr.nsteps != NSTEPS) + 500000 * pr.forb


def base_problem(jq, pr):
    """(params, pcof, rng) of a Prob, built once; ensembles draw their nodes from a generator of their own (ensemble)"""
    with _lock:
        if pr not in _problems:
            rng = np.random.default_rng(seed_of(pr))
            p, pcof = subsystem_problem(jq, rng, pr.n, pr.Ntot, pr.N, pr.Nc, pr.m, pr.flavour, pr.nsteps, OBJ_FUNC_TYPE)
            if pr.forb:      # real forbidden states, as tests/test_gpu_round5.py _real_forbidden: W = sum_k w_k f_k f_k' of rank pr.forb
                fs = rng.standard_normal((pr.Ntot, pr.forb))
                fs = fs / np.linalg.norm(fs, axis=0)
                fw = 0.5 + rng.random(pr.forb)
                p.forb_states, p.forb_weights = fs.astype(complex), fw
                W = sum(fw[k] * np.outer(fs[:, k], fs[:, k]) for k in range(pr.forb))
                p.wmat_real, p.wmat_imag = np.asfortranarray(W.copy()), np.zeros_like(W, order="F")
            _problems[pr] = (p, pcof)
        return _problems[pr]


def ensemble(jq, pr, ns):
    p, pcof = base_problem(jq, pr)
    rng = np.random.default_rng(seed_of(pr) + 7 * ns + 1)
    shift = 0.05 * rng.standard_normal(pr.Ntot)
    shift[0] = 0.0
    return Problem(p, pcof, 0.1 * rng.standard_normal(ns), rng.random(ns), shift)


def with_solver(jq, p, kind, forb):
    q = B.with_solver(jq, p, kind)
    assert not (forb and kind == "imr")
    return q


# ---- the CPU oracle's side ---------------------------------------------------------------------------------------------------------------
MI355X_CUS = 256      # (the pool starts before a handle exists: another device's two-workgroup ensembles are computed when asked for)


def _reference(jq, pr, kind, ns):
    return B.oracle_reference(jq, ensemble(jq, pr, ns), kind, True)


_pool = None


def reference(jq, cell, ns):
    global _pool
    if _pool is None:
        _pool = B.ReferencePool(lambda: [((c.prob, c.kind, c.ens or two_wg_samples(MI355X_CUS)), _reference, (jq, c.prob, c.kind, c.ens or two_wg_samples(MI355X_CUS)))
                                         for c in CELLS if c.name not in REFUSED],
                                missing=lambda key: (_reference, jq) + key)
    return _pool.result((cell.prob, cell.kind, ns))


# ---- the GPU's side ----------------------------------------------------------------------------------------------------------------------
def run_cell(jq, cell, opts=None, check=True):
    """A cell on the GPU with its options (opts: its bit-identical partner's): one gradient evaluation per chunking, then the per-step
    history and the ensemble on the last handle.  check: the last_kernels record, family / size / band of last_timing and the manifest
    after every evaluation with a gradient.
    -> {"tag", "evals": [(objfv, infidelity, leak, totalgrad, infidelgrad, leakgrad) per chunking], "history", "ensemble", "ns", "records"}"""
    pr, kind = cell.prob, cell.kind
    p0, pcof = base_problem(jq, pr)
    p = with_solver(jq, p0, kind, pr.forb)
    WA = jq.Working_Arrays_M_HIP if kind == "imr" else jq.Working_Arrays_HIP
    out = {"evals": [], "tag": cell.expect["object"], "records": []}

    def verify(wa, expect):
        plan, t = wa.plan_info(), wa.last_timing()
        out["records"].append(plan["last_kernels"])
        if not check:
            return
        assert plan["last_kernels"] == expect, (plan["last_kernels"], expect, plan["latency_split"])
        assert (t["kernel_family"], t["kernel_band"]) == family_of(cell) and t["kernel_size"] == cell.NT == plan["tile_rows"], (t, plan["tile_rows"])
        assert plan["structure"] == ("od" if cell.route == "od" else "t4") and plan["full_weight_rank"] == pr.forb
        assert plan["s_uniform"] == (cell.route != "od" and plan_uniform(pr))
        if plan["build"]["manifest"]:      # (the build manifest is linked in)
            assert {expect["object"], expect["forward_object"]} <= set(plan["build"]["objects"]), sorted(plan["build"]["objects"])

    for chunk in cell.chunks:
        o = dict(cell.opts if opts is None else opts)
        if chunk:
            o["chunk_steps"] = chunk
        wa = WA(p, pcof.size, options=o)
        try:
            assert wa.plan_info()["last_kernels"] is None      # (no evaluation yet)
            objfv, tg, prim, sec, tinf, ig, lg = jq.traceobjgrad(pcof, p, wa, False, True)
            out["evals"].append((objfv, prim, sec, tg.copy(), ig.copy(), lg.copy()))
            verify(wa, cell.expect)
            if chunk == cell.chunks[-1]:
                out["history"] = jq.traceobjgrad(pcof, p, wa, True, False)[1]
                ns = out["ns"] = cell.ens or two_wg_samples(wa.plan_info()["compute_units"], pr.N)
                e = ensemble(jq, pr, ns)
                jq.eval_f_g_grad(pcof, p, wa, e.nodes, e.weights, True, shift=e.shift)
                verify(wa, dict(cell.expect, **cell.expect_ens))
                out["ensemble"] = (p.last_infidelity, p.last_leak, p.last_infidelity_grad.copy(), p.last_leak_grad.copy())
        finally:
            wa.close()
    return out


if __name__ == "__main__":
    B.dump_main(lambda jq: ((c.name, run_cell(jq, c)) for c in VGPR_CELLS if c.name not in REFUSED))
