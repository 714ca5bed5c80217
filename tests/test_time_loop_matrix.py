"""CPU: the time-loop matrix of tests/test_gpu_time_loop.py is complete -- every propagator object csrc/Makefile builds (the LANE and
ROWLANE lists included) is the target of a cell or known unreachable --, its
runs cover what the time loop can differ in (chunk position x parity of its length, Neumann class x parity, chunks and problems of 1 and
2 steps, every order 0 .. 6 on every route), its expectations follow the options (workgroups of the split latency kernels by the
first backward chunk, `modd` by the run's order), and its references discriminate: on the ORACLE every Neumann order a run uses moves
the gradient by >= 1e-7 relative against the order below it, three orders of magnitude above the tolerance the GPU side asserts."""
import collections
import concurrent.futures
import os
import re

import numpy as np
import pytest

import block_band_matrix as B
import structured_matrix as M
import time_loop_matrix as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_EFFECT = 1e-7


def built_objects():
    """every propagator object of KOBJS: the pattern lists expanded, the explicit ones, l_ / r_ / m_ by their padded sizes"""
    text = open(os.path.join(ROOT, "juqbox.jl_amd", "csrc", "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2) for m in re.finditer(r"^(\w+) = (.*)$", text, re.M)}
    lists = {name: var[name].split() for name in ("INST", "QUAD", "QUADBIG", "BIG", "LANE", "ROWLANE")}
    m = re.fullmatch(r"\$\(filter-out ([\d_ ]+),\$\(INST\)\)", var["COOP"].strip())
    assert m, var["COOP"]
    lists["COOP"] = [x for x in lists["INST"] if x not in m.group(1).split()]
    built, rest = set(), var["KOBJS"]
    for name, prefix in re.findall(r"\$\((\w+):%=\$\(OBJDIR\)/(\w)_%\.o\)", rest):
        built |= {"%s_%s" % (prefix, e) for e in lists[name]}
    rest = re.sub(r"\$\(\w+:%=\$\(OBJDIR\)/\w_%\.o\)", "", rest)
    built |= set(re.findall(r"\$\(OBJDIR\)/(\w_\d+_\d+)\.o", rest))
    assert not re.sub(r"\$\(OBJDIR\)/\w_\d+_\d+\.o", "", rest).strip(), rest
    assert lists["LANE"] == [str(n) for n in T.LANE_NP] and lists["ROWLANE"] == [str(n) for n in T.ROWLANE_NPJ]
    return built


def test_every_propagator_object_is_the_target_of_a_cell_or_known_unreachable():
    built = built_objects()
    have = set().union(*(T.objects_of(c) for c in T.CELLS)) | {c.expect[3] for c in T.TL_CELLS if c.expect[3]}
    assert have - built == set(), "cells whose object is not built: %s" % sorted(have - built)
    left = built - have - set(T.UNREACHABLE)
    assert left == set(), "objects without a cell: %s" % sorted(left)
    assert set(T.UNREACHABLE) == {"u_1_7", "v_1_7", "t_1_7"} and set(T.UNREACHABLE) <= built and not set(T.UNREACHABLE) & have
    assert {"t_%d_7" % n for n in range(2, 7)} <= {c.expect[3] for c in T.TL_CELLS}
    for pre, sizes in (("l", T.LANE_NP), ("r", T.ROWLANE_NPJ), ("m", T.ROWLANE_NPJ)):
        assert {"%s_%d" % (pre, n) for n in sizes} <= have
    assert {"i_1_0", "k_1_0", "j_1_0", "w_1_0", "w_6_5", "x_1_0", "x_6_5"} | {"w_%d_7" % n for n in range(1, 9)} <= have


def test_every_cell_of_the_source_matrices_is_a_cell_here():
    band = [c for c in T.CELLS if c.source == "band"]
    assert [(c.key[0], c.key[1]) for c in band] == [(bc, 16 * bc.NT - 3) for bc in B.CELLS if bc.tag is not None]
    assert all((c.key[0], c.key[1]) in B.CASES for c in band)
    assert [c.key for c in T.CELLS if c.source == "structured"] == [sc for sc in M.CELLS if sc.name not in M.REFUSED]
    assert not B.REFUSED and not M.REFUSED      # (no cell is refused: nothing here is skipped)
    for c in T.CELLS:
        assert (c.index is None) == (c.kind != "neumann") and c.kind in ("neumann", "jacobi", "imr")
    for route, cells in _routes().items():
        assert [c.index for c in cells] == list(range(len(cells))), route


def test_the_small_cells_are_the_table_of_padded_sizes():
    for s in T.SMALL:
        family, size = s.timing[0], s.timing[1]
        if s.tag[0] in "wx":      # the objects with the low-rank terms of full weights: <tile rows, band code> of the tag
            assert s.forb > 0 and (family, size, s.timing[2], s.timing[3]) == (6 if s.tag.endswith("_7") else 0, int(s.tag.split("_")[1]), int(s.tag.split("_")[2]), 0)
            assert 16 * (size - 1) < s.Ntot <= 16 * size and s.kind == ("neumann" if s.tag[0] == "w" else "jacobi")
            continue
        assert s.Ntot <= 16 and 1 <= s.N <= s.Ntot and s.timing[2] == 0
        if s.tag[0] == "l":
            assert family == 2 and size == T.padded(s.Ntot, T.LANE_NP) and s.opts == {"rowlane_max": 0} and s.tag == "l_%d" % size
        elif s.tag[0] in "rm":
            assert family == (3 if s.tag[0] == "r" else 4) and size == T.padded(s.Ntot, T.ROWLANE_NPJ) and s.tag == "%s_%d" % (s.tag[0], size)
            waves = {None: 3 if s.tag[0] == "r" else 2, 2: 2, 0: 1}[s.opts.get("rl_split")]
            if s.forb:      # full weights: one wave
                waves = 1
            assert s.timing[3] == {1: 0, 2: 32, 3: 33}[waves], s
        else:
            assert s.timing == ({"i": 5, "k": 0, "j": 0}[s.tag[0]], 1, 0, 0) and s.Ntot == 13
    assert len({s.name for s in T.SMALL}) == len(T.SMALL)


def _routes():
    routes = collections.defaultdict(list)
    for c in T.CELLS:
        if c.kind == "neumann":
            routes[c.route].append(c)
    return routes


def _positions(run):
    cs = T.chunks(run)
    if len(cs) == 1:
        return {("only", cs[0] % 2)}
    return {("first", cs[0] % 2), ("last", cs[-1] % 2)} | {("middle", c % 2) for c in cs[1:-1]}


def test_chunk_lists_of_the_runs():
    want = {"A1": [1], "A2": [2], "A3": [1, 1], "A4": [2, 2, 2, 2, 1], "A5": [3, 3, 2], "A6": [4, 4, 3], "A7": [9], "A8": [9, 9, 2], "A9": [10, 10, 1]}
    assert {r.name: T.chunks(r) for r in T.RUNS + T.SPLIT_RUNS} == want
    assert all(sum(T.chunks(r)) == r.nsteps <= 25 for r in T.RUNS + T.SPLIT_RUNS)      # (n <= 25: inside the derivation of exception (i))


def test_every_cell_sees_every_chunk_position_at_both_parities():
    want = {(pos, par) for pos in ("only", "first", "middle", "last") for par in (0, 1)}
    for c in T.CELLS:
        runs = T.runs_of(c)
        assert runs[:6] == T.RUNS and set().union(*(_positions(r) for r in runs[:6])) == want
        assert {1, 2} <= {r.nsteps for r in runs} and {1, 2} <= {n for r in runs for n in T.chunks(r)}
        assert (len(runs) == 9) == T.splits(c)
        assert len({(r.nsteps, r.chunk) for r in runs}) == len(runs)      # (no two runs of a cell are the same (nsteps, chunking))


def test_every_route_sees_every_order_and_every_class_at_both_parities():
    cls = lambda m: "none" if m == 0 else "odd" if m % 2 else "even"
    for route, cells in _routes().items():
        assert len(cells) >= 3, route
        orders, pairs, per_run = set(), set(), collections.defaultdict(set)
        for c in cells:
            ms = {r.name: T.m_run(c, r) for r in T.runs_of(c)}
            assert ms["A4"] == 0 and ms["A5"] in T.ODD and ms["A6"] in T.EVEN
            assert {cls(ms[n]) for n in ("A1", "A2", "A3")} == {"none", "odd", "even"}, c.name
            for r in T.runs_of(c):
                orders.add(ms[r.name])
                per_run[r.name].add(cls(ms[r.name]))
                pairs |= {(cls(ms[r.name]), n % 2) for n in T.chunks(r)}
        assert orders == set(range(7)), (route, orders)
        assert pairs == {(k, par) for k in ("none", "odd", "even") for par in (0, 1)}, route
        for name in ("A1", "A2", "A3"):
            assert per_run[name] == {"none", "odd", "even"}, (route, name)
        if any(T.splits(c) for c in cells):
            assert all(per_run[name] == {"none", "odd", "even"} for name in ("A7", "A8", "A9")), route


def test_expectations_follow_the_options():
    split_cells = [c for c in T.CELLS if T.splits(c)]
    assert {c.key.route for c in split_cells} == {"cq-split", "cq-wlr", "imr"} and len(split_cells) >= 3 * 6
    for c in T.CELLS:
        if c.source != "structured":
            assert T.expected_record(c, T.RUNS[0]) is None
            continue
        sc = c.key
        if T.splits(c):      # default options on the cooperative-quad plan: nothing that switches the split off
            assert "cq3" not in sc.opts and "cq" not in sc.opts and "quad8" not in sc.opts, c.name
        for r in T.runs_of(c):
            e = T.expected_record(c, r)
            same = {k: v for k, v in e.items() if k not in ("modd", "backward_workgroups", "imr_two_sets")}
            assert same == {k: sc.expect[k] for k in same}
            m = T.m_run(c, r)
            assert e["modd"] == (sc.kind == "neumann" and e["forward_object"][0] == "u" and m % 2 == 1), (c.name, r.name)
            if T.splits(c):
                taken = T.chunks(r)[0] > T.RING
                assert taken == (r.name in ("A7", "A8", "A9")) and e["backward_workgroups"] == (3 if taken else 1)
                assert T.expected_decision(c, r).startswith("taken" if taken else "not taken: the first chunk")
                assert e["imr_two_sets"] == (sc.expect["imr_two_sets"] and not taken)
            else:
                assert e["backward_workgroups"] == sc.expect["backward_workgroups"] and e["imr_two_sets"] == sc.expect["imr_two_sets"]
            o = T.options(c, r)
            assert o.get("chunk_steps", 0) == r.chunk and {k: v for k, v in o.items() if k != "chunk_steps"} == sc.opts
        # at the source's own shape the table gives the source's record back
        src = T.Run("src", sc.prob.nsteps, 0, "odd")
        if sc.kind != "neumann" or T.m_of(c.index, src) % 2 == sc.prob.m % 2:
            assert T.expected_record(c, src) == sc.expect, c.name


def test_the_runs_keep_the_step_size_of_their_source(jq):
    for c in T.CELLS[::7]:
        p0, pcof0 = T.source_problem(jq, c)
        before = (p0.T, p0.nsteps, p0.linear_solver.max_iter)
        for r in T.runs_of(c):
            p, pcof = T.run_problem(jq, c, r)
            assert p is not p0 and p.nsteps == r.nsteps and abs(p.T / p.nsteps - p0.T / p0.nsteps) <= 1e-15 * p0.T and pcof is not None
            if c.kind == "neumann":
                assert p.linear_solver.max_iter == T.m_run(c, r)
        assert (p0.T, p0.nsteps, p0.linear_solver.max_iter) == before      # (the source matrices' problems are shared, not modified)




def _neumann_problems():
    """{problem key: (a cell, {(nsteps, m): run} for every m > 0 a run of any cell on the problem uses)}"""
    wanted = {}
    for c in T.CELLS:
        if c.kind == "neumann":
            for r in T.runs_of(c):
                if T.m_run(c, r) > 0:
                    wanted.setdefault(T.problem_key(c), (c, {}))[1].setdefault((r.nsteps, T.m_run(c, r)), (c, r))
    return wanted


def test_amplitude_keys_name_the_problems():
    keys = collections.defaultdict(set)
    for c in T.CELLS:
        keys[T.amplitude_key(c)].add(T.problem_key(c))
    assert all(len(v) == 1 for v in keys.values()), [k for k, v in keys.items() if len(v) > 1]
    assert set(T.AMPLITUDE) <= {T.amplitude_key(c) for c in T.CELLS if c.kind == "neumann"} and set(T.AMPLITUDE.values()) <= set(T.FACTORS[1:])
    assert all(T.amplitude(c) == 1 for c in T.CELLS if c.kind != "neumann")


def _pool():
    from oracle.oracle import lib
    lib()      # (loaded before the threads start)
    return concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(12, (os.cpu_count() or 2) - 1)))


def test_every_neumann_order_a_run_uses_is_visible_in_the_oracles_gradient_at_the_first_factor_that_does_it(jq):
    """relative change of the oracle's gradient from order m - 1 to m, for every (step count, m > 0) a run of the problem uses: >= 1e-7
    at the problem's amplitude factor, and -- the factor is the FIRST that does -- below it for some run at the factor before"""
    from oracle.oracle import Oracle

    def smallest(c, uses, f):
        worst = np.inf
        for (nsteps, m), (cc, r) in uses.items():
            g = [Oracle(p, use_sparse=T.sparse_oracle(cc)).traceobjgrad(pcof)["totalgrad"]
                 for p, pcof in (T.run_problem(jq, cc, r, m=k, scale=f) for k in (m, m - 1))]
            worst = min(worst, np.linalg.norm(g[0] - g[1]) / np.linalg.norm(g[0]))
        return worst

    def check(c, uses):
        f = T.amplitude(c)
        return smallest(c, uses, f), (smallest(c, uses, T.FACTORS[T.FACTORS.index(f) - 1]) if f > 1 else 0.0)

    problems = _neumann_problems()
    assert len(problems) >= 130 and all(len({T.amplitude(cc) for cc, _ in uses.values()}) == 1 for _, uses in problems.values())
    with _pool() as pool:
        futures = {k: pool.submit(check, c, uses) for k, (c, uses) in problems.items()}
        got = {k: f.result() for k, f in futures.items()}
    print("smallest effect of a Neumann term at the chosen factors: %.2e" % min(v[0] for v in got.values()))
    assert not [(k, v) for k, v in got.items() if not v[0] >= MIN_EFFECT], sorted((v[0], k) for k, v in got.items())[:5]
    assert not [(k, v) for k, v in got.items() if not v[1] < MIN_EFFECT], [(k, v) for k, v in got.items() if not v[1] < MIN_EFFECT][:5]


def test_the_reference_is_well_conditioned_at_the_amplitude_factors(jq):
    """moving every coefficient by one ulp moves the oracle's objective and gradient by <= 1e-12 relative, on the longest run of a cell
    of every Neumann problem (what the GPU side compares at rtol 1e-10 is the arithmetic, not the conditioning of the problem)"""
    from oracle.oracle import Oracle

    def moved(c):
        r = max(T.runs_of(c), key=lambda r: r.nsteps)
        p, pcof = T.run_problem(jq, c, r)
        orc = Oracle(p, use_sparse=T.sparse_oracle(c))
        a, b = orc.traceobjgrad(pcof), orc.traceobjgrad(np.nextafter(pcof, np.inf))
        return max(abs(a["objfv"] - b["objfv"]) / abs(a["objfv"]), np.linalg.norm(a["totalgrad"] - b["totalgrad"]) / np.linalg.norm(a["totalgrad"]))

    with _pool() as pool:
        futures = {k: pool.submit(moved, c) for k, (c, _) in _neumann_problems().items()}
        got = {k: f.result() for k, f in futures.items()}
    print("one ulp in every coefficient moves the oracle by %.1e .. %.1e relative" % (min(got.values()), max(got.values())))
    assert max(got.values()) <= 1e-12, sorted((v, k) for k, v in got.items())[-5:]


# ---- the sweeps on one representative per kernel template -----------------------------------------------------------------------------------
def test_every_kernel_template_has_a_representative_in_the_sweeps():
    text = open(os.path.join(ROOT, "juqbox.jl_amd", "csrc", "jq_inst_list.h")).read()
    templates = set(re.findall(r"\bX\((k_\w+)", text))
    assert len(templates) >= 35 and templates == set(T.TEMPLATES), sorted(templates ^ set(T.TEMPLATES))
    swept = {c.name for c in T.SWEEP_CELLS}
    for name, cells in T.TEMPLATES.items():
        if name.endswith("_tl") or name in ("k_forward_tl", "k_backward_tl"):      # the tangent-linear twins: the cells of TL_CELLS
            assert cells and set(cells) <= set(T.TL_BY_NAME), (name, cells)
        else:
            assert cells and set(cells) <= swept, (name, set(cells) - swept)
    assert swept == set().union(*(set(v) for k, v in T.TEMPLATES.items() if not k.endswith("_tl"))) | {"sweep-huge-Ntot257"}      # (the run-time-size kernels are no template of the list)
    assert set(T.SV_REPRESENTATIVES) == {c.name for c in T.SWEEP_CELLS if c.kind == "neumann"} == set(T.SWEEP_AMPLITUDE)


def test_the_sweeps_take_every_ring_past_its_depth_and_the_orders_past_the_specialised_range():
    for depth in (5, 7, 8):      # time points of the LDS windows, the split quad sweep's, the split latency kernels' ring
        assert {depth - 1, depth, depth + 1} <= set(T.STEP_SWEEP) and {n for n in T.STEP_SWEEP if n > 2 * depth}      # (... and a second wrap)
    assert {T.RING + 1, T.RING + 2, 2 * T.RING, 2 * T.RING + 1, 3 * T.RING, 3 * T.RING + 1} <= set(T.SPLIT_STEP_SWEEP) and min(T.SPLIT_STEP_SWEEP) > T.RING
    assert max(T.STEP_SWEEP + T.SPLIT_STEP_SWEEP) <= 25
    assert {0, 1, 2, 10, 11, 12} <= set(T.NEUMANN_SWEEP) and T.chunks(T.neumann_runs(T.SWEEP_CELLS[0])[0]) == [2, 2, 1]      # RlTerms<2 .. 10> and both sides
    for c in T.SWEEP_CELLS:
        runs = T.step_runs(c)
        assert [r.nsteps for r in runs] == list(T.SPLIT_STEP_SWEEP if T.always_split(c) else T.STEP_SWEEP) and all(r.chunk == 0 for r in runs)
        if T.splits(c):      # the table's expectation switches with the first backward chunk
            for r in runs + (T.BACKWARD_ONLY,):
                taken = T.first_backward_chunk(r) > T.RING
                if c.source == "structured":
                    assert T.expected_record(c, r)["backward_workgroups"] == (3 if taken else 1)
                else:
                    assert T.expected_timing(c, r)[3] == (3 if taken else 0)
    assert T.first_backward_chunk(T.BACKWARD_ONLY) == 1 and T.chunks(T.BACKWARD_ONLY) == [9]
    assert T.options(T.SWEEP_CELLS[0], T.BACKWARD_ONLY)["trace_bytes"] == 1 and "chunk_steps" not in T.options(T.SWEEP_CELLS[0], T.BACKWARD_ONLY)


def test_the_neumann_sweep_runs_at_the_first_factor_at_which_every_term_is_visible_and_the_reference_is_well_conditioned_there(jq):
    from oracle.oracle import Oracle

    def grads(c, f):
        return [Oracle(p, use_sparse=T.sparse_oracle(c)).traceobjgrad(pcof)["totalgrad"]
                for p, pcof in (T.run_problem(jq, c, r, scale=f) for r in T.neumann_runs(c))]

    def smallest(c, f):
        g = grads(c, f)
        return min(np.linalg.norm(g[m] - g[m - 1]) / np.linalg.norm(g[m]) for m in range(1, len(g)))

    def check(name):
        c, f = T.BY_NAME[name], T.SWEEP_AMPLITUDE[name]
        r = T.neumann_runs(c)[-1]
        p, pcof = T.run_problem(jq, c, r, scale=f)
        orc = Oracle(p, use_sparse=T.sparse_oracle(c))
        a, b = orc.traceobjgrad(pcof), orc.traceobjgrad(np.nextafter(pcof, np.inf))
        moved = max(abs(a["objfv"] - b["objfv"]) / abs(a["objfv"]), np.linalg.norm(a["totalgrad"] - b["totalgrad"]) / np.linalg.norm(a["totalgrad"]))
        return smallest(c, f), smallest(c, T.FACTORS[T.FACTORS.index(f) - 1]), smallest(c, 1), moved

    with _pool() as pool:
        got = dict(zip(T.SV_REPRESENTATIVES, pool.map(check, T.SV_REPRESENTATIVES)))
    print("Neumann sweep: smallest effect of a term %.2e, one ulp moves the oracle by <= %.1e" % (min(v[0] for v in got.values()), max(v[3] for v in got.values())))
    for name, (at, before, at1, moved) in got.items():
        assert at >= MIN_EFFECT > before and at1 < MIN_EFFECT and moved <= 1e-12, (name, at, before, at1, moved)


# ---- the tangent-linear sweeps ----------------------------------------------------------------------------------------------------------------
def test_the_tangent_linear_cells_cover_the_entry_points_routes_and_sizes():
    by = collections.defaultdict(list)
    for c in T.TL_CELLS:
        by[c.api, c.route].append(c)
    assert set(by) == {("jvp", "coop"), ("hvp", "coop"), ("ens", "lane"), ("ens", "rowlane"), ("ens", "quad"), ("drift", "lane"), ("drift", "rowlane"), ("drift", "quad")}
    assert all(c.case.Ntot == 17 for c in by["jvp", "coop"] + by["hvp", "coop"]) and T.TL_NDIR == 2
    assert {c.expect[1] for c in by["ens", "lane"]} == {2, 4, 6} and {c.expect[1] for c in by["ens", "rowlane"]} == {12, 16}
    assert {c.expect[1] for c in by["ens", "quad"]} == {2, 3, 4, 5, 6}
    assert [r.name for r in T.TL_RUNS] == ["A1", "A4", "A5", "A6"] and [T.chunks(r) for r in T.TL_RUNS] == [[1], [2, 2, 2, 2, 1], [3, 3, 2], [4, 4, 3]]
    for (api, route), cells in by.items():
        assert [c.index for c in cells] == list(range(len(cells)))
        if api != "drift":      # (one drift cell per route: orders 0, 1, 2)
            assert len(cells) >= 3 and {T.tl_m(c, r) for c in cells for r in T.TL_RUNS} == set(range(7)), (api, route)
    assert set(T.TL_AMPLITUDE) <= set(T.TL_BY_NAME)


def test_every_order_a_tangent_linear_run_uses_is_visible_at_the_first_factor_that_does_it(jq):
    from oracle.oracle import Oracle

    def smallest(c, f):
        worst = np.inf
        for r in T.TL_RUNS:
            m = T.tl_m(c, r)
            if m > 0:
                g = [Oracle(p).traceobjgrad(pcof)["totalgrad"] for p, pcof in (T.tl_problem(jq, c, r, m=k, scale=f) for k in (m, m - 1))]
                worst = min(worst, np.linalg.norm(g[0] - g[1]) / np.linalg.norm(g[0]))
        return worst

    def check(c):
        f = T.TL_AMPLITUDE.get(c.name, 1)
        r = T.TL_RUNS[-1]
        p, pcof = T.tl_problem(jq, c, r)
        orc = Oracle(p)
        a, b = orc.traceobjgrad(pcof), orc.traceobjgrad(np.nextafter(pcof, np.inf))
        moved = np.linalg.norm(a["totalgrad"] - b["totalgrad"]) / np.linalg.norm(a["totalgrad"])
        return smallest(c, f), (smallest(c, T.FACTORS[T.FACTORS.index(f) - 1]) if f > 1 else 0.0), moved

    for c in T.TL_CELLS:
        T.tl_source(jq, c)
    with _pool() as pool:
        got = dict(zip([c.name for c in T.TL_CELLS], pool.map(check, T.TL_CELLS)))
    for name, (at, before, moved) in got.items():
        assert at >= MIN_EFFECT > before and moved <= 1e-12, (name, at, before, moved)
