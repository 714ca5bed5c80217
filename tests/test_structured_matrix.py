"""CPU: the structured matrix of tests/test_gpu_structured.py is complete -- every object csrc/Makefile builds for the structure codes
7, 8, 9 (k / s / p / q / u / v_*_7, k / j_*_8, k / j / c / i_*_9) is the target of a cell or listed as unreachable with its reason, and
every specialised variant has a cell at every NT its object exists for, so a new instantiation without a cell (or a deleted cell) fails
here -- and its generator (tests/subsystem_problem.py) produces what the specialisations are selected for: control q on part 1 << q of
the T4 image only, exact (anti)symmetry, the 4 x 4 x n structure, uniform S images exactly for "uniform" at Ntot = 16 n, and a share of
every control in the oracle's gradients that keeps a dropped or misrouted trace product visible."""
import collections
import os
import re

import numpy as np
import pytest

import structured_matrix as M
from subsystem_problem import PARTS, t4_mode, t4_structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_lists():
    """{name: [entries]} of QUAD, QUADBIG, INST, COOP and {prefix: [list names]} of the users in KOBJS (explicit objects: {tag})"""
    text = open(os.path.join(ROOT, "juqbox.jl_amd", "csrc", "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2) for m in re.finditer(r"^(\w+) = (.*)$", text, re.M)}
    lists = {name: var[name].split() for name in ("INST", "QUAD", "QUADBIG")}
    m = re.fullmatch(r"\$\(filter-out ([\d_ ]+),\$\(INST\)\)", var["COOP"].strip())
    assert m, var["COOP"]
    lists["COOP"] = [x for x in lists["INST"] if x not in m.group(1).split()]
    users = collections.defaultdict(list)
    for name, prefix in re.findall(r"\$\((\w+):%=\$\(OBJDIR\)/(\w)_%\.o\)", var["KOBJS"]):
        if name in lists:
            users[prefix].append(name)
    explicit = set(re.findall(r"\$\(OBJDIR\)/(\w_\d+_\d+)\.o", var["KOBJS"]))
    return lists, dict(users), explicit


def built_structured_objects():
    lists, users, explicit = makefile_lists()
    assert {p: users[p] for p in "kspquvjci"} == {"k": ["INST", "QUAD", "QUADBIG"], "s": ["QUAD", "QUADBIG"], "p": ["QUAD"], "q": ["QUAD", "QUADBIG"],
                                                  "u": ["QUAD"], "v": ["QUAD"], "j": ["INST"], "c": ["COOP"], "i": ["COOP"]}, users
    assert all(e.endswith("_7") for name in ("QUAD", "QUADBIG") for e in lists[name])
    built = {"%s_%s" % (p, e) for p in "kspquvjci" for name in users[p] for e in lists[name] if e.split("_")[1] in ("7", "8", "9")}
    built |= {t for t in explicit if t[0] in "kspquvjci" and t.split("_")[2] in ("7", "8", "9")}
    assert {"u_7_7", "v_7_7"} <= built
    # out of scope (tests/test_gpu_dense_wmat.py): the objects with the low-rank full weights
    assert M.OUT_OF_SCOPE == ("w_*_7", "w_1_0", "w_6_5", "x_*") and {"w", "x"} & set("kspquvjci") == set()
    return built


def targets():
    return {c.expect[k] for c in M.CELLS if c.name not in M.REFUSED for k in ("object", "forward_object")}


def test_every_structured_object_of_the_makefile_is_the_target_of_a_cell_or_known_unreachable():
    built, have = built_structured_objects(), targets()
    assert set(M.UNREACHABLE) == {"u_1_7", "v_1_7"} and set(M.UNREACHABLE) <= built and not set(M.UNREACHABLE) & have
    assert built - have - set(M.UNREACHABLE) == set(), "objects without a cell: %s" % sorted(built - have - set(M.UNREACHABLE))
    assert have - built == set(), "cells whose object is not built: %s" % sorted(have - built)
    # as the object of the BACKWARD kernel too (forward_object alone would leave the specialised sweeps out)
    assert {c.expect["object"] for c in M.CELLS} == have


def variant_table():
    """(route, variant) -> the NTs it must have a cell at.  Three slabs per workgroup fit the LDS next to three controls up to NT = 6,
    two at NT = 7, one at NT = 8 (structured_matrix.py): ORD / SC need two controls, the three-control cells stop at NT = 6."""
    built = built_structured_objects()
    nts = lambda pre, code=7: sorted(int(t.split("_")[1]) for t in built if t.startswith(pre + "_") and t.endswith("_%d" % code) and t not in M.UNREACHABLE)
    k, s, p, q, u, v = (nts(c) for c in "kspquv")
    assert (k, s, p, q, u, v) == (list(range(1, 9)), list(range(1, 9)), list(range(1, 7)), list(range(1, 9)), list(range(2, 8)), list(range(2, 8)))
    two = [n for n in k if n != 8]
    t = {("quad3", "ord"): two, ("quad3", "ord+sc"): two, ("quad3", "s_compact0"): two, ("quad3", "uni"): k, ("quad3", "generic"): k,
         ("quad3", "generic-n2"): k, ("quad3", "ord-nc2"): [n for n in k if 2 <= n <= 6], ("quad3", "uni+scfwd"): [8],
         ("quad1", "generic"): s, ("quad2", "generic"): s,
         ("qsplit4", "ord"): p, ("qsplit4", "ride"): [n for n in p if n >= 2], ("qsplit4", "generic"): p}
    both = [n for n in p if n in u]
    t.update({("qsplit2", vv): both for vv in ("ride", "ord", "ord-nc2", "generic")})
    t.update({("cq1", vv): u for vv in ("ord-m3", "generic-m3", "ord-m4", "generic-m4", "ord-n2", "fwd2")})
    t.update({("cq1", "ord-m0"): [3], ("cq1", "ord-m1"): [3], ("cq-split", "three"): u, ("cq-split", "two"): u, ("cq-wlr", "one"): u, ("cq-wlr", "three"): u})
    t.update({("t4", "neumann"): nts("k", 8), ("t4", "jacobi"): nts("j", 8)})
    assert nts("k", 8) == nts("j", 8) == list(range(1, 9)) and nts("k", 9) == nts("j", 9) == nts("c", 9) == nts("i", 9) == list(range(2, 7))
    t.update({("od", vv): nts("k", 9) for vv in ("slab-neumann", "slab-jacobi", "coop-neumann", "coop-imr")})
    t.update({("imr", "quad-n2"): q, ("imr", "quad-n4"): q, ("imr", "cq"): v, ("imr", "cq-one-set"): [n for n in v if n <= 6]})
    return t


def test_every_variant_has_a_cell_at_every_tile_count_its_object_exists_for():
    want = {(r, vv, n) for (r, vv), ns in variant_table().items() for n in ns}
    have = [(c.route, c.variant, c.NT) for c in M.CELLS]
    assert len(have) == len(set(have)) and set(have) == want, sorted(want ^ set(have))
    assert set(M.REFUSED) <= set(M.BY_NAME)


def test_the_cells_expectations_follow_their_options():
    """the flags of a record are what select_quad_kernels / select_qsplit_kernel / select_cq_kernels derive from the cell's problem and options"""
    for c in M.CELLS:
        e, pr, o = c.expect, c.prob, c.opts
        per_subsystem = 2 <= pr.Nc <= 3      # (the generator's controls are single-subsystem by construction)
        uniform = M.plan_uniform(pr)
        assert 16 * (c.NT - 1) < pr.Ntot <= 16 * c.NT and pr.n == c.NT and (c.NT > 1 or o.get("lane") == 0)
        assert e["modd"] == (e["forward_object"][0] == "u" and pr.m % 2 == 1) and e["wlr"] == (pr.forb > 0)
        if c.route == "quad3":
            uni = pr.N % 4 == 0 and not o.get("no_uni")
            ordv = uni and per_subsystem and not o.get("no_ord")
            sc = uniform and o.get("s_compact", 1) == 1
            assert (e["uni"], e["ord"], e["sc_forward"], e["sc_backward"]) == (uni, ordv, sc, sc and ordv) and e["slabs_per_workgroup"] == 3, c.name
        elif c.route.startswith("qsplit"):
            qw = int(c.route[-1])
            ordv = per_subsystem and not o.get("no_ord")
            ride = ordv and pr.Nc == 3 and o.get("qs_ride") != 0 and (qw == 2 or o.get("qs_ride") == 1)
            assert (e["ord"], e["ride"], e["quads_per_workgroup"]) == (ordv, ride, qw), c.name
        elif c.route.startswith("cq"):
            assert e["ord"] == (not o.get("cq_generic_traces")) and e["fwd2"] == (o.get("cq_fwd2") == 1), c.name
            assert (c.route == "cq1") == (o.get("cq3") == 0 and e["backward_workgroups"] == 1) or c.route == "cq-wlr"
            if c.route == "cq-split" or c.variant == "three":      # default options, one chunk longer than the ring
                assert o == {} and c.chunks == (0,) and pr.nsteps == M.SPLIT_STEPS > 8 and e["backward_workgroups"] == 3
        else:
            assert not any(e[f] for f in M.FLAGS if f != "imr_two_sets"), c.name
        if c.partner is not None:      # bit-identity only where the source promises it
            diff = {k for k in set(c.opts) | set(c.partner) if c.opts.get(k) != c.partner.get(k)}
            assert diff in ({"s_compact"}, {"cq_fwd2"}, {"cq3"}, {"imr_cq2"}, {"qsplit"}), (c.name, diff)
    assert M.two_wg_samples(256) == 81 and M.two_wg_samples(304) == 97


PROBLEMS = sorted({c.prob for c in M.CELLS})


def test_problem_sizes_of_the_matrix():
    for NT in range(1, 9):
        sizes = {pr.Ntot for pr in PROBLEMS if pr.n == NT}
        assert sizes == {16 * NT - 3, 16 * NT}, (NT, sizes)
    assert {pr.m for pr in PROBLEMS} == {0, 1, 3, 4} and {pr.N for pr in PROBLEMS} == {2, 4} and {pr.Nc for pr in PROBLEMS} == {1, 2, 3}
    assert {pr.nsteps for pr in PROBLEMS} == {M.NSTEPS, M.SPLIT_STEPS} and M.NQUAD == 13


@pytest.mark.parametrize("pr", PROBLEMS, ids=lambda pr: "n%d-Ntot%d-N%d-Nc%d-m%d-%s-%dsteps-forb%d" % pr)
def test_generator_gives_single_subsystem_controls(jq, pr):
    p, pcof = M.base_problem(jq, pr)
    assert p.Ntot == pr.Ntot and p.N == pr.N and p.nsteps == pr.nsteps and len(p.Hsym_ops) == len(p.Hanti_ops) == pr.Nc
    for q in range(pr.Nc):      # jq_host_create.h: bw_trace[q] = t4_mode(Hsym_q) | t4_mode(Hanti_q); ctrl_per_subsystem: == 1 << q
        assert t4_mode(p.Hsym_ops[q]) == t4_mode(p.Hanti_ops[q]) == PARTS[q] == 1 << q
        assert np.array_equal(p.Hsym_ops[q], p.Hsym_ops[q].T) and np.array_equal(p.Hanti_ops[q], -p.Hanti_ops[q].T)      # to the bit
        assert t4_structure(p.Hsym_ops[q]) and t4_structure(p.Hanti_ops[q])
    assert np.array_equal(p.Hconst, p.Hconst.T) and t4_structure(p.Hconst) and t4_mode(p.Hconst) == (7 if pr.n > 1 else 3)
    # every entry the part allows is there (no accidental zero that would make a wrong coefficient invisible)
    r, c = np.indices((pr.Ntot, pr.Ntot))
    allowed = {1: r // 4 == c // 4, 2: (abs(r - c) == 4) & (r // 16 == c // 16), 4: abs(r - c) == 16}
    for q in range(pr.Nc):
        assert np.array_equal(p.Hsym_ops[q] != 0, allowed[PARTS[q]])
        assert np.array_equal(p.Hanti_ops[q] != 0, allowed[PARTS[q]] & (r != c))
    # weights on the guard levels: Diagonal, or with forbidden states the full real matrix of that rank
    if pr.forb:
        assert np.linalg.matrix_rank(p.wmat_real) == pr.forb and not np.any(p.wmat_imag)
    else:
        assert not p.wmat_real[:pr.N].any() and p.wmat_real[pr.N:].all()
    # uniform S images: exactly for true Kronecker products on full blocks
    if pr.Ntot % 16 == 0:
        from test_s_compact import s_uniform
        got = s_uniform(p.Hanti_ops)
        assert got == (1 if pr.flavour == "uniform" else 0), (pr, got)
    else:
        assert pr.flavour == "varied"      # (a cut Kronecker product is not uniform: the matrix uses the varied flavour at ragged sizes)


@pytest.mark.parametrize("pr", PROBLEMS, ids=lambda pr: "n%d-Ntot%d-N%d-Nc%d-m%d-%s-%dsteps-forb%d" % pr)
def test_every_control_carries_its_share_of_the_oracles_gradients(jq, pr):
    """each control's block of the infidelity gradient and of the leak gradient holds >= 0.01 of that gradient's norm ON THE ORACLE: a
    dropped or misrouted trace product of one control then moves the gradient by >= 1e-2 relative, eight orders above the tolerance"""
    from oracle.oracle import Oracle
    p, pcof = M.base_problem(jq, pr)
    r = Oracle(p, use_sparse=True).traceobjgrad(pcof)
    for name in ("infidelgrad", "leakgrad"):
        g = r[name].reshape(pr.Nc, -1)
        share = np.linalg.norm(g, axis=1) / np.linalg.norm(g)
        assert share.min() >= 0.01, (name, share)
