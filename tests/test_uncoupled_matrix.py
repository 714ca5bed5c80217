"""CPU: the matrix of tests/test_gpu_uncoupled.py is complete and its reference discriminates.  Uncoupled controls (Hunc_ops) differ
from coupled ones in four places -- the slot jq_create fills, ft(t) of k_ctrl, the fold B = P + Q of k_gradacc, and the structure
detection that sees a zero operator in every pair -- and every kernel family executes them.  Here, on the ORACLE alone: every kernel
family code of jq_timing.kernel_family, the dense policy and the run-time-size kernels are the target of a cell with each kind pattern;
on every problem of the table each control carries its share of the gradients (a dropped or misrouted trace is visible), Rfreq = 0 moves
objective and gradient (a dropped rotation cannot pass), and the operator in the other slot gives a different result (a wrong slot
cannot pass); and the oracle itself is pinned where the reference is not: its adjoint gradient against Richardson-extrapolated central
differences of its own objective at a Neumann order where the truncation does not show, and the identity with the coupled problem
Hsym = 2 Hunc at Rfreq = 0, bit for bit."""
import copy
import os
import re

import numpy as np
import pytest

import block_band_matrix as B
import structured_matrix as M
import uncoupled_problem as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float))
    return np.linalg.norm(a - b) / np.linalg.norm(b)


# ---- completeness ------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_family_is_the_target_of_a_cell_with_every_kind_pattern():
    plan = open(os.path.join(ROOT, "juqbox.jl_amd", "csrc", "jq_host_plan.h")).read()
    names = re.search(r"enum KernelFamily \{([^}]*)\}", plan).group(1).replace(" ", "").split(",")
    assert names == ["KF_SLAB", "KF_COOP", "KF_LANE", "KF_ROWLANE", "KF_ROWLANE_IMR", "KF_COOP_IMR", "KF_QUAD", "KF_QUAD_IMR", "KF_CQ", "KF_CQ_IMR"]
    header = open(os.path.join(ROOT, "include", "juqbox_hip.h")).read()
    doc = header[header.index("int32_t kernel_family;"):header.index("int32_t kernel_size;")]
    assert {int(x) for x in re.findall(r"\b(\d) (?:slab|cooperative|lane|row-lane|quad layout|the same)", doc)} == set(range(len(names)))
    patterns = {f: set() for f in range(len(names))}
    for c in U.CELLS:
        patterns[c.timing[0]].add(U.classify(c.kinds))
    assert all(v == {"s", "a", "mixed"} for v in patterns.values()), patterns
    # the dense policy of the cooperative-quad kernels, the run-time-size kernels, N > 16, control groups, the Jacobi solver
    assert {U.classify(c.kinds) for c in U.CELLS if c.timing[0] == 8 and c.timing[2] == 10} == {"s", "a", "mixed"}
    assert any(c.timing[:3] == (1, 17, 15) for c in U.CELLS)
    assert {c.timing[0] for c in U.CELLS if c.source == "random" and c.key[1] > 16} == {0, 1}
    assert {c.timing[0] for c in U.CELLS if len(c.kinds) > 4} == {0, 3, 6} and all(c.kinds == "sasas" for c in U.CELLS if len(c.kinds) > 4)
    assert {c.timing[0] for c in U.CELLS if c.kind == "jacobi"} == {0, 1}
    assert {c.timing[0] for c in U.IMR_CELLS} == {4, 5, 7, 9} and {c.timing[0] for c in U.SV_CELLS} == {0, 1, 2, 3, 6, 8}
    assert {c.timing[3] for c in U.CELLS} | {c.ens_timing[3] for c in U.CELLS} >= {0, 2, 3, 22, 24, 32, 33}
    for f in (0, 1, 2, 3, 6, 8):      # objFuncType rotates over the cells
        assert {c.oft for c in U.SV_CELLS if c.timing[0] == f} == {1, 2, 3}, f
    assert set(U.REFUSED) <= set(U.BY_NAME)


def test_the_cells_reuse_the_routes_of_the_two_matrices():
    # every NT = 2 cell of the structured matrix, and the interior-block cells
    want = {c.name for c in M.CELLS if c.NT == 2} | set(U.STRUCTURED_EXTRA)
    have = {c.key: c for c in U.CELLS if c.source == "structured"}
    assert set(have) == want and set(U.STRUCTURED_EXTRA) <= set(M.BY_NAME)
    assert {(M.BY_NAME[k].route, M.BY_NAME[k].variant) for k in have} >= {
        ("quad3", "ord"), ("quad3", "ord+sc"), ("quad3", "s_compact0"), ("quad3", "uni"), ("quad3", "generic"), ("quad3", "generic-n2"), ("quad1", "generic"),
        ("quad2", "generic"), ("qsplit4", "ord"), ("qsplit2", "ride"), ("cq1", "ord-m3"), ("cq-split", "three"), ("cq-split", "two"), ("cq-wlr", "one"),
        ("t4", "neumann"), ("t4", "jacobi"), ("od", "slab-neumann"), ("od", "coop-neumann"), ("od", "coop-imr"), ("imr", "quad-n2"), ("imr", "cq")}
    for key, c in have.items():
        sc = M.BY_NAME[key]
        assert c.opts == sc.opts and c.kind == sc.kind and c.ens == sc.ens and c.timing[1] == sc.NT
        assert {k: v for k, v in c.record.items() if not k.startswith("sc_")} == {k: v for k, v in sc.expect.items() if not k.startswith("sc_")}
        if sc.route == "cq-split":      # the first chunk must exceed the ring
            assert sc.prob.nsteps == M.SPLIT_STEPS == 11 and c.timing[3] == 3 and c.ens_timing[3] == (2 if sc.variant == "two" else 3)
        # every Stormer-Verlet cell runs one chunk and several: 3 + 3 + 1, or 9 + 2 where chunks of 3 would leave the split sweep
        if c.kind != "imr":
            split = c.record["backward_workgroups"] == 3
            assert c.chunks == (U.SPLIT_CHUNKS if split else U.CHUNKS) and (not split or U.SPLIT_CHUNKS[1] > 8 and sc.prob.nsteps > U.SPLIT_CHUNKS[1])
    # every route of the block-band matrix at NT = 2 with band codes 0 and 1, and the HBM-operand cooperative kernels at NT 7 / band 15
    band = {c.key[:3] for c in U.CELLS if c.source == "band"}
    assert band == {(2, code, r) for code in (0, 1) for r in B.ROUTES} | {(7, 15, r) for r in B.BIG_ROUTES}
    assert all(c.key[3] == 16 * c.key[0] - 3 for c in U.CELLS if c.source == "band")
    # sizes of the routes the matrices do not have
    assert {(c.key[0], c.timing[1]) for c in U.CELLS if c.timing[0] == 2} == {(5, 6), (8, 8)}
    assert {(c.key[0], c.timing[1]) for c in U.CELLS if c.timing[0] == 3} == {(10, 12), (13, 16)}
    assert all(c.alts == (({"rl_split": 0}, 0), ({"rl_split": 2}, 32), ({"rl_split": 3}, 33)) for c in U.CELLS if c.name.startswith("rowlane-Ntot"))
    assert all(c.chunks == U.CHUNKS for c in U.SV_CELLS if c.source != "structured") and all(c.chunks == (0,) for c in U.IMR_CELLS)
    assert sum(c.chunks == U.SPLIT_CHUNKS for c in U.SV_CELLS) == 3


def test_plan_level_expectations_of_the_converted_operators(jq):
    """jq_s_uniform (= plan info s_uniform) of the antisymmetric slots jq_create fills: an all-symmetric set leaves them zero, which is
    uniform at every size -- so "varied" problems, which the structured matrix runs on the generic S operand, take the SC kernels"""
    from subsystem_problem import t4_mode
    from test_s_compact import s_uniform
    turned_on = 0
    for c in U.CELLS:
        if c.source != "structured":
            continue
        sc, u = M.BY_NAME[c.key], U.problem(jq, c).p
        hanti = U.hanti_images(u)
        if "a" not in c.kinds:
            assert not any(h.any() for h in hanti) and U.plan_uniform(sc, c.kinds)
        if u.Ntot % 16 == 0:
            assert s_uniform(hanti) == int(U.plan_uniform(sc, c.kinds)), c.name
        else:      # a cut Kronecker product is not uniform: only the zero image is
            assert U.plan_uniform(sc, c.kinds) == ("a" not in c.kinds)
        if sc.route == "quad3":
            turned_on += c.record["sc_forward"] and not sc.expect["sc_forward"]
            assert c.record["sc_backward"] == (c.record["sc_forward"] and c.record["ord"])
        # ORD: the part of the T4 image control q fills is that of its ONE operator (bw_trace = t4_mode(Hsym) | t4_mode(Hanti))
        if sc.expect["ord"]:
            assert [t4_mode(h) for h in u.Hunc_ops] == [1 << q for q in range(u.Nunc)]
    assert turned_on >= 1


# ---- the reference must itself discriminate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", U.CELLS, ids=[c.name for c in U.CELLS])
def test_reference_discriminates(jq, cell):
    """(a) every control's coefficient block carries >= 0.01 of the infidelity gradient's norm and (objFuncType != 1) of the leak
    gradient's; (b) Rfreq = 0 moves objective and gradient by more than 1e-6 relative; (c) the first operator in the other slot is a
    different result.  (Implicit-midpoint cells: on the Stormer-Verlet oracle of the same problem -- they have no gradient.)"""
    from oracle.oracle import Oracle
    pr = U.problem(jq, cell)
    u, pcof, sparse = pr.p, pr.pcof, U.sparse_oracle(cell)
    assert u.Nunc == len(cell.kinds) and u.Ncoupled == 0 and u.isSymm == [k == "s" for k in cell.kinds] and u.objFuncType == cell.oft
    assert np.all((np.abs(u.Rfreq) >= 0.2) & (np.abs(u.Rfreq) <= 2.0)) and u.T >= 1.0
    for q, k in enumerate(cell.kinds):
        assert np.array_equal(u.Hunc_ops[q], (pr.coupled.Hsym_ops if k == "s" else pr.coupled.Hanti_ops)[q]) and u.Hunc_ops[q].any()
    assert np.array_equal(u.Hconst, pr.coupled.Hconst) and np.array_equal(u.Cfreq, pr.coupled.Cfreq) and u.T == pr.coupled.T
    r = Oracle(u, use_sparse=sparse).traceobjgrad(pcof)
    shares = []
    for name in ("infidelgrad",) + (("leakgrad",) if cell.oft != 1 else ()):
        g = r[name].reshape(u.Nunc, -1)
        shares.append((np.linalg.norm(g, axis=1) / np.linalg.norm(g)).min())
    v = copy.copy(u)
    v.Rfreq = np.zeros(u.Nunc)
    r0 = Oracle(v, use_sparse=sparse).traceobjgrad(pcof)
    w = copy.copy(u)
    w.isSymm = [not u.isSymm[0]] + list(u.isSymm[1:])
    rs = Oracle(w, use_sparse=sparse).traceobjgrad(pcof)
    e0, s0 = (rel(r0["objfv"], r["objfv"]), rel(r0["totalgrad"], r["totalgrad"])), (rel(rs["objfv"], r["objfv"]), rel(rs["totalgrad"], r["totalgrad"]))
    print("%s kinds %s: smallest gradient share %.3f; Rfreq = 0 moves objective / gradient by %.2e / %.2e; other slot %.2e / %.2e" %
          (cell.name, cell.kinds, min(shares), e0[0], e0[1], s0[0], s0[1]))
    assert min(shares) >= U.MIN_SHARE, shares
    assert min(e0) > 1e-6, e0
    assert not np.isfinite(s0).all() or min(s0) > 1e-6, s0


def test_an_operator_that_fits_neither_slot_is_the_references_error(jq):
    u = U.problem(jq, U.BY_NAME["lane-Ntot5-sa"]).p
    with pytest.raises(ValueError, match="not symmetric or anti-symmetric"):
        jq.objparams(u.Ne, u.Ng, u.T, u.nsteps, Uinit=u.Uinit, Utarget=u.Utarget_r + 0j, Cfreq=u.Cfreq, Rfreq=u.Rfreq, Hconst=u.Hconst,
                     Hunc_ops=[u.Hunc_ops[0] + u.Hunc_ops[1], u.Hunc_ops[1]])


# ---- the oracle, once per kind pattern at the smallest size --------------------------------------------------------------------------------
SMALLEST = ("lane-Ntot5-ss", "lane-Ntot8-aa", "lane-Ntot5-sa", "lane-Ntot8-as")


def richardson(f, x, d, h, levels=3):
    """central differences of f along d at steps h, h / 2, ...: extrapolated to O(h^(2 levels))"""
    T = [[(f(x + (h / 2 ** i) * d) - f(x - (h / 2 ** i) * d)) / (2 * h / 2 ** i)] for i in range(levels)]
    for i in range(1, levels):
        for k in range(1, i + 1):
            T[i].append(T[i][k - 1] + (T[i][k - 1] - T[i - 1][k - 1]) / (4 ** k - 1))
    return T[-1][-1]


@pytest.mark.parametrize("name", SMALLEST)
def test_oracle_gradient_against_richardson_central_differences(jq, name):
    """at Neumann order 24 (order 3 would show its truncation, 1e-6 .. 5e-4: DESIGN section 5) the adjoint gradient is the derivative of
    the objective the forward sweep evaluates: 1e-9 relative along a random direction"""
    from oracle.oracle import Oracle
    cell = U.BY_NAME[name]
    assert {U.BY_NAME[n].kinds for n in SMALLEST} == {"ss", "aa", "sa", "as"} and cell.key[0] <= 8
    pr = U.problem(jq, cell)
    u = copy.copy(pr.p)
    u.linear_solver = jq.lsolver_object(max_iter=U.FD_NEUMANN_TERMS)
    assert u.linear_solver.max_iter >= 20
    o = Oracle(u, use_sparse=False)
    g = o.traceobjgrad(pr.pcof)["totalgrad"]
    rng = np.random.default_rng(cell.seed + 1)
    d = rng.standard_normal(pr.pcof.size)
    d /= np.linalg.norm(d)
    fd = richardson(lambda x: o.traceobjgrad(x, evaladjoint=False)["objfv"], pr.pcof, d, 2e-2)
    print("%s: g.d %.12e, Richardson %.12e, relative difference %.2e (|g| %.3e)" % (name, g @ d, fd, abs(fd - g @ d) / abs(g @ d), np.linalg.norm(g)))
    assert abs(g @ d) > 0.02 * np.linalg.norm(g)      # (the direction sees the gradient)
    assert abs(fd - g @ d) <= 1e-9 * abs(g @ d)


@pytest.mark.parametrize("name", ["lane-Ntot5-ss", "rowlane-Ntot10"])
def test_without_rotation_symmetric_uncoupled_controls_are_the_coupled_problem(jq, name):
    """Rfreq = 0, symmetric operators: ft = 2 p -- the coupled problem Hsym = 2 Hunc, Hanti = 0 under the same coefficients; the oracle
    returns identical bits for the objective and all three gradients"""
    from oracle.oracle import Oracle
    cell = U.BY_NAME[name]
    assert set(cell.kinds) == {"s"}
    pr = U.problem(jq, cell)
    u = copy.copy(pr.p)
    u.Rfreq = np.zeros(u.Nunc)
    a = Oracle(u, use_sparse=False).traceobjgrad(pr.pcof)
    b = Oracle(U.coupled_twin_without_rotation(jq, u), use_sparse=False).traceobjgrad(pr.pcof)
    for k in ("objfv", "primaryobjf", "secondaryobjf", "totalgrad", "infidelgrad", "leakgrad"):
        assert np.array_equal(a[k], b[k]), k
