"""CPU: the block-band matrix of tests/test_gpu_block_band.py is complete -- every k_ / j_ / c_ / i_ object that csrc/Makefile builds
for a block band (NT >= 2, no structure code) is the target of a cell, so a new instantiation without a cell fails here -- and its
generator (tests/block_band_problem.py) produces what the cells need: the requested block band per operator, full off-diagonal blocks,
exact (anti)symmetry."""
import os
import re

import numpy as np
import pytest

import block_band_matrix as M
from block_band_problem import block_band, tile_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTURE_CODES = {"7", "8", "9"}      # JQ_BW_T4Q, JQ_BW_T4, JQ_BW_OD: the structured matrix (tests/structured_matrix.py, tests/test_structured_matrix.py)


def makefile_lists():
    """{name: [NT_BW, ...]} of INST, COOP and BIG, and {prefix: [list names]} of the k_ / j_ / c_ / i_ objects in KOBJS"""
    text = open(os.path.join(ROOT, "juqbox.jl_amd", "csrc", "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2) for m in re.finditer(r"^(\w+) = (.*)$", text, re.M)}
    lists = {"INST": var["INST"].split(), "BIG": var["BIG"].split()}
    m = re.fullmatch(r"\$\(filter-out ([\d_ ]+),\$\(INST\)\)", var["COOP"].strip())
    assert m, var["COOP"]
    lists["COOP"] = [x for x in lists["INST"] if x not in m.group(1).split()]
    users = {}
    for name, prefix in re.findall(r"\$\((\w+):%=\$\(OBJDIR\)/(\w)_%\.o\)", var["KOBJS"]):
        if prefix in "kjci" and name in lists:
            users.setdefault(prefix, []).append(name)
    return lists, users


def band_entries(entries):
    return [tuple(int(v) for v in e.split("_")) for e in entries if e.split("_")[1] not in STRUCTURE_CODES and e != "1_0"]


def test_every_block_band_object_of_the_makefile_is_the_target_of_a_cell():
    lists, users = makefile_lists()
    assert users == {"k": ["INST"], "j": ["INST"], "c": ["COOP", "BIG"], "i": ["COOP", "BIG"]}, users
    built = {"%s_%d_%d" % (prefix, NT, code) for prefix, names in users.items() for name in names for NT, code in band_entries(lists[name])}
    targets = {c.tag for c in M.CELLS if c.tag is not None}
    assert built - targets == set(), "objects without a cell: %s" % sorted(built - targets)
    assert targets - built == set(), "cells whose object is not built: %s" % sorted(targets - built)


def test_every_route_of_every_instantiation_has_its_cell():
    """slab instantiations: both slab routes; cooperative ones: the three cooperative routes -- removing any one cell fails here"""
    lists, _ = makefile_lists()
    want = {(NT, code, r) for NT, code in band_entries(lists["INST"]) for r in M.ROUTES[:2]} | \
           {(NT, code, r) for NT, code in band_entries(lists["COOP"]) + band_entries(lists["BIG"]) for r in M.ROUTES[2:]}
    have = [(c.NT, c.code, c.route) for c in M.CELLS]
    assert len(have) == len(set(have)) and set(have) == want, sorted(want ^ set(have))
    assert M.REFUSED <= want and all((c.tag is None) == ((c.NT, c.code, c.route) in M.REFUSED) for c in M.CELLS)
    ids = [M.cell_id(c, nt) for c, nt in M.CASES]
    assert len(ids) == len(set(ids))


def test_problem_sizes_of_the_cells():
    for c, Ntot in M.CASES:
        assert tile_rows(Ntot) == c.NT
    for NT in list(M.SMALL_BANDS) + list(M.BIG_NT):
        assert 16 * NT - 3 in M.sizes(NT) and ((16 * NT in M.sizes(NT)) == (NT in (4, 6, 16)))


PROBLEMS = sorted({(c.NT, c.code, Ntot) for c, Ntot in M.CASES})


@pytest.mark.parametrize("NT,code,Ntot", PROBLEMS, ids=lambda v: str(v))
def test_generator_fills_exactly_the_requested_band(jq, NT, code, Ntot):
    band, modes = M.generator_band(NT, code), M.modes(NT, code)
    assert modes == ([1, 0, 2] if band >= 1 else [1])
    # the band the planner will find is the cell's: jq_host_create.h picks BW in {0, 1, 2, NT - 1}, above 96 levels BWc in {1, 2, 15}
    assert code == (band if (band <= 2 and band < NT - 1) else (NT - 1 if NT <= 6 else 15))
    p = M.problem(jq, NT, code, Ntot).p
    assert p.Ntot == Ntot and p.N == M.N and p.nsteps == M.NSTEPS and len(p.Hsym_ops) == len(p.Hanti_ops) == len(modes)
    want = {0: 0, 1: band, 2: band}
    assert block_band(p.Hconst) == band
    for q, mode in enumerate(modes):
        assert block_band(p.Hsym_ops[q]) == want[mode] and block_band(p.Hanti_ops[q]) == want[mode]
    for H, anti, mode in [(p.Hconst, False, 1)] + [(h, False, m) for h, m in zip(p.Hsym_ops, modes)] + [(h, True, m) for h, m in zip(p.Hanti_ops, modes)]:
        assert np.array_equal(H, -H.T if anti else H.T)      # to the bit
        for bi in range(NT):
            for bj in range(NT):
                blk = H[16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16]
                stored = abs(bi - bj) <= band and not (mode == 0 and bi != bj) and not (mode == 2 and bi == bj)
                if not stored:
                    assert not blk.any(), (bi, bj, mode)
                elif bi != bj:
                    assert blk.all(), (bi, bj, mode)      # full: no zero entry, hence not diagonal either
                    assert min(blk.shape) > 1 and np.count_nonzero(blk * (1 - np.eye(*blk.shape))) > 0
                else:
                    assert np.count_nonzero(blk) >= blk.size - blk.shape[0]      # (an antisymmetric block has a zero diagonal)
    # off the structured plans: a dense diagonal block is not 4 x 4 x n (JQ_BW_T4), a full off-diagonal block is not diagonal (JQ_BW_OD)
    assert p.Hconst[0, 5] != 0.0 and (band == 0 or p.Hconst[1, 16] != 0.0)
    # weights on the guard levels only
    assert not p.wmat_real[:M.N].any() and p.wmat_real[M.N:].all()
