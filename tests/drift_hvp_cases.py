"""The cases of jq_eval_f_g_grad_drifts_hvp that tests/test_gpu_drift_hvp.py runs on the device and tests/test_drift_hvp_host.py holds
against the oracle alone (they must discriminate: every member matters, and the ensemble is not the handle's own drift).

A shape is the smallest at which the packing of a route can go wrong:
  lane     Ntot 3 (NP 4) N 2 ; Ntot 6 (NP 6) N 3           a member owns a wave of 64 column lanes, N of them used
  rowlane  Ntot 10 (NPJ 12) N 3 ; Ntot 13 (NPJ 16) N 5     one wave per member ; two waves per member, the second partly empty
  quad     4 x 4 x 2 (Ntot 32) N 4 ; 4 x 4 x 3 zero padded (Ntot 45) N 8     one quad per member ; two quads = one workgroup per member
Every shape: 3 members of unequal weights, 2 directions, 12 time steps (one chunk, or chunk_steps 5: 5 + 5 + 2), objFuncType 1 and 2.
Members: the problem's drift plus a symmetric perturbation of a quarter of its size inside the route's pattern (dense at one tile row,
the 4 x 4 x n pattern on the quad route)."""
import collections

import numpy as np

import drift_hessian_reference as DR
from block_band_problem import block_band_problem
from subsystem_problem import PARTS, _part, subsystem_problem, t4_structure

Shape = collections.namedtuple("Shape", "route Ntot N Nc m n")      # n: blocks of 16 rows (quad route), else 0
NSTEPS, CHUNK, NDIR = 12, 5, 2
WEIGHTS = np.array([0.5, 0.3, 0.2])
SHAPES = (
    Shape("lane", 3, 2, 2, 4, 0),
    Shape("lane", 6, 3, 1, 1, 0),
    Shape("rowlane", 10, 3, 2, 1, 0),
    Shape("rowlane", 13, 5, 1, 4, 0),
    Shape("quad", 32, 4, 3, 1, 2),
    Shape("quad", 45, 8, 2, 4, 3),
)
OBJ_TYPES = (1, 2)
KERNEL_FAMILY = {"lane": 2, "rowlane": 3, "quad": 6}


def kernel_size(s):
    return {"lane": 2 * ((s.Ntot + 1) // 2), "rowlane": 12 if s.Ntot <= 12 else 16, "quad": s.n}[s.route]


def kernel_object(s):
    return {"lane": "l_%d", "rowlane": "r_%d", "quad": "t_%d_7"}[s.route] % kernel_size(s)


def image_stride(s):
    """doubles of an operator image in the route's layout"""
    np_ = kernel_size(s)
    return {"lane": (np_ * np_ + 15) // 16 * 16, "rowlane": 16 * np_, "quad": 128 * s.n}[s.route]


def shape_id(s):
    return "%s-Ntot%d-N%d-Nc%d-m%d" % (s.route, s.Ntot, s.N, s.Nc, s.m)


def member_drifts(rng, s, H0, nmember, size=0.25):
    """[Ntot, Ntot, nmember] symmetric drifts H0 + perturbation, inside the pattern of the route"""
    out = np.zeros((s.Ntot, s.Ntot, nmember), order="F")
    for i in range(nmember):
        if s.route == "quad":
            E = sum(_part(rng, s.n, s.Ntot, part, False, "varied") for part in PARTS)
        else:
            A = rng.standard_normal((s.Ntot, s.Ntot))
            E = A + A.T
        E *= size * np.abs(np.linalg.eigvalsh(H0)).max() / np.abs(np.linalg.eigvalsh(E)).max()
        out[:, :, i] = H0 + E
        assert np.array_equal(out[:, :, i], out[:, :, i].T) and (s.route != "quad" or t4_structure(out[:, :, i]))
    return out


def problem(jq, s, objFuncType, nsteps=NSTEPS, nmember=3):
    """(params, pcof, drifts[Ntot, Ntot, nmember], directions[ncoeff, NDIR]) of a case; the same numbers for every caller"""
    rng = np.random.default_rng(61000 + 1000 * s.Ntot + 100 * s.N + 10 * s.Nc + s.m)
    if s.route == "quad":
        p, pcof = subsystem_problem(jq, rng, s.n, s.Ntot, s.N, s.Nc, s.m, "varied", nsteps, objFuncType)
    else:
        p, pcof = block_band_problem(jq, rng, s.Ntot, s.N, 0, [1] * s.Nc, nsteps, s.m, objFuncType)
    H = member_drifts(rng, s, np.asarray(p.Hconst, dtype=np.float64), nmember)
    D = rng.standard_normal((pcof.size, NDIR))
    return p, pcof, H, D


_cache = {}


def case(jq, s, objFuncType):
    """problem, members, directions and the CPU reference of a case, computed once and shared (never modified) by the tests that use it:
    (params, pcof, drifts, D, refs[j] = dict hv_infid, hv_leak, hv of direction j, members[j] = the members' own dicts, oracle sums)"""
    key = (s, objFuncType)
    if key not in _cache:
        p, pcof, H, D = problem(jq, s, objFuncType)
        ref = DR.DriftHessianReference(p, H, WEIGHTS)
        members = [ref.member_hvps(pcof, D[:, j]) for j in range(NDIR)]
        refs = []
        for mem in members:
            hv = sum(w * r["hv"] for w, r in zip(WEIGHTS, mem))
            hvi = sum(w * r["hv_infid"] for w, r in zip(WEIGHTS, mem))
            refs.append(dict(hv=hv, hv_infid=hvi, hv_leak=hv - hvi) if objFuncType != 1 else dict(hv=hv, hv_infid=hv, hv_leak=np.zeros(pcof.size)))
        _cache[key] = (p, pcof, H, D, refs, members, DR.weighted_oracle(p, pcof, H, WEIGHTS))
    return _cache[key]
