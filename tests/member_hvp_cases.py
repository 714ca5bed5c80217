"""The cases of jq_eval_f_g_grad_members_hvp that tests/test_gpu_member_hvp.py runs on the device and tests/test_member_hvp_host.py holds
against the oracle alone (they must discriminate: every member matters, the mixes matter, and a mix belongs to ITS member and is not
its transpose).

Shapes, weights, step count, chunk length, directions, problems and member drifts are those of tests/drift_hvp_cases.py (imported, not
copied).  On top of them every member gets a control mix eye(Nc) + 0.05 standard_normal((Nc, Nc)), drawn in member order from
default_rng(71000 + 1000 Ntot + 100 N + 10 Nc + m).

The reference needs no oracle code of its own: a member with mix C and drift H is the plain problem with Hsym'_k = sum_l C[l, k] Hsym_l,
Hanti'_k = sum_l C[l, k] Hanti_l and Hconst = H (mixed_params of tests/test_gpu_member_batch.py), so the reference is
sum_i w_i HessianReference(mixed_params(p, C_i, H_i)).hvp(pcof, d) next to sum_i w_i Oracle(mixed_params(p, C_i, H_i)).traceobjgrad(pcof)."""
import numpy as np

import hessian_reference as HR
from drift_hvp_cases import (CHUNK, KERNEL_FAMILY, NDIR, NSTEPS, OBJ_TYPES, SHAPES, WEIGHTS, Shape, image_stride, kernel_object,  # noqa: F401
                             kernel_size, member_drifts, problem, shape_id)
from test_gpu_member_batch import mixed_params

NMEMBER = 3


def member_mixes(s, nmember=NMEMBER):
    """[Nc, Nc, nmember] mixes of a shape, in member order"""
    rng = np.random.default_rng(71000 + 1000 * s.Ntot + 100 * s.N + 10 * s.Nc + s.m)
    out = np.zeros((s.Nc, s.Nc, nmember), order="F")
    for i in range(nmember):
        out[:, :, i] = np.eye(s.Nc) + 0.05 * rng.standard_normal((s.Nc, s.Nc))
    return out


def reference(p, pcof, D, mixes, drifts, weights):
    """(refs[j] = dict hv, hv_infid, hv_leak of direction j as the library returns them, members[j] = the members' own dicts, unweighted,
    orc = the oracle's weighted sums: dict infidelity, leak, totalgrad, infidelgrad).  mixes: [Nc, Nc, n]; drifts: [Ntot, Ntot, n] or None
    (the problem's own drift for every member)."""
    from oracle.oracle import Oracle
    n, ncoeff = mixes.shape[2], pcof.size
    probs = [mixed_params(p, mixes[:, :, i], None if drifts is None else drifts[:, :, i]) for i in range(n)]
    hrefs = [HR.HessianReference(q) for q in probs]
    members = [[r.hvp(pcof, D[:, j]) for r in hrefs] for j in range(D.shape[1])]
    refs = []
    for mem in members:
        hv = sum(w * r["hv"] for w, r in zip(weights, mem))
        hvi = sum(w * r["hv_infid"] for w, r in zip(weights, mem))
        refs.append(dict(hv=hv, hv_infid=hvi, hv_leak=hv - hvi) if p.objFuncType != 1 else dict(hv=hv, hv_infid=hv, hv_leak=np.zeros(ncoeff)))
    orc = dict(infidelity=0.0, leak=0.0, totalgrad=np.zeros(ncoeff), infidelgrad=np.zeros(ncoeff))
    for w, q in zip(weights, probs):
        r = Oracle(q).traceobjgrad(pcof)
        orc["infidelity"] += float(w) * r["primaryobjf"]
        orc["leak"] += float(w) * r["secondaryobjf"]
        orc["totalgrad"] += float(w) * r["totalgrad"]
        orc["infidelgrad"] += float(w) * r["infidelgrad"]
    return refs, members, orc


_cache = {}


def case(jq, s, objFuncType, drifts=True):
    """problem, members, directions and the CPU reference of a case, computed once and shared (never modified) by the tests that use it:
    (params, pcof, drifts or None, mixes, D, refs, members, orc); drifts=False: the members differ in their mixes alone"""
    key = (s, objFuncType, drifts)
    if key not in _cache:
        p, pcof, H, D = problem(jq, s, objFuncType)
        Cm = member_mixes(s)
        Hm = H if drifts else None
        _cache[key] = (p, pcof, Hm, Cm, D) + reference(p, pcof, D, Cm, Hm, WEIGHTS)
    return _cache[key]
