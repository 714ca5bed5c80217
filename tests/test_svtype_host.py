"""CPU: continuation adjoints (params.sv_type 2 / 3, params.dVds; src/evalobjgrad.jl:312-319, :815-844, :1492-1520) -- the reference
constructions that tests/test_gpu_svtype.py holds the kernels to, checked here oracle against oracle, the Python mirror's semantics,
the pFidType refusal and the Julia shim (lexically: there is no Julia in the image).

The oracle only knows sv_type 1, but type 1 with a chosen target reproduces the others.  With V the final state, s_X = tr(V' X)/N
(linear in X) and lambda(T) = s conj(X)/N:  type 1 = s_T conj(T)/N, type 2 = s_T conj(D)/N, type 3 = s_D conj(T)/N, where T is the target
and D = dVds.  The gradient is affine in lambda(T): g = L(lambda(T)) + l, with l the leakage-forcing part.

* Phase-aligned dVds (pins each type on its own): D' = D exp(i (arg s_T - arg s_D)) makes s_T / s_D' = rho > 0.  Then
  type 2 with dVds D' == type 1 with target sqrt(rho) D', and type 3 with dVds D' == type 1 with target T / sqrt(rho).
  (A global phase of the target never matters, so a complex scale cannot be used: hence the alignment.)
* Any dVds (pins the sum): with g(X) the type-1 total gradient for target X and l = (4 g(T) - g(2 T))/3,
  total_2 + total_3 = (g(T + D) - g(T - D))/2 + 2 l, and the project's type 4 (both terms in ONE sweep) = (g(T + D) - g(T - D))/2 + l.
The objective values are those of type 1 on the true target in every type.
"""
import copy
import os
import re

import numpy as np
import pytest
from conftest import ROOT, case_inputs, reference_pass

MIN_S = 1e-3      # the aligned constructions divide by |s_T| and |s_D|: precondition (asserted, never skipped)
SEED = 7          # D = randn + i randn from default_rng(SEED)


# ---- the reference constructions (shared with tests/test_gpu_svtype.py) -------------------------------------------------------------
def target_of(params):
    return np.asarray(params.Utarget_r) + 1j * np.asarray(params.Utarget_i)


def with_target(params, X):
    """a shallow copy of params whose target is X (the original is untouched)"""
    p = copy.copy(params)
    p.Utarget_r = np.asfortranarray(np.real(X).copy())
    p.Utarget_i = np.asfortranarray(np.imag(X).copy())
    return p


def random_dvds(params, seed=SEED):
    rng = np.random.default_rng(seed)
    shp = (params.Ntot, params.N)
    return rng.standard_normal(shp) + 1j * rng.standard_normal(shp)


def oracle_eval(pcof):
    """evaluate(params) -> dict(totalgrad, infidelgrad, leakgrad, ...) by the CPU oracle's traceobjgrad (sv_type 1)"""
    from oracle.oracle import Oracle
    return lambda p: Oracle(p).traceobjgrad(pcof)


def oracle_ensemble_eval(pcof, nodes, weights, shift):
    """the same for eval_f_g_grad: totalgrad = last_infidelity_grad + last_leak_grad"""
    from oracle.oracle import Oracle

    def ev(p):
        r = Oracle(p).eval_f_g_grad(pcof, nodes, weights, shift)
        return dict(totalgrad=r["last_infidelity_grad"] + r["last_leak_grad"], infidelgrad=r["last_infidelity_grad"],
                    leakgrad=r["last_leak_grad"], primaryobjf=r["last_infidelity"], secondaryobjf=r["last_leak"])
    return ev


def traces(params, pcof, D):
    """(s_T, s_D) at pcof: tracefidcomplex (src/evalobjgrad.jl:2078-2084) of the oracle's final state against the target and D"""
    from oracle.oracle import Oracle
    fs = Oracle(params).traceobjgrad(pcof, evaladjoint=False, final_state=True)["final_state"]
    V = fs[:, :, 0] - 1j * fs[:, :, 1]
    s = lambda X: np.trace(V.conj().T @ X) / params.N
    return s(target_of(params)), s(D)


def align(params, pcof, D):
    """(D', rho): D rotated so that s_T / s_D' = rho > 0"""
    sT, sD = traces(params, pcof, D)
    assert min(abs(sT), abs(sD)) > MIN_S, ("precondition of the aligned constructions: |s_T|, |s_D| away from zero", abs(sT), abs(sD))
    return D * np.exp(1j * (np.angle(sT) - np.angle(sD))), abs(sT) / abs(sD)


def leak_part(params, evaluate):
    """l = (4 g(T) - g(2 T))/3: what the leakage forcing alone contributes to the total gradient"""
    T = target_of(params)
    return (4.0 * evaluate(params)["totalgrad"] - evaluate(with_target(params, 2.0 * T))["totalgrad"]) / 3.0


def ref_type2(params, evaluate, Dp, rho):
    return evaluate(with_target(params, np.sqrt(rho) * Dp))


def ref_type3(params, evaluate, rho):
    return evaluate(with_target(params, target_of(params) / np.sqrt(rho)))


def ref_polar(params, evaluate, D):
    """(g(T + D) - g(T - D))/2 = L(lambda_2) + L(lambda_3), any D"""
    T = target_of(params)
    return 0.5 * (evaluate(with_target(params, T + D))["totalgrad"] - evaluate(with_target(params, T - D))["totalgrad"])


# ---- 1. the constructions, oracle against oracle ---------------------------------------------------------------------------------
CASES = ["swap02", "cnot2", "cnot2-leakieq"]


def _short(case):
    params, info, pcof, _ = case_inputs(case)
    return params, pcof


@pytest.mark.parametrize("case", CASES)
def test_preconditions_of_the_aligned_constructions(case):
    params, pcof = _short(case)
    sT, sD = traces(params, pcof, random_dvds(params))
    print("%s: |s_T| = %.3f  |s_D| = %.3f" % (case, abs(sT), abs(sD)))
    assert min(abs(sT), abs(sD)) > MIN_S


@pytest.mark.parametrize("case", CASES)
def test_sum_identity_agrees_with_the_aligned_constructions(case):
    """the two independent routes to total_2 + total_3 agree to the project's criterion: aligned D' through two type-1 runs with
    substituted targets, and the polarisation (g(T + D') - g(T - D'))/2 + 2 l"""
    params, pcof = _short(case)
    ev = oracle_eval(pcof)
    Dp, rho = align(params, pcof, random_dvds(params))
    r1, r2, r3 = ev(params), ref_type2(params, ev, Dp, rho), ref_type3(params, ev, rho)
    ell = leak_part(params, ev)
    lhs, rhs = r2["totalgrad"] + r3["totalgrad"], ref_polar(params, ev, Dp) + 2.0 * ell
    print("%s: sum identity rel %.2e, |l| = %.3e" % (case, np.linalg.norm(lhs - rhs) / np.linalg.norm(rhs), np.linalg.norm(ell)))
    assert reference_pass(lhs, rhs)
    # the substituted targets leave the leakage part alone ...
    assert reference_pass(r2["totalgrad"] - r2["infidelgrad"], r1["totalgrad"] - r1["infidelgrad"])
    assert reference_pass(r3["totalgrad"] - r3["infidelgrad"], r1["totalgrad"] - r1["infidelgrad"])
    if params.objFuncType != 1:      # ... which is the leakgrad the oracle returns separately, and l
        assert reference_pass(r2["leakgrad"], r1["leakgrad"]) and reference_pass(r3["leakgrad"], r1["leakgrad"])
        assert reference_pass(ell, r1["leakgrad"])


def test_aligned_constructions_are_the_derivatives_they_claim_to_be():
    """cnot2-leakieq returns infidelgrad on its own: type 2 is the gradient of -2 Re(conj(s_T0) s_D(alpha)), type 3 that of
    -2 Re(conj(s_D0) s_T(alpha)) (central differences, a few components; agreement ~1e-10 absolute, the unaligned ones are visibly off)"""
    params, pcof = _short("cnot2-leakieq")
    ev = oracle_eval(pcof)
    D = random_dvds(params)
    Dp, rho = align(params, pcof, D)
    sT0, sD0 = traces(params, pcof, Dp)
    g2, g3 = ref_type2(params, ev, Dp, rho)["infidelgrad"], ref_type3(params, ev, rho)["infidelgrad"]
    off = 0.0
    for k in (0, pcof.size // 2, pcof.size - 1):
        h = 1e-6 * max(1.0, abs(pcof[k]))
        e = np.zeros_like(pcof)
        e[k] = h
        (tp, dp), (tm, dm) = traces(params, pcof + e, Dp), traces(params, pcof - e, Dp)
        fd2 = -2.0 * np.real(np.conj(sT0) * (dp - dm)) / (2 * h)
        fd3 = -2.0 * np.real(np.conj(sD0) * (tp - tm)) / (2 * h)
        print("k=%d: type 2 %.12e fd %.12e | type 3 %.12e fd %.12e" % (k, g2[k], fd2, g3[k], fd3))
        scale = max(np.linalg.norm(g2, np.inf), np.linalg.norm(g3, np.inf))
        assert abs(g2[k] - fd2) < 1e-6 * scale and abs(g3[k] - fd3) < 1e-6 * scale      # (h^2 truncation + rounding / h of the differences)
        # without the alignment the substituted target is NOT type 2 (its global phase drops out, that of dVds does not)
        (_, up), (_, um) = traces(params, pcof + e, D), traces(params, pcof - e, D)
        off = max(off, abs(g2[k] - (-2.0 * np.real(np.conj(sT0) * (up - um)) / (2 * h))) / scale)
    assert off > 1e-3


# ---- 2. the Python mirror: objparams(...; dVds), change_target, set_adjoint_Sv_type ------------------------------------------------------
def _swap02_kwargs():
    import juqbox_jl_amd as jq
    p, _ = jq.cases.swap02()
    return p, dict(Uinit=p.Uinit, Utarget=target_of(p), Cfreq=p.Cfreq, Rfreq=p.Rfreq, Hconst=p.Hconst, Hsym_ops=p.Hsym_ops,
                   Hanti_ops=p.Hanti_ops)


def test_objparams_dvds_keyword():
    """src/evalobjgrad.jl:312-319: without dVds a copy of the target and sv_type 1; with it sv_type 2 and the size assert"""
    import juqbox_jl_amd as jq
    p0, kw = _swap02_kwargs()
    assert p0.sv_type == 1 and p0.pFidType == 2
    assert np.array_equal(p0.dVds_r, p0.Utarget_r) and np.array_equal(p0.dVds_i, p0.Utarget_i)
    assert p0.dVds_r is not p0.Utarget_r      # "make a copy to be safe"
    D = random_dvds(p0)
    p = jq.objparams(p0.Ne, p0.Ng, p0.T, p0.nsteps, dVds=D, **kw)
    assert p.sv_type == 2
    assert np.array_equal(p.dVds_r, D.real) and np.array_equal(p.dVds_i, D.imag)
    assert np.array_equal(p.Utarget_r, p0.Utarget_r)
    with pytest.raises(AssertionError):
        jq.objparams(p0.Ne, p0.Ng, p0.T, p0.nsteps, dVds=D[:, :-1], **kw)
    assert jq.objparams(p0.Ne, p0.Ng, p0.T, p0.nsteps, dVds=np.zeros((0, 0)), **kw).sv_type == 1      # length(dVds) == 0


def test_change_target_and_set_adjoint_sv_type():
    """src/evalobjgrad.jl:1492-1520: dVds follows the target only while sv_type == 1; set_adjoint_Sv_type! takes 1, 2, 3 (default 1)"""
    import juqbox_jl_amd as jq
    p, _ = _swap02_kwargs()
    T2 = target_of(p) * np.exp(0.3j) + 0.0
    jq.change_target(p, T2)
    assert np.array_equal(p.Utarget_r, T2.real) and np.array_equal(p.Utarget_i, T2.imag)
    assert np.array_equal(p.dVds_r, T2.real) and np.array_equal(p.dVds_i, T2.imag)
    jq.set_adjoint_Sv_type(p, 3)
    assert p.sv_type == 3
    T3 = target_of(p) * np.exp(-0.7j)
    jq.change_target(p, T3)
    assert np.array_equal(p.Utarget_r, T3.real) and np.array_equal(p.dVds_r, T2.real) and np.array_equal(p.dVds_i, T2.imag)
    jq.set_adjoint_Sv_type(p)
    assert p.sv_type == 1
    for bad in (0, 4, 5):      # (4 = both terms in one sweep is this project's addition: by assignment, not through the reference's setter)
        with pytest.raises(AssertionError):
            jq.set_adjoint_Sv_type(p, bad)
    with pytest.raises(AssertionError):
        jq.change_target(p, T3[:, :-1])
    T3[0, 0] = 99.0      # "make a copy to be safe"
    assert p.Utarget_r[0, 0] != 99.0


def test_pfidtype_other_than_2_is_refused_before_any_library_call():
    """DESIGN.md section 10 / INTEGRATION.md: "refused, JQ_EUNSUPPORTED" -- the struct is mutable, the check precedes the library"""
    import juqbox_jl_amd as jq
    p, _ = jq.cases.swap02()
    for bad in (1, 3, 4):
        p.pFidType = bad
        with pytest.raises(ValueError, match="JQ_EUNSUPPORTED"):
            jq.Working_Arrays_HIP(p, 8)
    wa = object.__new__(jq.Working_Arrays_HIP)      # an evaluation on an existing handle: sync_params refuses before it touches it
    wa.params, wa.handle = p, None
    with pytest.raises(ValueError, match="pFidType"):
        wa.sync_params()


# ---- 3. the C ABI and the Julia shim ----------------------------------------------------------------------------------------------------
def test_abi_6_null_handles():
    from juqbox_jl_amd import _lib
    L = _lib.load()
    assert L.jq_abi_version() == 6 == _lib.JQ_ABI_VERSION
    assert L.jq_set_sv_type(None, 2) == _lib.JQ_EINVAL
    assert L.jq_get_sv_type(None) == _lib.JQ_EINVAL
    assert L.jq_update_dvds(None, None, None) == _lib.JQ_EINVAL


def test_julia_sync_pushes_sv_type_and_dvds():
    """lexical (no Julia in the image): sync! refuses pFidType != 2 before its first ccall and pushes dVds / sv_type"""
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "hip_backend.jl")).read())
    body = re.search(r"function sync!\(wa::AbstractWorkingArraysHIP, params::objparams\)(.*?)\nend", txt, flags=re.S).group(1)
    for field in ("params.sv_type", "params.dVds_r", "params.dVds_i", "params.pFidType"):
        assert field in body, field
    assert ":jq_update_dvds" in body and ":jq_set_sv_type" in body
    refusal = body.index("params.pFidType")
    assert "error(" in body[refusal:body.index("\n", refusal)] and refusal < body.index("ccall(")
    assert body.index(":jq_update_dvds") < body.index(":jq_set_sv_type")      # dVds is in place when the type that reads it takes effect
    assert re.search(r"const JQ_ABI_VERSION = 6\b", txt)
