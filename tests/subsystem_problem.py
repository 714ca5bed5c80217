"""Random 4 x 4 x n problems whose control q acts on subsystem q ONLY (tests/test_structured_matrix.py, tests/test_gpu_structured.py):
control 0 has nothing but 4 x 4 diagonal blocks, control 1 nothing but (i, i +- 4) couplings inside a 16-row block, control 2 nothing
but (i, i +- 16) couplings -- Hsym and Hanti alike -- which is Juqbox's usual set-up Hsym_ops = [a + a', b + b', c + c'] and what the
library's ORD / RIDE / SC specialisations are selected for (jq_host_images.h ctrl_per_subsystem).  The "t4" generators of
tests/test_gpu_random.py and tests/kronecker_problem.py give control 0 all three parts, so they never reach those instantiations."""
import numpy as np

PARTS = (1, 2, 4)      # JQ_T4_DIAG, JQ_T4_RTERMS, JQ_T4_MTERMS (jq_kernels.h): the part of the T4 image control q fills


def t4_mode(M):
    """jq_host_images.h t4_mode restated: the parts of the T4 image of M that are non-zero"""
    mode = 0
    for row, col in zip(*np.nonzero(M)):
        mode |= 1 if row // 4 == col // 4 else 2 if abs(row - col) == 4 else 4
    return mode


def t4_structure(M):
    """jq_host_images.h t4_structure restated: outside the 4 x 4 diagonal blocks only (i, i +- 4) inside a 16-row block and (i, i +- 16)"""
    for row, col in zip(*np.nonzero(M)):
        if row // 4 == col // 4:
            continue
        d = abs(int(row) - int(col))
        if not ((row // 16 == col // 16 and d == 4) or d == 16):
            return False
    return True


def _tridiagonal(rng, k, anti):
    """k x k with the two first off-diagonals only (a diagonal entry would belong to the 4 x 4 diagonal blocks), symmetric or antisymmetric"""
    a = np.zeros((k, k))
    for i in range(k - 1):
        a[i, i + 1] = rng.standard_normal()
    return a - a.T if anti else a + a.T


def _part(rng, n, Ntot, part, anti, flavour):
    """one part of a T4 image on Ntot <= 16 n levels"""
    if flavour == "uniform":      # a true Kronecker product on 16 n levels, cut to the first Ntot
        if part == 1:
            blk = rng.standard_normal((4, 4))
            a = np.kron(np.eye(4 * n), blk - blk.T if anti else blk + blk.T)
        elif part == 2:
            a = np.kron(np.eye(n), np.kron(_tridiagonal(rng, 4, anti), np.eye(4)))
        else:
            a = np.kron(_tridiagonal(rng, n, anti), np.eye(16))
        return np.ascontiguousarray(a[:Ntot, :Ntot])
    a = np.zeros((Ntot, Ntot))      # "varied": the same sparsity, independent entries
    if part == 1:
        for b in range(0, Ntot, 4):
            e = min(b + 4, Ntot)
            blk = rng.standard_normal((e - b, e - b))
            a[b:e, b:e] = blk - blk.T if anti else blk + blk.T
    else:
        d = 4 if part == 2 else 16
        for i in range(Ntot - d):
            if d == 4 and i // 16 != (i + 4) // 16:
                continue
            a[i, i + d] = rng.standard_normal()
            a[i + d, i] = -a[i, i + d] if anti else a[i, i + d]
    return a


def subsystem_problem(jq, rng, n, Ntot, N, Nc, m, flavour, nsteps, objFuncType):
    """(params, pcof) of a 4 x 4 x n problem, 16 (n - 1) < Ntot <= 16 n, with Nc <= 3 controls (n = 1 has no +- 16 couplings: Nc <= 2);
    control q fills part PARTS[q] only.  "uniform": true Kronecker products kron(I_4n, A), kron(I_n, kron(B, I_4)), kron(C, I_16) with A
    dense 4 x 4, B (4 x 4) and C (n x n) tridiagonal -- the plan reports s_uniform when Ntot = 16 n; "varied": the same sparsity with
    independent random entries.  Hconst has all three parts with independent random entries.  Everything else as
    tests/test_gpu_random.py random_problem: random T in [1, 2), orthonormal Uinit, complex orthonormal target, two carrier frequencies,
    weights on the guard levels, operators scaled to spectral radius 2, Neumann solver with m terms."""
    assert 16 * (n - 1) < Ntot <= 16 * n and flavour in ("uniform", "varied") and 1 <= Nc <= (3 if n > 1 else 2)
    T = 1.0 + rng.random()
    Nfreq = 2
    Hs = [_part(rng, n, Ntot, PARTS[q], False, flavour) for q in range(Nc)]
    Ha = [_part(rng, n, Ntot, PARTS[q], True, flavour) for q in range(Nc)]
    H0 = sum(_part(rng, n, Ntot, part, False, "varied") for part in (PARTS if n > 1 else PARTS[:2]))
    scale = 2.0 / max(1.0, max(np.abs(np.linalg.eigvalsh(h)).max() for h in Hs + [H0]))
    H0 *= scale
    Hs = [h * scale for h in Hs]
    Ha = [h * scale for h in Ha]
    U0 = np.linalg.qr(rng.standard_normal((Ntot, N)))[0]
    Ut = np.linalg.qr(rng.standard_normal((Ntot, N)) + 1j * rng.standard_normal((Ntot, N)))[0]
    Cfreq = rng.standard_normal((Nc, Nfreq))
    p = jq.objparams([N], [Ntot - N], T, nsteps, Uinit=U0, Utarget=Ut, Cfreq=Cfreq, Rfreq=np.zeros(Nc), Hconst=H0,
                     Hsym_ops=Hs, Hanti_ops=Ha, objFuncType=objFuncType, linear_solver=jq.lsolver_object(max_iter=m))
    p.wmat_real = rng.random(Ntot) * (np.arange(Ntot) >= N)
    D1 = int(rng.integers(3, 7))
    pcof = 0.3 * rng.standard_normal(2 * Nc * Nfreq * D1)
    return p, pcof
