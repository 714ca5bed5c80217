"""Random problems whose operators FILL a block band of 16 x 16 tiles (tests/test_block_band_matrix.py, tests/test_gpu_block_band.py):
every block at block distance <= band is a full random block, nothing lies outside the band.  The generators of
tests/test_gpu_random.py reach the band kernels with one entry per off-diagonal block ("banded": a ladder operator) or with diagonal
ones ("od"); dense off-diagonal blocks keep a problem off the JQ_BW_OD and JQ_BW_T4 plans by construction."""
import numpy as np

TILE = 16


def tile_rows(Ntot):
    return (Ntot + TILE - 1) // TILE


def block_band(M):
    """jq_host_images.h block_band restated: the smallest block band width that contains every nonzero of M"""
    r, c = np.nonzero(M)
    return int(np.max(np.abs(r // TILE - c // TILE))) if r.size else 0


def band_operator(rng, Ntot, band, anti, mode=1):
    """mode 1: every block at block distance <= band; 0: the diagonal blocks only; 2: the band without its diagonal blocks.
    Mirrored symmetrically (anti: antisymmetrically); the last block row / column is ragged when Ntot is no multiple of 16."""
    NT = tile_rows(Ntot)
    a = np.zeros((Ntot, Ntot))
    for bi in range(NT):
        r0, r1 = TILE * bi, min(TILE * bi + TILE, Ntot)
        for bj in range(bi, min(NT, bi + band + 1)):
            if (mode == 0 and bj != bi) or (mode == 2 and bj == bi):
                continue
            c0, c1 = TILE * bj, min(TILE * bj + TILE, Ntot)
            blk = rng.standard_normal((r1 - r0, c1 - c0))
            if bi == bj:
                a[r0:r1, c0:c1] = blk - blk.T if anti else blk + blk.T
            else:
                a[r0:r1, c0:c1] = blk
                a[c0:c1, r0:r1] = -blk.T if anti else blk.T
    return a


def block_band_problem(jq, rng, Ntot, N, band, modes, nsteps, m, objFuncType):
    """(params, pcof) built like tests/test_gpu_random.py random_problem: random T in [1, 2), orthonormal Uinit, complex orthonormal
    target, two carrier frequencies, wmat_real on the guard levels, operators scaled to spectral radius 2, Neumann solver with m terms.
    H0 has the full band; modes[q] is the trace layout of control q (band_operator)."""
    T = 1.0 + rng.random()
    Nc, Nfreq = len(modes), 2
    H0 = band_operator(rng, Ntot, band, False)
    Hs = [band_operator(rng, Ntot, band, False, mode) for mode in modes]
    Ha = [band_operator(rng, Ntot, band, True, mode) for mode in modes]
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
