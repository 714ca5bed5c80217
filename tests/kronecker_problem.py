"""Random d1 x d2 x d3 Kronecker problems for the structure-embedding tests (tests/test_gpu_round2.py, tests/test_gpu_batch_twin.py)."""
import numpy as np


def random_kronecker_problem(jq, dims, N):
    """(params, pcof, rng): dense blocks on the fastest factor, diagonal couplings of the other two; three controls, objFuncType 3,
    Neumann solver with m = 3, 14 time steps.  rng (seeded by the level count) is handed back for the caller's ensemble."""
    d1, d2, d3 = dims
    Ntot = d1 * d2 * d3
    rng = np.random.default_rng(77 + Ntot)
    def op(anti, parts):
        a = np.zeros((Ntot, Ntot))
        if parts & 1:       # fastest factor: dense d1 x d1 blocks (different per block)
            for b in range(0, Ntot, d1):
                blk = rng.standard_normal((d1, d1))
                a[b:b + d1, b:b + d1] = blk - blk.T if anti else blk + blk.T
        for stride, bit, period in ((d1, 2, d1 * d2), (d1 * d2, 4, Ntot)):
            if parts & bit:
                for i in range(Ntot - stride):
                    if i // period != (i + stride) // period:
                        continue
                    a[i, i + stride] = rng.standard_normal()
                    a[i + stride, i] = -a[i, i + stride] if anti else a[i, i + stride]
        return a
    Nc = 3
    Hs = [op(False, (7, 2, 4)[q]) for q in range(Nc)]
    Ha = [op(True, (7, 2, 4)[q]) for q in range(Nc)]
    H0 = op(False, 7)
    scale = 2.0 / max(1.0, max(np.abs(np.linalg.eigvalsh(h)).max() for h in Hs + [H0]))
    nsteps, m = 14, 3
    U0 = np.linalg.qr(rng.standard_normal((Ntot, N)))[0]
    Ut = np.linalg.qr(rng.standard_normal((Ntot, N)) + 1j * rng.standard_normal((Ntot, N)))[0]
    p = jq.objparams([N], [Ntot - N], 1.3, nsteps, Uinit=U0, Utarget=Ut, Cfreq=rng.standard_normal((Nc, 2)), Rfreq=np.zeros(Nc),
                     Hconst=H0 * scale, Hsym_ops=[h * scale for h in Hs], Hanti_ops=[h * scale for h in Ha], objFuncType=3,
                     linear_solver=jq.lsolver_object(max_iter=m))
    p.wmat_real = rng.random(Ntot) * (np.arange(Ntot) >= N)
    pcof = 0.3 * rng.standard_normal(2 * Nc * 2 * 4)
    return p, pcof, rng
