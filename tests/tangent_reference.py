"""CPU reference for the tangent (Jacobian-vector product) of the discrete forward map, from the UNCHANGED oracle.

The derivative of a scheme built from products and truncated series of K(t), S(t) is that same scheme applied to the block-triangular
operators [[M, 0], [Md, M]] (Md: the derivative of M along the direction d).  So the oracle, forward only, on the 2 Ntot problem

    Hconst'  = I2 x Hconst
    controls = I2 x Hsym_k, I2 x Hanti_k  (k < Nc)  and  E21 x Hsym_k, E21 x Hanti_k  (the second half; E21 = [[0, 0], [1, 0]])
    Cfreq'   = Cfreq stacked twice          pcof' = [pcof; d]          Uinit' = [Uinit; 0]
    wmat_real' = [[0, D], [D, 0]] (dense), D = diag(wmat_real)

returns the final state [V; Vd] exactly, and its own secondaryobjf -- 2 Re(V' D Vd) integrated -- equals d(secondaryobjf).  The
oracle's forward path never uses the symmetry of an operator.  Uncoupled controls (Hunc_ops) are doubled the same way.
"""
import types

import numpy as np

from oracle.oracle import Oracle

_I2 = np.eye(2)
_E21 = np.array([[0.0, 0.0], [1.0, 0.0]])


def doubled_params(params):
    """the 2 Ntot problem whose forward sweep carries (state, tangent); pcof' = [pcof; d]"""
    p = params
    Ntot, N = int(p.Ntot), int(p.N)
    nunc = int(getattr(p, "Nunc", 0))
    q = types.SimpleNamespace()
    q.Ntot, q.N, q.nsteps, q.T, q.Nfreq = 2 * Ntot, N, int(p.nsteps), float(p.T), int(p.Nfreq)
    q.objFuncType, q.linear_solver, q.use_sparse = p.objFuncType, p.linear_solver, False
    q.Hconst = np.kron(_I2, np.asarray(p.Hconst, dtype=np.float64))
    if nunc:
        ops = [np.asarray(h, dtype=np.float64) for h in p.Hunc_ops[:nunc]]
        q.Nunc, q.Ncoupled = 2 * nunc, 0
        q.Hunc_ops = [np.kron(_I2, h) for h in ops] + [np.kron(_E21, h) for h in ops]
        q.isSymm = list(p.isSymm[:nunc]) * 2
        q.Rfreq = np.concatenate([np.asarray(p.Rfreq[:nunc], dtype=np.float64)] * 2)
        q.Hsym_ops, q.Hanti_ops = [], []
        nctrl = nunc
    else:
        nctrl = int(p.Ncoupled)
        hs = [np.asarray(h, dtype=np.float64) for h in p.Hsym_ops]
        ha = [np.asarray(h, dtype=np.float64) for h in p.Hanti_ops]
        q.Nunc, q.Ncoupled = 0, 2 * nctrl
        q.Hsym_ops = [np.kron(_I2, h) for h in hs] + [np.kron(_E21, h) for h in hs]
        q.Hanti_ops = [np.kron(_I2, h) for h in ha] + [np.kron(_E21, h) for h in ha]
    cf = np.asarray(p.Cfreq, dtype=np.float64)[:nctrl, :]
    q.Cfreq = np.vstack([cf, cf])
    z = np.zeros((Ntot, N))
    q.Uinit = np.vstack([np.asarray(p.Uinit, dtype=np.float64), z])
    q.Utarget_r = np.vstack([np.asarray(p.Utarget_r, dtype=np.float64), z])
    q.Utarget_i = np.vstack([np.asarray(p.Utarget_i, dtype=np.float64), z])
    w = np.asarray(p.wmat_real, dtype=np.float64)
    if w.ndim != 1:
        raise ValueError("tangent_reference: Diagonal leakage weights (a vector wmat_real) only")
    D = np.diag(w)
    q.wmat_real = np.block([[np.zeros_like(D), D], [D, np.zeros_like(D)]])
    q.wmat_imag = None
    return q


def trace_s(U, params):
    """s = tr(Vtg' U)/N of tracefidcomplex (src/evalobjgrad.jl:2078-2084) for U = vr - i vi"""
    T = np.asarray(params.Utarget_r, dtype=np.float64) + 1j * np.asarray(params.Utarget_i, dtype=np.float64)
    return np.sum(T * np.conj(U)) / params.N


class TangentReference:
    """tangent(pcof, d) of one problem; the doubled oracle is built once"""

    def __init__(self, params):
        self.params = params
        self.oracle = Oracle(doubled_params(params))

    def tangent(self, pcof, d):
        """dict: V, W (complex [Ntot, N]: the final state vr - i vi and its derivative along d), primaryobjf, d_primary, d_secondary"""
        p = self.params
        pcof, d = np.asarray(pcof, dtype=np.float64).ravel(), np.asarray(d, dtype=np.float64).ravel()
        assert pcof.size == d.size
        r = self.oracle.traceobjgrad(np.concatenate([pcof, d]), evaladjoint=False, final_state=True)
        fs = r["final_state"]
        U = fs[:, :, 0] - 1j * fs[:, :, 1]
        n = int(p.Ntot)
        V, W = U[:n], U[n:]
        s, sd = trace_s(V, p), trace_s(W, p)
        return dict(V=V, W=W, primaryobjf=1.0 - abs(s) ** 2, d_primary=-2.0 * np.real(np.conj(s) * sd), d_secondary=r["secondaryobjf"])


def tangent(params, pcof, d):
    return TangentReference(params).tangent(pcof, d)
