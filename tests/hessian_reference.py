"""CPU reference for the derivative of the adjoint gradient (Hessian-vector products), from the UNCHANGED oracle.

hv(alpha; d) = d/d eps totalgrad(alpha + eps d) at eps = 0 is the tangent of the oracle's own backward sweep.  Both sweeps are built
from products and truncated series of K(t), S(t), so their tangents are the same sweeps on block-triangular operators
[[M, 0], [Md, M]] (tests/tangent_reference.py); the oracle's adjoint applies K and S as they are (it uses K' = K, S' = -S and never
transposes), so on the 2 Ntot problem

    Hconst'  = I2 x Hconst
    controls = I2 x (Hsym_k, Hanti_k),  E21 x (Hsym_k, Hanti_k),  X x (Hsym_k, Hanti_k)      E21 = [[0, 0], [1, 0]], X = [[0, 1], [1, 0]]
    Cfreq'   = Cfreq stacked three times      pcof' = [pcof; d; 0]      Uinit' = [Uinit; 0]
    wmat_real' = I2 x diag(w), dense

the forward sweep carries [V; Vd] and the backward sweep [lambda; lambdad], each half with its own forcing W V, W Vd, provided
lambda'(T) = [s conj(T); sd conj(T)]/N.  The gradient block of the third control group is then tr-products of [V; Vd] with
X x H applied to [lambda; lambdad] = the derivative of the trace products of the plain gradient, and the controls are linear in the
coefficients.  The oracle forms lambda'(T) from ITS target, so three runs that differ in the target only are combined -- the gradient
is affine in lambda(T):

    A: [T; 0] -> lambda'(T) = [s conj(T); 0]/N      B: [0; T] -> [0; sd conj(T)]/N      C: 0 -> forcing only
    hv = (A + B - C) of the third coefficient block of totalgrad, hv_infid the same of infidelgrad.

The doubled problem's objective is not used.  Verified against Richardson-extrapolated central differences of the oracle's gradient in
tests/test_hvp_host.py.
"""
import types

import numpy as np

from oracle.oracle import Oracle

_I2 = np.eye(2)
_E21 = np.array([[0.0, 0.0], [1.0, 0.0]])
_X = np.array([[0.0, 1.0], [1.0, 0.0]])


def doubled_params(params, target):
    """the 2 Ntot problem with 3 Nc controls; target: "A", "B" or "C" (above)"""
    p = params
    Ntot, N, Nc = int(p.Ntot), int(p.N), int(p.Ncoupled)
    if int(getattr(p, "Nunc", 0)):
        raise ValueError("hessian_reference: coupled controls only")
    q = types.SimpleNamespace()
    q.Ntot, q.N, q.nsteps, q.T, q.Nfreq = 2 * Ntot, N, int(p.nsteps), float(p.T), int(p.Nfreq)
    q.objFuncType, q.linear_solver, q.use_sparse = p.objFuncType, p.linear_solver, False
    q.Hconst = np.kron(_I2, np.asarray(p.Hconst, dtype=np.float64))
    hs = [np.asarray(h, dtype=np.float64) for h in p.Hsym_ops[:Nc]]
    ha = [np.asarray(h, dtype=np.float64) for h in p.Hanti_ops[:Nc]]
    q.Nunc, q.Ncoupled = 0, 3 * Nc
    q.Hsym_ops = [np.kron(B, h) for B in (_I2, _E21, _X) for h in hs]
    q.Hanti_ops = [np.kron(B, h) for B in (_I2, _E21, _X) for h in ha]
    cf = np.asarray(p.Cfreq, dtype=np.float64)[:Nc, :]
    q.Cfreq = np.vstack([cf, cf, cf])
    z = np.zeros((Ntot, N))
    q.Uinit = np.vstack([np.asarray(p.Uinit, dtype=np.float64), z])
    tr, ti = np.asarray(p.Utarget_r, dtype=np.float64), np.asarray(p.Utarget_i, dtype=np.float64)
    q.Utarget_r = {"A": np.vstack([tr, z]), "B": np.vstack([z, tr]), "C": np.vstack([z, z])}[target]
    q.Utarget_i = {"A": np.vstack([ti, z]), "B": np.vstack([z, ti]), "C": np.vstack([z, z])}[target]
    w = np.asarray(p.wmat_real, dtype=np.float64)
    if w.ndim != 1:
        raise ValueError("hessian_reference: Diagonal leakage weights (a vector wmat_real) only")
    q.wmat_real = np.kron(_I2, np.diag(w))
    q.wmat_imag = None
    return q


class HessianReference:
    """hvp(pcof, d) of one problem; the three doubled oracles are built once"""

    def __init__(self, params):
        self.params = params
        self.oracles = [Oracle(doubled_params(params, t)) for t in "ABC"]

    def hvp(self, pcof, d):
        """dict: hv[ncoeff] = d(totalgrad) along d, hv_infid[ncoeff] = d(infidelgrad) along d"""
        pcof, d = np.asarray(pcof, dtype=np.float64).ravel(), np.asarray(d, dtype=np.float64).ravel()
        assert pcof.size == d.size
        n = pcof.size
        x = np.concatenate([pcof, d, np.zeros(n)])
        A, B, C = [o.traceobjgrad(x) for o in self.oracles]
        comb = lambda k: (A[k] + B[k] - C[k])[2 * n:]
        return dict(hv=comb("totalgrad"), hv_infid=comb("infidelgrad"))

    def jacobian(self, pcof):
        n = np.asarray(pcof).size
        return np.stack([self.hvp(pcof, e)["hv"] for e in np.eye(n)], axis=1)


def hvp(params, pcof, d):
    return HessianReference(params).hvp(pcof, d)
