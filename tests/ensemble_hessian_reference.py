"""CPU reference for the Hessian-vector products of a risk-neutral ensemble (jq_eval_f_g_grad_hvp):

    sum_i w_i HessianReference(p_i).hvp(pcof, d),

p_i a copy of the problem whose Hconst diagonal carries node i's shift, Hconst[j, j] += eps_i shift[j] (the reference's perturbation,
src/ipopt_interface.jl:41-44; shift None: its table 0.01 * 10^(j-2), j = 2 .. Ntot).  tests/hessian_reference.py does the work per node.
hv_infid is the derivative of what jq_eval_f_g_grad returns as infid_grad, hv_leak of leak_grad: for objFuncType 1 the total gradient's
and zeros, else the infidelity part and total minus infidelity."""
import copy

import numpy as np

import hessian_reference as HR


def default_shift(Ntot):
    return np.array([0.0] + [0.01 * 10.0 ** (j - 1) for j in range(1, int(Ntot))])


def node_params(params, eps, shift=None):
    """the problem of one quadrature node"""
    p = copy.copy(params)
    sh = default_shift(params.Ntot) if shift is None else np.asarray(shift, dtype=np.float64)
    H = np.array(params.Hconst, dtype=np.float64, order="F", copy=True)
    H[np.diag_indices(int(params.Ntot))] += float(eps) * sh
    p.Hconst = H
    return p


class EnsembleHessianReference:
    """hvp(pcof, d) of one ensemble; the nodes' doubled oracles are built once"""

    def __init__(self, params, nodes, weights, shift=None):
        self.two = params.objFuncType != 1
        self.weights = [float(w) for w in weights]
        assert len(nodes) == len(self.weights)
        self.refs = [HR.HessianReference(node_params(params, e, shift)) for e in nodes]

    def hvp(self, pcof, d):
        """dict: hv_infid[ncoeff], hv_leak[ncoeff] as the library returns them, hv[ncoeff] = the weighted derivative of totalgrad"""
        n = np.asarray(pcof).size
        hv, hvi = np.zeros(n), np.zeros(n)
        for w, ref in zip(self.weights, self.refs):
            r = ref.hvp(pcof, d)
            hv += w * r["hv"]
            hvi += w * r["hv_infid"]
        if self.two:
            return dict(hv=hv, hv_infid=hvi, hv_leak=hv - hvi)
        return dict(hv=hv, hv_infid=hv, hv_leak=np.zeros(n))


def weighted_oracle_gradients(params, pcof, nodes, weights, shift=None):
    """sum_i w_i (totalgrad, infidelgrad) of the unchanged oracle over the nodes"""
    from oracle.oracle import Oracle
    n = np.asarray(pcof).size
    tg, ig = np.zeros(n), np.zeros(n)
    for e, w in zip(nodes, weights):
        r = Oracle(node_params(params, e, shift)).traceobjgrad(pcof)
        tg += float(w) * r["totalgrad"]
        ig += float(w) * r["infidelgrad"]
    return tg, ig
