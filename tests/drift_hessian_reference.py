"""CPU reference for the Hessian-vector products of a drift ensemble (jq_eval_f_g_grad_drifts_hvp):

    sum_i w_i HessianReference(p_i).hvp(pcof, d),

p_i a copy of the problem with Hconst = H_i, member i of the ensemble.  tests/hessian_reference.py does the work per member; the sibling
for ensembles over eps-nodes is tests/ensemble_hessian_reference.py.  hv_infid is the derivative of what jq_eval_f_g_grad_drifts returns
as infid_grad, hv_leak of leak_grad: for objFuncType 1 the total gradient's and zeros, else the infidelity part and total minus
infidelity."""
import copy

import numpy as np

import hessian_reference as HR


def member_params(params, H):
    """the problem of one member"""
    p = copy.copy(params)
    p.Hconst = np.array(H, dtype=np.float64, order="F", copy=True)
    return p


def _members(drifts):
    D = np.asarray(drifts, dtype=np.float64)
    return [D] if D.ndim == 2 else [D[:, :, i] for i in range(D.shape[2])]


class DriftHessianReference:
    """hvp(pcof, d) of one ensemble; the members' doubled oracles are built once"""

    def __init__(self, params, drifts, weights):
        self.two = params.objFuncType != 1
        self.weights = [float(w) for w in weights]
        mats = _members(drifts)
        assert len(mats) == len(self.weights)
        self.refs = [HR.HessianReference(member_params(params, H)) for H in mats]

    def member_hvps(self, pcof, d):
        """the members' own products, unweighted: a list of the dicts of HessianReference.hvp"""
        return [ref.hvp(pcof, d) for ref in self.refs]

    def hvp(self, pcof, d):
        """dict: hv_infid[ncoeff], hv_leak[ncoeff] as the library returns them, hv[ncoeff] = the weighted derivative of totalgrad"""
        n = np.asarray(pcof).size
        hv, hvi = np.zeros(n), np.zeros(n)
        for w, r in zip(self.weights, self.member_hvps(pcof, d)):
            hv += w * r["hv"]
            hvi += w * r["hv_infid"]
        if self.two:
            return dict(hv=hv, hv_infid=hvi, hv_leak=hv - hvi)
        return dict(hv=hv, hv_infid=hv, hv_leak=np.zeros(n))


def weighted_oracle(params, pcof, drifts, weights):
    """sum_i w_i of the unchanged oracle over the members: dict infidelity, leak, totalgrad, infidelgrad"""
    from oracle.oracle import Oracle
    n = np.asarray(pcof).size
    out = dict(infidelity=0.0, leak=0.0, totalgrad=np.zeros(n), infidelgrad=np.zeros(n))
    for H, w in zip(_members(drifts), weights):
        r = Oracle(member_params(params, H)).traceobjgrad(pcof)
        out["infidelity"] += float(w) * r["primaryobjf"]
        out["leak"] += float(w) * r["secondaryobjf"]
        out["totalgrad"] += float(w) * r["totalgrad"]
        out["infidelgrad"] += float(w) * r["infidelgrad"]
    return out


def weighted_oracle_gradients(params, pcof, drifts, weights):
    """sum_i w_i (totalgrad, infidelgrad) of the unchanged oracle over the members"""
    r = weighted_oracle(params, pcof, drifts, weights)
    return r["totalgrad"], r["infidelgrad"]
