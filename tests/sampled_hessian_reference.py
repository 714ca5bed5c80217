"""CPU reference for Hessian-vector products in SAMPLE space (jq_eval_f_g_grad_samples_hvp), from the unchanged oracle.

The oracle knows spline coefficients only.  With one carrier frequency and D1 = 2 nsteps + 3 coefficients per spline the matrix
B = d pq / d pcof (spline_sample_matrix) has full ROW rank (tests/test_sampled_controls_host.py: sigma_min / sigma_max >= 0.35), so any
table S and any direction table V are S = B x and V = B d with x, d from lstsq.  The oracle's gradients of the objective x -> J(B x) are
B' G(S), and their derivatives along d are what tests/ensemble_hessian_reference.py computes:

    EnsembleHessianReference(p, nodes, weights, shift).hvp(x, d) = B' Hs V.

B' has full COLUMN rank, so Hs V = lstsq(B', .) is unique -- per sample entry -- and the same holds for the primal gradients.  Null-space
components of x and d (B has more columns than rows) do not enter: the oracle sees the controls B x only.

Tables are 2 Ncoupled x (2 nsteps + 1) arrays as the library takes them, flattened column-major where B acts."""
import numpy as np

import ensemble_hessian_reference as ER


def sample_grid(p):
    """the times of jq_sample_times restated: t accumulated like the forward sweep's table, half points t + dt / 2"""
    dt = p.T / p.nsteps
    t, out = 0.0, []
    for n in range(p.nsteps + 1):
        out.append(t)
        if n < p.nsteps:
            out.append(t + 0.5 * dt)
        t = t + dt
    return np.array(out)


def flat(table):
    return np.asarray(table, dtype=np.float64).ravel(order="F")


class SampledHessianReference:
    """gradients and Hessian-vector products with respect to the samples of one ensemble; B, its factorisations and the nodes' doubled
    oracles are built once"""

    def __init__(self, jq, p, nodes=(0.0,), weights=(1.0,), shift=None, times=None):
        assert int(p.Nfreq) == 1, "the rank condition needs one carrier frequency"
        self.p, self.nodes, self.weights, self.shift = p, [float(e) for e in nodes], [float(w) for w in weights], shift
        self.shape = (2 * int(p.Ncoupled), 2 * int(p.nsteps) + 1)
        self.ncoeff = 2 * int(p.Ncoupled) * (2 * int(p.nsteps) + 3)
        self.B = jq.spline_sample_matrix(p, self.ncoeff, sample_grid(p) if times is None else times)
        assert self.B.shape == (self.shape[0] * self.shape[1], self.ncoeff)
        self.ens = ER.EnsembleHessianReference(p, self.nodes, self.weights, shift)
        self.residual = 0.0      # the largest lstsq residual seen (relative)

    def coefficients(self, table):
        """x with B x = table (the minimum-norm one)"""
        s = flat(table)
        assert s.size == self.B.shape[0]
        x = np.linalg.lstsq(self.B, s, rcond=None)[0]
        self.residual = max(self.residual, np.abs(self.B @ x - s).max() / max(np.abs(s).max(), 1e-300))
        return x

    def unfold(self, g):
        """the sample-space vector G with B' G = g, as a table"""
        G = np.linalg.lstsq(self.B.T, g, rcond=None)[0]
        self.residual = max(self.residual, np.abs(self.B.T @ G - g).max() / max(np.abs(g).max(), 1e-300))
        return G.reshape(self.shape, order="F")

    def gradients(self, table, x=None):
        """dict: infid_grad, leak_grad (tables) as jq_eval_f_g_grad_samples returns them, and totalgrad"""
        x = self.coefficients(table) if x is None else x
        tg, ig = ER.weighted_oracle_gradients(self.p, x, self.nodes, self.weights, self.shift)
        if self.p.objFuncType != 1:
            return dict(totalgrad=self.unfold(tg), infid_grad=self.unfold(ig), leak_grad=self.unfold(tg - ig))
        return dict(totalgrad=self.unfold(tg), infid_grad=self.unfold(tg), leak_grad=np.zeros(self.shape))

    def hvp(self, table, direction, x=None, d=None):
        """dict: hv_infid, hv_leak (tables) as the library returns them, hv = the derivative of the total gradient"""
        x = self.coefficients(table) if x is None else x
        d = self.coefficients(direction) if d is None else d
        r = self.ens.hvp(x, d)
        return {k: self.unfold(r[k]) for k in ("hv", "hv_infid", "hv_leak")}


def piecewise_constant_table(rng, nf, nt, scale=0.4):
    """every control function a different random piecewise-constant pulse of 3 .. 5 segments, asymmetric in time
    (tests/test_gpu_sampled_controls.py, test_index_maps_with_an_asymmetric_piecewise_constant_pulse; short grids: as many cuts as fit)"""
    pq = np.zeros((nf, nt))
    for f in range(nf):
        ncuts = min(int(rng.integers(2, 5)), nt - 1)
        cuts = np.sort(rng.choice(np.arange(1, nt), size=ncuts, replace=False))
        for lo, hi in zip(np.r_[0, cuts], np.r_[cuts, nt]):
            pq[f, lo:hi] = scale * rng.standard_normal()
    assert not np.allclose(pq, pq[:, ::-1])
    return pq
