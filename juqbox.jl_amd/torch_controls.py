"""PyTorch autograd over the sampled-controls entry points (the only module of the package that imports torch).

  SampledObjective.apply(pq, params, wa, nodes=None, weights=None, shift=None)
      the objective of a table of control values pq[2 Ncoupled, 2 nsteps + 1] on the time grid (traceobjgrad_samples; with nodes and
      weights the risk-neutral one, eval_f_g_grad_samples: infidelity + leak) as a 0-dimensional float64 tensor on pq's device, with
      dJ/dpq as its backward.  Whatever produced pq -- a piecewise-constant pulse through repeat_interleave, an envelope, a filter, a
      torch.nn.Module -- is differentiated by torch; the time loops run in the library.

  SampledMembersObjective.apply(pq, params, wa, weights, Hconsts, ctrl_mix)
      the weighted infidelity + leak of a member ensemble under ONE table (eval_f_g_grad_samples_members: members that differ in their
      drift, in a real mix of the controls, or in both) as a 0-dimensional tensor with dJ/dpq -- the robust objective of such a pulse.

  SampledBatchObjective.apply(pqs, params, wa)
      the objectives of ntab tables pqs[ntab, 2 Ncoupled, 2 nsteps + 1] in one library call (traceobjgrad_samples_batch) as a tensor of
      ntab values; its backward contracts grad_output with the per-table gradients.

  sampled_hessvec(fn, theta, v, params, wa, nodes=None, weights=None, shift=None)
      the derivative along v of the gradient of J(fn(theta)): the library's Hessian-vector product in sample space
      (eval_f_g_grad_samples_hvp) between torch.func.jvp and vjp of fn, plus the curvature of fn against the sample gradient.

The samples go through host memory (the library's entry points take host pointers); a device-pointer variant is not offered."""
import numpy as np
import torch

from .evalobjgrad import traceobjgrad_samples, traceobjgrad_samples_batch
from .ipopt_interface import eval_f_g_grad_samples, eval_f_g_grad_samples_hvp, eval_f_g_grad_samples_members


class SampledObjective(torch.autograd.Function):
    """J(pq) = objfv of traceobjgrad_samples (no Tikhonov term), or sum_i w_i (infidelity_i + leak_i) over quadrature nodes."""

    @staticmethod
    def forward(ctx, pq, params, wa, nodes=None, weights=None, shift=None):
        if not isinstance(pq, torch.Tensor) or pq.dtype != torch.float64:
            raise TypeError("SampledObjective: pq must be a float64 tensor")
        if (nodes is None) != (weights is None):
            raise ValueError("SampledObjective: give nodes and weights together")
        table = pq.detach().to("cpu").numpy()
        want_grad = bool(ctx.needs_input_grad[0])
        if nodes is None:
            r = traceobjgrad_samples(table, params, wa, want_grad)
            value, grad = r[0], (r[1] if want_grad else None)
        else:
            r = eval_f_g_grad_samples(table, params, wa, nodes, weights, shift, want_grad)
            value = r["infidelity"] + r["leak"]
            grad = r["infid_grad"] + r["leak_grad"] if want_grad else None
        if want_grad:
            ctx.save_for_backward(torch.from_numpy(np.ascontiguousarray(grad)).to(pq.device))
        return torch.tensor(float(value), dtype=torch.float64, device=pq.device)

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return grad_output * grad, None, None, None, None, None


class SampledMembersObjective(torch.autograd.Function):
    """J(pq) = sum_g w_g (infidelity_g + leak_g) over the members of eval_f_g_grad_samples_members (Hconsts or ctrl_mix may be None)."""

    @staticmethod
    def forward(ctx, pq, params, wa, weights, Hconsts=None, ctrl_mix=None):
        if not isinstance(pq, torch.Tensor) or pq.dtype != torch.float64:
            raise TypeError("SampledMembersObjective: pq must be a float64 tensor")
        table = pq.detach().to("cpu").numpy()
        want_grad = bool(ctx.needs_input_grad[0])
        r = eval_f_g_grad_samples_members(table, params, wa, weights, Hconsts=Hconsts, ctrl_mix=ctrl_mix, compute_adjoint=want_grad)
        if want_grad:
            ctx.save_for_backward(torch.from_numpy(np.ascontiguousarray(r["infid_grad"] + r["leak_grad"])).to(pq.device))
        return torch.tensor(float(r["infidelity"] + r["leak"]), dtype=torch.float64, device=pq.device)

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return grad_output * grad, None, None, None, None, None


class SampledBatchObjective(torch.autograd.Function):
    """J_i = objfv of traceobjgrad_samples(pqs[i]) for the ntab tables of pqs[ntab, 2 Ncoupled, 2 nsteps + 1], in one library call."""

    @staticmethod
    def forward(ctx, pqs, params, wa):
        if not isinstance(pqs, torch.Tensor) or pqs.dtype != torch.float64 or pqs.dim() != 3:
            raise TypeError("SampledBatchObjective: pqs must be a float64 tensor [ntab, 2 Ncoupled, 2 nsteps + 1]")
        tables = pqs.detach().to("cpu").numpy()
        want_grad = bool(ctx.needs_input_grad[0])
        r = traceobjgrad_samples_batch(tables, params, wa, want_grad)
        if want_grad:
            ctx.save_for_backward(torch.from_numpy(np.ascontiguousarray(r[1])).to(pqs.device))
        return torch.from_numpy(np.ascontiguousarray(r[0])).to(pqs.device)

    @staticmethod
    def backward(ctx, grad_output):
        (grads,) = ctx.saved_tensors
        return grad_output[:, None, None] * grads, None, None


def sampled_hessvec(fn, theta, v, params, wa, nodes=None, weights=None, shift=None):
    """The derivative, along v, of the gradient of J(fn(theta)) with respect to theta, for a differentiable theta -> pq = fn(theta) (a
    float64 tensor in the shape of a sample table) and J the objective of SampledObjective:

        d/d eps grad_theta J(fn(theta + eps v)) at eps = 0  =  Jfn' (Hs (Jfn v))  +  d/d eps [ Jfn(theta + eps v)' G ] at eps = 0

    with Jfn the Jacobian of fn at theta, G the library's sample gradient at fn(theta) held constant, and Hs u the library's exact
    Hessian-vector product in sample space (eval_f_g_grad_samples_hvp).  Computed as
        u = Jfn v                                  torch.func.jvp of fn,
        G, Hs u                                    ONE library call,
        Jfn' (Hs u)                                torch.func.vjp of fn,
        the second term                            torch.func.jvp of theta -> vjp_fn(theta)(G): the curvature of fn, zero for a linear fn.
    fn must be composed of torch operations torch.func can differentiate twice.  Returns a tensor in the shape of theta.

    SampledObjective is deliberately NOT twice differentiable through autograd: double backward would need Hs' w, the library gives
    Hs w, the two differ at truncation level of the Neumann series (traceobjgrad_hvp), and this package never symmetrises silently.
    This function needs Hs w only, so it returns exactly the derivative of the gradient that SampledObjective's backward returns."""
    if not isinstance(theta, torch.Tensor) or theta.dtype != torch.float64:
        raise TypeError("sampled_hessvec: theta must be a float64 tensor")
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float64 or v.shape != theta.shape:
        raise TypeError("sampled_hessvec: v must be a float64 tensor in the shape of theta")
    if (nodes is None) != (weights is None):
        raise ValueError("sampled_hessvec: give nodes and weights together")
    theta, v = theta.detach(), v.detach()
    pq, u = torch.func.jvp(fn, (theta,), (v,))
    if nodes is None:
        r = eval_f_g_grad_samples_hvp(pq.to("cpu").numpy(), u.to("cpu").numpy(), params, wa, _who="sampled_hessvec")
    else:
        r = eval_f_g_grad_samples_hvp(pq.to("cpu").numpy(), u.to("cpu").numpy(), params, wa, nodes, weights, shift, _who="sampled_hessvec")
    G = torch.from_numpy(np.ascontiguousarray(r["infid_grad"] + r["leak_grad"])).to(theta.device)
    Hu = torch.from_numpy(np.ascontiguousarray((r["hv_infid"] + r["hv_leak"])[:, :, 0])).to(theta.device)

    def pullback(th, w):
        return torch.func.vjp(fn, th)[1](w)[0]

    curvature = torch.func.jvp(lambda th: pullback(th, G), (theta,), (v,))[1]
    return pullback(theta, Hu) + curvature
