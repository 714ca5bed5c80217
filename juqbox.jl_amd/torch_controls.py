"""PyTorch autograd over the sampled-controls entry points (the only module of the package that imports torch).

  SampledObjective.apply(pq, params, wa, nodes=None, weights=None, shift=None)
      the objective of a table of control values pq[2 Ncoupled, 2 nsteps + 1] on the time grid (traceobjgrad_samples; with nodes and
      weights the risk-neutral one, eval_f_g_grad_samples: infidelity + leak) as a 0-dimensional float64 tensor on pq's device, with
      dJ/dpq as its backward.  Whatever produced pq -- a piecewise-constant pulse through repeat_interleave, an envelope, a filter, a
      torch.nn.Module -- is differentiated by torch; the time loops run in the library.

The samples go through host memory (the library's entry points take host pointers); a device-pointer variant is not offered."""
import numpy as np
import torch

from .evalobjgrad import traceobjgrad_samples
from .ipopt_interface import eval_f_g_grad_samples


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
