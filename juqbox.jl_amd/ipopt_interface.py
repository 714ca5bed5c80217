"""Mirror of the reference's optimiser glue around the hot path (src/ipopt_interface.jl:24-179):
eval_f_g_grad! (the risk-neutral ensemble = the multi-GPU sharding site) and the Ipopt callbacks
that consume its memoised results.  Ipopt itself stays outside (the callbacks have the reference's
signatures, so any L-BFGS driver can call them)."""
import numpy as np

from . import _lib
from .evalobjgrad import Working_Arrays_HIP, _directions, _drift_members, _f64, _direction_tables, _members, _pcof_columns, _ptr, _sample_table
from .setup_utils import tikhonov_grad, tikhonov_pen


def _dist():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist
    except Exception:  # torch absent: single process
        pass
    return None


def _shard_bounds_py(nquad, rank, world):
    """jq_shard_bounds restated (juqbox_hip.hip): shard `rank` owns [lo, hi); the first nquad % world shards get one more."""
    nquad, rank, world = int(nquad), int(rank), int(world)
    if nquad < 0 or world < 1 or not 0 <= rank < world:
        raise ValueError("shard_bounds: need nquad >= 0, world >= 1, 0 <= rank < world")
    base, rem = divmod(nquad, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_bounds(nquad, rank, world):
    """Contiguous block partition of the nquad ensemble samples over `world` ranks: the library's own
    jq_shard_bounds (the partition a multi-device handle uses for its GPUs), so ranks and devices shard alike.
    Pure host arithmetic: where the library cannot be loaded (CPU-only sharding tests on a box without the build) the
    same rule is evaluated in Python (tests/test_host_logic.py pins the two against each other)."""
    import ctypes
    try:
        L = _lib.load()
    except (ImportError, OSError, AttributeError):
        return _shard_bounds_py(nquad, rank, world)
    lo, hi = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(L.jq_shard_bounds(int(nquad), int(rank), int(world), ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def allreduce_sum_(vec):
    """ONE all-reduce (sum, fp64) of a packed host vector over all ranks (the gloo path of the CPU tests; the RCCL path
    keeps the vector on the device, _hip_shard_eval_dev).  No-op without an initialised process group."""
    dist = _dist()
    if dist is None or dist.get_world_size() == 1:
        return vec
    import torch
    t = torch.from_numpy(vec)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return vec


def _hip_shard_eval(pcof, params, wa, nodes, weights, shift, compute_adjoint):
    """Evaluate one shard of the ensemble on this rank's GPU: returns the packed partial sums
    [infidelity, leak, grad_infid(nCoeff), grad_leak(nCoeff)]."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("eval_f_g_grad: wa must be a Working_Arrays_HIP")
    L, h = _lib.load(), wa.handle
    n = pcof.size
    wa.sync_params()
    out2 = np.zeros(2)
    ig, lg = np.zeros(n), np.zeros(n)
    sh = _f64(shift) if shift is not None else None
    _lib.check(L.jq_eval_f_g_grad(h, _ptr(pcof), n, _ptr(nodes), _ptr(weights), nodes.size, _ptr(sh),
                                  1 if compute_adjoint else 0, _ptr(out2), _ptr(ig), _ptr(lg)), h)
    return np.concatenate([out2, ig, lg])


def _hip_shard_eval_dev(pcof, params, wa, nodes, weights, shift, compute_adjoint):
    """The same evaluation for a job with one process per GPU over RCCL: the library leaves the packed partial sums
    on the device (jq_eval_f_g_grad_dev), torch.distributed all-reduces them in place, ONE copy brings the result back.
    A rank without a shard contributes zeros."""
    import torch
    dist = _dist()
    L, h = _lib.load(), wa.handle
    n = pcof.size
    wa.sync_params()
    t = torch.empty(2 + 2 * n, dtype=torch.float64, device=torch.device("cuda", wa.device))      # on the HANDLE's device
    sh = _f64(shift) if shift is not None else None
    import ctypes
    _lib.check(L.jq_eval_f_g_grad_dev(h, _ptr(pcof), n, _ptr(nodes), _ptr(weights), nodes.size, _ptr(sh),
                                      1 if compute_adjoint else 0, ctypes.c_void_p(t.data_ptr())), h)
    import time
    t0 = time.perf_counter()                      # (jq_eval_f_g_grad_dev returned after its stream was synchronised)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    res = t.cpu().numpy()                         # waits for the collective
    wa.last_allreduce_ms = (time.perf_counter() - t0) * 1e3
    return res


def eval_f_g_grad(pcof, params, wa, nodes=(0.0,), weights=(1.0,), compute_adjoint=True, shift=None,
                  distributed=True, _shard_eval=_hip_shard_eval):
    """eval_f_g_grad!(pcof, params, wa, nodes, weights, compute_adjoint) -- src/ipopt_interface.jl:24-70.

    All quadrature nodes are evaluated concurrently on the GPU as one batch of N*nquad columns; with an
    initialised torch.distributed process group the nodes are block-partitioned over the ranks and the
    packed result [infidelity, leak, grad_infid(nCoeff), grad_leak(nCoeff)] is summed with ONE
    all-reduce.  Results land in params.last_* exactly like the reference (:27-31, :48-59, :67-68).
    `_shard_eval` exists for the CPU (gloo) tests of the sharding logic; the product default is the
    HIP library and there is no CPU fallback."""
    pcof = _f64(pcof)
    n = pcof.size
    nodes = _f64(nodes)
    weights = _f64(weights)
    if nodes.size != weights.size:
        raise ValueError("nodes and weights must have the same length")
    dist = _dist() if distributed else None
    lo, hi = 0, nodes.size
    if dist is not None and dist.get_world_size() > 1:
        lo, hi = shard_bounds(nodes.size, dist.get_rank(), dist.get_world_size())
    # reset the memoised gradients like the reference (src/ipopt_interface.jl:27-31): a call with compute_adjoint = false
    # must not leave the gradients of an older pcof behind the new last_pcof
    params.last_infidelity_grad = np.zeros(n)
    params.last_leak_grad = np.zeros(n) if params.objFuncType != 1 else np.zeros(0)
    packed = np.zeros(2 + 2 * n)
    if dist is not None and dist.get_backend() == "nccl" and _shard_eval is _hip_shard_eval and wa.num_devices == 1:
        # one process per GPU (also with a single rank): partial sums stay on the device for the RCCL all-reduce
        packed[:] = _hip_shard_eval_dev(pcof, params, wa, nodes[lo:hi].copy(), weights[lo:hi].copy(), shift, compute_adjoint)
    else:
        if hi > lo:
            packed[:] = _shard_eval(pcof, params, wa, nodes[lo:hi].copy(), weights[lo:hi].copy(), shift, compute_adjoint)
        if dist is not None and dist.get_world_size() > 1:
            if dist.get_backend() == "nccl":      # (multi-device handle under an RCCL process group: collective on a device copy)
                import torch
                t = torch.from_numpy(packed).to(torch.device("cuda", wa.device))
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
                packed[:] = t.cpu().numpy()
            else:
                allreduce_sum_(packed)
    params.last_pcof = pcof.copy()
    params.last_infidelity = float(packed[0])
    params.last_leak = float(packed[1])
    if compute_adjoint:
        params.last_infidelity_grad = packed[2:2 + n].copy()
        params.last_leak_grad = packed[2 + n:].copy() if params.objFuncType != 1 else np.zeros(0)
    params.lastTraceInfidelity = params.last_infidelity
    params.lastLeakIntegral = params.last_leak
    return params.last_infidelity, params.last_leak


def eval_f_g_grad_batch(pcofs, params, wa, nodes, weights, compute_adjoint=True, shift=None, per_node=False):
    """eval_f_g_grad for npcof control vectors over ONE set of quadrature nodes in one library call (jq_eval_f_g_grad_batch): multi-start
    optimisation, batched line searches, finite-difference checks of the risk-neutral gradient, population optimisers, robustness curves
    of several pulses.  Stormer-Verlet / Neumann on the row-lane and cooperative-quad kernels: launches of G vectors x nquad nodes, every
    workgroup reading the operator stream of its own vector; everywhere else one ensemble evaluation per vector inside the call
    (wa.plan_info()["pcof_batch"] says which).  Column i is bit-identical to eval_f_g_grad(pcofs[:, i], ...) on the same kernel variant
    and chunk length.

    pcofs: an ncoeff x npcof array (one vector per column) or a sequence of equal-length vectors.
    Returns (infidelity[npcof], leak[npcof], infid_grad[ncoeff, npcof], leak_grad[ncoeff, npcof]) -- the gradients are zero without
    compute_adjoint, leak_grad is 0 x npcof for objFuncType == 1 -- and with per_node=True also the array [4, nquad, npcof] of
    (objfv, primaryobjf, secondaryobjf, traceInfidelity) per node and vector (traceobj_sweep of every vector).
    params.last_* are left alone: they memoise ONE vector.  Shape errors raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("eval_f_g_grad_batch: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("eval_f_g_grad_batch: wa was allocated for a different objparams")
    ncoeff = int(wa.nCoeff)
    try:
        nodes, weights = np.asarray(nodes, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("eval_f_g_grad_batch: nodes and weights must be vectors of numbers (%s)" % e)
    if nodes.ndim != 1 or weights.ndim != 1 or nodes.size != weights.size:
        raise ValueError("eval_f_g_grad_batch: nodes and weights must be vectors of the same length, not %r and %r" % (nodes.shape, weights.shape))
    if nodes.size < 1:
        raise ValueError("eval_f_g_grad_batch: need at least one node")
    nodes, weights = _f64(nodes), _f64(weights)
    sh = None
    if shift is not None:
        if np.shape(shift) != (int(params.Ntot),):
            raise ValueError("eval_f_g_grad_batch: shift must have one entry per level, not shape %r" % (np.shape(shift),))
        sh = _f64(shift)
    P = _pcof_columns(pcofs, ncoeff)
    n, nq = P.shape[0], nodes.size
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out2 = np.zeros((n, 2))
    node_out = np.zeros((n, nq, 4)) if per_node else None
    ig = lg = None
    if compute_adjoint:
        ig, lg = np.zeros((n, ncoeff)), np.zeros((n, ncoeff))
    _lib.check(L.jq_eval_f_g_grad_batch(h, _ptr(P), ncoeff, n, _ptr(nodes), _ptr(weights), nq, _ptr(sh), 1 if compute_adjoint else 0,
                                        _ptr(out2), _ptr(ig), _ptr(lg), _ptr(node_out)), h)
    infid_grad = np.ascontiguousarray(ig.T) if compute_adjoint else np.zeros((ncoeff, n))
    if params.objFuncType == 1:
        leak_grad = np.zeros((0, n))
    else:
        leak_grad = np.ascontiguousarray(lg.T) if compute_adjoint else np.zeros((ncoeff, n))
    res = (out2[:, 0].copy(), out2[:, 1].copy(), infid_grad, leak_grad)
    if per_node:
        res += (np.ascontiguousarray(node_out.transpose(2, 1, 0)),)
    return res


def eval_f_g_grad_hvp(pcof, dirs, params, wa, nodes=(0.0,), weights=(1.0,), shift=None):
    """eval_f_g_grad over the quadrature nodes and the derivative of its two gradients along the columns of dirs in one library call
    (jq_eval_f_g_grad_hvp): Hessian-vector products of the risk-neutral objective, sum_i w_i d/d eps grad_i(pcof + eps dirs[:, j]) at
    eps = 0 -- exact derivatives of the gradients eval_f_g_grad returns, truncated Neumann series included (not symmetric at truncation
    level, traceobjgrad_hvp).  Ntot <= 6 with at most four controls: tangent-linear lane kernels, every node and every direction of a
    round in ONE launch per chunk (route "lane"); Ntot 9 .. 16 with at most four controls: the same on the tangent-linear row-lane
    kernels, four columns per wave (route "rowlane"); Ntot > 16 with the 4 x 4 x n structure in the handle's own plan (NT = 2 .. 6 blocks
    of 16 rows, e.g. cnot3) and at most four controls: the same on the tangent-linear quad-layout kernels (route "quad"; option quad=0
    switches it off); everything else traceobjgrad_hvp serves (Ntot 7, 8, Ntot > 16 without that structure, with NT = 7, 8 or through an
    embedded twin, options lane=0 / quad=0, more than four controls): the nodes one after the other (route "sequential";
    wa.plan_info()["ens_hvp"]["route"] says which).

    dirs: an ncoeff x ndir array (one direction per column) or a single vector.  Returns a dict: infidelity, leak, infid_grad[ncoeff],
    leak_grad[ncoeff] (as eval_f_g_grad leaves them in params.last_*; objFuncType == 1: infid_grad is the total gradient, leak_grad
    zeros), hv_infid[ncoeff, ndir], hv_leak[ncoeff, ndir] (objFuncType == 1: hv_infid is the derivative of the total gradient, hv_leak
    zeros).  No Tikhonov term; params.last_* are left alone.  Shape errors raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("eval_f_g_grad_hvp: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("eval_f_g_grad_hvp: wa was allocated for a different objparams")
    ncoeff = int(wa.nCoeff)
    try:
        p = np.asarray(pcof, dtype=np.float64)
        nodes, weights = np.asarray(nodes, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("eval_f_g_grad_hvp: pcof, nodes and weights must be vectors of numbers (%s)" % e)
    if p.ndim != 1 or p.size != ncoeff:
        raise ValueError("eval_f_g_grad_hvp: pcof has shape %r, expected (%d,) (wa.nCoeff)" % (p.shape, ncoeff))
    if nodes.ndim != 1 or weights.ndim != 1 or nodes.size != weights.size:
        raise ValueError("eval_f_g_grad_hvp: nodes and weights must be vectors of the same length, not %r and %r" % (nodes.shape, weights.shape))
    if nodes.size < 1:
        raise ValueError("eval_f_g_grad_hvp: need at least one node")
    D = _directions(dirs, ncoeff, "eval_f_g_grad_hvp")
    sh = None
    if shift is not None:
        if np.shape(shift) != (int(params.Ntot),):
            raise ValueError("eval_f_g_grad_hvp: shift must have one entry per level, not shape %r" % (np.shape(shift),))
        sh = _f64(shift)
    p, nodes, weights = _f64(p), _f64(nodes), _f64(weights)
    nd = D.shape[0]
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out2 = np.zeros(2)
    ig, lg = np.zeros(ncoeff), np.zeros(ncoeff)
    hvi, hvl = np.zeros((nd, ncoeff)), np.zeros((nd, ncoeff))
    _lib.check(L.jq_eval_f_g_grad_hvp(h, _ptr(p), ncoeff, _ptr(D), nd, _ptr(nodes), _ptr(weights), nodes.size, _ptr(sh), _ptr(out2), _ptr(ig),
                                      _ptr(lg), _ptr(hvi), _ptr(hvl)), h)
    return dict(infidelity=float(out2[0]), leak=float(out2[1]), infid_grad=ig, leak_grad=lg, hv_infid=np.ascontiguousarray(hvi.T),
                hv_leak=np.ascontiguousarray(hvl.T))


def eval_f_g_grad_samples(pq, params, wa, nodes=(0.0,), weights=(1.0,), shift=None, compute_adjoint=True):
    """eval_f_g_grad over the quadrature nodes for controls given as VALUES on the time grid (jq_eval_f_g_grad_samples): pq is the
    2 Ncoupled x (2 nsteps + 1) table of traceobjgrad_samples, node i the evaluation with Hconst + nodes[i] diag(shift), all nodes in one
    batch like eval_f_g_grad's (its kernel families, rounds and embedded twin).

    Returns a dict: infidelity, leak, and with compute_adjoint infid_grad, leak_grad in the shape of pq -- the weighted sums of the nodes'
    gradients with respect to every sample (objFuncType == 1: infid_grad is the total gradient, leak_grad zeros).  No Tikhonov term;
    params.last_* are left alone.  Shape errors raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("eval_f_g_grad_samples: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("eval_f_g_grad_samples: wa was allocated for a different objparams")
    tab, shape = _sample_table(pq, params, "eval_f_g_grad_samples")
    try:
        nodes, weights = np.asarray(nodes, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("eval_f_g_grad_samples: nodes and weights must be vectors of numbers (%s)" % e)
    if nodes.ndim != 1 or weights.ndim != 1 or nodes.size != weights.size:
        raise ValueError("eval_f_g_grad_samples: nodes and weights must be vectors of the same length, not %r and %r" % (nodes.shape, weights.shape))
    if nodes.size < 1:
        raise ValueError("eval_f_g_grad_samples: need at least one node")
    sh = None
    if shift is not None:
        if np.shape(shift) != (int(params.Ntot),):
            raise ValueError("eval_f_g_grad_samples: shift must have one entry per level, not shape %r" % (np.shape(shift),))
        sh = _f64(shift)
    nodes, weights = _f64(nodes), _f64(weights)
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out2 = np.zeros(2)
    ig = np.zeros(tab.size) if compute_adjoint else None
    lg = np.zeros(tab.size) if compute_adjoint else None
    _lib.check(L.jq_eval_f_g_grad_samples(h, _ptr(tab), shape[1], _ptr(nodes), _ptr(weights), nodes.size, _ptr(sh), 1 if compute_adjoint else 0,
                                          _ptr(out2), _ptr(ig), _ptr(lg)), h)
    r = dict(infidelity=float(out2[0]), leak=float(out2[1]))
    if compute_adjoint:
        r["infid_grad"], r["leak_grad"] = ig.reshape(shape, order="F"), lg.reshape(shape, order="F")
    return r


def eval_f_g_grad_samples_hvp(pq, dirs, params, wa, nodes=(0.0,), weights=(1.0,), shift=None, _who="eval_f_g_grad_samples_hvp"):
    """eval_f_g_grad_samples over the quadrature nodes and the derivative of its two gradients along direction tables in one library call
    (jq_eval_f_g_grad_samples_hvp): Hessian-vector products in sample space, sum_i w_i d/d eps grad_i(pq + eps dirs[:, :, j]) at eps = 0
    -- eval_f_g_grad_hvp with "coefficient" read as "sample".  The products are exact derivatives of the gradients eval_f_g_grad_samples
    returns, truncated Neumann series included: not symmetric at truncation level, and never symmetrised.  The routes are those of
    eval_f_g_grad_hvp -- a table never changes the route (wa.plan_info()["sampled_hvp"]["route"]: "lane", "rowlane", "quad" or
    "sequential") -- on the same tangent-linear kernels.  With a parameterisation pq = fn(theta) the second derivative along v is
    Jfn' Hs (Jfn v) plus the curvature of fn against the sample gradient (torch_controls.sampled_hessvec).

    pq: the 2 Ncoupled x (2 nsteps + 1) table of traceobjgrad_samples; dirs: one such table or a stack (2 Ncoupled, 2 nsteps + 1, ndir).
    Returns a dict: infidelity, leak, infid_grad, leak_grad in the shape of pq (objFuncType == 1: infid_grad is the total gradient,
    leak_grad zeros), hv_infid, hv_leak of shape (2 Ncoupled, 2 nsteps + 1, ndir) (objFuncType == 1: hv_infid is the derivative of the
    total gradient, hv_leak zeros).  No Tikhonov term; params.last_* are left alone.  Shape errors and entries that are not finite raise
    ValueError before any library call; the library refuses what eval_f_g_grad_hvp refuses, uncoupled controls among it."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("%s: wa must be a Working_Arrays_HIP" % _who)
    if wa.params is not params:
        raise ValueError("%s: wa was allocated for a different objparams" % _who)
    tab, shape = _sample_table(pq, params, _who)
    D, nd = _direction_tables(dirs, params, _who)
    try:
        nodes, weights = np.asarray(nodes, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("%s: nodes and weights must be vectors of numbers (%s)" % (_who, e))
    if nodes.ndim != 1 or weights.ndim != 1 or nodes.size != weights.size:
        raise ValueError("%s: nodes and weights must be vectors of the same length, not %r and %r" % (_who, nodes.shape, weights.shape))
    if nodes.size < 1:
        raise ValueError("%s: need at least one node" % _who)
    sh = None
    if shift is not None:
        if np.shape(shift) != (int(params.Ntot),):
            raise ValueError("%s: shift must have one entry per level, not shape %r" % (_who, np.shape(shift)))
        sh = _f64(shift)
    nodes, weights = _f64(nodes), _f64(weights)
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out2 = np.zeros(2)
    ig, lg = np.zeros(tab.size), np.zeros(tab.size)
    hvi, hvl = np.zeros(tab.size * nd), np.zeros(tab.size * nd)
    _lib.check(L.jq_eval_f_g_grad_samples_hvp(h, _ptr(tab), shape[1], _ptr(D), nd, _ptr(nodes), _ptr(weights), nodes.size, _ptr(sh), _ptr(out2),
                                              _ptr(ig), _ptr(lg), _ptr(hvi), _ptr(hvl)), h)
    return dict(infidelity=float(out2[0]), leak=float(out2[1]), infid_grad=ig.reshape(shape, order="F"), leak_grad=lg.reshape(shape, order="F"),
                hv_infid=hvi.reshape(shape + (nd,), order="F"), hv_leak=hvl.reshape(shape + (nd,), order="F"))


def tikhonov_hessvec(d, tik0):
    """The second derivative of the Tikhonov term along d: tikhonov_grad is affine in pcof (2 tik0 (pcof - prior) / Npar), so its
    derivative along d is tikhonov_grad(d) without the prior -- the prior is a constant."""
    return tikhonov_grad(d, tik0, None)


def eval_hessvec_par(pcof, d, params, wa, nodes=(0.0,), weights=(1.0,)):
    """The derivative along d of what eval_grad_f_par returns (the exact-Hessian callback of setup_ipopt_problem(hessian="exact")):
    hv_infid of eval_f_g_grad_hvp -- objFuncType == 1: the derivative of the total gradient, which that call returns as hv_infid with
    hv_leak zero -- plus the second derivative of the Tikhonov term.  The routes are eval_f_g_grad_hvp's: lane kernels (Ntot <= 6),
    row-lane kernels (Ntot 9 .. 16), quad-layout kernels (Ntot > 16 with the 4 x 4 x n structure), else the nodes one after the other."""
    d = np.asarray(d, dtype=np.float64)
    r = eval_f_g_grad_hvp(pcof, d, params, wa, nodes, weights)
    hv = r["hv_infid"][:, 0]
    if params.objFuncType == 1:
        hv = hv + r["hv_leak"][:, 0]
    return hv + tikhonov_hessvec(d, params.tik0)


def _drift_ensemble(params, Hconsts, weights, who):
    """(members [ndrift, Ntot * Ntot], weights [ndrift]) of a drift ensemble; ValueError for wrong shapes"""
    H = _drift_members(Hconsts, int(params.Ntot), who)
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("%s: weights must be a vector of numbers (%s)" % (who, e))
    if w.ndim != 1 or w.size != H.shape[0]:
        raise ValueError("%s: need one weight per member drift (%d), not shape %r" % (who, H.shape[0], w.shape))
    return H, _f64(w)


def eval_f_g_grad_drifts(pcof, params, wa, Hconsts, weights, compute_adjoint=True, per_member=False):
    """eval_f_g_grad over an ensemble of ARBITRARY drift Hamiltonians in one library call (jq_eval_f_g_grad_drifts): the weighted sums
    sum_i w_i infidelity_i, sum_i w_i leak_i and, with compute_adjoint, of the members' gradients, member i being the evaluation with
    params.Hconst = Hconsts[:, :, i] -- uncertain frequencies on a tensor grid, an uncertain anharmonicity, cross-Kerr or coupling term.
    Routing as traceobjgrad_drifts (wa.plan_info()["drift_batch"]).  Results land in params.last_* exactly as eval_f_g_grad leaves them.

    Hconsts: an Ntot x Ntot x ndrift array or a sequence of Ntot x Ntot matrices; weights: one per member.
    Returns (last_infidelity, last_leak), with per_member=True also the array [4, ndrift] of (objfv, primaryobjf, secondaryobjf,
    traceInfidelity) per member -- the bits of traceobjgrad_drifts.  Shape errors raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("eval_f_g_grad_drifts: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("eval_f_g_grad_drifts: wa was allocated for a different objparams")
    H, w = _drift_ensemble(params, Hconsts, weights, "eval_f_g_grad_drifts")
    p = np.asarray(pcof, dtype=np.float64)
    n = int(wa.nCoeff)
    if p.ndim != 1 or p.size != n:
        raise ValueError("eval_f_g_grad_drifts: pcof has shape %r, expected (%d,) (wa.nCoeff)" % (p.shape, n))
    p = _f64(p)
    nd = H.shape[0]
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    # (the memoised gradients are reset like eval_f_g_grad resets them: src/ipopt_interface.jl:27-31)
    params.last_infidelity_grad = np.zeros(n)
    params.last_leak_grad = np.zeros(n) if params.objFuncType != 1 else np.zeros(0)
    out2 = np.zeros(2)
    ig, lg = np.zeros(n), np.zeros(n)
    member_out = np.zeros((nd, 4)) if per_member else None
    _lib.check(L.jq_eval_f_g_grad_drifts(h, _ptr(p), n, _ptr(H), _ptr(w), nd, 1 if compute_adjoint else 0, _ptr(out2), _ptr(ig), _ptr(lg),
                                         _ptr(member_out)), h)
    params.last_pcof = p.copy()
    params.last_infidelity = float(out2[0])
    params.last_leak = float(out2[1])
    if compute_adjoint:
        params.last_infidelity_grad = ig.copy()
        params.last_leak_grad = lg.copy() if params.objFuncType != 1 else np.zeros(0)
    params.lastTraceInfidelity = params.last_infidelity
    params.lastLeakIntegral = params.last_leak
    if per_member:
        return params.last_infidelity, params.last_leak, np.ascontiguousarray(member_out.T)
    return params.last_infidelity, params.last_leak


def eval_f_g_grad_drifts_hvp(pcof, dirs, params, wa, drifts, weights):
    """eval_f_g_grad_hvp over the members of a drift ensemble instead of over eps-nodes, in one library call
    (jq_eval_f_g_grad_drifts_hvp): the weighted sums sum_i w_i of infidelity and leak, of the two gradients and of their derivatives
    along the columns of dirs, member i being the evaluation with params.Hconst = drifts[:, :, i] (the members of eval_f_g_grad_drifts).
    The routes are eval_f_g_grad_hvp's with a member where that call has a node: every wave reads the operator stream of its own member,
    the members that the stream budget (option stream_bytes) has no room for follow in further member rounds.  A member outside the
    structure the handle was planned for, and every problem whose nodes eval_f_g_grad_hvp runs one after the other, sends the members
    one after the other (route "sequential"; wa.plan_info()["drift_hvp"] = {route, members_per_launch, directions_per_launch,
    chunk_steps, rounds}).  The handle is never re-planned; params.Hconst, the handle's drift and params.last_* are left alone.

    dirs: an ncoeff x ndir array (one direction per column) or a single vector; drifts: an Ntot x Ntot x ndrift array or a sequence
    of Ntot x Ntot matrices; weights: one per member.  Returns the dict of eval_f_g_grad_hvp.  Not served: control mixes, members x
    eps-nodes, sharding over devices.  Shape errors raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("eval_f_g_grad_drifts_hvp: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("eval_f_g_grad_drifts_hvp: wa was allocated for a different objparams")
    ncoeff = int(wa.nCoeff)
    try:
        p = np.asarray(pcof, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("eval_f_g_grad_drifts_hvp: pcof must be a vector of numbers (%s)" % e)
    if p.ndim != 1 or p.size != ncoeff:
        raise ValueError("eval_f_g_grad_drifts_hvp: pcof has shape %r, expected (%d,) (wa.nCoeff)" % (p.shape, ncoeff))
    H, w = _drift_ensemble(params, drifts, weights, "eval_f_g_grad_drifts_hvp")
    D = _directions(dirs, ncoeff, "eval_f_g_grad_drifts_hvp")
    p = _f64(p)
    nd, nm = D.shape[0], H.shape[0]
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out2 = np.zeros(2)
    ig, lg = np.zeros(ncoeff), np.zeros(ncoeff)
    hvi, hvl = np.zeros((nd, ncoeff)), np.zeros((nd, ncoeff))
    _lib.check(L.jq_eval_f_g_grad_drifts_hvp(h, _ptr(p), ncoeff, _ptr(D), nd, _ptr(H), _ptr(w), nm, _ptr(out2), _ptr(ig), _ptr(lg), _ptr(hvi),
                                             _ptr(hvl)), h)
    return dict(infidelity=float(out2[0]), leak=float(out2[1]), infid_grad=ig, leak_grad=lg, hv_infid=np.ascontiguousarray(hvi.T),
                hv_leak=np.ascontiguousarray(hvl.T))


def eval_hessvec_drifts(pcof, d, params, wa, drifts, weights):
    """eval_hessvec_par for a drift ensemble: the derivative along d of the ensemble's gradient (eval_grad_f_par with drifts=...), hv_infid
    of eval_f_g_grad_drifts_hvp -- objFuncType == 1: the derivative of the total gradient -- plus the second derivative of the Tikhonov
    term.  (setup_ipopt_problem(hessian="exact") does not take a drift ensemble; this is the callback for a caller's own trust-region loop.)"""
    d = np.asarray(d, dtype=np.float64)
    r = eval_f_g_grad_drifts_hvp(pcof, d, params, wa, drifts, weights)
    hv = r["hv_infid"][:, 0]
    if params.objFuncType == 1:
        hv = hv + r["hv_leak"][:, 0]
    return hv + tikhonov_hessvec(d, params.tik0)


def eval_f_g_grad_members_hvp(pcof, dirs, params, wa, weights, Hconsts=None, ctrl_mix=None):
    """eval_f_g_grad_drifts_hvp over the members of eval_f_g_grad_members, in one library call (jq_eval_f_g_grad_members_hvp): the weighted
    sums sum_i w_i of infidelity and leak, of the two gradients and of their derivatives along the columns of dirs, over members that
    differ in a real mixing matrix of the controls (ctrl_mix: Nc x Nc x nmember; amplitude_mix for miscalibrated amplitudes), in their
    drift (Hconsts), or in both.  ctrl_mix=None is eval_f_g_grad_drifts_hvp, bit for bit.  With mixes the routes stay that call's, but the
    tangent stream of a direction is the member's own (sum_l (C_i d)_l H_l): a member brings 1 + directions_per_launch streams into a
    launch, the members that the stream budget (option stream_bytes) has no room for follow in further member rounds
    (wa.plan_info()["member_hvp"] = {route, members_per_launch, directions_per_launch, chunk_steps, rounds, drifts, ctrl_mix}).  The
    handle is never re-planned; params.Hconst, the handle's drift and params.last_* are left alone.

    dirs: an ncoeff x ndir array (one direction per column) or a single vector; weights: one per member; Hconsts: None (the drift of
    params) or as for eval_f_g_grad_drifts_hvp; ctrl_mix: None (identity), an Nc x Nc x nmember array or a sequence of Nc x Nc matrices.
    Returns the dict of eval_f_g_grad_hvp.  Not served: members x eps-nodes, sharding over devices.  Shape errors raise ValueError
    before any library call."""
    who = "eval_f_g_grad_members_hvp"
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("%s: wa must be a Working_Arrays_HIP" % who)
    if wa.params is not params:
        raise ValueError("%s: wa was allocated for a different objparams" % who)
    ncoeff = int(wa.nCoeff)
    try:
        p = np.asarray(pcof, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("%s: pcof must be a vector of numbers (%s)" % (who, e))
    if p.ndim != 1 or p.size != ncoeff:
        raise ValueError("%s: pcof has shape %r, expected (%d,) (wa.nCoeff)" % (who, p.shape, ncoeff))
    H, C, nm = _members(params, Hconsts, ctrl_mix, who)
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("%s: weights must be a vector of numbers (%s)" % (who, e))
    if w.ndim != 1 or w.size != nm:
        raise ValueError("%s: need one weight per member (%d), not shape %r" % (who, nm, w.shape))
    D = _directions(dirs, ncoeff, who)
    p, w = _f64(p), _f64(w)
    nd = D.shape[0]
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out2 = np.zeros(2)
    ig, lg = np.zeros(ncoeff), np.zeros(ncoeff)
    hvi, hvl = np.zeros((nd, ncoeff)), np.zeros((nd, ncoeff))
    _lib.check(L.jq_eval_f_g_grad_members_hvp(h, _ptr(p), ncoeff, _ptr(D), nd, _ptr(H), _ptr(C), _ptr(w), nm, _ptr(out2), _ptr(ig), _ptr(lg),
                                              _ptr(hvi), _ptr(hvl)), h)
    return dict(infidelity=float(out2[0]), leak=float(out2[1]), infid_grad=ig, leak_grad=lg, hv_infid=np.ascontiguousarray(hvi.T),
                hv_leak=np.ascontiguousarray(hvl.T))


def eval_hessvec_members(pcof, d, params, wa, weights, Hconsts=None, ctrl_mix=None):
    """eval_hessvec_drifts for a member ensemble: the derivative along d of the ensemble's gradient (eval_grad_f_par with ctrl_mix=...),
    hv_infid of eval_f_g_grad_members_hvp -- objFuncType == 1: the derivative of the total gradient -- plus the second derivative of the
    Tikhonov term.  (setup_ipopt_problem(hessian="exact") does not take a member ensemble; this is the callback for a caller's own
    trust-region loop.)"""
    d = np.asarray(d, dtype=np.float64)
    r = eval_f_g_grad_members_hvp(pcof, d, params, wa, weights, Hconsts=Hconsts, ctrl_mix=ctrl_mix)
    hv = r["hv_infid"][:, 0]
    if params.objFuncType == 1:
        hv = hv + r["hv_leak"][:, 0]
    return hv + tikhonov_hessvec(d, params.tik0)


def eval_f_g_grad_members(pcof, params, wa, weights, Hconsts=None, ctrl_mix=None, compute_adjoint=True, per_member=False):
    """eval_f_g_grad_drifts over the members of traceobjgrad_members (jq_eval_f_g_grad_members): the weighted sums over members that differ
    in a real mixing matrix of the controls (ctrl_mix: Nc x Nc x nmember; amplitude_mix for miscalibrated amplitudes), in their drift
    (Hconsts), or in both.  Results land in params.last_* exactly as eval_f_g_grad leaves them; routing: wa.plan_info()["member_batch"].

    weights: one per member.  Returns (last_infidelity, last_leak), with per_member=True also the array [4, nmember] of the members'
    records -- the bits of traceobjgrad_members.  Shape errors raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("eval_f_g_grad_members: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("eval_f_g_grad_members: wa was allocated for a different objparams")
    H, C, nm = _members(params, Hconsts, ctrl_mix, "eval_f_g_grad_members")
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("eval_f_g_grad_members: weights must be a vector of numbers (%s)" % e)
    if w.ndim != 1 or w.size != nm:
        raise ValueError("eval_f_g_grad_members: need one weight per member (%d), not shape %r" % (nm, w.shape))
    w = _f64(w)
    p = np.asarray(pcof, dtype=np.float64)
    n = int(wa.nCoeff)
    if p.ndim != 1 or p.size != n:
        raise ValueError("eval_f_g_grad_members: pcof has shape %r, expected (%d,) (wa.nCoeff)" % (p.shape, n))
    p = _f64(p)
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    # (the memoised gradients are reset like eval_f_g_grad resets them: src/ipopt_interface.jl:27-31)
    params.last_infidelity_grad = np.zeros(n)
    params.last_leak_grad = np.zeros(n) if params.objFuncType != 1 else np.zeros(0)
    out2 = np.zeros(2)
    ig, lg = np.zeros(n), np.zeros(n)
    member_out = np.zeros((nm, 4)) if per_member else None
    _lib.check(L.jq_eval_f_g_grad_members(h, _ptr(p), n, _ptr(H), _ptr(C), _ptr(w), nm, 1 if compute_adjoint else 0, _ptr(out2), _ptr(ig),
                                          _ptr(lg), _ptr(member_out)), h)
    params.last_pcof = p.copy()
    params.last_infidelity = float(out2[0])
    params.last_leak = float(out2[1])
    if compute_adjoint:
        params.last_infidelity_grad = ig.copy()
        params.last_leak_grad = lg.copy() if params.objFuncType != 1 else np.zeros(0)
    params.lastTraceInfidelity = params.last_infidelity
    params.lastLeakIntegral = params.last_leak
    if per_member:
        return params.last_infidelity, params.last_leak, np.ascontiguousarray(member_out.T)
    return params.last_infidelity, params.last_leak


def eval_f_g_grad_samples_members(pq, params, wa, weights, Hconsts=None, ctrl_mix=None, compute_adjoint=True, per_member=False):
    """eval_f_g_grad_members for controls given as VALUES on the time grid (jq_eval_f_g_grad_samples_members): the weighted sums over
    members that share ONE sample table and differ in a real mixing matrix of the controls (ctrl_mix), in their drift (Hconsts), or in
    both -- the robust objective of a piecewise-constant, filtered or network-generated pulse.  The two gradients are summed on the device
    in member order; the members' own gradient tables are never fetched.  Routing: wa.plan_info()["sampled_batch"].

    weights: one per member.  Returns the dict of eval_f_g_grad_samples (infidelity, leak, and with compute_adjoint infid_grad, leak_grad in
    the shape of pq), with per_member=True also members: the array [4, nmember] of the members' records -- the bits of
    traceobjgrad_samples_members.  No Tikhonov term; params.last_* are left alone.  Shape errors and entries that are not finite raise
    ValueError before any library call."""
    who = "eval_f_g_grad_samples_members"
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("%s: wa must be a Working_Arrays_HIP" % who)
    if wa.params is not params:
        raise ValueError("%s: wa was allocated for a different objparams" % who)
    tab, shape = _sample_table(pq, params, who)
    H, C, nm = _members(params, Hconsts, ctrl_mix, who)
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("%s: weights must be a vector of numbers (%s)" % (who, e))
    if w.ndim != 1 or w.size != nm:
        raise ValueError("%s: need one weight per member (%d), not shape %r" % (who, nm, w.shape))
    w = _f64(w)
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out2 = np.zeros(2)
    ig = np.zeros(tab.size) if compute_adjoint else None
    lg = np.zeros(tab.size) if compute_adjoint else None
    member_out = np.zeros((nm, 4)) if per_member else None
    _lib.check(L.jq_eval_f_g_grad_samples_members(h, _ptr(tab), shape[1], _ptr(H), _ptr(C), _ptr(w), nm, 1 if compute_adjoint else 0, _ptr(out2),
                                                  _ptr(ig), _ptr(lg), _ptr(member_out)), h)
    r = dict(infidelity=float(out2[0]), leak=float(out2[1]))
    if compute_adjoint:
        r["infid_grad"], r["leak_grad"] = ig.reshape(shape, order="F"), lg.reshape(shape, order="F")
    if per_member:
        r["members"] = np.ascontiguousarray(member_out.T)
    return r


def _stale(pcof, params):
    # memoisation on ||pcof - last_pcof|| > 1e-15 (src/ipopt_interface.jl:83-84)
    last = params.last_pcof
    return last.size != np.size(pcof) or np.linalg.norm(np.asarray(pcof, dtype=np.float64) - last) > 1.0e-15


def _refresh(pcof, params, wa, nodes, weights, drifts, drift_weights, ctrl_mix=None):
    """the evaluation the callbacks memoise: eval_f_g_grad over the eps-nodes, (drifts given) eval_f_g_grad_drifts over the members, or
    (ctrl_mix given, with or without drifts; drift_weights: the members' weights) eval_f_g_grad_members"""
    if ctrl_mix is not None:
        eval_f_g_grad_members(pcof, params, wa, drift_weights, Hconsts=drifts, ctrl_mix=ctrl_mix, compute_adjoint=True)
    elif drifts is not None:
        eval_f_g_grad_drifts(pcof, params, wa, drifts, drift_weights, True)
    else:
        eval_f_g_grad(pcof, params, wa, nodes, weights, True)


def eval_f_par(pcof, params, wa, nodes=(0.0,), weights=(1.0,), drifts=None, drift_weights=None, ctrl_mix=None):
    """src/ipopt_interface.jl:77-99"""
    if _stale(pcof, params):
        _refresh(pcof, params, wa, nodes, weights, drifts, drift_weights, ctrl_mix)
    f = params.last_infidelity + params.last_leak if params.objFuncType == 1 else params.last_infidelity
    prior = params.priorCoeffs if params.usingPriorCoeffs else None
    return f + tikhonov_pen(pcof, params.tik0, prior)


def eval_g_par(pcof, g, params, wa, nodes=(0.0,), weights=(1.0,), drifts=None, drift_weights=None, ctrl_mix=None):
    """src/ipopt_interface.jl:104-118"""
    if _stale(pcof, params):
        _refresh(pcof, params, wa, nodes, weights, drifts, drift_weights, ctrl_mix)
    g[0] = params.last_leak
    return g[0]


def eval_grad_f_par(pcof, grad_f, params, wa, nodes=(0.0,), weights=(1.0,), drifts=None, drift_weights=None, ctrl_mix=None):
    """src/ipopt_interface.jl:124-148"""
    if _stale(pcof, params):
        _refresh(pcof, params, wa, nodes, weights, drifts, drift_weights, ctrl_mix)
    grad_f[:] = params.last_infidelity_grad
    prior = params.priorCoeffs if params.usingPriorCoeffs else None
    wa.gr[:] = tikhonov_grad(pcof, params.tik0, prior)
    grad_f += wa.gr
    if params.save_pcof_hist:
        params.pcof_hist.append(np.array(pcof, dtype=np.float64))


def eval_jac_g_par(pcof, rows, cols, jac_g, params, wa, nodes=(0.0,), weights=(1.0,), drifts=None, drift_weights=None, ctrl_mix=None):
    """src/ipopt_interface.jl:153-179 (including its quirk: when it has to recompute it returns
    without filling jac_g, :169-173)."""
    if jac_g is None:
        if len(rows) > 0:
            for i in range(len(pcof)):
                rows[i] = 1
                cols[i] = i + 1
        return
    if _stale(pcof, params):
        _refresh(pcof, params, wa, nodes, weights, drifts, drift_weights, ctrl_mix)
        return
    jac_g[:] = params.last_leak_grad


def traceobj_sweep(pcof, params, wa, ep_vals, shift=None):
    """The loop of ep_plot (examples/Risk_Neutral/run_all.jl:6-32) as one batched call: returns an
    array [len(ep_vals), 4] = (objfv, primaryobjf, secondaryobjf, traceInfidelity) per perturbation."""
    L, h = _lib.load(), wa.handle
    pcof = _f64(pcof)
    ep = _f64(ep_vals)
    wa.sync_params()
    out = np.zeros(4 * ep.size)
    sh = _f64(shift) if shift is not None else None
    _lib.check(L.jq_traceobj_sweep(h, _ptr(pcof), pcof.size, _ptr(ep), ep.size, _ptr(sh), _ptr(out)), h)
    return out.reshape((ep.size, 4))


# ---------------------------------------------------------------------------------------------
# Optimiser loop on top of the callbacks.  The reference hands the callbacks to
# Ipopt (L-BFGS Hessian approximation, bound constraints, optionally the leakage as one inequality
# constraint); Ipopt is not available in this image, so run_optimizer drives the SAME callbacks with
# scipy's bound-constrained quasi-Newton methods.  Names, arguments, memoisation, convergence history and
# the early-stop thresholds follow src/ipopt_interface.jl:205-437; the iterates differ from Ipopt's
# (different line search / barrier), the objective and gradient they see do not.
def intermediate_par(alg_mod, iter_count, obj_value, inf_pr, inf_du, mu, d_norm, regularization_size,
                     alpha_du, alpha_pr, ls_trials, params):
    """src/ipopt_interface.jl:205-236: record the convergence history, stop on the thresholds."""
    if params.saveConvHist:
        params.objHist.append(obj_value)
        params.dualInfidelityHist.append(inf_du)
        params.primaryHist.append(params.lastTraceInfidelity)
        params.secondaryHist.append(params.lastLeakIntegral)
    if obj_value < params.objThreshold:
        if not params.quiet:
            print("Stopping because objective value = ", obj_value, " < threshold = ", params.objThreshold)
        return False
    if params.lastTraceInfidelity < params.traceInfidelityThreshold:
        if not params.quiet:
            print("Stopping because trace infidelity = ", params.lastTraceInfidelity, " < threshold = ",
                  params.traceInfidelityThreshold)
        return False
    return True


class OptimProblem:
    """What setup_ipopt_problem returns: callbacks + options (the fields an IpoptProblem carries)."""

    def __init__(self):
        self.x = None
        self.obj_val = None
        self.status = None
        self.n_iter = 0


def setup_ipopt_problem(params, wa, nCoeff, minCoeff, maxCoeff, maxIter=50, lbfgsMax=10, startFromScratch=True,
                        ipTol=1.0e-5, acceptTol=1.0e-5, acceptIter=15, nodes=(0.0,), weights=(1.0,),
                        jacob_approx="exact", drifts=None, drift_weights=None, ctrl_mix=None, member_weights=None,
                        hessian="limited-memory"):
    """src/ipopt_interface.jl:262-415.
    drifts (an Ntot x Ntot x ndrift array or a sequence of matrices) with drift_weights (one per member): the callbacks memoise through
    eval_f_g_grad_drifts instead of eval_f_g_grad, so run_optimizer optimises the risk-neutral objective over that drift ensemble
    (nodes / weights are then not used).
    ctrl_mix (an Nc x Nc x nmember array or a sequence of matrices; amplitude_mix builds diagonal ones) with member_weights (one per member):
    the callbacks memoise through eval_f_g_grad_members -- the risk-neutral objective over miscalibrated amplitudes / crosstalk.  drifts and
    ctrl_mix may be given together (member i has both) with ONE weight vector, under either keyword; giving both weight keywords is an error.
    hessian: "limited-memory" (the reference's L-BFGS approximation; the default changes nothing) or "exact": prob.eval_hessvec(pcof, d) =
    eval_hessvec_par over the nodes (one launch per chunk on the lane kernels at Ntot <= 6, on the row-lane kernels at Ntot 9 .. 16 and on
    the quad-layout kernels at Ntot > 16 with the 4 x 4 x n structure, the nodes one after the other otherwise), and run_optimizer drives scipy's trust-constr with it.  "exact" with objFuncType == 3 (the leakage
    is a constraint), drifts or ctrl_mix raises ValueError: those Hessians are not built.
    Shape errors raise ValueError before any library call."""
    if hessian not in ("limited-memory", "exact"):
        raise ValueError("setup_ipopt_problem: hessian must be \"limited-memory\" or \"exact\", not %r" % (hessian,))
    if hessian == "exact":
        if params.objFuncType == 3:
            raise ValueError("setup_ipopt_problem: hessian=\"exact\" with objFuncType == 3 (leakage as a constraint) is not built")
        if drifts is not None or ctrl_mix is not None:
            raise ValueError("setup_ipopt_problem: hessian=\"exact\" with drifts or ctrl_mix is not built (eps-node ensembles only)")
    if drift_weights is not None and member_weights is not None:
        raise ValueError("setup_ipopt_problem: give drift_weights or member_weights, not both")
    if member_weights is not None:      # (one weight vector for the members, whatever differs between them)
        drift_weights = member_weights
    if ctrl_mix is not None:
        if drift_weights is None:
            raise ValueError("setup_ipopt_problem: ctrl_mix needs member_weights (one weight per member)")
        H, C, nm = _members(params, drifts, ctrl_mix, "setup_ipopt_problem")
        try:
            mw = np.asarray(drift_weights, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError("setup_ipopt_problem: member_weights must be a vector of numbers (%s)" % e)
        if mw.ndim != 1 or mw.size != nm:
            raise ValueError("setup_ipopt_problem: need one weight per member (%d), not shape %r" % (nm, mw.shape))
        nc = int(round(np.sqrt(C.shape[1])))
        ctrl_mix = [M.reshape((nc, nc), order="F") for M in C]
        drifts = [M.reshape((int(params.Ntot), int(params.Ntot)), order="F") for M in H] if H is not None else None
        drift_weights = _f64(mw)
    elif drifts is not None:
        if drift_weights is None:
            raise ValueError("setup_ipopt_problem: drifts needs drift_weights (one weight per member)")
        drifts, drift_weights = _drift_ensemble(params, drifts, drift_weights, "setup_ipopt_problem")
        drifts = [M.reshape((int(params.Ntot), int(params.Ntot)), order="F") for M in drifts]
    elif drift_weights is not None:
        raise ValueError("setup_ipopt_problem: member weights without drifts or ctrl_mix")
    minCoeff = np.asarray(minCoeff, dtype=np.float64)
    maxCoeff = np.asarray(maxCoeff, dtype=np.float64)
    if minCoeff.size != nCoeff or maxCoeff.size != nCoeff:
        raise ValueError("minCoeff and maxCoeff must have nCoeff elements")
    rng = np.random.default_rng()
    params.last_pcof = 1e9 * rng.random(nCoeff)              # :277-281: force the first evaluation
    params.last_infidelity_grad = 1e9 * rng.random(nCoeff)
    if params.objFuncType != 1:
        params.last_leak_grad = 1e9 * rng.random(nCoeff)
    nodes = np.asarray(nodes, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.float64)

    prob = OptimProblem()
    prob.params, prob.wa, prob.nCoeff = params, wa, int(nCoeff)
    prob.x_L, prob.x_U = minCoeff, maxCoeff
    ens = dict(drifts=drifts, drift_weights=drift_weights, ctrl_mix=ctrl_mix)
    prob.eval_f = lambda pcof: eval_f_par(pcof, params, wa, nodes, weights, **ens)

    def _grad(pcof):
        g = np.zeros(nCoeff)
        eval_grad_f_par(pcof, g, params, wa, nodes, weights, **ens)
        return g
    prob.eval_grad_f = _grad
    prob.eval_hessvec = (lambda pcof, d: eval_hessvec_par(pcof, d, params, wa, nodes, weights)) if hessian == "exact" else None
    if params.objFuncType == 3:                               # :299-306: leakage as an inequality constraint
        prob.m = 1
        prob.g_L, prob.g_U = np.array([-2e19]), np.array([params.leak_ubound])
    else:
        prob.m = 0
        prob.g_L, prob.g_U = np.zeros(0), np.zeros(0)

    def _g(pcof):
        g = np.zeros(1)
        eval_g_par(pcof, g, params, wa, nodes, weights, **ens)
        return g

    def _jac_g(pcof):
        jac = np.zeros(nCoeff)
        if _stale(pcof, params):     # the reference's callback returns unfilled in this case (:169-173); Ipopt
            _refresh(pcof, params, wa, nodes, weights, drifts, drift_weights, ctrl_mix)   # always calls eval_g first -- here we recompute
        eval_jac_g_par(pcof, [], [], jac, params, wa, nodes, weights, **ens)
        return jac
    prob.eval_g, prob.eval_jac_g = _g, _jac_g
    prob.intermediate = lambda it, obj, inf_du: intermediate_par(0, it, obj, 0.0, inf_du, 0.0, 0.0, 0.0, 0.0, 0.0, 0,
                                                                 params)
    prob.options = dict(max_iter=int(maxIter), limited_memory_max_history=int(lbfgsMax), tol=float(ipTol),
                        acceptable_tol=float(acceptTol), acceptable_iter=int(acceptIter),
                        warm_start=not startFromScratch, jacobian_approximation=jacob_approx, hessian_approximation=hessian)
    if not params.quiet:
        print("Optimizer parameters: max # iterations = ", maxIter)
        print("Optimizer parameters: max history L-BFGS = ", lbfgsMax)
        print("Optimizer parameters: tol = ", ipTol)
    return prob


class _Stop(Exception):
    pass


def run_optimizer(prob, pcof0, baseName=""):
    """src/ipopt_interface.jl:417-437: optimise the control vector, optionally save it as <baseName>.jld2."""
    from scipy import optimize
    from .pcof_io import save_pcof
    params = prob.params
    x0 = np.clip(np.array(pcof0, dtype=np.float64), prob.x_L, prob.x_U)     # copy: pcof0 is not overwritten
    opt = prob.options
    bounds = optimize.Bounds(prob.x_L, prob.x_U)
    state = {"it": 0, "x": x0.copy()}

    def callback(xk, *_):
        state["it"] += 1
        state["x"] = np.array(xk, dtype=np.float64)
        obj = prob.eval_f(xk)                      # memoised: no extra propagation for an accepted iterate
        g = prob.eval_grad_f(xk)
        # projected-gradient norm as the dual infeasibility measure of the bound-constrained problem
        pg = np.where((xk <= prob.x_L) & (g > 0) | (xk >= prob.x_U) & (g < 0), 0.0, g)
        if not prob.intermediate(state["it"], obj, float(np.max(np.abs(pg))) if pg.size else 0.0):
            raise _Stop()

    if not params.quiet:
        print("*** Starting the optimization ***")
    try:
        if prob.m == 0 and getattr(prob, "eval_hessvec", None) is not None:      # hessian="exact": Newton-type steps on exact products
            res = optimize.minimize(prob.eval_f, x0, jac=prob.eval_grad_f, hessp=prob.eval_hessvec, method="trust-constr", bounds=bounds,
                                    callback=callback, options=dict(maxiter=opt["max_iter"], gtol=opt["tol"], xtol=1e-12))
        elif prob.m == 0:
            res = optimize.minimize(prob.eval_f, x0, jac=prob.eval_grad_f, method="L-BFGS-B", bounds=bounds,
                                    callback=callback,
                                    options=dict(maxiter=opt["max_iter"], maxcor=opt["limited_memory_max_history"],
                                                 ftol=0.0, gtol=opt["tol"]))
        else:
            cons = [dict(type="ineq", fun=lambda x: prob.g_U - prob.eval_g(x), jac=lambda x: -prob.eval_jac_g(x)[None, :])]
            res = optimize.minimize(prob.eval_f, x0, jac=prob.eval_grad_f, method="SLSQP", bounds=bounds,
                                    constraints=cons, callback=callback,
                                    options=dict(maxiter=opt["max_iter"], ftol=opt["tol"] * 1e-3))
        x, prob.status = np.array(res.x), str(res.message)
    except _Stop:
        x, prob.status = state["x"], "stopped by intermediate callback (threshold reached)"
    prob.x = x
    prob.obj_val = prob.eval_f(x)
    prob.n_iter = state["it"]
    if len(baseName) > 0:
        save_pcof(baseName + ".jld2", x)
        if not params.quiet:
            print("Saved B-spline parameters on binary jld2-file '%s.jld2'" % baseName)
    return x
