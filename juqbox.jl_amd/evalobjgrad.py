"""Host-side mirror of the reference's hot-path entry points over the C ABI:

  Working_Arrays_HIP(params, nCoeff)    the drop-in third working-array type:
                                        where the reference dispatches traceobjgrad on
                                        wa::Working_Arrays (src/evalobjgrad.jl:504) this type forwards
                                        to libjuqbox_hip.so.  Offers `wa.gr` like Working_Arrays (:400),
                                        which eval_grad_f_par uses (src/ipopt_interface.jl:139-141).
  traceobjgrad(pcof0, params, wa, verbose=False, evaladjoint=True)
                                        same argument order and return tuples as
                                        src/evalobjgrad.jl:504, :1027-1036.
  traceobjgrad_batch(pcofs, params, wa, evaladjoint=True)
                                        many control vectors of ONE problem in one library call
                                        (jq_traceobjgrad_batch): column i = traceobjgrad of vector i.
  traceobjgrad_drifts(pcof, params, wa, Hconsts, evaladjoint=True)
                                        ONE control vector over an ensemble of drift Hamiltonians in one library
                                        call (jq_traceobjgrad_drifts): column i = traceobjgrad with Hconst = member i.
  traceobjgrad_members(pcof, params, wa, Hconsts=None, ctrl_mix=None, evaladjoint=True)
                                        ... over members that differ in a real mixing matrix of the controls (amplitude
                                        miscalibration, crosstalk), in their drift, or in both (jq_traceobjgrad_members).
  amplitude_mix(scales)                 [nmember, Nc] amplitude factors -> the diagonal mixes of such an ensemble.
  traceobj_jvp(pcof, dirs, params, wa, final=True)
                                        the tangent of the discrete forward map along directions of coefficient space
                                        (jq_traceobj_jvp): d(objective) and dV(T)/d(alpha) . d, exact to rounding.
  traceobjgrad_hvp(pcof, dirs, params, wa)
                                        the gradient and its derivative along directions of coefficient space
                                        (jq_traceobjgrad_hvp): Hessian-vector products, exact to rounding.
  hessian(pcof, params, wa, symmetrize=False)
                                        all unit directions through one traceobjgrad_hvp call.
  gradient_check(pcof0, params, wa, kpars, h=1e-6)
                                        adjoint gradient entries against central differences, from one batch.
  traceobjgrad_samples(pq, params, wa, evaladjoint=True)
                                        traceobjgrad for controls given as values on the time grid (jq_traceobjgrad_samples): the
                                        objective of a 2 Ncoupled x (2 nsteps + 1) table and its gradient per entry -- any
                                        parameterisation is then a chain rule on the host.
  traceobjgrad_samples_batch(pqs, params, wa, evaladjoint=True)
  traceobjgrad_samples_members(pq, params, wa, Hconsts=None, ctrl_mix=None, evaladjoint=True)
                                        traceobjgrad_samples for many tables, or for ONE table under members that differ in their drift
                                        and in a real mix of the controls, in one library call (jq_traceobjgrad_samples_batch,
                                        jq_traceobjgrad_samples_members): the groups share launches where the spline batch does.
  traceobjgrad_samples_hvp(pq, dirs, params, wa)
                                        its gradient and the derivative of that gradient along direction tables
                                        (jq_eval_f_g_grad_samples_hvp, one node): Hessian-vector products in sample space.
  control_sample_times(params, wa), control_samples(pcof, params, wa), spline_sample_matrix(params, ncoeff, times)
                                        the grid, the library's own controls on it, and their dense derivative d pq / d pcof.
"""
import contextlib
import ctypes
import threading

import numpy as np

from . import _lib
from .objparams import (JACOBI_SOLVER, JACOBI_SOLVER_M, NEUMANN_SOLVER, Implicit_Midpoint, Stormer_Verlet,
                        objparams)


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel(order="F"))


def _ptr(a):
    return a.ctypes.data_as(_lib.c_dp) if a is not None else None


class _Csc:
    """A dense operator in the fields of Julia's SparseMatrixCSC{Float64,Int64} (1-based Int64 colptr / rowval) with the
    jq_csc descriptor pointing at them -- what the Julia binding passes for use_sparse = true problems."""

    def __init__(self, M):
        M = np.asarray(M, dtype=np.float64)
        n = M.shape[0]
        cols, rows, vals = [1], [], []
        for j in range(n):
            nz = np.nonzero(M[:, j])[0]
            rows.extend((nz + 1).tolist())
            vals.extend(M[nz, j].tolist())
            cols.append(len(rows) + 1)
        self.colptr = np.array(cols, dtype=np.int64)
        self.rowval = np.array(rows if rows else [1], dtype=np.int64)
        self.nzval = np.array(vals if vals else [0.0], dtype=np.float64)
        self.desc = _lib.jq_csc(n, n, self.colptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                self.rowval.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _ptr(self.nzval))


def _csc_array(mats):
    keep = [_Csc(M) for M in mats]
    arr = (_lib.jq_csc * max(len(keep), 1))(*[k.desc for k in keep])
    return keep, arr


# ---- per-handle options (include/juqbox_hip.h: jq_create_opts / jq_set_option; the table of names is in INTEGRATION.md section 4) ----
_defaults = threading.local()


def _option_string(opts):
    return ",".join("%s=%d" % (k, int(v)) for k, v in opts.items())


def _norm_options(opts):
    """{"quad": 0} or the historic spelling {"JQ_QUAD": "0"} -> {"quad": 0}"""
    return {(k[3:].lower() if k.startswith("JQ_") else k): int(v) for k, v in (opts or {}).items()}


@contextlib.contextmanager
def options(**opts):
    """Default options for the handles CREATED inside the `with` block (tests, bisection):
        with jq.options(quad=0, coop_max=0):
            wa = jq.Working_Arrays_HIP(params, nCoeff)
    They are options of those handles from then on (nothing is read from the environment); an explicit `options=` argument of the
    constructor is applied on top.  Nested blocks add up.  Options of an existing handle: wa.set_option(name, value)."""
    prev = dict(getattr(_defaults, "opts", {}))
    merged = dict(prev)
    merged.update(_norm_options(opts))
    _defaults.opts = merged
    try:
        yield
    finally:
        _defaults.opts = prev


def check_supported(params):
    """What the reference's objparams can hold and this path does not evaluate is refused, never served by something else: the kernels
    implement the trace fidelity pFidType == 2 (the constructor's value, src/evalobjgrad.jl:164; the struct is mutable).  Called before
    any library call."""
    if getattr(params, "pFidType", 2) != 2:
        raise ValueError("JQ_EUNSUPPORTED: pFidType = %r -- only pFidType = 2 (the trace fidelity objparams sets, "
                         "src/evalobjgrad.jl:164) is implemented" % (params.pFidType,))


class Working_Arrays_HIP:
    """Owns the device handle for one `objparams`.  Mutable fields of `params` that scripts change
    after construction (Hconst, wmat_real, Utarget_r/i, linear_solver.max_iter) are re-synchronised
    with the device at every call, so `params` stays the single source of truth like in the reference."""

    INTEGRATOR = Stormer_Verlet
    SOLVERS = (NEUMANN_SOLVER, JACOBI_SOLVER)

    def _weights(self, p):
        """leakage weights of this path: params.wmat_real (src/evalobjgrad.jl:583) -- a vector (the Diagonal default) or, with
        use_custom_forbidden (:214-232), a full matrix next to params.wmat_imag: then (wmat_real, wmat_imag) stacked"""
        wi = getattr(p, "wmat_imag", None)
        if np.ndim(p.wmat_real) == 2:
            wi = np.zeros_like(p.wmat_real) if wi is None or np.ndim(wi) != 2 else wi      # (Diagonal(zeros(Ntot)), :236)
            return np.concatenate([_f64(p.wmat_real), _f64(wi)])
        if wi is not None and np.any(np.asarray(wi) != 0):
            # a Diagonal wmat_real next to a non-zero wmat_imag: the Julia binding passes both as full matrices (a full wmat_imag) or
            # refuses (a Diagonal one is not a Hermitian weight); dropping wmat_imag silently would evaluate something else
            if np.ndim(wi) == 2:
                return np.concatenate([_f64(np.diag(np.asarray(p.wmat_real, dtype=np.float64))), _f64(wi)])
            raise ValueError("a non-zero Diagonal wmat_imag is not a Hermitian leakage weight (julia/hip_backend.jl refuses it too)")
        return _f64(p.wmat_real)

    def _push_weights(self, w):
        L, p, h = _lib.load(), self.params, self.handle
        if w.size == p.Ntot:
            _lib.check(L.jq_update_wmat_diag(h, _ptr(w)), h)
        elif w.size == 2 * p.Ntot * p.Ntot:
            wr, wi = w[:p.Ntot * p.Ntot].copy(), w[p.Ntot * p.Ntot:].copy()
            _lib.check(L.jq_update_wmat(h, _ptr(wr), _ptr(wi)), h)
        else:
            raise ValueError("wmat_real must be a vector of length Ntot (Diagonal) or an Ntot x Ntot matrix")

    def __init__(self, params: objparams, nCoeff: int, devices=None, csc=None, options=None):
        """devices: None = the current HIP device (one process per GPU); an int n or a list of device ids = ONE process
        driving several GPUs (jq_create_multi: the ensemble of eval_f_g_grad is sharded over them and summed with one
        RCCL all-reduce inside the library).
        csc: hand the operators over in sparse (SparseMatrixCSC) storage like the Julia binding does for use_sparse = true
        problems (default: params.use_sparse); the results are bit-identical to the dense form.
        options: {name: value} for jq_create_opts (on top of the defaults of an enclosing `with options(...)` block)."""
        check_supported(params)
        L = _lib.load()
        if params.linear_solver.solver_id not in self.SOLVERS:
            raise ValueError("Please specify a supported linear solver")
        self.params = params
        self.nCoeff = int(nCoeff)
        self.gr = np.zeros(self.nCoeff)            # Working_Arrays.gr (src/evalobjgrad.jl:400)
        p = params
        hs = np.concatenate([_f64(h) for h in p.Hsym_ops]) if p.Ncoupled else np.zeros(1)
        ha = np.concatenate([_f64(h) for h in p.Hanti_ops]) if p.Ncoupled else np.zeros(1)
        self._hconst = _f64(p.Hconst).copy()
        w0 = self._weights(p).copy()
        self._wd = w0 if w0.size == p.Ntot else np.zeros(p.Ntot)      # (full weights follow the creation: jq_update_wmat)
        self._utr = _f64(p.Utarget_r).copy()
        self._uti = _f64(p.Utarget_i).copy()
        self._dvr, self._dvi, self._sv_type = self._utr, self._uti, 1      # (a new handle: dVds = target, sv_type 1)
        self._m = int(p.linear_solver.max_iter) if self.INTEGRATOR == Stormer_Verlet else 0
        self._solver = None
        nunc = getattr(p, "Nunc", 0)
        hu = np.concatenate([_f64(h) for h in p.Hunc_ops]) if nunc else None
        rf = _f64(p.Rfreq[:nunc]) if nunc else None
        keep = [self._hconst, hs, ha, _f64(p.Uinit), self._utr, self._uti, self._wd, _f64(p.Cfreq[:p.Ncoupled + nunc, :]), hu, rf]
        ptrs = [_ptr(a) for a in keep]
        sparse_args = [None, None, None]
        use_csc = bool(getattr(p, "use_sparse", False)) if csc is None else bool(csc)
        if use_csc and not nunc:
            k0, a0 = _csc_array([p.Hconst])
            ks, as_ = _csc_array(p.Hsym_ops)
            ka, aa = _csc_array(p.Hanti_ops)
            keep += [k0, a0, ks, as_, ka, aa]
            ptrs[0] = ptrs[1] = ptrs[2] = None
            sparse_args = [a0, as_, aa]
        self._csc = use_csc and not nunc
        prob = _lib.jq_problem(p.Ntot, p.N, p.Ncoupled, p.Nfreq, p.nsteps, self._m, p.objFuncType, nunc, p.T, *ptrs, *sparse_args)
        h = ctypes.c_void_p()
        opts = dict(getattr(_defaults, "opts", {}))
        opts.update(_norm_options(options))
        self.options = opts
        ostr = _option_string(opts).encode() if opts else None
        if devices is None:
            opts.pop("multi_same_device", None)
            ostr = _option_string(opts).encode() if opts else None
            rc = L.jq_create_opts(ctypes.byref(prob), ostr, ctypes.byref(h))
        else:
            devs = list(range(devices)) if isinstance(devices, int) else [int(d) for d in devices]
            arr = (ctypes.c_int32 * len(devs))(*devs)
            rc = L.jq_create_multi_opts(ctypes.byref(prob), arr, len(devs), ostr, ctypes.byref(h))
        if rc != _lib.JQ_OK:
            msg = L.jq_last_error(None)
            raise _lib.JuqboxHipError(rc, msg.decode() if msg else "?")
        self.handle = h
        self.num_devices = L.jq_num_devices(h)
        self.device = L.jq_handle_device(h)      # HIP device the handle is bound to (first one of a multi-device handle)
        self.last_allreduce_ms = 0.0             # one process per GPU: wall time of the caller's all-reduce (ipopt_interface.py)
        if w0.size != p.Ntot:
            try:
                self._push_weights(w0)
            except Exception:
                self.close()
                raise
            self._wd = w0

    def close(self):
        if getattr(self, "handle", None):
            _lib.load().jq_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync_params(self):
        """Push post-construction mutations of `params` to the device (only what changed)."""
        check_supported(self.params)
        L, p, h = _lib.load(), self.params, self.handle
        ls = p.linear_solver
        if ls.solver_id not in self.SOLVERS:
            raise ValueError("Please specify a supported linear solver")
        key = (int(ls.solver_id), int(ls.max_iter), float(ls.tol))
        # Diagonal weights go in BEFORE the solver / integrator, full weights AFTER it: full weights exist with the Neumann solver only,
        # so (full weights, Neumann) <-> (Diagonal, Jacobi) is a valid switch in one step in either direction (as julia/hip_backend.jl)
        wd = self._weights(p)
        if wd.size == p.Ntot and (wd.size != self._wd.size or not np.array_equal(wd, self._wd)):
            self._push_weights(wd)
            self._wd = wd.copy()
        if key != self._solver:
            if self.INTEGRATOR == Stormer_Verlet:
                _lib.check(L.jq_set_linear_solver(h, key[0], key[1], key[2]), h)
                self._m = key[1]
            else:
                _lib.check(L.jq_set_integrator(h, Implicit_Midpoint, key[1], key[2]), h)
            self._solver = key
        hc = _f64(p.Hconst)
        if not np.array_equal(hc, self._hconst):
            if self._csc:
                k0 = _Csc(p.Hconst)
                _lib.check(L.jq_update_hconst_csc(h, ctypes.byref(k0.desc)), h)
            else:
                _lib.check(L.jq_update_hconst(h, _ptr(hc)), h)
            self._hconst = hc.copy()
        if wd.size != self._wd.size or not np.array_equal(wd, self._wd):      # (full weights)
            self._push_weights(wd)
            self._wd = wd.copy()
        utr, uti = _f64(p.Utarget_r), _f64(p.Utarget_i)
        if not (np.array_equal(utr, self._utr) and np.array_equal(uti, self._uti)):
            _lib.check(L.jq_update_target(h, _ptr(utr), _ptr(uti)), h)
            self._utr, self._uti = utr.copy(), uti.copy()
        # continuation adjoints: dVds (needed on the device only while sv_type != 1), then the type
        sv = int(getattr(p, "sv_type", 1))
        if sv != 1:
            dvr, dvi = _f64(p.dVds_r), _f64(p.dVds_i)
            if not (np.array_equal(dvr, self._dvr) and np.array_equal(dvi, self._dvi)):
                _lib.check(L.jq_update_dvds(h, _ptr(dvr), _ptr(dvi)), h)
                self._dvr, self._dvi = dvr.copy(), dvi.copy()
        if sv != self._sv_type:
            _lib.check(L.jq_set_sv_type(h, sv), h)
            self._sv_type = sv

    def set_option(self, name, value=None):
        """jq_set_option: change one option of this handle (value None: back to "not set"); plan-shaping options re-plan it"""
        name = name[3:].lower() if name.startswith("JQ_") else name
        v = _lib.JQ_OPTION_DEFAULT if value is None else int(value)
        _lib.check(_lib.load().jq_set_option(self.handle, name.encode(), v), self.handle)

    def get_option(self, name):
        v = ctypes.c_int64()
        rc = _lib.load().jq_get_option(self.handle, name.encode(), ctypes.byref(v))
        if rc != _lib.JQ_OK:
            raise KeyError(name)
        return None if v.value == _lib.JQ_OPTION_DEFAULT else v.value

    @property
    def num_compute_units(self):
        return _lib.load().jq_num_compute_units(self.handle)

    @property
    def rccl_world_size(self):
        return _lib.load().jq_rccl_world_size(self.handle)

    def plan_info(self):
        """jq_plan_info: structure found in the operators, control groups, batch-size thresholds of the kernel families and, under
        "last_kernels", the instantiation the last evaluation ran (object tags, slabs / quads per workgroup, variant flags; None before the
        first evaluation) (dict)"""
        import json
        L = _lib.load()
        n = L.jq_plan_info(self.handle, None, 0)
        if n < 0:
            _lib.check(n, self.handle)
        buf = ctypes.create_string_buffer(n + 1)
        L.jq_plan_info(self.handle, buf, n + 1)
        return json.loads(buf.value.decode())

    def last_timing(self):
        t = _lib.jq_timing()
        _lib.check(_lib.load().jq_last_timing(self.handle, ctypes.byref(t)), self.handle)
        return {k: getattr(t, k) for k, _ in _lib.jq_timing._fields_}


class Working_Arrays_M_HIP(Working_Arrays_HIP):
    """Working_Arrays_M (src/evalobjgrad.jl:445-500): selects the IMPLICIT-MIDPOINT method of traceobjgrad
    (:1042-1481) the way the reference does, by the type of `wa`.  `params.linear_solver` must be
    lsolver_object(solver=JACOBI_SOLVER_M, max_iter=..., tol=...) (test/runtests.jl:70); the leakage weights of this
    path are params.wmat (:1147), not params.wmat_real.  Device support: Ntot <= 96 (dense 96 x 96 operators excepted),
    N <= 16."""
    INTEGRATOR = Implicit_Midpoint
    SOLVERS = (JACOBI_SOLVER_M,)

    def _weights(self, p):
        return _f64(p.wmat)


def traceobjgrad(pcof0, params: objparams, wa: Working_Arrays_HIP, verbose: bool = False, evaladjoint: bool = True):
    """traceobjgrad(pcof0, params, wa, verbose, evaladjoint) -- src/evalobjgrad.jl:504-1038.

    evaladjoint (not verbose): (objfv, totalgrad, primaryobjf, secondaryobjf, traceInfidelity,
                                infidelgrad, leakgrad)                                     (:1033)
    neither:                   (objfv, primaryobjf, secondaryobjf)                         (:1035)
    verbose (not evaladjoint): (objfv, unitaryhistory[Ntot,N,nsteps+1] complex, fidelity)  (:1031)
    verbose and evaladjoint:   (objfv, totalgrad, unitaryhistory, fidelity, dfdp, wfinal[Ntot,N] complex)      (:1028)
        the reference's forward-sensitivity self check along d = e_kpar (params.kpar is 1-based, :205), built from the adjoint call,
        the verbose call and one jq_traceobj_jvp: totalgrad is bit-identical to the plain adjoint call, the history to the verbose
        call, wfinal = d(vr - i vi)/d(alpha_kpar) (the reference's wr1 - im wi).  dfdp = d(objfv)/d(alpha_kpar) WITHOUT a Tikhonov term,
        as objfv is: the reference adds gr[kpar] (:965), which at that point indexes the forcing work array -- a deviation on purpose.
        ValueError for sv_type != 1 (the reference's salpha1 is then a trace against dVds, :770) and for kpar outside 1 .. ncoeff;
        Stormer-Verlet with the Neumann solver and Diagonal weights only (traceobj_jvp).  gradient_check() below is the
        finite-difference companion (adjoint entries against central differences, all from one traceobjgrad_batch call).
    objfv excludes the Tikhonov term (added by the Ipopt callbacks, src/ipopt_interface.jl:96-98).
    """
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("traceobjgrad: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("traceobjgrad: wa was allocated for a different objparams")
    if verbose and evaladjoint:
        return _traceobjgrad_selfcheck(pcof0, params, wa)
    L, h = _lib.load(), wa.handle
    pcof = _f64(pcof0)
    n = pcof.size
    wa.sync_params()
    out4 = np.zeros(4)
    if verbose:
        shp = (params.Ntot, params.N, params.nsteps + 1)
        ur = np.zeros(int(np.prod(shp)))
        ui = np.zeros_like(ur)
        # history and objective from ONE forward sweep, like the reference's single pass
        _lib.check(L.jq_traceobj_verbose(h, _ptr(pcof), n, _ptr(out4), _ptr(ur), _ptr(ui)), h)
        hist = ur.reshape(shp, order="F") + 1j * ui.reshape(shp, order="F")
        return out4[0], hist, 1.0 - out4[3]
    if evaladjoint:
        tg, ig, lg = np.zeros(n), np.zeros(n), np.zeros(n)
        _lib.check(L.jq_traceobjgrad(h, _ptr(pcof), n, 1, _ptr(out4), _ptr(tg), _ptr(ig), _ptr(lg)), h)
        if params.objFuncType == 1:
            lg = np.zeros(0)      # the reference returns an empty leakgrad here (:808, :948-952)
        return out4[0], tg, out4[1], out4[2], out4[3], ig, lg
    _lib.check(L.jq_traceobjgrad(h, _ptr(pcof), n, 0, _ptr(out4), None, None, None), h)
    return out4[0], out4[1], out4[2]


def _traceobjgrad_selfcheck(pcof0, params, wa):
    """traceobjgrad(pcof0, params, wa, True, True): the 6-tuple of src/evalobjgrad.jl:1028 (see traceobjgrad)"""
    ncoeff = int(np.size(pcof0))
    kpar = getattr(params, "kpar", 1)
    if int(getattr(params, "sv_type", 1)) != 1:
        raise ValueError("traceobjgrad: verbose && evaladjoint needs sv_type == 1 (with another type the reference takes the tangent's "
                         "trace against dVds, src/evalobjgrad.jl:770)")
    if int(kpar) != kpar or not 1 <= int(kpar) <= ncoeff:
        raise ValueError("traceobjgrad: params.kpar = %r outside 1 .. %d" % (kpar, ncoeff))
    objfv, totalgrad = traceobjgrad(pcof0, params, wa, False, True)[:2]
    _, hist, fidelity = traceobjgrad(pcof0, params, wa, True, False)
    d = np.zeros(ncoeff)
    d[int(kpar) - 1] = 1.0
    r = traceobj_jvp(pcof0, d, params, wa, final=True)
    return objfv, totalgrad, hist, fidelity, float(r["d_objfv"][0]), r["W"][:, :, 0].copy()


def _directions(dirs, ncoeff, who="traceobj_jvp"):
    """dirs -> contiguous [ndir, ncoeff] array (one direction per row = the C ABI's column-major ncoeff x ndir).  A 1-D array or sequence
    of numbers is one direction, a 2-D array holds one direction per COLUMN.  ValueError (in the name of `who`) for everything else."""
    try:
        d = np.asarray(dirs, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("%s: dirs must be a vector or an ncoeff x ndir array of numbers (%s)" % (who, e))
    if d.ndim == 1:
        d = d[:, None]
    if d.ndim != 2:
        raise ValueError("%s: dirs must be a vector or an ncoeff x ndir array, not %d-dimensional" % (who, d.ndim))
    if d.shape[0] != ncoeff or d.shape[1] < 1:
        raise ValueError("%s: dirs has shape %r, expected (%d,) or (%d, ndir >= 1) (wa.nCoeff)" % (who, np.shape(dirs), ncoeff, ncoeff))
    if not np.all(np.isfinite(d)):
        raise ValueError("%s: dirs has an entry that is not finite" % who)
    return np.ascontiguousarray(d.T)


def traceobj_jvp(pcof, dirs, params: objparams, wa: Working_Arrays_HIP, final: bool = True):
    """The tangent (Jacobian-vector product) of the discrete forward map at pcof along directions of coefficient space, in one library
    call (jq_traceobj_jvp): a tangent-linear Stormer-Verlet sweep that differentiates the forward step as the device executes it, the
    truncated Neumann series included -- exact to rounding, where finite differences (gradient_check) agree to about 1e-7.

    dirs: one direction (ncoeff numbers) or an ncoeff x ndir array, one direction per column.
    Returns a dict: objfv, primaryobjf, secondaryobjf (the primal, no Tikhonov term), d_objfv[ndir], d_primary[ndir], d_secondary[ndir]
    and, with final, W[Ntot, N, ndir] complex = d(vr - i vi)(T)/d(alpha) . d (the reference's wr1 - im wi, src/evalobjgrad.jl:1028).
    Direction j does not depend on the other directions of the call.  Served: Stormer-Verlet with the Neumann solver, Diagonal weights,
    coupled and uncoupled controls, any objFuncType and sv_type (the objective depends on neither); the library refuses the
    implicit-midpoint integrator, the Jacobi solver and full leakage weights.  Shape errors raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("traceobj_jvp: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("traceobj_jvp: wa was allocated for a different objparams")
    ncoeff = int(wa.nCoeff)
    p = np.asarray(pcof, dtype=np.float64)
    if p.ndim != 1 or p.size != ncoeff:
        raise ValueError("traceobj_jvp: pcof has shape %r, expected (%d,) (wa.nCoeff)" % (p.shape, ncoeff))
    D = _directions(dirs, ncoeff)
    p = _f64(p)
    nd = D.shape[0]
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out4, dout = np.zeros(4), np.zeros((nd, 3))
    shp = (int(params.Ntot), int(params.N), nd)
    wr = np.zeros(int(np.prod(shp))) if final else None
    wi = np.zeros_like(wr) if final else None
    _lib.check(L.jq_traceobj_jvp(h, _ptr(p), ncoeff, _ptr(D), nd, _ptr(out4), _ptr(dout), _ptr(wr), _ptr(wi)), h)
    r = {"objfv": out4[0], "primaryobjf": out4[1], "secondaryobjf": out4[2],
         "d_objfv": dout[:, 0].copy(), "d_primary": dout[:, 1].copy(), "d_secondary": dout[:, 2].copy()}
    if final:
        r["W"] = wr.reshape(shp, order="F") + 1j * wi.reshape(shp, order="F")
    return r


def traceobjgrad_hvp(pcof, dirs, params: objparams, wa: Working_Arrays_HIP):
    """The gradient at pcof and its derivative along directions of coefficient space (Hessian-vector products) in one library call
    (jq_traceobjgrad_hvp):  hv[:, j] = d/d eps totalgrad(pcof + eps dirs[:, j]) at eps = 0, the exact derivative of the gradient
    traceobjgrad returns -- the backward sweep differentiated as the device executes it, truncated Neumann series included.  It is
    the Hessian of the discrete objective only as far as that gradient is its gradient: with a truncated series it is not symmetric
    at truncation level (order 0: 1e-1 .. 7e-1, order 4: 4e-7 .. 4e-4 relative, order 20: rounding); symmetrise it or raise the order where a
    symmetric operator is needed (hessian(..., symmetrize=True)).

    dirs: one direction (ncoeff numbers) or an ncoeff x ndir array, one direction per column (what traceobj_jvp accepts).
    Returns a dict: objfv, primaryobjf, secondaryobjf, totalgrad[ncoeff], hv[ncoeff, ndir] -- none with a Tikhonov term -- and for
    objFuncType != 1 hv_infid (the same for infidelgrad) and hv_leak = hv - hv_infid.  Direction j does not depend on the other
    directions of the call.  Served: Stormer-Verlet with the Neumann solver, Diagonal weights, coupled controls, sv_type 1; the library
    refuses the implicit-midpoint integrator, the Jacobi solver, full leakage weights, sv_type != 1 and uncoupled controls.  Shape
    errors raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("traceobjgrad_hvp: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("traceobjgrad_hvp: wa was allocated for a different objparams")
    ncoeff = int(wa.nCoeff)
    p = np.asarray(pcof, dtype=np.float64)
    if p.ndim != 1 or p.size != ncoeff:
        raise ValueError("traceobjgrad_hvp: pcof has shape %r, expected (%d,) (wa.nCoeff)" % (p.shape, ncoeff))
    D = _directions(dirs, ncoeff, "traceobjgrad_hvp")
    p = _f64(p)
    nd = D.shape[0]
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    two = params.objFuncType != 1
    out4, grad, hv = np.zeros(4), np.zeros(ncoeff), np.zeros((nd, ncoeff))
    hvi = np.zeros((nd, ncoeff)) if two else None
    _lib.check(L.jq_traceobjgrad_hvp(h, _ptr(p), ncoeff, _ptr(D), nd, _ptr(out4), _ptr(grad), _ptr(hv), _ptr(hvi)), h)
    r = {"objfv": out4[0], "primaryobjf": out4[1], "secondaryobjf": out4[2], "totalgrad": grad, "hv": hv.T.copy()}
    if two:
        r["hv_infid"] = hvi.T.copy()
        r["hv_leak"] = r["hv"] - r["hv_infid"]
    return r


def hessian(pcof, params: objparams, wa: Working_Arrays_HIP, symmetrize: bool = False):
    """The ncoeff x ncoeff Jacobian of totalgrad at pcof: all unit directions through one traceobjgrad_hvp call, column j = hv along
    e_j.  Not symmetric at truncation level of the Neumann series (traceobjgrad_hvp); symmetrize=True returns (J + J')/2."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("hessian: wa must be a Working_Arrays_HIP")
    J = traceobjgrad_hvp(pcof, np.eye(int(wa.nCoeff)), params, wa)["hv"]
    return 0.5 * (J + J.T) if symmetrize else J


def _pcof_columns(pcofs, ncoeff):
    """pcofs -> contiguous [npcof, ncoeff] array (one vector per row = the C ABI's column-major ncoeff x npcof).  A 2-D array holds one
    vector per COLUMN, a sequence one vector per element, a 1-D array is one vector.  ValueError for everything else."""
    if isinstance(pcofs, np.ndarray):
        if pcofs.ndim == 1:
            cols = [pcofs]
        elif pcofs.ndim == 2:
            cols = [pcofs[:, i] for i in range(pcofs.shape[1])]
        else:
            raise ValueError("traceobjgrad_batch: pcofs must be an ncoeff x npcof array or a sequence of vectors, not %d-dimensional" % pcofs.ndim)
    else:
        try:
            cols = [np.asarray(c, dtype=np.float64) for c in pcofs]
        except (TypeError, ValueError) as e:
            raise ValueError("traceobjgrad_batch: pcofs must be an ncoeff x npcof array or a sequence of vectors (%s)" % e)
    if len(cols) == 0:
        raise ValueError("traceobjgrad_batch: need at least one control vector")
    for i, c in enumerate(cols):
        if np.ndim(c) != 1 or np.size(c) != ncoeff:
            raise ValueError("traceobjgrad_batch: control vector %d has shape %r, expected (%d,) (wa.nCoeff)" % (i, np.shape(c), ncoeff))
    return np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64) for c in cols]))


def traceobjgrad_batch(pcofs, params: objparams, wa: Working_Arrays_HIP, evaladjoint: bool = True):
    """npcof independent evaluations traceobjgrad(pcofs[:, i], params, wa, False, evaladjoint) of ONE problem in one library call
    (jq_traceobjgrad_batch).  On the row-lane and cooperative-quad (latency) kernels with the Stormer-Verlet integrator the vectors share
    launches -- every workgroup reads the operator stream of its own vector --, everywhere else they run one after the other inside
    the call (wa.plan_info()["pcof_batch"] says which).  Column i is bit-identical to the single call's result on the same kernel variant.

    pcofs: an ncoeff x npcof array (one vector per column) or a sequence of equal-length vectors.
    evaladjoint: (objfv[n], totalgrad[ncoeff, n], primaryobjf[n], secondaryobjf[n], traceInfidelity[n], infidelgrad[ncoeff, n],
                  leakgrad[ncoeff, n] -- 0 x n for objFuncType == 1, like the single call's empty vector)
    else:        (objfv[n], primaryobjf[n], secondaryobjf[n])
    Shape errors raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("traceobjgrad_batch: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("traceobjgrad_batch: wa was allocated for a different objparams")
    ncoeff = int(wa.nCoeff)
    P = _pcof_columns(pcofs, ncoeff)
    n = P.shape[0]
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out4 = np.zeros((n, 4))
    if not evaladjoint:
        _lib.check(L.jq_traceobjgrad_batch(h, _ptr(P), ncoeff, n, 0, _ptr(out4), None, None, None), h)
        return out4[:, 0].copy(), out4[:, 1].copy(), out4[:, 2].copy()
    tg, ig, lg = np.zeros((n, ncoeff)), np.zeros((n, ncoeff)), np.zeros((n, ncoeff))
    _lib.check(L.jq_traceobjgrad_batch(h, _ptr(P), ncoeff, n, 1, _ptr(out4), _ptr(tg), _ptr(ig), _ptr(lg)), h)
    leak = np.zeros((0, n)) if params.objFuncType == 1 else np.ascontiguousarray(lg.T)
    return (out4[:, 0].copy(), np.ascontiguousarray(tg.T), out4[:, 1].copy(), out4[:, 2].copy(), out4[:, 3].copy(),
            np.ascontiguousarray(ig.T), leak)


def _drift_members(Hconsts, Ntot, who):
    """Hconsts -> contiguous [ndrift, Ntot * Ntot] array, member i column-major in row i (= the C ABI's Ntot x Ntot x ndrift).  An
    Ntot x Ntot x ndrift array holds one member per slice [:, :, i], a sequence one matrix per element, a 2-D array is one member.
    ValueError for everything else."""
    if isinstance(Hconsts, np.ndarray):
        if Hconsts.ndim == 2:
            mats = [Hconsts]
        elif Hconsts.ndim == 3:
            mats = [Hconsts[:, :, i] for i in range(Hconsts.shape[2])]
        else:
            raise ValueError("%s: Hconsts must be an Ntot x Ntot x ndrift array or a sequence of matrices, not %d-dimensional" % (who, Hconsts.ndim))
    else:
        try:
            mats = [np.asarray(M, dtype=np.float64) for M in Hconsts]
        except (TypeError, ValueError) as e:
            raise ValueError("%s: Hconsts must be an Ntot x Ntot x ndrift array or a sequence of matrices (%s)" % (who, e))
    if len(mats) == 0:
        raise ValueError("%s: need at least one member drift" % who)
    for i, M in enumerate(mats):
        if np.ndim(M) != 2 or np.shape(M) != (Ntot, Ntot):
            raise ValueError("%s: member %d has shape %r, expected (%d, %d) (params.Ntot)" % (who, i, np.shape(M), Ntot, Ntot))
    return np.ascontiguousarray(np.stack([_f64(M) for M in mats]))


def traceobjgrad_drifts(pcof, params: objparams, wa: Working_Arrays_HIP, Hconsts, evaladjoint: bool = True):
    """ndrift evaluations traceobjgrad(pcof, params with Hconst = Hconsts[:, :, i], wa, False, evaladjoint) of ONE control vector in one
    library call (jq_traceobjgrad_drifts) -- the loop `params.Hconst = H_i; traceobjgrad(...)` of the reference's scripts.  On the row-lane
    and cooperative-quad (latency) kernels with the Stormer-Verlet integrator and the Neumann solver the members share launches -- every
    workgroup reads the operator stream of its own member's drift --, everywhere else the handle's drift is swapped per member inside the
    call (wa.plan_info()["drift_batch"] says which).  Column i is bit-identical to that loop on the same kernel variant and chunk length;
    params.Hconst and the handle's drift are what they were afterwards.  A member outside the structure the handle was planned for
    re-plans it once, for the union of all patterns (see include/juqbox_hip.h).

    Hconsts: an Ntot x Ntot x ndrift array or a sequence of Ntot x Ntot matrices.
    Returns the arrays of traceobjgrad_batch, one column per member.  Shape errors raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("traceobjgrad_drifts: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("traceobjgrad_drifts: wa was allocated for a different objparams")
    ncoeff = int(wa.nCoeff)
    H = _drift_members(Hconsts, int(params.Ntot), "traceobjgrad_drifts")
    p = np.asarray(pcof, dtype=np.float64)
    if p.ndim != 1 or p.size != ncoeff:
        raise ValueError("traceobjgrad_drifts: pcof has shape %r, expected (%d,) (wa.nCoeff)" % (p.shape, ncoeff))
    p = _f64(p)
    n = H.shape[0]
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out4 = np.zeros((n, 4))
    if not evaladjoint:
        _lib.check(L.jq_traceobjgrad_drifts(h, _ptr(p), ncoeff, _ptr(H), n, 0, _ptr(out4), None, None, None), h)
        return out4[:, 0].copy(), out4[:, 1].copy(), out4[:, 2].copy()
    tg, ig, lg = np.zeros((n, ncoeff)), np.zeros((n, ncoeff)), np.zeros((n, ncoeff))
    _lib.check(L.jq_traceobjgrad_drifts(h, _ptr(p), ncoeff, _ptr(H), n, 1, _ptr(out4), _ptr(tg), _ptr(ig), _ptr(lg)), h)
    leak = np.zeros((0, n)) if params.objFuncType == 1 else np.ascontiguousarray(lg.T)
    return (out4[:, 0].copy(), np.ascontiguousarray(tg.T), out4[:, 1].copy(), out4[:, 2].copy(), out4[:, 3].copy(),
            np.ascontiguousarray(ig.T), leak)


def _ncontrols(params):
    """the controls a mix acts on: the coupled pairs, or the uncoupled controls of a problem that has those"""
    return max(int(getattr(params, "Ncoupled", 0)), int(getattr(params, "Nunc", 0)))


def amplitude_mix(scales):
    """Amplitude miscalibration as control mixes: scales[i, k] is the factor with which p_k, q_k of member i arrive (1 + delta_k); returns
    the [Nc, Nc, nmember] array of diagonal mixes C_i = diag(scales[i]).  A vector is one member.  ValueError for other shapes."""
    try:
        s = np.asarray(scales, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("amplitude_mix: scales must be an [nmember, Nc] array of numbers (%s)" % e)
    if s.ndim == 1:
        s = s[None, :]
    if s.ndim != 2 or s.shape[0] < 1 or s.shape[1] < 1:
        raise ValueError("amplitude_mix: scales must be an [nmember, Nc] array, not shape %r" % (s.shape,))
    n, nc = s.shape
    C = np.zeros((nc, nc, n))
    for i in range(n):
        C[:, :, i] = np.diag(s[i])
    return C


def _mix_members(ctrl_mix, Nc, who):
    """ctrl_mix -> contiguous [nmember, Nc * Nc] array, member i column-major in row i (= the C ABI's Nc x Nc x nmember).  An Nc x Nc x
    nmember array holds one member per slice [:, :, i], a sequence one matrix per element, a 2-D array is one member.  ValueError for
    everything else, entries that are not finite included."""
    if isinstance(ctrl_mix, np.ndarray):
        if ctrl_mix.ndim == 2:
            mats = [ctrl_mix]
        elif ctrl_mix.ndim == 3:
            mats = [ctrl_mix[:, :, i] for i in range(ctrl_mix.shape[2])]
        else:
            raise ValueError("%s: ctrl_mix must be an Nc x Nc x nmember array or a sequence of matrices, not %d-dimensional" % (who, ctrl_mix.ndim))
    else:
        try:
            mats = [np.asarray(M) for M in ctrl_mix]
            mats = [M if np.iscomplexobj(M) else np.asarray(M, dtype=np.float64) for M in mats]      # (complex: refused below, not cast)
        except (TypeError, ValueError) as e:
            raise ValueError("%s: ctrl_mix must be an Nc x Nc x nmember array or a sequence of real matrices (%s)" % (who, e))
    if len(mats) == 0:
        raise ValueError("%s: need at least one member mix" % who)
    for i, M in enumerate(mats):
        if np.ndim(M) != 2 or np.shape(M) != (Nc, Nc):
            raise ValueError("%s: mix %d has shape %r, expected (%d, %d) (the controls of params)" % (who, i, np.shape(M), Nc, Nc))
        if np.iscomplexobj(M):
            raise ValueError("%s: mix %d is complex; only real mixing matrices are served" % (who, i))
        if not np.all(np.isfinite(M)):
            raise ValueError("%s: mix %d has an entry that is not finite" % (who, i))
    return np.ascontiguousarray(np.stack([_f64(M) for M in mats]))


def _members(params, Hconsts, ctrl_mix, who):
    """(drifts [n, Ntot * Ntot] or None, mixes [n, Nc * Nc] or None, n) of a member ensemble; ValueError for wrong shapes"""
    if Hconsts is None and ctrl_mix is None:
        raise ValueError("%s: give Hconsts, ctrl_mix or both (neither: the plain evaluation, traceobjgrad)" % who)
    H = _drift_members(Hconsts, int(params.Ntot), who) if Hconsts is not None else None
    C = _mix_members(ctrl_mix, _ncontrols(params), who) if ctrl_mix is not None else None
    if H is not None and C is not None and H.shape[0] != C.shape[0]:
        raise ValueError("%s: %d member drifts but %d member mixes" % (who, H.shape[0], C.shape[0]))
    return H, C, (H if H is not None else C).shape[0]


def traceobjgrad_members(pcof, params: objparams, wa: Working_Arrays_HIP, Hconsts=None, ctrl_mix=None, evaladjoint: bool = True):
    """nmember evaluations of ONE control vector in one library call (jq_traceobjgrad_members) whose member i has the real Nc x Nc mixing
    matrix C_i = ctrl_mix[:, :, i] of the controls -- operator l is driven by sum_k C_i[l, k] (p_k, q_k); diag(1 + delta): miscalibrated
    amplitudes (amplitude_mix), off-diagonal entries: crosstalk -- and, with Hconsts, its own drift.  Column i equals traceobjgrad on the
    problem whose operators are Hsym'_k = sum_l C_i[l, k] Hsym_l, Hanti'_k likewise, and is bit-identical to that member evaluated alone.
    Routing as traceobjgrad_drifts (wa.plan_info()["member_batch"]); ctrl_mix=None is traceobjgrad_drifts.

    Hconsts: None (the drift of params) or as for traceobjgrad_drifts; ctrl_mix: None (identity), an Nc x Nc x nmember array or a sequence
    of Nc x Nc matrices.  Returns the arrays of traceobjgrad_batch, one column per member.  Shape errors raise ValueError before any
    library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("traceobjgrad_members: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("traceobjgrad_members: wa was allocated for a different objparams")
    ncoeff = int(wa.nCoeff)
    H, C, n = _members(params, Hconsts, ctrl_mix, "traceobjgrad_members")
    p = np.asarray(pcof, dtype=np.float64)
    if p.ndim != 1 or p.size != ncoeff:
        raise ValueError("traceobjgrad_members: pcof has shape %r, expected (%d,) (wa.nCoeff)" % (p.shape, ncoeff))
    p = _f64(p)
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out4 = np.zeros((n, 4))
    if not evaladjoint:
        _lib.check(L.jq_traceobjgrad_members(h, _ptr(p), ncoeff, _ptr(H), _ptr(C), n, 0, _ptr(out4), None, None, None), h)
        return out4[:, 0].copy(), out4[:, 1].copy(), out4[:, 2].copy()
    tg, ig, lg = np.zeros((n, ncoeff)), np.zeros((n, ncoeff)), np.zeros((n, ncoeff))
    _lib.check(L.jq_traceobjgrad_members(h, _ptr(p), ncoeff, _ptr(H), _ptr(C), n, 1, _ptr(out4), _ptr(tg), _ptr(ig), _ptr(lg)), h)
    leak = np.zeros((0, n)) if params.objFuncType == 1 else np.ascontiguousarray(lg.T)
    return (out4[:, 0].copy(), np.ascontiguousarray(tg.T), out4[:, 1].copy(), out4[:, 2].copy(), out4[:, 3].copy(),
            np.ascontiguousarray(ig.T), leak)


# ---- controls given as samples on the time grid (include/juqbox_hip.h, "controls given as samples") ----
def _sample_table(pq, params, who):
    """pq -> the flat [2 Nc x nt] column-major table of the C ABI; ValueError for another shape or entries that are not finite"""
    shape = (2 * int(params.Ncoupled), 2 * int(params.nsteps) + 1)
    try:
        a = np.asarray(pq, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("%s: pq must be a 2 Ncoupled x (2 nsteps + 1) array of numbers (%s)" % (who, e))
    if a.shape != shape:
        raise ValueError("%s: pq has shape %r, expected %r (2 Ncoupled x (2 nsteps + 1): row 2k is p_k, row 2k + 1 is q_k)" % (who, a.shape, shape))
    if not np.all(np.isfinite(a)):
        raise ValueError("%s: pq has an entry that is not finite" % who)
    return _f64(a), shape


def control_sample_times(params: objparams, wa: Working_Arrays_HIP):
    """The 2 nsteps + 1 time points the integrator reads controls at (jq_sample_times): t[2n] is the time of step n as the forward sweep
    accumulates it, t[2n + 1] = t[2n] + dt / 2.  Column J of a sample table belongs to t[J]."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("control_sample_times: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("control_sample_times: wa was allocated for a different objparams")
    t = np.zeros(2 * int(params.nsteps) + 1)
    rc = _lib.load().jq_sample_times(wa.handle, _ptr(t), t.size)
    if rc != _lib.JQ_OK:
        raise _lib.JuqboxHipError(rc, "jq_sample_times: the handle has another number of time steps than params")
    return t


def control_samples(pcof, params: objparams, wa: Working_Arrays_HIP):
    """The handle's own spline-with-carrier controls of pcof on the grid of control_sample_times (jq_control_samples): a 2 Ncoupled x
    (2 nsteps + 1) array, row 2k = p_k, row 2k + 1 = q_k -- bit for bit what an evaluation of pcof streams, so traceobjgrad_samples of it
    returns the objective of traceobjgrad(pcof) bit for bit.  Coupled controls only."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("control_samples: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("control_samples: wa was allocated for a different objparams")
    p = _f64(pcof)
    shape = (2 * int(params.Ncoupled), 2 * int(params.nsteps) + 1)
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    pq = np.zeros(shape[0] * shape[1])
    _lib.check(L.jq_control_samples(h, _ptr(p), p.size, _ptr(pq)), h)
    return pq.reshape(shape, order="F")


def traceobjgrad_samples(pq, params: objparams, wa: Working_Arrays_HIP, evaladjoint: bool = True):
    """traceobjgrad for controls given as VALUES on the time grid instead of spline coefficients (jq_traceobjgrad_samples): pq is a
    2 Ncoupled x (2 nsteps + 1) array, column J the controls (p_1, q_1, p_2, q_2, ...) at control_sample_times()[J].  The gradients are
    those of the discrete objective with respect to every entry of pq, in the shape of pq; any parameterisation theta -> pq is then a chain
    rule on the host (spline_sample_matrix is the one of the library's own splines; torch_controls.SampledObjective the autograd form).
    Sweeps, plan and kernel families are those of traceobjgrad.  The implicit-midpoint integrator reads the odd columns only: its
    gradient columns at even J are exact zeros.

    evaladjoint: (objfv, totalgrad, primaryobjf, secondaryobjf, traceInfidelity, infidelgrad, leakgrad) -- leakgrad empty for
                 objFuncType == 1, like traceobjgrad's
    else:        (objfv, primaryobjf, secondaryobjf)
    No Tikhonov term.  Shape errors and entries that are not finite raise ValueError before any library call; the library refuses
    uncoupled controls."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("traceobjgrad_samples: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("traceobjgrad_samples: wa was allocated for a different objparams")
    tab, shape = _sample_table(pq, params, "traceobjgrad_samples")
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out4 = np.zeros(4)
    if not evaladjoint:
        _lib.check(L.jq_traceobjgrad_samples(h, _ptr(tab), shape[1], 0, _ptr(out4), None, None, None), h)
        return out4[0], out4[1], out4[2]
    tg, ig, lg = np.zeros(tab.size), np.zeros(tab.size), np.zeros(tab.size)
    _lib.check(L.jq_traceobjgrad_samples(h, _ptr(tab), shape[1], 1, _ptr(out4), _ptr(tg), _ptr(ig), _ptr(lg)), h)
    leak = np.zeros((0, 0)) if params.objFuncType == 1 else lg.reshape(shape, order="F")
    return out4[0], tg.reshape(shape, order="F"), out4[1], out4[2], out4[3], ig.reshape(shape, order="F"), leak


def _sample_tables(pqs, params, who):
    """pqs -> ([ntab, 2 Nc * nt] array, table i column-major in row i, and the shape of one table).  An [ntab, 2 Ncoupled, 2 nsteps + 1]
    array or a sequence of tables; ValueError for anything else, through _sample_table per table"""
    try:
        tabs = list(pqs)
    except TypeError as e:
        raise ValueError("%s: pqs must be an [ntab, 2 Ncoupled, 2 nsteps + 1] array or a sequence of tables (%s)" % (who, e))
    if len(tabs) == 0:
        raise ValueError("%s: need at least one table" % who)
    flat, shape = [], None
    for t in tabs:
        f, shape = _sample_table(t, params, who)
        flat.append(f)
    return np.ascontiguousarray(np.stack(flat)), shape


def _sample_columns(params, out4, tg, ig, lg, shape, evaladjoint):
    """the return tuple of traceobjgrad_batch for n groups over sample tables: gradients [n, 2 Nc, nt]"""
    if not evaladjoint:
        return out4[:, 0].copy(), out4[:, 1].copy(), out4[:, 2].copy()
    n = out4.shape[0]

    def tables(g):
        return np.ascontiguousarray(g.reshape((n, shape[1], shape[0])).transpose(0, 2, 1))

    leak = np.zeros((n, 0, 0)) if params.objFuncType == 1 else tables(lg)
    return out4[:, 0].copy(), tables(tg), out4[:, 1].copy(), out4[:, 2].copy(), out4[:, 3].copy(), tables(ig), leak


def traceobjgrad_samples_batch(pqs, params: objparams, wa: Working_Arrays_HIP, evaladjoint: bool = True):
    """ntab evaluations traceobjgrad_samples(pqs[i], params, wa) in one library call (jq_traceobjgrad_samples_batch).  On the row-lane and
    cooperative-quad (latency) kernels with the Stormer-Verlet integrator and the Neumann solver the tables share launches -- every
    workgroup reads the operator stream of its own table --, everywhere else they run one after the other inside the call
    (wa.plan_info()["sampled_batch"] says which).  Entry i equals the single call's at the same chunk length.

    pqs: an [ntab, 2 Ncoupled, 2 nsteps + 1] array or a sequence of tables.
    Returns the tuple of traceobjgrad_samples with a leading axis of length ntab on every element (gradients [ntab, 2 Ncoupled, nt];
    leakgrad empty for objFuncType == 1).  Shape errors and entries that are not finite raise ValueError before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("traceobjgrad_samples_batch: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("traceobjgrad_samples_batch: wa was allocated for a different objparams")
    T, shape = _sample_tables(pqs, params, "traceobjgrad_samples_batch")
    n, ln = T.shape
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out4 = np.zeros((n, 4))
    if not evaladjoint:
        _lib.check(L.jq_traceobjgrad_samples_batch(h, _ptr(T), shape[1], n, 0, _ptr(out4), None, None, None), h)
        return _sample_columns(params, out4, None, None, None, shape, False)
    tg, ig, lg = np.zeros((n, ln)), np.zeros((n, ln)), np.zeros((n, ln))
    _lib.check(L.jq_traceobjgrad_samples_batch(h, _ptr(T), shape[1], n, 1, _ptr(out4), _ptr(tg), _ptr(ig), _ptr(lg)), h)
    return _sample_columns(params, out4, tg, ig, lg, shape, True)


def traceobjgrad_samples_members(pq, params: objparams, wa: Working_Arrays_HIP, Hconsts=None, ctrl_mix=None, evaladjoint: bool = True):
    """ONE sample table under nmember members in one library call (jq_traceobjgrad_samples_members): member i has the drift
    Hconsts[:, :, i] (None: the drift of params) and the real Nc x Nc control mix C_i = ctrl_mix[:, :, i] (None: identity) -- operator l is
    driven by sum_k C_i[l, k] (p_k, q_k)(t_J), as in traceobjgrad_members.  Member i's gradients are those with respect to the SHARED
    table (its mix folded in by C_i').  Routing as traceobjgrad_samples_batch (wa.plan_info()["sampled_batch"]); params.Hconst and the
    handle's drift are what they were afterwards.

    Returns the tuple of traceobjgrad_samples_batch, one entry per member.  Shape errors and entries that are not finite raise ValueError
    before any library call."""
    if not isinstance(wa, Working_Arrays_HIP):
        raise TypeError("traceobjgrad_samples_members: wa must be a Working_Arrays_HIP")
    if wa.params is not params:
        raise ValueError("traceobjgrad_samples_members: wa was allocated for a different objparams")
    tab, shape = _sample_table(pq, params, "traceobjgrad_samples_members")
    H, C, n = _members(params, Hconsts, ctrl_mix, "traceobjgrad_samples_members")
    L, h = _lib.load(), wa.handle
    wa.sync_params()
    out4 = np.zeros((n, 4))
    if not evaladjoint:
        _lib.check(L.jq_traceobjgrad_samples_members(h, _ptr(tab), shape[1], _ptr(H), _ptr(C), n, 0, _ptr(out4), None, None, None), h)
        return _sample_columns(params, out4, None, None, None, shape, False)
    tg, ig, lg = np.zeros((n, tab.size)), np.zeros((n, tab.size)), np.zeros((n, tab.size))
    _lib.check(L.jq_traceobjgrad_samples_members(h, _ptr(tab), shape[1], _ptr(H), _ptr(C), n, 1, _ptr(out4), _ptr(tg), _ptr(ig), _ptr(lg)), h)
    return _sample_columns(params, out4, tg, ig, lg, shape, True)


def _direction_tables(dirs, params, who):
    """dirs -> the flat [ndir][2 Nc x nt] stack of column-major tables of the C ABI and ndir.  One table (the shape of pq) or a stack
    (2 Ncoupled, 2 nsteps + 1, ndir); ValueError for another shape or entries that are not finite"""
    shape = (2 * int(params.Ncoupled), 2 * int(params.nsteps) + 1)
    try:
        d = np.asarray(dirs, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("%s: dirs must be a table like pq or a stack of tables (%s)" % (who, e))
    if d.ndim == 2:
        d = d[:, :, None]
    if d.ndim != 3 or d.shape[:2] != shape or d.shape[2] < 1:
        raise ValueError("%s: dirs has shape %r, expected %r or %r with ndir >= 1" % (who, np.shape(dirs), shape, shape + ("ndir",)))
    if not np.all(np.isfinite(d)):
        raise ValueError("%s: dirs has an entry that is not finite" % who)
    return _f64(d), d.shape[2]


def traceobjgrad_samples_hvp(pq, dirs, params: objparams, wa: Working_Arrays_HIP):
    """The gradient of traceobjgrad_samples at the table pq and its derivative along direction tables (Hessian-vector products in
    sample space) in one library call: the one-node form of eval_f_g_grad_samples_hvp (jq_eval_f_g_grad_samples_hvp with node 0, weight
    1).  hv[:, :, j] = d/d eps totalgrad(pq + eps dirs[:, :, j]) at eps = 0, the exact derivative of the gradient the library returns,
    truncated Neumann series included -- not symmetric at truncation level and never symmetrised (traceobjgrad_hvp).

    dirs: one table in the shape of pq or a stack (2 Ncoupled, 2 nsteps + 1, ndir).  Returns a dict: objfv, primaryobjf, secondaryobjf,
    totalgrad in the shape of pq, hv and hv_infid (the same for infidelgrad; objFuncType == 1: equal to hv) of shape
    (2 Ncoupled, 2 nsteps + 1, ndir).  No Tikhonov term.  Shape errors and entries that are not finite raise ValueError before any
    library call."""
    from .ipopt_interface import eval_f_g_grad_samples_hvp
    r = eval_f_g_grad_samples_hvp(pq, dirs, params, wa, _who="traceobjgrad_samples_hvp")
    return {"objfv": r["infidelity"] + r["leak"], "primaryobjf": r["infidelity"], "secondaryobjf": r["leak"],
            "totalgrad": r["infid_grad"] + r["leak_grad"], "hv": r["hv_infid"] + r["hv_leak"], "hv_infid": r["hv_infid"]}


def spline_sample_matrix(params: objparams, ncoeff: int, times):
    """The dense B = d pq / d pcof of the library's own parameterisation (bcarrier2, src/bsplines.jl:211-304) on the given times, in
    numpy: (2 Ncoupled len(times)) x ncoeff, row 2 Ncoupled J + f = control function f (2k: p_k, 2k + 1: q_k) at times[J], so that
        pq = (B @ pcof).reshape((2 Ncoupled, len(times)), order="F")        and        dJ/dpcof = B.T @ G.ravel(order="F")
    for a sample gradient G of traceobjgrad_samples.  With times = control_sample_times() the first agrees with control_samples(pcof)
    to rounding (the device evaluates sin / cos and the sums in its own order).  The controls are linear in pcof, so B does not depend
    on it.  Host only: no handle, no device."""
    Nc, Nfreq = int(params.Ncoupled), int(params.Nfreq)
    ncoeff = int(ncoeff)
    if Nc < 1 or ncoeff % (2 * Nc * Nfreq) != 0 or ncoeff // (2 * Nc * Nfreq) < 3:
        raise ValueError("spline_sample_matrix: ncoeff = %d is not 2 Ncoupled Nfreq D1 with D1 >= 3" % ncoeff)
    D1 = ncoeff // (2 * Nc * Nfreq)
    t = np.asarray(times, dtype=np.float64).ravel()
    dtknot = float(params.T) / (D1 - 2)      # bcparams (src/bsplines.jl:174)
    width = 3.0 * dtknot
    k = np.clip(np.ceil(t / dtknot + 2.0).astype(np.int64), 3, D1)      # 1-based knot index (:224-225)
    tau = [(t - dtknot * ((k - i) - 1.5)) / width for i in range(3)]      # centres k, k - 1, k - 2 (:238-250)
    b = [9.0 / 8.0 + 4.5 * tau[0] + 4.5 * tau[0] * tau[0], 0.75 - 9.0 * tau[1] * tau[1], 9.0 / 8.0 - 4.5 * tau[2] + 4.5 * tau[2] * tau[2]]
    Cfreq = np.asarray(params.Cfreq, dtype=np.float64).reshape(-1, Nfreq)
    B = np.zeros((2 * Nc * t.size, ncoeff))
    J = np.arange(t.size)
    for osc in range(Nc):
        for freq in range(Nfreq):
            off1 = 2 * osc * Nfreq * D1 + freq * 2 * D1
            off2 = off1 + D1
            cs, sn = np.cos(Cfreq[osc, freq] * t), np.sin(Cfreq[osc, freq] * t)
            for i in range(3):
                col = k - 1 - i
                rp, rq = 2 * Nc * J + 2 * osc, 2 * Nc * J + 2 * osc + 1
                B[rp, off1 + col] += b[i] * cs      # p = fbs1 cos - fbs2 sin (:260)
                B[rp, off2 + col] += -b[i] * sn
                B[rq, off1 + col] += b[i] * sn      # q = fbs1 sin + fbs2 cos (:258)
                B[rq, off2 + col] += b[i] * cs
    return B


def gradient_check(pcof0, params: objparams, wa: Working_Arrays_HIP, kpars, h: float = 1e-6):
    """The adjoint gradient against central differences: returns (totalgrad[kpars], fd) with
    fd[j] = (f(p + h e_k) - f(p - h e_k)) / 2h for k = kpars[j], f = objfv.  All 2 len(kpars) + 1 evaluations are ONE
    traceobjgrad_batch call (vector 0: p itself, then the + and - vector of every k).  A finite-difference companion of the reference's
    `verbose && evaladjoint` self check, which traceobjgrad serves with the exact tangent (traceobj_jvp)."""
    p0 = np.asarray(pcof0, dtype=np.float64).ravel()
    ks = [int(k) for k in np.atleast_1d(kpars)]
    if p0.size != int(wa.nCoeff):
        raise ValueError("gradient_check: pcof0 has %d elements, wa.nCoeff = %d" % (p0.size, wa.nCoeff))
    for k in ks:
        if not 0 <= k < p0.size:
            raise ValueError("gradient_check: index %d outside 0 .. %d" % (k, p0.size - 1))
    vecs = [p0]
    for k in ks:
        for sgn in (1.0, -1.0):
            v = p0.copy()
            v[k] += sgn * h
            vecs.append(v)
    objfv, tg = traceobjgrad_batch(vecs, params, wa, True)[:2]
    fd = np.array([(objfv[1 + 2 * j] - objfv[2 + 2 * j]) / (2.0 * h) for j in range(len(ks))])
    return tg[ks, 0].copy(), fd
