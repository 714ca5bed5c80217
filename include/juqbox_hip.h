/*
 * juqbox_hip.h -- C ABI of libjuqbox_hip.so: the MI355X (gfx950) replacement for Juqbox.jl's
 * Stormer-Verlet `traceobjgrad` hot path.
 *
 * The reference has NO foreign-function boundary on this path (it is 100% Julia); the seam this
 * ABI plugs into is the multiple-dispatch method
 *     traceobjgrad(pcof0, params::objparams, wa::Working_Arrays, verbose, evaladjoint)
 * (src/evalobjgrad.jl:504) and its ensemble caller eval_f_g_grad! (src/ipopt_interface.jl:24-70).
 * A new working-array type whose traceobjgrad method `ccall`s the entry points below is the
 * drop-in (INTEGRATION.md shows the Julia shim).  File:line citations are relative to the
 * reference repository root.
 *
 * Conventions
 *  - all matrices are Float64, COLUMN-MAJOR (Julia Array layout); indices in comments are 1-based
 *    when they quote the reference.
 *  - every pointer argument is a HOST pointer owned by the caller and only read/written during the
 *    call; the library copies what it keeps.  The handle owns all device memory.
 *  - every function returns 0 on success, a negative JQ_E* code otherwise; jq_last_error() gives
 *    the message.  No C++ exception crosses this boundary.
 *  - one handle = one in-flight call (not re-entrant), like the reference's single-threaded use.
 *  - the handle is bound to the HIP device that was current when jq_create() ran
 *    (jq_set_device() selects it; one process per GPU under torch.distributed / RCCL), or to the
 *    devices given to jq_create_multi() (one process, several GPUs, RCCL inside the library).
 */
#ifndef JUQBOX_HIP_H
#define JUQBOX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header: the layout of jq_problem / jq_timing and the set of entry points.  jq_abi_version() returns the
 * value the LIBRARY was built with; every binding (juqbox.jl_amd/_lib.py, julia/hip_backend.jl, examples/c_abi_demo.c) compares
 * the two when it loads the library, so a caller compiled against an older header fails loudly instead of having
 * jq_last_timing write past its struct.  History: 1 = round 1; 2 = jq_timing.mfma_backward, jq_problem.Hunc_ops / Rfreq;
 * 3 = jq_timing.ms_allreduce / ms_shard_min / ms_shard_max, jq_abi_version(), up to JQ_MAX_CONTROLS control Hamiltonians;
 * 4 = jq_problem.Hconst_csc / Hsym_csc / Hanti_csc (sparse operator storage), jq_csc, jq_update_hconst_csc, jq_update_wmat (full /
 *     complex leakage weights);
 * 5 = per-handle options instead of environment variables (jq_create_opts, jq_create_multi_opts, jq_set_option, jq_get_option),
 *     jq_timing.reserved renamed kernel_variant, jq_rccl_world_size; no size limits on Ntot, the number of control Hamiltonians or
 *     the rank of a full weight matrix; full leakage weights with the Jacobi solver;
 * 6 = continuation adjoints: jq_update_dvds, jq_set_sv_type, jq_get_sv_type (params.dVds_r / dVds_i / sv_type); later, with no
 *     change of a layout or of an existing entry point: jq_s_uniform (host-only structure test), jq_traceobjgrad_batch (many control
 *     vectors of one problem in one call), jq_eval_f_g_grad_batch (many control vectors x the nodes of one ensemble in one call),
 *     jq_traceobjgrad_drifts / jq_eval_f_g_grad_drifts (one control vector over an ensemble of arbitrary drift Hamiltonians in one call),
 *     jq_traceobjgrad_members / jq_eval_f_g_grad_members (... over members that differ in their drift, in a real mixing matrix of the
 *     controls -- amplitude miscalibration, crosstalk -- or in both), jq_traceobj_jvp (the tangent of the discrete forward map along
 *     directions of coefficient space: the reference's verbose && evaladjoint forward-sensitivity sweep), jq_traceobjgrad_hvp (the
 *     derivative of the gradient along directions of coefficient space: Hessian-vector products), jq_eval_f_g_grad_hvp (the same for
 *     the two gradients of a risk-neutral ensemble: the nodes in the lanes, the directions in the grid), jq_eval_f_g_grad_drifts_hvp (the
 *     same for an ensemble of arbitrary drift Hamiltonians: every wave reads the operator stream of its own member),
 *     jq_eval_f_g_grad_members_hvp (the same for members with a control mix as well: every wave reads the tangent stream of its own
 *     member too), jq_sample_times / jq_control_samples / jq_traceobjgrad_samples / jq_eval_f_g_grad_samples (the objective of a table
 *     of control values on the time grid and its gradient per entry: any parameterisation by a host-side chain rule). */
#define JQ_ABI_VERSION 6

#define JQ_MAX_CONTROLS 16 /* control Hamiltonians the fast kernels hold in registers; more: cooperative kernels (no limit)    */
#define JQ_MAX_WRANK 16    /* rank of a full leakage-weight matrix every kernel family takes; beyond: slab / cooperative kernels */

#define JQ_OK 0
#define JQ_EINVAL -1      /* bad argument (the reference's @assert / error(...) sites)            */
#define JQ_EDIM -2        /* DimensionMismatch: nCoeff != length(pcof) (src/bsplines.jl:178-181)   */
#define JQ_EUNSUPPORTED -3/* valid for the reference but outside what the HIP path implements     */
#define JQ_EHIP -4        /* HIP runtime failure                                                   */
#define JQ_ENOMEM -5

typedef struct jq_handle jq_handle;

/*
 * A sparse operator exactly as Julia's SparseMatrixCSC{Float64,Int64} stores it (the reference keeps Hconst, Hsym_ops, Hanti_ops
 * like this when objparams(...; use_sparse=true), src/evalobjgrad.jl:249-262, and multiplies them through KS!/KS_alloc,
 * :2392-2426, :3072-3105): m x n, column j holds the entries nzval[colptr[j]-1 .. colptr[j+1]-2] in the rows
 * rowval[...] -- colptr and rowval are 1-BASED Int64, like the fields of the Julia struct, so the binding passes the three
 * vectors without copying or shifting them.  Repeated (row, column) entries are summed.
 */
typedef struct jq_csc {
    int64_t m, n;            /* size; must be Ntot x Ntot                                           */
    const int64_t *colptr;   /* [n + 1], colptr[0] == 1, colptr[n] == nnz + 1                       */
    const int64_t *rowval;   /* [nnz], 1 <= rowval <= m                                             */
    const double *nzval;     /* [nnz]                                                               */
} jq_csc;

/*
 * Problem description = the objparams fields the device needs (src/evalobjgrad.jl:53-148;
 * SURVEY.md section 8 row a13).  Hard-wired in the reference and therefore not passed:
 * use_bcarrier=true (:208), pFidType=2 (:164), order=2/stages=1 (:507,:644).  (sv_type and dVds: jq_set_sv_type, jq_update_dvds.)
 */
typedef struct jq_problem {
    int32_t Ntot;          /* prod(Ne+Ng): Hilbert dimension incl. guard levels                   */
    int32_t N;             /* prod(Ne): number of initial-condition columns                       */
    int32_t Ncoupled;      /* number of (Hsym_ops[k], Hanti_ops[k]) control pairs, <= JQ_MAX_CONTROLS (with more than four the
                              backward sweep runs once per group of four controls)                   */
    int32_t Nfreq;         /* carrier frequencies per control = size(Cfreq,2)                     */
    int32_t nsteps;        /* params.nsteps                                                        */
    int32_t neumann_terms; /* params.linear_solver.max_iter (NEUMANN_SOLVER, linear_solvers.jl:37) */
    int32_t objFuncType;   /* 1: infidelity+leak; 2/3: second, unforced adjoint gives infidelgrad  */
    int32_t Nunc;          /* number of uncoupled controls Hunc_ops (0, or > 0 with Ncoupled == 0: src/evalobjgrad.jl:176) */
    double T;              /* gate duration                                                        */
    const double *Hconst;    /* [Ntot x Ntot]                                                      */
    const double *Hsym_ops;  /* [Ncoupled][Ntot x Ntot]                                            */
    const double *Hanti_ops; /* [Ncoupled][Ntot x Ntot]                                            */
    const double *Uinit;     /* [Ntot x N]                                                         */
    const double *Utarget_r; /* [Ntot x N]  real(Utarget) (rotating frame)                         */
    const double *Utarget_i; /* [Ntot x N]  imag(Utarget)                                          */
    const double *wmat_real_diag; /* [Ntot] diag(params.wmat_real); Diagonal weights only          */
    const double *Cfreq;     /* [(Ncoupled + Nunc) x Nfreq] carrier (angular) frequencies          */
    /* Uncoupled controls (the lab-frame evaluation of a pulse, e.g. examples/cnot2-lab.jl): KS! adds
     * 2 (p_q(t) cos(2 pi Rfreq[q] t) - q_q(t) sin(2 pi Rfreq[q] t)) * Hunc_ops[q] to K when Hunc_ops[q] is symmetric,
     * to S when it is antisymmetric (src/evalobjgrad.jl:2373-2387; anything else is the reference's ArgumentError,
     * :186-196 -> JQ_EINVAL).  Parity-unpinned in the reference (no golden): checked against the CPU oracle.
     * Gradients (Stormer-Verlet integrator): the exact gradient of the discrete objective, the traces of Hunc_ops[q] weighted
     * with grad ft = 2 cos(.) grad p_q - 2 sin(.) grad q_q.  The reference's own code for this (adjoint_grad_calc!, :2620-2656)
     * is not a usable reference -- it differentiates control functions of an older numbering (func = 2 Ncoupled - 1 + q, no
     * rotation factor), i.e. not what KS! applies, and throws for objFuncType != 1 (gradSize, :801) -- so this gradient is
     * pinned by finite differences of the objective (tests/test_uncoupled.py).  Implicit midpoint: JQ_EUNSUPPORTED (the
     * reference's adjoint_grad_calc_m has no term for uncoupled controls). */
    const double *Hunc_ops;  /* [Nunc][Ntot x Ntot], NULL when Nunc == 0                           */
    const double *Rfreq;     /* [Nunc] rotation frequencies params.Rfreq, NULL when Nunc == 0      */
    /* Sparse storage of the coupled operators (use_sparse = true): when Hconst == NULL, Hconst_csc is read instead; likewise
     * Hsym_csc / Hanti_csc (arrays of Ncoupled descriptors) when Hsym_ops / Hanti_ops == NULL.  The library plans its kernels
     * from the nonzero structure either way, so the dense and the CSC form of the same operators give bit-identical results.
     * All three NULL (with the dense pointers set): a dense problem, as before. */
    const jq_csc *Hconst_csc;
    const jq_csc *Hsym_csc;  /* [Ncoupled]                                                         */
    const jq_csc *Hanti_csc; /* [Ncoupled]                                                         */
} jq_problem;

/* Timing of the last evaluation, measured with HIP events on the library's stream. */
typedef struct jq_timing {
    double ms_total;        /* whole call on the device (generate + propagate + reduce)            */
    double ms_propagate;    /* sum over launches of the forward+backward propagator kernels        */
    double ms_generate;     /* everything else: control evaluation, K(t)/S(t) tile stream, reductions*/
    double ms_forward;      /* sum over k_forward launches                                         */
    double ms_backward;     /* sum over k_backward launches                                        */
    int64_t n_forward_launches;
    int64_t n_backward_launches;
    int64_t mfma_executed;  /* v_mfma_f64_16x16x4 instructions issued by the propagators (all waves)*/
    int64_t svts;           /* state-vector-time-steps processed (columns x nsteps), SURVEY 8(d)   */
    int32_t kernel_family;  /* propagators used: 0 slab (MFMA, wave per slab), 1 cooperative (MFMA, row split),
                               2 lane (VALU, lane per column), 3 row-lane (VALU, lane per (row, column)),
                               4 row-lane, implicit midpoint, 5 cooperative, implicit midpoint,
                               6 quad layout (MFMA 4x4x4, four columns per wave; JQ_BW_T4), 7 the same, implicit midpoint,
                               8 cooperative quad (one 16-row block per wave: single evaluations / small ensembles),
                               9 the same, implicit midpoint (N = 4)                                              */
    int32_t kernel_size;    /* template size parameter: NT (16-row tiles) for 0/1, NP for 2, NPJ for 3       */
    int32_t kernel_band;    /* block band of the MFMA families (9 = JQ_BW_OD: diagonal off-diagonal blocks,
                               8 = JQ_BW_T4: 4x4 diagonal blocks + diagonal couplings, 7 = the same, quad layout,
                               10 = dense blocks on the cooperative-quad kernels: 17 .. 32 levels without the structure) */
    int32_t kernel_variant; /* variant of the backward sweep.  Family 8: workgroups (CUs) per column quad -- 3: state re-integration, adjoint
                               step and trace products pipelined over three workgroups (single evaluations, <= 80 cnot3 samples);
                               2: state re-integration | adjoint step + trace products (81 .. 128 samples); 22: more column quads than
                               CUs, backward sweep on k_backward_qsplit with two quads per workgroup.  Family 6: 24 = one slab per
                               workgroup with the state and the adjoint chain of a quad on two waves (k_backward_qsplit).  Family 3: 32 = the backward
                               sweep's state and adjoint chain on two waves (k_backward_rowlane2), 33 = state chain, adjoint chain and traces on
                               three or four waves (k_backward_rowlane3).  Else 0 */
    int64_t mfma_backward;  /* the part of mfma_executed issued by the k_backward launches                  */
    double ms_allreduce;    /* multi-device handles: host wall time of the ONE all-reduce (group start .. result on the host);
                               0 for single-device handles (their caller runs the collective)                  */
    double ms_shard_min;    /* multi-device handles: smallest / largest ms_total over the devices that had a shard */
    double ms_shard_max;    /* (single-device handles: both = ms_total)                                        */
} jq_timing;

/* ---- lifetime --------------------------------------------------------------------------------*/
int jq_device_count(void);
int jq_set_device(int device);
/* Replaces: objparams(...) constructor + Working_Arrays(params, nCoeff) (src/evalobjgrad.jl:152-343,
 * :405-440): validates sizes, uploads the operators as MFMA A-fragment tile images. */
int jq_create(const jq_problem *problem, jq_handle **out);
/*
 * The same with OPTIONS for the new handle: "name=value,name=value" (integers; ',', ';' or blanks separate; NULL or "" = none).
 * Options replace the JQ_* environment variables of ABI <= 4: they belong to ONE handle, are parsed once, and nothing in the
 * environment changes kernel selection behind the caller's back any more.  The defaults are the measured optimum; options exist for
 * tests (kernel variants that must agree bit for bit), bisection and experiments -- a production caller passes none.  The table of
 * names is in INTEGRATION.md section 4 (generated from juqbox.jl_amd/csrc/jq_options.h).  The ONE environment variable that still
 * reaches kernel selection is JQ_OPTIONS (same syntax, applied in front of `options`): for callers that cannot pass a string, e.g. an
 * unmodified script.  Errors: JQ_EINVAL for an unknown name or a malformed string (message: jq_last_error(NULL)); options that exist
 * in experiment builds only (-DJQ_EXPERIMENTS) are refused by a release library.
 */
int jq_create_opts(const jq_problem *problem, const char *options, jq_handle **out);
/*
 * Change one option of a handle (multi-device handles: of every device).  Options that shape the plan (structure, kernel families,
 * chunking: marked "plan" in the table) re-plan the handle in place -- same pointer, settings kept, like jq_update_hconst with a drift
 * outside the planned structure; the others take effect with the next evaluation.  value == JQ_OPTION_DEFAULT: back to "not set".
 * Errors: JQ_EINVAL unknown name; JQ_EUNSUPPORTED an experiment-only option in a release library.
 */
#define JQ_OPTION_DEFAULT INT64_MIN
int jq_set_option(jq_handle *h, const char *name, int64_t value);
/* the value in force (the default when the option is not set; JQ_OPTION_DEFAULT for an unset option without a default) */
int jq_get_option(const jq_handle *h, const char *name, int64_t *value);
void jq_destroy(jq_handle *h);
/* Message of the last failing call on `h` (h == NULL: last jq_create failure of this thread). */
const char *jq_last_error(const jq_handle *h);

/*
 * Multi-device handle: ONE process drives `ndev` GPUs of a node -- what the single-threaded Julia caller of
 * eval_f_g_grad! (src/ipopt_interface.jl:38-65: a serial loop over the quadrature nodes) needs to use 8 GPUs without
 * MPI.  devices: `ndev` distinct HIP device ids, or NULL for 0..ndev-1.  Every entry point below accepts such a handle:
 *   jq_eval_f_g_grad   block-partitions the nquad nodes over the devices (jq_shard_bounds), evaluates the shards
 *                      concurrently and sums the packed results with ONE ncclAllReduce (RCCL over xGMI, sum, fp64);
 *   jq_traceobj_sweep  partitions the nodes the same way (independent outputs: no collective);
 *   jq_traceobjgrad / jq_state_history / jq_state_populations (ONE evaluation: not shardable) run on the first device;
 *   jq_set_* / jq_update_* apply to every device.
 * librccl.so is loaded at run time by this call (JQ_EUNSUPPORTED if it cannot be found); single-device users never
 * need it.  Errors: JQ_EINVAL if ndev < 1, ndev > jq_device_count() or a device id repeats.
 * The environment variable JQ_RCCL_LIB=<path> makes this call load exactly that librccl.
 * TEST MODE: with the option multi_same_device=1 (jq_create_multi_opts, or JQ_OPTIONS) the `ndev` (<= 16) sub-handles may share physical GPUs (ids modulo
 * the visible count) and the all-reduce is replaced by a host-side sum in device order -- host threads, streams, sharding and
 * packing are the production code.  It exists so that the ndev > 1 paths run on a one-GPU box (tests/test_gpu_round3.py).
 */
int jq_create_multi(const jq_problem *problem, const int32_t *devices, int32_t ndev, jq_handle **out);
/* ... with options (jq_create_opts) for every device's handle; multi_same_device=1 selects the TEST MODE below */
int jq_create_multi_opts(const jq_problem *problem, const int32_t *devices, int32_t ndev, const char *options, jq_handle **out);
/* ranks of the RCCL communicator behind a multi-device handle (ncclCommCount): ndev when RCCL saw every device; 0 for single-device
 * handles and in the same-device test mode (no communicator) */
int jq_rccl_world_size(const jq_handle *h);
/* number of GPUs behind a handle (1 for jq_create handles) */
int jq_num_devices(const jq_handle *h);
/* compute units of the handle's GPU (256 on MI355X): the granularity of the batch-size staircase -- one round of the throughput
 * kernels is 3 slabs (= 3 * (16 / N) samples for N <= 16) per compute unit */
int jq_num_compute_units(const jq_handle *h);
/* HIP device id a handle is bound to (the first device of a multi-device handle; -1 for NULL): device pointers handed to
 * jq_eval_f_g_grad_dev must live on THIS device */
int jq_handle_device(const jq_handle *h);
/*
 * The contiguous block partition of `nquad` ensemble samples over `world` shards (devices of a multi-device handle, or
 * the ranks of a torch.distributed / MPI job with one process per GPU): shard `rank` owns samples [*lo, *hi); the first
 * nquad % world shards get one sample more.  Pure host arithmetic (no GPU needed).
 */
int jq_shard_bounds(int32_t nquad, int32_t rank, int32_t world, int32_t *lo, int32_t *hi);

/* ---- mutations scripts apply to `params` after construction ----------------------------------*/
/* params.linear_solver.max_iter = m (estimate_Neumann!, src/evalobjgrad.jl:2922-2925) */
int jq_set_neumann_terms(jq_handle *h, int32_t m);
/* params.linear_solver = lsolver_object(solver=..., max_iter=..., tol=...) (src/linear_solvers.jl:28-78):
 * solver_id 1 = NEUMANN_SOLVER (neumann!, :81-106; tol ignored), 2 = JACOBI_SOLVER (jacobi!, :110-153; `tol` is
 * the already nrhs-scaled tolerance, :40).  Other ids: JQ_EUNSUPPORTED.
 * JACOBI_SOLVER convergence is tested per evaluation like the reference's norm(T - X) over the Ntot x N block -- for N <= 64 with
 * Ntot <= 96 (round 5: N > 16 columns take ceil(N / 16) slabs; up to four of them are the waves of ONE workgroup, which adds their
 * residual norms before it decides).  With N > 64, or with Ntot > 96 (cooperative kernels: a slab per workgroup), every 16-column
 * part is still tested on its own: parts may stop at different iterations, and the result then differs from the reference's by
 * O(tol) instead of agreeing to rounding (tests/test_gpu_round4.py holds such a case to c * tol). */
int jq_set_linear_solver(jq_handle *h, int32_t solver_id, int32_t max_iter, double tol);
/* params.Integrator_id (src/evalobjgrad.jl:100, constants Stormer_Verlet = 1, Implicit_Midpoint = 2) selects which
 * traceobjgrad method runs: 1 = the Stormer-Verlet path (default), 2 = the implicit-midpoint path
 * (traceobjgrad for Working_Arrays_M, src/evalobjgrad.jl:1042-1481) with the fixed-point solver
 * lsolver_object(solver=JACOBI_SOLVER_M, max_iter, tol) (src/linear_solvers.jl:52-55, :156-270).  For integrator 2 the
 * leakage weights are params.wmat (pass them with jq_update_wmat_diag).  Kernels: row-lane (Ntot <= 16, N <= 4), cooperative MFMA
 * (any Ntot and batch size -- run-time-size kernels beyond 256 levels; both images of a step resident in LDS when they fit, else -- dense 96 x 96, Ntot > 96 -- read from
 * HBM / L2 per product), quad-layout and cooperative-quad kernels for the 4 x 4 x n structure with N = 1, 2, 4.  N > 16 columns per
 * evaluation (round 4): the solver's per-evaluation stopping rule needs an evaluation's columns in one workgroup, so ONE cooperative
 * workgroup per evaluation walks over its 16-column parts (a correctness-first path: the parts' iterates live in HBM / L2). */
int jq_set_integrator(jq_handle *h, int32_t integrator_id, int32_t max_iter, double tol);
/* change_target!(params, new_Utarget) (src/evalobjgrad.jl:1492) */
int jq_update_target(jq_handle *h, const double *Utarget_r, const double *Utarget_i);
/*
 * Continuation adjoints (ABI 6).  objparams(...; dVds = D) sets params.sv_type = 2 (src/evalobjgrad.jl:312-319), set_adjoint_Sv_type!
 * (:1516-1520) sets 1, 2 or 3, and the Stormer-Verlet adjoint then starts differently (:815-844).  With T the target, D = dVds and
 * s_X = tr(X' V(T))/N:
 *   JQ_SV_TARGET 1: lambda(T) = s_T conj(T)/N  (the default)
 *   JQ_SV_TERM1  2: lambda(T) = s_T conj(D)/N  ("term 1 of d/ds grad G")
 *   JQ_SV_TERM2  3: lambda(T) = s_D conj(T)/N  ("term 2 of d/ds grad G")
 *   JQ_SV_BOTH   4: lambda(T) = (s_T conj(D) + s_D conj(T))/N -- not in the reference: the gradient is affine in lambda(T), so ONE backward
 *                   sweep returns (total gradient of type 2) + (total gradient of type 3) - (leakage-forcing part, which both contain),
 *                   and for objFuncType != 1 the sum of the two infidelity gradients; the leakage gradient is that of every type.
 * The objective values are taken against the target in every type; only gradients change.  Forward-only evaluations ignore the type.
 * jq_update_dvds: dVds_r / dVds_i are Ntot x N, column major, like jq_update_target's arguments.  A new handle holds a copy of its
 * target (:312-314).  jq_update_target does NOT touch dVds: "dVds follows the target while sv_type == 1" is change_target!'s rule
 * (:1492-1506), which the bindings apply.  With type 1 dVds is kept on the host only -- type-1 callers pay nothing.
 * jq_set_sv_type: JQ_EINVAL outside 1 .. 4.  The reference's implicit-midpoint traceobjgrad (:1042-1481) never reads sv_type or dVds,
 * so a type other than 1 together with integrator 2 is JQ_EUNSUPPORTED from whichever of jq_set_sv_type / jq_set_integrator comes
 * second (the refused call changes nothing).  jq_get_sv_type: the type in force (JQ_EINVAL for NULL).
 */
#define JQ_SV_TARGET 1
#define JQ_SV_TERM1 2
#define JQ_SV_TERM2 3
#define JQ_SV_BOTH 4
int jq_update_dvds(jq_handle *h, const double *dVds_r, const double *dVds_i);
int jq_set_sv_type(jq_handle *h, int32_t sv_type);
int jq_get_sv_type(const jq_handle *h);
/* params.Hconst is mutated freely (src/ipopt_interface.jl:41-44, run_all.jl:13-15).  Kernels, operator images and LDS plan are
 * chosen from the operators' nonzero structure at jq_create; a new drift with entries outside that structure re-plans the handle
 * in place (same pointer, settings kept) -- slower kernels may result, never an error for a valid Hconst. */
int jq_update_hconst(jq_handle *h, const double *Hconst);
/* the same with the new drift in sparse storage (use_sparse = true problems) */
int jq_update_hconst_csc(jq_handle *h, const jq_csc *Hconst);
/* params.wmat_real = orig_wmatsetup(Ne,Ng) (e.g. test/cases/cnot3-setup.jl:253); returns the handle to Diagonal weights */
int jq_update_wmat_diag(jq_handle *h, const double *wmat_real_diag);
/*
 * Full leakage weights: params.wmat_real / params.wmat_imag as Ntot x Ntot matrices, what objparams(...;
 * use_custom_forbidden=true, forb_states, forb_weights) builds (src/evalobjgrad.jl:214-232: W = sum_k w_k f_k f_k^H).  They enter
 * the objective through penalf2aTrap / penalf2a (full versions, :2183-2223) and penalf2imag (:2226-2228) at :700, :716-718 and the
 * adjoint forcing through the products at :862, :882-888.  wmat_imag may be NULL (= 0).
 * The device exploits the structure: W = wmat_real + i wmat_imag must be Hermitian (wmat_real symmetric, wmat_imag
 * antisymmetric -- what the constructor produces) and is eigen-decomposed on the host into its rank terms
 * lam_k f_k f_k^H; W x then costs two column dot products and two axpys per term instead of dense products.  A diagonal
 * wmat_real with wmat_imag == 0 is recognised and takes the Diagonal fast path (as jq_update_wmat_diag).
 * Stormer-Verlet integrator (the implicit-midpoint path of the reference reads params.wmat, which is always Diagonal, :90, :1155), with
 * the Neumann or the Jacobi solver; a rank above JQ_MAX_WRANK or the Jacobi solver route the handle to the slab / cooperative /
 * run-time-size kernels (ABI 5; before: refused).  Errors: JQ_EUNSUPPORTED for a non-Hermitian W or a handle set to the
 * implicit-midpoint integrator; evaluations on kernel families without the low-rank terms are refused, never
 * silently evaluated with other weights.  Parity-unpinned in the reference (no test or golden uses the branch): checked against
 * the CPU oracle, whose gradient is checked by finite differences (tests/test_dense_wmat.py).
 * Latency path (4 x 4 x n structure, at most one column quad per compute unit; round 5): a W that fits FOUR SLOTS -- real (wmat_imag
 * = 0, i.e. real forbidden states) of rank <= 4, or complex of rank <= 2 -- runs on the cooperative-quad kernels (kernel_family 8): one
 * cnot3 evaluation 0.161 s (Diagonal weights: 0.153 s) with the backward sweep on three workgroups per quad, real W on one workgroup
 * (more than 128 samples, or the split not available) 0.204 s.  A complex W needs the split kernels; without them, and any W of higher
 * rank, on the quad-layout kernels (family 6: 0.55 s + ~ 0.1 s per further forbidden state).
 */
int jq_update_wmat(jq_handle *h, const double *wmat_real, const double *wmat_imag);

/* ---- the hot path ----------------------------------------------------------------------------*/
/*
 * Replaces traceobjgrad(pcof0, params, wa, false, evaladjoint) (src/evalobjgrad.jl:504-1038).
 * out4 = { objfv, primaryobjf, secondaryobjf, traceInfidelity } (return tuple :1033/:1035; objfv
 * excludes the Tikhonov term, which the Ipopt callbacks add: src/ipopt_interface.jl:96-98).
 * totalgrad / infidelgrad / leakgrad: caller-allocated length ncoeff, written when evaladjoint != 0
 * (leakgrad is zero-filled and infidelgrad == totalgrad when objFuncType == 1, where the reference
 * returns an empty leakgrad, :948-952).  May be NULL when evaladjoint == 0.
 * Errors: JQ_EINVAL for the reference's error at :604-606, JQ_EDIM for bcparams' DimensionMismatch.
 */
int jq_traceobjgrad(jq_handle *h, const double *pcof, int32_t ncoeff, int32_t evaladjoint, double *out4,
                    double *totalgrad, double *infidelgrad, double *leakgrad);
/*
 * npcof independent evaluations traceobjgrad(pcofs[:, i], params, wa, false, evaladjoint) of ONE problem: multi-start optimisation,
 * batched line searches, finite-difference checks, population optimisers, parameter scans of a pulse.
 * pcofs: [ncoeff x npcof] column-major; out4: [4 x npcof]; totalgrad / infidelgrad / leakgrad: [ncoeff x npcof]
 * (conventions per column exactly those of jq_traceobjgrad; NULL allowed when evaladjoint == 0).
 * Column i of every output equals what jq_traceobjgrad returns for pcofs[:, i] under the handle's current settings (sv_type, weights,
 * solver, target, objFuncType) -- bit for bit on the same kernel variant.
 * Grouped batches: with the Stormer-Verlet integrator and the Neumann solver on the latency kernels -- row-lane (family 3) and
 * cooperative quad (family 8, its dense policy included) -- the vectors SHARE launches: every workgroup belongs to one vector and
 * reads the operator tile stream of that vector.  At most one vector's workgroups per compute unit go into a launch (option
 * pcof_batch_max: fewer), larger batches run in rounds.  Column counts that would put two vectors into one wave / column quad
 * (N = 3, 5, 6, 7 ...; cooperative quad: N not dividing 16 and not beyond it), every other kernel family and the implicit-midpoint
 * integrator evaluate the vectors one after the other inside the call.  jq_plan_info reports what the last call did ("pcof_batch").
 * Errors: those of the single call (JQ_EINVAL / JQ_EDIM for the coefficient count, JQ_EINVAL for NULL arguments), JQ_EINVAL for
 * npcof < 1; a refused call writes nothing.  Multi-device handles shard the vectors like jq_traceobj_sweep (jq_shard_bounds).
 */
int jq_traceobjgrad_batch(jq_handle *h, const double *pcofs, int32_t ncoeff, int32_t npcof, int32_t evaladjoint,
                          double *out4, double *totalgrad, double *infidelgrad, double *leakgrad);

/*
 * Replaces the verbose branch's state history (src/evalobjgrad.jl:677-680, :748-752, returned at
 * :1031 as usaver + im*usavei): ur/ui are [Ntot x N x (nsteps+1)], ui = -vi.
 */
int jq_state_history(jq_handle *h, const double *pcof, int32_t ncoeff, double *ur, double *ui);
/*
 * The whole verbose, evaladjoint = false call traceobjgrad(pcof0, params, wa, true, false) (return tuple
 * src/evalobjgrad.jl:1031) from ONE forward sweep: the history as above plus out4 = { objfv, primaryobjf,
 * secondaryobjf, traceInfidelity } of the same sweep (out4 may be NULL).  The verbose, evaladjoint = true call (return tuple :1028)
 * is this call, jq_traceobjgrad and one jq_traceobj_jvp (below) along e_kpar.
 */
int jq_traceobj_verbose(jq_handle *h, const double *pcof, int32_t ncoeff, double *out4, double *ur, double *ui);

/*
 * The tangent (Jacobian-vector product) of the discrete forward map at pcof along ndir directions of coefficient space -- what the
 * verbose && evaladjoint branch of traceobjgrad computes along e_kpar with its forward-sensitivity sweep (src/evalobjgrad.jl:682-689,
 * :723-745, :768-784, returned at :1028; step_fwdGrad!, src/StormerVerlet.jl:151-250), here for any direction and exact to rounding:
 * a tangent-linear Stormer-Verlet sweep propagates (state, tangent) in dual-number arithmetic, differentiating the forward step as
 * the device executes it, the truncated Neumann series included.
 *   dirs : [ncoeff x ndir] column-major, one direction per column
 *   out4 : the primal { objfv, primaryobjf, secondaryobjf, traceInfidelity } (no Tikhonov term)
 *   dout : [3 x ndir] column-major: d(objfv), d(primaryobjf), d(secondaryobjf) along each direction, with
 *          d(primaryobjf) = -2 Re(conj(s) sd), s = tr(Vtg' V)/N, sd = tr(Vtg' Vd)/N
 *   wr,wi: [Ntot x N x ndir] each, real and imaginary part of d(vr - i vi)(T)/d(alpha) . d (the reference's wr1 - im wi); both NULL:
 *          not wanted
 * Direction j does not depend on the other directions of the call (the same operations in the same order).  Directions beyond what
 * one launch holds next to the primal operator stream run in rounds; jq_plan_info reports "jvp": {directions_per_launch, chunk_steps,
 * rounds} after a call, jq_last_timing the launches as the run-time-size kernels report theirs (family 1, tile rows, band 15).
 * Served: the Stormer-Verlet integrator with the Neumann solver (order 0 included), Diagonal weights, coupled and uncoupled controls,
 * any objFuncType and sv_type (the objective depends on neither), any Ntot and N, the handle's own drift.  Refused with
 * JQ_EUNSUPPORTED, never served by something else: the implicit-midpoint integrator, the Jacobi solver (its stopping rule has no
 * derivative), full leakage weights (jq_update_wmat).  JQ_EINVAL for NULL required pointers, ndir < 1 or exactly one of wr / wi; the
 * codes of jq_traceobjgrad for the coefficient count.  A refused call writes nothing and leaves the handle as it was.  Multi-device
 * handles run the call on their first device.
 */
int jq_traceobj_jvp(jq_handle *h, const double *pcof, int32_t ncoeff, const double *dirs, int32_t ndir, double *out4, double *dout,
                    double *wr, double *wi);

/*
 * The gradient at pcof and its derivative along ndir directions of coefficient space (Hessian-vector products; the reference has no
 * second-order path):
 *   hv(alpha; d) = d/d eps totalgrad(alpha + eps d) at eps = 0,
 * the exact derivative of the gradient jq_traceobjgrad returns, obtained by differentiating the backward sweep as the device executes
 * it (tangent-linear forward sweep as jq_traceobj_jvp, then the adjoint step in dual-number arithmetic, truncated Neumann series
 * included).  This is the Hessian of the discrete objective only as far as that gradient is its gradient: the adjoint is the exact
 * transpose of the forward scheme for exact linear solves, with a truncated series the operator is not symmetric at truncation level
 * (|e.Jd - d.Je| / |e.Jd| on random 7-step problems: order 0 1e-1 .. 7e-1, order 1 1e-3 .. 2e-2, order 4 4e-7 .. 4e-4, order 20 1e-15 .. 3e-14).
 * Callers who need a symmetric operator symmetrise it or raise the order; the library does not symmetrise silently.
 *   dirs     : [ncoeff x ndir] column-major, one direction per column
 *   out4     : the primal { objfv, primaryobjf, secondaryobjf, traceInfidelity } (no Tikhonov term), as jq_traceobj_jvp
 *   grad     : [ncoeff] totalgrad
 *   hv       : [ncoeff x ndir] column-major: d(totalgrad) along each direction (no Tikhonov term, like totalgrad)
 *   hv_infid : NULL, or [ncoeff x ndir]: the same for infidelgrad (objFuncType != 1: an unforced second backward pass; objFuncType 1:
 *              infidelgrad is totalgrad, so is this)
 * Direction j does not depend on the other directions of the call nor on the rounds they run in (jq_plan_info "hvp":
 * {directions_per_launch, chunk_steps, rounds} after a call; jq_last_timing counts forward and backward launches).  More than four
 * controls run in control groups.  Served: the Stormer-Verlet integrator with the Neumann solver (order 0 included), Diagonal weights,
 * coupled controls, sv_type 1, any objFuncType, Ntot and N, the handle's own drift.  Refused with JQ_EUNSUPPORTED: the
 * implicit-midpoint integrator, the Jacobi solver, full leakage weights (jq_update_wmat), sv_type != 1, uncoupled controls.
 * JQ_EINVAL for NULL required pointers or ndir < 1; the codes of jq_traceobjgrad for the coefficient count.  A refused call writes
 * nothing and leaves the handle as it was.  Multi-device handles run the call on their first device.
 */
int jq_traceobjgrad_hvp(jq_handle *h, const double *pcof, int32_t ncoeff, const double *dirs, int32_t ndir, double *out4, double *grad,
                        double *hv, double *hv_infid);

/*
 * jq_eval_f_g_grad and the derivative of its two gradients along ndir directions of coefficient space: Hessian-vector products of a
 * risk-neutral ensemble (the objective of eval_f_g_grad!, src/ipopt_interface.jl:24-70),
 *   hv_infid[:, j] = sum_i w_i d/d eps infidelgrad_i(alpha + eps d_j),  hv_leak[:, j] = sum_i w_i d/d eps leakgrad_i(alpha + eps d_j)  at eps = 0,
 * node i being the evaluation with Hconst + nodes[i] diag(shift).  Exact derivatives of the gradients jq_eval_f_g_grad returns, truncated
 * Neumann series included: not symmetric at truncation level, and the library does not symmetrise silently (jq_traceobjgrad_hvp).
 *   dirs     : [ncoeff x ndir] column-major, one direction per column
 *   nodes, weights : [nquad]; shift : [Ntot] or NULL (the reference's 0.01 * 10^(j-2))
 *   out2, infid_grad, leak_grad : as jq_eval_f_g_grad with compute_adjoint (objFuncType 1: infid_grad carries totalgrad, leak_grad zeros)
 *   hv_infid, hv_leak : [ncoeff x ndir] column-major (objFuncType 1: hv_infid carries the derivative of totalgrad, hv_leak zeros)
 * Lane route: Ntot <= 6 with at most four controls (and option lane != 0) runs on the tangent-linear lane kernels -- all N nquad columns
 * x the directions of a round in ONE launch per chunk, independent of the options lane_min / lane_max (one node is served too).
 * Row-lane route: Ntot 9 .. 16 with at most four controls (and option lane != 0) runs on the tangent-linear row-lane kernels -- four
 * columns per wave, ceil(N nquad / 4) waves x the directions of a round in ONE launch per chunk, independent of option rowlane_max.
 * Quad route: Ntot > 16 with the 4 x 4 x n structure of the handle's own plan (NT = 2 .. 6 blocks of 16 rows, e.g. cnot3; never an embedded
 * twin), at most four controls and the quad-layout kernels enabled (option quad != 0) runs on the tangent-linear quad-layout kernels -- four
 * columns per wave, up to four waves of a direction per workgroup sharing its operator images in LDS, x the directions of a round in ONE
 * launch per chunk.
 * Sequential route: everything else jq_traceobjgrad_hvp serves (Ntot 7 and 8, which have no tangent kernel; Ntot > 16 without that structure,
 * with NT = 7, 8 or through an embedded twin; options lane=0 / quad=0; more than four controls) runs the nodes one after the other on its
 * run-time-size sweeps -- correct and no faster.  Direction j does not depend on the other directions of the
 * call nor on the rounds they run in (option stream_bytes).  jq_plan_info "ens_hvp": {route: "lane" | "rowlane" | "quad" | "sequential",
 * directions_per_launch, chunk_steps, rounds} after a call; jq_last_timing reports the lane family and NP on the lane route, the
 * row-lane family and NPJ on the row-lane route, the quad family, NT and band 7 on the quad route, and counts
 * forward and backward launches; "last_kernels" names the instantiations.  Refused with JQ_EUNSUPPORTED: what jq_traceobjgrad_hvp
 * refuses (implicit midpoint, the Jacobi solver, full leakage weights, sv_type != 1, uncoupled controls).  JQ_EINVAL for NULL pointers
 * (all but shift are required), ndir < 1 or nquad < 1; the codes of jq_traceobjgrad for the coefficient count.  A refused call writes
 * nothing and leaves the handle as it was.  Multi-device handles run the call on their first device.
 */
int jq_eval_f_g_grad_hvp(jq_handle *h, const double *pcof, int32_t ncoeff, const double *dirs, int32_t ndir, const double *nodes,
                         const double *weights, int32_t nquad, const double *shift, double *out2, double *infid_grad, double *leak_grad,
                         double *hv_infid, double *hv_leak);

/*
 * jq_eval_f_g_grad_hvp over the members of a drift ensemble instead of over eps-nodes: the weighted sums sum_i w_i of infidelity and leak,
 * of the two gradients and of their derivatives along ndir directions, member i being the handle's problem with Hconst = drifts[:, :, i]
 * (the members of jq_traceobjgrad_drifts / jq_eval_f_g_grad_drifts).
 *   dirs    : [ncoeff x ndir] column-major, one direction per column
 *   drifts  : [Ntot x Ntot x ndrift] column-major member drifts; weights : [ndrift]
 *   out2, infid_grad, leak_grad, hv_infid, hv_leak : as jq_eval_f_g_grad_hvp
 * Routes as jq_eval_f_g_grad_hvp (lane, row-lane, quad), with a member where that call has a node: a member brings an operator stream of
 * its own and its N columns start at fresh waves -- lane route: a wave of 64 column lanes per member; row-lane and quad routes:
 * ceil(N / 4) waves per member, on the quad route padded to whole workgroups (a workgroup shares its operator images) -- and as many
 * members as the stream budget (option stream_bytes) leaves streams for next to the directions share a launch; the others follow in
 * further member rounds.  Every member must lie inside the structure the handle was planned for (what jq_update_hconst would accept
 * without re-planning); otherwise, and wherever jq_eval_f_g_grad_hvp runs its nodes one after the other, the members run one after the
 * other on the run-time-size sweeps (route "sequential").  The call never re-plans the handle and never touches its drift or operator
 * images.  jq_plan_info "drift_hvp": {route, members_per_launch, directions_per_launch, chunk_steps, rounds} after a call (rounds:
 * direction rounds x member rounds); "ens_hvp", "hvp" and "drift_batch" keep the values of their own calls.  jq_last_timing and
 * "last_kernels" as jq_eval_f_g_grad_hvp.  Refused with JQ_EUNSUPPORTED: what that call refuses.  JQ_EINVAL for NULL pointers (all are
 * required), ndir < 1 or ndrift < 1; the codes of jq_traceobjgrad for the coefficient count.  A refused call writes nothing and leaves
 * the handle as it was.  Multi-device handles run the call on their first device.  Not served: members x eps-nodes, sharding over
 * devices; control mixes: jq_eval_f_g_grad_members_hvp.
 */
int jq_eval_f_g_grad_drifts_hvp(jq_handle *h, const double *pcof, int32_t ncoeff, const double *dirs, int32_t ndir, const double *drifts,
                                const double *weights, int32_t ndrift, double *out2, double *infid_grad, double *leak_grad,
                                double *hv_infid, double *hv_leak);

/*
 * jq_eval_f_g_grad_drifts_hvp over the members of jq_traceobjgrad_members / jq_eval_f_g_grad_members: member i has the drift
 * Hconsts[:, :, i] and the control mix ctrl_mix[:, :, i] -- an amplitude miscalibration or crosstalk between control lines.
 *   dirs     : [ncoeff x ndir] column-major, one direction per column
 *   Hconsts  : [Ntot x Ntot x nmember] column-major member drifts, or NULL: every member has the handle's drift
 *   ctrl_mix : [Nc x Nc x nmember] column-major real mixing matrices, or NULL: every member has the identity mix.  Operator l of member i
 *              is driven by sum_k C_i[l, k] (p_k, q_k); every control keeps its own carriers and coefficients
 *   weights  : [nmember]
 *   out2, infid_grad, leak_grad, hv_infid, hv_leak : as jq_eval_f_g_grad_hvp -- hv_infid the derivative of infid_grad, hv_leak that of
 *              leak_grad (objFuncType 1: leak_grad and hv_leak are zeros), no Tikhonov term, not symmetrised
 * Without a mix (ctrl_mix == NULL) the call IS jq_eval_f_g_grad_drifts_hvp: the same launches, the same bits.  With one, routes and
 * packing stay that call's -- a mix never changes the route, operators and structure are the handle's -- but the tangent stream of a
 * direction is no longer shared by the members: member i differentiates along sum_l (C_i d_j)_l H_l, so a member brings 1 + D streams into a
 * launch of D directions, and as many members share a launch as the stream budget (option stream_bytes) has room for at that price; the
 * others follow in further member rounds.  The traces of a member are reduced with its mix into a gradient block of its own and the
 * blocks are added in member order: one member with the identity mix gives the bits of jq_eval_f_g_grad_drifts_hvp with that member,
 * members of weight zero change no bit, and a column of zeros in every mix gives exactly zero blocks for that control.  Where that
 * call runs its members one after the other (route "sequential": a member drift outside the plan, Ntot 7 or 8, options lane=0 / quad=0,
 * more than four controls, ...) so does this one, every member with its mix.  The call never re-plans the handle and never touches its
 * drift or operator images.  jq_plan_info "member_hvp": {route: "lane" | "rowlane" | "quad" | "sequential", members_per_launch,
 * directions_per_launch, chunk_steps, rounds (direction rounds x member rounds), drifts: were member drifts given, ctrl_mix: were mixes
 * given}, present after a call; "drift_hvp", "ens_hvp", "hvp" and "member_batch" keep the values of their own calls.  jq_last_timing
 * and "last_kernels" as jq_eval_f_g_grad_hvp.  Refused with JQ_EUNSUPPORTED: what that call refuses.  JQ_EINVAL for NULL pointers (all
 * but Hconsts and ctrl_mix are required; both NULL is the plain problem: jq_eval_f_g_grad_hvp with one node), a mix entry that is not
 * finite, ndir < 1 or nmember < 1; the codes of jq_traceobjgrad for the coefficient count.  A refused call writes nothing and leaves
 * the handle as it was.  Multi-device handles run the call on their first device.  Not served: members x eps-nodes, sharding over
 * devices.
 */
int jq_eval_f_g_grad_members_hvp(jq_handle *h, const double *pcof, int32_t ncoeff, const double *dirs, int32_t ndir, const double *Hconsts,
                                 const double *ctrl_mix, const double *weights, int32_t nmember, double *out2, double *infid_grad,
                                 double *leak_grad, double *hv_infid, double *hv_leak);

/*
 * Device-side consumers of the state history, so that the [Ntot x N x (nsteps+1)] arrays (199 MB at cnot3)
 * never leave the GPU.  Replaces what the reference derives from usaver/usavei on the host:
 *   pop    : [ngroups x N x nout] (column-major) level populations  sum_{rows r in group g} |psi[r,q,k*every]|^2
 *            for the sampled steps k*every, k = 0..nout-1, nout = nsteps/every + 1.  With group_of_row == NULL
 *            (ngroups == Ntot) these are the curves of plotunitary / plotspecified (src/plotstatectrl.jl);
 *            with group_of_row[r] = third-subsystem index they are marginalize3 (src/plotstatectrl.jl:405-423).
 *            Rows with group_of_row[r] < 0 are skipped.  May be NULL (then ngroups/every/nout are ignored).
 *   maxpop : [Ntot] max over columns and ALL time steps of |psi[r,q,:]|^2 -- the forbidden-level maxima of the
 *            verbose branch (src/evalobjgrad.jl:1004-1018).  May be NULL.
 * Errors: JQ_EINVAL for NULL/size errors (nout must equal nsteps/every + 1, group indices < ngroups).
 */
int jq_state_populations(jq_handle *h, const double *pcof, int32_t ncoeff, const int32_t *group_of_row, int32_t ngroups,
                         int32_t every, int32_t nout, double *pop, double *maxpop);

/*
 * Replaces eval_f_g_grad!(pcof, params, wa, nodes, weights, compute_adjoint)
 * (src/ipopt_interface.jl:24-70): for each quadrature node ep_i the drift Hamiltonian is
 * Hconst + ep_i*diag(shift) and the four weighted sums are accumulated.  All nquad evaluations run
 * concurrently as one batch of N*nquad state columns.
 *   shift  : [Ntot] per-level factor; NULL selects the reference's 0.01*10^(j-2), j=2..Ntot (:41-44)
 *   out2   : { last_infidelity, last_leak } (:58-59)
 *   infid_grad / leak_grad : [ncoeff] weighted sums of infidelgrad / leakgrad (:48-53); leak_grad is
 *            zero-filled for objFuncType == 1.  Ignored (may be NULL) when compute_adjoint == 0.
 * Multi-GPU: a jq_create_multi handle shards the nodes over its devices and all-reduces inside this call; with one
 * process per GPU each rank passes its shard of (nodes, weights) (jq_shard_bounds) to jq_eval_f_g_grad_dev and the
 * caller sums the packed vector over the ranks with ONE all-reduce (RCCL), see juqbox.jl_amd/ipopt_interface.py.
 */
int jq_eval_f_g_grad(jq_handle *h, const double *pcof, int32_t ncoeff, const double *nodes, const double *weights,
                     int32_t nquad, const double *shift, int32_t compute_adjoint, double *out2, double *infid_grad,
                     double *leak_grad);

/*
 * npcof risk-neutral evaluations jq_eval_f_g_grad(pcofs[:, i], nodes, weights, shift, ...) of ONE problem over ONE set of nodes:
 * multi-start optimisation, batched line searches, finite-difference checks of the risk-neutral gradient, population optimisers,
 * robustness curves of several pulses.
 * pcofs: [ncoeff x npcof] column-major; out2: [2 x npcof]; infid_grad / leak_grad: [ncoeff x npcof] (NULL allowed when
 * compute_adjoint == 0); node_out: [4 x nquad x npcof] or NULL -- per vector and node the record of jq_traceobj_sweep.
 * Column i of every output equals what jq_eval_f_g_grad (node_out: jq_traceobj_sweep) returns for pcofs[:, i] under the handle's
 * current settings (sv_type, weights, solver, target, objFuncType) -- bit for bit on the same kernel variant and chunk length.
 * Grouped batches: Stormer-Verlet with the Neumann solver on the row-lane (family 3) and cooperative-quad kernels (family 8, its dense
 * policy included).  A vector's nquad * N columns are laid out as the single call lays them out and padded to a whole wave / column
 * quad (zero-weight slots / samples); the next vector starts at the next one, every workgroup reads the tile stream of its vector.  A
 * launch takes as many vectors as keep its samples inside what the family accepts for an ensemble (option pcof_batch_max: fewer),
 * larger batches run in rounds.  Everything else -- implicit midpoint, the Jacobi solver, the other kernel families, an ensemble that
 * is itself too large for families 3 / 8, cooperative quad with N not dividing 16 and not beyond it -- runs one ensemble evaluation
 * per vector inside the call.  jq_plan_info reports what the last call did ("pcof_batch": mode, vectors_per_launch, nodes_per_vector).
 * Errors: the single call's codes for the coefficient count, JQ_EINVAL for NULL required pointers, npcof < 1 or nquad < 1; a refused
 * call writes nothing.  Multi-device handles shard the VECTORS (jq_shard_bounds); the nodes of a vector stay on one device.
 */
int jq_eval_f_g_grad_batch(jq_handle *h, const double *pcofs, int32_t ncoeff, int32_t npcof, const double *nodes,
                           const double *weights, int32_t nquad, const double *shift, int32_t compute_adjoint, double *out2,
                           double *infid_grad, double *leak_grad, double *node_out);

/*
 * Ensembles over ARBITRARY drift Hamiltonians: ndrift evaluations traceobjgrad(pcof, params with Hconst = Hconsts[:, :, i], wa, false,
 * evaladjoint) of ONE control vector -- what the reference's scripts get by mutating params.Hconst in a loop (examples/Risk_Neutral/
 * run_all.jl:13-15): two uncertain transition frequencies on a tensor quadrature grid, an uncertain anharmonicity or cross-Kerr term, an
 * uncertain coupling strength (off-diagonal entries).  jq_eval_f_g_grad serves only Hconst + ep * diag(shift).
 * Hconsts: [Ntot x Ntot x ndrift] column-major, every member under the contract of jq_update_hconst's argument.  out4: [4 x ndrift],
 * totalgrad / infidelgrad / leakgrad: [ncoeff x ndrift] (laid out like jq_traceobjgrad_batch's; conventions per column exactly those of
 * jq_traceobjgrad; NULL allowed when evaladjoint == 0).
 * Column i equals what the handle returns after jq_update_hconst(h, Hconsts[:, :, i]) followed by jq_traceobjgrad(h, pcof, ...) under the
 * handle's current settings (sv_type, weights, solver, target, objFuncType) -- bit for bit on the same kernel variant and chunk length.
 * After the call the handle's own drift is what it was: a jq_traceobjgrad before the call and one after it return the same bits (the
 * re-plan below excepted).
 * Grouped ensembles: Stormer-Verlet with the Neumann solver on the row-lane (family 3) and cooperative-quad kernels (family 8, its dense
 * policy included) -- the members SHARE launches: every workgroup belongs to one member and reads the operator tile stream generated
 * from that member's drift (the time-loop kernels are those of jq_traceobjgrad_batch).  At most one member's workgroups per compute unit
 * go into a launch (option pcof_batch_max: fewer), larger ensembles run in rounds.  Everything else -- the implicit-midpoint integrator,
 * the Jacobi solver, the lane, quad-layout, slab, cooperative and run-time-size kernels, handles whose options select one of those,
 * ndrift == 1 -- makes member after member the handle's drift inside the call and runs the single evaluation: correct and bit-identical
 * to the loop a caller writes, but no faster.  jq_plan_info reports what the last call did ("drift_batch": mode, family,
 * members_per_launch, reason).
 * Planning: before anything runs every member is tested against the structure the handle was planned for.  When a member lies outside
 * it, the handle is re-planned ONCE for the union of the members' and its own nonzero pattern (as jq_update_hconst re-plans for such a
 * drift: same pointer, settings kept; slower kernels may result, never an error) and its own drift is restored; later evaluations of
 * the handle run on that more general plan until a jq_update_hconst plans back.  A member that breaks the structure of the handle's
 * embedded twin makes the handle work on without the twin, as jq_update_hconst does.
 * Errors: JQ_EINVAL for NULL required pointers and ndrift < 1, the single call's codes for the coefficient count (JQ_EINVAL / JQ_EDIM);
 * a refused call writes nothing.  Multi-device handles shard the MEMBERS (jq_shard_bounds).
 */
int jq_traceobjgrad_drifts(jq_handle *h, const double *pcof, int32_t ncoeff, const double *Hconsts, int32_t ndrift,
                           int32_t evaladjoint, double *out4, double *totalgrad, double *infidelgrad, double *leakgrad);
/*
 * The weighted sums eval_f_g_grad! forms (src/ipopt_interface.jl:48-59), over the members of a drift ensemble instead of over eps-nodes:
 * out2 = { sum_i w_i infidelity_i, sum_i w_i leak_i }, infid_grad / leak_grad: [ncoeff] the weighted sums of the members' infidelgrad /
 * leakgrad (leak_grad zero-filled for objFuncType == 1; may be NULL when compute_adjoint == 0), formed on the host in member order.
 * member_out: [4 x ndrift] or NULL -- the per-member record, bit-identical to out4 of jq_traceobjgrad_drifts.  weights: [ndrift].
 * Routing, planning, errors and multi-device behaviour: those of jq_traceobjgrad_drifts.
 */
int jq_eval_f_g_grad_drifts(jq_handle *h, const double *pcof, int32_t ncoeff, const double *Hconsts, const double *weights,
                            int32_t ndrift, int32_t compute_adjoint, double *out2, double *infid_grad, double *leak_grad,
                            double *member_out);

/*
 * Ensembles over uncertainty in the DRIVE: nmember evaluations of ONE control vector whose member i has a real Nc x Nc mixing matrix
 * C_i of the controls and, optionally, its own drift.  The controls keep their carriers and spline coefficients; what reaches operator
 * l is
 *     p~_l(t) = sum_k C_i[l, k] p_k(t),   q~_l(t) = sum_k C_i[l, k] q_k(t),
 *     H_i(t) = Hconst_i + sum_l p~_l(t) Hsym_l + i sum_l q~_l(t) Hanti_l
 * -- the plain problem whose operators are Hsym'_k = sum_l C_i[l, k] Hsym_l, Hanti'_k = sum_l C_i[l, k] Hanti_l.  A miscalibrated
 * amplitude of line k (p_k, q_k arrive scaled by 1 + delta_k) is C = diag(1 + delta); control lines that leak into each other
 * (crosstalk) are the off-diagonal entries; C = I is jq_traceobjgrad.  Uncoupled controls: the mix acts on their functions
 * ft_k(t) alike.  A complex (phase-carrying) crosstalk matrix is not served.
 * ctrl_mix: [Nc x Nc x nmember] column-major, element (l, k) of member i at l + Nc * k + Nc * Nc * i, or NULL: identity for every member.
 * Hconsts: [Ntot x Ntot x nmember] as for jq_traceobjgrad_drifts, or NULL: the handle's drift for every member.  Not both NULL.
 * Outputs: exactly those of jq_traceobjgrad_drifts, one column per member; the gradient is that with respect to the caller's
 * coefficients (the block of control k collects sum_l C_i[l, k] times what operator l contributes, with k's own carrier).
 * Zero entries of a mix are skipped, not multiplied: C = I returns the bits of the unmixed evaluation, and a zero column k of C an
 * exactly zero gradient block of control k.
 * Only two small kernels see the mix -- the one that evaluates the control functions of a chunk and the one that sums the trace records
 * the gradient is assembled from; no operator image, tile stream or time-loop kernel differs from jq_traceobjgrad_drifts'.  Routing is
 * that call's: grouped on the row-lane and cooperative-quad kernels (the members share launches, through the embedded twin as well),
 * member after member on every other route -- there with the member's mix on the single evaluation, no operator is swapped for a mix,
 * the drift (if given) as in jq_traceobjgrad_drifts.  Column i is bit-identical to the same member evaluated alone (nmember == 1) on
 * the same kernel variant and chunk length.  Hconsts != NULL: planning as in jq_traceobjgrad_drifts.  jq_plan_info: "member_batch"
 * (the fields of "drift_batch" and the booleans "drifts", "ctrl_mix"; the two drifts calls report there as well).
 * Errors: JQ_EINVAL for NULL required pointers, Hconsts and ctrl_mix both NULL, nmember < 1 and a mix entry that is not finite; the
 * single call's codes for the coefficient count; a refused call writes nothing and leaves the handle as it was.  Multi-device handles
 * shard the MEMBERS (jq_shard_bounds).  jq_traceobjgrad_drifts / jq_eval_f_g_grad_drifts are the ctrl_mix == NULL case of this call.
 */
int jq_traceobjgrad_members(jq_handle *h, const double *pcof, int32_t ncoeff, const double *Hconsts, const double *ctrl_mix,
                            int32_t nmember, int32_t evaladjoint, double *out4, double *totalgrad, double *infidelgrad,
                            double *leakgrad);
/*
 * The weighted sums of jq_eval_f_g_grad_drifts over the members of jq_traceobjgrad_members (weights: [nmember]; formed on the host in
 * member order; member_out: [4 x nmember] or NULL, bit-identical to out4 of jq_traceobjgrad_members).
 */
int jq_eval_f_g_grad_members(jq_handle *h, const double *pcof, int32_t ncoeff, const double *Hconsts, const double *ctrl_mix,
                             const double *weights, int32_t nmember, int32_t compute_adjoint, double *out2, double *infid_grad,
                             double *leak_grad, double *member_out);

/*
 * The same evaluation with the result left ON THE DEVICE for a caller that runs its own collective (one process per GPU:
 * torch.distributed / RCCL, MPI.jl): d_packed is a DEVICE pointer on the handle's GPU to 2 + 2*ncoeff doubles
 *   { sum_i w_i*infidelity_i, sum_i w_i*leak_i, infid_grad[ncoeff], leak_grad[ncoeff] }
 * -- exactly the vector that ONE all-reduce (sum) over the ranks turns into the results of eval_f_g_grad!.  The call
 * returns after the handle's stream has been synchronised.  nquad == 0 (a rank without a shard) writes zeros.
 * Single-device handles only.
 */
int jq_eval_f_g_grad_dev(jq_handle *h, const double *pcof, int32_t ncoeff, const double *nodes, const double *weights,
                         int32_t nquad, const double *shift, int32_t compute_adjoint, void *d_packed);

/*
 * Robustness sweep (ep_plot, examples/Risk_Neutral/run_all.jl:6-32): nquad independent
 * traceobjgrad evaluations with Hconst + ep_i*diag(shift), forward sweep only.
 * out: [4 x nquad] column-major = { objfv, primaryobjf, secondaryobjf, traceInfidelity } per node.
 */
int jq_traceobj_sweep(jq_handle *h, const double *pcof, int32_t ncoeff, const double *nodes, int32_t nquad,
                      const double *shift, double *out);

/* ---- controls given as samples on the time grid ----------------------------------------------*/
/*
 * Every call above takes its controls in ONE parameterisation, quadratic B-splines with carrier waves (bcarrier2, the reference's only
 * one).  The time loops know nothing of it: they read the table pq[time point][2 Nc] = (p_1, q_1, p_2, q_2, ...) and write per-step trace
 * records; two small kernels turn coefficients into the table and records into a coefficient gradient.  The calls below put the table
 * itself in the caller's hands: the objective for ANY table of control values on the 2 nsteps + 1 time points the integrator reads, and
 * its exact gradient with respect to every entry.  Any parameterisation theta -> pq (piecewise-constant pulses, DRAG or Gaussian
 * envelopes, Fourier or Slepian bases, a pulse filtered by a transfer function, the output of a neural network) is then a host-side
 * chain rule, dJ/dtheta = (d pq / d theta)' dJ/dpq.  Sweeps, plan, chunking, kernel families, control groups, two-pass gradients,
 * sv_type, full weights, the Jacobi solver, the implicit-midpoint integrator, the eps ensemble with its rounds and the embedded twin
 * are those of jq_traceobjgrad / jq_eval_f_g_grad: no time-loop kernel differs, and the plan does not depend on whether samples or
 * coefficients are given.
 *
 * The grid: nt = 2 nsteps + 1 points, J = 0 .. 2 nsteps counting half steps; jq_sample_times returns t[2 n] = the time of step n as the
 * forward sweep accumulates it (t = t + h) and t[2 n + 1] = t[2 n] + h / 2.  A Stormer-Verlet step n reads the points 2 n, 2 n + 1,
 * 2 n + 2; an implicit-midpoint step reads 2 n + 1 only, so its gradient entries at the even points are exact zeros.
 * A sample is ONE number used by the forward and by the backward sweep.  The spline calls evaluate the backward sweep at the times of
 * its own table (T - n h accumulated downwards), which differ from the forward ones in the last place: the objective of
 * jq_traceobjgrad_samples with the table of jq_control_samples is bit-identical to jq_traceobjgrad's, the gradients agree to rounding.
 *   pq : [2 Nc x nt] column-major: element (2 k, J) = p_k, (2 k + 1, J) = q_k at time point J (k = 0 .. Nc - 1)
 * jq_sample_times: JQ_EINVAL for NULL or nt != 2 nsteps + 1.
 * jq_control_samples: the handle's own spline-with-carrier controls of pcof on the grid -- the launch of the control kernel a forward
 * sweep makes, over all steps at once, so the bits are the ones an evaluation of pcof streams.  Errors: the codes of jq_traceobjgrad
 * for the coefficient count.
 * jq_traceobjgrad_samples: out4 as jq_traceobjgrad; totalgrad / infidelgrad / leakgrad: [2 Nc x nt], the layout of pq, written when
 * evaladjoint != 0 with the conventions of jq_traceobjgrad per entry (leakgrad zero-filled and infidelgrad == totalgrad for
 * objFuncType 1); may be NULL when evaladjoint == 0.  No Tikhonov term.  A point shared by two chunks of the time loop receives its two
 * halves from two launches in stream order: results are deterministic, equal across chunk lengths to rounding.
 * jq_eval_f_g_grad_samples: jq_eval_f_g_grad with the table in place of the coefficients; infid_grad / leak_grad: [2 Nc x nt].
 * jq_plan_info reports "sampled_controls": {time_points, nodes, chunk_steps} after such a call (additive key).
 * Errors: JQ_EINVAL for NULL required pointers, nt != 2 nsteps + 1, a sample that is not finite, nquad < 1.  JQ_EUNSUPPORTED for
 * uncoupled controls (their operators are driven by ft = 2 (p cos(2 pi Rfreq t) - q sin(2 pi Rfreq t)), a function of both slots: a
 * lab-frame sample interface is a later step), and whatever jq_traceobjgrad refuses for the handle's settings.  A refused call writes
 * nothing and leaves the handle as it was.  Multi-device handles run these calls on their first device.  Not served: device pointers,
 * sharding over devices (batches of tables and member ensembles: the three calls at the end of this section).
 *
 * jq_eval_f_g_grad_samples_hvp: jq_eval_f_g_grad_samples with its gradients, and Hessian-vector products in sample space -- the semantics
 * of jq_eval_f_g_grad_hvp with "coefficient" read as "sample":
 *   hv_infid[:, :, j] = d/d eps infid_grad(pq + eps dirs[:, :, j]),  hv_leak[:, :, j] = d/d eps leak_grad(pq + eps dirs[:, :, j])  at eps = 0,
 * the exact derivatives of the two gradients jq_eval_f_g_grad_samples returns, Neumann truncation included and not symmetrised
 * (objFuncType 1: hv_infid is the total gradient's derivative, hv_leak zero-filled).  A table is linear in itself, so the tangent
 * stream of a direction is the stream of its table with a zero drift: the tangent-linear time-loop kernels, the routes (lane, row-lane,
 * quad, sequential -- a table never changes the route), the budget and the rounds are those of jq_eval_f_g_grad_hvp; only the two small
 * kernels that turn tables into operator streams and trace records into gradients differ.  A single evaluation is nquad = 1 with node
 * 0 and weight 1.
 *   dirs : ndir tables, each [2 Nc x nt] column-major (the layout of pq), one after the other
 *   infid_grad / leak_grad : [2 Nc x nt];  hv_infid / hv_leak : [2 Nc x nt x ndir]
 * jq_plan_info reports "sampled_hvp": {route, directions_per_launch, chunk_steps, rounds, time_points, nodes} after such a call
 * (additive key; "ens_hvp" and "hvp" keep the values of the coefficient calls); jq_last_timing and "last_kernels" as for
 * jq_eval_f_g_grad_hvp.  Errors: JQ_EINVAL for NULL required pointers (every output is required), nt != 2 nsteps + 1, ndir < 1, nquad < 1,
 * an entry of pq or dirs that is not finite.  JQ_EUNSUPPORTED for what jq_eval_f_g_grad_hvp refuses (the implicit-midpoint integrator,
 * the Jacobi solver, full leakage weights, sv_type != 1, uncoupled controls).  A refused call writes nothing and leaves the handle as it
 * was.  Multi-device handles run the call on their first device.  Not served: products over drift or member ensembles, batches of
 * tables, device pointers, sharding over devices.
 */
int jq_sample_times(const jq_handle *h, double *t, int32_t nt);
int jq_control_samples(jq_handle *h, const double *pcof, int32_t ncoeff, double *pq);
int jq_traceobjgrad_samples(jq_handle *h, const double *pq, int32_t nt, int32_t evaladjoint, double *out4, double *totalgrad,
                            double *infidelgrad, double *leakgrad);
int jq_eval_f_g_grad_samples(jq_handle *h, const double *pq, int32_t nt, const double *nodes, const double *weights, int32_t nquad,
                             const double *shift, int32_t compute_adjoint, double *out2, double *infid_grad, double *leak_grad);
int jq_eval_f_g_grad_samples_hvp(jq_handle *h, const double *pq, int32_t nt, const double *dirs, int32_t ndir, const double *nodes,
                                 const double *weights, int32_t nquad, const double *shift, double *out2, double *infid_grad,
                                 double *leak_grad, double *hv_infid, double *hv_leak);
/*
 * Sample tables in batches and over member ensembles, in one call -- jq_traceobjgrad_batch, jq_traceobjgrad_members and
 * jq_eval_f_g_grad_members with "control vector" read as "sample table".  Where the spline calls share launches (row-lane and
 * cooperative-quad kernels, Stormer-Verlet with the Neumann solver, the column counts of jq_traceobjgrad_batch; option pcof_batch_max
 * applies, 0 forces the other route) the groups of these calls do: every workgroup reads the operator stream of its own table, or of the
 * shared table under its member's drift and mix.  On every other route the groups run one after the other inside the call (member
 * drifts become the handle's drift in turn; the handle's own is restored at the end).
 * jq_traceobjgrad_samples_batch: pqs holds ntab tables [2 Nc x nt] one after the other; column i of every output (out4: [4 x ntab], the
 * gradients: [2 Nc x nt x ntab]) is what jq_traceobjgrad_samples(pqs[i]) returns -- the record bit for bit at the same chunk length.
 * jq_traceobjgrad_samples_members: ONE table; member g has the drift Hconsts[:, :, g] (NULL: the handle's) and the real mix
 * ctrl_mix[:, :, g] (Nc x Nc column-major; NULL: identity): what reaches operator l of member g is sum_k C_g[l, k] (p_k, q_k)(t_J), as in
 * jq_traceobjgrad_members.  Member g's gradients ([2 Nc x nt x nmember]) are those with respect to the SHARED table -- its mix is folded in
 * by C_g'.  C = I writes the table's bits, a zero column k of C gives exactly zero rows 2 k, 2 k + 1 of that member's gradient.
 * jq_eval_f_g_grad_samples_members: out2 = sum_g w_g (infidelity_g, leak_g), infid_grad / leak_grad ([2 Nc x nt]) the weighted sample
 * gradients, summed ON THE DEVICE in member order from the members' finished tables (they are not fetched), so their bits do not depend
 * on how many members share a launch; member_out (may be NULL): the 4 x nmember records, as jq_eval_f_g_grad_members.
 * jq_plan_info reports "sampled_batch": {kind ("tables" | "members"), mode ("grouped" | "sequential"), why, family, per_launch, drifts,
 * mixes, time_points, chunk_steps} after such a call (additive key; "pcof_batch", "drift_batch", "member_batch" keep describing the
 * spline calls, "sampled_controls" is refreshed as by any sampled evaluation).
 * Errors: the union of the sampled calls' and the member calls' -- JQ_EINVAL for NULL required pointers, nt != 2 nsteps + 1, a sample
 * of ANY table that is not finite, ntab < 1, nmember < 1, Hconsts and ctrl_mix both NULL, a mix entry that is not finite; JQ_EUNSUPPORTED
 * for uncoupled controls.  A refused call writes nothing and leaves the handle as it was.  Member drifts are tested against the plan
 * like jq_traceobjgrad_members' (one re-plan for the union of all patterns, with that call's caveats).  Multi-device handles run these
 * calls on their first device.  Not served: Hessian-vector products over members or batches in sample space, members x eps nodes,
 * uncoupled controls, device pointers, sharding over devices.
 */
int jq_traceobjgrad_samples_batch(jq_handle *h, const double *pqs, int32_t nt, int32_t ntab, int32_t evaladjoint,
                                  double *out4, double *totalgrad, double *infidelgrad, double *leakgrad);
int jq_traceobjgrad_samples_members(jq_handle *h, const double *pq, int32_t nt, const double *Hconsts, const double *ctrl_mix,
                                    int32_t nmember, int32_t evaladjoint,
                                    double *out4, double *totalgrad, double *infidelgrad, double *leakgrad);
int jq_eval_f_g_grad_samples_members(jq_handle *h, const double *pq, int32_t nt, const double *Hconsts, const double *ctrl_mix,
                                     const double *weights, int32_t nmember, int32_t compute_adjoint,
                                     double *out2, double *infid_grad, double *leak_grad, double *member_out);

/* ---- introspection ---------------------------------------------------------------------------*/
/*
 * The plan of a handle as a JSON object (NUL-terminated, at most buflen - 1 characters; returns the length the full text needs,
 * negative JQ_E* on error): Hilbert dimension and tile rows, the structure the operators were found to have ("t4" = 4 x 4 x n
 * Kronecker structure, "od" = diagonal off-diagonal blocks, "band" / "dense"), the embedded twin if any, the control groups, the
 * integrator / solver settings and -- the part a caller sizing an ensemble needs -- the batch-size thresholds of the kernel
 * families: "families" lists, in the order run_eval tries them, {family, name, max_columns / max_slabs / max_quads} for the
 * current settings.  jq_last_timing() reports which one actually ran, and "last_kernels" which instantiation of it: null before the
 * first evaluation (and after a re-plan), then {"object", "forward_object": the kernel objects of the backward and the forward sweep
 * as csrc/Makefile names them (k_6_7, s_6_7, p_6_7, u_6_7, k_6_8, c_6_9, ...; "host": the run-time-size kernels), "slabs_per_workgroup"
 * (quad layout, else 0), "quads_per_workgroup" (split quad backward sweep: 4 / 2, else 0), "backward_workgroups" (cooperative quad: 1 /
 * 2 / 3 workgroups per column quad, else 0), and the compile-time variant as booleans "uni", "ord", "sc_forward", "sc_backward", "ride",
 * "modd", "fwd2", "wlr", "imr_two_sets"} -- recorded by the functions that pick the kernel (csrc/jq_host_select.h), for the first (larger)
 * part of a batch that was split into two launches.  The key is additive: no ABI version change.
 */
int jq_plan_info(const jq_handle *h, char *buf, int32_t buflen);

/*
 * The test behind "s_uniform" of jq_plan_info, on its own (host only; no handle, no device): 1 if the S image of every time point,
 * sum_k q_k(t) Hanti_k, repeats its first 16-row block on a 4 x 4 x n space -- every Hanti_k (Ntot x Ntot, column-major, one after the
 * other) has the same 4 x 4 diagonal blocks and the same (i, i +- 4) couplings in every 16-row block and one (i, i +- 16) coupling per
 * pair of neighbouring blocks, as Hanti_k = a_k - a_k' has -- 0 if not (or if an operator lacks the 4 x 4 x n structure), JQ_EINVAL for
 * Ntot that is not a multiple of 16 up to 128.  The three-slab quad-layout kernels then read a compact S operand (option s_compact).
 */
int jq_s_uniform(const double *Hanti_ops, int32_t Ntot, int32_t Ncoupled);

/* ---- measurement -----------------------------------------------------------------------------*/
int jq_last_timing(const jq_handle *h, jq_timing *t);
/* Library build info: "gfx950 juqbox_hip <version> src:<12 hex digits> code:<12 hex digits>" -- src: the SHA-256 prefix of the library's
 * sources (the .hip and .h files under csrc/ and include/juqbox_hip.h) AND of the flags they were built with, so measurements recorded
 * for one build (profiles/) cannot be paired with another build by accident (bench.py compares it); code: of the sources alone (the
 * shipped library and its default-register-form twin of `make check-forms-lib` agree in it). */
const char *jq_version(void);
/* JQ_ABI_VERSION of the header the library was built with */
int jq_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* JUQBOX_HIP_H */
