# hip_backend.jl -- Julia binding of libjuqbox_hip.so (C ABI: include/juqbox_hip.h), the MI355X drop-in for
# Juqbox.jl's Stormer-Verlet traceobjgrad path.
#
# Usage (inside module Juqbox, after evalobjgrad.jl / ipopt_interface.jl):  include("hip_backend.jl")
#   wa = Working_Arrays_HIP(params, nCoeff)                      # one GPU (the current HIP device)
#   wa = Working_Arrays_HIP(params, nCoeff; devices = 8)         # ONE Julia process, 8 GPUs: the risk-neutral ensemble of
#                                                                # eval_f_g_grad! is sharded over them, one RCCL all-reduce
# Everything above stays as it is: the reference dispatches traceobjgrad on the type of `wa`
# (src/evalobjgrad.jl:504 vs :1042; every caller passes `wa` untyped, src/ipopt_interface.jl:24,47,55,77,104,124,153,267),
# so setup_ipopt_problem / run_optimizer / plot_results run unchanged on top of the methods below.
#
# tests/test_julia_shim.py checks every struct layout and ccall signature of this file against include/juqbox_hip.h
# (Julia itself is not available in the build image).
using LinearAlgebra
using SparseArrays

const libjq = get(ENV, "JUQBOX_HIP_LIB", "libjuqbox_hip")      # on LD_LIBRARY_PATH, or an absolute path

struct JQCsc                              # == jq_csc: the fields of a SparseMatrixCSC{Float64,Int64}, 1-based, passed as they are
    m::Int64
    n::Int64
    colptr::Ptr{Int64}
    rowval::Ptr{Int64}
    nzval::Ptr{Float64}
end
JQCsc(A::SparseMatrixCSC{Float64,Int64}) = JQCsc(size(A, 1), size(A, 2), pointer(A.colptr), pointer(A.rowval), pointer(A.nzval))

struct JQProblem                          # == jq_problem
    Ntot::Int32
    N::Int32
    Ncoupled::Int32
    Nfreq::Int32
    nsteps::Int32
    neumann_terms::Int32
    objFuncType::Int32
    Nunc::Int32
    T::Float64
    Hconst::Ptr{Float64}
    Hsym_ops::Ptr{Float64}
    Hanti_ops::Ptr{Float64}
    Uinit::Ptr{Float64}
    Utarget_r::Ptr{Float64}
    Utarget_i::Ptr{Float64}
    wmat_real_diag::Ptr{Float64}
    Cfreq::Ptr{Float64}
    Hunc_ops::Ptr{Float64}
    Rfreq::Ptr{Float64}
    Hconst_csc::Ptr{JQCsc}                # use_sparse = true: read when the dense pointer above is NULL
    Hsym_csc::Ptr{JQCsc}
    Hanti_csc::Ptr{JQCsc}
end

struct JQTiming                           # == jq_timing
    ms_total::Float64
    ms_propagate::Float64
    ms_generate::Float64
    ms_forward::Float64
    ms_backward::Float64
    n_forward_launches::Int64
    n_backward_launches::Int64
    mfma_executed::Int64
    svts::Int64
    kernel_family::Int32
    kernel_size::Int32
    kernel_band::Int32
    kernel_variant::Int32
    mfma_backward::Int64
    ms_allreduce::Float64
    ms_shard_min::Float64
    ms_shard_max::Float64
end

# the struct layouts above are those of JQ_ABI_VERSION 6 of include/juqbox_hip.h: refuse a library built for another one
const JQ_ABI_VERSION = 6
function jq_check_abi()
    v = ccall((:jq_abi_version, libjq), Cint, ())
    v == JQ_ABI_VERSION || error("libjuqbox_hip has ABI version $v, hip_backend.jl was written for $JQ_ABI_VERSION")
    return nothing
end

abstract type AbstractWorkingArraysHIP end

# Working_Arrays_HIP: the Stormer-Verlet method of traceobjgrad (src/evalobjgrad.jl:504);
# Working_Arrays_M_HIP: the implicit-midpoint method (:1042), same handle with jq_set_integrator(2, ...)
mutable struct Working_Arrays_HIP <: AbstractWorkingArraysHIP
    handle::Ptr{Cvoid}
    gr::Vector{Float64}                   # eval_grad_f_par writes Tikhonov's gradient through wa.gr (ipopt_interface.jl:139-141)
end
mutable struct Working_Arrays_M_HIP <: AbstractWorkingArraysHIP
    handle::Ptr{Cvoid}
    gr::Vector{Float64}
end

jq_create_error() = unsafe_string(ccall((:jq_last_error, libjq), Cstring, (Ptr{Cvoid},), C_NULL))
jqcheck(wa, rc) = rc == 0 || error(unsafe_string(ccall((:jq_last_error, libjq), Cstring, (Ptr{Cvoid},), wa.handle)))

# Leakage weights.  The Stormer-Verlet path reads params.wmat_real / params.wmat_imag (src/evalobjgrad.jl:629-630): Diagonal by
# default, FULL matrices with use_custom_forbidden (:214-232) -- those go to jq_update_wmat; the diagonal alone would silently
# change the objective and the gradient.  The implicit-midpoint path reads params.wmat (:1155), a Diagonal by its field type (:90).
full_weights(params) = !(params.wmat_real isa Diagonal) || !iszero(params.wmat_imag)
function push_weights!(wa::Working_Arrays_HIP, params)
    if full_weights(params)
        params.wmat_imag isa Diagonal && !iszero(params.wmat_imag) &&
            error("hip_backend: a non-zero Diagonal wmat_imag is not a Hermitian weight (the reference ignores it in the objective, " *
                  "src/evalobjgrad.jl:2231-2233, but not in the forcing): refusing instead of evaluating something else")
        Wr = Matrix{Float64}(params.wmat_real)
        Wi = Matrix{Float64}(params.wmat_imag)
        jqcheck(wa, ccall((:jq_update_wmat, libjq), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), wa.handle, Wr, Wi))
    else
        wd = Vector{Float64}(diag(params.wmat_real))
        jqcheck(wa, ccall((:jq_update_wmat_diag, libjq), Cint, (Ptr{Cvoid}, Ptr{Float64}), wa.handle, wd))
    end
end
function push_weights!(wa::Working_Arrays_M_HIP, params)
    params.wmat isa Diagonal || error("hip_backend: the implicit-midpoint path needs Diagonal params.wmat")
    wd = Vector{Float64}(diag(params.wmat))
    jqcheck(wa, ccall((:jq_update_wmat_diag, libjq), Cint, (Ptr{Cvoid}, Ptr{Float64}), wa.handle, wd))
end

# options: "name=value,name=value" for jq_create_opts (INTEGRATION.md section 4) -- per handle, parsed once; "" = none (production)
function jq_new_handle(params, devices, options::AbstractString = "")
    jq_check_abi()
    Ntot = params.N + params.Nguard
    # use_sparse = true (src/evalobjgrad.jl:249-262): Hconst, Hsym_ops, Hanti_ops are SparseMatrixCSC{Float64,Int64}; their
    # colptr / rowval / nzval go to the library as they are (jq_csc), nothing is densified on this side
    sparse = params.Hconst isa SparseMatrixCSC{Float64,Int64} && params.Nunc == 0 &&
             all(h -> h isa SparseMatrixCSC{Float64,Int64}, params.Hsym_ops) && all(h -> h isa SparseMatrixCSC{Float64,Int64}, params.Hanti_ops)
    Hc   = sparse ? zeros(1, 1) : Matrix{Float64}(params.Hconst)                          # dense, column-major
    Hs   = (!sparse && params.Ncoupled > 0) ? reduce(hcat, [vec(Matrix{Float64}(h)) for h in params.Hsym_ops]) : zeros(1, 1)
    Ha   = (!sparse && params.Ncoupled > 0) ? reduce(hcat, [vec(Matrix{Float64}(h)) for h in params.Hanti_ops]) : zeros(1, 1)
    c0   = sparse ? [JQCsc(params.Hconst)] : JQCsc[]
    cs   = sparse ? [JQCsc(h) for h in params.Hsym_ops] : JQCsc[]
    ca   = sparse ? [JQCsc(h) for h in params.Hanti_ops] : JQCsc[]
    Hu   = params.Nunc > 0 ? reduce(hcat, [vec(Matrix{Float64}(h)) for h in params.Hunc_ops]) : zeros(1, 1)   # lab-frame evaluation
    Rf   = Vector{Float64}(params.Rfreq)
    wd   = zeros(Ntot)                                             # the weights follow the creation: push_weights!
    Cf   = Matrix{Float64}(params.Cfreq[1:params.Ncoupled+params.Nunc, :])
    Ui   = Matrix{Float64}(params.Uinit)
    h    = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Hc Hs Ha Hu Rf wd Cf Ui c0 cs ca params begin
        prob = JQProblem(Ntot, params.N, params.Ncoupled, params.Nfreq, params.nsteps,
                         params.linear_solver.max_iter, params.objFuncType, params.Nunc, params.T,
                         sparse ? Ptr{Float64}(C_NULL) : pointer(Hc), sparse ? Ptr{Float64}(C_NULL) : pointer(Hs),
                         sparse ? Ptr{Float64}(C_NULL) : pointer(Ha), pointer(Ui),
                         pointer(params.Utarget_r), pointer(params.Utarget_i), pointer(wd), pointer(Cf),
                         params.Nunc > 0 ? pointer(Hu) : Ptr{Float64}(C_NULL), params.Nunc > 0 ? pointer(Rf) : Ptr{Float64}(C_NULL),
                         sparse ? pointer(c0) : Ptr{JQCsc}(C_NULL), sparse ? pointer(cs) : Ptr{JQCsc}(C_NULL),
                         sparse ? pointer(ca) : Ptr{JQCsc}(C_NULL))
        if devices === nothing
            rc = isempty(options) ? ccall((:jq_create, libjq), Cint, (Ref{JQProblem}, Ref{Ptr{Cvoid}}), prob, h) :
                                    ccall((:jq_create_opts, libjq), Cint, (Ref{JQProblem}, Cstring, Ref{Ptr{Cvoid}}), prob, options, h)
        else
            devs = devices isa Integer ? collect(Int32, 0:devices-1) : collect(Int32, devices)
            rc = isempty(options) ? ccall((:jq_create_multi, libjq), Cint, (Ref{JQProblem}, Ptr{Int32}, Int32, Ref{Ptr{Cvoid}}),
                                          prob, devs, length(devs), h) :
                                    ccall((:jq_create_multi_opts, libjq), Cint, (Ref{JQProblem}, Ptr{Int32}, Int32, Cstring, Ref{Ptr{Cvoid}}),
                                          prob, devs, length(devs), options, h)
        end
    end
    rc == 0 || error(jq_create_error())
    return h[]
end

function Working_Arrays_HIP(params::objparams, nCoeff::Int64; devices = nothing, options::AbstractString = "")
    @assert params.linear_solver.solver_id in (NEUMANN_SOLVER, JACOBI_SOLVER)
    wa = Working_Arrays_HIP(jq_new_handle(params, devices, options), zeros(nCoeff))
    finalizer(w -> ccall((:jq_destroy, libjq), Cvoid, (Ptr{Cvoid},), w.handle), wa)
    return wa
end
function Working_Arrays_M_HIP(params::objparams, nCoeff::Int64; devices = nothing, options::AbstractString = "")
    @assert params.linear_solver.solver_id == JACOBI_SOLVER_M
    wa = Working_Arrays_M_HIP(jq_new_handle(params, devices, options), zeros(nCoeff))
    finalizer(w -> ccall((:jq_destroy, libjq), Cvoid, (Ptr{Cvoid},), w.handle), wa)
    return wa
end

num_devices(wa::AbstractWorkingArraysHIP) = ccall((:jq_num_devices, libjq), Cint, (Ptr{Cvoid},), wa.handle)
# ranks of the RCCL communicator behind a multi-device handle (ncclCommCount; 0: single device)
rccl_world_size(wa::AbstractWorkingArraysHIP) = ccall((:jq_rccl_world_size, libjq), Cint, (Ptr{Cvoid},), wa.handle)
# options of a live handle (INTEGRATION.md section 4); value = nothing: back to "not set"
function set_option!(wa::AbstractWorkingArraysHIP, name::AbstractString, value)
    v = value === nothing ? typemin(Int64) : Int64(value)      # JQ_OPTION_DEFAULT
    jqcheck(wa, ccall((:jq_set_option, libjq), Cint, (Ptr{Cvoid}, Cstring, Int64), wa.handle, name, v))
end
function get_option(wa::AbstractWorkingArraysHIP, name::AbstractString)
    v = Ref{Int64}(0)
    ccall((:jq_get_option, libjq), Cint, (Ptr{Cvoid}, Cstring, Ref{Int64}), wa.handle, name, v) == 0 || error("hip_backend: unknown option $name")
    return v[] == typemin(Int64) ? nothing : v[]
end
num_compute_units(wa::AbstractWorkingArraysHIP) = ccall((:jq_num_compute_units, libjq), Cint, (Ptr{Cvoid},), wa.handle)
function plan_info(wa::AbstractWorkingArraysHIP)      # JSON text: structure, control groups, batch-size thresholds of the kernel families, "last_kernels" (the instantiation the last evaluation ran)
    n = ccall((:jq_plan_info, libjq), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32), wa.handle, C_NULL, 0)
    n >= 0 || error("jq_plan_info failed")
    buf = Vector{UInt8}(undef, n + 1)
    ccall((:jq_plan_info, libjq), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32), wa.handle, buf, n + 1)
    return String(buf[1:n])
end
# the structure test behind "s_uniform" of plan_info (host only): do the S images of these Hanti_ops repeat their first 16-row block?
function s_uniform(Hanti_ops)
    Ntot = size(Hanti_ops[1], 1)
    Ha = reduce(hcat, [vec(Matrix{Float64}(h)) for h in Hanti_ops])
    return ccall((:jq_s_uniform, libjq), Cint, (Ptr{Float64}, Int32, Int32), Ha, Ntot, length(Hanti_ops)) == 1
end
handle_device(wa::AbstractWorkingArraysHIP) = ccall((:jq_handle_device, libjq), Cint, (Ptr{Cvoid},), wa.handle)

# What the reference's solver WOULD use.  lsolver_object's `solve` closure captures max_iter (and tol) when it is constructed
# (src/linear_solvers.jl:36-57): a script that later assigns params.linear_solver.max_iter without calling
# recreate_linear_solver_closure! (:68-78; estimate_Neumann! does call it, src/evalobjgrad.jl:2924-2925) still solves with the OLD
# values on the CPU path.  The captured variables are fields of the closure object (a Core.Box when the constructor reassigned them:
# tol *= sqrt(nrhs)); after recreate_linear_solver_closure! the closure captures the object itself (field :lsolver) and the struct's
# fields count.  Reading them here makes both back ends agree for such scripts too (round 4 read the struct's fields every call).
function solver_in_effect(ls)
    f = ls.solve
    unbox(x) = x isa Core.Box ? x.contents : x
    mi = hasfield(typeof(f), :max_iter) ? unbox(getfield(f, :max_iter)) : ls.max_iter
    tl = hasfield(typeof(f), :tol) ? unbox(getfield(f, :tol)) : ls.tol
    return Int32(mi), Float64(tl)
end

# params is mutated freely by scripts (Hconst inside eval_f_g_grad!, wmat_real, max_iter, targets): push before each call.
# Order: Diagonal weights go in BEFORE the solver / integrator and full weights AFTER it -- full weights exist with the Neumann solver
# only, so a script that switches (full weights, Neumann) <-> (Diagonal, Jacobi) in one step is valid in either direction
# (jq_update_wmat returns at once when the matrices are the ones it has: no eigen-decomposition per call).
function sync!(wa::AbstractWorkingArraysHIP, params::objparams)
    # the kernels implement the trace fidelity the constructor sets (src/evalobjgrad.jl:164); the struct is mutable
    params.pFidType == 2 || error("JQ_EUNSUPPORTED: pFidType = $(params.pFidType) -- only pFidType = 2 is implemented by the HIP backend")
    ls = params.linear_solver            # solver_id 1 = NEUMANN_SOLVER, 2 = JACOBI_SOLVER (src/linear_solvers.jl:5-8)
    max_iter, tol = solver_in_effect(ls)
    fullw = wa isa Working_Arrays_HIP && full_weights(params)
    fullw || push_weights!(wa, params)
    if wa isa Working_Arrays_M_HIP
        jqcheck(wa, ccall((:jq_set_integrator, libjq), Cint, (Ptr{Cvoid}, Int32, Int32, Float64),
                          wa.handle, 2, max_iter, tol))
    else
        jqcheck(wa, ccall((:jq_set_linear_solver, libjq), Cint, (Ptr{Cvoid}, Int32, Int32, Float64),
                          wa.handle, ls.solver_id, max_iter, tol))
    end
    fullw && push_weights!(wa, params)
    if params.Hconst isa SparseMatrixCSC{Float64,Int64}
        Hsp = params.Hconst
        GC.@preserve Hsp begin
            jqcheck(wa, ccall((:jq_update_hconst_csc, libjq), Cint, (Ptr{Cvoid}, Ref{JQCsc}), wa.handle, JQCsc(Hsp)))
        end
    else
        Hc = Matrix{Float64}(params.Hconst)
        jqcheck(wa, ccall((:jq_update_hconst, libjq), Cint, (Ptr{Cvoid}, Ptr{Float64}), wa.handle, Hc))
    end
    jqcheck(wa, ccall((:jq_update_target, libjq), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, params.Utarget_r, params.Utarget_i))
    # continuation adjoints (objparams(...; dVds), set_adjoint_Sv_type!, change_target!: src/evalobjgrad.jl:312-319, :1492-1520): dVds is
    # needed on the device only while sv_type != 1; with Working_Arrays_M_HIP a type other than 1 is refused by the library (the
    # reference's implicit-midpoint traceobjgrad never reads it)
    if params.sv_type != 1
        jqcheck(wa, ccall((:jq_update_dvds, libjq), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                          wa.handle, Matrix{Float64}(params.dVds_r), Matrix{Float64}(params.dVds_i)))
    end
    if params.sv_type != sv_type(wa)
        jqcheck(wa, ccall((:jq_set_sv_type, libjq), Cint, (Ptr{Cvoid}, Int32), wa.handle, params.sv_type))
    end
end
# the type in force on the handle (1, 2, 3 as set_adjoint_Sv_type! sets them; 4 = both terms in one backward sweep, JQ_SV_BOTH)
sv_type(wa::AbstractWorkingArraysHIP) = Int(ccall((:jq_get_sv_type, libjq), Cint, (Ptr{Cvoid},), wa.handle))

# the new method: same signature and return tuples as src/evalobjgrad.jl:504 / :1027-1036
function traceobjgrad(pcof0::Array{Float64,1}, params::objparams, wa::AbstractWorkingArraysHIP,
                      verbose::Bool = false, evaladjoint::Bool = true)
    sync!(wa, params)
    n = length(pcof0)
    out4 = zeros(4)
    if verbose && evaladjoint
        # the reference's forward-sensitivity self check (src/evalobjgrad.jl:1028) along e_kpar, from the adjoint call, the verbose call and
        # one jq_traceobj_jvp: (objfv, totalgrad, unitaryhistory, fidelity, dfdp, wr1 - im wi).  dfdp = d(objfv)/d(alpha_kpar) without a
        # Tikhonov term, as objfv is (the reference adds gr[kpar], :965, which at that point indexes the forcing work array)
        params.sv_type == 1 || throw(ArgumentError("verbose && evaladjoint needs sv_type == 1 (src/evalobjgrad.jl:770 traces against dVds otherwise)"))
        1 <= params.kpar <= n || throw(ArgumentError("params.kpar outside 1 .. length(pcof0)"))
        objfv, totalgrad = traceobjgrad(pcof0, params, wa, false, true)[1:2]
        _, hist, fidelity = traceobjgrad(pcof0, params, wa, true, false)
        d = zeros(n)
        d[params.kpar] = 1.0
        r = traceobj_jvp(pcof0, d, params, wa, true)
        return objfv, totalgrad, hist, fidelity, r.d_objfv[1], r.W[:, :, 1]
    end
    if verbose                                              # plot_results path (plot-results.jl:44): ONE forward sweep
        Ntot = params.N + params.Nguard
        ur = zeros(Ntot, params.N, params.nsteps + 1)
        ui = similar(ur)
        jqcheck(wa, ccall((:jq_traceobj_verbose, libjq), Cint,
                          (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                          wa.handle, pcof0, n, out4, ur, ui))
        return out4[1], ur + 1im * ui, 1.0 - out4[4]
    end
    tg = zeros(n); ig = zeros(n); lg = zeros(n)
    jqcheck(wa, ccall((:jq_traceobjgrad, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pcof0, n, evaladjoint ? 1 : 0, out4, tg, ig, lg))
    evaladjoint || return out4[1], out4[2], out4[3]
    return out4[1], tg, out4[2], out4[3], out4[4], ig, (params.objFuncType == 1 ? zeros(0) : lg)
end

# The tangent (Jacobian-vector product) of the discrete forward map at pcof along the columns of dirs (jq_traceobj_jvp): a tangent-linear
# Stormer-Verlet sweep, exact to rounding.  Returns (objfv, primaryobjf, secondaryobjf, d_objfv[ndir], d_primary[ndir], d_secondary[ndir],
# W[Ntot, N, ndir] complex = d(vr - i vi)(T)/d(alpha) . d, or nothing without `final`).  Stormer-Verlet with the Neumann solver and Diagonal
# weights; the library refuses the implicit-midpoint integrator, the Jacobi solver and full leakage weights.
function traceobj_jvp(pcof::Vector{Float64}, dirs::VecOrMat{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, final::Bool = true)
    ncoeff = length(pcof)
    D = dirs isa Vector ? reshape(dirs, :, 1) : Matrix{Float64}(dirs)
    size(D, 1) == ncoeff || throw(DimensionMismatch("traceobj_jvp: dirs must have length(pcof) rows"))
    nd = size(D, 2)
    nd >= 1 || throw(ArgumentError("traceobj_jvp: need at least one direction"))
    sync!(wa, params)
    Ntot = params.N + params.Nguard
    out4 = zeros(4); dout = zeros(3, nd)
    wr = zeros(Ntot, params.N, final ? nd : 0); wi = similar(wr)
    jqcheck(wa, ccall((:jq_traceobj_jvp, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pcof, ncoeff, D, nd, out4, dout, final ? pointer(wr) : C_NULL, final ? pointer(wi) : C_NULL))
    return (objfv = out4[1], primaryobjf = out4[2], secondaryobjf = out4[3], d_objfv = dout[1, :], d_primary = dout[2, :],
            d_secondary = dout[3, :], W = final ? wr + 1im * wi : nothing)
end

# The gradient at pcof and its derivative along the columns of dirs (jq_traceobjgrad_hvp; Hessian-vector products): hv[:, j] =
# d/d eps totalgrad(pcof + eps dirs[:, j]) at eps = 0, the exact derivative of the gradient the library returns -- not symmetric at truncation
# level of the Neumann series; symmetrise it or raise the order where a symmetric operator is needed.  Returns (objfv, primaryobjf,
# secondaryobjf, totalgrad[ncoeff], hv[ncoeff, ndir], hv_infid and hv_leak = hv - hv_infid for objFuncType != 1, else nothing).  No Tikhonov
# term.  Stormer-Verlet with the Neumann solver, Diagonal weights, coupled controls and sv_type 1; the library refuses everything else.
function traceobjgrad_hvp(pcof::Vector{Float64}, dirs::VecOrMat{Float64}, params::objparams, wa::AbstractWorkingArraysHIP)
    ncoeff = length(pcof)
    D = dirs isa Vector ? reshape(dirs, :, 1) : Matrix{Float64}(dirs)
    size(D, 1) == ncoeff || throw(DimensionMismatch("traceobjgrad_hvp: dirs must have length(pcof) rows"))
    nd = size(D, 2)
    nd >= 1 || throw(ArgumentError("traceobjgrad_hvp: need at least one direction"))
    sync!(wa, params)
    two = params.objFuncType != 1
    out4 = zeros(4); tg = zeros(ncoeff); hv = zeros(ncoeff, nd); hvi = zeros(ncoeff, two ? nd : 0)
    jqcheck(wa, ccall((:jq_traceobjgrad_hvp, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pcof, ncoeff, D, nd, out4, tg, hv, two ? pointer(hvi) : C_NULL))
    return (objfv = out4[1], primaryobjf = out4[2], secondaryobjf = out4[3], totalgrad = tg, hv = hv,
            hv_infid = two ? hvi : nothing, hv_leak = two ? hv - hvi : nothing)
end

# eval_f_g_grad over the quadrature nodes and the derivative of its two gradients along the columns of dirs (jq_eval_f_g_grad_hvp):
# Hessian-vector products of the risk-neutral objective, sum_i w_i d/d eps grad_i(pcof + eps dirs[:, j]).  Ntot <= 6 with at most four
# controls: tangent-linear lane kernels, every node and direction of a round in one launch per chunk; Ntot 9 .. 16 with at most four
# controls: the same on the tangent-linear row-lane kernels (four columns per wave); Ntot > 16 with the 4 x 4 x n structure (NT = 2 .. 6,
# e.g. cnot3) and at most four controls: the same on the tangent-linear quad-layout kernels (route "quad" of jq_plan_info "ens_hvp"; option
# quad=0 switches it off); else the nodes one after the other.
# Returns (infidelity, leak, infid_grad[ncoeff], leak_grad[ncoeff], hv_infid[ncoeff, ndir], hv_leak[ncoeff, ndir]); objFuncType == 1:
# infid_grad / hv_infid carry the total gradient's, leak_grad / hv_leak are zero.  No Tikhonov term.
function eval_f_g_grad_hvp(pcof::Vector{Float64}, dirs::VecOrMat{Float64}, params::objparams, wa::AbstractWorkingArraysHIP,
                           nodes::Vector{Float64} = [0.0], weights::Vector{Float64} = [1.0], shift::Union{Nothing, Vector{Float64}} = nothing)
    ncoeff = length(pcof)
    D = dirs isa Vector ? reshape(dirs, :, 1) : Matrix{Float64}(dirs)
    size(D, 1) == ncoeff || throw(DimensionMismatch("eval_f_g_grad_hvp: dirs must have length(pcof) rows"))
    nd = size(D, 2)
    nd >= 1 || throw(ArgumentError("eval_f_g_grad_hvp: need at least one direction"))
    nq = length(nodes)
    (nq >= 1 && length(weights) == nq) || throw(ArgumentError("eval_f_g_grad_hvp: nodes and weights must have the same length >= 1"))
    sync!(wa, params)
    out2 = zeros(2); ig = zeros(ncoeff); lg = zeros(ncoeff); hvi = zeros(ncoeff, nd); hvl = zeros(ncoeff, nd)
    jqcheck(wa, ccall((:jq_eval_f_g_grad_hvp, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64},
                       Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pcof, ncoeff, D, nd, nodes, weights, nq, shift === nothing ? C_NULL : pointer(shift), out2, ig, lg, hvi, hvl))
    return (infidelity = out2[1], leak = out2[2], infid_grad = ig, leak_grad = lg, hv_infid = hvi, hv_leak = hvl)
end

# eval_f_g_grad_hvp over the members of a drift ensemble instead of over eps-nodes (jq_eval_f_g_grad_drifts_hvp): the weighted sums of
# infidelity and leak, of the two gradients and of their derivatives along the columns of dirs, member i being the evaluation with
# params.Hconst = Hconsts[:, :, i].  The routes of eval_f_g_grad_hvp with a member where that call has a node -- every wave reads the
# operator stream of its own member; a member outside the structure the handle was planned for sends the members one after the other
# (jq_plan_info "drift_hvp").  The handle's drift and plan are left alone.  Returns what eval_f_g_grad_hvp returns.
function eval_f_g_grad_drifts_hvp(pcof::Vector{Float64}, dirs::VecOrMat{Float64}, params::objparams, wa::AbstractWorkingArraysHIP,
                                  Hconsts::Array{Float64, 3}, weights::Vector{Float64})
    ncoeff = length(pcof)
    D = dirs isa Vector ? reshape(dirs, :, 1) : Matrix{Float64}(dirs)
    size(D, 1) == ncoeff || throw(DimensionMismatch("eval_f_g_grad_drifts_hvp: dirs must have length(pcof) rows"))
    nd = size(D, 2)
    nd >= 1 || throw(ArgumentError("eval_f_g_grad_drifts_hvp: need at least one direction"))
    Ntot = params.N + params.Nguard
    nm = size(Hconsts, 3)
    (size(Hconsts, 1) == Ntot && size(Hconsts, 2) == Ntot && nm >= 1) || throw(DimensionMismatch("eval_f_g_grad_drifts_hvp: Hconsts must be Ntot x Ntot x ndrift, ndrift >= 1"))
    length(weights) == nm || throw(ArgumentError("eval_f_g_grad_drifts_hvp: need one weight per member drift"))
    sync!(wa, params)
    out2 = zeros(2); ig = zeros(ncoeff); lg = zeros(ncoeff); hvi = zeros(ncoeff, nd); hvl = zeros(ncoeff, nd)
    jqcheck(wa, ccall((:jq_eval_f_g_grad_drifts_hvp, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64},
                       Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pcof, ncoeff, D, nd, Hconsts, weights, nm, out2, ig, lg, hvi, hvl))
    return (infidelity = out2[1], leak = out2[2], infid_grad = ig, leak_grad = lg, hv_infid = hvi, hv_leak = hvl)
end

# eval_f_g_grad_drifts_hvp over the members of eval_f_g_grad_members! (jq_eval_f_g_grad_members_hvp): members that differ in a real
# Nc x Nc mixing matrix of the controls (ctrl_mix; operator l is driven by sum_k C[l, k] (p_k, q_k)), in their drift (Hconsts), or in both;
# `nothing` for either means the handle's drift / the identity mix, ctrl_mix === nothing is eval_f_g_grad_drifts_hvp bit for bit.  With
# mixes every wave reads the tangent stream of its own member as well (jq_plan_info "member_hvp").  The handle's drift and plan are left
# alone.  Returns what eval_f_g_grad_hvp returns.
function eval_f_g_grad_members_hvp(pcof::Vector{Float64}, dirs::VecOrMat{Float64}, params::objparams, wa::AbstractWorkingArraysHIP,
                                   Hconsts::Union{Nothing,Array{Float64,3}}, ctrl_mix::Union{Nothing,Array{Float64,3}}, weights::Vector{Float64})
    ncoeff = length(pcof)
    D = dirs isa Vector ? reshape(dirs, :, 1) : Matrix{Float64}(dirs)
    size(D, 1) == ncoeff || throw(DimensionMismatch("eval_f_g_grad_members_hvp: dirs must have length(pcof) rows"))
    nd = size(D, 2)
    nd >= 1 || throw(ArgumentError("eval_f_g_grad_members_hvp: need at least one direction"))
    Ntot = params.N + params.Nguard
    Nc = max(params.Ncoupled, params.Nunc)
    (Hconsts === nothing && ctrl_mix === nothing) && throw(ArgumentError("eval_f_g_grad_members_hvp: give Hconsts, ctrl_mix or both"))
    nm = ctrl_mix === nothing ? size(Hconsts, 3) : size(ctrl_mix, 3)
    nm >= 1 || throw(ArgumentError("eval_f_g_grad_members_hvp: need at least one member"))
    Hconsts === nothing || (size(Hconsts) == (Ntot, Ntot, nm)) || throw(DimensionMismatch("eval_f_g_grad_members_hvp: Hconsts must be Ntot x Ntot x nmember"))
    ctrl_mix === nothing || (size(ctrl_mix) == (Nc, Nc, nm)) || throw(DimensionMismatch("eval_f_g_grad_members_hvp: ctrl_mix must be Nc x Nc x nmember"))
    length(weights) == nm || throw(ArgumentError("eval_f_g_grad_members_hvp: need one weight per member"))
    sync!(wa, params)
    out2 = zeros(2); ig = zeros(ncoeff); lg = zeros(ncoeff); hvi = zeros(ncoeff, nd); hvl = zeros(ncoeff, nd)
    jqcheck(wa, ccall((:jq_eval_f_g_grad_members_hvp, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64},
                       Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pcof, ncoeff, D, nd, Hconsts === nothing ? C_NULL : pointer(Hconsts),
                      ctrl_mix === nothing ? C_NULL : pointer(ctrl_mix), weights, nm, out2, ig, lg, hvi, hvl))
    return (infidelity = out2[1], leak = out2[2], infid_grad = ig, leak_grad = lg, hv_infid = hvi, hv_leak = hvl)
end

# All unit directions through one traceobjgrad_hvp call: the ncoeff x ncoeff Jacobian of totalgrad, (J + J')/2 with symmetrize.
function hessian(pcof::Vector{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, symmetrize::Bool = false)
    J = traceobjgrad_hvp(pcof, Matrix{Float64}(LinearAlgebra.I, length(pcof), length(pcof)), params, wa).hv
    return symmetrize ? (J + J') / 2 : J
end

# ---- controls given as samples on the time grid (include/juqbox_hip.h): the objective of ANY table pq[2 Nc, nt] of control values on the
# nt = 2 nsteps + 1 time points the integrator reads, and its gradient with respect to every entry -- a parameterisation theta -> pq
# (piecewise-constant pulses, envelopes, Fourier bases, a filtered pulse) is then the chain rule (d pq / d theta)' * gradient on the host.
# Row 2k - 1 of pq is p_k, row 2k is q_k.  Coupled controls only; the library refuses uncoupled ones.
function control_sample_times(params::objparams, wa::AbstractWorkingArraysHIP)
    t = zeros(2 * params.nsteps + 1)
    rc = ccall((:jq_sample_times, libjq), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32), wa.handle, t, length(t))
    rc == 0 || error("jq_sample_times: error $rc (the handle has another number of time steps than params)")
    return t
end
# the handle's own spline-with-carrier controls of pcof on that grid, bit for bit what an evaluation of pcof streams
function control_samples(pcof::Vector{Float64}, params::objparams, wa::AbstractWorkingArraysHIP)
    sync!(wa, params)
    pq = zeros(2 * params.Ncoupled, 2 * params.nsteps + 1)
    jqcheck(wa, ccall((:jq_control_samples, libjq), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}), wa.handle, pcof, length(pcof), pq))
    return pq
end
# the return tuples of traceobjgrad (not verbose) with [2 Nc, nt] gradients
function traceobjgrad_samples(pq::Matrix{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, evaladjoint::Bool = true)
    size(pq) == (2 * params.Ncoupled, 2 * params.nsteps + 1) || throw(DimensionMismatch("traceobjgrad_samples: pq must be 2 Ncoupled x (2 nsteps + 1)"))
    sync!(wa, params)
    out4 = zeros(4)
    tg = zeros(size(pq)); ig = zeros(size(pq)); lg = zeros(size(pq))
    jqcheck(wa, ccall((:jq_traceobjgrad_samples, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pq, size(pq, 2), evaladjoint ? 1 : 0, out4, tg, ig, lg))
    evaladjoint || return out4[1], out4[2], out4[3]
    return out4[1], tg, out4[2], out4[3], out4[4], ig, (params.objFuncType == 1 ? zeros(0, 0) : lg)
end
# eval_f_g_grad over the quadrature nodes with the table in place of the coefficients: (infidelity, leak, infid_grad, leak_grad), the
# gradients [2 Nc, nt]; params.last_* are left alone
function eval_f_g_grad_samples(pq::Matrix{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, nodes::Vector{Float64} = [0.0],
                               weights::Vector{Float64} = [1.0], shift::Union{Nothing, Vector{Float64}} = nothing, compute_adjoint::Bool = true)
    size(pq) == (2 * params.Ncoupled, 2 * params.nsteps + 1) || throw(DimensionMismatch("eval_f_g_grad_samples: pq must be 2 Ncoupled x (2 nsteps + 1)"))
    nq = length(nodes)
    (nq >= 1 && length(weights) == nq) || throw(ArgumentError("eval_f_g_grad_samples: nodes and weights must have the same length >= 1"))
    sync!(wa, params)
    out2 = zeros(2); ig = zeros(size(pq)); lg = zeros(size(pq))
    jqcheck(wa, ccall((:jq_eval_f_g_grad_samples, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pq, size(pq, 2), nodes, weights, nq, shift === nothing ? C_NULL : pointer(shift), compute_adjoint ? 1 : 0, out2, ig, lg))
    return (infidelity = out2[1], leak = out2[2], infid_grad = ig, leak_grad = lg)
end
# eval_f_g_grad_samples and the derivative of its two gradients along direction tables (jq_eval_f_g_grad_samples_hvp): Hessian-vector
# products in sample space, eval_f_g_grad_hvp with "coefficient" read as "sample" -- exact derivatives of the gradients the library
# returns, truncated Neumann series included, never symmetrised.  dirs: one table like pq or [2 Nc, nt, ndir].  A table never changes the
# route (jq_plan_info "sampled_hvp").  Returns (infidelity, leak, infid_grad[2 Nc, nt], leak_grad[2 Nc, nt], hv_infid[2 Nc, nt, ndir],
# hv_leak[2 Nc, nt, ndir]); objFuncType == 1: infid_grad / hv_infid carry the total gradient's, leak_grad / hv_leak are zero.
function eval_f_g_grad_samples_hvp(pq::Matrix{Float64}, dirs::Union{Matrix{Float64}, Array{Float64, 3}}, params::objparams, wa::AbstractWorkingArraysHIP,
                                   nodes::Vector{Float64} = [0.0], weights::Vector{Float64} = [1.0], shift::Union{Nothing, Vector{Float64}} = nothing)
    size(pq) == (2 * params.Ncoupled, 2 * params.nsteps + 1) || throw(DimensionMismatch("eval_f_g_grad_samples_hvp: pq must be 2 Ncoupled x (2 nsteps + 1)"))
    D = dirs isa Matrix ? reshape(dirs, size(dirs, 1), size(dirs, 2), 1) : dirs
    nd = size(D, 3)
    (size(D, 1) == size(pq, 1) && size(D, 2) == size(pq, 2) && nd >= 1) || throw(DimensionMismatch("eval_f_g_grad_samples_hvp: dirs must be one table like pq or 2 Ncoupled x (2 nsteps + 1) x ndir, ndir >= 1"))
    nq = length(nodes)
    (nq >= 1 && length(weights) == nq) || throw(ArgumentError("eval_f_g_grad_samples_hvp: nodes and weights must have the same length >= 1"))
    sync!(wa, params)
    out2 = zeros(2); ig = zeros(size(pq)); lg = zeros(size(pq)); hvi = zeros(size(D)); hvl = zeros(size(D))
    jqcheck(wa, ccall((:jq_eval_f_g_grad_samples_hvp, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64},
                       Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pq, size(pq, 2), D, nd, nodes, weights, nq, shift === nothing ? C_NULL : pointer(shift), out2, ig, lg, hvi, hvl))
    return (infidelity = out2[1], leak = out2[2], infid_grad = ig, leak_grad = lg, hv_infid = hvi, hv_leak = hvl)
end
# Many sample tables in one call (jq_traceobjgrad_samples_batch): pqs is [2 Nc, nt, ntab]; slice i of every result is what
# traceobjgrad_samples(pqs[:, :, i]) returns.  Where the spline batch shares launches the tables do (jq_plan_info "sampled_batch").
function traceobjgrad_samples_batch(pqs::Array{Float64, 3}, params::objparams, wa::AbstractWorkingArraysHIP, evaladjoint::Bool = true)
    (size(pqs, 1) == 2 * params.Ncoupled && size(pqs, 2) == 2 * params.nsteps + 1 && size(pqs, 3) >= 1) ||
        throw(DimensionMismatch("traceobjgrad_samples_batch: pqs must be 2 Ncoupled x (2 nsteps + 1) x ntab, ntab >= 1"))
    ntab = size(pqs, 3)
    sync!(wa, params)
    out4 = zeros(4, ntab)
    tg = zeros(size(pqs)); ig = zeros(size(pqs)); lg = zeros(size(pqs))
    jqcheck(wa, ccall((:jq_traceobjgrad_samples_batch, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pqs, size(pqs, 2), ntab, evaladjoint ? 1 : 0, out4, tg, ig, lg))
    evaladjoint || return out4[1, :], out4[2, :], out4[3, :]
    return out4[1, :], tg, out4[2, :], out4[3, :], out4[4, :], ig, (params.objFuncType == 1 ? zeros(0, 0, 0) : lg)
end
# the shapes of a member ensemble over ONE sample table: (nmember); `nothing` for Hconsts / ctrl_mix means the handle's drift / the identity
function samples_members_count(who::String, pq::Matrix{Float64}, params::objparams, Hconsts, ctrl_mix)
    size(pq) == (2 * params.Ncoupled, 2 * params.nsteps + 1) || throw(DimensionMismatch("$who: pq must be 2 Ncoupled x (2 nsteps + 1)"))
    (Hconsts === nothing && ctrl_mix === nothing) && throw(ArgumentError("$who: give Hconsts, ctrl_mix or both"))
    Ntot = params.N + params.Nguard
    nm = ctrl_mix === nothing ? size(Hconsts, 3) : size(ctrl_mix, 3)
    nm >= 1 || throw(ArgumentError("$who: need at least one member"))
    Hconsts === nothing || (size(Hconsts) == (Ntot, Ntot, nm)) || throw(DimensionMismatch("$who: Hconsts must be Ntot x Ntot x nmember"))
    ctrl_mix === nothing || (size(ctrl_mix) == (params.Ncoupled, params.Ncoupled, nm)) || throw(DimensionMismatch("$who: ctrl_mix must be Nc x Nc x nmember"))
    return nm
end
# ONE sample table under nmember members (jq_traceobjgrad_samples_members): member i has the drift Hconsts[:, :, i] and the real control
# mix ctrl_mix[:, :, i] (operator l is driven by sum_k C[l, k] (p_k, q_k)); its gradients [2 Nc, nt, i] are those with respect to the
# shared table.  The handle's drift and plan are left alone.
function traceobjgrad_samples_members(pq::Matrix{Float64}, params::objparams, wa::AbstractWorkingArraysHIP,
                                      Hconsts::Union{Nothing,Array{Float64,3}}, ctrl_mix::Union{Nothing,Array{Float64,3}}, evaladjoint::Bool = true)
    nm = samples_members_count("traceobjgrad_samples_members", pq, params, Hconsts, ctrl_mix)
    sync!(wa, params)
    out4 = zeros(4, nm)
    tg = zeros(size(pq)..., nm); ig = zeros(size(pq)..., nm); lg = zeros(size(pq)..., nm)
    jqcheck(wa, ccall((:jq_traceobjgrad_samples_members, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pq, size(pq, 2), Hconsts === nothing ? C_NULL : pointer(Hconsts), ctrl_mix === nothing ? C_NULL : pointer(ctrl_mix),
                      nm, evaladjoint ? 1 : 0, out4, tg, ig, lg))
    evaladjoint || return out4[1, :], out4[2, :], out4[3, :]
    return out4[1, :], tg, out4[2, :], out4[3, :], out4[4, :], ig, (params.objFuncType == 1 ? zeros(0, 0, 0) : lg)
end
# the weighted ensemble of those members (jq_eval_f_g_grad_samples_members): sum_i w_i (infidelity_i, leak_i) and the two weighted sample
# gradients [2 Nc, nt], summed on the device; members: the 4 x nmember records
function eval_f_g_grad_samples_members(pq::Matrix{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, weights::Vector{Float64},
                                       Hconsts::Union{Nothing,Array{Float64,3}}, ctrl_mix::Union{Nothing,Array{Float64,3}}, compute_adjoint::Bool = true)
    nm = samples_members_count("eval_f_g_grad_samples_members", pq, params, Hconsts, ctrl_mix)
    length(weights) == nm || throw(ArgumentError("eval_f_g_grad_samples_members: need one weight per member"))
    sync!(wa, params)
    out2 = zeros(2); ig = zeros(size(pq)); lg = zeros(size(pq)); rec = zeros(4, nm)
    jqcheck(wa, ccall((:jq_eval_f_g_grad_samples_members, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pq, size(pq, 2), Hconsts === nothing ? C_NULL : pointer(Hconsts), ctrl_mix === nothing ? C_NULL : pointer(ctrl_mix),
                      weights, nm, compute_adjoint ? 1 : 0, out2, ig, lg, rec))
    return (infidelity = out2[1], leak = out2[2], infid_grad = ig, leak_grad = lg, members = rec)
end

# Many control vectors of ONE problem in one call (jq_traceobjgrad_batch): column i of every result is what
# traceobjgrad(pcofs[:, i], params, wa, false, evaladjoint) returns.  On the latency kernels (row-lane, cooperative quad; Stormer-Verlet)
# the vectors share launches, elsewhere they run one after the other inside the call.
# evaladjoint: (objfv[n], totalgrad[ncoeff, n], primaryobjf[n], secondaryobjf[n], traceInfidelity[n], infidelgrad[ncoeff, n],
#               leakgrad[ncoeff, n] -- 0 x n for objFuncType == 1); else (objfv[n], primaryobjf[n], secondaryobjf[n])
function traceobjgrad_batch(pcofs::Matrix{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, evaladjoint::Bool = true)
    ncoeff, n = size(pcofs)
    n >= 1 || throw(ArgumentError("traceobjgrad_batch: need at least one control vector"))
    sync!(wa, params)
    out4 = zeros(4, n)
    tg = zeros(ncoeff, evaladjoint ? n : 0); ig = similar(tg); lg = similar(tg)
    jqcheck(wa, ccall((:jq_traceobjgrad_batch, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pcofs, ncoeff, n, evaladjoint ? 1 : 0, out4,
                      evaladjoint ? pointer(tg) : C_NULL, evaladjoint ? pointer(ig) : C_NULL, evaladjoint ? pointer(lg) : C_NULL))
    evaladjoint || return out4[1, :], out4[2, :], out4[3, :]
    return out4[1, :], tg, out4[2, :], out4[3, :], out4[4, :], ig, (params.objFuncType == 1 ? zeros(0, n) : lg)
end

# the state history alone (usaver, usavei of src/evalobjgrad.jl:677-680, :748-752)
function state_history(pcof::Vector{Float64}, params::objparams, wa::AbstractWorkingArraysHIP)
    sync!(wa, params)
    Ntot = params.N + params.Nguard
    ur = zeros(Ntot, params.N, params.nsteps + 1)
    ui = similar(ur)
    jqcheck(wa, ccall((:jq_state_history, libjq), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pcof, length(pcof), ur, ui))
    return ur, ui
end

# Replaces the serial loop of eval_f_g_grad! (src/ipopt_interface.jl:24-70): all quadrature nodes run concurrently on the
# GPU(s); with a multi-device handle they are sharded over the GPUs and summed with one RCCL all-reduce inside the call.
# shift = nothing: the reference's perturbation Hconst[j,j] += 0.01*ep*10^(j-2) (:41-44).
function eval_f_g_grad!(pcof::Vector{Float64}, params::objparams, wa::AbstractWorkingArraysHIP,
                        nodes::AbstractArray = [0.0], weights::AbstractArray = [1.0], compute_adjoint::Bool = true;
                        shift = nothing)
    sync!(wa, params)
    n = length(pcof)
    out2 = zeros(2); ig = zeros(n); lg = zeros(n)
    nd = collect(Float64, nodes); wt = collect(Float64, weights)
    sh = shift === nothing ? C_NULL : pointer(shift)
    GC.@preserve shift begin
        jqcheck(wa, ccall((:jq_eval_f_g_grad, libjq), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            wa.handle, pcof, n, nd, wt, length(nd), sh, compute_adjoint ? 1 : 0, out2, ig, lg))
    end
    params.last_pcof .= pcof                                   # :23-27, :48-59, :67-68
    params.last_infidelity, params.last_leak = out2
    params.last_infidelity_grad .= compute_adjoint ? ig : 0.0
    length(params.last_leak_grad) > 0 && (params.last_leak_grad .= compute_adjoint ? lg : 0.0)
    params.lastTraceInfidelity = params.last_infidelity
    params.lastLeakIntegral = params.last_leak
end

# eval_f_g_grad! for many control vectors over ONE set of nodes in one call (jq_eval_f_g_grad_batch): column i of every result is what
# eval_f_g_grad!(pcofs[:, i], ...) leaves in params.last_* -- which this method does not touch (they memoise one vector).  On the
# latency kernels (row-lane, cooperative quad; Stormer-Verlet) launches hold G vectors x nquad nodes, elsewhere one ensemble per vector.
# Returns (infidelity[n], leak[n], infid_grad[ncoeff, n], leak_grad[ncoeff, n] -- 0 x n for objFuncType == 1) and with per_node = true
# also the 4 x nquad x n array of traceobj_sweep records.
function eval_f_g_grad_batch(pcofs::Matrix{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, nodes::AbstractArray,
                             weights::AbstractArray, compute_adjoint::Bool = true; shift = nothing, per_node::Bool = false)
    ncoeff, n = size(pcofs)
    n >= 1 || throw(ArgumentError("eval_f_g_grad_batch: need at least one control vector"))
    nd = collect(Float64, nodes); wt = collect(Float64, weights)
    (length(nd) == length(wt) && length(nd) >= 1) || throw(ArgumentError("eval_f_g_grad_batch: nodes and weights must have the same length >= 1"))
    sync!(wa, params)
    out2 = zeros(2, n)
    ig = zeros(ncoeff, compute_adjoint ? n : 0); lg = similar(ig)
    node_out = zeros(4, length(nd), per_node ? n : 0)
    sh = shift === nothing ? C_NULL : pointer(shift)
    GC.@preserve shift begin
        jqcheck(wa, ccall((:jq_eval_f_g_grad_batch, libjq), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            wa.handle, pcofs, ncoeff, n, nd, wt, length(nd), sh, compute_adjoint ? 1 : 0, out2,
            compute_adjoint ? pointer(ig) : C_NULL, compute_adjoint ? pointer(lg) : C_NULL, per_node ? pointer(node_out) : C_NULL))
    end
    compute_adjoint || (ig = zeros(ncoeff, n); lg = zeros(ncoeff, n))
    res = (out2[1, :], out2[2, :], ig, (params.objFuncType == 1 ? zeros(0, n) : lg))
    return per_node ? (res..., node_out) : res
end

# ONE control vector over an ensemble of arbitrary drift Hamiltonians in one call (jq_traceobjgrad_drifts): column i of every result is
# what traceobjgrad(pcof, params, wa, false, evaladjoint) returns with params.Hconst = Hconsts[:, :, i] -- the loop of
# examples/Risk_Neutral/run_all.jl:13-15.  On the latency kernels (row-lane, cooperative quad; Stormer-Verlet, Neumann) the members share
# launches, elsewhere the handle's drift is swapped per member inside the call; params.Hconst and the handle's drift stay what they were.
# Returns what traceobjgrad_batch returns, one column per member.
function traceobjgrad_drifts(pcof::Vector{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, Hconsts::Array{Float64,3},
                             evaladjoint::Bool = true)
    Ntot = params.N + params.Nguard
    n = size(Hconsts, 3)
    n >= 1 || throw(ArgumentError("traceobjgrad_drifts: need at least one member drift"))
    (size(Hconsts, 1) == Ntot && size(Hconsts, 2) == Ntot) || throw(ArgumentError("traceobjgrad_drifts: members must be Ntot x Ntot"))
    sync!(wa, params)
    ncoeff = length(pcof)
    out4 = zeros(4, n)
    tg = zeros(ncoeff, evaladjoint ? n : 0); ig = similar(tg); lg = similar(tg)
    jqcheck(wa, ccall((:jq_traceobjgrad_drifts, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pcof, ncoeff, Hconsts, n, evaladjoint ? 1 : 0, out4,
                      evaladjoint ? pointer(tg) : C_NULL, evaladjoint ? pointer(ig) : C_NULL, evaladjoint ? pointer(lg) : C_NULL))
    evaladjoint || return out4[1, :], out4[2, :], out4[3, :]
    return out4[1, :], tg, out4[2, :], out4[3, :], out4[4, :], ig, (params.objFuncType == 1 ? zeros(0, n) : lg)
end

# eval_f_g_grad! over the members of a drift ensemble instead of over eps-nodes (jq_eval_f_g_grad_drifts): the weighted sums land in
# params.last_* exactly as eval_f_g_grad! leaves them; per_member = true also returns the 4 x ndrift array of the members' records.
function eval_f_g_grad_drifts!(pcof::Vector{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, Hconsts::Array{Float64,3},
                               weights::AbstractArray, compute_adjoint::Bool = true; per_member::Bool = false)
    Ntot = params.N + params.Nguard
    nm = size(Hconsts, 3)
    wt = collect(Float64, weights)
    nm >= 1 || throw(ArgumentError("eval_f_g_grad_drifts!: need at least one member drift"))
    (size(Hconsts, 1) == Ntot && size(Hconsts, 2) == Ntot) || throw(ArgumentError("eval_f_g_grad_drifts!: members must be Ntot x Ntot"))
    length(wt) == nm || throw(ArgumentError("eval_f_g_grad_drifts!: need one weight per member drift"))
    sync!(wa, params)
    n = length(pcof)
    out2 = zeros(2); ig = zeros(n); lg = zeros(n)
    member_out = zeros(4, per_member ? nm : 0)
    jqcheck(wa, ccall((:jq_eval_f_g_grad_drifts, libjq), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        wa.handle, pcof, n, Hconsts, wt, nm, compute_adjoint ? 1 : 0, out2, ig, lg, per_member ? pointer(member_out) : C_NULL))
    params.last_pcof .= pcof
    params.last_infidelity, params.last_leak = out2
    params.last_infidelity_grad .= compute_adjoint ? ig : 0.0
    length(params.last_leak_grad) > 0 && (params.last_leak_grad .= compute_adjoint ? lg : 0.0)
    params.lastTraceInfidelity = params.last_infidelity
    params.lastLeakIntegral = params.last_leak
    return per_member ? member_out : nothing
end

# ONE control vector over members that differ in a real Nc x Nc mixing matrix of the controls -- operator l is driven by
# sum_k ctrl_mix[l, k, i] (p_k, q_k): diag(1 + delta) is a miscalibrated amplitude, off-diagonal entries are crosstalk -- and, optionally,
# in their drift (jq_traceobjgrad_members).  Hconsts / ctrl_mix: `nothing` stands for the drift of params / the identity; not both.
# Returns what traceobjgrad_drifts returns, one column per member.
function traceobjgrad_members(pcof::Vector{Float64}, params::objparams, wa::AbstractWorkingArraysHIP,
                              Hconsts::Union{Nothing,Array{Float64,3}}, ctrl_mix::Union{Nothing,Array{Float64,3}}, evaladjoint::Bool = true)
    Ntot = params.N + params.Nguard
    Nc = max(params.Ncoupled, params.Nunc)
    (Hconsts === nothing && ctrl_mix === nothing) && throw(ArgumentError("traceobjgrad_members: give Hconsts, ctrl_mix or both"))
    n = ctrl_mix === nothing ? size(Hconsts, 3) : size(ctrl_mix, 3)
    n >= 1 || throw(ArgumentError("traceobjgrad_members: need at least one member"))
    Hconsts === nothing || (size(Hconsts) == (Ntot, Ntot, n)) || throw(ArgumentError("traceobjgrad_members: Hconsts must be Ntot x Ntot x nmember"))
    ctrl_mix === nothing || (size(ctrl_mix) == (Nc, Nc, n)) || throw(ArgumentError("traceobjgrad_members: ctrl_mix must be Nc x Nc x nmember"))
    sync!(wa, params)
    ncoeff = length(pcof)
    out4 = zeros(4, n)
    tg = zeros(ncoeff, evaladjoint ? n : 0); ig = similar(tg); lg = similar(tg)
    jqcheck(wa, ccall((:jq_traceobjgrad_members, libjq), Cint,
                      (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                      wa.handle, pcof, ncoeff, Hconsts === nothing ? C_NULL : pointer(Hconsts), ctrl_mix === nothing ? C_NULL : pointer(ctrl_mix),
                      n, evaladjoint ? 1 : 0, out4,
                      evaladjoint ? pointer(tg) : C_NULL, evaladjoint ? pointer(ig) : C_NULL, evaladjoint ? pointer(lg) : C_NULL))
    evaladjoint || return out4[1, :], out4[2, :], out4[3, :]
    return out4[1, :], tg, out4[2, :], out4[3, :], out4[4, :], ig, (params.objFuncType == 1 ? zeros(0, n) : lg)
end

# eval_f_g_grad_drifts! over the members of traceobjgrad_members (jq_eval_f_g_grad_members): the weighted sums land in params.last_*
# exactly as eval_f_g_grad! leaves them; per_member = true also returns the 4 x nmember array of the members' records.
function eval_f_g_grad_members!(pcof::Vector{Float64}, params::objparams, wa::AbstractWorkingArraysHIP,
                                Hconsts::Union{Nothing,Array{Float64,3}}, ctrl_mix::Union{Nothing,Array{Float64,3}},
                                weights::AbstractArray, compute_adjoint::Bool = true; per_member::Bool = false)
    Ntot = params.N + params.Nguard
    Nc = max(params.Ncoupled, params.Nunc)
    (Hconsts === nothing && ctrl_mix === nothing) && throw(ArgumentError("eval_f_g_grad_members!: give Hconsts, ctrl_mix or both"))
    nm = ctrl_mix === nothing ? size(Hconsts, 3) : size(ctrl_mix, 3)
    wt = collect(Float64, weights)
    nm >= 1 || throw(ArgumentError("eval_f_g_grad_members!: need at least one member"))
    Hconsts === nothing || (size(Hconsts) == (Ntot, Ntot, nm)) || throw(ArgumentError("eval_f_g_grad_members!: Hconsts must be Ntot x Ntot x nmember"))
    ctrl_mix === nothing || (size(ctrl_mix) == (Nc, Nc, nm)) || throw(ArgumentError("eval_f_g_grad_members!: ctrl_mix must be Nc x Nc x nmember"))
    length(wt) == nm || throw(ArgumentError("eval_f_g_grad_members!: need one weight per member"))
    sync!(wa, params)
    n = length(pcof)
    out2 = zeros(2); ig = zeros(n); lg = zeros(n)
    member_out = zeros(4, per_member ? nm : 0)
    jqcheck(wa, ccall((:jq_eval_f_g_grad_members, libjq), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        wa.handle, pcof, n, Hconsts === nothing ? C_NULL : pointer(Hconsts), ctrl_mix === nothing ? C_NULL : pointer(ctrl_mix), wt, nm,
        compute_adjoint ? 1 : 0, out2, ig, lg, per_member ? pointer(member_out) : C_NULL))
    params.last_pcof .= pcof
    params.last_infidelity, params.last_leak = out2
    params.last_infidelity_grad .= compute_adjoint ? ig : 0.0
    length(params.last_leak_grad) > 0 && (params.last_leak_grad .= compute_adjoint ? lg : 0.0)
    params.lastTraceInfidelity = params.last_infidelity
    params.lastLeakIntegral = params.last_leak
    return per_member ? member_out : nothing
end

# One process per GPU (MPI.jl): each rank evaluates its shard and leaves the packed sums on its device; the caller
# all-reduces `d_packed` (2 + 2 nCoeff doubles on the GPU, e.g. a ROCArray) over the ranks.
function shard_bounds(nquad::Integer, rank::Integer, world::Integer)
    lo = Ref{Int32}(0); hi = Ref{Int32}(0)
    rc = ccall((:jq_shard_bounds, libjq), Cint, (Int32, Int32, Int32, Ref{Int32}, Ref{Int32}), nquad, rank, world, lo, hi)
    rc == 0 || error("jq_shard_bounds: invalid arguments")
    return Int(lo[]) + 1, Int(hi[])                             # 1-based inclusive range lo:hi
end
function eval_f_g_grad_dev!(pcof::Vector{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, nodes::Vector{Float64},
                            weights::Vector{Float64}, compute_adjoint::Bool, d_packed::Ptr{Cvoid}; shift = nothing)
    sync!(wa, params)
    sh = shift === nothing ? C_NULL : pointer(shift)
    GC.@preserve shift begin
        jqcheck(wa, ccall((:jq_eval_f_g_grad_dev, libjq), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Cvoid}),
            wa.handle, pcof, length(pcof), nodes, weights, length(nodes), sh, compute_adjoint ? 1 : 0, d_packed))
    end
end

# ep_plot's serial robustness sweep (examples/Risk_Neutral/run_all.jl:6-32) as one call: 4 x nquad matrix
# (objfv, primaryobjf, secondaryobjf, traceInfidelity) per perturbation
function traceobj_sweep(pcof::Vector{Float64}, params::objparams, wa::AbstractWorkingArraysHIP, ep_vals::AbstractArray;
                        shift = nothing)
    sync!(wa, params)
    ep = collect(Float64, ep_vals)
    out = zeros(4, length(ep))
    sh = shift === nothing ? C_NULL : pointer(shift)
    GC.@preserve shift begin
        jqcheck(wa, ccall((:jq_traceobj_sweep, libjq), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
            wa.handle, pcof, length(pcof), ep, length(ep), sh, out))
    end
    return out
end

# plot_results / the verbose report need the history only through reductions: they stay on the device
# (199 MB at cnot3 never cross PCIe).  marginalize3: src/plotstatectrl.jl:405-423
function marginalize3(params::objparams, pcof::Vector{Float64}, wa::AbstractWorkingArraysHIP; every::Int = 1)
    Ntot = params.N + params.Nguard
    nout = div(params.nsteps, every) + 1
    grp  = Int32[div(k - 1, params.Nt[1] * params.Nt[2]) for k in 1:Ntot]
    pop  = zeros(params.Nt[3], params.N, nout)
    sync!(wa, params)
    jqcheck(wa, ccall((:jq_state_populations, libjq), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Int32}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
        wa.handle, pcof, length(pcof), grp, params.Nt[3], every, nout, pop, C_NULL))
    return pop
end

# estimate_Neumann! (src/evalobjgrad.jl:2922-2925) mutates params.linear_solver.max_iter; sync! picks it up.  The direct
# setter, for callers that bypass params:
set_neumann_terms!(wa::AbstractWorkingArraysHIP, m::Integer) =
    jqcheck(wa, ccall((:jq_set_neumann_terms, libjq), Cint, (Ptr{Cvoid}, Int32), wa.handle, m))

function last_timing(wa::AbstractWorkingArraysHIP)
    t = Ref{JQTiming}()
    jqcheck(wa, ccall((:jq_last_timing, libjq), Cint, (Ptr{Cvoid}, Ref{JQTiming}), wa.handle, t))
    return t[]
end

device_count() = ccall((:jq_device_count, libjq), Cint, ())
set_device(d::Integer) = ccall((:jq_set_device, libjq), Cint, (Cint,), d)
version() = unsafe_string(ccall((:jq_version, libjq), Cstring, ()))
