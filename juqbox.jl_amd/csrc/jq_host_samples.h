// jq_host_samples.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// controls given as samples on the time grid -- jq_sample_times, jq_control_samples, jq_traceobjgrad_samples, jq_eval_f_g_grad_samples,
// and jq_eval_f_g_grad_samples_hvp (at the end: Hessian-vector products along direction tables, through the drivers of jq_host_ens_hvp.h).
// The time loops see the table pq[time point][2 Nc] and the trace records R only; the parameterisation lives in k_ctrl and k_gradacc.  These
// entry points put k_ctrl_samples / k_gradsamples (jq_aux_kernels.h) in their place through EvalRequest::samples: the objective of a
// caller-given table and its gradient with respect to every entry, from the sweeps, the plan and the kernels of jq_traceobjgrad.

// the grid the samples live on: t[2 n] = entry n of the forward table, t[2 n + 1] = t[2 n] + h / 2 -- the times k_ctrl evaluates (stream_time)
extern "C" int jq_sample_times(const jq_handle* hh, double* t, int32_t nt)
{
    if (!hh || !t) return JQ_EINVAL;
    const jq_handle* h = hh->subs.empty() ? hh : hh->subs[0];
    if (nt != 2 * h->nsteps + 1) return JQ_EINVAL;
    const double dt = h->T / h->nsteps;
    for (int n = 0; n <= h->nsteps; ++n) {
        t[2 * n] = h->tf[n];
        if (n < h->nsteps) t[2 * n + 1] = h->tf[n] + 0.5 * dt;
    }
    return JQ_OK;
}

// the argument rules the two evaluations share: the table has one row per time point of the grid and holds finite numbers
static int samples_args(jq_handle* h, const char* who, const double* pq, int nt)
{
    const std::string w(who);
    if (nt != 2 * h->nsteps + 1) {
        char buf[96];
        snprintf(buf, sizeof buf, ": nt = %d, the grid has 2 nsteps + 1 = %d time points", nt, 2 * h->nsteps + 1);
        return fail(h, JQ_EINVAL, (w + buf).c_str());
    }
    for (size_t e = 0; e < (size_t)2 * h->Nc * nt; ++e)
        if (!std::isfinite(pq[e])) return fail(h, JQ_EINVAL, (w + ": a sample is not finite").c_str());
    return JQ_OK;
}

// the handle's own spline-with-carrier controls on the grid: k_ctrl on the forward table, the launch of a forward chunk that covers
// every step, so the bits are the ones an evaluation of pcof streams.  The table is staged in d_grad (no evaluation is in flight).
extern "C" int jq_control_samples(jq_handle* h, const double* pcof, int32_t ncoeff, double* pq)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_control_samples", [&]() -> int {
        if (!pcof || !pq) return fail(h, JQ_EINVAL, "jq_control_samples: NULL pointer");
        JQ_ON_FIRST(h, jq_control_samples(s0_, pcof, ncoeff, pq))
        if (int rc = samples_refuse(h, "jq_control_samples")) return rc;
        if (int rc = check_ncoeff(h, ncoeff)) return rc;
        EvalGate gate(h);
        HIPCHK(h, hipSetDevice(h->device));
        const int nt = 2 * h->nsteps + 1;
        const size_t len = (size_t)nt * 2 * h->Nc;
        if (int rc = dev_grow(h, &h->d_pcof, &h->cap_pcof, (size_t)ncoeff)) return rc;
        if (int rc = dev_grow(h, &h->d_grad, &h->cap_grad, len)) return rc;
        hipStream_t s = h->stream;
        HIPCHK(h, hipMemcpyAsync(h->d_pcof, pcof, (size_t)ncoeff * sizeof(double), hipMemcpyHostToDevice, s));
        SplineArgs sp;
        sp.pcof = h->d_pcof; sp.cfreq = h->d_cfreq; sp.D1 = ncoeff / (2 * h->Nc * h->Nfreq); sp.Nfreq = h->Nfreq; sp.Ncoupled = h->Nc; sp.nCoeff = ncoeff;
        sp.dtknot = h->T / (sp.D1 - 2);
        sp.rfreq = nullptr;
        hipLaunchKernelGGL(k_ctrl, dim3((nt + 127) / 128, 1), dim3(128), 0, s, sp, h->d_tf, 0, nt, h->T / h->nsteps, h->d_grad, (const double*)nullptr, (double*)nullptr);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(pq, h->d_grad, len * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        return JQ_OK;
    });
}

extern "C" int jq_traceobjgrad_samples(jq_handle* h, const double* pq, int32_t nt, int32_t evaladjoint, double* out4, double* totalgrad,
                                       double* infidelgrad, double* leakgrad)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_traceobjgrad_samples", [&]() -> int {
        if (!pq || !out4) return fail(h, JQ_EINVAL, "jq_traceobjgrad_samples: NULL pointer");
        if (evaladjoint && (!totalgrad || !infidelgrad || !leakgrad))
            return fail(h, JQ_EINVAL, "jq_traceobjgrad_samples: gradient outputs are required when evaladjoint != 0");
        JQ_ON_FIRST(h, jq_traceobjgrad_samples(s0_, pq, nt, evaladjoint, out4, totalgrad, infidelgrad, leakgrad))
        if (int rc = samples_refuse(h, "jq_traceobjgrad_samples")) return rc;
        if (int rc = samples_args(h, "jq_traceobjgrad_samples", pq, nt)) return rc;
        EvalRequest rq;
        rq.samples = pq, rq.ncoeff = 2 * h->Nc * nt, rq.adjoint = evaladjoint != 0;
        EvalOut o;
        if (int rc = run_eval(h, rq, &o)) return rc;
        out_record(out4, o.res.data());
        if (evaladjoint) out_grads(h, rq.ncoeff, o.grad0.data(), o.grad1.data(), totalgrad, infidelgrad, leakgrad);
        return JQ_OK;
    });
}

extern "C" int jq_eval_f_g_grad_samples(jq_handle* h, const double* pq, int32_t nt, const double* nodes, const double* weights, int32_t nquad,
                                        const double* shift, int32_t compute_adjoint, double* out2, double* infid_grad, double* leak_grad)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_eval_f_g_grad_samples", [&]() -> int {
        if (!pq || !nodes || !weights || !out2) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_samples: NULL pointer");
        if (nquad < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_samples: nquad must be >= 1");
        if (compute_adjoint && (!infid_grad || !leak_grad))
            return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_samples: gradient outputs are required when compute_adjoint != 0");
        JQ_ON_FIRST(h, jq_eval_f_g_grad_samples(s0_, pq, nt, nodes, weights, nquad, shift, compute_adjoint, out2, infid_grad, leak_grad))
        if (int rc = samples_refuse(h, "jq_eval_f_g_grad_samples")) return rc;
        if (int rc = samples_args(h, "jq_eval_f_g_grad_samples", pq, nt)) return rc;
        EvalRequest rq;
        rq.samples = pq, rq.ncoeff = 2 * h->Nc * nt, rq.nsamples = nquad, rq.eps = nodes, rq.wgt = weights, rq.shift = shift, rq.adjoint = compute_adjoint != 0;
        EvalOut o;
        if (int rc = run_eval(h, rq, &o)) return rc;
        double inf = 0.0, leak = 0.0;
        for (int i = 0; i < nquad; ++i) {  // src/ipopt_interface.jl:58-59
            inf += o.res[(size_t)i * 4 + 0] * weights[i];
            leak += o.res[(size_t)i * 4 + 1] * weights[i];
        }
        out2[0] = inf;
        out2[1] = leak;
        if (compute_adjoint) out_grads(h, rq.ncoeff, o.grad0.data(), o.grad1.data(), nullptr, infid_grad, leak_grad);
        return JQ_OK;
    });
}

// jq_eval_f_g_grad_samples and the derivative of its two gradients along direction tables: jq_eval_f_g_grad_hvp (jq_host_ens_hvp.h) with
// "coefficient" read as "sample".  The tangent-linear time loops read a primal operator stream and one stream per direction and write
// trace records and their tangents; the parameterisation lives in tl_generate and tl_reduce_chunk (jq_host_tl.h), which EnsHvpArgs::sampled
// switches to k_ctrl_samples_grouped / k_gradsamples_grouped.  A table never changes the route: lane, row-lane, quad or sequential exactly
// as for coefficients, on the same propagator kernels.
extern "C" int jq_eval_f_g_grad_samples_hvp(jq_handle* h, const double* pq, int32_t nt, const double* dirs, int32_t ndir, const double* nodes,
                                            const double* weights, int32_t nquad, const double* shift, double* out2, double* infid_grad,
                                            double* leak_grad, double* hv_infid, double* hv_leak)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_eval_f_g_grad_samples_hvp", [&]() -> int {
        if (!pq || !dirs || !nodes || !weights || !out2 || !infid_grad || !leak_grad || !hv_infid || !hv_leak)
            return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_samples_hvp: NULL pointer");
        if (ndir < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_samples_hvp: ndir must be >= 1");
        if (nquad < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_samples_hvp: nquad must be >= 1");
        JQ_ON_FIRST(h, jq_eval_f_g_grad_samples_hvp(s0_, pq, nt, dirs, ndir, nodes, weights, nquad, shift, out2, infid_grad, leak_grad, hv_infid, hv_leak))
        if (int rc = tl_refuse(h, "jq_eval_f_g_grad_samples_hvp", true)) return rc;
        if (int rc = samples_refuse(h, "jq_eval_f_g_grad_samples_hvp")) return rc;
        if (int rc = samples_args(h, "jq_eval_f_g_grad_samples_hvp", pq, nt)) return rc;
        const size_t len = (size_t)2 * h->Nc * nt;
        for (size_t e = 0; e < len * (size_t)ndir; ++e)
            if (!std::isfinite(dirs[e])) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_samples_hvp: an entry of a direction table is not finite");
        EvalGate gate(h);
        EnsHvpArgs x = {"jq_eval_f_g_grad_samples_hvp", pq, dirs, nodes, weights, shift, nullptr, (int)len, ndir, nquad, out2, infid_grad, leak_grad, hv_infid, hv_leak};
        x.sampled = true;
        return ens_hvp_dispatch(h, x);
    });
}
