// jq_host_hvp.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// jq_traceobjgrad_hvp -- the derivative of the gradient (Hessian-vector products) along directions of coefficient space, on the
// tangent-linear forward sweep of jq_tl_kernels.h and the tangent of the adjoint sweep of jq_tl_adjoint_kernels.h.
//
// hv(alpha; d) = d/d eps totalgrad(alpha + eps d) at eps = 0, the exact derivative of the gradient the library returns; not symmetric
// at truncation level of the Neumann series (jq_tl_adjoint_kernels.h).
//
// Per round of `dpl` directions (jq_host_tl.h) the forward sweep of jq_traceobj_jvp (tl_forward_sweep); k_terminal_hvp then writes
// lambda(T) and its tangent, and the chunks run in reverse with streams generated with -dt and the backward schedule of the cooperative
// kernels (pack_backward_schedule): after every k_backward_tl launch the trace records go into the gradient and into hv
// (tl_reduce_chunk).  More controls than JQ_MAXNC run in control groups, the infidelity part (hv_infid) in an unforced second pass, each
// sweep from the saved terminal state.  The backward work area and state file are about twice the forward's.
// drift: the Ntot x Ntot drift Hamiltonian of the sweeps (column-major; jq_traceobjgrad_hvp: the handle's, jq_eval_f_g_grad_hvp's sequential
// route: a node's).  grad_infid (may be NULL): the gradient of the unforced pass where there is one, else the gradient.  who: the entry
// point that runs.  mix (may be NULL; jq_eval_f_g_grad_members_hvp's sequential route: a member's): the HOST Nc x Nc control mix, column-major --
// operator l is driven by sum_k C[l, k] (p_k, q_k), in the primal stream and in every direction's; k_ctrl and the reducer see it, the
// operators stay the handle's.  A control group's sweep then contributes to the coefficients of ALL controls (k_trace_reduce's q0).
// sampled (jq_eval_f_g_grad_samples_hvp's sequential route; never with a mix): pcof and the directions are sample tables [2 Nc x nt] on the
// time grid, ncoeff = 2 Nc nt, and grad, hv are with respect to the samples (TlGen::sampled); a control group adds its own columns.
static int hvp_run(jq_handle* h, const double* drift, const double* pcof, int ncoeff, const double* dirs, int ndir, double* out4, double* grad, double* hv,
                   double* hv_infid, double* grad_infid = nullptr, const char* who = "jq_traceobjgrad_hvp", const double* mix = nullptr, bool sampled = false)
{
    HIPCHK(h, hipSetDevice(h->device));
    const int NT = (h->Ntot + 15) / 16, KT = 4 * NT, Nc = h->Nc, parts = h->parts;
    const size_t stride = (size_t)NT * KT * 64;      // doubles of a dense operator image: tile (mt, kk) at (mt KT + kk) 64
    const double dt = h->T / h->nsteps;
    const int ngroups = ctrl_ngroups(Nc), ntr_max = std::min(Nc, JQ_MAXNC) * JQ_NTR;
    const bool two_pass = hv_infid && h->objFuncType != 1;
    const int nsweeps = (two_pass ? 2 : 1) * ngroups;
    const int rows = parts * JQ_HUGE_WAVES;      // trace rows of a direction
    const TlBudget b = tl_budget(h, stride, ndir, JQ_JVP_MAX_DIRS / parts, (size_t)rows * ntr_max);
    const int dpl = b.dpl, cs = b.cs, rounds = b.rounds, nvec = 1 + dpl, nblocks = dpl * parts;
    const long long sstride = (long long)JQ_TLB_STATE_ROWS(KT) * 64;

    // the trace images in control-group order (upload_operators), the weight table
    const std::vector<double> img = tl_dense_images(h, drift);
    std::vector<double> cimg((size_t)2 * Nc * stride);
    for (int g = 0; g < ngroups; ++g) {
        const int gs = ctrl_gstart(Nc, g), ng = ctrl_gstart(Nc, g + 1) - gs;
        for (int q = 0; q < ng; ++q) {
            std::copy_n(img.data() + (size_t)(1 + gs + q) * stride, stride, cimg.data() + (size_t)(2 * gs + q) * stride);
            std::copy_n(img.data() + (size_t)(1 + Nc + gs + q) * stride, stride, cimg.data() + (size_t)(2 * gs + ng + q) * stride);
        }
    }
    std::vector<double> wd((size_t)16 * NT, 0.0);
    std::copy(h->wd.begin(), h->wd.begin() + h->Ntot, wd.begin());
    DevBuf d_img, d_cimg, d_h0, d_pc, d_pq, d_stream, d_state, d_save, d_work, d_wd, d_res, d_tr, d_R, d_g, d_mix, d_raw;
    const int ntr_R = mix ? Nc * JQ_NTR : ntr_max;      // a reduced record's doubles per step
    int rc;
    if ((rc = d_img.alloc(h, who, img.size())) || (rc = d_cimg.alloc(h, who, cimg.size())) || (rc = d_h0.alloc(h, who, (size_t)nvec * stride)) ||
        (rc = d_pc.alloc(h, who, (size_t)nvec * ncoeff)) || (rc = d_pq.alloc(h, who, (size_t)nvec * (2 * cs + 1) * 2 * Nc)) ||
        (rc = d_stream.alloc(h, who, (size_t)nvec * b.gstride)) || (rc = d_state.alloc(h, who, (size_t)nblocks * sstride)) ||
        (rc = d_save.alloc(h, who, nsweeps > 1 ? (size_t)nblocks * sstride : 1)) || (rc = d_work.alloc(h, who, (size_t)nblocks * JQ_TLB_WORK_VECS * KT * 64)) ||
        (rc = d_wd.alloc(h, who, wd.size())) || (rc = d_res.alloc(h, who, (size_t)dpl * 4)) || (rc = d_tr.alloc(h, who, (size_t)2 * dpl * rows * cs * ntr_max)) ||
        (rc = d_R.alloc(h, who, (size_t)nvec * cs * ntr_R)) || (rc = d_g.alloc(h, who, (size_t)2 * nvec * ncoeff)) ||
        (mix && ((rc = d_mix.alloc(h, who, (size_t)nvec * Nc * Nc)) || (rc = d_raw.alloc(h, who, (size_t)nvec * (2 * cs + 1) * 2 * Nc)))))
        return rc;
    // d_g: [pass][primal | direction ...][ncoeff]
    hipStream_t s = h->stream;
    if ((rc = tl_upload_dense(h, img, wd, stride, nvec, d_img.p, d_h0.p, d_wd.p))) return rc;
    HIPCHK(h, hipMemcpyAsync(d_cimg.p, cimg.data(), cimg.size() * sizeof(double), hipMemcpyHostToDevice, s));
    std::vector<double> mixes;      // the member's mix once per stream [primal | direction ...]: one group, one mix
    if (mix) {
        for (int g = 0; g < nvec; ++g) mixes.insert(mixes.end(), mix, mix + (size_t)Nc * Nc);
        HIPCHK(h, hipMemcpyAsync(d_mix.p, mixes.data(), mixes.size() * sizeof(double), hipMemcpyHostToDevice, s));
    }
    const TlMix mx = {d_mix.p, d_mix.p, 1};
    const TlGen gen = {sampled ? tl_samples(h, d_pc.p, ncoeff) : tl_spline(h, d_pc.p, ncoeff, nullptr), d_img.p, d_h0.p, d_pq.p, d_stream.p, stride, b.gstride, nvec, d_mix.p, d_raw.p, sampled};
    PropArgs a = tl_prop_args(h, gen, dpl, d_state.p, sstride, d_work.p, d_wd.p);
    a.traces = d_tr.p;

    LaunchTimer tm{h};
    if ((rc = tm.start((size_t)b.nchunks * rounds * (1 + nsweeps)))) return rc;
    std::vector<double> res((size_t)dpl * 4), res0(4), blk((size_t)nvec * ncoeff), gbuf((size_t)2 * nvec * ncoeff);
    const double leak_scale = 0.5 * dt * (1.0 / h->T);
    long long mfma_bwd = 0;
    for (int r = 0; r < rounds; ++r) {
        const int j0 = r * dpl, nd = std::min(dpl, ndir - j0);
        if ((rc = tl_upload_round(h, blk, d_pc.p, pcof, dirs, j0, nd, dpl, ncoeff))) return rc;
        HIPCHK(h, hipMemsetAsync(d_g.p, 0, (size_t)2 * nvec * ncoeff * sizeof(double), s));
        if ((rc = tl_forward_sweep(h, a, gen, cs, tm))) return rc;
        hipLaunchKernelGGL(k_terminal_hvp, dim3(dpl), dim3(64), 0, s, d_state.p, sstride, h->d_vtr, h->d_vti, KT, h->N, parts, leak_scale, d_res.p);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(res.data(), d_res.p, (size_t)dpl * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
        // ---- backward sweeps: one per (control group, forcing), each from the terminal state ----
        if (nsweeps > 1) HIPCHK(h, hipMemcpyAsync(d_save.p, d_state.p, (size_t)nblocks * sstride * sizeof(double), hipMemcpyDeviceToDevice, s));
        for (int sweep = 0; sweep < nsweeps; ++sweep) {
            const int pass = sweep / ngroups, grp = sweep % ngroups;
            const int q0 = ctrl_gstart(Nc, grp), ng = ctrl_gstart(Nc, grp + 1) - q0;
            if (sweep > 0) HIPCHK(h, hipMemcpyAsync(d_state.p, d_save.p, (size_t)nblocks * sstride * sizeof(double), hipMemcpyDeviceToDevice, s));
            a.Ncoupled = ng;
            a.cimg = d_cimg.p + (size_t)2 * q0 * stride;
            a.h = -dt; a.forced = (pass == 0);
            pack_backward_schedule(a, JQ_SCHED[1], ng);
            for (int n0 = 0; n0 < h->nsteps; n0 += cs) {
                const int nc = std::min(cs, h->nsteps - n0);
                tl_generate(h, gen, n0, nc, -dt);
                a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0); a.npro = (n0 == 0) ? ng : 0;
                if ((rc = tm.begin(true))) return rc;
                hipLaunchKernelGGL(k_backward_tl<>, dim3(nblocks), dim3(64 * JQ_HUGE_WAVES), 0, s, a);
                if ((rc = tm.end())) return rc;
                tl_reduce_chunk(h, gen.sp, r == 0, d_tr.p, rows, dpl, n0, nc, q0, ng, d_R.p, d_R.p + (size_t)cs * ntr_R, d_g.p + (size_t)pass * nvec * ncoeff,
                                mix ? &mx : nullptr, sampled);
                mfma_bwd += (long long)nblocks * nc * (6 * (8 + 2 * h->m) + 8 * ng) * NT * KT;      // (two MFMAs per tile of a trace product)
                if (n0 == 0) mfma_bwd += (long long)nblocks * 2 * ng * NT * KT;
            }
        }
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(gbuf.data(), d_g.p, gbuf.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));      // (the host blocks are reused by the next round)
        if (r == 0) std::copy_n(res.begin(), 4, res0.begin());      // (the primal of the first direction's workgroups: every direction recomputes the same)
        tl_copy_out(gbuf, nvec, ncoeff, two_pass, r == 0, j0, nd, grad, grad_infid, hv, hv_infid);
    }
    if ((rc = tm.stop())) return rc;
    out_record(out4, res0.data());
    h->hvp_per_launch = dpl, h->hvp_chunk = cs, h->hvp_rounds = rounds;

    if ((rc = tm.finish("tangent-linear"))) return rc;
    h->timing.mfma_executed = tl_forward_mfma(h, rounds, nblocks) + mfma_bwd;
    h->timing.mfma_backward = mfma_bwd;
    h->timing.svts = (long long)ndir * h->N * h->nsteps;
    h->timing.kernel_family = KF_COOP;      // (as the run-time-size kernels report themselves: cooperative, NT tile rows, dense)
    h->timing.kernel_size = NT;
    h->timing.kernel_band = 15;
    return JQ_OK;
}

extern "C" int jq_traceobjgrad_hvp(jq_handle* h, const double* pcof, int32_t ncoeff, const double* dirs, int32_t ndir, double* out4, double* grad,
                                   double* hv, double* hv_infid)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_traceobjgrad_hvp", [&]() -> int {
        if (!pcof || !dirs || !out4 || !grad || !hv) return fail(h, JQ_EINVAL, "jq_traceobjgrad_hvp: NULL pointer");
        if (ndir < 1) return fail(h, JQ_EINVAL, "jq_traceobjgrad_hvp: ndir must be >= 1");
        JQ_ON_FIRST(h, jq_traceobjgrad_hvp(s0_, pcof, ncoeff, dirs, ndir, out4, grad, hv, hv_infid))
        if (int rc = tl_refuse(h, "jq_traceobjgrad_hvp", true)) return rc;
        if (int rc = check_ncoeff(h, ncoeff)) return rc;
        EvalGate gate(h);
        return hvp_run(h, h->Hconst.data(), pcof, ncoeff, dirs, ndir, out4, grad, hv, hv_infid);
    });
}
