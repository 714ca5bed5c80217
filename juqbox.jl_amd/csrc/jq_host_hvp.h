// jq_host_hvp.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// jq_traceobjgrad_hvp -- the derivative of the gradient (Hessian-vector products) along directions of coefficient space, on the
// tangent-linear forward sweep of jq_tl_kernels.h and the tangent of the adjoint sweep of jq_tl_adjoint_kernels.h.
//
// hv(alpha; d) = d/d eps totalgrad(alpha + eps d) at eps = 0, the exact derivative of the gradient the library returns; not symmetric
// at truncation level of the Neumann series (jq_tl_adjoint_kernels.h).
//
// The forward half is jvp_run's (jq_host_jvp.h): per round of `dpl` directions a grouped chunk of 1 + dpl tile streams, k_forward_tl
// chunk by chunk.  k_terminal_hvp then writes lambda(T) and its tangent, and the chunks run in reverse with streams generated with -dt
// and the backward schedule of run_eval (jq_host_eval.h): after every k_backward_tl launch k_trace_reduce / k_gradacc run twice, on the
// primal record of the round's first direction into the gradient (first round only: every direction recomputes the same primal) and on
// the tangent records into hv.  More controls than JQ_MAXNC run in control groups, the infidelity part (hv_infid) in an unforced second
// pass, each sweep from the saved terminal state.  A direction's arithmetic does not depend on the launch it rides in.  Like the JVP
// the call plans nothing and frees what it allocates; the backward work area and state file are about twice the forward's.
// drift: the Ntot x Ntot drift Hamiltonian of the sweeps (column-major; jq_traceobjgrad_hvp: the handle's, jq_eval_f_g_grad_hvp's sequential
// route: a node's).  grad_infid (may be NULL): the gradient of the unforced pass where there is one, else the gradient.
static int hvp_run(jq_handle* h, const double* drift, const double* pcof, int ncoeff, const double* dirs, int ndir, double* out4, double* grad, double* hv,
                   double* hv_infid, double* grad_infid = nullptr)
{
    HIPCHK(h, hipSetDevice(h->device));
    const int NT = (h->Ntot + 15) / 16, KT = 4 * NT, Nc = h->Nc, parts = h->parts;
    const size_t stride = (size_t)NT * KT * 64;      // doubles of a dense operator image: tile (mt, kk) at (mt KT + kk) 64
    const size_t nn = (size_t)h->Ntot * h->Ntot;
    const int D1 = ncoeff / (2 * Nc * h->Nfreq);
    const double dt = h->T / h->nsteps;
    const int ngroups = ctrl_ngroups(Nc), ntr_max = std::min(Nc, JQ_MAXNC) * JQ_NTR;
    const bool two_pass = hv_infid && h->objFuncType != 1;
    const int nsweeps = (two_pass ? 2 : 1) * ngroups;

    // directions per launch, chunk length, rounds: jvp_run's budgeting; the two trace records of a chunk stay within the same budget
    size_t budget = ((size_t)1 << 30) / sizeof(double);
    if (h->opt.has(O_STREAM_BYTES) && h->opt.get(O_STREAM_BYTES) > 0) budget = (size_t)h->opt.get(O_STREAM_BYTES) / sizeof(double);
    const long long want = 2LL * std::min(JQ_JVP_MIN_CHUNK, h->nsteps) + 1;
    const long long fit = (long long)(budget / (2 * stride * (size_t)want)) - 1;
    const int dpl = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(ndir, JQ_JVP_MAX_DIRS / parts), fit));
    const int nvec = 1 + dpl, nblocks = dpl * parts;
    const long long tps = (long long)(budget / ((size_t)(1 + dpl) * 2 * stride));
    const long long trc = (long long)(budget / ((size_t)2 * nblocks * JQ_HUGE_WAVES * ntr_max));
    const int cs = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(std::min(h->chunk_steps, h->nsteps), (tps - 1) / 2), trc));
    const int rounds = (ndir + dpl - 1) / dpl;
    const size_t gstride = (size_t)(2 * cs + 1) * 2 * stride;
    const long long sstride = (long long)JQ_TLB_STATE_ROWS(KT) * 64;
    const size_t trows = (size_t)nblocks * JQ_HUGE_WAVES;      // rows of one trace record

    // operator images [H0 | Hsym_q | Hanti_q], the trace images in control-group order (upload_operators), the drift images of the
    // groups [H0 | 0 ...], tables
    std::vector<double> img((size_t)(1 + 2 * Nc) * stride, 0.0), cimg((size_t)2 * Nc * stride);
    tile_image_coop(drift, h->Ntot, NT, 15, img.data());
    for (int q = 0; q < Nc; ++q) {
        tile_image_coop(h->Hsym.data() + q * nn, h->Ntot, NT, 15, img.data() + (size_t)(1 + q) * stride);
        tile_image_coop(h->Hanti.data() + q * nn, h->Ntot, NT, 15, img.data() + (size_t)(1 + Nc + q) * stride);
    }
    for (int g = 0; g < ngroups; ++g) {
        const int gs = ctrl_gstart(Nc, g), ng = ctrl_gstart(Nc, g + 1) - gs;
        for (int q = 0; q < ng; ++q) {
            std::copy_n(img.data() + (size_t)(1 + gs + q) * stride, stride, cimg.data() + (size_t)(2 * gs + q) * stride);
            std::copy_n(img.data() + (size_t)(1 + Nc + gs + q) * stride, stride, cimg.data() + (size_t)(2 * gs + ng + q) * stride);
        }
    }
    std::vector<double> wd((size_t)16 * NT, 0.0);
    std::copy(h->wd.begin(), h->wd.begin() + h->Ntot, wd.begin());
    JvpBuf d_img, d_cimg, d_h0, d_pc, d_pq, d_stream, d_state, d_save, d_work, d_wd, d_res, d_tr, d_R, d_g;
    int rc;
    if ((rc = d_img.alloc(h, img.size())) || (rc = d_cimg.alloc(h, cimg.size())) || (rc = d_h0.alloc(h, (size_t)nvec * stride)) ||
        (rc = d_pc.alloc(h, (size_t)nvec * ncoeff)) || (rc = d_pq.alloc(h, (size_t)nvec * (2 * cs + 1) * 2 * Nc)) ||
        (rc = d_stream.alloc(h, (size_t)nvec * gstride)) || (rc = d_state.alloc(h, (size_t)nblocks * sstride)) ||
        (rc = d_save.alloc(h, nsweeps > 1 ? (size_t)nblocks * sstride : 1)) || (rc = d_work.alloc(h, (size_t)nblocks * JQ_TLB_WORK_VECS * KT * 64)) ||
        (rc = d_wd.alloc(h, wd.size())) || (rc = d_res.alloc(h, (size_t)dpl * 4)) || (rc = d_tr.alloc(h, 2 * trows * cs * ntr_max)) ||
        (rc = d_R.alloc(h, (size_t)nvec * cs * ntr_max)) || (rc = d_g.alloc(h, (size_t)2 * nvec * ncoeff)))
        return rc;
    // d_g: [pass][primal | direction ...][ncoeff]
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(d_img.p, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_cimg.p, cimg.data(), cimg.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemsetAsync(d_h0.p, 0, (size_t)nvec * stride * sizeof(double), s));
    HIPCHK(h, hipMemcpyAsync(d_h0.p, img.data(), stride * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_wd.p, wd.data(), wd.size() * sizeof(double), hipMemcpyHostToDevice, s));

    SplineArgs sp;
    sp.pcof = d_pc.p; sp.cfreq = h->d_cfreq; sp.D1 = D1; sp.Nfreq = h->Nfreq; sp.Ncoupled = Nc; sp.nCoeff = ncoeff;
    sp.dtknot = h->T / (D1 - 2);
    sp.rfreq = nullptr;
    PropArgs a;
    memset(&a, 0, sizeof a);
    a.stream = d_stream.p; a.stream_gstride = (long long)gstride; a.group_units = 1; a.state = d_state.p; a.state_stride = sstride;
    a.park = d_work.p; a.tabs = d_wd.p; a.traces = d_tr.p; a.stride = (long long)stride; a.m = h->m; a.nslabs = nblocks; a.Ntot = h->Ntot;
    a.N = h->N; a.parts = parts; a.nsamples = dpl; a.sps = 1; a.tinv = 1.0 / h->T;

    const int nchunks = (h->nsteps + cs - 1) / cs;
    const size_t nev = 2 + 2 * (size_t)nchunks * rounds * (1 + nsweeps);
    while (h->ev.size() < nev) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreate(&e));
        h->ev.push_back(e);
    }
    size_t evi = 2;
    std::vector<char> ev_bwd;      // per event pair: a backward launch?
    HIPCHK(h, hipEventRecord(h->ev[0], s));
    std::vector<double> res((size_t)dpl * 4), res0(4), blk((size_t)nvec * ncoeff), gbuf((size_t)2 * nvec * ncoeff);
    const double leak_scale = 0.5 * dt * (1.0 / h->T);
    long long mfma_fwd = 0, mfma_bwd = 0;
    for (int r = 0; r < rounds; ++r) {
        const int j0 = r * dpl, nd = std::min(dpl, ndir - j0);      // (a short last round repeats its last direction: every group has a stream)
        std::copy(pcof, pcof + ncoeff, blk.begin());
        for (int j = 0; j < dpl; ++j) std::copy_n(dirs + (size_t)(j0 + std::min(j, nd - 1)) * ncoeff, ncoeff, blk.begin() + (size_t)(1 + j) * ncoeff);
        HIPCHK(h, hipMemcpyAsync(d_pc.p, blk.data(), blk.size() * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemsetAsync(d_g.p, 0, (size_t)2 * nvec * ncoeff * sizeof(double), s));
        // ---- forward sweep of (state, tangent): the launches of jvp_run ----
        hipLaunchKernelGGL(k_init_tl, dim3(nblocks), dim3(64), 0, s, d_state.p, sstride, h->d_uimg, KT, parts, h->N);
        a.h = dt; a.forced = 1; a.period = 7; a.npro = 0; a.Ncoupled = 0; a.cimg = nullptr;
        a.sched_bits[0] = a.sched_bits[1] = a.sched_bits[2] = a.pro_bits = 0;
        for (int i = 0; i < 7; ++i) sched_pack(a.sched_bits, i, JQ_SCHED[1][0][i], JQ_SCHED[1][1][i]);      // Kp05 S05 Kn0 Kn1 S0 S1 Kp05
        for (int n0 = 0; n0 < h->nsteps; n0 += cs) {
            const int nc = std::min(cs, h->nsteps - n0), ntp = 2 * nc + 1;
            hipLaunchKernelGGL(k_ctrl, dim3((ntp + 127) / 128, nvec), dim3(128), 0, s, sp, h->d_tf, n0, ntp, dt, d_pq.p, (const double*)nullptr, (double*)nullptr);
            hipLaunchKernelGGL(k_stream, dim3((unsigned)((stride + 255) / 256), ntp, nvec), dim3(256), 0, s, d_img.p, d_h0.p, (long long)stride, d_pq.p, Nc,
                               (long long)stride, 0.5 * dt, d_stream.p, (long long)gstride);
            a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0);
            HIPCHK(h, hipEventRecord(h->ev[evi++], s));
            hipLaunchKernelGGL(k_forward_tl<>, dim3(nblocks), dim3(64 * JQ_HUGE_WAVES), 0, s, a);
            HIPCHK(h, hipEventRecord(h->ev[evi++], s));
            ev_bwd.push_back(0);
            mfma_fwd += (long long)nblocks * nc * 3 * (8 + 2 * h->m) * NT * KT;
        }
        hipLaunchKernelGGL(k_terminal_hvp, dim3(dpl), dim3(64), 0, s, d_state.p, sstride, h->d_vtr, h->d_vti, KT, h->N, parts, leak_scale, d_res.p);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(res.data(), d_res.p, (size_t)dpl * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
        // ---- backward sweeps: one per (control group, forcing), each from the terminal state ----
        if (nsweeps > 1) HIPCHK(h, hipMemcpyAsync(d_save.p, d_state.p, (size_t)nblocks * sstride * sizeof(double), hipMemcpyDeviceToDevice, s));
        for (int sweep = 0; sweep < nsweeps; ++sweep) {
            const int pass = sweep / ngroups, grp = sweep % ngroups;
            const int q0 = ctrl_gstart(Nc, grp), ng = ctrl_gstart(Nc, grp + 1) - q0, ntr_g = ng * JQ_NTR;
            if (sweep > 0) HIPCHK(h, hipMemcpyAsync(d_state.p, d_save.p, (size_t)nblocks * sstride * sizeof(double), hipMemcpyDeviceToDevice, s));
            a.Ncoupled = ng;
            a.cimg = d_cimg.p + (size_t)2 * q0 * stride;
            a.h = -dt; a.forced = (pass == 0); a.period = 13 + 3 * ng;
            {   // Kp05 S05 Kn0 Kn1 S0 S1 Kp05 | S0 | Hanti_q.. | Kn0 Kn1 S05 Kp05 S1 | (Hanti_q Hsym_q)..   (run_eval)
                const int kinds2[5] = {0, 0, 1, 0, 1}, tps2[5] = {0, 2, 1, 1, 2};
                a.sched_bits[0] = a.sched_bits[1] = a.sched_bits[2] = a.pro_bits = 0;
                int k = 0;
                for (int i = 0; i < 8; ++i) sched_pack(a.sched_bits, k++, JQ_SCHED[1][0][i], JQ_SCHED[1][1][i]);
                for (int q = 0; q < ng; ++q) sched_pack(a.sched_bits, k++, 2, ng + q);
                for (int i = 0; i < 5; ++i) sched_pack(a.sched_bits, k++, kinds2[i], tps2[i]);
                for (int q = 0; q < ng; ++q) {
                    sched_pack(a.sched_bits, k++, 2, ng + q);
                    sched_pack(a.sched_bits, k++, 2, q);
                    sched_pack(&a.pro_bits, q, 2, q);      // first chunk: carry products with Hsym_q
                }
            }
            for (int n0 = 0; n0 < h->nsteps; n0 += cs) {
                const int nc = std::min(cs, h->nsteps - n0), ntp = 2 * nc + 1;
                hipLaunchKernelGGL(k_ctrl, dim3((ntp + 127) / 128, nvec), dim3(128), 0, s, sp, h->d_tb, n0, ntp, -dt, d_pq.p, (const double*)nullptr, (double*)nullptr);
                hipLaunchKernelGGL(k_stream, dim3((unsigned)((stride + 255) / 256), ntp, nvec), dim3(256), 0, s, d_img.p, d_h0.p, (long long)stride, d_pq.p, Nc,
                                   (long long)stride, -0.5 * dt, d_stream.p, (long long)gstride);
                a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0); a.npro = (n0 == 0) ? ng : 0;
                HIPCHK(h, hipEventRecord(h->ev[evi++], s));
                hipLaunchKernelGGL(k_backward_tl<>, dim3(nblocks), dim3(64 * JQ_HUGE_WAVES), 0, s, a);
                HIPCHK(h, hipEventRecord(h->ev[evi++], s));
                ev_bwd.push_back(1);
                const unsigned rblocks = (unsigned)(((long long)nc * ntr_g + 255) / 256);
                const double* d_trd = d_tr.p + trows * nc * ntr_g;      // the tangents' record (k_backward_tl)
                double *d_Rd = d_R.p + (size_t)cs * ntr_max, *gp = d_g.p + (size_t)pass * nvec * ncoeff;
                if (r == 0) {      // the primal record of the first direction's slabs
                    hipLaunchKernelGGL(k_trace_reduce, dim3(rblocks, 1), dim3(256), 0, s, (const double*)d_tr.p, parts * JQ_HUGE_WAVES, nc, ntr_g, d_R.p,
                                       (const double*)nullptr, Nc, q0);
                    hipLaunchKernelGGL(k_gradacc, dim3(ng * 2 * h->Nfreq * D1, 1), dim3(JQ_GRADACC_THREADS), 0, s, sp, (const double*)d_R.p, h->d_tb, n0, nc, -dt,
                                       gp, q0, ng, (long long)ncoeff);
                }
                hipLaunchKernelGGL(k_trace_reduce, dim3(rblocks, dpl), dim3(256), 0, s, d_trd, parts * JQ_HUGE_WAVES, nc, ntr_g, d_Rd, (const double*)nullptr, Nc, q0);
                hipLaunchKernelGGL(k_gradacc, dim3(ng * 2 * h->Nfreq * D1, dpl), dim3(JQ_GRADACC_THREADS), 0, s, sp, (const double*)d_Rd, h->d_tb, n0, nc, -dt,
                                   gp + ncoeff, q0, ng, (long long)ncoeff);
                mfma_bwd += (long long)nblocks * nc * (6 * (8 + 2 * h->m) + 8 * ng) * NT * KT;      // (two MFMAs per tile of a trace product)
                if (n0 == 0) mfma_bwd += (long long)nblocks * 2 * ng * NT * KT;
            }
        }
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(gbuf.data(), d_g.p, gbuf.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));      // (the host blocks are reused by the next round)
        if (r == 0) {
            std::copy_n(res.begin(), 4, res0.begin());      // (the primal of the first direction's workgroups: every direction recomputes the same)
            std::copy_n(gbuf.begin(), ncoeff, grad);
            if (grad_infid) std::copy_n(gbuf.begin() + (size_t)(two_pass ? nvec : 0) * ncoeff, ncoeff, grad_infid);
        }
        for (int j = 0; j < nd; ++j) {
            std::copy_n(gbuf.begin() + (size_t)(1 + j) * ncoeff, ncoeff, hv + (size_t)(j0 + j) * ncoeff);
            if (hv_infid) std::copy_n(gbuf.begin() + (size_t)((two_pass ? nvec : 0) + 1 + j) * ncoeff, ncoeff, hv_infid + (size_t)(j0 + j) * ncoeff);
        }
    }
    HIPCHK(h, hipEventRecord(h->ev[1], s));
    HIPCHK(h, hipStreamSynchronize(s));
    out_record(out4, res0.data());
    h->hvp_per_launch = dpl, h->hvp_chunk = cs, h->hvp_rounds = rounds;

    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->timing = jq_timing{};
    h->timing.ms_total = ms;
    double fwd = 0.0, bwd = 0.0;
    long long nbwd = 0;
    for (size_t i = 2, k = 0; i + 1 < evi; i += 2, ++k) {
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        if (debug_timing()) fprintf(stderr, "jq launch %zu (tangent-linear %s): %.3f ms\n", k, ev_bwd[k] ? "backward" : "forward", ms);
        (ev_bwd[k] ? bwd : fwd) += ms;
        nbwd += ev_bwd[k];
    }
    h->timing.ms_forward = fwd, h->timing.ms_backward = bwd, h->timing.ms_propagate = fwd + bwd;
    h->timing.ms_generate = h->timing.ms_total - (fwd + bwd);
    h->timing.n_forward_launches = (long long)ev_bwd.size() - nbwd;
    h->timing.n_backward_launches = nbwd;
    h->timing.mfma_executed = mfma_fwd + mfma_bwd;
    h->timing.mfma_backward = mfma_bwd;
    h->timing.svts = (long long)ndir * h->N * h->nsteps;
    h->timing.kernel_family = KF_COOP;      // (as the run-time-size kernels report themselves: cooperative, NT tile rows, dense)
    h->timing.kernel_size = NT;
    h->timing.kernel_band = 15;
    h->timing.ms_shard_min = h->timing.ms_shard_max = h->timing.ms_total;
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
        if (h->integrator != 1)
            return fail(h, JQ_EUNSUPPORTED, "jq_traceobjgrad_hvp: the tangent-linear sweeps are the Stormer-Verlet integrator's (no implicit-midpoint tangent)");
        if (h->solver_id != 1)
            return fail(h, JQ_EUNSUPPORTED, "jq_traceobjgrad_hvp: the Jacobi solver's stopping rule has no derivative; use the Neumann solver");
        if (h->wrank > 0)
            return fail(h, JQ_EUNSUPPORTED, "jq_traceobjgrad_hvp: the handle carries full leakage weights (jq_update_wmat); the tangent-linear sweeps "
                                            "weight with params.wmat (Diagonal)");
        if (h->sv_type != 1)
            return fail(h, JQ_EUNSUPPORTED, "jq_traceobjgrad_hvp: sv_type != 1 (continuation adjoints) has no tangent of the terminal condition; set sv_type 1");
        if (!h->rfreq.empty())
            return fail(h, JQ_EUNSUPPORTED, "jq_traceobjgrad_hvp: uncoupled controls (Hunc_ops) are not served; coupled controls only");
        if (int rc = check_ncoeff(h, ncoeff)) return rc;
        DevGate& gate = dev_gate(h->device);
        const bool outer = g_eval_depth++ == 0;
        if (outer) gate.enter();
        struct Leave {      // (also when a host allocation throws)
            DevGate& g;
            bool outer;
            ~Leave()
            {
                if (outer) g.leave();
                --g_eval_depth;
            }
        } leave{gate, outer};
        return hvp_run(h, h->Hconst.data(), pcof, ncoeff, dirs, ndir, out4, grad, hv, hv_infid);
    });
}
