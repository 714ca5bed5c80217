// jq_host_jvp.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// jq_traceobj_jvp -- the tangent (Jacobian-vector product) of the discrete forward map along directions of coefficient space, on the
// tangent-linear sweep of jq_tl_kernels.h.
//
// Per round of `dpl` directions (jq_host_tl.h: the grouped chunk of 1 + dpl tile streams, budgeting, timing) the forward sweep
// k_forward_tl chunk by chunk on the handle's operators in the dense row-window layout, built here from the host copies for ANY Ntot;
// k_terminal_tl then writes the objective's record, its derivative and (wr, wi) the tangent of the final state.
static int jvp_run(jq_handle* h, const double* pcof, int ncoeff, const double* dirs, int ndir, double* out4, double* dout, double* wr, double* wi)
{
    const char* who = "jq_traceobj_jvp";
    HIPCHK(h, hipSetDevice(h->device));
    const int NT = (h->Ntot + 15) / 16, KT = 4 * NT, Nc = h->Nc, parts = h->parts;
    const size_t stride = (size_t)NT * KT * 64;      // doubles of a dense operator image: tile (mt, kk) at (mt KT + kk) 64
    const size_t ncol = (size_t)h->Ntot * h->N;
    const TlBudget b = tl_budget(h, stride, ndir, JQ_JVP_MAX_DIRS / parts, 0);
    const int dpl = b.dpl, cs = b.cs, rounds = b.rounds, nvec = 1 + dpl, nblocks = dpl * parts;
    const long long sstride = (long long)JQ_TL_STATE_ROWS(KT) * 64;

    const std::vector<double> img = tl_dense_images(h, h->Hconst.data());
    std::vector<double> wd((size_t)16 * NT, 0.0);
    std::copy(h->wd.begin(), h->wd.begin() + h->Ntot, wd.begin());
    DevBuf d_img, d_h0, d_pc, d_pq, d_stream, d_state, d_work, d_wd, d_res, d_w;
    int rc;
    if ((rc = d_img.alloc(h, who, img.size())) || (rc = d_h0.alloc(h, who, (size_t)nvec * stride)) || (rc = d_pc.alloc(h, who, (size_t)nvec * ncoeff)) ||
        (rc = d_pq.alloc(h, who, (size_t)nvec * (2 * cs + 1) * 2 * Nc)) || (rc = d_stream.alloc(h, who, (size_t)nvec * b.gstride)) ||
        (rc = d_state.alloc(h, who, (size_t)nblocks * sstride)) || (rc = d_work.alloc(h, who, (size_t)nblocks * 2 * TV_COUNT * KT * 64)) ||
        (rc = d_wd.alloc(h, who, wd.size())) || (rc = d_res.alloc(h, who, (size_t)dpl * 8)) || (rc = d_w.alloc(h, who, wr ? (size_t)2 * dpl * ncol : 1)))
        return rc;
    hipStream_t s = h->stream;
    if ((rc = tl_upload_dense(h, img, wd, stride, nvec, d_img.p, d_h0.p, d_wd.p))) return rc;
    const TlGen gen = {tl_spline(h, d_pc.p, ncoeff, h->rfreq.empty() ? nullptr : h->d_rfreq), d_img.p, d_h0.p, d_pq.p, d_stream.p, stride, b.gstride, nvec};
    PropArgs a = tl_prop_args(h, gen, dpl, d_state.p, sstride, d_work.p, d_wd.p);

    LaunchTimer tm{h};
    if ((rc = tm.start((size_t)b.nchunks * rounds))) return rc;
    std::vector<double> res((size_t)ndir * 8), blk((size_t)nvec * ncoeff), wbuf(wr ? (size_t)2 * dpl * ncol : 0);
    std::vector<double> wro(wr ? (size_t)ndir * ncol : 0), wio(wr ? (size_t)ndir * ncol : 0);
    const double leak_scale = 0.5 * (h->T / h->nsteps) * (1.0 / h->T);
    for (int r = 0; r < rounds; ++r) {
        const int j0 = r * dpl, nd = std::min(dpl, ndir - j0);
        if ((rc = tl_upload_round(h, blk, d_pc.p, pcof, dirs, j0, nd, dpl, ncoeff))) return rc;
        if ((rc = tl_forward_sweep(h, a, gen, cs, tm))) return rc;
        hipLaunchKernelGGL(k_terminal_tl, dim3(dpl), dim3(64), 0, s, d_state.p, sstride, h->d_vtr, h->d_vti, KT, h->Ntot, h->N, parts, leak_scale,
                           d_res.p, wr ? d_w.p : nullptr, wr ? d_w.p + (size_t)dpl * ncol : nullptr);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(res.data() + (size_t)j0 * 8, d_res.p, (size_t)nd * 8 * sizeof(double), hipMemcpyDeviceToHost, s));
        if (wr) HIPCHK(h, hipMemcpyAsync(wbuf.data(), d_w.p, wbuf.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));      // (the host blocks are reused by the next round)
        if (wr) {
            std::copy_n(wbuf.begin(), (size_t)nd * ncol, wro.begin() + (size_t)j0 * ncol);
            std::copy_n(wbuf.begin() + (size_t)dpl * ncol, (size_t)nd * ncol, wio.begin() + (size_t)j0 * ncol);
        }
    }
    if ((rc = tm.stop())) return rc;

    out_record(out4, res.data());      // (the primal of the first direction's workgroups: every direction recomputes the same)
    for (int j = 0; j < ndir; ++j) {
        const double dp = res[(size_t)j * 8 + 4], dsec = res[(size_t)j * 8 + 5];
        dout[(size_t)3 * j] = dp + dsec, dout[(size_t)3 * j + 1] = dp, dout[(size_t)3 * j + 2] = dsec;
    }
    if (wr) {
        std::copy(wro.begin(), wro.end(), wr);
        std::copy(wio.begin(), wio.end(), wi);
    }
    h->jvp_per_launch = dpl, h->jvp_chunk = cs, h->jvp_rounds = rounds;

    if ((rc = tm.finish("tangent-linear"))) return rc;
    h->timing.mfma_executed = tl_forward_mfma(h, rounds, nblocks);
    h->timing.svts = (long long)ndir * h->N * h->nsteps;
    h->timing.kernel_family = KF_COOP;      // (as the run-time-size kernels report themselves: cooperative, NT tile rows, dense)
    h->timing.kernel_size = NT;
    h->timing.kernel_band = 15;
    return JQ_OK;
}

extern "C" int jq_traceobj_jvp(jq_handle* h, const double* pcof, int32_t ncoeff, const double* dirs, int32_t ndir, double* out4, double* dout,
                               double* wr, double* wi)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_traceobj_jvp", [&]() -> int {
        if (!pcof || !dirs || !out4 || !dout) return fail(h, JQ_EINVAL, "jq_traceobj_jvp: NULL pointer");
        if (ndir < 1) return fail(h, JQ_EINVAL, "jq_traceobj_jvp: ndir must be >= 1");
        if ((wr == nullptr) != (wi == nullptr)) return fail(h, JQ_EINVAL, "jq_traceobj_jvp: wr and wi are given together or not at all");
        JQ_ON_FIRST(h, jq_traceobj_jvp(s0_, pcof, ncoeff, dirs, ndir, out4, dout, wr, wi))
        if (int rc = tl_refuse(h, "jq_traceobj_jvp", false)) return rc;
        if (int rc = check_ncoeff(h, ncoeff)) return rc;
        EvalGate gate(h);
        return jvp_run(h, pcof, ncoeff, dirs, ndir, out4, dout, wr, wi);
    });
}
