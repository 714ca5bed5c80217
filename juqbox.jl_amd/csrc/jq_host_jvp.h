// jq_host_jvp.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// jq_traceobj_jvp -- the tangent (Jacobian-vector product) of the discrete forward map along directions of coefficient space, on the
// tangent-linear sweep of jq_tl_kernels.h.
//
// A launch of `dpl` directions is a grouped chunk of 1 + dpl tile streams from the generators every sweep uses (k_ctrl over the
// coefficient blocks [pcof | dirs[:, j] ...], k_stream with one drift image per group): group 0 = (pcof, the handle's drift) is the primal
// stream, group 1 + j = (direction j, an all-zero drift image) is the pre-scaled derivative +-c Kd(t), c Sd(t) of the operators along
// direction j -- p_k, q_k and the uncoupled ft are linear in the coefficients, so no operator code of its own is needed.  The images are
// the handle's operators in the dense row-window layout the run-time-size kernels read (band code 15), built here from the host copies for
// ANY Ntot: the call plans nothing and shares no buffer with run_eval -- everything it allocates is released when it returns, and the
// handle keeps only what jq_plan_info and jq_last_timing report about it.
struct JvpBuf {      // device memory of one call
    double* p = nullptr;
    ~JvpBuf() { if (p) (void)hipFree(p); }
    int alloc(jq_handle* h, size_t count)
    {
        if (hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(double)) != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            char buf[160];
            snprintf(buf, sizeof buf, "jq_traceobj_jvp: out of device memory (%zu bytes requested)", std::max<size_t>(count, 1) * sizeof(double));
            return fail(h, JQ_ENOMEM, buf);
        }
        return JQ_OK;
    }
};
#define JQ_JVP_MIN_CHUNK 16      // directions per launch: as many as leave the stream budget room for chunks of this many steps
#define JQ_JVP_MAX_DIRS 4096     // ... and at most this many (workgroups of a launch: directions x parts)

static int jvp_run(jq_handle* h, const double* pcof, int ncoeff, const double* dirs, int ndir, double* out4, double* dout, double* wr, double* wi)
{
    HIPCHK(h, hipSetDevice(h->device));
    const int NT = (h->Ntot + 15) / 16, KT = 4 * NT, Nc = h->Nc, parts = h->parts;
    const size_t stride = (size_t)NT * KT * 64;      // doubles of a dense operator image: tile (mt, kk) at (mt KT + kk) 64
    const size_t nn = (size_t)h->Ntot * h->Ntot, ncol = (size_t)h->Ntot * h->N;
    const int D1 = ncoeff / (2 * Nc * h->Nfreq);
    const double dt = h->T / h->nsteps;

    // directions per launch, chunk length, rounds: 1 + dpl streams of the dense image size within the stream budget (option stream_bytes,
    // default 1 GiB); never longer chunks than the handle's (option chunk_steps)
    size_t budget = ((size_t)1 << 30) / sizeof(double);
    if (h->opt.has(O_STREAM_BYTES) && h->opt.get(O_STREAM_BYTES) > 0) budget = (size_t)h->opt.get(O_STREAM_BYTES) / sizeof(double);
    const long long want = 2LL * std::min(JQ_JVP_MIN_CHUNK, h->nsteps) + 1;
    const long long fit = (long long)(budget / (2 * stride * (size_t)want)) - 1;
    const int dpl = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(ndir, JQ_JVP_MAX_DIRS / parts), fit));
    const long long tps = (long long)(budget / ((size_t)(1 + dpl) * 2 * stride));
    const int cs = (int)std::max<long long>(1, std::min<long long>(std::min(h->chunk_steps, h->nsteps), (tps - 1) / 2));
    const int rounds = (ndir + dpl - 1) / dpl;
    const int nvec = 1 + dpl, nblocks = dpl * parts;
    const size_t gstride = (size_t)(2 * cs + 1) * 2 * stride;
    const long long sstride = (long long)JQ_TL_STATE_ROWS(KT) * 64;

    // operator images [H0 | Hsym_q | Hanti_q], the drift images of the groups [H0 | 0 ...], tables, initial coefficient blocks
    std::vector<double> img((size_t)(1 + 2 * Nc) * stride, 0.0);
    tile_image_coop(h->Hconst.data(), h->Ntot, NT, 15, img.data());
    for (int q = 0; q < Nc; ++q) {
        tile_image_coop(h->Hsym.data() + q * nn, h->Ntot, NT, 15, img.data() + (size_t)(1 + q) * stride);
        tile_image_coop(h->Hanti.data() + q * nn, h->Ntot, NT, 15, img.data() + (size_t)(1 + Nc + q) * stride);
    }
    std::vector<double> wd((size_t)16 * NT, 0.0);
    std::copy(h->wd.begin(), h->wd.begin() + h->Ntot, wd.begin());
    JvpBuf d_img, d_h0, d_pc, d_pq, d_stream, d_state, d_work, d_wd, d_res, d_w;
    int rc;
    if ((rc = d_img.alloc(h, img.size())) || (rc = d_h0.alloc(h, (size_t)nvec * stride)) || (rc = d_pc.alloc(h, (size_t)nvec * ncoeff)) ||
        (rc = d_pq.alloc(h, (size_t)nvec * (2 * cs + 1) * 2 * Nc)) || (rc = d_stream.alloc(h, (size_t)nvec * gstride)) ||
        (rc = d_state.alloc(h, (size_t)nblocks * sstride)) || (rc = d_work.alloc(h, (size_t)nblocks * 2 * TV_COUNT * KT * 64)) ||
        (rc = d_wd.alloc(h, wd.size())) || (rc = d_res.alloc(h, (size_t)dpl * 8)) || (rc = d_w.alloc(h, wr ? (size_t)2 * dpl * ncol : 1)))
        return rc;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(d_img.p, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemsetAsync(d_h0.p, 0, (size_t)nvec * stride * sizeof(double), s));
    HIPCHK(h, hipMemcpyAsync(d_h0.p, img.data(), stride * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_wd.p, wd.data(), wd.size() * sizeof(double), hipMemcpyHostToDevice, s));

    SplineArgs sp;
    sp.pcof = d_pc.p; sp.cfreq = h->d_cfreq; sp.D1 = D1; sp.Nfreq = h->Nfreq; sp.Ncoupled = Nc; sp.nCoeff = ncoeff;
    sp.dtknot = h->T / (D1 - 2);
    sp.rfreq = h->rfreq.empty() ? nullptr : h->d_rfreq;
    PropArgs a;
    memset(&a, 0, sizeof a);
    a.stream = d_stream.p; a.stream_gstride = (long long)gstride; a.group_units = 1; a.state = d_state.p; a.state_stride = sstride;
    a.park = d_work.p; a.tabs = d_wd.p; a.stride = (long long)stride; a.m = h->m; a.nslabs = nblocks; a.Ntot = h->Ntot; a.N = h->N;
    a.parts = parts; a.nsamples = dpl; a.sps = 1; a.tinv = 1.0 / h->T; a.h = dt; a.forced = 1; a.period = 7;
    for (int i = 0; i < 7; ++i) sched_pack(a.sched_bits, i, JQ_SCHED[1][0][i], JQ_SCHED[1][1][i]);      // Kp05 S05 Kn0 Kn1 S0 S1 Kp05

    const int nchunks = (h->nsteps + cs - 1) / cs;
    const size_t nev = 2 + 2 * (size_t)nchunks * rounds;
    while (h->ev.size() < nev) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreate(&e));
        h->ev.push_back(e);
    }
    size_t evi = 2;
    HIPCHK(h, hipEventRecord(h->ev[0], s));
    std::vector<double> res((size_t)ndir * 8), blk((size_t)nvec * ncoeff), wbuf(wr ? (size_t)2 * dpl * ncol : 0);
    std::vector<double> wro(wr ? (size_t)ndir * ncol : 0), wio(wr ? (size_t)ndir * ncol : 0);
    const double leak_scale = 0.5 * dt * (1.0 / h->T);
    for (int r = 0; r < rounds; ++r) {
        const int j0 = r * dpl, nd = std::min(dpl, ndir - j0);      // (a short last round repeats its last direction: every group has a stream)
        std::copy(pcof, pcof + ncoeff, blk.begin());
        for (int j = 0; j < dpl; ++j) std::copy_n(dirs + (size_t)(j0 + std::min(j, nd - 1)) * ncoeff, ncoeff, blk.begin() + (size_t)(1 + j) * ncoeff);
        HIPCHK(h, hipMemcpyAsync(d_pc.p, blk.data(), blk.size() * sizeof(double), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_init_tl, dim3(nblocks), dim3(64), 0, s, d_state.p, sstride, h->d_uimg, KT, parts, h->N);
        for (int n0 = 0; n0 < h->nsteps; n0 += cs) {
            const int nc = std::min(cs, h->nsteps - n0), ntp = 2 * nc + 1;
            hipLaunchKernelGGL(k_ctrl, dim3((ntp + 127) / 128, nvec), dim3(128), 0, s, sp, h->d_tf, n0, ntp, dt, d_pq.p, (const double*)nullptr, (double*)nullptr);
            hipLaunchKernelGGL(k_stream, dim3((unsigned)((stride + 255) / 256), ntp, nvec), dim3(256), 0, s, d_img.p, d_h0.p, (long long)stride, d_pq.p, Nc,
                               (long long)stride, 0.5 * dt, d_stream.p, (long long)gstride);
            a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0);
            HIPCHK(h, hipEventRecord(h->ev[evi++], s));
            hipLaunchKernelGGL(k_forward_tl<>, dim3(nblocks), dim3(64 * JQ_HUGE_WAVES), 0, s, a);
            HIPCHK(h, hipEventRecord(h->ev[evi++], s));
        }
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
    HIPCHK(h, hipEventRecord(h->ev[1], s));
    HIPCHK(h, hipStreamSynchronize(s));

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

    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->timing = jq_timing{};
    h->timing.ms_total = ms;
    double fwd = 0.0;
    for (size_t i = 2; i + 1 < evi; i += 2) {
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        if (debug_timing()) fprintf(stderr, "jq launch %zu (tangent-linear forward): %.3f ms\n", (i - 2) / 2, ms);
        fwd += ms;
    }
    h->timing.ms_forward = h->timing.ms_propagate = fwd;
    h->timing.ms_generate = h->timing.ms_total - fwd;
    h->timing.n_forward_launches = (long long)((evi - 2) / 2);
    h->timing.mfma_executed = (long long)rounds * nblocks * h->nsteps * 3 * (8 + 2 * h->m) * NT * KT;
    h->timing.svts = (long long)ndir * h->N * h->nsteps;
    h->timing.kernel_family = KF_COOP;      // (as the run-time-size kernels report themselves: cooperative, NT tile rows, dense)
    h->timing.kernel_size = NT;
    h->timing.kernel_band = 15;
    h->timing.ms_shard_min = h->timing.ms_shard_max = h->timing.ms_total;
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
        if (h->integrator != 1)
            return fail(h, JQ_EUNSUPPORTED, "jq_traceobj_jvp: the tangent-linear sweep is the Stormer-Verlet integrator's (no implicit-midpoint tangent)");
        if (h->solver_id != 1)
            return fail(h, JQ_EUNSUPPORTED, "jq_traceobj_jvp: the Jacobi solver's stopping rule has no derivative; use the Neumann solver");
        if (h->wrank > 0)
            return fail(h, JQ_EUNSUPPORTED, "jq_traceobj_jvp: the handle carries full leakage weights (jq_update_wmat); the tangent-linear sweep "
                                            "weights with params.wmat (Diagonal)");
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
        return jvp_run(h, pcof, ncoeff, dirs, ndir, out4, dout, wr, wi);
    });
}
