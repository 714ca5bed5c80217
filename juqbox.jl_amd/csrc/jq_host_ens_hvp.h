// jq_host_ens_hvp.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// jq_eval_f_g_grad_hvp -- jq_eval_f_g_grad and the derivative of its two gradients along directions of coefficient space: Hessian-vector
// products of a risk-neutral ensemble, sum_i w_i d/d eps grad_i(alpha + eps d) over the quadrature nodes i.
//
// Lane route (Ntot <= 6 padded to NP = 2, 4, 6; at most JQ_MAXNC controls): the tangent-linear lane kernels of jq_lane_tl_kernels.h, all
// N nquad columns x `dpl` directions in ONE launch per chunk -- the nodes fill the lanes, the directions the grid.  The chunk is the
// grouped chunk of hvp_run (jq_host_hvp.h) in the lane image layout: group 0 the primal stream at pcof, group 1 + j the stream of
// direction j (k_ctrl / k_stream with the direction as coefficient vector and a zero drift image).  After every k_backward_lane_tl launch
// k_trace_reduce / k_gradacc run on the primal record of the round's first direction into the gradient (first round only) and on the
// tangent records into hv; objFuncType != 1 repeats the backward sweep unforced from the saved terminal state for the infidelity part.
// Directions per launch, chunk length and rounds are budgeted against option stream_bytes like hvp_run's.  A direction's arithmetic
// does not depend on the launch it rides in.  The call reads the handle's lane images and time tables, allocates everything it writes
// and frees it when it returns.
//
// Sequential route (everything else jq_traceobjgrad_hvp serves: Ntot > 6, option lane=0, more than JQ_MAXNC controls): the nodes one
// after the other through hvp_run with the drift Hconst + eps_i diag(shift) -- correct and no faster.
static double ens_hvp_shift(const double* shift, int i) { return shift ? shift[i] : (i >= 1 ? 0.01 * pow(10.0, (double)(i - 1)) : 0.0); }

struct EnsHvpArgs {
    const double *pcof, *dirs, *nodes, *weights, *shift;
    int ncoeff, ndir, nquad;
    double *out2, *infid_grad, *leak_grad, *hv_infid, *hv_leak;
};
// the four outputs from the forced (g0, v0) and unforced (g1, v1; objFuncType != 1 only) gradients and products (out_grads' rule)
static void ens_hvp_outputs(const jq_handle* h, const EnsHvpArgs& x, const double* g0, const double* g1, const double* v0, const double* v1)
{
    const bool two = h->objFuncType != 1;
    out_grads(h, x.ncoeff, g0, g1, nullptr, x.infid_grad, x.leak_grad);
    for (size_t i = 0; i < (size_t)x.ncoeff * x.ndir; ++i) {
        x.hv_infid[i] = two ? v1[i] : v0[i];
        x.hv_leak[i] = two ? v0[i] - v1[i] : 0.0;
    }
}

static int ens_hvp_lane(jq_handle* h, const EnsHvpArgs& x, prop_kernel_t kinit, prop_kernel_t kfwd, prop_kernel_t kterm, prop_kernel_t kbwd, const KernelSel& sel)
{
    HIPCHK(h, hipSetDevice(h->device));
    const int NP = h->lane_np, Nc = h->Nc, ncoeff = x.ncoeff, ndir = x.ndir, nquad = x.nquad;
    const size_t stride = (size_t)h->lane_stride;
    const long long ncols_used = (long long)nquad * h->N, ncols = (ncols_used + 63) / 64 * 64;
    const int nwaves = (int)(ncols / 64), ntr = Nc * JQ_NTR;
    const int D1 = ncoeff / (2 * Nc * h->Nfreq);
    const double dt = h->T / h->nsteps;
    const bool two_pass = h->objFuncType != 1;
    const int npass = two_pass ? 2 : 1;
    const size_t sstride = (size_t)JQ_LANE_TL_ROWS(NP) * (size_t)ncols;      // doubles of one direction's state file

    // directions per launch, chunk length, rounds (hvp_run's budgeting): 1 + dpl streams and the two trace records of a chunk
    size_t budget = ((size_t)1 << 30) / sizeof(double);
    if (h->opt.has(O_STREAM_BYTES) && h->opt.get(O_STREAM_BYTES) > 0) budget = (size_t)h->opt.get(O_STREAM_BYTES) / sizeof(double);
    const long long want = 2LL * std::min(JQ_JVP_MIN_CHUNK, h->nsteps) + 1;
    const long long fit = (long long)(budget / (2 * stride * (size_t)want)) - 1;
    const int dpl = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(ndir, JQ_JVP_MAX_DIRS), fit));
    const long long tps = (long long)(budget / ((size_t)(1 + dpl) * 2 * stride));
    const long long trc = (long long)(budget / ((size_t)2 * dpl * nwaves * ntr));
    const int cs = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(std::min(h->chunk_steps, h->nsteps), (tps - 1) / 2), trc));
    const int rounds = (ndir + dpl - 1) / dpl, nvec = 1 + dpl;
    const size_t gstride = (size_t)(2 * cs + 1) * 2 * stride;
    const size_t trec = (size_t)dpl * nwaves * cs * ntr;      // doubles of one trace record

    // tables [wd | ws], column info [eps | weight] (run_eval's for the lane layout), drift images of the groups [H0 | 0 ...]
    std::vector<double> tabs((size_t)2 * NP, 0.0), colinfo((size_t)2 * ncols, 0.0);
    bool use_shift = false;
    for (int i = 0; i < h->Ntot; ++i) tabs[i] = h->wd[i], tabs[NP + i] = ens_hvp_shift(x.shift, i);
    for (long long c = 0; c < ncols_used; ++c) {
        const int smp = (int)(c / h->N);
        colinfo[c] = x.nodes[smp];
        colinfo[ncols + c] = x.weights[smp];
        if (x.nodes[smp] != 0.0) use_shift = true;
    }
    JvpBuf d_h0, d_pc, d_pq, d_stream, d_state, d_save, d_tabs, d_col, d_res, d_tr, d_R, d_g;
    int rc;
    if ((rc = d_h0.alloc(h, (size_t)nvec * stride)) || (rc = d_pc.alloc(h, (size_t)nvec * ncoeff)) || (rc = d_pq.alloc(h, (size_t)nvec * (2 * cs + 1) * 2 * Nc)) ||
        (rc = d_stream.alloc(h, (size_t)nvec * gstride)) || (rc = d_state.alloc(h, (size_t)dpl * sstride)) ||
        (rc = d_save.alloc(h, two_pass ? (size_t)dpl * sstride : 1)) || (rc = d_tabs.alloc(h, tabs.size())) || (rc = d_col.alloc(h, colinfo.size())) ||
        (rc = d_res.alloc(h, (size_t)dpl * nquad * 4)) || (rc = d_tr.alloc(h, 2 * trec)) || (rc = d_R.alloc(h, (size_t)nvec * cs * ntr)) ||
        (rc = d_g.alloc(h, (size_t)2 * nvec * ncoeff)))
        return rc;
    // d_g: [pass][primal | direction ...][ncoeff]
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemsetAsync(d_h0.p, 0, (size_t)nvec * stride * sizeof(double), s));
    HIPCHK(h, hipMemcpyAsync(d_h0.p, h->d_himg_l, stride * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_tabs.p, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_col.p, colinfo.data(), colinfo.size() * sizeof(double), hipMemcpyHostToDevice, s));

    SplineArgs sp;
    sp.pcof = d_pc.p; sp.cfreq = h->d_cfreq; sp.D1 = D1; sp.Nfreq = h->Nfreq; sp.Ncoupled = Nc; sp.nCoeff = ncoeff;
    sp.dtknot = h->T / (D1 - 2);
    sp.rfreq = nullptr;
    PropArgs a;
    memset(&a, 0, sizeof a);
    a.stream = d_stream.p; a.stream_gstride = (long long)gstride; a.group_units = 1; a.state = d_state.p; a.state_stride = (long long)sstride;
    a.colinfo = d_col.p; a.tabs = d_tabs.p; a.traces = d_tr.p; a.cimg = h->d_cimg_l; a.stride = (long long)stride; a.m = h->m; a.nslabs = (int)ncols;
    a.Ncoupled = Nc; a.Ntot = h->Ntot; a.N = h->N; a.parts = 1; a.nsamples = nquad; a.sps = 1; a.tinv = 1.0 / h->T; a.use_shift = use_shift ? 1 : 0;
    PropArgs ai = a, at = a;      // the init and terminal kernels read their images and scalars through the fields jq_lane_tl_kernels.h names
    ai.cimg = h->d_uinit_l;
    at.cimg = h->d_vtr_l; at.tabs = h->d_vti_l; at.traces = d_res.p; at.h = 0.5 * dt * (1.0 / h->T);

    const int nchunks = (h->nsteps + cs - 1) / cs;
    const size_t nev = 2 + 2 * (size_t)nchunks * rounds * (1 + npass);
    while (h->ev.size() < nev) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreate(&e));
        h->ev.push_back(e);
    }
    size_t evi = 2;
    std::vector<char> ev_bwd;      // per event pair: a backward launch?
    HIPCHK(h, hipEventRecord(h->ev[0], s));
    std::vector<double> res((size_t)nquad * 4), blk((size_t)nvec * ncoeff), gbuf((size_t)2 * nvec * ncoeff);
    std::vector<double> g0(ncoeff), g1(two_pass ? ncoeff : 0), v0((size_t)ncoeff * ndir), v1(two_pass ? (size_t)ncoeff * ndir : 0);
    const dim3 grid((unsigned)nwaves, (unsigned)dpl);
    for (int r = 0; r < rounds; ++r) {
        const int j0 = r * dpl, nd = std::min(dpl, ndir - j0);      // (a short last round repeats its last direction: every group has a stream)
        std::copy(x.pcof, x.pcof + ncoeff, blk.begin());
        for (int j = 0; j < dpl; ++j) std::copy_n(x.dirs + (size_t)(j0 + std::min(j, nd - 1)) * ncoeff, ncoeff, blk.begin() + (size_t)(1 + j) * ncoeff);
        HIPCHK(h, hipMemcpyAsync(d_pc.p, blk.data(), blk.size() * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemsetAsync(d_g.p, 0, (size_t)2 * nvec * ncoeff * sizeof(double), s));
        // ---- forward sweep of (state, tangent) ----
        hipLaunchKernelGGL(kinit, grid, dim3(64), 0, s, ai);
        a.h = dt; a.forced = 1;
        for (int n0 = 0; n0 < h->nsteps; n0 += cs) {
            const int nc = std::min(cs, h->nsteps - n0), ntp = 2 * nc + 1;
            hipLaunchKernelGGL(k_ctrl, dim3((ntp + 127) / 128, nvec), dim3(128), 0, s, sp, h->d_tf, n0, ntp, dt, d_pq.p, (const double*)nullptr, (double*)nullptr);
            hipLaunchKernelGGL(k_stream, dim3((unsigned)((stride + 255) / 256), ntp, nvec), dim3(256), 0, s, h->d_himg_l, d_h0.p, (long long)stride, d_pq.p, Nc,
                               (long long)stride, 0.5 * dt, d_stream.p, (long long)gstride);
            a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0);
            HIPCHK(h, hipEventRecord(h->ev[evi++], s));
            hipLaunchKernelGGL(kfwd, grid, dim3(64), 0, s, a);
            HIPCHK(h, hipEventRecord(h->ev[evi++], s));
            ev_bwd.push_back(0);
        }
        hipLaunchKernelGGL(kterm, dim3((unsigned)((nquad + 63) / 64), (unsigned)dpl), dim3(64), 0, s, at);
        HIPCHK(h, hipGetLastError());
        if (r == 0) HIPCHK(h, hipMemcpyAsync(res.data(), d_res.p, (size_t)nquad * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
        // ---- backward sweeps: forced, then (objFuncType != 1) unforced from the saved terminal state ----
        if (two_pass) HIPCHK(h, hipMemcpyAsync(d_save.p, d_state.p, (size_t)dpl * sstride * sizeof(double), hipMemcpyDeviceToDevice, s));
        for (int pass = 0; pass < npass; ++pass) {
            if (pass > 0) HIPCHK(h, hipMemcpyAsync(d_state.p, d_save.p, (size_t)dpl * sstride * sizeof(double), hipMemcpyDeviceToDevice, s));
            a.h = -dt; a.forced = (pass == 0);
            for (int n0 = 0; n0 < h->nsteps; n0 += cs) {
                const int nc = std::min(cs, h->nsteps - n0), ntp = 2 * nc + 1;
                hipLaunchKernelGGL(k_ctrl, dim3((ntp + 127) / 128, nvec), dim3(128), 0, s, sp, h->d_tb, n0, ntp, -dt, d_pq.p, (const double*)nullptr, (double*)nullptr);
                hipLaunchKernelGGL(k_stream, dim3((unsigned)((stride + 255) / 256), ntp, nvec), dim3(256), 0, s, h->d_himg_l, d_h0.p, (long long)stride, d_pq.p, Nc,
                                   (long long)stride, -0.5 * dt, d_stream.p, (long long)gstride);
                a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0);
                HIPCHK(h, hipEventRecord(h->ev[evi++], s));
                hipLaunchKernelGGL(kbwd, grid, dim3(64), 0, s, a);
                HIPCHK(h, hipEventRecord(h->ev[evi++], s));
                ev_bwd.push_back(1);
                const unsigned rblocks = (unsigned)(((long long)nc * ntr + 255) / 256);
                const double* d_trd = d_tr.p + (size_t)dpl * nwaves * nc * ntr;      // the tangents' record (k_backward_lane_tl)
                double *d_Rd = d_R.p + (size_t)cs * ntr, *gp = d_g.p + (size_t)pass * nvec * ncoeff;
                if (r == 0) {      // the primal record of the first direction
                    hipLaunchKernelGGL(k_trace_reduce, dim3(rblocks, 1), dim3(256), 0, s, (const double*)d_tr.p, nwaves, nc, ntr, d_R.p, (const double*)nullptr, Nc, 0);
                    hipLaunchKernelGGL(k_gradacc, dim3(Nc * 2 * h->Nfreq * D1, 1), dim3(JQ_GRADACC_THREADS), 0, s, sp, (const double*)d_R.p, h->d_tb, n0, nc, -dt, gp, 0, Nc,
                                       (long long)ncoeff);
                }
                hipLaunchKernelGGL(k_trace_reduce, dim3(rblocks, dpl), dim3(256), 0, s, d_trd, nwaves, nc, ntr, d_Rd, (const double*)nullptr, Nc, 0);
                hipLaunchKernelGGL(k_gradacc, dim3(Nc * 2 * h->Nfreq * D1, dpl), dim3(JQ_GRADACC_THREADS), 0, s, sp, (const double*)d_Rd, h->d_tb, n0, nc, -dt, gp + ncoeff, 0,
                                   Nc, (long long)ncoeff);
            }
        }
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(gbuf.data(), d_g.p, gbuf.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));      // (the host blocks are reused by the next round)
        if (r == 0) {
            std::copy_n(gbuf.begin(), ncoeff, g0.begin());
            if (two_pass) std::copy_n(gbuf.begin() + (size_t)nvec * ncoeff, ncoeff, g1.begin());
        }
        for (int j = 0; j < nd; ++j) {
            std::copy_n(gbuf.begin() + (size_t)(1 + j) * ncoeff, ncoeff, v0.begin() + (size_t)(j0 + j) * ncoeff);
            if (two_pass) std::copy_n(gbuf.begin() + (size_t)(nvec + 1 + j) * ncoeff, ncoeff, v1.begin() + (size_t)(j0 + j) * ncoeff);
        }
    }
    HIPCHK(h, hipEventRecord(h->ev[1], s));
    HIPCHK(h, hipStreamSynchronize(s));
    double inf = 0.0, leak = 0.0;
    for (int i = 0; i < nquad; ++i) {      // (jq_eval_f_g_grad's sums)
        inf += res[(size_t)i * 4 + 0] * x.weights[i];
        leak += res[(size_t)i * 4 + 1] * x.weights[i];
    }
    x.out2[0] = inf, x.out2[1] = leak;
    ens_hvp_outputs(h, x, g0.data(), g1.data(), v0.data(), v1.data());
    h->ens_hvp_route = 1, h->ens_hvp_per_launch = dpl, h->ens_hvp_chunk = cs, h->ens_hvp_rounds = rounds;

    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->timing = jq_timing{};
    h->timing.ms_total = ms;
    double fwd = 0.0, bwd = 0.0;
    long long nbwd = 0;
    for (size_t i = 2, k = 0; i + 1 < evi; i += 2, ++k) {
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        if (debug_timing()) fprintf(stderr, "jq launch %zu (tangent-linear lane %s): %.3f ms\n", k, ev_bwd[k] ? "backward" : "forward", ms);
        (ev_bwd[k] ? bwd : fwd) += ms;
        nbwd += ev_bwd[k];
    }
    h->timing.ms_forward = fwd, h->timing.ms_backward = bwd, h->timing.ms_propagate = fwd + bwd;
    h->timing.ms_generate = h->timing.ms_total - (fwd + bwd);
    h->timing.n_forward_launches = (long long)ev_bwd.size() - nbwd;
    h->timing.n_backward_launches = nbwd;
    h->timing.svts = (long long)ndir * nquad * h->N * h->nsteps;
    h->timing.kernel_family = KF_LANE;
    h->timing.kernel_size = NP;
    h->timing.kernel_band = 0;
    h->timing.ms_shard_min = h->timing.ms_shard_max = h->timing.ms_total;
    h->last_kernels = sel;
    return JQ_OK;
}

static int ens_hvp_sequential(jq_handle* h, const EnsHvpArgs& x)
{
    const int ncoeff = x.ncoeff, ndir = x.ndir, Ntot = h->Ntot;
    const bool two_pass = h->objFuncType != 1;
    const size_t nv = (size_t)ncoeff * ndir;
    std::vector<double> drift, g0(ncoeff, 0.0), g1(two_pass ? ncoeff : 0, 0.0), v0(nv, 0.0), v1(two_pass ? nv : 0, 0.0);
    std::vector<double> gi(ncoeff), gin(ncoeff), vi(nv), vin(nv);
    double inf = 0.0, leak = 0.0, out4[4];
    jq_timing sum = jq_timing{};
    const int keep[3] = {h->hvp_per_launch, h->hvp_chunk, h->hvp_rounds};      // ("hvp" of jq_plan_info stays jq_traceobjgrad_hvp's)
    int rc = JQ_OK, dpl = 0, cs = 0, rounds = 0;
    for (int i = 0; i < x.nquad && rc == JQ_OK; ++i) {
        drift = h->Hconst;
        for (int j = 0; j < Ntot; ++j) drift[(size_t)j * Ntot + j] += x.nodes[i] * ens_hvp_shift(x.shift, j);      // src/ipopt_interface.jl:41-44
        rc = hvp_run(h, drift.data(), x.pcof, ncoeff, x.dirs, ndir, out4, gi.data(), vi.data(), vin.data(), gin.data());
        if (rc != JQ_OK) break;
        const double w = x.weights[i];
        inf += out4[1] * w, leak += out4[2] * w;
        for (int k = 0; k < ncoeff; ++k) {
            g0[k] += w * gi[k];
            if (two_pass) g1[k] += w * gin[k];
        }
        for (size_t k = 0; k < nv; ++k) {
            v0[k] += w * vi[k];
            if (two_pass) v1[k] += w * vin[k];
        }
        const jq_timing t = h->timing;
        if (i == 0) sum = t;
        else timing_add(sum, t);
        dpl = h->hvp_per_launch, cs = h->hvp_chunk, rounds += h->hvp_rounds;
    }
    h->hvp_per_launch = keep[0], h->hvp_chunk = keep[1], h->hvp_rounds = keep[2];
    if (rc != JQ_OK) return rc;
    x.out2[0] = inf, x.out2[1] = leak;
    ens_hvp_outputs(h, x, g0.data(), g1.data(), v0.data(), v1.data());
    h->timing = sum;
    h->timing.ms_shard_min = h->timing.ms_shard_max = h->timing.ms_total;
    h->ens_hvp_route = 2, h->ens_hvp_per_launch = dpl, h->ens_hvp_chunk = cs, h->ens_hvp_rounds = rounds;
    return JQ_OK;
}

extern "C" int jq_eval_f_g_grad_hvp(jq_handle* h, const double* pcof, int32_t ncoeff, const double* dirs, int32_t ndir, const double* nodes,
                                    const double* weights, int32_t nquad, const double* shift, double* out2, double* infid_grad, double* leak_grad,
                                    double* hv_infid, double* hv_leak)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_eval_f_g_grad_hvp", [&]() -> int {
        if (!pcof || !dirs || !nodes || !weights || !out2 || !infid_grad || !leak_grad || !hv_infid || !hv_leak)
            return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_hvp: NULL pointer");
        if (ndir < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_hvp: ndir must be >= 1");
        if (nquad < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_hvp: nquad must be >= 1");
        JQ_ON_FIRST(h, jq_eval_f_g_grad_hvp(s0_, pcof, ncoeff, dirs, ndir, nodes, weights, nquad, shift, out2, infid_grad, leak_grad, hv_infid, hv_leak))
        // (the refusals of jq_traceobjgrad_hvp)
        if (h->integrator != 1)
            return fail(h, JQ_EUNSUPPORTED, "jq_eval_f_g_grad_hvp: the tangent-linear sweeps are the Stormer-Verlet integrator's (no implicit-midpoint tangent)");
        if (h->solver_id != 1)
            return fail(h, JQ_EUNSUPPORTED, "jq_eval_f_g_grad_hvp: the Jacobi solver's stopping rule has no derivative; use the Neumann solver");
        if (h->wrank > 0)
            return fail(h, JQ_EUNSUPPORTED, "jq_eval_f_g_grad_hvp: the handle carries full leakage weights (jq_update_wmat); the tangent-linear sweeps "
                                            "weight with params.wmat (Diagonal)");
        if (h->sv_type != 1)
            return fail(h, JQ_EUNSUPPORTED, "jq_eval_f_g_grad_hvp: sv_type != 1 (continuation adjoints) has no tangent of the terminal condition; set sv_type 1");
        if (!h->rfreq.empty())
            return fail(h, JQ_EUNSUPPORTED, "jq_eval_f_g_grad_hvp: uncoupled controls (Hunc_ops) are not served; coupled controls only");
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
        const EnsHvpArgs x = {pcof, dirs, nodes, weights, shift, ncoeff, ndir, nquad, out2, infid_grad, leak_grad, hv_infid, hv_leak};
        // lane route: the tangent-linear lane kernels exist for the handle's NP and one pass takes its controls; independent of the column
        // bounds of the lane GRADIENT kernels (options lane_min / lane_max): one node is served here too
        if (h->lane_np > 0 && h->Nc <= JQ_MAXNC) {
            KernelSel sel = sel_start();
            char unused[JQ_SEL_TAG];
            const int np = h->lane_np;
            const prop_kernel_t kfwd = pick(sel.fwd, np, -1, "k_forward_lane_tl", {np}), kbwd = pick(sel.bwd, np, -1, "k_backward_lane_tl", {np});
            const prop_kernel_t kinit = pick(unused, np, -1, "k_init_lane_tl", {np}), kterm = pick(unused, np, -1, "k_terminal_lane_tl", {np});
            if (kfwd && kbwd && kinit && kterm) return ens_hvp_lane(h, x, kinit, kfwd, kterm, kbwd, sel);
        }
        return ens_hvp_sequential(h, x);
    });
}
