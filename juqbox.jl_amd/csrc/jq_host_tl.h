// jq_host_tl.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// what the drivers of the tangent-linear sweeps share -- jvp_run (jq_host_jvp.h), hvp_run (jq_host_hvp.h), ens_hvp_lane (jq_host_ens_hvp.h).
//
// A launch of `dpl` directions is a grouped chunk of 1 + dpl tile streams from the generators every sweep uses (k_ctrl over the
// coefficient blocks [pcof | dirs[:, j] ...], k_stream with one drift image per group): group 0 = (pcof, the drift) is the primal
// stream, group 1 + j = (direction j, an all-zero drift image) is the pre-scaled derivative +-c Kd(t), c Sd(t) of the operators along
// direction j -- p_k, q_k and the uncoupled ft are linear in the coefficients, so no operator code of its own is needed.  The directions
// run in rounds of dpl; a direction's arithmetic does not depend on the launch it rides in.  A call plans nothing and shares no buffer
// with run_eval: everything it allocates (DevBuf) is released when it returns, and the handle keeps only what jq_plan_info and
// jq_last_timing report about it.
struct DevBuf {      // device memory of one call (who: the entry point that runs)
    double* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(jq_handle* h, const char* who, size_t count)
    {
        if (hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(double)) != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            char buf[160];
            snprintf(buf, sizeof buf, "%s: out of device memory (%zu bytes requested)", who, std::max<size_t>(count, 1) * sizeof(double));
            return fail(h, JQ_ENOMEM, buf);
        }
        return JQ_OK;
    }
};

// What the tangent-linear sweeps do not serve, in the order every entry point reports it: three refusals of the forward sweep, two more
// of the tangent of the adjoint sweep.
static int tl_refuse(jq_handle* h, const char* who, bool with_adjoint)
{
    const std::string w = std::string(who) + ": ";
    if (h->integrator != 1)
        return fail(h, JQ_EUNSUPPORTED, (w + "the tangent-linear sweeps are the Stormer-Verlet integrator's (no implicit-midpoint tangent)").c_str());
    if (h->solver_id != 1) return fail(h, JQ_EUNSUPPORTED, (w + "the Jacobi solver's stopping rule has no derivative; use the Neumann solver").c_str());
    if (h->wrank > 0)
        return fail(h, JQ_EUNSUPPORTED, (w + "the handle carries full leakage weights (jq_update_wmat); the tangent-linear sweeps weight with params.wmat (Diagonal)").c_str());
    if (with_adjoint && h->sv_type != 1)
        return fail(h, JQ_EUNSUPPORTED, (w + "sv_type != 1 (continuation adjoints) has no tangent of the terminal condition; set sv_type 1").c_str());
    if (with_adjoint && !h->rfreq.empty()) return fail(h, JQ_EUNSUPPORTED, (w + "uncoupled controls (Hunc_ops) are not served; coupled controls only").c_str());
    return JQ_OK;
}

// Directions per launch, chunk length, rounds: 1 + dpl streams of `stride` doubles per image within the stream budget (option
// stream_bytes), and -- trec > 0: the doubles of ONE trace record per step and direction -- the two trace records of a chunk within the
// same budget; never longer chunks than the handle's (option chunk_steps), never more than dir_cap directions.
#define JQ_JVP_MIN_CHUNK 16      // directions per launch: as many as leave the stream budget room for chunks of this many steps
#define JQ_JVP_MAX_DIRS 4096     // ... and at most this many workgroups in a launch's grid dimension (run-time-size kernels: directions x parts)
// A drift ensemble (nmember > 1; jq_eval_f_g_grad_drifts_hvp) brings one primal stream per member: the directions are sized first, as for one
// member, then as many members per launch (mpl) as the budget leaves streams for next to them, in mrounds rounds of equal size; trec is the
// record of ONE member.  nmember == 1 is the budget it always was.
// Members with a control mix (per_member; jq_eval_f_g_grad_members_hvp) bring the streams of their own directions along: a member costs
// 1 + dpl streams instead of 1, so (fit + 1) / (1 + dpl) members fit next to each other (in rounds of equal size again) and the chunk
// length follows from mpl (1 + dpl) streams.
struct TlBudget {
    int dpl, cs, rounds, nchunks;
    size_t gstride;      // doubles of one group's stream of a chunk
    int mpl, mrounds;    // primal streams (members) per launch, member rounds
};
static TlBudget tl_budget(const jq_handle* h, size_t stride, int ndir, int dir_cap, size_t trec, int nmember = 1, bool per_member = false)
{
    const size_t budget = stream_budget_bytes(h) / sizeof(double);
    const long long want = 2LL * std::min(JQ_JVP_MIN_CHUNK, h->nsteps) + 1;
    const long long fit = (long long)(budget / (2 * stride * (size_t)want)) - 1;
    TlBudget b;
    b.dpl = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(ndir, dir_cap), fit));
    const long long mfit = std::max<long long>(1, std::min<long long>(nmember, per_member ? (fit + 1) / (1 + b.dpl) : fit + 1 - b.dpl));
    b.mrounds = (int)((nmember + mfit - 1) / mfit);
    b.mpl = (nmember + b.mrounds - 1) / b.mrounds;
    const size_t nstreams = per_member ? (size_t)b.mpl * (1 + b.dpl) : (size_t)(b.mpl + b.dpl);
    const long long tps = (long long)(budget / (nstreams * 2 * stride));
    long long cs = std::min<long long>(std::min(h->chunk_steps, h->nsteps), (tps - 1) / 2);
    if (trec) cs = std::min<long long>(cs, (long long)(budget / ((size_t)2 * b.dpl * b.mpl * trec)));
    b.cs = (int)std::max<long long>(1, cs);
    b.rounds = (ndir + b.dpl - 1) / b.dpl;
    b.nchunks = (h->nsteps + b.cs - 1) / b.cs;
    b.gstride = (size_t)(2 * b.cs + 1) * 2 * stride;
    return b;
}

// The generators of a chunk's 1 + dpl streams: k_ctrl over the coefficient blocks in sp.pcof, k_stream over the operator images
// himg = [H0 | Hsym_q | Hanti_q] with the groups' drift images h0 = [H0 | 0 ...].  dt > 0: the forward time table, dt < 0: the backward one.
// mix (NULL: none, the launches they always were): one Nc x Nc control mix per group for k_ctrl, raw: its unmixed values in pq's layout.
// sampled (jq_eval_f_g_grad_samples_hvp): the blocks in sp.pcof are sample tables [2 Nc x nt] on the time grid (tl_samples), sp.nCoeff
// = 2 Nc nt doubles apart, and k_ctrl_samples_grouped takes the place of k_ctrl -- a table is linear in itself, so the stream of a
// direction table with a zero drift image is its tangent stream; no mix.
struct TlGen {
    SplineArgs sp;
    const double *himg, *h0;
    double *pq, *stream;
    size_t stride, gstride;
    int nvec;
    const double* mix = nullptr;
    double* raw = nullptr;
    bool sampled = false;
};
static SplineArgs tl_spline(const jq_handle* h, const double* d_pcof, int ncoeff, const double* d_rfreq)
{
    SplineArgs sp;
    sp.pcof = d_pcof; sp.cfreq = h->d_cfreq; sp.D1 = ncoeff / (2 * h->Nc * h->Nfreq); sp.Nfreq = h->Nfreq; sp.Ncoupled = h->Nc; sp.nCoeff = ncoeff;
    sp.dtknot = h->T / (sp.D1 - 2);
    sp.rfreq = d_rfreq;
    return sp;
}
// the blocks of sample tables in the place of the coefficient blocks: only pcof and nCoeff (the table stride) are read
static SplineArgs tl_samples(const jq_handle* h, const double* d_tables, int ncoeff)
{
    SplineArgs sp;
    sp.pcof = d_tables; sp.cfreq = h->d_cfreq; sp.D1 = 0; sp.Nfreq = h->Nfreq; sp.Ncoupled = h->Nc; sp.nCoeff = ncoeff;
    sp.dtknot = 0.0;
    sp.rfreq = nullptr;
    return sp;
}
static void tl_generate(const jq_handle* h, const TlGen& g, int n0, int nc, double dt)
{
    const int ntp = 2 * nc + 1;
    if (g.sampled)      // (run_eval's index map: a forward chunk reads the table upwards from 2 n0, a backward one downwards from 2 (nsteps - n0))
        hipLaunchKernelGGL(k_ctrl_samples_grouped, dim3((ntp + 127) / 128, g.nvec), dim3(128), 0, h->stream, g.sp.pcof, (long long)g.sp.nCoeff, 2 * h->nsteps + 1,
                           dt > 0 ? 2 * n0 : 2 * (h->nsteps - n0), dt > 0 ? 1 : -1, ntp, h->Nc, g.pq);
    else
        hipLaunchKernelGGL(k_ctrl, dim3((ntp + 127) / 128, g.nvec), dim3(128), 0, h->stream, g.sp, dt > 0 ? h->d_tf : h->d_tb, n0, ntp, dt, g.pq, g.mix, g.raw);
    hipLaunchKernelGGL(k_stream, dim3((unsigned)((g.stride + 255) / 256), ntp, g.nvec), dim3(256), 0, h->stream, g.himg, g.h0, (long long)g.stride, g.pq, h->Nc,
                       (long long)g.stride, 0.5 * dt, g.stream, (long long)g.gstride);
}

// the coefficient blocks [pcof | dirs[:, j0 + j] ...] of a round on the device (a short last round repeats its last direction: every group has a stream)
// np primal streams (the members of a drift ensemble share ONE control vector): pcof in front np times
// per_member (members with a control mix): the directions once per member, [pcof x np | member 0: direction ... | member 1: ...]
static int tl_upload_round(jq_handle* h, std::vector<double>& blk, double* d_pc, const double* pcof, const double* dirs, int j0, int nd, int dpl, int ncoeff, int np = 1,
                           bool per_member = false)
{
    for (int g = 0; g < np; ++g) std::copy(pcof, pcof + ncoeff, blk.begin() + (size_t)g * ncoeff);
    for (int g = 0; g < (per_member ? np : 1); ++g)
        for (int j = 0; j < dpl; ++j)
            std::copy_n(dirs + (size_t)(j0 + std::min(j, nd - 1)) * ncoeff, ncoeff, blk.begin() + (size_t)(np + (size_t)g * dpl + j) * ncoeff);
    HIPCHK(h, hipMemcpyAsync(d_pc, blk.data(), blk.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return JQ_OK;
}

// HIP events of a call: [0] = start, [1] = end, then a pair around every propagator launch, and the jq_timing they give
struct LaunchTimer {
    jq_handle* h;
    size_t evi = 2;
    std::vector<char> bwd;      // per event pair: a backward launch?
    int start(size_t nlaunches)
    {
        if (int rc = ensure_events(h, 2 + 2 * nlaunches)) return rc;
        HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
        return JQ_OK;
    }
    int begin(bool backward)
    {
        bwd.push_back(backward);
        HIPCHK(h, hipEventRecord(h->ev[evi++], h->stream));
        return JQ_OK;
    }
    int end()
    {
        HIPCHK(h, hipEventRecord(h->ev[evi++], h->stream));
        return JQ_OK;
    }
    int stop()      // the end of the call: everything on the stream is through when it returns
    {
        HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return JQ_OK;
    }
    // a fresh h->timing: times and launch counts (JQ_DEBUG_TIMING: every launch on stderr as "<label> forward / backward"); the caller adds
    // mfma_*, svts, kernel_family / size / band
    int finish(const char* label)
    {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        h->timing = jq_timing{};
        h->timing.ms_total = ms;
        double fwd = 0.0, back = 0.0;
        long long nbwd = 0;
        for (size_t k = 0; k < bwd.size(); ++k) {
            HIPCHK(h, hipEventElapsedTime(&ms, h->ev[2 + 2 * k], h->ev[3 + 2 * k]));
            if (debug_timing()) fprintf(stderr, "jq launch %zu (%s %s): %.3f ms\n", k, label, bwd[k] ? "backward" : "forward", ms);
            (bwd[k] ? back : fwd) += ms;
            nbwd += bwd[k];
        }
        h->timing.ms_forward = fwd, h->timing.ms_backward = back, h->timing.ms_propagate = fwd + back;
        h->timing.ms_generate = h->timing.ms_total - (fwd + back);
        h->timing.n_forward_launches = (long long)bwd.size() - nbwd;
        h->timing.n_backward_launches = nbwd;
        h->timing.ms_shard_min = h->timing.ms_shard_max = h->timing.ms_total;
        return JQ_OK;
    }
};

// ---- the run-time-size kernels (jq_tl_kernels.h, jq_tl_adjoint_kernels.h): any Ntot, dense row-window images (band code 15) ----
// operator images [H0 = drift | Hsym_q | Hanti_q] from the host copies, NT x 4 NT tiles of 64 doubles each
static std::vector<double> tl_dense_images(const jq_handle* h, const double* drift)
{
    const int NT = (h->Ntot + 15) / 16, Nc = h->Nc;
    const size_t stride = (size_t)NT * 4 * NT * 64, nn = (size_t)h->Ntot * h->Ntot;
    std::vector<double> img((size_t)(1 + 2 * Nc) * stride, 0.0);
    tile_image_coop(drift, h->Ntot, NT, 15, img.data());
    for (int q = 0; q < Nc; ++q) {
        tile_image_coop(h->Hsym.data() + q * nn, h->Ntot, NT, 15, img.data() + (size_t)(1 + q) * stride);
        tile_image_coop(h->Hanti.data() + q * nn, h->Ntot, NT, 15, img.data() + (size_t)(1 + Nc + q) * stride);
    }
    return img;
}
// what both drivers upload before their rounds: the images, the groups' drift images [H0 | 0 ...], the weight table padded to 16 NT rows
// (img, wd: the caller's host blocks -- they stay until the stream is through)
static int tl_upload_dense(jq_handle* h, const std::vector<double>& img, const std::vector<double>& wd, size_t stride, int nvec, double* d_img, double* d_h0, double* d_wd)
{
    HIPCHK(h, hipMemcpyAsync(d_img, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(d_h0, 0, (size_t)nvec * stride * sizeof(double), h->stream));
    HIPCHK(h, hipMemcpyAsync(d_h0, img.data(), stride * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_wd, wd.data(), wd.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return JQ_OK;
}
// the PropArgs both sweeps of a round share (the sweeps set h, forced, the schedule and the chunk)
static PropArgs tl_prop_args(const jq_handle* h, const TlGen& g, int dpl, double* d_state, long long sstride, double* d_work, const double* d_wd)
{
    PropArgs a;
    memset(&a, 0, sizeof a);
    a.stream = g.stream; a.stream_gstride = (long long)g.gstride; a.group_units = 1; a.state = d_state; a.state_stride = sstride;
    a.park = d_work; a.tabs = d_wd; a.stride = (long long)g.stride; a.m = h->m; a.nslabs = dpl * h->parts; a.Ntot = h->Ntot; a.N = h->N;
    a.parts = h->parts; a.nsamples = dpl; a.sps = 1; a.tinv = 1.0 / h->T;
    return a;
}
// the forward half of a round: initial state and zero tangent, then per chunk its streams and one k_forward_tl launch under the timer
static int tl_forward_sweep(jq_handle* h, PropArgs& a, const TlGen& g, int cs, LaunchTimer& tm)
{
    const double dt = h->T / h->nsteps;
    hipLaunchKernelGGL(k_init_tl, dim3(a.nslabs), dim3(64), 0, h->stream, a.state, a.state_stride, h->d_uimg, 4 * ((h->Ntot + 15) / 16), a.parts, h->N);
    a.h = dt; a.forced = 1; a.Ncoupled = 0; a.cimg = nullptr;
    pack_forward_schedule(a, JQ_SCHED[1]);
    for (int n0 = 0; n0 < h->nsteps; n0 += cs) {
        const int nc = std::min(cs, h->nsteps - n0);
        tl_generate(h, g, n0, nc, dt);
        a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0);
        if (int rc = tm.begin(false)) return rc;
        hipLaunchKernelGGL(k_forward_tl<>, dim3(a.nslabs), dim3(64 * JQ_HUGE_WAVES), 0, h->stream, a);
        if (int rc = tm.end()) return rc;
    }
    return JQ_OK;
}
// MFMA instructions of `rounds` forward sweeps of nblocks workgroups (state and tangent: three products where the plain sweep has one)
static long long tl_forward_mfma(const jq_handle* h, int rounds, int nblocks)
{
    const int NT = (h->Ntot + 15) / 16;
    return (long long)rounds * nblocks * h->nsteps * 3 * (8 + 2 * h->m) * NT * 4 * NT;
}

// After a backward launch over the steps [n0, n0 + nc) with the controls [q0, q0 + ng): k_trace_reduce / k_gradacc on the primal record
// of the round's first direction (primal: first round only -- every direction recomputes the same primal) into gp[0] and on the tangent
// records behind it into gp[1 + j]; gp = [primal | direction ...][ncoeff].  rows: trace rows per direction; R, Rd: the reduced records.
// mx (members with a control mix): every direction has P members of `rows` trace rows each, reduced apart with the member's mix -- R, Rd
// then hold rows for ALL Nc controls and the assembly covers all of them, the other control groups add theirs in their sweeps (run_eval's
// rule) -- into gradient blocks of their own, gp = [member 0 .. P - 1 | direction 0: member 0 .. P - 1 | direction 1: ...][ncoeff], for
// the caller to add in member order (tl_fold_members).  primal: [C_0 .. C_{P - 1}], dirs: that dpl times.
// sampled (TlGen::sampled; never with mx): gp = [primal | direction ...][2 Nc nt] are gradients with respect to the samples, assembled by
// k_gradsamples_grouped from the same records.
struct TlMix {
    const double *primal, *dirs;
    int P;
};
static void tl_reduce_chunk(const jq_handle* h, const SplineArgs& sp, bool primal, const double* tr, int rows, int dpl, int n0, int nc, int q0, int ng, double* R,
                            double* Rd, double* gp, const TlMix* mx = nullptr, bool sampled = false)
{
    const int ntr = ng * JQ_NTR, P = mx ? mx->P : 1;
    const int ntr_R = mx ? h->Nc * JQ_NTR : ntr, gq0 = mx ? 0 : q0, gng = mx ? h->Nc : ng;
    const double dt = h->T / h->nsteps;
    const unsigned rblocks = (unsigned)(((long long)nc * ntr_R + 255) / 256), gblocks = (unsigned)(gng * 2 * h->Nfreq * sp.D1);
    const double* trd = tr + (size_t)dpl * P * rows * nc * ntr;      // the tangents' record (k_backward_tl, k_backward_lane_tl)
    hipStream_t s = h->stream;
    if (sampled) {
        const int nt = 2 * h->nsteps + 1, J0 = 2 * (h->nsteps - n0);
        const unsigned sblocks = (unsigned)(((long long)(2 * nc + 1) * ng * 2 + 255) / 256);
        if (primal) {
            hipLaunchKernelGGL(k_trace_reduce, dim3(rblocks, 1), dim3(256), 0, s, tr, rows, nc, ntr, R, (const double*)nullptr, h->Nc, q0);
            hipLaunchKernelGGL(k_gradsamples_grouped, dim3(sblocks, 1), dim3(256), 0, s, (const double*)R, nc, -dt, gp, (long long)sp.nCoeff, nt, J0, h->Nc, q0, ng);
        }
        hipLaunchKernelGGL(k_trace_reduce, dim3(rblocks, dpl), dim3(256), 0, s, trd, rows, nc, ntr, Rd, (const double*)nullptr, h->Nc, q0);
        hipLaunchKernelGGL(k_gradsamples_grouped, dim3(sblocks, dpl), dim3(256), 0, s, (const double*)Rd, nc, -dt, gp + sp.nCoeff, (long long)sp.nCoeff, nt, J0, h->Nc, q0, ng);
        return;
    }
    if (primal) {
        hipLaunchKernelGGL(k_trace_reduce, dim3(rblocks, P), dim3(256), 0, s, tr, rows, nc, ntr, R, mx ? mx->primal : (const double*)nullptr, h->Nc, q0);
        hipLaunchKernelGGL(k_gradacc, dim3(gblocks, P), dim3(JQ_GRADACC_THREADS), 0, s, sp, (const double*)R, h->d_tb, n0, nc, -dt, gp, gq0, gng, (long long)sp.nCoeff);
    }
    hipLaunchKernelGGL(k_trace_reduce, dim3(rblocks, dpl * P), dim3(256), 0, s, trd, rows, nc, ntr, Rd, mx ? mx->dirs : (const double*)nullptr, h->Nc, q0);
    hipLaunchKernelGGL(k_gradacc, dim3(gblocks, dpl * P), dim3(JQ_GRADACC_THREADS), 0, s, sp, (const double*)Rd, h->d_tb, n0, nc, -dt, gp + (size_t)P * sp.nCoeff, gq0,
                       gng, (long long)sp.nCoeff);
}
// The per-member gradient blocks of a launch, blk = [pass][member 0 .. P - 1 | direction 0: member 0 .. P - 1 | ...][ncoeff] on the host, added
// onto fold = [pass][primal | direction ...][ncoeff] (tl_copy_out's layout): the first `nm` members of the launch, in member order.
static void tl_fold_members(const std::vector<double>& blk, std::vector<double>& fold, int npass, int P, int nm, int dpl, int ncoeff)
{
    const size_t pb = (size_t)P * (1 + dpl) * ncoeff, pf = (size_t)(1 + dpl) * ncoeff;
    for (int pass = 0; pass < npass; ++pass)
        for (int j = -1; j < dpl; ++j) {
            double* f = fold.data() + pass * pf + (size_t)(1 + j) * ncoeff;
            for (int g = 0; g < nm; ++g) {
                const double* b = blk.data() + pass * pb + ((size_t)(j < 0 ? g : P + j * P + g)) * ncoeff;
                for (int k = 0; k < ncoeff; ++k) f[k] += b[k];
            }
        }
}
// A round's gradient blocks gbuf = [pass][primal | direction ...][ncoeff] on the host -> the caller's arrays: g0 / g1 the gradient of the
// forced / of the unforced pass (first: the first round only), v0 / v1 the products of the directions [j0, j0 + nd).  Without an
// unforced pass (two_pass == false) g1 and v1 are what g0 and v0 are; either may be NULL.
static void tl_copy_out(const std::vector<double>& gbuf, int nvec, int ncoeff, bool two_pass, bool first, int j0, int nd, double* g0, double* g1, double* v0, double* v1)
{
    const double *b0 = gbuf.data(), *b1 = b0 + (size_t)(two_pass ? nvec : 0) * ncoeff;
    if (first) {
        std::copy_n(b0, ncoeff, g0);
        if (g1) std::copy_n(b1, ncoeff, g1);
    }
    for (int j = 0; j < nd; ++j) {
        std::copy_n(b0 + (size_t)(1 + j) * ncoeff, ncoeff, v0 + (size_t)(j0 + j) * ncoeff);
        if (v1) std::copy_n(b1 + (size_t)(1 + j) * ncoeff, ncoeff, v1 + (size_t)(j0 + j) * ncoeff);
    }
}
