// jq_host_ens_hvp.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// jq_eval_f_g_grad_hvp -- jq_eval_f_g_grad and the derivative of its two gradients along directions of coefficient space: Hessian-vector
// products of a risk-neutral ensemble, sum_i w_i d/d eps grad_i(alpha + eps d) over the quadrature nodes i.
//
// Lane route (Ntot <= 6 padded to NP = 2, 4, 6; at most JQ_MAXNC controls): the tangent-linear lane kernels of jq_lane_tl_kernels.h, all
// N nquad columns x `dpl` directions in ONE launch per chunk -- the nodes fill the lanes, the directions the grid.  The chunk is the
// grouped chunk of jq_host_tl.h in the lane image layout, budgeted, generated, reduced and timed by its helpers; objFuncType != 1
// repeats the backward sweep unforced from the saved terminal state for the infidelity part.  The call reads the handle's lane images
// and time tables, allocates everything it writes and frees it when it returns.
//
// Row-lane route (Ntot 9 .. 16 padded to NPJ = 12, 16; at most JQ_MAXNC controls): the same driver on the tangent-linear row-lane
// kernels of jq_rowlane_tl_kernels.h -- four columns per wave, ceil(N nquad / 4) waves x `dpl` directions in one launch per chunk, the
// handle's row-lane images.  What differs between the two is the layout record (EnsHvpLayout) the driver reads.
//
// Quad route (Ntot > 16 with the 4 x 4 x n structure of the handle's own plan, NT = 2 .. 6 blocks of 16 rows, quad-layout kernels enabled; at
// most JQ_MAXNC controls): the same driver on the tangent-linear quad-layout kernels of jq_quad_tl_kernels.h -- four columns per wave, up to
// JQ_QUAD_TL_WAVES waves of one direction per workgroup sharing its operator rings, the handle's T4 images and slab images.
//
// Sequential route (everything else jq_traceobjgrad_hvp serves: Ntot 7, 8, Ntot > 16 without that structure or with NT = 7, 8, embedded
// structures, options lane=0 / quad=0, more than JQ_MAXNC controls): the nodes one after the other through hvp_run with the drift
// Hconst + eps_i diag(shift) -- correct and no faster.
//
// jq_eval_f_g_grad_drifts_hvp -- the same sums over the members of a drift ensemble, member i being the handle's problem with
// Hconst = drifts[:, :, i]: the same driver and routes with another notion of a sample.  A sample of the eps ensemble is a node: its N
// columns follow the node before it, every wave reads ONE primal stream and the node shift tells the columns apart.  A sample of a drift
// ensemble is a member: it brings a primal stream of its own (its drift image in the route's layout in front of k_stream), its columns
// start at fresh waves -- a wave propagates with one member's operators; quad route: a workgroup shares its operator rings, so a member
// is padded to whole workgroups -- and P members share a launch ([member 0 .. P - 1 | direction ...] streams, PropArgs::nprimal).
// Members beyond the stream budget run in further member rounds that accumulate into the same gradient blocks, in member order.  A
// member outside the structure the handle was planned for (hconst_fits_plan) sends the whole call down the sequential route: the call
// never re-plans the handle and never touches its operator images.
//
// jq_eval_f_g_grad_members_hvp -- members that differ in a real Nc x Nc mix of the controls as well (operator l is driven by
// sum_k C_i[l, k] (p_k, q_k)), with or without a drift of their own.  Without a mix it IS the drift ensemble above.  With one the tangent
// stream of a direction is no longer shared: member i differentiates along sum_l (C_i d_j)_l H_l, so a member brings 1 + dpl streams
// ([member 0 .. P - 1 | member 0: direction ... | member 1: ...], PropArgs::tl_dirs_per_member), k_ctrl mixes every stream with the mix of
// its member, and the traces of a member are reduced apart with its mix (k_trace_reduce) into gradient blocks of their own, which the
// host adds in member order.  A mix never changes the route: operators and structure are the handle's.
//
// jq_eval_f_g_grad_samples_hvp (jq_host_samples.h) -- the eps ensemble with the controls and the directions given as sample tables on the
// time grid (EnsHvpArgs::sampled): the same driver, routes, budget and rounds with blocks of 2 Nc nt doubles where the coefficient blocks
// are; tl_generate and tl_reduce_chunk launch the sample kernels instead of k_ctrl and k_gradacc.  A table never changes the route.
static double ens_hvp_shift(const double* shift, int i) { return shift ? shift[i] : (i >= 1 ? 0.01 * pow(10.0, (double)(i - 1)) : 0.0); }

struct EnsHvpArgs {
    const char* who;            // the entry point that runs
    const double *pcof, *dirs, *nodes, *weights, *shift;
    const double* drifts;       // NULL: nquad eps-nodes (nodes, shift); else HOST [Ntot x Ntot x nquad] member drifts (nodes, shift unused)
    int ncoeff, ndir, nquad;    // nquad: samples -- nodes or members
    double *out2, *infid_grad, *leak_grad, *hv_infid, *hv_leak;
    const double* mix = nullptr;      // HOST [Nc x Nc x nquad] control mixes of the members (NULL: none); with drifts == NULL the members have the handle's drift
    bool member_call = false;         // jq_eval_f_g_grad_members_hvp runs: the call is recorded as "member_hvp" of jq_plan_info, not as "drift_hvp"
    // jq_eval_f_g_grad_samples_hvp runs (jq_host_samples.h): pcof and dirs are sample tables [2 Nc x nt], ncoeff = 2 Nc nt, the gradients and products
    // are those with respect to the samples; nodes only (no drifts, no mix).  The call is recorded as "sampled_hvp" of jq_plan_info.
    bool sampled = false;
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

// What the driver needs to know about a kernel family: the handle's images in its layout, the geometry of a wave and of the state file.
struct EnsHvpLayout {
    int route;                  // ens_hvp_route: 1 lane, 3 row-lane, 4 quad
    int family, size, band;     // jq_last_timing: kernel_family, kernel_size (NP / NPJ / NT), kernel_band
    const char* label;          // JQ_DEBUG_TIMING
    size_t stride;              // doubles per operator image
    const double *himg, *cimg, *uinit, *vtr, *vti;
    int cpw;                    // columns per wave; colinfo = [eps per column | weight per column] at cpw nwaves
    int state_rows;             // rows of 64 doubles per wave in one direction's state file
    bool slabs_are_waves;       // PropArgs::nslabs: waves (row-lane kernels) or padded columns (lane kernels)
    int tab_off;                // tables [wd(tab_off) | ws(tab_off)]
    size_t lds_fwd, lds_bwd;    // dynamic LDS bytes of the sweep kernels
    int wpg;                    // most waves of one direction per workgroup of the sweep kernels (they share its LDS)
    bool modes;                 // the backward kernel multiplies a trace image in the T4 mode of its control (PropArgs::bw_trace)
};
static EnsHvpLayout ens_hvp_layout_lane(const jq_handle* h)
{
    return {1, KF_LANE, h->lane_np, 0, "tangent-linear lane", (size_t)h->lane_stride, h->d_himg_l, h->d_cimg_l, h->d_uinit_l, h->d_vtr_l, h->d_vti_l,
            64, JQ_LANE_TL_ROWS(h->lane_np), false, h->lane_np, 0, 0, 1, false};
}
static EnsHvpLayout ens_hvp_layout_rowlane(const jq_handle* h)
{
    const size_t rings = JQ_ROWLANE_TL_RINGS(h->rl_npj);
    return {3, KF_ROWLANE, h->rl_npj, 0, "tangent-linear row-lane", (size_t)h->rl_stride, h->d_himg_r, h->d_cimg_r, h->d_uinit_r, h->d_vtr_r, h->d_vti_r,
            4, JQ_ROWLANE_TL_ROWS, true, 16, rings, rings + (size_t)2 * h->Nc * h->rl_stride * sizeof(double), 1, false};
}
static EnsHvpLayout ens_hvp_layout_quad(const jq_handle* h)
{
    const size_t rings = JQ_QUAD_TL_RINGS(h->mat_elems);
    return {4, KF_QUAD, h->NT, JQ_BW_T4Q, "tangent-linear quad", (size_t)h->mat_elems, h->d_himg, h->d_cimg, h->d_uimg, h->d_vtr, h->d_vti,
            4, JQ_QUAD_TL_ROWS(h->NT), true, 16 * h->NT, rings, rings + (size_t)2 * h->Nc * h->mat_elems * sizeof(double), JQ_QUAD_TL_WAVES, true};
}

static int ens_hvp_lane(jq_handle* h, const EnsHvpArgs& x, const EnsHvpLayout& lay, prop_kernel_t kfwd, prop_kernel_t kbwd, const KernelSel& sel)
{
    const char* who = x.who;
    HIPCHK(h, hipSetDevice(h->device));
    const int Nc = h->Nc, ncoeff = x.ncoeff, ndir = x.ndir, nquad = x.nquad, ntr = Nc * JQ_NTR;
    const bool members = x.drifts != nullptr || x.mix != nullptr, mixed = x.mix != nullptr;
    const size_t stride = lay.stride, nn = (size_t)h->Ntot * h->Ntot, ncnc = (size_t)Nc * Nc;
    // What a sample is.  wps: the waves that read one primal stream -- all the waves of the packed node columns, or a member's ceil(N / cpw)
    // padded to whole workgroups of the sweep kernels; gcols: the columns in front of such a group of wps cpw column slots.
    const long long gcols = members ? h->N : (long long)nquad * h->N;
    int wps = (int)((gcols + lay.cpw - 1) / lay.cpw);
    if (members) wps = (wps + std::min(lay.wpg, wps) - 1) / std::min(lay.wpg, wps) * std::min(lay.wpg, wps);
    const long long cpg = (long long)wps * lay.cpw;
    const double dt = h->T / h->nsteps;
    const bool two_pass = h->objFuncType != 1;
    const int npass = two_pass ? 2 : 1;
    const TlBudget b = tl_budget(h, stride, ndir, JQ_JVP_MAX_DIRS, (size_t)wps * ntr, members ? nquad : 1, mixed);      // (the directions are a grid dimension of their own)
    // P primal streams (members) and spl samples per launch, mrounds launches per direction round; ngb gradient blocks [primal | direction ...]
    // (mixed: every member its own direction streams and its own gradient blocks, ndb of them, folded into the ngb on the host)
    const int dpl = b.dpl, cs = b.cs, rounds = b.rounds, P = b.mpl, mrounds = b.mrounds, nvec = mixed ? P * (1 + dpl) : P + dpl, ngb = 1 + dpl;
    const int ndb = mixed ? P * ngb : ngb, PR = mixed ? P : 1;
    const int spl = members ? P : nquad, nwaves = P * wps;
    const long long ncols = (long long)nwaves * lay.cpw;
    const size_t sstride = (size_t)lay.state_rows * (size_t)nwaves * 64;      // doubles of one direction's state file

    // tables [wd | ws]; per member round the column info [eps | weight] per column slot (run_eval's for the layout) and the drift images
    // of its members in the route's layout (the builders and the bits of upload_operators' image 0; a short last round repeats its last
    // member with weight 0: every group has a stream)
    // mixed: per member round k_ctrl's mixes [C_0 .. C_{P - 1} | C_0 x dpl | C_1 x dpl | ...] and behind them the reducer's for the tangent
    // records [C_0 .. C_{P - 1}] x dpl (its primal ones are the first P of k_ctrl's), nmix matrices in all
    const size_t nmix = (size_t)nvec + (size_t)dpl * P;
    std::vector<double> tabs((size_t)2 * lay.tab_off, 0.0), colinfo((size_t)mrounds * 2 * ncols, 0.0), mimg(x.drifts ? (size_t)mrounds * P * stride : 0, 0.0);
    std::vector<double> mixtab(mixed ? (size_t)mrounds * nmix * ncnc : 0);
    bool use_shift = false;
    for (int i = 0; i < h->Ntot; ++i) tabs[i] = h->wd[i], tabs[lay.tab_off + i] = ens_hvp_shift(x.shift, i);
    for (int mr = 0; mr < mrounds; ++mr)
        for (int sl = 0; sl < spl; ++sl) {
            const int smp = mr * spl + sl;
            if (mixed) {
                const double* C = x.mix + ncnc * std::min(smp, nquad - 1);
                double* t = mixtab.data() + (size_t)mr * nmix * ncnc;
                std::copy_n(C, ncnc, t + sl * ncnc);
                for (int j = 0; j < dpl; ++j) {
                    std::copy_n(C, ncnc, t + ((size_t)P + (size_t)sl * dpl + j) * ncnc);
                    std::copy_n(C, ncnc, t + ((size_t)nvec + (size_t)j * P + sl) * ncnc);
                }
            }
            if (x.drifts) {
                const double* M = x.drifts + nn * std::min(smp, nquad - 1);
                double* img = mimg.data() + ((size_t)mr * P + sl) * stride;
                if (lay.route == 1) plain_image(M, h->Ntot, lay.size, img);
                else if (lay.route == 3) rowlane_image(M, h->Ntot, lay.size, img);
                else tile_image(M, h->Ntot, lay.size, JQ_BW_T4, img);
            }
            if (smp >= nquad) continue;
            for (int ic = 0; ic < h->N; ++ic) {
                const long long c = (size_t)mr * 2 * ncols + (members ? sl * cpg + ic : (long long)sl * h->N + ic);
                colinfo[c] = members ? 0.0 : x.nodes[smp];
                colinfo[ncols + c] = x.weights[smp];
                if (!members && x.nodes[smp] != 0.0) use_shift = true;
            }
        }
    DevBuf d_h0, d_pc, d_pq, d_stream, d_state, d_save, d_tabs, d_col, d_res, d_tr, d_R, d_g, d_mix, d_raw;
    int rc;
    if ((rc = d_h0.alloc(h, who, (size_t)nvec * stride)) || (rc = d_pc.alloc(h, who, (size_t)nvec * ncoeff)) ||
        (rc = d_pq.alloc(h, who, (size_t)nvec * (2 * cs + 1) * 2 * Nc)) || (rc = d_stream.alloc(h, who, (size_t)nvec * b.gstride)) ||
        (rc = d_state.alloc(h, who, (size_t)dpl * sstride)) || (rc = d_save.alloc(h, who, two_pass ? (size_t)dpl * sstride : 1)) ||
        (rc = d_tabs.alloc(h, who, tabs.size())) || (rc = d_col.alloc(h, who, (size_t)2 * ncols)) || (rc = d_res.alloc(h, who, (size_t)dpl * spl * 4)) ||
        (rc = d_tr.alloc(h, who, (size_t)2 * dpl * nwaves * cs * ntr)) || (rc = d_R.alloc(h, who, (size_t)ndb * cs * ntr)) ||
        (rc = d_g.alloc(h, who, (size_t)2 * ndb * ncoeff)) ||
        (mixed && ((rc = d_mix.alloc(h, who, nmix * ncnc)) || (rc = d_raw.alloc(h, who, (size_t)nvec * (2 * cs + 1) * 2 * Nc)))))
        return rc;
    // d_g: [pass][primal | direction ...][ncoeff]; mixed: [pass][member 0 .. P - 1 | direction 0: member 0 .. P - 1 | ...][ncoeff] (tl_reduce_chunk)
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemsetAsync(d_h0.p, 0, (size_t)nvec * stride * sizeof(double), s));
    // (the handle's own image 0: the one primal stream of the eps ensemble, or once per member of an ensemble of mixes alone)
    for (int g = 0; g < (members ? P : 1) && !x.drifts; ++g) HIPCHK(h, hipMemcpyAsync(d_h0.p + (size_t)g * stride, lay.himg, stride * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_tabs.p, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice, s));
    // the samples of member round mr: column info, drift images [H_0 .. H_{P - 1} | 0 ...]
    const auto upload_samples = [&](int mr) -> int {
        HIPCHK(h, hipMemcpyAsync(d_col.p, colinfo.data() + (size_t)mr * 2 * ncols, (size_t)2 * ncols * sizeof(double), hipMemcpyHostToDevice, s));
        if (x.drifts) HIPCHK(h, hipMemcpyAsync(d_h0.p, mimg.data() + (size_t)mr * P * stride, (size_t)P * stride * sizeof(double), hipMemcpyHostToDevice, s));
        if (mixed) HIPCHK(h, hipMemcpyAsync(d_mix.p, mixtab.data() + (size_t)mr * nmix * ncnc, nmix * ncnc * sizeof(double), hipMemcpyHostToDevice, s));
        return JQ_OK;
    };
    if (mrounds == 1 && (rc = upload_samples(0))) return rc;

    const TlGen gen = {x.sampled ? tl_samples(h, d_pc.p, ncoeff) : tl_spline(h, d_pc.p, ncoeff, nullptr), lay.himg, d_h0.p, d_pq.p, d_stream.p, stride, b.gstride, nvec, d_mix.p, d_raw.p, x.sampled};
    const TlMix mx = {d_mix.p, d_mix.p + (size_t)nvec * ncnc, P};
    PropArgs a;
    memset(&a, 0, sizeof a);
    a.stream = d_stream.p; a.stream_gstride = (long long)b.gstride; a.group_units = wps; a.nprimal = P; a.tl_dirs_per_member = mixed ? 1 : 0; a.state = d_state.p; a.state_stride = (long long)sstride;
    a.colinfo = d_col.p; a.tabs = d_tabs.p; a.traces = d_tr.p; a.cimg = lay.cimg; a.stride = (long long)stride; a.m = h->m; a.nslabs = lay.slabs_are_waves ? nwaves : (int)ncols;
    a.Ncoupled = Nc; a.Ntot = h->Ntot; a.N = h->N; a.parts = 1; a.nsamples = spl; a.sps = 1; a.tinv = 1.0 / h->T; a.use_shift = use_shift ? 1 : 0;
    for (int q = 0; q < JQ_MAXNC && lay.modes; ++q) a.bw_trace[q] = q < Nc ? h->bw_trace[q] : 0;
    if (lay.lds_fwd) HIPCHK(h, hipFuncSetAttribute((const void*)kfwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay.lds_fwd));
    if (lay.lds_bwd) HIPCHK(h, hipFuncSetAttribute((const void*)kbwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay.lds_bwd));

    LaunchTimer tm{h};
    if ((rc = tm.start((size_t)b.nchunks * rounds * mrounds * (1 + npass)))) return rc;
    std::vector<double> res((size_t)nquad * 4), blk((size_t)nvec * ncoeff), gbuf((size_t)2 * ndb * ncoeff), fold(mixed ? (size_t)2 * ngb * ncoeff : 0);
    std::vector<double> g0(ncoeff), g1(two_pass ? ncoeff : 0), v0((size_t)ncoeff * ndir), v1(two_pass ? (size_t)ncoeff * ndir : 0);
    const dim3 grid((unsigned)nwaves, (unsigned)dpl);
    // the sweep kernels: wpg consecutive waves of a direction per workgroup (1 on the lane and row-lane routes: the launch it always was)
    const int wpg = std::min(lay.wpg, wps);
    const dim3 sgrid((unsigned)((nwaves + wpg - 1) / wpg), (unsigned)dpl), sblock((unsigned)(64 * wpg));
    // The two launches that bracket a forward sweep, the one place where the driver tells the routes apart.  init: the state files <- (Uinit, 0 ...);
    // else fidelity, leak, lambda(T) and its tangent per (node, direction).  The leak partials are in the last row of a file; lay.size is NP / NT.
    const auto endpoint = [&](bool init) {
        // (a drift ensemble's members start at fresh groups of cpg column slots: the layout's map behind MemberMap)
        const auto terminal = [&](auto map, int nrows) {
            if (members)
                terminal_cols<EP_TL>(s, MemberMap<decltype(map)>{map, nrows, h->N, cpg}, dpl, d_state.p, sstride, lay.vtr, lay.vti, nullptr, nullptr, 1, h->N, spl,
                                     0.5 * dt * (1.0 / h->T), d_res.p);
            else terminal_cols<EP_TL>(s, map, dpl, d_state.p, sstride, lay.vtr, lay.vti, nullptr, nullptr, 1, h->N, spl, 0.5 * dt * (1.0 / h->T), d_res.p);
        };
        const long long nw = nwaves, ss = (long long)sstride;
        const int last = lay.state_rows - 1;
        switch (lay.route) {
        case 1:
            if (init) hipLaunchKernelGGL(k_init_lane, grid, dim3(64), 0, s, d_state.p, ncols, lay.size, lay.state_rows, ss, lay.uinit, h->N, gcols, cpg);
            else terminal(LaneMap{lay.size, ncols, last}, lay.size);
            break;
        case 3:      // (k_init_rowlane's packing: every gcols columns start at a fresh group of wps waves)
            if (init)
                hipLaunchKernelGGL(k_init_rowlane, grid, dim3(64), 0, s, d_state.p, nw, lay.state_rows, ss, lay.uinit, h->N, members ? spl * gcols : gcols,
                                   members ? (int)gcols : lay.cpw, members ? wps : 1);
            else terminal(RowlaneMap{nw, lay.cpw, 1, last}, RowlaneMap::nrows);
            break;
        default:
            if (init) hipLaunchKernelGGL(k_init_quad_tl, grid, dim3(64), 0, s, d_state.p, nw, ss, lay.uinit, lay.size, h->N, gcols, cpg);
            else terminal(QuadMap{h->Ntot, lay.size, nw, last, (size_t)lay.size * nwaves * 64}, h->Ntot);
        }
    };
    // rounds of dpl directions; within one, mrounds launches of P members each accumulate into the round's gradient blocks, in member order
    // (mixed: every launch has fresh per-member blocks, which the host adds to the round's in member order)
    for (int it = 0; it < rounds * mrounds; ++it) {
        const int r = it / mrounds, mr = it % mrounds, j0 = r * dpl, nd = std::min(dpl, ndir - j0);
        if (mr == 0) {
            if ((rc = tl_upload_round(h, blk, d_pc.p, x.pcof, x.dirs, j0, nd, dpl, ncoeff, P, mixed))) return rc;
            std::fill(fold.begin(), fold.end(), 0.0);
        }
        if (mr == 0 || mixed) HIPCHK(h, hipMemsetAsync(d_g.p, 0, (size_t)2 * ndb * ncoeff * sizeof(double), s));
        if (mrounds > 1 && (rc = upload_samples(mr))) return rc;
        // ---- forward sweep of (state, tangent) ----
        endpoint(true);
        a.h = dt; a.forced = 1;
        for (int n0 = 0; n0 < h->nsteps; n0 += cs) {
            const int nc = std::min(cs, h->nsteps - n0);
            tl_generate(h, gen, n0, nc, dt);
            a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0);
            if ((rc = tm.begin(false))) return rc;
            hipLaunchKernelGGL(kfwd, sgrid, sblock, lay.lds_fwd, s, a);
            if ((rc = tm.end())) return rc;
        }
        endpoint(false);
        HIPCHK(h, hipGetLastError());
        if (r == 0)      // (the records of this launch's samples, from the first direction's file)
            HIPCHK(h, hipMemcpyAsync(res.data() + (size_t)mr * spl * 4, d_res.p, (size_t)std::min(spl, nquad - mr * spl) * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
        // ---- backward sweeps: forced, then (objFuncType != 1) unforced from the saved terminal state ----
        if (two_pass) HIPCHK(h, hipMemcpyAsync(d_save.p, d_state.p, (size_t)dpl * sstride * sizeof(double), hipMemcpyDeviceToDevice, s));
        for (int pass = 0; pass < npass; ++pass) {
            if (pass > 0) HIPCHK(h, hipMemcpyAsync(d_state.p, d_save.p, (size_t)dpl * sstride * sizeof(double), hipMemcpyDeviceToDevice, s));
            a.h = -dt; a.forced = (pass == 0);
            for (int n0 = 0; n0 < h->nsteps; n0 += cs) {
                const int nc = std::min(cs, h->nsteps - n0);
                tl_generate(h, gen, n0, nc, -dt);
                a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0);
                if ((rc = tm.begin(true))) return rc;
                hipLaunchKernelGGL(kbwd, sgrid, sblock, lay.lds_bwd, s, a);
                if ((rc = tm.end())) return rc;
                tl_reduce_chunk(h, gen.sp, r == 0, d_tr.p, mixed ? wps : nwaves, dpl, n0, nc, 0, Nc, d_R.p, d_R.p + (size_t)PR * cs * ntr, d_g.p + (size_t)pass * ndb * ncoeff,
                                mixed ? &mx : nullptr, x.sampled);
            }
        }
        HIPCHK(h, hipGetLastError());
        if (mr < mrounds - 1 && !mixed) continue;
        HIPCHK(h, hipMemcpyAsync(gbuf.data(), d_g.p, gbuf.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));      // (the host blocks are reused by the next round)
        if (mixed) tl_fold_members(gbuf, fold, npass, P, std::min(P, nquad - mr * P), dpl, ncoeff);
        if (mr < mrounds - 1) continue;
        tl_copy_out(mixed ? fold : gbuf, ngb, ncoeff, two_pass, r == 0, j0, nd, g0.data(), two_pass ? g1.data() : nullptr, v0.data(), two_pass ? v1.data() : nullptr);
    }
    if ((rc = tm.stop())) return rc;
    double inf = 0.0, leak = 0.0;
    for (int i = 0; i < nquad; ++i) {      // (jq_eval_f_g_grad's sums)
        inf += res[(size_t)i * 4 + 0] * x.weights[i];
        leak += res[(size_t)i * 4 + 1] * x.weights[i];
    }
    x.out2[0] = inf, x.out2[1] = leak;
    ens_hvp_outputs(h, x, g0.data(), g1.data(), v0.data(), v1.data());
    if (x.sampled) h->sampled_hvp = {lay.route, dpl, cs, rounds, 2 * h->nsteps + 1, nquad};
    else if (x.member_call)
        h->member_hvp = {lay.route, P, dpl, cs, rounds * mrounds, x.drifts != nullptr, mixed};
    else if (members) h->drift_hvp_route = lay.route, h->drift_hvp_members = P, h->drift_hvp_per_launch = dpl, h->drift_hvp_chunk = cs, h->drift_hvp_rounds = rounds * mrounds;
    else h->ens_hvp_route = lay.route, h->ens_hvp_per_launch = dpl, h->ens_hvp_chunk = cs, h->ens_hvp_rounds = rounds;

    if ((rc = tm.finish(lay.label))) return rc;
    h->timing.svts = (long long)ndir * nquad * h->N * h->nsteps;
    h->timing.kernel_family = lay.family;
    h->timing.kernel_size = lay.size;
    h->timing.kernel_band = lay.band;
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
    // (sampled: pcof and dirs are sample tables, hvp_run generates and assembles without a basis; a node still only shifts the drift)
    int rc = JQ_OK, dpl = 0, cs = 0, rounds = 0;
    for (int i = 0; i < x.nquad && rc == JQ_OK; ++i) {
        if (x.drifts) drift.assign(x.drifts + (size_t)i * Ntot * Ntot, x.drifts + (size_t)(i + 1) * Ntot * Ntot);      // member i
        else {
            drift = h->Hconst;      // (a member of an ensemble of mixes alone: the handle's drift)
            for (int j = 0; j < Ntot && !x.mix; ++j) drift[(size_t)j * Ntot + j] += x.nodes[i] * ens_hvp_shift(x.shift, j);      // src/ipopt_interface.jl:41-44
        }
        rc = hvp_run(h, drift.data(), x.pcof, ncoeff, x.dirs, ndir, out4, gi.data(), vi.data(), vin.data(), gin.data(), x.who,
                     x.mix ? x.mix + (size_t)i * h->Nc * h->Nc : nullptr, x.sampled);
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
    if (x.sampled) h->sampled_hvp = {2, dpl, cs, rounds, 2 * h->nsteps + 1, x.nquad};
    else if (x.member_call) h->member_hvp = {2, 1, dpl, cs, rounds, x.drifts != nullptr, x.mix != nullptr};
    else if (x.drifts) h->drift_hvp_route = 2, h->drift_hvp_members = 1, h->drift_hvp_per_launch = dpl, h->drift_hvp_chunk = cs, h->drift_hvp_rounds = rounds;
    else h->ens_hvp_route = 2, h->ens_hvp_per_launch = dpl, h->ens_hvp_chunk = cs, h->ens_hvp_rounds = rounds;
    return JQ_OK;
}

// The route of a call whose arguments have passed: lane, row-lane, quad, else sequential.
static int ens_hvp_dispatch(jq_handle* h, const EnsHvpArgs& x)
{
    // a drift ensemble: every member inside the structure the handle's kernels and images were chosen for, or the members one after the
    // other on the run-time-size kernels (which take any drift) -- never a re-plan
    if (x.drifts)
        for (int i = 0; i < x.nquad; ++i)
            if (!hconst_fits_plan(h, x.drifts + (size_t)i * h->Ntot * h->Ntot)) return ens_hvp_sequential(h, x);
    // lane route: the tangent-linear lane kernels exist for the handle's NP and one pass takes its controls; independent of the column
    // bounds of the lane GRADIENT kernels (options lane_min / lane_max): one node is served here too
    if (h->lane_np > 0 && h->Nc <= JQ_MAXNC) {
        KernelSel sel = sel_start();
        const int np = h->lane_np;
        const prop_kernel_t kfwd = pick(sel.fwd, np, -1, "k_forward_lane_tl", {np}), kbwd = pick(sel.bwd, np, -1, "k_backward_lane_tl", {np});
        if (kfwd && kbwd) return ens_hvp_lane(h, x, ens_hvp_layout_lane(h), kfwd, kbwd, sel);
    }
    // row-lane route: Ntot 9 .. 16 (rl_npj is 0 under option lane=0 and on embedded twins; NPJ <= 8 has no tangent kernels: Ntot <= 6 went
    // the lane route above, Ntot 7 and 8 stay sequential)
    if (h->rl_npj >= 12 && h->Nc <= JQ_MAXNC) {
        KernelSel sel = sel_start();
        const int np = h->rl_npj;
        const prop_kernel_t kfwd = pick(sel.fwd, np, -1, "k_forward_rowlane_tl", {np}), kbwd = pick(sel.bwd, np, -1, "k_backward_rowlane_tl", {np});
        if (kfwd && kbwd) return ens_hvp_lane(h, x, ens_hvp_layout_rowlane(h), kfwd, kbwd, sel);
    }
    // quad route: Ntot > 16 with the 4 x 4 x n structure of the handle's own plan (never an embedded twin) and its quad-layout kernels enabled
    // (option quad=0 switches the route off); NT = 7, 8 have no tangent kernels (their backward kernels need scratch) and stay sequential
    if (h->BW == JQ_BW_T4 && h->quad_max_slabs > 0 && h->NT >= 2 && h->Nc <= JQ_MAXNC && h->mat_elems == (long long)JQ_T4_ELEMS(h->NT)) {
        KernelSel sel = sel_start();
        const int nt = h->NT;
        const prop_kernel_t kfwd = pick(sel.fwd, nt, JQ_BW_T4Q, "k_forward_quad_tl", {nt}), kbwd = pick(sel.bwd, nt, JQ_BW_T4Q, "k_backward_quad_tl", {nt});
        if (kfwd && kbwd) return ens_hvp_lane(h, x, ens_hvp_layout_quad(h), kfwd, kbwd, sel);
    }
    return ens_hvp_sequential(h, x);
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
        if (int rc = tl_refuse(h, "jq_eval_f_g_grad_hvp", true)) return rc;
        if (int rc = check_ncoeff(h, ncoeff)) return rc;
        EvalGate gate(h);
        return ens_hvp_dispatch(h, {"jq_eval_f_g_grad_hvp", pcof, dirs, nodes, weights, shift, nullptr, ncoeff, ndir, nquad, out2, infid_grad, leak_grad, hv_infid, hv_leak});
    });
}

extern "C" int jq_eval_f_g_grad_drifts_hvp(jq_handle* h, const double* pcof, int32_t ncoeff, const double* dirs, int32_t ndir, const double* drifts,
                                           const double* weights, int32_t ndrift, double* out2, double* infid_grad, double* leak_grad, double* hv_infid,
                                           double* hv_leak)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_eval_f_g_grad_drifts_hvp", [&]() -> int {
        if (!pcof || !dirs || !drifts || !weights || !out2 || !infid_grad || !leak_grad || !hv_infid || !hv_leak)
            return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_drifts_hvp: NULL pointer");
        if (ndir < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_drifts_hvp: ndir must be >= 1");
        if (ndrift < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_drifts_hvp: the member count must be >= 1");
        JQ_ON_FIRST(h, jq_eval_f_g_grad_drifts_hvp(s0_, pcof, ncoeff, dirs, ndir, drifts, weights, ndrift, out2, infid_grad, leak_grad, hv_infid, hv_leak))
        if (int rc = tl_refuse(h, "jq_eval_f_g_grad_drifts_hvp", true)) return rc;
        if (int rc = check_ncoeff(h, ncoeff)) return rc;
        EvalGate gate(h);
        return ens_hvp_dispatch(h, {"jq_eval_f_g_grad_drifts_hvp", pcof, dirs, nullptr, weights, nullptr, drifts, ncoeff, ndir, ndrift, out2, infid_grad, leak_grad, hv_infid,
                                 hv_leak});
    });
}

extern "C" int jq_eval_f_g_grad_members_hvp(jq_handle* h, const double* pcof, int32_t ncoeff, const double* dirs, int32_t ndir, const double* Hconsts,
                                            const double* ctrl_mix, const double* weights, int32_t nmember, double* out2, double* infid_grad,
                                            double* leak_grad, double* hv_infid, double* hv_leak)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_eval_f_g_grad_members_hvp", [&]() -> int {
        if (!dirs || !weights || !infid_grad || !leak_grad || !hv_infid || !hv_leak) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_members_hvp: NULL pointer");
        if (int rc = members_args(h, "jq_eval_f_g_grad_members_hvp", false, pcof, Hconsts, ctrl_mix, nmember, out2)) return rc;      // (jq_eval_f_g_grad_members' rules)
        if (ndir < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_members_hvp: ndir must be >= 1");
        JQ_ON_FIRST(h, jq_eval_f_g_grad_members_hvp(s0_, pcof, ncoeff, dirs, ndir, Hconsts, ctrl_mix, weights, nmember, out2, infid_grad, leak_grad, hv_infid, hv_leak))
        if (int rc = tl_refuse(h, "jq_eval_f_g_grad_members_hvp", true)) return rc;
        if (int rc = check_ncoeff(h, ncoeff)) return rc;
        EvalGate gate(h);
        EnsHvpArgs x = {"jq_eval_f_g_grad_members_hvp", pcof, dirs, nullptr, weights, nullptr, Hconsts, ncoeff, ndir, nmember, out2, infid_grad, leak_grad, hv_infid, hv_leak};
        x.mix = ctrl_mix, x.member_call = true;
        return ens_hvp_dispatch(h, x);
    });
}
