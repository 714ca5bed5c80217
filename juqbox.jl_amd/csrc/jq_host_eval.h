// jq_host_eval.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// run_eval: one EvalRequest -- everything an evaluation is given; the handle carries none of it -- evaluated by its plan (plan_batch,
// jq_host_plan.h), chunk by chunk, into an EvalOut; and what the entry points make of an EvalOut (out_record, out_grads, timing_add).
struct EvalRequest {
    const double* pcof = nullptr;   // ncoeff coefficients (grouped batch: `groups` blocks of them)
    int ncoeff = 0;
    int nsamples = 1;               // (grouped batch: groups x spg)
    const double* eps = nullptr;    // [nsamples] perturbation per sample (NULL: none); grouped batch: [nodes], the same for every vector
    const double* wgt = nullptr;    // ... weight per sample (NULL: 1)
    const double* shift = nullptr;  // [Ntot] perturbation per level (NULL: the reference's table)
    bool adjoint = false;
    double *hist_r = nullptr, *hist_i = nullptr;   // DEVICE arrays of Ntot x N x (nsteps + 1) doubles: the state history of the one sample
    double* d_packed = nullptr;     // the packed ensemble result (k_pack) is also left at this DEVICE address of h's GPU
    // grouped batch (pcof_batch): `groups` control vectors (0: none), each padded to `spg` samples (cooperative-quad kernels with N < 4: a column
    // quad per vector, the other columns weigh 0), of which the first `nodes` are the caller's
    int groups = 0, spg = 1, nodes = 1;
    // drift ensemble (jq_traceobjgrad_drifts): HOST array [Ntot x Ntot x groups] of member drifts (NULL: none), a grouped batch whose groups
    // share ONE control vector (pcof: ncoeff coefficients) and differ in image 0 of their tile stream
    const double* drifts = nullptr;
    // control mixes (jq_traceobjgrad_members): HOST array [Nc x Nc x max(groups, 1)] column-major (NULL: none) -- what reaches operator l of
    // group g is sum_k C_g[l, k] (p_k, q_k).  In a grouped batch the groups share ONE control vector, as with drifts; without groups it is
    // the mix of the single evaluation.  Only k_ctrl and k_trace_reduce see it.
    const double* mix = nullptr;
    // controls as samples on the time grid (jq_traceobjgrad_samples): HOST array [2 Nc x nt], nt = 2 nsteps + 1 (NULL: none), the values
    // (p_1, q_1, p_2, q_2, ...) at every time point of jq_sample_times.  It takes the place of the coefficients: pcof is not read, ncoeff
    // = 2 Nc nt is the length of the gradients, which are those with respect to the samples.  Only k_ctrl_samples and k_gradsamples see it.
    const double* samples = nullptr;
    // ... in a grouped batch (jq_host_samples_batch.h): `groups` tables one after the other (jq_traceobjgrad_samples_batch), or -- with
    // drifts / mix -- the ONE table the members share, uploaded once.  Only k_ctrl_samples_members and k_gradsamples_grouped see those.
    // ens_w (jq_eval_f_g_grad_samples_members; NULL: none): HOST weights [max(groups, 1)] of the launch's members.  The gradients of the
    // EvalOut are then ONE pair of tables, ens_acc0 / ens_acc1 (HOST [ncoeff]; NULL: zeros) plus the members' weighted gradients in member
    // order (k_gradsamples_wsum) -- the members' own tables are not fetched.
    const double *ens_w = nullptr, *ens_acc0 = nullptr, *ens_acc1 = nullptr;
    bool split_part = false;        // one part of a split batch: not split again
};
struct EvalOut {
    std::vector<double> res;    // [nsamples][4] primary, secondary, Re s, Im s
    std::vector<double> grad0;  // forced adjoint (total gradient), weighted sum over samples
    std::vector<double> grad1;  // unforced adjoint (infidelity gradient), only objFuncType != 1
};
// (objfv, primaryobjf, secondaryobjf, traceInfidelity) of a sample from its record in EvalOut::res
static void out_record(double* out4, const double* res)
{
    const double primary = res[0], secondary = res[1];
    out4[0] = primary + secondary;  // objfv (src/evalobjgrad.jl:765-766)
    out4[1] = primary;
    out4[2] = secondary;
    out4[3] = primary;              // traceInfidelity == 1 - |s|^2 for pFidType 2 (:792)
}
// the gradients the reference returns from the forced (g0) and the unforced (g1, objFuncType != 1 only) adjoint; total may be NULL
static void out_grads(const jq_handle* h, int ncoeff, const double* g0, const double* g1, double* total, double* infid, double* leak)
{
    const bool two = h->objFuncType != 1;
    for (int i = 0; i < ncoeff; ++i) {
        if (total) total[i] = g0[i];
        infid[i] = two ? g1[i] : g0[i];       // "infidelgrad stores the totalgrad" (src/evalobjgrad.jl:949-951)
        leak[i] = two ? g0[i] - g1[i] : 0.0;  // :947
    }
}
// the fields of a timing record that add up over the launches of one call
static void timing_add(jq_timing& sum, const jq_timing& part)
{
    sum.ms_total += part.ms_total, sum.ms_propagate += part.ms_propagate, sum.ms_generate += part.ms_generate;
    sum.ms_forward += part.ms_forward, sum.ms_backward += part.ms_backward;
    sum.n_forward_launches += part.n_forward_launches, sum.n_backward_launches += part.n_backward_launches;
    sum.mfma_executed += part.mfma_executed, sum.mfma_backward += part.mfma_backward, sum.svts += part.svts;
}

__global__ void k_add_to(double* __restrict__ y, const double* __restrict__ x, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += x[i];
}

// the coefficient count of a control vector (src/evalobjgrad.jl:604-608, src/bsplines.jl:177-181): the codes of every evaluation entry point
static int check_ncoeff(jq_handle* h, int ncoeff)
{
    const int Nsig = 2 * h->Nc;
    // src/evalobjgrad.jl:604-606
    if (ncoeff % Nsig != 0 || ncoeff < 3 * Nsig) {
        char buf[160];
        snprintf(buf, sizeof buf, "pcof must have an even number of elements >= %d, not %d", 3 * Nsig, ncoeff);
        return fail(h, JQ_EINVAL, buf);
    }
    const int D1 = ncoeff / (Nsig * h->Nfreq);  // :608
    // bcparams: nCoeff = Nfreq*D1*2*Ncoupled must equal length(pcof) (src/bsplines.jl:177-181)
    if (h->Nfreq * D1 * Nsig != ncoeff)
        return fail(h, JQ_EDIM, "DimensionMismatch: Inconsistent number of coefficients and size of parameter vector (nCoeff != length(pcof))");
    if (D1 < 3) return fail(h, JQ_EINVAL, "need at least 3 B-spline coefficients per control function");
    return JQ_OK;
}
// The handle that evaluates a Stormer-Verlet batch of `nsamples` samples without a state history: h, or its embedded twin (structure
// embedding, try_embed: batches that would run on the dense / band MFMA families go to the twin, whose operators have the JQ_BW_T4 structure)
static jq_handle* eval_target(jq_handle* h, int nsamples, bool hist)
{
    if (h->emb && !hist && h->integrator == 1) {
        const long long nc_used = (long long)nsamples * h->N;
        // (full leakage weights: the row-lane kernels take every batch of an Ntot <= 16 problem -- the lane kernels have no low-rank terms)
        const bool small_family = h->solver_id == 1 && ((h->rl_npj > 0 && (nc_used <= h->rl_max_cols || h->wrank > 0)) ||
                                                        (h->lane_np > 0 && nc_used >= h->lane_min_cols && nc_used <= h->lane_max_cols));
        if (h->emb_mode == 2 || !small_family) return h->emb;
    }
    return h;
}
// The batched evaluation behind every hot-path entry point.  It writes the handle's buffers and their capacities, the bookkeeping of the
// three-workgroup kernels, `timing` and `err`.
// what every sampled-controls call refuses before anything is written: uncoupled controls -- ft is a function of BOTH slots of a pair
// and of the rotation frequency, so a table of (p, q) values is not what their operators are driven with
static int samples_refuse(jq_handle* h, const char* who)
{
    if (!h->rfreq.empty())
        return fail(h, JQ_EUNSUPPORTED, (std::string(who) + ": uncoupled controls are not served with sampled controls (their operators are driven by "
                                                            "ft = 2 (p cos(2 pi Rfreq t) - q sin(2 pi Rfreq t)), not by p and q)").c_str());
    return JQ_OK;
}
#define JQ_ERETRY_INTERNAL (-1000)      // run_eval_impl: k_backward_cq3 gave up (the handle leaves it alone for a while): evaluate again
#define JQ_CQ3_MAX_FAULTS 6
static int run_eval_impl(jq_handle* h, const EvalRequest& rq, EvalOut* out);
static int run_eval(jq_handle* h, const EvalRequest& rq, EvalOut* out)
{
    EvalGate gate(h);
    int rc = run_eval_impl(h, rq, out);
    if (rc == JQ_ERETRY_INTERNAL) rc = run_eval_impl(h, rq, out);
    return rc;
}
// the handle's event pool holds at least nev events ([0] = start, [1] = end of a call, then pairs around its propagator launches)
static int ensure_events(jq_handle* h, size_t nev)
{
    while (h->ev.size() < nev) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreate(&e));
        h->ev.push_back(e);
    }
    return JQ_OK;
}
// The operator schedule of a sweep's launches from the family's rows of JQ_SCHED (rows = JQ_SCHED[cooperative]; kind 0 K, 1 S at time
// point 0, 1, 2 of a step = t_n "n0 / 0", t_n + h/2 "p05 / 05", t_n + h "n1 / 1"; kind 2: image q of the launch's trace images
// [Hsym_q.. | Hanti_q..]).  Forward: the first seven entries,
//   slab kernels Kp05 S05 Kn0 S0 Kn1 S1 Kp05, cooperative kernels Kp05 S05 Kn0 Kn1 S0 S1 Kp05.
// Backward: all eight (the seven and S0), then the same tail for every family,
//   | Hanti_q.. (early traces) | Kn0 Kn1 S05 Kp05 S1 | (Hanti_q Hsym_q).. (late traces),
// and, for a sweep's first chunk (npro = ng, the caller's), the carry products with Hsym_q in pro_bits.
static void pack_forward_schedule(PropArgs& a, const int (*rows)[8])
{
    a.period = 7; a.npro = 0;
    a.sched_bits[0] = a.sched_bits[1] = a.sched_bits[2] = a.pro_bits = 0;
    for (int i = 0; i < 7; ++i) sched_pack(a.sched_bits, i, rows[0][i], rows[1][i]);
}
static void pack_backward_schedule(PropArgs& a, const int (*rows)[8], int ng)
{
    const int kinds2[5] = {0, 0, 1, 0, 1}, tps2[5] = {0, 2, 1, 1, 2};
    a.period = 13 + 3 * ng;
    a.sched_bits[0] = a.sched_bits[1] = a.sched_bits[2] = a.pro_bits = 0;
    int k = 0;
    for (int i = 0; i < 8; ++i) sched_pack(a.sched_bits, k++, rows[0][i], rows[1][i]);
    for (int q = 0; q < ng; ++q) sched_pack(a.sched_bits, k++, 2, ng + q);
    for (int i = 0; i < 5; ++i) sched_pack(a.sched_bits, k++, kinds2[i], tps2[i]);
    for (int q = 0; q < ng; ++q) {
        sched_pack(a.sched_bits, k++, 2, ng + q);
        sched_pack(a.sched_bits, k++, 2, q);
        sched_pack(&a.pro_bits, q, 2, q);
    }
}
// k_terminal_cols (jq_aux_kernels.h) on `files` state files, dstride doubles apart: a thread per sample and file
template <int FLAVOR, class Map>
static void terminal_cols(hipStream_t s, Map m, int files, double* state, size_t dstride, const double* vtr, const double* vti, const double* dvr,
                          const double* dvi, int mode, int N, int nsamples, double leak_scale, double* res)
{
    hipLaunchKernelGGL((k_terminal_cols<Map, FLAVOR>), dim3((unsigned)((nsamples + 63) / 64), (unsigned)files), dim3(64), 0, s, m, state,
                       (long long)dstride, vtr, vti, dvr, dvi, mode, N, nsamples, leak_scale, res);
}

static int run_eval_impl(jq_handle* h, const EvalRequest& rq, EvalOut* out)
{
    const bool sampled = rq.samples != nullptr;      // (the sample table travels where the coefficients do: d_pcof)
    const double *const pcof = sampled ? rq.samples : rq.pcof, *const shift = rq.shift, *eps = rq.eps, *wgt = rq.wgt;      // (eps, wgt: a grouped batch expands them below)
    const int ncoeff = rq.ncoeff, nsamples = rq.nsamples;
    const int nt = 2 * h->nsteps + 1;
    if (sampled) {
        if (int rc = samples_refuse(h, "run_eval")) return rc;
        if ((rq.groups > 0 || rq.drifts || rq.mix) && (rq.eps || rq.wgt || rq.nodes != 1 || rq.hist_r || rq.d_packed))
            return fail(h, JQ_EUNSUPPORTED, "sampled controls in a batch of tables or a member ensemble together with eps nodes, a state history or a packed result are not served");
        if (ncoeff != 2 * h->Nc * nt) return fail(h, JQ_EHIP, "internal error: sampled controls with a gradient length other than 2 Nc nt");
    }
    if (rq.ens_w && !sampled) return fail(h, JQ_EHIP, "internal error: ensemble weights without sampled controls");
    const bool adjoint = rq.adjoint;
    double *const hist_r = rq.hist_r, *const hist_i = rq.hist_i, *const d_packed = rq.d_packed;
    HIPCHK(h, hipSetDevice(h->device));
    // Ensembles that do not fill their last round: the time of a batch is a staircase in its size (every workgroup runs the
    // whole sequential time loop; cnot3: 3 072 samples = one round of the three-slab quad-layout kernels 1.18 s, 3 200 samples =
    // two rounds 2.35 s).  A batch of q full rounds + a remainder is evaluated as two batches when the plan says that is
    // faster -- the remainder on whatever suits ITS size (3 200 samples: 1.18 + 0.20 s on the cooperative-quad kernels).
    // Samples are independent and the results are sums over samples, so only the order of those sums changes.
    // (the cost model is that of the 4 x 4 x n MFMA families: a batch that the row-lane / lane kernels take -- small Hilbert spaces
    //  with that structure, e.g. SWAP-02 -- must not be split: round 2 did, and paid two latency-bound launches for one)
    const long long ncols_split = (long long)nsamples * h->N;
    const bool small_family_batch = (h->rl_npj > 0 && ncols_split <= h->rl_max_cols) ||
                                    (h->lane_np > 0 && ncols_split >= h->lane_min_cols && ncols_split <= h->lane_max_cols);
    if (!rq.split_part && rq.groups == 0 && !small_family_batch && h->wrank == 0 && h->quad_max_slabs > 0 && h->integrator == 1 && h->solver_id == 1 && !hist_r && eps && nsamples > 1 && !h->opt.on(O_NOSPLIT)) {
        // candidates: the largest number of FULL rounds of the quad-layout kernels with 1, 2 or 3 slabs per workgroup
        long long n_main = 0;
        double best = t4_plan_cost(h, nsamples) - 1e-9;
        for (int k = 1; k <= 3; ++k) {
            const long long per_round = (long long)k * h->num_cu * (h->parts > 1 ? 1 : h->sps) / (h->parts > 1 ? h->parts : 1);      // samples of a full round
            const long long nm = per_round > 0 ? (long long)nsamples / per_round * per_round : 0;
            if (nm <= 0 || nm >= nsamples) continue;
            const double c = t4_plan_cost(h, nm) + t4_plan_cost(h, nsamples - nm);
            if (c < best) best = c, n_main = nm;
        }
        if (n_main > 0) {
            EvalOut o2;
            const int n1 = (int)n_main, n2 = nsamples - n1;
            EvalRequest part = rq;
            part.split_part = true, part.nsamples = n1;
            int rc = run_eval(h, part, out);
            const jq_timing t1 = h->timing;
            const KernelSel k1 = h->last_kernels;
            const size_t npk = (size_t)2 + 2 * (size_t)ncoeff;
            if (rc == JQ_OK && d_packed) {
                rc = dev_grow(h, &h->d_pk2, &h->cap_pk2, npk);
                if (rc == JQ_OK && hipMemcpyAsync(h->d_pk2, d_packed, npk * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
                    rc = fail(h, JQ_EHIP, "hipMemcpyAsync (packed result of the first part of a split batch)");
            }
            part.nsamples = n2, part.eps = eps + n1, part.wgt = wgt ? wgt + n1 : nullptr;
            if (rc == JQ_OK) rc = run_eval(h, part, &o2);
            if (rc != JQ_OK) return rc;
            if (d_packed) {
                hipLaunchKernelGGL(k_add_to, dim3((unsigned)((npk + 255) / 256)), dim3(256), 0, h->stream, d_packed, h->d_pk2, (int)npk);
                HIPCHK(h, hipGetLastError());
                HIPCHK(h, hipStreamSynchronize(h->stream));
            }
            out->res.insert(out->res.end(), o2.res.begin(), o2.res.end());
            for (size_t i = 0; i < out->grad0.size() && i < o2.grad0.size(); ++i) out->grad0[i] += o2.grad0[i];
            for (size_t i = 0; i < out->grad1.size() && i < o2.grad1.size(); ++i) out->grad1[i] += o2.grad1[i];
            // timing: sums; the kernel family / size / band reported are those of the first (larger) part
            timing_add(h->timing, t1);
            h->timing.kernel_family = t1.kernel_family, h->timing.kernel_size = t1.kernel_size, h->timing.kernel_band = t1.kernel_band;
            h->last_kernels = k1;
            h->timing.ms_shard_min = h->timing.ms_shard_max = h->timing.ms_total;
            if (sampled) h->sc_nodes = nsamples;
            return JQ_OK;
        }
    }
    int rc = sampled ? JQ_OK : check_ncoeff(h, ncoeff);
    if (rc) return rc;
    const int D1 = sampled ? 3 : ncoeff / (2 * h->Nc * h->Nfreq);  // src/evalobjgrad.jl:608 (sampled controls: no spline is evaluated)
    if (nsamples < 1) return fail(h, JQ_EINVAL, "need at least one sample");
    // grouped batch (pcof_batch): G control vectors, pcof = their G coefficient blocks, nsamples = G x spg samples: per vector the Q samples
    // of the caller (eps, wgt: [Q], the same nodes for every vector; without them one sample of weight 1) and the padding that ends its
    // last column quad
    const int G = rq.groups, spg = rq.spg, Q = rq.nodes;
    if (G > 0 && (nsamples != G * spg || Q < 1 || Q > spg || hist_r || d_packed)) return fail(h, JQ_EHIP, "internal error: grouped batch with a state history or a packed result");
    if (rq.drifts && G == 0) return fail(h, JQ_EHIP, "internal error: member drifts outside a grouped batch");
    const int nvec = G > 0 ? G : 1;      // (coefficient blocks, tile streams, gradients of the launch)
    // sample tables per group, or one table under a mix: the grouped sample kernels take the place of k_ctrl_samples / k_gradsamples
    const bool sampled_grp = sampled && (G > 0 || rq.mix);
    const bool shared_table = sampled && (rq.drifts || rq.mix);      // (an ensemble's members share ONE table: no copies)
    const int ntab = (sampled && !shared_table) ? nvec : 1;
    const bool ens = rq.ens_w != nullptr && adjoint;
    // Structure embedding (try_embed): batches that would run on the dense / band MFMA families go to the embedded twin,
    // whose operators have the JQ_BW_T4 structure (quad-layout / JQ_BW_T4 slab kernels).  State histories stay here (their
    // rows are the user's), the implicit-midpoint path too.
    if (eval_target(h, nsamples, hist_r != nullptr) != h) {
        jq_handle* e = h->emb;
        std::vector<double> sh(e->Ntot, 0.0);
        for (int i = 0; i < h->Ntot; ++i)   // (default: the reference's 0.01 * 10^(j-2) by the USER's level index, src/ipopt_interface.jl:41-44)
            sh[h->emb_row[i]] = shift ? shift[i] : (i >= 1 ? 0.01 * pow(10.0, (double)(i - 1)) : 0.0);
        EvalRequest er = rq;      // (a grouped batch stays one; eps, wgt: the caller's)
        er.shift = sh.data();
        std::vector<double> ed;      // (member drifts in the twin's rows, like jq_update_hconst embeds the handle's)
        if (rq.drifts) {
            const size_t nn = (size_t)h->Ntot * h->Ntot, ne = (size_t)e->Ntot * e->Ntot;
            ed.assign((size_t)G * ne, 0.0);
            for (int g = 0; g < G; ++g) embed_matrix(rq.drifts + (size_t)g * nn, h->Ntot, h->emb_row, e->Ntot, ed.data() + (size_t)g * ne);
            er.drifts = ed.data();
        }
        // (er.mix: the caller's, unchanged -- the twin has the same controls)
        const int rc = run_eval(e, er, out);
        if (rc != JQ_OK) h->err = e->err;
        h->timing = e->timing;
        if (rc == JQ_OK) h->last_kernels = e->last_kernels;
        if (rc == JQ_OK && sampled) h->sc_nt = e->sc_nt, h->sc_nodes = e->sc_nodes, h->sc_chunk = e->sc_chunk;
        return rc;
    }
    GateHold gate_hold;      // (held until the evaluation ends when the plan takes the split latency kernels)
    BatchPlan p;
    rc = plan_batch(h, nsamples, adjoint, hist_r != nullptr, gate_hold, &p, G);
    if (rc) return rc;
    if (p.groups != G) return fail(h, JQ_EHIP, "internal error: grouped batch on a kernel family that does not serve one");
    std::vector<double> gwgt, geps;
    if (G > 0 && (spg > 1 || eps || wgt)) {      // (the padding samples of a vector's column quad weigh nothing -- like the unused columns of a single evaluation's quad)
        gwgt.assign((size_t)nsamples, 0.0);
        if (eps) geps.assign((size_t)nsamples, 0.0);
        for (int g = 0; g < G; ++g)
            for (int q = 0; q < Q; ++q) {
                gwgt[(size_t)g * spg + q] = wgt ? wgt[q] : 1.0;
                if (eps) geps[(size_t)g * spg + q] = eps[q];
            }
        wgt = gwgt.data();
        if (eps) eps = geps.data();
    }
    const bool imr = (h->integrator == 2);
    const bool cq3 = p.cq_nr > 0, qsplit = p.qs_qw > 0;
    const long long ncols_used = (long long)nsamples * h->N;
    const int ntr = h->NcK * JQ_NTR;      // (trace scalars per step of the LARGEST control group)
    const int ngroups = ctrl_ngroups(h->Nc);
    const bool two_pass = adjoint && h->objFuncType != 1;

    // ---- capacity ------------------------------------------------------------------------------
    if ((rc = dev_grow(h, &h->d_pcof, &h->cap_pcof, (size_t)(sampled ? ntab : nvec) * ncoeff))) return rc;
    const size_t gstride = G > 0 ? (size_t)(2 * p.cs + 1) * 2 * (size_t)p.stride : 0;      // doubles between the tile streams of two vectors
    if (G > 0) {      // (sized by jq_create for ONE vector and the handle's chunk length)
        if ((rc = dev_grow(h, &h->d_stream, &h->cap_stream, (size_t)G * gstride))) return rc;
        if ((rc = dev_grow(h, &h->d_pq, &h->cap_pq, (size_t)G * (2 * p.cs + 1) * 2 * h->Nc))) return rc;
        if (adjoint && (rc = dev_grow(h, &h->d_R, &h->cap_R, (size_t)G * p.cs * h->NcK * JQ_NTR))) return rc;
    }
    const size_t ncnc = (size_t)h->Nc * h->Nc;
    if (rq.mix) {      // (the mixes, k_ctrl's unmixed values in the layout of d_pq, trace rows for ALL controls per group)
        if ((rc = dev_grow(h, &h->d_mix, &h->cap_mix, (size_t)nvec * ncnc + (size_t)nvec * (2 * p.cs + 1) * 2 * h->Nc))) return rc;
        if (adjoint && (rc = dev_grow(h, &h->d_R, &h->cap_R, (size_t)nvec * p.cs * h->Nc * JQ_NTR))) return rc;
    }
    if (p.state_doubles > h->cap_state || !h->d_state || !h->d_state_save) {
        h->cap_state = 0;
        if ((rc = dev_alloc(h, &h->d_state, p.state_doubles))) return rc;
        if ((rc = dev_alloc(h, &h->d_state_save, p.state_doubles))) return rc;
        h->cap_state = p.state_doubles;
    }
    if ((rc = dev_grow(h, &h->d_colinfo, &h->cap_colinfo, p.colinfo_doubles))) return rc;
    if (p.park_slabs && (p.park_slabs > h->cap_slabs || !h->d_park)) {
        h->cap_slabs = 0;
        if ((rc = dev_alloc(h, &h->d_park, p.park_slabs * h->KT * 64))) return rc;
        h->cap_slabs = p.park_slabs;
    }
    if (adjoint && (rc = dev_grow(h, &h->d_traces, &h->cap_traces, (size_t)p.trace_rows * p.cs * ntr))) return rc;
    if ((rc = dev_grow(h, &h->d_grad, &h->cap_grad, (size_t)(nvec + (ens ? 1 : 0)) * 2 * ncoeff))) return rc;      // [vector][forced | unforced][ncoeff] (+ the ensemble's pair)
    if (ens && (rc = dev_grow(h, &h->d_wq, &h->cap_wq, (size_t)nvec))) return rc;
    if ((rc = dev_grow(h, &h->d_res, &h->cap_res, (size_t)nsamples * 4))) return rc;
    const size_t cq3_quad = 64 + (size_t)8 * 8 * h->NT * 64 + 64;      // doubles per quad: JQ_CQ3_HEAD + JQ_CQ3_SLOTS * JQ_CQ3_ARRAYS * NT * 64 + JQ_CQ3_TAIL
    if (cq3) {
        if ((rc = dev_grow(h, &h->d_cq3, &h->cap_cq3, 64 + (size_t)p.nq_pad * cq3_quad))) return rc;
        HIPCHK(h, hipMemsetAsync(h->d_cq3, 0, 64 * sizeof(double), h->stream));      // (the error word of the evaluation)
    }
    if (qsplit && (rc = dev_grow(h, &h->d_qsplit, &h->cap_qsplit, (size_t)p.qs_blocks * p.qs_qw * 2 * JQ_QS_ARRAYS * h->NT * 64))) return rc;

    // ---- inputs --------------------------------------------------------------------------------
    hipStream_t s = h->stream;
    std::vector<double> gpcof, dimg;
    const bool one_vector = G > 0 && (rq.drifts || rq.mix);      // (an ensemble's members share ONE control vector)
    // one control vector for every group: its block replicated (k_ctrl, k_gradacc stay the launches of a control-vector batch)
    if (one_vector && !sampled)
        for (int g = 0; g < G; ++g) gpcof.insert(gpcof.end(), pcof, pcof + ncoeff);
    if (rq.drifts) {
        // the members' drift images in the planned family's layout -- the builders and the bits of upload_operators' image 0
        const size_t nn = (size_t)h->Ntot * h->Ntot;
        dimg.assign((size_t)G * (size_t)p.stride, 0.0);
        for (int g = 0; g < G; ++g) {
            const double* M = rq.drifts + (size_t)g * nn;
            double* img = dimg.data() + (size_t)g * (size_t)p.stride;
            if (p.dense) dq_image(M, h->Ntot, img);
            else if (p.family == KF_ROWLANE) rowlane_image(M, h->Ntot, h->rl_npj, img);
            else if (p.family == KF_CQ && !h->big) tile_image(M, h->Ntot, h->NT, h->BW, img);
            else return fail(h, JQ_EHIP, "internal error: drift ensemble on a kernel family without grouped streams");
        }
        if ((rc = dev_grow(h, &h->d_drift, &h->cap_drift, dimg.size()))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->d_drift, dimg.data(), dimg.size() * sizeof(double), hipMemcpyHostToDevice, s));
    }
    const double* const h0img = rq.drifts ? h->d_drift : p.himg;      // image 0 of group 0 and the stride to the next group's
    const long long h0_gstride = rq.drifts ? p.stride : 0;
    if (sampled)
        HIPCHK(h, hipMemcpyAsync(h->d_pcof, pcof, (size_t)ntab * ncoeff * sizeof(double), hipMemcpyHostToDevice, s));
    else
        HIPCHK(h, hipMemcpyAsync(h->d_pcof, one_vector ? gpcof.data() : pcof, (size_t)nvec * ncoeff * sizeof(double), hipMemcpyHostToDevice, s));
    if (rq.mix) HIPCHK(h, hipMemcpyAsync(h->d_mix, rq.mix, (size_t)nvec * ncnc * sizeof(double), hipMemcpyHostToDevice, s));
    const double* const d_mix = rq.mix ? h->d_mix : nullptr;
    double* const d_pqraw = rq.mix ? h->d_mix + (size_t)nvec * ncnc : nullptr;
    bool use_shift = false;
    std::vector<double> colinfo(p.colinfo_doubles, 0.0);
    if (p.layout != SL_SLABS) {   // [eps per column slot | weight per column slot]  (lane kernels: cpw = 4, one slot per column)
        for (long long c = 0; c < ncols_used; ++c) {
            const int smp = (int)(c / h->N);
            const long long slot = (c / p.cpw) * 4 * p.wpg + (c % p.cpw);
            colinfo[slot] = eps ? eps[smp] : 0.0;
            colinfo[p.ncols + slot] = wgt ? wgt[smp] : 1.0;
            if (eps && eps[smp] != 0.0) use_shift = true;
        }
    } else {
        for (int sl = 0; sl < p.nslabs; ++sl)
            for (int c = 0; c < (h->parts > 1 ? 16 : h->sps * h->N); ++c) {
                const int smp = h->parts > 1 ? sl / h->parts : sl * h->sps + c / h->N;
                if (smp < nsamples && (h->parts == 1 || 16 * (sl % h->parts) + c < h->N)) {
                    colinfo[(size_t)sl * 32 + c] = eps ? eps[smp] : 0.0;
                    colinfo[(size_t)sl * 32 + 16 + c] = wgt ? wgt[smp] : 1.0;
                    if (eps && eps[smp] != 0.0) use_shift = true;
                }
            }
    }
    HIPCHK(h, hipMemcpyAsync(h->d_colinfo, colinfo.data(), colinfo.size() * sizeof(double), hipMemcpyHostToDevice, s));
    std::vector<double> tabs((size_t)32 * h->NT, 0.0);
    for (int i = 0; i < h->Ntot; ++i) {
        tabs[i] = h->wd[i];
        // reference perturbation: Hconst[j,j] += ep*0.01*10^(j-2), j = 2..Ntot (src/ipopt_interface.jl:41-44)
        tabs[p.ws_off + i] = shift ? shift[i] : (i >= 1 ? 0.01 * pow(10.0, (double)(i - 1)) : 0.0);
    }
    HIPCHK(h, hipMemcpyAsync(h->d_tabs, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemsetAsync(h->d_grad, 0, (size_t)(nvec + (ens ? 1 : 0)) * 2 * ncoeff * sizeof(double), s));
    double* const d_ens = h->d_grad + (size_t)nvec * 2 * ncoeff;      // (the ensemble's pair of tables, behind the members')
    if (ens) {
        if (rq.ens_acc0) HIPCHK(h, hipMemcpyAsync(d_ens, rq.ens_acc0, (size_t)ncoeff * sizeof(double), hipMemcpyHostToDevice, s));
        if (rq.ens_acc1 && two_pass) HIPCHK(h, hipMemcpyAsync(d_ens + ncoeff, rq.ens_acc1, (size_t)ncoeff * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemcpyAsync(h->d_wq, rq.ens_w, (size_t)nvec * sizeof(double), hipMemcpyHostToDevice, s));
    }
    const long long tstride = shared_table ? 0 : ncoeff;      // doubles between the tables of two groups

    SplineArgs sp;
    sp.pcof = h->d_pcof; sp.cfreq = h->d_cfreq; sp.D1 = D1; sp.Nfreq = h->Nfreq; sp.Ncoupled = h->Nc; sp.nCoeff = ncoeff;
    sp.dtknot = h->T / (D1 - 2);
    sp.rfreq = h->rfreq.empty() ? nullptr : h->d_rfreq;

    const double dt = h->T / h->nsteps;
    PropArgs a;
    memset(&a, 0, sizeof a);
    a.stream = h->d_stream; a.stream_gstride = (long long)gstride; a.group_units = G > 0 ? p.upg : 1; a.cimg = p.cimg; a.state = h->d_state; a.colinfo = h->d_colinfo;
    a.traces = h->d_traces;
    a.tabs = h->d_tabs; a.stride = p.stride; a.pieces = (int)(p.stride * 8 / 1024); a.m = h->m;
    a.nslabs = p.prop_nslabs; a.Ncoupled = ctrl_gstart(h->Nc, 1) /* first control group */; a.Ntot = h->Ntot; a.N = h->N; a.use_shift = use_shift ? 1 : 0;
    a.tinv = 1.0 / h->T; a.state_stride = h->state_stride; a.parts = h->parts; a.nsamples = nsamples; a.sps = h->sps; a.qps = p.qps;
    a.wlr = h->d_wlr; a.wrank = h->wrank; a.wlam = h->wlam; a.wstride = h->NP; a.wcplx = (h->wrank > 0 && !h->wlr_real) ? 1 : 0;
    // JACOBI_SOLVER: the kernels iterate on c-scaled right-hand sides (A = c rhs, c = h / 2: DESIGN.md section 3), so their
    // residual norm is |c| times the reference's ||X_j - X_{j-1}|| (src/linear_solvers.jl:121): the threshold is scaled alike
    a.jacobi_tol2 = (h->solver_id == 2) ? (h->solver_tol * 0.5 * dt) * (h->solver_tol * 0.5 * dt) : 0.0;
    if (imr) {   // fixed-point solver of the implicit-midpoint step: iteration cap and per-lane threshold (jq_rowlane_imr_kernels.h)
        a.m = h->imr_max_iter;
        a.jacobi_tol2 = h->imr_tol * h->imr_tol;
    }
    for (int q = 0; q < JQ_MAXNC; ++q) a.bw_trace[q] = q < h->Nc ? h->bw_trace[q] : 0;      // (first control group; the backward sweeps set their own)
    a.batch = p.batch; a.lds_tab_off = (int)p.lds_stage;
    a.park = h->d_park; a.park_lds = p.park_lds;
    a.debug = (int)h->opt.get(O_DEBUG);
    if (p.layout == SL_SLABS) {
        HIPCHK(h, hipFuncSetAttribute((const void*)p.kfwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.fwd.total));
        HIPCHK(h, hipFuncSetAttribute((const void*)p.kbwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.bwd.total));
    }

    // events: [0]=start [1]=end, then pairs around every propagator launch
    const int nchunks = (h->nsteps + p.cs - 1) / p.cs;
    const size_t nev = 2 + 2 * (size_t)nchunks * (1 + (adjoint ? (two_pass ? 2 : 1) * ngroups : 0));
    if ((rc = ensure_events(h, nev))) return rc;
    size_t evi = 2;
    HIPCHK(h, hipEventRecord(h->ev[0], s));

    if (p.layout == SL_ROWLANE)
        hipLaunchKernelGGL(k_init_rowlane, dim3((unsigned)p.nwaves_rl), dim3(64), 0, s, h->d_state, p.nwaves_rl, JQ_ROWLANE_ROWS, 0LL, h->d_uinit_r,
                           h->N, ncols_used, p.cpw, p.wpg);
    else if (p.layout == SL_LANE)
        hipLaunchKernelGGL(k_init_lane, dim3((unsigned)(p.ncols / 64)), dim3(64), 0, s, h->d_state, p.ncols, h->lane_np, JQ_LANE_ROWS(h->lane_np), 0LL,
                           h->d_uinit_l, h->N, ncols_used, p.ncols);
    else
        hipLaunchKernelGGL(k_init_state, dim3(p.nslabs), dim3(64), 0, s, h->d_state, h->state_stride, h->d_uimg, h->KT, h->parts);

    long long mfma = 0, mfma_fwd = 0;
    // ---- forward sweep -------------------------------------------------------------------------
    for (int n0 = 0; n0 < h->nsteps; n0 += p.cs) {
        const int nc = std::min(p.cs, h->nsteps - n0);
        const int ntp = 2 * nc + 1;
        if (sampled_grp)
            hipLaunchKernelGGL(k_ctrl_samples_members, dim3((ntp + 127) / 128, nvec), dim3(128), 0, s, h->d_pcof, tstride, nt, 2 * n0, 1, ntp, h->Nc, d_mix, h->d_pq);
        else if (sampled)
            hipLaunchKernelGGL(k_ctrl_samples, dim3((ntp + 127) / 128), dim3(128), 0, s, h->d_pcof, nt, 2 * n0, 1, ntp, h->Nc, h->d_pq);
        else
            hipLaunchKernelGGL(k_ctrl, dim3((ntp + 127) / 128, nvec), dim3(128), 0, s, sp, h->d_tf, n0, ntp, dt, h->d_pq, d_mix, d_pqraw);
        hipLaunchKernelGGL(k_stream, dim3((unsigned)((p.stride + 255) / 256), ntp, nvec), dim3(256), 0, s, p.himg, h0img, h0_gstride,
                           h->d_pq, h->Nc, p.stride, 0.5 * dt, h->d_stream, (long long)gstride);
        a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0); a.h = dt; a.forced = 1;
        a.hist_r = hist_r; a.hist_i = hist_i;
        a.wlr_lds = p.fwd.wlr;
        a.wlr_sc_lds = p.fwd.wsc;
        a.jac_wg_lds = p.fwd.jac;
        a.nslots = h->nslots;
        pack_forward_schedule(a, p.sched);
        HIPCHK(h, hipEventRecord(h->ev[evi++], s));
        hipLaunchKernelGGL(p.kfwd, dim3(p.fwd_grid), dim3(p.fwd_block), p.fwd.total, s, a);
        HIPCHK(h, hipEventRecord(h->ev[evi++], s));
        mfma += (long long)p.nslabs * nc * (8 + 2 * h->m) * p.tiles;
    }
    HIPCHK(h, hipGetLastError());
    mfma_fwd = mfma;
    const double leak_scale = imr ? 0.25 * dt * (1.0 / h->T) : 0.5 * dt * (1.0 / h->T);
    // continuation adjoints (jq_set_sv_type): only the adjoint's terminal condition knows the type -- forward-only evaluations run as type 1,
    // the implicit-midpoint kernels have no other (plan_batch refused)
    const int sv_mode = (adjoint && !imr) ? h->sv_type : 1;
    if (sv_mode != 1 && (h->dv_stale || !h->dv_alloc)) return fail(h, JQ_EHIP, "internal error: sv_type != 1 without the dVds images on the device");
    if (p.term == TK_PARTS || p.term == TK_IMR_PARTS)
        hipLaunchKernelGGL(k_terminal_parts, dim3(nsamples), dim3(64), 0, s, h->d_state, h->state_stride, h->d_vtr, h->d_vti, h->KT,
                           h->N, h->parts, leak_scale, h->d_res, p.term == TK_IMR_PARTS, h->d_dvr, h->d_dvi, sv_mode);
    else if (p.term == TK_IMR)
        hipLaunchKernelGGL(k_terminal_imr, dim3(p.nslabs), dim3(64), 0, s, h->d_state, h->state_stride, h->d_vtr, h->d_vti, h->KT,
                           h->N, h->sps, nsamples, leak_scale, h->d_res);
    else if (p.term == TK_ROWLANE_IMR)
        terminal_cols<EP_IMR>(s, RowlaneMap{p.nwaves_rl, p.cpw, p.wpg, JQ_ROWLANE_ROWS - 1}, 1, h->d_state, 0, h->d_vtr_r, h->d_vti_r, nullptr, nullptr, 1,
                              h->N, nsamples, leak_scale, h->d_res);
    else if (p.term == TK_ROWLANE)
        terminal_cols<EP_SV>(s, RowlaneMap{p.nwaves_rl, p.cpw, p.wpg, JQ_ROWLANE_ROWS - 1}, 1, h->d_state, 0, h->d_vtr_r, h->d_vti_r, h->d_dvr_r, h->d_dvi_r,
                             sv_mode, h->N, nsamples, leak_scale, h->d_res);
    else if (p.term == TK_LANE)
        terminal_cols<EP_SV>(s, LaneMap{h->lane_np, p.ncols, JQ_LANE_ROWS(h->lane_np) - 1}, 1, h->d_state, 0, h->d_vtr_l, h->d_vti_l, h->d_dvr_l, h->d_dvi_l,
                             sv_mode, h->N, nsamples, leak_scale, h->d_res);
    else
        hipLaunchKernelGGL(k_terminal, dim3(p.nslabs), dim3(64), 0, s, h->d_state, h->state_stride, h->d_vtr, h->d_vti, h->KT,
                           h->N, h->sps, nsamples, leak_scale, h->d_res, h->d_dvr, h->d_dvi, sv_mode);

    // ---- backward sweep(s) ---------------------------------------------------------------------
    // one sweep per (control group, forcing): the forced adjoint gives the total gradient, the unforced one (objFuncType != 1)
    // the infidelity gradient; every sweep restarts from the state the forward sweep and the terminal kernel left behind
    unsigned long long cq3_fault = 0;
    if (adjoint) {
        const int nsweeps = (two_pass ? 2 : 1) * ngroups;
        if (nsweeps > 1)
            HIPCHK(h, hipMemcpyAsync(h->d_state_save, h->d_state, p.state_doubles * sizeof(double),
                                     hipMemcpyDeviceToDevice, s));
        for (int sweep = 0; sweep < nsweeps; ++sweep) {
            const int pass = sweep / ngroups, grp = sweep % ngroups;
            const int q0 = ctrl_gstart(h->Nc, grp), ng = ctrl_gstart(h->Nc, grp + 1) - q0;
            const int ntr_g = ng * JQ_NTR;
            if (sweep > 0)
                HIPCHK(h, hipMemcpyAsync(h->d_state, h->d_state_save, p.state_doubles * sizeof(double),
                                         hipMemcpyDeviceToDevice, s));
            a.Ncoupled = ng;
            a.cimg = p.cimg + (size_t)2 * q0 * p.stride;
            long long trace_tiles = 0;
            for (int q = 0; q < JQ_MAXNC; ++q) {
                a.bw_trace[q] = q < ng ? h->bw_trace[q0 + q] : 0;
                if (q < ng) trace_tiles += plan_trace_tiles(h, p, q0 + q);
            }
            for (int n0 = 0; n0 < h->nsteps; n0 += p.cs) {
                const int nc = std::min(p.cs, h->nsteps - n0);
                const int ntp = 2 * nc + 1;
                if (sampled_grp)
                    hipLaunchKernelGGL(k_ctrl_samples_members, dim3((ntp + 127) / 128, nvec), dim3(128), 0, s, h->d_pcof, tstride, nt, 2 * (h->nsteps - n0), -1, ntp,
                                       h->Nc, d_mix, h->d_pq);
                else if (sampled)
                    hipLaunchKernelGGL(k_ctrl_samples, dim3((ntp + 127) / 128), dim3(128), 0, s, h->d_pcof, nt, 2 * (h->nsteps - n0), -1, ntp, h->Nc, h->d_pq);
                else
                    hipLaunchKernelGGL(k_ctrl, dim3((ntp + 127) / 128, nvec), dim3(128), 0, s, sp, h->d_tb, n0, ntp, -dt, h->d_pq, d_mix, d_pqraw);
                hipLaunchKernelGGL(k_stream, dim3((unsigned)((p.stride + 255) / 256), ntp, nvec), dim3(256), 0, s, p.himg, h0img,
                                   h0_gstride, h->d_pq, h->Nc, p.stride, -0.5 * dt, h->d_stream, (long long)gstride);
                a.nsteps_chunk = nc; a.step0 = n0; a.first_chunk = (n0 == 0); a.h = -dt; a.forced = (pass == 0);
                a.hist_r = nullptr; a.hist_i = nullptr;
                a.wlr_lds = p.bwd.wlr;
                a.wlr_sc_lds = p.bwd.wsc;
                a.jac_wg_lds = p.bwd.jac;
                a.npro = (n0 == 0) ? ng : 0; a.nslots = h->nslots_bwd;
                pack_backward_schedule(a, p.sched, ng);
                if (cq3) {      // (progress counters of the launch: the 64-double header in front of every quad's ring -- the ring itself is written
                                // before it is read; the error word in front of everything survives until the end of the evaluation, the
                                // arrival counter of the start-up rendezvous behind it is per launch)
                    HIPCHK(h, hipMemset2DAsync(h->d_cq3 + 64, cq3_quad * sizeof(double), 0, 64 * sizeof(double), (size_t)p.nq_pad, s));
                    HIPCHK(h, hipMemsetAsync(h->d_cq3 + 1, 0, 2 * sizeof(double), s));      // (arrival counter, state word of the launch)
                    a.park = h->d_cq3;
                    // rendezvous: about ONE launch duration (2 .. 100 ms; option cq3_rdv_us overrides) in polls of ~ 1.3 us -- an abandoned launch
                    // then costs at most what the launch itself would have; waits after a passed rendezvous: ~ 10 x the launch's expected
                    // duration, at least 50 ms (measured on this handle; before the first launch: 25 us per step, four times the slowest size measured)
                    const double us_step = h->cq3_us_per_step > 0.0 ? h->cq3_us_per_step : 25.0;
                    const double rdv_us = h->opt.has(O_CQ3_RDV_US) ? (double)h->opt.get(O_CQ3_RDV_US) : std::min(100.0e3, std::max(2.0e3, us_step * nc));
                    a.rdv_polls = (int)std::min<double>(2.0e9, std::max(16.0, rdv_us / 1.3));
                    a.wait_polls = (int)std::min<double>(2.0e9, (h->opt.has(O_CQ3_WAIT_MS) ? 1.0e3 * (double)h->opt.get(O_CQ3_WAIT_MS) : std::max(50.0e3, 10.0 * us_step * nc)) / 1.3);
                }
                HIPCHK(h, hipEventRecord(h->ev[evi++], s));
                if (qsplit) {      // (two waves per column quad; its window ring is deeper than the forward kernel's)
                    a.park = h->d_qsplit;
                    a.lds_tab_off = (int)((size_t)(2 * JQ_QS_TPS + 2 * h->NcK) * p.stride * 8);
                    a.batch = -1;
                }
                hipLaunchKernelGGL(p.kbwd, dim3(p.bwd_grid), dim3(ng >= 2 ? p.bwd_block_ng2 : p.bwd_block), p.bwd.total, s, a);
                HIPCHK(h, hipEventRecord(h->ev[evi++], s));
                if (cq3 && sweep == 0 && n0 == 0) {
                    // the first launch of the split says whether its workgroups were resident together: read the error word now instead
                    // of running every other chunk and sweep (each dead wait costs ~ 1.3 s) before the evaluation is repeated anyway
                    unsigned long long e1 = 0;
                    HIPCHK(h, hipMemcpyAsync(&e1, h->d_cq3, sizeof(e1), hipMemcpyDeviceToHost, s));
                    HIPCHK(h, hipStreamSynchronize(s));
                    if (h->opt.on(O_CQ3_FAULT)) e1 = (unsigned long long)h->opt.get(O_CQ3_FAULT);      // (test hook: as if a wait had been abandoned (1) / the rendezvous had failed (3))
                    if (e1) {
                        cq3_fault = e1;
                        break;
                    }
                }
                // (grouped batch: per vector its own trace rows -- p.upg of them, the padding rows of the last slab belong to nobody -- and its own gradient)
                // (control mixes: the rows of the sweep's operators become rows for ALL controls, and the assembly covers all of them)
                const int ntr_R = d_mix ? h->Nc * JQ_NTR : ntr_g;
                hipLaunchKernelGGL(k_trace_reduce, dim3((unsigned)(((long long)nc * ntr_R + 255) / 256), nvec), dim3(256), 0, s,
                                   h->d_traces, G > 0 ? p.upg : p.trace_rows, nc, ntr_g, h->d_R, d_mix, h->Nc, q0);
                if (sampled_grp) {      // per group its record into its own table; with a mix the records are the rows of ALL controls
                    const int gq0 = d_mix ? 0 : q0, gng = d_mix ? h->Nc : ng;
                    hipLaunchKernelGGL(k_gradsamples_grouped, dim3((unsigned)(((long long)ntp * gng * 2 + 255) / 256), nvec), dim3(256), 0, s, h->d_R, nc, -dt,
                                       h->d_grad + (size_t)pass * ncoeff, (long long)2 * ncoeff, nt, 2 * (h->nsteps - n0), h->Nc, gq0, gng);
                } else if (sampled)      // the same records without the basis: one thread per (time point of the chunk, control of the group, p | q)
                    hipLaunchKernelGGL(k_gradsamples, dim3((unsigned)(((long long)ntp * ng * 2 + 255) / 256)), dim3(256), 0, s, h->d_R, nc, -dt,
                                       h->d_grad + (size_t)pass * ncoeff, nt, 2 * (h->nsteps - n0), h->Nc, q0, ng);
                else      // gradbcarrier2! as a scatter: one workgroup per coefficient of the group's controls
                    hipLaunchKernelGGL(k_gradacc, dim3((d_mix ? h->Nc : ng) * 2 * h->Nfreq * D1, nvec), dim3(JQ_GRADACC_THREADS), 0, s, sp, h->d_R, h->d_tb, n0, nc, -dt,
                                       h->d_grad + (size_t)pass * ncoeff, d_mix ? 0 : q0, d_mix ? h->Nc : ng, (long long)2 * ncoeff);
                mfma += (long long)p.nslabs * nc * (2 * (8 + 2 * h->m) * p.tiles + 4 * trace_tiles);
                if (n0 == 0) mfma += (long long)p.nslabs * trace_tiles;
            }
            if (cq3_fault) break;
        }
    }
    HIPCHK(h, hipGetLastError());
    if (ens && !cq3_fault)      // the members' finished tables, weighted, onto the ensemble's pair in member order
        for (int pass = 0; pass < (two_pass ? 2 : 1); ++pass)
            hipLaunchKernelGGL(k_gradsamples_wsum, dim3((unsigned)((ncoeff + 255) / 256)), dim3(256), 0, s, h->d_grad + (size_t)pass * ncoeff, (long long)2 * ncoeff, nvec,
                               h->d_wq, d_ens + (size_t)pass * ncoeff, (long long)ncoeff);
    if (d_packed) {
        if (wgt) {
            if ((rc = dev_grow(h, &h->d_wq, &h->cap_wq, (size_t)nsamples))) return rc;
            HIPCHK(h, hipMemcpyAsync(h->d_wq, wgt, (size_t)nsamples * sizeof(double), hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(k_pack, dim3(1), dim3(256), 0, s, h->d_res, wgt ? h->d_wq : nullptr, nsamples, h->d_grad, ncoeff,
                           adjoint ? 1 : 0, two_pass ? 1 : 0, d_packed);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(h->ev[1], s));

    // ---- outputs -------------------------------------------------------------------------------
    out->res.resize((size_t)nsamples * 4);
    HIPCHK(h, hipMemcpyAsync(out->res.data(), h->d_res, out->res.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    if (ens) {      // (the ensemble's pair alone)
        out->grad0.resize((size_t)ncoeff);
        HIPCHK(h, hipMemcpyAsync(out->grad0.data(), d_ens, (size_t)ncoeff * sizeof(double), hipMemcpyDeviceToHost, s));
        if (two_pass) {
            out->grad1.resize((size_t)ncoeff);
            HIPCHK(h, hipMemcpyAsync(out->grad1.data(), d_ens + ncoeff, (size_t)ncoeff * sizeof(double), hipMemcpyDeviceToHost, s));
        }
    } else if (adjoint) {      // (grouped batch: [vector][ncoeff] each)
        out->grad0.resize((size_t)nvec * ncoeff);
        if (two_pass) out->grad1.resize((size_t)nvec * ncoeff);
        for (int g = 0; g < nvec; ++g) {
            HIPCHK(h, hipMemcpyAsync(out->grad0.data() + (size_t)g * ncoeff, h->d_grad + (size_t)g * 2 * ncoeff, (size_t)ncoeff * sizeof(double), hipMemcpyDeviceToHost, s));
            if (two_pass)
                HIPCHK(h, hipMemcpyAsync(out->grad1.data() + (size_t)g * ncoeff, h->d_grad + (size_t)g * 2 * ncoeff + ncoeff, (size_t)ncoeff * sizeof(double),
                                         hipMemcpyDeviceToHost, s));
        }
    }
    unsigned long long cq3_err = cq3_fault;
    if (cq3 && !cq3_fault) HIPCHK(h, hipMemcpyAsync(&cq3_err, h->d_cq3, sizeof(cq3_err), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (cq3 && debug_timing()) {      // development aid: progress counters, error word and XCC ids (+ 1) of the first quads
        std::vector<unsigned long long> hw((size_t)64 + 2 * cq3_quad);
        HIPCHK(h, hipMemcpy(hw.data(), h->d_cq3, hw.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int qd = 0; qd < 2; ++qd) {
            const unsigned long long* q = hw.data() + 64 + (size_t)qd * cq3_quad;
            fprintf(stderr, "jq cq3 quad %d: steps %llu %llu %llu, error %llu (launch %llu), xcc %llu %llu %llu\n", qd, q[0], q[8], q[16], q[24], hw[0], q[32], q[33], q[34]);
        }
    }
    if (cq3 && h->opt.on(O_CQ3_FAULT)) cq3_err = (unsigned long long)h->opt.get(O_CQ3_FAULT);
    if (cq3_err == 3) {
        // the launch was abandoned at its start-up rendezvous: not every workgroup became resident within cq3_rdv_us -- another process
        // holds the compute units.  Nothing is wrong with the handle: repeat on the one-workgroup kernel (milliseconds lost), stay off
        // the split for a few evaluations (2, 4, ... 64 while it keeps happening), never for good.
        ++h->cq3_busy;
        h->cq3_busy_streak = std::min(h->cq3_busy_streak + 1, 5);
        h->cq3_skip = 2 << h->cq3_busy_streak;      // (the repeat below counts as one)
        if (debug_timing()) fprintf(stderr, "jq: split latency kernel abandoned at its start-up rendezvous (GPU busy) -- evaluated again on one workgroup per quad\n");
        return JQ_ERETRY_INTERNAL;
    }
    if (cq3_err) {      // a wait between the three workgroups of a quad was abandoned (1), or they ran on different XCDs (2): the results are void
        ++h->cq3_faults;
        if (cq3_err == 2) ++h->cq3_faults_xcd;
        h->cq3_skip = 2 << std::min(h->cq3_faults, 10);      // (4, 8, 16, ... evaluations; the repeat below counts as one)
        if (h->cq3_faults >= JQ_CQ3_MAX_FAULTS) h->cq3_off = true;
        if (debug_timing()) fprintf(stderr, "jq: k_backward_cq3 reported %llu -- evaluated again with k_backward_cq\n", cq3_err);
        return JQ_ERETRY_INTERNAL;
    }

    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->timing.ms_total = ms;
    double fwd = 0.0, bwd = 0.0;
    const size_t nfwd = (size_t)nchunks;
    const bool show = debug_timing();      // development aid: every propagator launch on stderr
    for (size_t i = 2, k = 0; i + 1 < evi; i += 2, ++k) {
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        if (show) fprintf(stderr, "jq launch %zu (%s): %.3f ms\n", k, k < (size_t)nchunks ? "forward" : "backward", ms);
        if (k < nfwd)
            fwd += ms;
        else
            bwd += ms;
    }
    if (cq3 && bwd > 0.0) {
        h->cq3_us_per_step = 1.0e3 * bwd / ((double)h->nsteps * (two_pass ? 2 : 1) * ngroups);
        h->cq3_busy_streak = 0;
    }
    h->timing.ms_forward = fwd;
    h->timing.ms_backward = bwd;
    h->timing.ms_propagate = fwd + bwd;
    h->timing.ms_generate = h->timing.ms_total - (fwd + bwd);
    h->timing.n_forward_launches = (long long)nfwd;
    h->timing.n_backward_launches = (long long)((evi - 2) / 2 - nfwd);
    h->timing.mfma_executed = p.mfma_div ? mfma / p.mfma_div : 0;
    h->timing.mfma_backward = p.mfma_div ? (mfma - mfma_fwd) / p.mfma_div : 0;
    h->timing.svts = (long long)nsamples * h->N * h->nsteps;
    h->timing.kernel_family = p.family;
    h->timing.kernel_size = p.kernel_size;
    h->timing.kernel_band = p.kernel_band;
    h->timing.kernel_variant = p.kernel_variant;
    h->last_kernels = p.sel;
    h->timing.ms_allreduce = 0.0;
    h->timing.ms_shard_min = h->timing.ms_shard_max = h->timing.ms_total;
    if (sampled) h->sc_nt = nt, h->sc_nodes = nsamples, h->sc_chunk = p.cs;
    return JQ_OK;
}

