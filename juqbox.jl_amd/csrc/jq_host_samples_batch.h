// jq_host_samples_batch.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// sample tables in batches and over member ensembles -- jq_traceobjgrad_samples_batch, jq_traceobjgrad_samples_members and
// jq_eval_f_g_grad_samples_members.  The driver is pcof_batch's (juqbox_hip.hip) with "control vector" read as "sample table": the launch
// size is pcof_batch_per_launch's, a grouped launch hands run_eval a request with samples AND groups (and, for members, drifts / mix), every
// other route runs the groups one after the other inside the call.  The time loops are the ones of the spline calls; what knows tables is
// k_ctrl_samples_members, k_gradsamples_grouped and k_gradsamples_wsum (jq_aux_kernels.h).

// n groups over sample tables on this (single-device) handle.  tables: n of them (drifts == mixes == NULL), or the ONE the members share
// (drifts: [Ntot x Ntot x n] that drifts_prepare has tested, NULL: the handle's; mixes: [Nc x Nc x n], NULL: identity).
// put(i, res, g0, g1): column i of the caller's outputs from its record and its gradients.  ens_w (NULL: none): the members' weights of
// jq_eval_f_g_grad_samples_members -- put gets no gradients then, *ens receives the weighted sums of the forced (grad0) and the unforced
// (grad1, objFuncType != 1) sample gradients, which every launch continues on the device from where the launch before it stopped.
template <typename Put>
static int samples_batch(jq_handle* h, const double* tables, int nt, int n, const double* drifts, const double* mixes, const double* ens_w, bool adjoint,
                         EvalOut* ens, Put&& put)
{
    int spg = 1, family = -1;
    const char* why = "";
    const int per = pcof_batch_per_launch(h, n, 1, adjoint, &spg, &family, &why);
    const int step = per > 0 ? per : 1;
    const bool members = drifts || mixes;
    const int len = 2 * h->Nc * nt;
    jq_handle::SampledBatch& sb = h->sampled_batch;
    sb.kind = members ? "members" : "tables", sb.mode = per > 0 ? "grouped" : "sequential", sb.why = why, sb.per_launch = step;
    sb.drifts = drifts != nullptr, sb.mix = mixes != nullptr, sb.nt = nt;
    EvalRequest rq;
    rq.ncoeff = len, rq.adjoint = adjoint;
    if (per > 0) rq.spg = spg, rq.nodes = 1;
    const size_t nn = (size_t)h->Ntot * h->Ntot, ncnc = (size_t)h->Nc * h->Nc;
    const bool swap = drifts && per == 0;
    const std::vector<double> own = swap ? h->Hconst : std::vector<double>();
    struct Restore {      // (also when a member's evaluation fails)
        jq_handle* h;
        const std::vector<double>* own;
        ~Restore() { if (own) (void)apply_hconst(h, own->data()); }
    } restore{h, swap ? &own : nullptr};
    jq_timing tsum = {};
    const bool weighted = ens_w && adjoint;
    for (int i0 = 0; i0 < n; i0 += step) {
        const int G = std::min(step, n - i0);      // (sequential: one group, spg == 1)
        rq.samples = members ? tables : tables + (size_t)len * i0;
        if (mixes) rq.mix = mixes + ncnc * i0;
        if (per > 0) rq.groups = G, rq.nsamples = G * spg;
        if (drifts && per > 0) rq.drifts = drifts + nn * i0;
        if (swap)
            if (int rc = apply_hconst(h, drifts + nn * i0)) return rc;
        if (weighted) {
            rq.ens_w = ens_w + i0;
            rq.ens_acc0 = i0 > 0 ? ens->grad0.data() : nullptr;
            rq.ens_acc1 = (i0 > 0 && !ens->grad1.empty()) ? ens->grad1.data() : nullptr;
        }
        EvalOut o;
        if (int rc = run_eval(h, rq, &o)) return rc;
        for (int g = 0; g < G; ++g)
            put(i0 + g, o.res.data() + (size_t)4 * g * spg, (adjoint && !weighted) ? o.grad0.data() + (size_t)len * g : nullptr,
                (adjoint && !weighted && h->objFuncType != 1) ? o.grad1.data() + (size_t)len * g : nullptr);
        if (weighted) ens->grad0.swap(o.grad0), ens->grad1.swap(o.grad1);
        timing_add(h->timing, tsum);      // (this launch's record + the sums so far)
        tsum = h->timing;
    }
    h->timing.ms_shard_min = h->timing.ms_shard_max = h->timing.ms_total;
    sb.family = h->timing.kernel_family, sb.chunk = h->sc_chunk;
    return JQ_OK;
}

extern "C" int jq_traceobjgrad_samples_batch(jq_handle* h, const double* pqs, int32_t nt, int32_t ntab, int32_t evaladjoint, double* out4,
                                             double* totalgrad, double* infidelgrad, double* leakgrad)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_traceobjgrad_samples_batch", [&]() -> int {
        if (!pqs || !out4) return fail(h, JQ_EINVAL, "jq_traceobjgrad_samples_batch: NULL pointer");
        if (evaladjoint && (!totalgrad || !infidelgrad || !leakgrad))
            return fail(h, JQ_EINVAL, "jq_traceobjgrad_samples_batch: gradient outputs are required when evaladjoint != 0");
        if (ntab < 1) return fail(h, JQ_EINVAL, "jq_traceobjgrad_samples_batch: ntab must be >= 1");
        JQ_ON_FIRST(h, jq_traceobjgrad_samples_batch(s0_, pqs, nt, ntab, evaladjoint, out4, totalgrad, infidelgrad, leakgrad))
        if (int rc = samples_refuse(h, "jq_traceobjgrad_samples_batch")) return rc;
        const size_t len = (size_t)2 * h->Nc * (nt > 0 ? nt : 0);
        for (int i = 0; i < ntab; ++i)      // (every table, before anything is written)
            if (int rc = samples_args(h, "jq_traceobjgrad_samples_batch", pqs + len * i, nt)) return rc;
        return samples_batch(h, pqs, nt, ntab, nullptr, nullptr, nullptr, evaladjoint != 0, nullptr, [&](int i, const double* res, const double* g0, const double* g1) {
            out_record(out4 + (size_t)4 * i, res);
            if (evaladjoint) out_grads(h, (int)len, g0, g1, totalgrad + len * i, infidelgrad + len * i, leakgrad + len * i);
        });
    });
}

// the checks the two member calls share, in the order: pointers and counts, the table, the handle's controls -- and only then the member
// drifts, whose test may plan the handle again (drifts_prepare)
static int samples_members_args(jq_handle* h, const char* who, const double* pq, int nt, const double* Hconsts, const double* ctrl_mix, int nmember, const void* out)
{
    if (int rc = members_args(h, who, false, pq, Hconsts, ctrl_mix, nmember, out)) return rc;
    if (int rc = samples_refuse(h, who)) return rc;
    if (int rc = samples_args(h, who, pq, nt)) return rc;
    if (Hconsts)
        if (int rc = drifts_prepare(h, Hconsts, nmember)) return rc;
    return JQ_OK;
}

extern "C" int jq_traceobjgrad_samples_members(jq_handle* h, const double* pq, int32_t nt, const double* Hconsts, const double* ctrl_mix, int32_t nmember,
                                               int32_t evaladjoint, double* out4, double* totalgrad, double* infidelgrad, double* leakgrad)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_traceobjgrad_samples_members", [&]() -> int {
        const char* who = "jq_traceobjgrad_samples_members";
        if (evaladjoint && (!totalgrad || !infidelgrad || !leakgrad))
            return fail(h, JQ_EINVAL, "jq_traceobjgrad_samples_members: gradient outputs are required when evaladjoint != 0");
        if (!pq || !out4) return fail(h, JQ_EINVAL, "jq_traceobjgrad_samples_members: NULL pointer");
        JQ_ON_FIRST(h, jq_traceobjgrad_samples_members(s0_, pq, nt, Hconsts, ctrl_mix, nmember, evaladjoint, out4, totalgrad, infidelgrad, leakgrad))
        if (int rc = samples_members_args(h, who, pq, nt, Hconsts, ctrl_mix, nmember, out4)) return rc;
        const size_t len = (size_t)2 * h->Nc * nt;
        return samples_batch(h, pq, nt, nmember, Hconsts, ctrl_mix, nullptr, evaladjoint != 0, nullptr, [&](int i, const double* res, const double* g0, const double* g1) {
            out_record(out4 + (size_t)4 * i, res);
            if (evaladjoint) out_grads(h, (int)len, g0, g1, totalgrad + len * i, infidelgrad + len * i, leakgrad + len * i);
        });
    });
}

// the weighted sums of eval_f_g_grad! (src/ipopt_interface.jl:48-59) over the members: the two objective parts on the host in member order
// (eval_f_g_grad_members' sums), the two gradients on the device
extern "C" int jq_eval_f_g_grad_samples_members(jq_handle* h, const double* pq, int32_t nt, const double* Hconsts, const double* ctrl_mix, const double* weights,
                                                int32_t nmember, int32_t compute_adjoint, double* out2, double* infid_grad, double* leak_grad, double* member_out)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_eval_f_g_grad_samples_members", [&]() -> int {
        const char* who = "jq_eval_f_g_grad_samples_members";
        if (!pq || !weights || !out2) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_samples_members: NULL pointer");
        if (compute_adjoint && (!infid_grad || !leak_grad))
            return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_samples_members: gradient outputs are required when compute_adjoint != 0");
        JQ_ON_FIRST(h, jq_eval_f_g_grad_samples_members(s0_, pq, nt, Hconsts, ctrl_mix, weights, nmember, compute_adjoint, out2, infid_grad, leak_grad, member_out))
        if (int rc = samples_members_args(h, who, pq, nt, Hconsts, ctrl_mix, nmember, out2)) return rc;
        const size_t len = (size_t)2 * h->Nc * nt;
        std::vector<double> rec((size_t)4 * nmember);
        EvalOut ens;
        const int rc = samples_batch(h, pq, nt, nmember, Hconsts, ctrl_mix, weights, compute_adjoint != 0, &ens,
                                     [&](int i, const double* res, const double*, const double*) { out_record(rec.data() + (size_t)4 * i, res); });
        if (rc) return rc;
        double inf = 0.0, leak = 0.0;
        for (int i = 0; i < nmember; ++i) {
            inf += rec[(size_t)4 * i + 1] * weights[i];      // (primaryobjf, secondaryobjf of the member's record)
            leak += rec[(size_t)4 * i + 2] * weights[i];
        }
        out2[0] = inf, out2[1] = leak;
        if (member_out) std::copy(rec.begin(), rec.end(), member_out);
        if (compute_adjoint) out_grads(h, (int)len, ens.grad0.data(), ens.grad1.data(), nullptr, infid_grad, leak_grad);
        return JQ_OK;
    });
}
