// jq_host_info.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// options of a live handle, plan and timing introspection.
extern "C" int jq_set_option(jq_handle* h, const char* name, int64_t value)
{
    if (!h) return JQ_EINVAL;
    if (!name) return fail(h, JQ_EINVAL, "jq_set_option: NULL name");
    const int o = JqOptions::find(name, strlen(name));
    if (o < 0) return fail(h, JQ_EINVAL, (std::string("jq_set_option: unknown option '") + name + "'").c_str());
    const long long v = (value == JQ_OPTION_DEFAULT) ? JQ_OPT_UNSET : (long long)value;
    if (!h->subs.empty()) {
        // validate first (on a copy), apply to the sub-handles, commit h->opt only when every one of them accepted the value: after a
        // refusal jq_get_option and jq_plan_info report what the sub-handles have
        if (o == O_MULTI_SAME_DEVICE) return fail(h, JQ_EINVAL, "jq_set_option: multi_same_device is an option of jq_create_multi_opts");
        JqOptions want = h->opt;
        std::string err;
        if (!want.set(o, v, &err)) return fail(h, JQ_EUNSUPPORTED, ("jq_set_option: " + err).c_str());
        const long long old = h->opt.v[o];
        const int64_t old_value = (old == JQ_OPT_UNSET) ? JQ_OPTION_DEFAULT : (int64_t)old;
        const int rc = multi_forall(h, [&](jq_handle* sub) { return jq_set_option(sub, name, value); });
        if (rc != JQ_OK) {      // nothing half-applied: the sub-handles that took the value get the old one back
            std::string why = h->err;
            // (a restore that fails itself -- a re-plan back that runs out of memory -- leaves that sub-handle on the new value: said in the message)
            if (multi_forall(h, [&](jq_handle* sub) { return jq_set_option(sub, name, old_value); }) != JQ_OK)
                why += " (and restoring the old value on the devices failed: " + h->err + "; destroy this handle)";
            h->err = why;
            return rc;
        }
        h->opt = want;
        return JQ_OK;
    }
    const long long old = h->opt.v[o];
    if (old == v) return JQ_OK;
    std::string err;
    if (!h->opt.set(o, v, &err)) return fail(h, JQ_EUNSUPPORTED, ("jq_set_option: " + err).c_str());
    if (g_jq_opt[o].flags & JQ_OPT_PLAN) {      // shapes the plan: plan again from the handle's own copy of the problem
        HIPCHK(h, hipSetDevice(h->device));
        const std::vector<double> H0 = h->Hconst;
        const int rc = replan(h, H0.data());
        if (rc != JQ_OK) {
            h->opt.v[o] = old;
            return rc;
        }
        h->replanned = false;      // (an option change is not a drift outside the planned structure)
        return JQ_OK;
    }
    if (h->emb) h->emb->opt = h->opt;
    return JQ_OK;
}

extern "C" int jq_get_option(const jq_handle* h, const char* name, int64_t* value)
{
    if (!h || !name || !value) return JQ_EINVAL;
    const int o = JqOptions::find(name, strlen(name));
    if (o < 0) return JQ_EINVAL;
    const long long v = h->opt.get(o);
    *value = (v == JQ_OPT_UNSET) ? JQ_OPTION_DEFAULT : (int64_t)v;
    return JQ_OK;
}

// ranks of the RCCL communicator behind a multi-device handle (ncclCommCount of its first communicator): what the first real
// multi-GPU run prints to show that RCCL saw every device.  0: no communicator (single-device handle, same-device test mode).
extern "C" int jq_rccl_world_size(const jq_handle* h)
{
    if (!h || h->comms.empty() || !h->comms[0] || !g_rccl.CommCount) return 0;
    int n = 0;
    if (g_rccl.CommCount(h->comms[0], &n) != ncclSuccess) return -1;
    return n;
}

extern "C" int jq_plan_info(const jq_handle* hh, char* buf, int32_t buflen)
{
    if (!hh || (!buf && buflen > 0) || buflen < 0) return JQ_EINVAL;
    const jq_handle* h = hh->subs.empty() ? hh : hh->subs[0];
    std::string o = "{";
    auto kv = [&](const char* k, const std::string& v, bool quote = false) {
        if (o.size() > 1) o += ", ";
        o += std::string("\"") + k + "\": " + (quote ? "\"" + v + "\"" : v);
    };
    auto num = [](long long v) { return std::to_string(v); };
    kv("devices", num(hh->subs.empty() ? 1 : (long long)hh->subs.size()));
    kv("Ntot", num(h->Ntot));
    kv("N", num(h->N));
    kv("controls", num(h->Nc));
    kv("control_groups", num(ctrl_ngroups(h->Nc)));
    kv("tile_rows", num(h->NT));
    kv("compute_units", num(h->num_cu));
    const char* structure = h->big ? (h->BWc == 15 ? "dense" : "band") : h->BW == JQ_BW_T4 ? "t4" : h->BW == JQ_BW_OD ? "od" : h->BW == h->NT - 1 ? "dense" : "band";
    kv("structure", structure, true);
    kv("block_band", num(h->big ? h->BWc : h->BW));
    kv("embedded_twin_Ntot", num(h->emb ? h->emb->Ntot : 0));
    kv("integrator", h->integrator == 2 ? "implicit_midpoint" : "stormer_verlet", true);
    kv("linear_solver", h->solver_id == 2 ? "jacobi" : "neumann", true);
    kv("sv_type", num(h->sv_type));
    kv("neumann_terms_or_max_iter", num(h->integrator == 2 ? h->imr_max_iter : h->m));
    kv("chunk_steps", num(h->chunk_steps));
    kv("replanned", h->replanned ? "true" : "false");
    // uniform S images (4 x 4 x n plans; the embedded twin's where it serves the batches) and the option that lets the three-slab quad-layout
    // kernels use the compact S operand then
    kv("s_uniform", (h->emb ? h->emb : h)->s_uniform ? "true" : "false");
    kv("s_compact", num(hh->opt.get(O_S_COMPACT)));
    // kernel families in the order plan_batch considers them for a Stormer-Verlet / Neumann batch (the embedded twin, if any, serves
    // the batches beyond the row-lane / lane range with ITS plan)
    std::string fam = "[";
    auto add = [&](int id, const char* name, const char* unit, long long mx) {
        if (fam.size() > 1) fam += ", ";
        fam += std::string("{\"family\": ") + std::to_string(id) + ", \"name\": \"" + name + "\", \"max_" + unit + "\": " + std::to_string(mx) + "}";
    };
    const jq_handle* t = h->emb ? h->emb : h;
    if (h->rl_npj > 0) add(3, "row-lane (VALU, lane per (row, column); backward sweep on three or four waves, implicit midpoint: two)", "columns", h->rl_max_cols);
    if (h->lane_np > 0) add(2, "lane (VALU, lane per column)", "columns", h->lane_max_cols);
    if (t->cq_max_quads > 0) add(8, "cooperative quad (one 16-row block per wave)", "quads", t->cq_max_quads);
    if (t->dq_max_quads > 0) add(8, "cooperative quad, dense blocks (17 .. 32 levels without the 4 x 4 x n structure; Neumann, Diagonal weights)", "quads", t->dq_max_quads);
    if (t->quad_max_slabs > 0) add(6, "quad layout (four columns per wave; 1 / 2 / 3 slabs per workgroup by round count)", "slabs", t->quad_max_slabs);
    if (t->coop_ok && t->NT >= 2) add(1, "cooperative (tile row per wave)", "slabs", t->coop_max_slabs);
    if (!t->big) add(0, "slab (wave per 16-column slab)", "slabs", 1LL << 30);
    fam += "]";
    kv("families", fam);
    {   // the objects this handle's kernels come from, as the build manifest records them (register form, registers, scratch)
        const std::string man(jq_build_manifest);
        std::vector<std::string> tags;
        auto tag = [&](const char* prefix, int a, int b) {
            char buf[32];
            if (b >= 0) snprintf(buf, sizeof buf, "%s_%d_%d", prefix, a, b);
            else snprintf(buf, sizeof buf, "%s_%d", prefix, a);
            tags.push_back(buf);
        };
        for (const jq_handle* x : {h, (const jq_handle*)h->emb}) {
            if (!x) continue;
            if (x->BW == JQ_BW_T4) {
                for (const char* pre : {"k", "s", "p", "u", "w", "q", "v"}) tag(pre, x->NT, JQ_BW_T4Q);
                tag("k", x->NT, JQ_BW_T4);
                tag("j", x->NT, JQ_BW_T4);
            } else if (!x->big) {
                tag("k", x->NT, x->BW);
                tag("j", x->NT, x->BW);
            }
            if (x->mat_elems_c > 0) tag("c", x->NT, x->BWc), tag("i", x->NT, x->BWc);
            if (x->rl_npj > 0) tag("r", x->rl_npj, -1), tag("m", x->rl_npj, -1);
            if (x->lane_np > 0) tag("l", x->lane_np, -1);
        }
        std::string objs = "{";
        for (const std::string& t : tags) {
            const std::string key = "\"" + t + "\": {";
            const size_t at = man.find(key);
            if (at == std::string::npos) continue;
            const size_t end = man.find('}', at);
            if (end == std::string::npos) continue;
            if (objs.size() > 1) objs += ", ";
            objs += man.substr(at, end - at + 1);
        }
        objs += "}";
        std::string hipcc = "null";      // the compiler the kernel objects came from (build manifest)
        {
            const size_t at = man.find("\"hipcc\": {");
            const size_t end = at == std::string::npos ? at : man.find('}', at);
            if (end != std::string::npos) hipcc = man.substr(at + 9, end - at - 8);
        }
        kv("build", std::string("{\"manifest\": ") + (man.size() > 2 ? "true" : "false") + ", \"hipcc\": " + hipcc + ", \"objects\": " + objs + "}");
    }
    {   // the instantiation the last evaluation ran on, recorded where the select_* functions of jq_host_select.h picked its kernels (null: no evaluation
        // since the handle was created or planned again): the objects of the backward and the forward kernel as csrc/Makefile names them
        // (jq_timing's family / size / band cannot tell k_N_7 from s_N_7, nor a specialised instantiation from the generic one) and the
        // compile-time variant.  The first (larger) part's where a batch was split into two launches; the embedded twin's where it served.
        const KernelSel& k = h->last_kernels;
        auto tf = [](bool v) { return std::string(v ? "true" : "false"); };
        kv("last_kernels", !k.set ? std::string("null")
                                  : std::string("{\"object\": \"") + k.bwd + "\", \"forward_object\": \"" + k.fwd + "\", \"slabs_per_workgroup\": " + num(k.spw) +
                                        ", \"quads_per_workgroup\": " + num(k.qs_qw) + ", \"backward_workgroups\": " + num(k.bwd_wgs) + ", \"uni\": " + tf(k.uni) +
                                        ", \"ord\": " + tf(k.ord) + ", \"sc_forward\": " + tf(k.sc_fwd) + ", \"sc_backward\": " + tf(k.sc_bwd) + ", \"ride\": " + tf(k.ride) +
                                        ", \"modd\": " + tf(k.modd) + ", \"fwd2\": " + tf(k.fwd2) + ", \"wlr\": " + tf(k.wlr) + ", \"imr_two_sets\": " + tf(k.imr_two) + "}");
    }
    kv("full_weight_rank", num(h->wrank));
    kv("options", hh->opt.str(), true);      // the options that are set (jq_create_opts / JQ_OPTIONS / jq_set_option); "" = all defaults
    kv("rccl_selfchecks", num(hh->rccl_checks));      // all-reduces of a multi-device handle verified against the host-order sum
    {   // the three-workgroup latency kernels: what the last batch of the cooperative-quad families decided, and why
        const jq_handle* t2 = h->emb ? h->emb : h;
        const std::string d = t2->cq3_last.empty() ? "no batch of the cooperative-quad families yet" : t2->cq3_last;
        kv("latency_split", std::string("{\"last_decision\": \"") + d + "\", \"faults\": " + num(t2->cq3_faults) + ", \"faults_xcd\": " + num(t2->cq3_faults_xcd) + ", \"abandoned_at_rendezvous\": " + num(t2->cq3_busy) + ", \"cooling_down\": " + num(t2->cq3_skip) +
                                ", \"off\": " + (t2->cq3_off ? "true" : "false") + "}");
    }
    // jq_traceobjgrad_batch / jq_eval_f_g_grad_batch (nodes_per_vector: 1 / its nquad): what the last call did with its control vectors -- "grouped" (one launch for many vectors, each workgroup reading
    // the tile stream of its own) or "sequential" (the single evaluation per vector), and why
    kv("pcof_batch", std::string("{\"mode\": \"") + (h->pb_mode.empty() ? "none yet" : h->pb_mode) + "\", \"family\": " + num(h->pb_family) + ", \"vectors_per_launch\": " + num(h->pb_per_launch) +
                         ", \"nodes_per_vector\": " + num(h->pb_nodes) + ", \"reason\": \"" + h->pb_why + "\"}");
    // jq_traceobjgrad_drifts / jq_eval_f_g_grad_drifts: what the last call did with its members -- "grouped" (every workgroup reads the tile
    // stream of its own member's drift) or "sequential" (the handle's operator images swapped per member for the single evaluation), and why
    kv("drift_batch", std::string("{\"mode\": \"") + (h->db_mode.empty() ? "none yet" : h->db_mode) + "\", \"family\": " + num(h->db_family) + ", \"members_per_launch\": " + num(h->db_per_launch) +
                          ", \"reason\": \"" + h->db_why + "\"}");
    // the last member ensemble of any kind (jq_traceobjgrad_members / jq_eval_f_g_grad_members and the two drifts calls): the fields of
    // "drift_batch", and what differed between its members -- their drifts, their control mixes
    kv("member_batch", std::string("{\"mode\": \"") + (h->mb_mode.empty() ? "none yet" : h->mb_mode) + "\", \"family\": " + num(h->mb_family) + ", \"members_per_launch\": " + num(h->mb_per_launch) +
                           ", \"reason\": \"" + h->mb_why + "\", \"drifts\": " + (h->mb_drifts ? "true" : "false") + ", \"ctrl_mix\": " + (h->mb_mix ? "true" : "false") + "}");
    // jq_traceobj_jvp (after a call): directions one launch carried next to the primal stream, steps per chunk, launches' rounds
    if (h->jvp_rounds > 0)
        kv("jvp", std::string("{\"directions_per_launch\": ") + num(h->jvp_per_launch) + ", \"chunk_steps\": " + num(h->jvp_chunk) + ", \"rounds\": " + num(h->jvp_rounds) + "}");
    // jq_traceobjgrad_hvp (after a call): the same three of its launches, forward and backward
    if (h->hvp_rounds > 0)
        kv("hvp", std::string("{\"directions_per_launch\": ") + num(h->hvp_per_launch) + ", \"chunk_steps\": " + num(h->hvp_chunk) + ", \"rounds\": " + num(h->hvp_rounds) + "}");
    // jq_eval_f_g_grad_hvp (after a call): the route its nodes took and the same three
    if (h->ens_hvp_route > 0)
        kv("ens_hvp", std::string("{\"route\": \"") + (h->ens_hvp_route == 1 ? "lane" : h->ens_hvp_route == 3 ? "rowlane" : h->ens_hvp_route == 4 ? "quad" : "sequential") + "\", \"directions_per_launch\": " + num(h->ens_hvp_per_launch) +
                          ", \"chunk_steps\": " + num(h->ens_hvp_chunk) + ", \"rounds\": " + num(h->ens_hvp_rounds) + "}");
    // jq_eval_f_g_grad_drifts_hvp (after a call): the route its members took, members and directions per launch, chunk length, launches'
    // rounds (direction rounds x member rounds; sequential: one member per launch, the rounds of all members)
    if (h->drift_hvp_route > 0)
        kv("drift_hvp", std::string("{\"route\": \"") + (h->drift_hvp_route == 1 ? "lane" : h->drift_hvp_route == 3 ? "rowlane" : h->drift_hvp_route == 4 ? "quad" : "sequential") + "\", \"members_per_launch\": " + num(h->drift_hvp_members) +
                          ", \"directions_per_launch\": " + num(h->drift_hvp_per_launch) + ", \"chunk_steps\": " + num(h->drift_hvp_chunk) + ", \"rounds\": " + num(h->drift_hvp_rounds) + "}");
    // jq_eval_f_g_grad_members_hvp (after a call): the fields of "drift_hvp", and what differed between its members -- their drifts, their
    // control mixes (with mixes a member brings 1 + directions_per_launch streams into a launch)
    if (h->member_hvp.route > 0) {
        const jq_handle::MemberHvp& m = h->member_hvp;
        kv("member_hvp", std::string("{\"route\": \"") + (m.route == 1 ? "lane" : m.route == 3 ? "rowlane" : m.route == 4 ? "quad" : "sequential") + "\", \"members_per_launch\": " + num(m.members) +
                           ", \"directions_per_launch\": " + num(m.per_launch) + ", \"chunk_steps\": " + num(m.chunk) + ", \"rounds\": " + num(m.rounds) + ", \"drifts\": " +
                           (m.drifts ? "true" : "false") + ", \"ctrl_mix\": " + (m.mix ? "true" : "false") + "}");
    }
    // jq_traceobjgrad_samples / jq_eval_f_g_grad_samples (after a call): time points of the sample table, nodes, steps per chunk
    if (h->sc_nt > 0)
        kv("sampled_controls", std::string("{\"time_points\": ") + num(h->sc_nt) + ", \"nodes\": " + num(h->sc_nodes) + ", \"chunk_steps\": " + num(h->sc_chunk) + "}");
    // jq_eval_f_g_grad_samples_hvp (after a call): the route its nodes took, the three of "ens_hvp", time points of the tables, nodes
    if (h->sampled_hvp.route > 0) {
        const jq_handle::SampledHvp& m = h->sampled_hvp;
        kv("sampled_hvp", std::string("{\"route\": \"") + (m.route == 1 ? "lane" : m.route == 3 ? "rowlane" : m.route == 4 ? "quad" : "sequential") + "\", \"directions_per_launch\": " + num(m.per_launch) +
                            ", \"chunk_steps\": " + num(m.chunk) + ", \"rounds\": " + num(m.rounds) + ", \"time_points\": " + num(m.nt) + ", \"nodes\": " + num(m.nodes) + "}");
    }
    // jq_traceobjgrad_samples_batch / jq_traceobjgrad_samples_members / jq_eval_f_g_grad_samples_members (after a call): what the groups
    // were, the route ("grouped": the groups share launches; "sequential": one after the other inside the call) and why, the kernel family
    // that ran, groups per launch, what differed between the members, time points of the tables, steps per chunk
    if (!h->sampled_batch.kind.empty()) {
        const jq_handle::SampledBatch& m = h->sampled_batch;
        kv("sampled_batch", std::string("{\"kind\": \"") + m.kind + "\", \"mode\": \"" + m.mode + "\", \"why\": \"" + m.why + "\", \"family\": " + num(m.family) + ", \"per_launch\": " + num(m.per_launch) +
                              ", \"drifts\": " + (m.drifts ? "true" : "false") + ", \"mixes\": " + (m.mix ? "true" : "false") + ", \"time_points\": " + num(m.nt) + ", \"chunk_steps\": " + num(m.chunk) + "}");
    }
    o += "}";
    if (buflen > 0) {
        const size_t n = std::min(o.size(), (size_t)buflen - 1);
        memcpy(buf, o.data(), n);
        buf[n] = 0;
    }
    return (int)o.size();
}

// the structure test behind "s_uniform" on its own (host only, no device): Hanti_ops as jq_problem passes them
extern "C" int jq_s_uniform(const double* Hanti_ops, int32_t Ntot, int32_t Ncoupled)
{
    if (!Hanti_ops || Ntot < 1 || Ntot > 128 || Ntot % 16 != 0 || Ncoupled < 1) return JQ_EINVAL;
    const size_t nn = (size_t)Ntot * Ntot;
    for (int q = 0; q < Ncoupled; ++q)
        if (block_band(Hanti_ops + q * nn, Ntot) > 1 || !t4_structure(Hanti_ops + q * nn, Ntot)) return 0;
    return hanti_s_uniform(Hanti_ops, Ntot, Ntot / 16, Ncoupled) ? 1 : 0;
}

extern "C" int jq_last_timing(const jq_handle* h, jq_timing* t)
{
    if (!h || !t) return JQ_EINVAL;
    *t = h->timing;
    return JQ_OK;
}

