// jq_host_plan.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// plan_batch: how a batch is routed to a kernel family, its variant, geometry and LDS layout (run_eval executes the plan).

// JQ_BW_T4 structure, Stormer-Verlet / Neumann: time of one round of the 4 x 4 x n kernel families relative to a round of the slab
// kernels (4 #CU slabs), measured at cnot3 (scripts/time_staircase.py; round 5, unit 1.7935 s: 0.378 / 0.741 / 1.038 s for #CU / 2 #CU /
// 3 #CU slabs on the quad-layout kernels with 1 / 2 / 3 slabs per workgroup -- one slab per workgroup with its backward sweep on two waves
// per column quad, jq_quad_split_kernels.h; 0.192 s for up to #CU column quads on the cooperative-quad kernels, 0.298 s for up to 2 #CU)
static const double T4_REL[4] = {1.0, 0.2108, 0.413, 0.579};
static const double T4_REL_CQ = 0.107;      // <= #CU column quads
static const double T4_REL_CQ2 = 0.166;     // <= 2 #CU: forward sweep with two quads per workgroup, backward sweep k_backward_qsplit<.., 2>

// Which kernels for nslabs slabs of this structure?  Fewest round units (the returned estimate) wins: the quad
// layout with *spw = 1 / 2 / 3 slabs per workgroup, as far as its backward kernel fits the LDS (quad = false: not considered), or the slab
// kernels (*spw = 0).  NT <= 2 beyond one slab per CU: the slab kernels (4 NT state registers, two workgroups per CU -- 3.5e9 vs 2.2e9
// SVTS/s for cnot2 x 65 536 samples; the quad layout keeps the latency regime).
static double t4_rounds(const jq_handle* h, long long nslabs, bool quad, int* spw)
{
    double best = T4_REL[0] * (double)((nslabs + 4 * h->num_cu - 1) / (4 * h->num_cu));
    *spw = 0;
    if (!quad || (h->NT <= 2 && nslabs > h->num_cu)) return best;
    for (int k = 1; k <= 3; ++k) {
        if (quad_bwd_lds(h, k) > JQ_LDS_MAX) continue;
        const double c = T4_REL[k] * (double)((nslabs + k * h->num_cu - 1) / (k * h->num_cu));
        if (c < best - 1e-9) {
            best = c;
            *spw = k;
        }
    }
    return best;
}

// Estimated time of one batch in the same unit, by the plan plan_batch would choose: cooperative-quad kernels (<= cq_max_quads column
// quads: 0.196 s per round of #CU quads against 1.917 s at cnot3), else t4_rounds.
static double t4_plan_cost(const jq_handle* h, long long nsamples)
{
    const long long nslabs = h->parts > 1 ? nsamples * h->parts : (nsamples + h->sps - 1) / h->sps;
    const long long nquads = (nsamples * h->N + 3) / 4;
    if (h->cq_max_quads > 0 && nquads <= h->cq_max_quads) return nquads <= h->num_cu ? T4_REL_CQ : nquads <= 2 * h->num_cu ? T4_REL_CQ2 : T4_REL_CQ * (double)((nquads + h->num_cu - 1) / h->num_cu);
    int spw;
    return t4_rounds(h, nslabs, nslabs <= h->quad_max_slabs, &spw);
}

// Chunk length of a backward sweep whose per-step trace records have `trace_rows` rows: h->chunk_steps, fewer when the records of a chunk
// ([trace_rows][cs][NcK JQ_NTR] doubles) would exceed option trace_bytes (default 4 GiB).  ONE function for the sweep and for the split
// latency kernels' decision (they need a first chunk longer than their ring).
#define JQ_CQ3_RING 8      // = JQ_CQ3_SLOTS (jq_cq_split_kernels.h, compiled in its own translation units)
static int backward_chunk_steps(const jq_handle* h, size_t trace_rows)
{
    size_t tbudget = (size_t)4 << 30;
    if (h->opt.has(O_TRACE_BYTES) && h->opt.get(O_TRACE_BYTES) > 0) tbudget = (size_t)h->opt.get(O_TRACE_BYTES);
    const long long cst = (long long)(tbudget / (std::max<size_t>(trace_rows, 1) * (size_t)h->NcK * JQ_NTR * sizeof(double)));
    return (int)std::max<long long>(1, std::min<long long>(h->chunk_steps, cst));
}

// Evaluations in flight per device, process-wide.  Every outermost run_eval is counted (enter / leave); an evaluation that wants the
// three-workgroup latency kernels asks for the device EXCLUSIVELY (try_exclusive: granted when it is the only one in flight) and new
// evaluations wait at enter() until it is through (~ 0.15 s at cnot3).  So inside a process a grid whose workgroups wait for each other
// never shares the GPU with another launch of the library (two handles in two threads, the sub-handles of a same-device multi handle ...).
struct DevGate {
    std::mutex m;
    std::condition_variable cv;
    int active = 0;
    bool exclusive = false;
    void enter()
    {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return !exclusive; });
        ++active;
    }
    void leave()
    {
        std::lock_guard<std::mutex> l(m);
        --active;
    }
    bool try_exclusive()      // (the caller is one of the active evaluations)
    {
        std::lock_guard<std::mutex> l(m);
        if (exclusive || active != 1) return false;
        exclusive = true;
        return true;
    }
    void release_exclusive()
    {
        {
            std::lock_guard<std::mutex> l(m);
            exclusive = false;
        }
        cv.notify_all();
    }
};
static DevGate g_gate[64];
static DevGate& dev_gate(int device) { return g_gate[(unsigned)device % 64u]; }
static thread_local int g_eval_depth = 0;      // run_eval calls itself (split batches, the embedded twin): only the outermost call is counted
struct EvalGate {      // an evaluation in flight on the handle's device for the rest of a scope (also when it throws): run_eval and the derivative calls
    DevGate& g;
    const bool outer;
    explicit EvalGate(const jq_handle* h) : g(dev_gate(h->device)), outer(g_eval_depth++ == 0)
    {
        if (outer) g.enter();
    }
    ~EvalGate()
    {
        if (outer) g.leave();
        --g_eval_depth;
    }
    EvalGate(const EvalGate&) = delete;
    EvalGate& operator=(const EvalGate&) = delete;
};
struct GateHold {      // exclusive use of a device for the rest of a scope
    DevGate* g = nullptr;
    bool acquire(DevGate& gate)
    {
        if (gate.try_exclusive()) g = &gate;
        return g != nullptr;
    }
    ~GateHold()
    {
        if (g) g->release_exclusive();
    }
};
#define JQ_RL_ROOM 12          // waves per compute unit the two-wave implicit-midpoint row-lane kernel may ask for (NPJ <= 8)
#define JQ_RL_ROOM_WIDE 4      // ... NPJ = 12, 16

// The kernel families: the codes of jq_timing.kernel_family (include/juqbox_hip.h)
enum KernelFamily { KF_SLAB, KF_COOP, KF_LANE, KF_ROWLANE, KF_ROWLANE_IMR, KF_COOP_IMR, KF_QUAD, KF_QUAD_IMR, KF_CQ, KF_CQ_IMR };
enum StateLayout { SL_SLABS, SL_LANE, SL_ROWLANE };      // state file: slabs of 16-row tiles, one lane per column, one lane per (row, column)
enum TermKernel { TK_SLAB, TK_PARTS, TK_IMR, TK_IMR_PARTS, TK_ROWLANE, TK_ROWLANE_IMR, TK_LANE };
// dynamic LDS of a sweep's launches, and the offsets of the areas behind the layout (-1: not in LDS): low-rank weight table / dots, per-wave
// column scalars of the low-rank terms, Jacobi residual exchange
struct SweepLds { size_t total; int wlr, wsc, jac; };
// operator schedule of a time step, [cooperative][kind (0 K, 1 S, 2 constant image) | time point offset / image index][step]: slab kernels
// Kp05 S05 Kn0 S0 Kn1 S1 Kp05, cooperative kernels Kp05 S05 Kn0 Kn1 S0 S1 Kp05; the backward sweep appends S0
static const int JQ_SCHED[2][2][8] = {{{0, 1, 0, 1, 0, 1, 0, 1}, {1, 1, 0, 0, 2, 2, 1, 0}}, {{0, 1, 0, 0, 1, 1, 0, 1}, {1, 1, 0, 2, 0, 2, 1, 0}}};
struct BatchPlan {
    KernelFamily family;
    StateLayout layout;
    bool coop;                  // cooperative (row-split) operator layout
    // variants: quad-layout slabs per workgroup, split latency kernels' workgroups per quad (3 / 2), k_backward_qsplit quads per workgroup
    // (4 / 2) -- 0: not taken; row-lane backward waves (1 .. 3); implicit-midpoint cooperative quad: 1 / 2 sets of waves, 3 workgroups
    int spw, cq_nr, qs_qw, rl_waves, imr_cq_bwd;
    bool fwd2, dense, parts, hbm, jac_wg, huge;
    prop_kernel_t kfwd, kbwd;   // kernels
    TermKernel term;
    // geometry (prop_nslabs: PropArgs::nslabs -- waves of the row-lane kernels, columns of the lane kernels; bwd_block_ng2: backward
    // sweeps of two or more controls)
    int nslabs, prop_nslabs, cpw, qps, qs_blocks, trace_rows, cs;
    // grouped batch (jq_traceobjgrad_batch, jq_eval_f_g_grad_batch): control vectors of the launch (0: not grouped -- also the answer to a
    // request the chosen family cannot serve) and the units one vector owns = its trace rows (row-lane: waves, cooperative quad: column
    // quads; PropArgs::group_units); wpg: waves that every cpw columns of the row-lane layouts start afresh at (1 unless grouped)
    int groups, upg, wpg;
    long long nwaves_rl, ncols, nq_pad, stride;
    unsigned fwd_grid, fwd_block, bwd_grid, bwd_block, bwd_block_ng2;
    const double *himg, *cimg;
    size_t state_doubles, colinfo_doubles, park_slabs, ws_off;
    const int (*sched)[8];      // JQ_SCHED[coop]
    long long tiles;            // MFMA tiles per operator product (0: VALU kernels)
    int mfma_div;               // MFMA instructions per counted one (JQ_BW_T4: 4x4x4), 0: not counted (implicit midpoint)
    int batch, park_lds;        // LDS layout: PropArgs::batch (operator staging), parking images in LDS, ...
    size_t lds_stage;           // ... bytes of the operator staging (the tables behind it), ...
    SweepLds fwd, bwd;          // ... each sweep's areas behind its layout
    int kernel_size, kernel_band, kernel_variant;      // jq_timing (kernel_family: family)
    KernelSel sel;              // what select_* chose for kfwd / kbwd (jq_plan_info "last_kernels")
};
// MFMA tiles of the trace products of control q per step (jq_timing.mfma_executed)
static long long plan_trace_tiles(const jq_handle* h, const BatchPlan& p, int q)
{
    return p.layout != SL_SLABS ? 0 : p.coop ? coop_tiles(h->NT, h->BWc) : (h->BW == JQ_BW_T4) ? ((h->bw_trace[q] & JQ_T4_DIAG) ? 4 * h->NT : 0)
                                                                                             : band_tiles(h->NT, h->bw_trace[q] == 0 ? 0 : h->BW, h->bw_trace[q] == 2);
}

// plan_batch: every routing decision of an evaluation, no HIP calls.  Refusals set h->err (fail) and return its code.
// The eligibility tests of the families exclude each other (each test names the families it yields to), so exactly one takes the batch:
//   implicit midpoint: row-lane (4) > cooperative quad (9) > quad layout (7) > cooperative (5);
//   Stormer-Verlet:    row-lane (3) > lane (2) > cooperative quad (8) > quad layout (6) > cooperative (1) > slab (0).
// Side effects: the split latency kernels' cool-down (cq3_skip, cq3_last: once per evaluation of those families with a gradient) and,
// when they are taken, the device held exclusively in gate_hold until the caller's scope ends.
// groups > 0: a GROUPED batch of that many control vectors (nsamples = groups x samples per vector -- one, or the nodes of an ensemble with
// the padding samples the caller added), every workgroup working for exactly one of them: Stormer-Verlet on the row-lane kernels (a vector's
// columns packed four per wave like an ensemble of its samples, the next vector at the next wave: cpw, wpg) and on the cooperative-quad
// kernels (a vector per column quad or consecutive quads, packed like an ensemble of its samples; one workgroup per quad in both sweeps --
// no two-quad forward variant, no split backward kernels).  Column counts that would put two vectors into one quad, and every other
// family, answer p->groups = 0: the caller evaluates the vectors one after the other.  A grouped plan has no side effects.
static int plan_batch(jq_handle* h, int nsamples, bool adjoint, bool hist, GateHold& gate_hold, BatchPlan* p, int groups = 0)
{
    memset(p, 0, sizeof *p);
    const bool grp = groups > 0;
    if (adjoint && !h->rfreq.empty() && h->integrator != 1)
        return fail(h, JQ_EUNSUPPORTED, "uncoupled controls (Hunc_ops): gradients with the Stormer-Verlet integrator only (the reference's "
                                        "implicit-midpoint adjoint has no term for them, src/evalobjgrad.jl:1347)");

    if (adjoint && h->sv_type != 1 && h->integrator != 1) return fail(h, JQ_EUNSUPPORTED, JQ_SV_IMR_REFUSAL);

    p->nslabs = h->parts > 1 ? nsamples * h->parts : (nsamples + h->sps - 1) / h->sps;
    const long long ncols_used = (long long)nsamples * h->N;
    // implicit midpoint: row-lane kernels for Ntot <= 16 with N <= 4 (an evaluation's columns share one wave: the solver's convergence test)
    const bool imr = (h->integrator == 2);
    const bool imr_rl = imr && h->rl_npj > 0 && h->N <= 4;
    // JQ_BW_T4 structure with an evaluation's columns inside one quad: quad-layout kernels (jq_quad_imr_kernels.h, any batch size); two
    // 16-row blocks WITHOUT the structure, N = 4: the dense policy of the cooperative-quad kernels, routed like their latency path (round 6)
    const bool imr_dq = imr && !imr_rl && h->quad_max_slabs == 0 && h->dq_max_quads > 0 && h->N == 4 && h->parts == 1 && h->wrank == 0 &&
                        (ncols_used + 3) / 4 <= h->dq_max_quads && h->opt.on(O_IMR_CQ);
    const bool imr_quad = imr && !imr_rl && ((h->quad_max_slabs > 0 && (h->N == 1 || h->N == 2 || h->N == 4)) || imr_dq);
    const bool imr_coop = imr && !imr_rl && !imr_quad;
    p->parts = imr_coop && h->parts > 1;      // N > 16: one workgroup per evaluation, its 16-column parts in turn
    // (both images of a step in LDS when they fit; dense 96 x 96 operators: the <6, 5> instantiation reads them from HBM / L2 per product)
    p->hbm = imr_coop && h->NT <= 6 && h->mat_elems_c > 0 && coop_imr_lds_bytes(h->NT, h->mat_elems_c) > JQ_LDS_MAX;
    if (imr_coop && (h->mat_elems_c == 0 || (p->hbm && !(h->NT == 6 && h->BWc == 5))))
        return fail(h, JQ_EUNSUPPORTED, "implicit midpoint: no kernels for these operators (no cooperative layout / images that do not fit the LDS)");
    const int spv = grp ? nsamples / groups : 1;      // samples of one control vector
    p->cpw = imr_rl ? imr_cols_per_wave(h->N) : grp ? spv * h->N : 4;   // columns per wave of the row-lane kernels (grouped: per vector, on wpg waves)
    p->wpg = (grp && !imr_rl) ? (spv * h->N + 3) / 4 : 1;
    // Full leakage weights (jq_update_wmat): row-lane kernels for every batch of an Ntot <= 16 problem, quad-layout kernels with one slab
    // per workgroup for the 4 x 4 x n structure (cooperative-quad kernels: wfull_cq below), else the cooperative kernels (every batch size)
    // or where those do not exist the slab kernels <1, 0> / <6, 5>; no lane or JQ_BW_T4 slab kernels
    const bool wfull = h->wrank > 0;
    if (wfull && imr)
        return fail(h, JQ_EUNSUPPORTED, "full leakage weights (jq_update_wmat): the implicit-midpoint path weights with params.wmat (Diagonal)");
    const bool wjac = wfull && h->solver_id == 2;      // full weights with the Jacobi solver: cooperative kernels, else the slab kernels <1, 0> / <6, 5>
    const bool rl = imr_rl || (!imr && h->rl_npj > 0 && h->solver_id == 1 && (ncols_used <= h->rl_max_cols || wfull));
    const bool lane = !imr && !rl && !wfull && h->lane_np > 0 && h->solver_id == 1 && ncols_used >= h->lane_min_cols && ncols_used <= h->lane_max_cols;
    p->nwaves_rl = (ncols_used + p->cpw - 1) / p->cpw * p->wpg;
    p->ncols = rl ? 4 * p->nwaves_rl : (ncols_used + 63) / 64 * 64;      // row-lane: column SLOTS (4 per wave)
    // JQ_BW_T4 structure: the quad-layout kernels (a slab per wave quartet: 3 x shorter dependent chain than the cooperative kernels)
    if (!imr && !lane && !rl && h->solver_id == 1 && p->nslabs <= h->quad_max_slabs) {
        t4_rounds(h, p->nslabs, true, &p->spw);
        if (h->opt.has(O_QUAD8)) {      // experiments / tests: force 4 / 8 / 12 waves (as far as the LDS allows)
            p->spw = std::max(1, std::min(3, (int)h->opt.get(O_QUAD8) + 1));
            while (p->spw > 1 && quad_bwd_lds(h, p->spw) > JQ_LDS_MAX) --p->spw;
        }
        if (wfull) p->spw = 1;      // (the instantiations with the low-rank terms: one slab per workgroup, any number of rounds)
    }
    if (wfull && !wjac && !rl && h->BW == JQ_BW_T4 && p->spw == 0)
        return fail(h, JQ_EUNSUPPORTED, "full leakage weights (jq_update_wmat): the quad-layout kernels are disabled or do not fit for this "
                                        "4 x 4 x n problem, and the JQ_BW_T4 slab kernels have no low-rank terms");
    // (one slab per workgroup, one wave per SIMD, the operators of a step in registers for all its fixed-point iterations; a
    // two-slab variant that re-reads them from LDS was measured 1.4 x slower, jq_kernel_inst.hip)
    if (imr_quad) p->spw = 1;
    // latency regime of the JQ_BW_T4 structure: one workgroup of NT waves per column quad (jq_cq_kernels.h)
    const long long nquads_used = (ncols_used + 3) / 4;
    // (full weights, round 5: four slots -- real W of rank <= 4, complex of rank <= 2 -- with one quad per workgroup, LDS permitting: jq_cq_kernels.h
    //  CqW; a complex W only with the split backward sweep, see below; option cq_w=0: the quad-layout kernels)
    const bool wfull_cq = wfull && (h->wlr_real ? h->wrank <= 4 : h->wrank <= 2) && h->NT <= 7 && h->opt.on(O_CQ_W) && (ncols_used + 3) / 4 <= h->num_cu &&
                          cq_lds(h, win_lds(h, h->mat_elems)) + (size_t)2 * h->NT * 64 * 8 <= JQ_LDS_MAX;
    bool cq = !imr && !lane && !rl && (!wfull || wfull_cq) && h->solver_id == 1 && h->cq_max_quads > 0 && nquads_used <= h->cq_max_quads &&
              !h->opt.has(O_QUAD8);      // (quad8 asks for a quad-layout variant explicitly)
    // ... and their DENSE policy (round 6): 17 .. 32 levels without the structure, Neumann, Diagonal weights (no two-quad forward variant)
    const bool cq_dn = !cq && !imr && !lane && !rl && !wfull && h->solver_id == 1 && h->dq_max_quads > 0 && nquads_used <= h->dq_max_quads;
    if (cq_dn) cq = true;
    p->qps = h->parts > 1 ? 4 : (h->sps * h->N + 3) / 4;      // column quads of a full slab
    // ... and of the implicit-midpoint integrator (jq_cq_imr_kernels.h): N = 4, one workgroup of NT waves per evaluation
    const bool imr_cq = imr_dq || (imr_quad && h->N == 4 && h->parts == 1 && h->cq_max_quads > 0 && nquads_used <= h->cq_max_quads &&
                                   h->opt.on(O_IMR_CQ));
    // more column quads than CUs: the forward sweep takes two quads per workgroup (one round at ~ 1.5 x the time instead of two; cq_fwd2=0 / 1)
    p->fwd2 = cq && !cq_dn && !wfull && !grp && (h->opt.has(O_CQ_FWD2) ? h->opt.on(O_CQ_FWD2) : nquads_used > h->num_cu);
    // single evaluations and small ensembles: the backward sweep on three workgroups per column quad (state re-integration | adjoint step |
    // trace products, through a ring in global memory: jq_cq_split_kernels.h), all resident at once, in groups of 8 quads (quad q is slot
    // q & 3 of slab q >> 2); round 5: two workgroups (state | adjoint + traces) for 2 x quads <= CUs, Stormer-Verlet only (cq3=3: three or none)
    p->nq_pad = (4LL * p->nslabs + 7) / 8 * 8;
    const bool c3_set = h->opt.has(O_CQ3);
    const long long c3_v = h->opt.get(O_CQ3);
    // Co-residency is checked, not assumed: the split is taken only when this evaluation is the only one of the process on the device
    // (GateHold: others then wait until it is through), with no CU mask in force, and not while the handle cools down after a fault.
    bool cq3 = false;
    if ((cq || imr_cq) && adjoint) {
        const char* why = nullptr;
        p->cq_nr = 3 * p->nq_pad <= h->num_cu ? 3 : (cq && 2 * p->nq_pad <= h->num_cu && !(c3_set && c3_v == 3)) ? 2 : 0;
        // The consumer roles read the sweep's starting state from the state file, which the state role overwrites when it is through: it
        // must have to WAIT for them, which it does from step 8 on (8 ring slots), so the first chunk must be longer than the ring (shorter
        // ones were a race, found in round 5 with option debug=16).  backward_chunk_steps gives the chunk length of the sweep below too.
        const long long cs_first = std::min<long long>(backward_chunk_steps(h, (size_t)p->nslabs * p->qps * (imr_cq ? h->NT : 1)), h->nsteps);
        if (grp) why = "not taken: grouped batch of control vectors (one workgroup per column quad)";
        else if (c3_set && c3_v == 0) why = "not taken: option cq3=0";
        else if (cs_first <= JQ_CQ3_RING) why = "not taken: the first chunk of the sweep is not longer than the hand-off ring (8 steps)";
        else if (p->cq_nr == 0) why = "not taken: two / three workgroups per column quad exceed the compute units";
        else if (h->cq3_off) why = "not taken: switched off after repeated faults (dead waits between the workgroups of a quad)";
        else if (h->cq3_skip > 0) why = "not taken: cooling down after a fault";
        else if (getenv("HSA_CU_MASK") || getenv("ROC_GLOBAL_CU_MASK")) why = "not taken: a CU mask is set (HSA_CU_MASK / ROC_GLOBAL_CU_MASK)";
        else if (g_eval_depth != 1) why = "not taken: nested evaluation (part of a split batch / embedded twin)";
        else if (!gate_hold.acquire(dev_gate(h->device))) why = "not taken: another evaluation of this process is in flight on the device";
        cq3 = (why == nullptr);
        if (!cq3) p->cq_nr = 0;
        if (h->cq3_skip > 0 && !grp) --h->cq3_skip;
        if (!grp) h->cq3_last = cq3 ? (p->cq_nr == 3 ? "taken: three workgroups per column quad, device held exclusively" : "taken: two workgroups per column quad, device held exclusively") : why;
    }
    // A complex W needs W_i vr(t_n) mid-step: only the split kernels (state role steps ahead) have it; without them the quad-layout kernels.
    if (cq && wfull && !h->wlr_real && adjoint && !cq3) cq = false;
    const bool imr_cq3 = imr_cq && cq3 && p->cq_nr == 3;
    const bool imr_cq2 = imr_cq && !imr_dq && !imr_cq3 && h->NT <= 6 && h->opt.on(O_IMR_CQ2) && cq_imr2_lds(h, win_lds(h, h->mat_elems)) <= JQ_LDS_MAX;
    if (cq) p->spw = 0;
    const bool quad = p->spw > 0;
    const bool quad8 = p->spw > 1;
    // mid-size ensembles of the 4 x 4 x n structure: the backward sweep with the state and the adjoint chain of a quad on two waves, one
    // step apart (jq_quad_split_kernels.h; qsplit=0: one wave).  qw = 4: the quad-layout plan with one slab per workgroup; qw = 2: more
    // column quads than CUs on the cooperative-quad plan, whose one-workgroup backward sweep would take two rounds
    const bool qs_set = h->opt.has(O_QSPLIT);
    const bool qs_on = adjoint && h->NT <= 6 && !(qs_set && h->opt.get(O_QSPLIT) == 0);
    if (qs_on && quad && !imr && p->spw == 1 && !wfull && qsplit_lds(h, 4) <= JQ_LDS_MAX) p->qs_qw = 4;      // (!imr: the implicit-midpoint quad kernels also run with spw = 1)
    // (option qsplit=2: qw = 2 for every batch of the cooperative-quad plan that does not take the three-workgroup kernels -- tests)
    const bool qs_force2 = qs_set && h->opt.get(O_QSPLIT) == 2;
    if (qs_on && cq && !cq_dn && !cq3 && !wfull && !grp && ((nquads_used > h->num_cu && 2 * p->nslabs <= h->num_cu) || qs_force2) && qsplit_lds(h, 2) <= JQ_LDS_MAX) p->qs_qw = 2;
    const bool qsplit = p->qs_qw > 0;
    p->qs_blocks = qsplit ? (4 * p->nslabs + p->qs_qw - 1) / p->qs_qw : 0;
    // (full weights: the cooperative kernels sum their column dots through an LDS record behind the Jacobi norms, else the slab kernels serve)
    const size_t coop_w_bytes = wfull ? (size_t)2 * JQ_COOP_WDOTS * h->NT * 16 * 8 : 0;
    const bool coop_w_fits = !wfull || coop_hbm(h->NT, h->BWc) ||
                             (size_t)2 * h->mat_elems_c * 8 + (size_t)32 * h->NT * 8 + (size_t)2 * h->KT * 64 * 8 + (size_t)16 * h->NT * 8 + coop_w_bytes <= JQ_LDS_MAX;
    const bool coop = imr_coop || (!cq && !quad && !lane && !rl && h->NT >= 2 && h->coop_ok && coop_w_fits && (h->solver_id == 1 || h->big || wjac) &&
                                   (p->nslabs <= h->coop_max_slabs || (wfull && !(h->NT == 6 && h->BW == 5))));      // (dense 96 x 96: the slab kernels <6, 5> carry the low-rank terms too -- large batches stay there)
    if (wjac && !coop && h->BW == JQ_BW_T4)      // (jq_update_wmat / jq_set_linear_solver re-plan such handles without the structure: cannot happen)
        return fail(h, JQ_EHIP, "internal error: full leakage weights with the Jacobi solver on a 4 x 4 x n plan without cooperative kernels");      // (Ntot > 96: also the Jacobi solver; full weights: every batch size -- the slab kernels have no low-rank terms)
    // row-lane backward sweep: implicit midpoint, the two chains on two waves while the doubled wave count still finds idle issue slots
    // (round 3: NPJ <= 8 up to three waves per SIMD, NPJ = 12, 16 one); Stormer-Verlet, three or four waves (state | adjoint | traces,
    // k_backward_rowlane3) at every batch size: they beat one wave from 1 to 2 048 samples, two never beat three (profiles/r06_rowlane3.txt).
    // Option rl_split: 0 = one wave, 1 = by these rules, 2 / 3 = two / three waves at every batch size (all bit-identical)
    const int rl_want = (int)h->opt.get(O_RL_SPLIT);
    const bool rl_sv = rl && !imr_rl;
    bool rl_split = rl && (rl_want >= 2 || rl_sv || 2 * p->nwaves_rl <= (long long)(h->rl_npj > 8 ? JQ_RL_ROOM_WIDE : JQ_RL_ROOM) * h->num_cu);
    if (rl_want == 0) rl_split = false;
    if (wfull) rl_split = false;      // (the one-wave backward kernel carries the low-rank terms)
    const bool rl_split3 = rl_split && rl_sv && rl_want != 2;
    p->family = imr_rl ? KF_ROWLANE_IMR : imr_cq ? KF_CQ_IMR : imr_quad ? KF_QUAD_IMR : imr_coop ? KF_COOP_IMR : rl ? KF_ROWLANE
              : lane ? KF_LANE : cq ? KF_CQ : quad ? KF_QUAD : coop ? KF_COOP : KF_SLAB;
    p->layout = rl ? SL_ROWLANE : lane ? SL_LANE : SL_SLABS;
    if (grp) {      // units per vector; only column counts under which the single evaluation has the same layout (bit-identical results)
        const bool n4 = spv > 1 || h->N < 4 || h->N % 4 == 0;      // (one sample per vector: the column counts jq_traceobjgrad_batch has always grouped)
        if (nsamples != groups * spv) return JQ_OK;
        if (p->family == KF_ROWLANE && !hist && n4) p->upg = p->wpg;
        // (cooperative quad: full slabs of whole samples, so that a quad is a trace row and holds one vector -- the caller pads with samples)
        else if (p->family == KF_CQ && !hist && h->parts > 1) p->upg = 4 * h->parts * spv;
        else if (p->family == KF_CQ && !hist && 16 % h->N == 0 && (spv * h->N) % 4 == 0) p->upg = spv * h->N / 4;
        if (p->upg == 0) return JQ_OK;      // (p->groups == 0: not served)
        p->groups = groups;
    }
    p->coop = coop;
    p->sched = JQ_SCHED[coop];
    p->rl_waves = rl_split3 ? 3 : rl_split ? 2 : 1;
    p->imr_cq_bwd = imr_cq3 ? 3 : imr_cq2 ? 2 : 1;
    p->dense = cq_dn || imr_dq;
    int rc = JQ_OK;
    switch (p->family) {
    case KF_CQ_IMR: rc = select_cq_imr_kernels(h, imr_cq2, imr_cq3, imr_dq, &p->kfwd, &p->kbwd, &p->sel); break;
    case KF_QUAD_IMR: rc = select_quad_imr_kernels(h, &p->kfwd, &p->kbwd, &p->sel); break;
    case KF_COOP_IMR: rc = p->parts ? select_coop_imr_parts_kernels(h, p->hbm, &p->kfwd, &p->kbwd, &p->sel) : select_coop_imr_kernels(h, p->hbm, &p->kfwd, &p->kbwd, &p->sel); break;
    case KF_ROWLANE_IMR: rc = select_rowlane_imr_kernels(h, rl_split, &p->kfwd, &p->kbwd, &p->sel); break;
    case KF_ROWLANE: rc = select_rowlane_kernels(h, p->rl_waves, hist, &p->kfwd, &p->kbwd, &p->sel); break;
    case KF_LANE: rc = select_lane_kernels(h, &p->kfwd, &p->kbwd, &p->sel); break;
    case KF_CQ: rc = select_cq_kernels(h, p->fwd2, p->cq_nr, wfull, cq_dn, &p->kfwd, &p->kbwd, &p->sel); break;
    case KF_COOP: rc = select_coop_kernels(h, &p->kfwd, &p->kbwd, &p->sel); break;
    case KF_QUAD: rc = wfull ? select_quad_w_kernels(h, &p->kfwd, &p->kbwd, &p->sel) : select_quad_kernels(h, p->spw, &p->kfwd, &p->kbwd, &p->sel); break;
    case KF_SLAB: rc = select_kernels(h, &p->kfwd, &p->kbwd, &p->sel); break;
    }
    if (rc) return rc;
    if (qsplit && (rc = select_qsplit_kernel(h, p->qs_qw, &p->kbwd, &p->sel))) return rc;
    // Jacobi solver with N > 16 on the slab kernels: ONE workgroup per sample when its parts fit one (N <= 64): the waves add their parts'
    // residual norms through LDS, so the stopping test is the reference's (src/linear_solvers.jl:121), not one per 16-column part (round 5;
    // option jac_wg=0: per part, as with more parts or the cooperative kernels)
    p->jac_wg = p->family == KF_SLAB && h->solver_id == 2 && h->parts > 1 && h->parts <= JQ_WAVES && h->opt.on(O_JAC_WG);
    p->huge = coop && h->huge;
    const int nblocks = p->jac_wg ? nsamples : p->parts ? nsamples : (cq || imr_cq) ? 4 * p->nslabs : rl ? (int)p->nwaves_rl : lane ? (int)(p->ncols / 64) : quad8 ? (p->nslabs + p->spw - 1) / p->spw : (coop || quad) ? p->nslabs : (p->nslabs + JQ_WAVES - 1) / JQ_WAVES;
    const int nthreads = p->huge ? 64 * JQ_HUGE_WAVES : p->jac_wg ? 64 * h->parts : (lane || rl) ? 64 : (coop || cq || imr_cq) ? 64 * h->NT : quad8 ? 256 * p->spw : 256;
    // per-step trace records: one per wave (cooperative, lane, row-lane, implicit-midpoint kernels) or per workgroup (slab / quad kernels)
    p->trace_rows = qsplit ? p->qs_blocks : p->parts ? nsamples * h->NT : imr_cq ? p->nslabs * p->qps * h->NT : cq ? p->nslabs * p->qps : (lane || rl) ? nblocks : p->huge ? p->nslabs * JQ_HUGE_WAVES : coop ? p->nslabs * h->NT : imr_quad ? p->nslabs * JQ_WAVES : nblocks;
    p->stride = p->dense ? (long long)JQ_DQ_ELEMS : rl ? h->rl_stride : lane ? h->lane_stride : coop ? h->mat_elems_c : h->mat_elems;
    p->himg = p->dense ? h->d_himg_dq : rl ? h->d_himg_r : lane ? h->d_himg_l : coop ? h->d_himg_c : h->d_himg;
    p->cimg = p->dense ? h->d_cimg_dq : rl ? h->d_cimg_r : lane ? h->d_cimg_l : coop ? h->d_cimg_c : h->d_cimg;      // (control-group order)
    p->state_doubles = rl ? (size_t)JQ_ROWLANE_ROWS * p->nwaves_rl * 64 : lane ? (size_t)JQ_LANE_ROWS(h->lane_np) * p->ncols : (size_t)p->nslabs * h->state_stride;
    p->colinfo_doubles = (lane || rl) ? (size_t)2 * p->ncols : (size_t)p->nslabs * 32;
    // (parking images: one array per slab; ImrParts (implicit midpoint, N > 16) ten, huge the work area of a slab; none for the lane layouts)
    p->park_slabs = (lane || rl) ? 0 : (size_t)p->nslabs * (p->parts ? JQ_IMRP_ARRAYS : p->huge ? JQ_HUGE_VECS : 1);
    p->ws_off = rl ? 16 : lane ? (size_t)h->lane_np : (size_t)16 * h->NT;   // tables: [wd | ws]
    p->tiles = (lane || rl) ? 0 : coop ? coop_tiles(h->NT, h->BWc) : band_tiles(h->NT, h->BW);
    // (JQ_BW_T4: a v_mfma_f64_4x4x4_4b is a quarter of the 16x16x4 instruction counted; implicit midpoint: data-dependent iteration counts)
    p->mfma_div = imr ? 0 : (!coop && !lane && !rl && h->BW == JQ_BW_T4) ? 4 : 1;
    p->cs = adjoint ? backward_chunk_steps(h, (size_t)p->trace_rows) : h->chunk_steps;
    if (grp) {
        // a chunk holds one tile stream per vector, each of THIS family's image size (not the largest image of any family jq_create sized the
        // buffer by): as many steps as the stream budget holds -- option stream_bytes, default 1 GiB, or the buffer the handle has; run_eval
        // grows a buffer that option chunk_steps kept below the budget.  Never longer than the single evaluation's chunk.
        const size_t budget = stream_budget_bytes(h) / sizeof(double);
        const long long tps = (long long)(std::max(budget, h->cap_stream) / ((size_t)groups * 2 * (size_t)p->stride));
        p->cs = (int)std::max<long long>(1, std::min<long long>(p->cs, (tps - 1) / 2));
    }
    if (cq3 && std::min(p->cs, h->nsteps) <= JQ_CQ3_RING)      // (the decision above was made for this very chunking)
        return fail(h, JQ_EHIP, "internal error: split latency kernels selected for a first chunk that is not longer than their hand-off ring");
    p->prop_nslabs = rl ? (int)p->nwaves_rl : lane ? (int)p->ncols : p->nslabs;
    // backward sweep: two waves per column quad (qsplit), three / two workgroups per quad of NT block + two staging waves (cq3), else the family's
    p->fwd_grid = p->fwd2 ? nblocks / 2 : nblocks;
    p->fwd_block = (cq || imr_cq) ? nthreads + 128 : nthreads;      // (cooperative quad: two staging waves)
    p->bwd_grid = qsplit ? p->qs_blocks : cq3 ? (unsigned)(p->cq_nr * p->nq_pad) : nblocks;
    p->bwd_block = qsplit ? 128 * p->qs_qw : cq3 ? nthreads + 128 : rl_split3 ? 3 * nthreads /* state | adjoint | traces */ : (cq || rl_split) ? 2 * nthreads
                 : imr_cq2 ? 2 * (nthreads + 128) : imr_cq ? nthreads + 128 : nthreads;      // (cooperative quad: state and adjoint chain on separate waves)
    p->bwd_block_ng2 = (!qsplit && !cq3 && rl_split3) ? 4 * nthreads : p->bwd_block;      // (two trace waves for two or more controls)
    // dynamic LDS layout: [operator staging | tables wd, ws | (backward: carry, parking images)]
    // cooperative kernels: [two operator slots | tables wd, ws | two x exchange buffers]
    p->batch = coop ? 0 : (quad || cq || imr_dq) ? -1 : h->batch;
    p->lds_stage = (coop && (h->NT > 6 || p->hbm || (!imr_coop && coop_hbm(h->NT, h->BWc)))) ? 0      // operators are read from HBM, no LDS staging
                             : p->batch > 0   ? (size_t)2 * (2 * p->batch + 1) * 2 * p->stride * 8 + (size_t)2 * h->NcK * p->stride * 8
                             : p->batch < 0 ? win_lds(h, p->stride)
                                         : (size_t)2 * p->stride * 8;
    const size_t lds_fwd = p->huge ? 0 : (rl && !imr_rl) ? (wfull ? (size_t)JQ_RL_WTAB * 8 : 0) + JQ_RL_RING_BYTES(h->rl_npj) /* operator ring of the forward sweep */ : rl ? 0 : lane ? 0 : (cq || imr_cq) ? cq_lds(h, p->lds_stage) : imr_coop ? coop_imr_lds_bytes(h->NT, p->hbm ? 0 : p->stride)
                                           : p->lds_stage + (size_t)32 * h->NT * 8 + (coop ? (size_t)2 * h->KT * 64 * 8 + (size_t)16 * h->NT * 8 + coop_w_bytes : 0);      // (+ the Jacobi solver's column norms [NT][16], the low-rank weights' dot exchange)
    const size_t lds_bwd = p->huge ? 0 : qsplit ? qsplit_lds(h, p->qs_qw) : rl_split3 ? JQ_RL3_LDS(h->rl_npj) : rl ? (h->rl_npj > 8 ? (size_t)2 * h->NcK * h->rl_stride * 8 : 0) + (rl_split ? (size_t)2 * 3 * 64 * 8 : 0) /* records: 3 values per lane and slot, implicit midpoint 2 */ + (wfull ? (size_t)JQ_RL_WTAB * 8 : 0) /* low-rank weight table */ : lane ? 0 : imr_cq2 ? cq_imr2_lds(h, p->lds_stage) : (coop || cq || imr_cq) ? lds_fwd
                                : imr_quad ? lds_fwd + (size_t)JQ_MAXNC * nthreads * 8 + (size_t)(nthreads / 64) * h->NT * 64 * 8
                                : quad ? quad_bwd_lds(h, p->spw)
                                : p->lds_stage + (size_t)bwd_lds_tail(h->NT, h->NcK, JQ_WAVES, h->park_lds ? (long long)h->KT * 64 : 0);
    // full leakage weights on the slab / quad kernels: a copy of the low-rank table behind everything else in LDS when it fits
    const size_t wlr_bytes = (wfull && cq) ? (size_t)2 * h->NT * 64 * 8      // (cooperative quad: the partial dots of two vectors, CqW)
                             : (wfull && !coop && !rl && !lane) ? ((size_t)h->wlam + (size_t)2 * h->wrank * h->NP) * 8 : 0;
    p->fwd.wlr = (wlr_bytes && lds_fwd + wlr_bytes <= JQ_LDS_MAX) ? (int)lds_fwd : -1;
    p->bwd.wlr = (wlr_bytes && lds_bwd + wlr_bytes <= JQ_LDS_MAX) ? (int)lds_bwd : -1;
    // (the cooperative-quad kernels have no table in global memory to fall back to: wfull_cq above admitted them only when this fits)
    if (wfull && cq && (p->fwd.wlr < 0 || p->bwd.wlr < 0)) return fail(h, JQ_EHIP, "internal error: no LDS left for the partial dots of the full leakage weights");
    // ... and, quad layout, the per-wave column scalars of the terms behind it (jq_kernels.h WLow::sc): OFF unless option wlr_sc=1, measured
    // SLOWER than recomputing the dots (round 5, cnot3: 57 -> 70 ms per forbidden state; profiles/r05_exp_variants.txt (3))
    const size_t wsc_bytes = (wlr_bytes && quad && h->opt.get(O_WLR_SC) == 1) ? (size_t)(nthreads / 64) * JQ_MAX_WRANK * 24 * 8 : 0;
    const size_t wsc_off_fwd = lds_fwd + (p->fwd.wlr >= 0 ? wlr_bytes : 0), wsc_off_bwd = lds_bwd + (p->bwd.wlr >= 0 ? wlr_bytes : 0);
    p->fwd.wsc = (wsc_bytes && wsc_off_fwd + wsc_bytes <= JQ_LDS_MAX) ? (int)wsc_off_fwd : -1;
    p->bwd.wsc = (wsc_bytes && wsc_off_bwd + wsc_bytes <= JQ_LDS_MAX) ? (int)wsc_off_bwd : -1;
    const size_t jac_bytes = p->jac_wg ? (size_t)2 * JQ_WAVES * 8 : 0;      // (residual exchange of the workgroup-wide Jacobi test, behind everything else)
    if (p->jac_wg && std::max(lds_fwd, lds_bwd) + jac_bytes > JQ_LDS_MAX) return fail(h, JQ_EHIP, "internal error: no LDS left for the Jacobi residual exchange");
    p->fwd.jac = p->jac_wg ? (int)lds_fwd : -1;
    p->bwd.jac = p->jac_wg ? (int)lds_bwd : -1;
    p->fwd.total = lds_fwd + (p->fwd.wlr >= 0 ? wlr_bytes : 0) + (p->fwd.wsc >= 0 ? wsc_bytes : 0) + jac_bytes;
    p->bwd.total = lds_bwd + (p->bwd.wlr >= 0 ? wlr_bytes : 0) + (p->bwd.wsc >= 0 ? wsc_bytes : 0) + jac_bytes;
    p->park_lds = quad ? 1 : h->park_lds;
    p->term = p->parts ? TK_IMR_PARTS : (imr_coop || imr_quad) ? TK_IMR : imr ? TK_ROWLANE_IMR : rl ? TK_ROWLANE : lane ? TK_LANE : h->parts > 1 ? TK_PARTS : TK_SLAB;
    p->kernel_size = rl ? h->rl_npj : lane ? h->lane_np : h->NT;
    p->kernel_band = (rl || lane) ? 0 : coop ? h->BWc : p->dense ? 10 /* dense blocks on the cooperative-quad kernels */ : (quad || cq) ? JQ_BW_T4Q : h->BW;
    p->kernel_variant = cq3 ? p->cq_nr : qsplit ? 20 + p->qs_qw : (rl && rl_split3) ? 33 : (rl && rl_split) ? 32 : 0;      // (workgroups per column quad in the backward sweep of the cooperative-quad kernels)
    return JQ_OK;
}
