// juqbox_hip.hip -- C ABI (include/juqbox_hip.h) and host orchestration of the gfx950 propagator.
//
// One evaluation = { forward sweep, terminal condition, backward sweep(s), gradient assembly } over a
// batch of N*nsamples state columns.  Time is processed in chunks: for each chunk the controls are
// evaluated on the device (k_ctrl), the K(t)/S(t) tile stream is generated into a reusable HBM buffer
// (k_stream) and one persistent propagator launch consumes it (k_forward / k_backward).  Everything
// runs in order on the handle's HIP stream; the call returns after one stream synchronisation.
#include "../../include/juqbox_hip.h"
#include "jq_aux_kernels.h"
#include "jq_coop_kernels.h"
#include "jq_kernels.h"
#include "jq_lane_kernels.h"
#include "jq_lane_tl_kernels.h"
#include "jq_rowlane_kernels.h"
#include "jq_rowlane_tl_kernels.h"
#include "jq_rowlane_imr_kernels.h"
#include "jq_coop_imr_kernels.h"
#include "jq_huge_kernels.h"
#include "jq_tl_kernels.h"
#include "jq_tl_adjoint_kernels.h"
#include "jq_options.h"

#include <rccl/rccl.h>   // types and prototypes only: librccl is loaded at run time by jq_create_multi (load_rccl)

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#ifndef JQ_SRC_HASH
#define JQ_SRC_HASH "unknown"      // (the Makefile passes the SHA-256 prefix of the library's sources)
#endif
#ifndef JQ_CODE_HASH
#define JQ_CODE_HASH "unknown"
#endif
#define JQ_VERSION "gfx950 juqbox_hip 0.4.0 src:" JQ_SRC_HASH " code:" JQ_CODE_HASH

static thread_local std::string g_create_error;
// JQ_DEBUG_TIMING=1: every propagator launch's HIP-event time on stderr (development aid; changes no result and no kernel choice)
static bool debug_timing()
{
    static const bool on = getenv("JQ_DEBUG_TIMING") != nullptr;
    return on;
}

// build manifest (scripts/make_manifest.py -> build/manifest.c): {"<object tag>": {"vgpr_form": .., "fallback": .., "max_vgprs": ..,
// "max_agprs": .., "max_scratch_bytes": ..}, ...} -- flat entries, quoted by jq_plan_info
extern "C" const char jq_build_manifest[];

// Which instantiation the select_* functions of jq_host_select.h chose for a batch: the objects (csrc/Makefile tags) of the forward and the
// backward kernel and the compile-time variant.  select_* fill the record of the BatchPlan that plan_batch hands them, run_eval publishes
// the plan's record as jq_handle::last_kernels once the evaluation is through (jq_plan_info "last_kernels").
#define JQ_SEL_TAG 12
struct KernelSel {
    bool set = false;
    char fwd[JQ_SEL_TAG] = "", bwd[JQ_SEL_TAG] = "";
    int spw = 0;                // quad layout: slabs per workgroup (0: another family)
    int qs_qw = 0;              // k_backward_qsplit: column quads per workgroup (0: not taken)
    int bwd_wgs = 0;            // cooperative quad: workgroups per column quad in the backward sweep (0: another family)
    bool uni = false, ord = false, sc_fwd = false, sc_bwd = false, ride = false, modd = false, fwd2 = false, wlr = false, imr_two = false;
};

struct jq_handle {
    int device = 0;
    KernelSel last_kernels;
    JqOptions opt;              // per-handle options (jq_options.h): jq_create_opts / JQ_OPTIONS / jq_set_option
    hipStream_t stream = nullptr;
    // problem
    int Ntot = 0, N = 0, Nc = 0, Nfreq = 0, nsteps = 0, m = 0, objFuncType = 1;
    int integrator = 1;         // 1 Stormer-Verlet, 2 implicit midpoint (JACOBI_SOLVER_M fixed-point solver)
    int imr_max_iter = 100;
    double imr_tol = 1e-12;
    int solver_id = 1;          // 1 NEUMANN_SOLVER, 2 JACOBI_SOLVER
    double solver_tol = 0.0;
    double T = 0.0;
    int NT = 0, KT = 0, NP = 0, sps = 0;
    int parts = 1;              // N > 16: a sample's columns take `parts` = ceil(N / 16) consecutive slabs (sps = 1)
    int BW = 0;                 // block band width the kernels are instantiated for (JQ_BW_OD: see jq_kernels.h)
    int BWc = 0;                // ... of the cooperative kernels (plain band)
    // More than JQ_MAXNC (= 4, the kernels' trace / carry bookkeeping) control Hamiltonians: the propagators see ALL controls
    // in K(t), S(t) (k_ctrl / k_stream are generic), only the gradient traces are per control -- the backward sweep then runs once
    // per GROUP of at most JQ_MAXNC controls (ctrl_groups(); 5 .. 8 controls: two sweeps), each with its own trace images.
    int NcK = 0;                // controls per backward sweep the LDS plan is made for: min(Nc, JQ_MAXNC)
    std::vector<int> bw_trace;  // [Nc]
    bool s_uniform = false;     // 4 x 4 x n plan: every 16-row block of an S image repeats block 0 (hanti_s_uniform, jq_host_images.h)
    long long mat_elems = 0;    // doubles per operator image slot ("stride"): band tiles, padded to 1 KiB
    long long mat_elems_c = 0;  // ... in the row-window layout of the cooperative kernels (0: not available)
    bool coop_ok = false;       // the cooperative Stormer-Verlet kernels fit the LDS (dense 96 x 96: only the implicit-midpoint variant that reads its images from HBM)
    int coop_max_slabs = 256;   // batches with at most this many slabs (= CUs: one workgroup each) use the cooperative kernels
    long long state_stride = 0;
    int nslots = 2;             // LDS ring depth of the forward kernel
    int nslots_bwd = 2;         // ... of the backward kernel (shares LDS with carry + parking images)
    int park_lds = 0;           // backward kernel parks its dormant array in LDS (1) or HBM (0)
    int batch = 0;              // > 0: batched staging (K/S images of `batch` time steps per DMA burst); < 0: window staging
    bool big = false;           // Ntot > 96 (NT = 7 .. 16): only the cooperative kernels with operators read from HBM (jq_coop_kernels.h
                                // OpCursor) exist -- Stormer-Verlet, Neumann solver, any batch size
    bool huge = false;          // Ntot > 256 (more than 16 tile rows): the run-time-size kernels of jq_huge_kernels.h (one workgroup of 16 waves per slab,
                                // every vector of a step in a global work area, dense tiles); a huge handle is also `big`
    bool force_plain = false;   // full leakage weights WITH the Jacobi solver on a 4 x 4 x n plan whose kernels do not combine the two (one tile row,
                                // or seven / eight): the handle is planned without that structure (cooperative / slab kernels that do)
    bool replanned = false;     // jq_update_hconst re-planned this handle (a later drift plans again when it violates the plan or regains a better structure)
    double* d_pk2 = nullptr;    // packed result of the first part of a split batch
    size_t cap_pk2 = 0;
    int dq_max_quads = 0;       // no structure, 17 .. 32 levels: batches of at most this many column quads on the DENSE cooperative-quad kernels (round 6)
    double *d_himg_dq = nullptr, *d_cimg_dq = nullptr;      // their operator images (jq_host_images.h dq_image), JQ_DQ_ELEMS doubles each
    int cq_max_quads = 0;       // JQ_BW_T4 structure: batches of at most this many column quads (4 columns) run on the cooperative-quad
                                // (latency) kernels, one workgroup of NT waves per quad (0: never)
    int quad_max_slabs = 0;     // JQ_BW_T4 structure: batches of at most this many slabs may use the quad-layout kernels (0: never)
    int num_cu = 256;
    int lane_np = 0;            // > 0: lane kernels available (Ntot <= 12), padded Hilbert dimension NP
    long long lane_stride = 0;  // doubles per plain NP x NP operator image (padded to 64 B)
    int lane_min_cols = 0, lane_max_cols = 0;   // column counts (samples x N) routed to the lane kernels
    int rl_npj = 0;             // > 0: row-lane kernels available (Ntot <= 16), padded row length NPJ
    long long rl_stride = 0;    // doubles per [16][NPJ] operator image
    int rl_max_cols = 0;        // batches of at most this many columns use the row-lane kernels (latency regime)
    std::vector<double> Hconst, Hsym, Hanti, Uinit, Utr, Uti, wd, cfreq;
    // Continuation adjoints (jq_set_sv_type / jq_update_dvds; src/evalobjgrad.jl:312-319, :815-844): which of the target and dVds the terminal
    // kernels trace against and build lambda(T) from (JQ_SV_*).  dVr / dVi start as a copy of the target; their device images (the three
    // layouts of the target's) exist only once a type other than 1 has been asked for -- dv_stale: the host copy is newer than they are.
    int sv_type = 1;
    std::vector<double> dVr, dVi;
    bool dv_stale = true, dv_alloc = false;
    double *d_dvr = nullptr, *d_dvi = nullptr, *d_dvr_l = nullptr, *d_dvi_l = nullptr, *d_dvr_r = nullptr, *d_dvi_r = nullptr;
    std::vector<double> rfreq;  // uncoupled controls (Nunc > 0): params.Rfreq; empty otherwise
    double* d_rfreq = nullptr;
    // Full leakage weights (jq_update_wmat): W = wmat_real + i wmat_imag = sum_{k < wrank} lam_k f_k f_k^H.  wrank > 0: `wd` is all
    // zero, Wr / Wi keep the caller's matrices (re-planning applies them again), wlr is the kernels' table
    // lam[JQ_MAX_WRANK] | a_k[NP], b_k[NP] per k in natural row order (PropArgs::wlr).
    int wrank = 0;
    int wlam = JQ_MAX_WRANK;    // lam slots in front of the rows of the table: max(JQ_MAX_WRANK, wrank)
    std::vector<double> Wr, Wi, wlr;
    double* d_wlr = nullptr;
    bool wlr_real = false;      // every kept eigenvector is real (wmat_imag = 0): the cooperative-quad kernels take rank <= 4 of those
    std::vector<double> tf, tb;
    // device buffers (owned)
    double *d_cimg = nullptr, *d_park = nullptr;
    double* d_cq3 = nullptr;    // hand-off buffer of k_backward_cq3 (jq_cq_split_kernels.h)
    size_t cap_cq3 = 0;
    // Three-workgroup latency kernels (k_backward_cq3 / k_backward_cq_imr3): their workgroups wait for each other, so all of them must be
    // resident at once.  Inside this process that is CHECKED (DevGate below: the split is taken only while no other evaluation runs on
    // the device, and nothing else starts until it is through); what other processes, CU masks or a partitioned device do cannot be
    // seen from here -- a wait that is declared dead raises the error word, the evaluation is repeated without the split (the word is
    // read after the FIRST backward launch), and the handle leaves the split alone for cq3_skip evaluations (4, 8, 16 ... per fault;
    // for good after JQ_CQ3_MAX_FAULTS faults).
    bool cq3_off = false;       // never again on this handle (too many faults)
    int cq3_faults = 0;         // launches that reported a dead wait / workgroups on different XCDs
    int cq3_faults_xcd = 0;     // ... of them: the workgroups of a quad ran on different XCDs (error word 2)
    int cq3_busy = 0;           // launches abandoned at their start-up rendezvous (the GPU was busy: not every workgroup became resident in time)
    int cq3_busy_streak = 0;    // ... in a row (sets the cool-down)
    double cq3_us_per_step = 0.0;   // measured duration of a split backward launch per time step (sizes the in-launch wait guard)
    int cq3_skip = 0;           // evaluations left for which the split is not tried
    std::string cq3_last;       // why the last batch of the latency families did / did not take the split (jq_plan_info)
    double* d_qsplit = nullptr; // hand-off buffer of k_backward_qsplit (jq_quad_split_kernels.h): [quad][parity][2][NT][64]
    size_t cap_qsplit = 0;
    double *d_himg_c = nullptr, *d_cimg_c = nullptr;   // operator images in the cooperative layout
    double *d_himg_l = nullptr, *d_uinit_l = nullptr, *d_vtr_l = nullptr, *d_vti_l = nullptr;   // lane kernels
    double *d_himg_r = nullptr, *d_uinit_r = nullptr, *d_vtr_r = nullptr, *d_vti_r = nullptr;   // row-lane kernels
    double *d_cimg_l = nullptr, *d_cimg_r = nullptr;   // their trace images in control-group order
    double *d_himg = nullptr, *d_uimg = nullptr, *d_vtr = nullptr, *d_vti = nullptr, *d_tabs = nullptr;
    double *d_tf = nullptr, *d_tb = nullptr, *d_cfreq = nullptr, *d_pcof = nullptr;
    double *d_stream = nullptr, *d_pq = nullptr;
    double* d_drift = nullptr;  // drift images of the members of a drift ensemble's launch, [groups][stride of the planned family] (run_eval)
    size_t cap_drift = 0;
    double* d_mix = nullptr;    // control mixes of an evaluation's groups [groups][Nc x Nc], behind them k_ctrl's unmixed values in d_pq's layout (run_eval)
    size_t cap_mix = 0;
    double *d_state = nullptr, *d_state_save = nullptr, *d_colinfo = nullptr, *d_traces = nullptr, *d_R = nullptr;
    double *d_grad = nullptr, *d_res = nullptr;
    double *d_wq = nullptr, *d_pack = nullptr;   // ensemble weights per sample; packed result [2 + 2 nCoeff] (multi-device all-reduce)
    size_t cap_pcof = 0, cap_slabs = 0, cap_traces = 0, cap_grad = 0, cap_res = 0, cap_state = 0, cap_colinfo = 0, cap_wq = 0, cap_pack = 0;
    int chunk_steps = 0;
    size_t cap_stream = 0, cap_pq = 0, cap_R = 0;      // doubles of d_stream, d_pq, d_R (jq_create sizes them for one control vector; a grouped batch may grow them)
    // what the last jq_traceobjgrad_batch / jq_eval_f_g_grad_batch did (pcof_batch; jq_plan_info "pcof_batch").  An evaluation's inputs are
    // not kept here: they travel in its EvalRequest (jq_host_eval.h)
    std::string pb_mode, pb_why;
    int pb_family = -1, pb_per_launch = 0, pb_nodes = 1;
    // ... and the last jq_traceobjgrad_drifts / jq_eval_f_g_grad_drifts with its members (jq_plan_info "drift_batch")
    std::string db_mode, db_why;
    int db_family = -1, db_per_launch = 0;
    // ... and the last member ensemble of any kind, the two drifts calls included (jq_plan_info "member_batch")
    std::string mb_mode, mb_why;
    int mb_family = -1, mb_per_launch = 0;
    bool mb_drifts = false, mb_mix = false;
    // ... and the last jq_traceobj_jvp: directions per launch, chunk length, rounds (jq_plan_info "jvp"; rounds 0: no call yet)
    int jvp_per_launch = 0, jvp_chunk = 0, jvp_rounds = 0;
    // ... and the last jq_traceobjgrad_hvp, the same three (jq_plan_info "hvp")
    int hvp_per_launch = 0, hvp_chunk = 0, hvp_rounds = 0;
    // ... and the last jq_eval_f_g_grad_hvp: its route (0: no call yet, 1 lane, 2 sequential, 3 row-lane) and the same three (jq_plan_info "ens_hvp")
    int ens_hvp_route = 0, ens_hvp_per_launch = 0, ens_hvp_chunk = 0, ens_hvp_rounds = 0;
    // ... and the last jq_eval_f_g_grad_drifts_hvp: its route (the same codes), members and directions per launch, chunk length, rounds
    // (direction rounds x member rounds; sequential: the members' sums) (jq_plan_info "drift_hvp")
    int drift_hvp_route = 0, drift_hvp_members = 0, drift_hvp_per_launch = 0, drift_hvp_chunk = 0, drift_hvp_rounds = 0;
    // ... and the last jq_eval_f_g_grad_members_hvp: the same five, and what differed between its members (jq_plan_info "member_hvp")
    struct MemberHvp {
        int route = 0, members = 0, per_launch = 0, chunk = 0, rounds = 0;
        bool drifts = false, mix = false;
    } member_hvp;
    // ... and the last evaluation with sampled controls (jq_traceobjgrad_samples / jq_eval_f_g_grad_samples): time points of the table,
    // nodes, chunk length (jq_plan_info "sampled_controls"; sc_nt 0: no call yet)
    int sc_nt = 0, sc_nodes = 0, sc_chunk = 0;
    // ... and the last jq_eval_f_g_grad_samples_hvp: its route (the codes of ens_hvp_route), directions per launch, chunk length, rounds,
    // time points of the tables, nodes (jq_plan_info "sampled_hvp"; route 0: no call yet)
    struct SampledHvp {
        int route = 0, per_launch = 0, chunk = 0, rounds = 0, nt = 0, nodes = 0;
    } sampled_hvp;
    // ... and the last jq_traceobjgrad_samples_batch / jq_traceobjgrad_samples_members / jq_eval_f_g_grad_samples_members: what its groups were
    // ("tables" | "members"), the route with its reason, the kernel family that ran, groups per launch, what differed between the members,
    // time points of the tables, chunk length (jq_plan_info "sampled_batch"; kind empty: no call yet)
    struct SampledBatch {
        std::string kind, mode, why;
        int family = -1, per_launch = 0, nt = 0, chunk = 0;
        bool drifts = false, mix = false;
    } sampled_batch;
    // Structure embedding (try_embed): a second handle of the SAME problem with its two fastest Kronecker factors zero-padded
    // to 4 levels each (row i1 + d1 i2 + d1 d2 i3 -> i1 + 4 i2 + 16 i3), under which the operators have the JQ_BW_T4 structure;
    // batches that would otherwise run on the dense / band MFMA kernels go there (quad-layout / JQ_BW_T4 slab kernels).
    jq_handle* emb = nullptr;
    std::vector<int> emb_row;   // user row -> row of the embedded problem
    int emb_mode = 1;           // JQ_EMBED: 0 never, 1 for batches of the MFMA families (default), 2 whenever possible (tests)
    bool is_emb = false;        // this handle IS an embedded twin: no lane / row-lane / cooperative families, no further embedding
    // multi-device handle (jq_create_multi): one single-device handle per GPU and one RCCL communicator each; such a
    // handle owns no device memory itself
    std::vector<jq_handle*> subs;
    std::vector<ncclComm_t> comms;
    bool host_reduce = false;   // option multi_same_device test mode: host-side sum instead of the ncclAllReduce (no communicators)
    bool comm_broken = false;   // an RCCL call failed inside a collective: the communicators are aborted at destroy, calls refuse
    int rccl_checks = 0;        // all-reduces of this handle that were verified against the host-order sum (JQ_RCCL_SELFCHECK)
    std::vector<hipEvent_t> ev;
    std::string err;
    jq_timing timing = {};
};

#define HIPCHK(h, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            char buf_[512];                                                                          \
            snprintf(buf_, sizeof buf_, "HIP error '%s' at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #call); \
            (h)->err = buf_;                                                                         \
            return JQ_EHIP;                                                                          \
        }                                                                                            \
    } while (0)

static int fail(jq_handle* h, int code, const char* msg)
{
    h->err = msg;
    return code;
}

// control groups: group g of ctrl_ngroups(Nc) holds the controls [ctrl_gstart(Nc, g), ctrl_gstart(Nc, g + 1)); sizes differ by <= 1
static int ctrl_ngroups(int Nc) { return (Nc + JQ_MAXNC - 1) / JQ_MAXNC; }
static int ctrl_gstart(int Nc, int g)
{
    const int ng = ctrl_ngroups(Nc), base = Nc / ng, rem = Nc % ng;
    return g * base + std::min(g, rem);
}

// restores the caller's current HIP device when a multi-device entry point returns (a Julia / PyTorch caller that was on
// another device must not find itself switched)
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

#include "jq_host_images.h"      // operator / state images in the kernels' layouts and the structure tests the planner uses
#include "jq_host_create.h"      // device buffers, uploads, jq_create* (planning from the operators' nonzero structure), structure embedding
#include "jq_host_update.h"      // the mutations scripts apply to params after construction: solver / integrator, target, drift (re-planning), leakage weights
#include "jq_inst_list.h"        // the list of the propagator-kernel instantiations
#include "jq_host_select.h"      // ... declared (they are compiled in their own translation units), and the functions that pick one
#include "jq_host_plan.h"      // plan_batch: how a batch is routed to a kernel family, its geometry and LDS layout
#include "jq_host_eval.h"      // run_eval: an EvalRequest evaluated by its plan, chunk by chunk
extern "C" int jq_traceobjgrad(jq_handle* h, const double* pcof, int32_t ncoeff, int32_t evaladjoint, double* out4,
                               double* totalgrad, double* infidelgrad, double* leakgrad)
{
    if (!h) return JQ_EINVAL;
    if (!pcof || !out4) return fail(h, JQ_EINVAL, "jq_traceobjgrad: NULL pointer");
    if (evaladjoint && (!totalgrad || !infidelgrad || !leakgrad))
        return fail(h, JQ_EINVAL, "jq_traceobjgrad: gradient outputs are required when evaladjoint != 0");
    JQ_ON_FIRST(h, jq_traceobjgrad(s0_, pcof, ncoeff, evaladjoint, out4, totalgrad, infidelgrad, leakgrad))
    EvalRequest rq;
    rq.pcof = pcof, rq.ncoeff = ncoeff, rq.adjoint = evaladjoint != 0;
    EvalOut o;
    int rc = run_eval(h, rq, &o);
    if (rc) return rc;
    out_record(out4, o.res.data());
    if (evaladjoint) out_grads(h, ncoeff, o.grad0.data(), o.grad1.data(), totalgrad, infidelgrad, leakgrad);
    return JQ_OK;
}

// What jq_traceobjgrad_batch (Q = 1) / jq_eval_f_g_grad_batch (Q nodes per vector) do with npcof control vectors on this (single-device)
// handle: the number of vectors per launch of a grouped batch (plan_batch with groups), or 0 -- the vectors one after the other -- with the
// reason in *why.  *spg: samples a vector is padded to.
static int pcof_batch_per_launch(jq_handle* h, int npcof, int Q, bool adjoint, int* spg, int* family, const char** why)
{
    *spg = 1, *family = -1;
    if (h->opt.has(O_PCOF_BATCH_MAX) && h->opt.get(O_PCOF_BATCH_MAX) <= 0) return *why = "option pcof_batch_max=0", 0;
    if (npcof == 1) return *why = "one vector: the single evaluation (with the split backward kernels where they apply)", 0;
    if (h->integrator != 1) return *why = "implicit-midpoint integrator: no grouped streams on its kernels", 0;
    if (h->solver_id != 1) return *why = "Jacobi solver: served by the slab / cooperative kernels", 0;
    // Two candidates, in plan_batch's order: row-lane kernels (a vector per wave(s)), cooperative-quad kernels (a vector per column quad(s); a
    // slab's samples are packed, so a vector brings the padding samples that end its last quad along).  Q = 1: one vector's workgroups per
    // compute unit.  An ensemble per vector (Q > 1) fills the device by itself (SWAP-02 x 512 nodes: 384 waves): as many vectors as the family
    // accepts samples for (rl_max_cols, cq_max_quads, dq_max_quads).  The candidate stands when the plan of a full launch AND of the last,
    // shorter one choose its family (dry runs: a grouped plan has no side effects).
    const int N = h->N;
    *why = "the kernel family of this plan keeps one tile stream per launch (grouped: row-lane and cooperative-quad kernels, column counts 1, 2, 4, 8, 16 or beyond 16)";
    for (int cand = 0; cand < 2; ++cand) {
        const bool rl = cand == 0;
        if (rl && (h->rl_npj == 0 || h->rl_max_cols < N)) continue;
        const jq_handle* t = (!rl && h->emb) ? h->emb : h;      // (the embedded twin serves what the row-lane kernels do not)
        if (!rl && t->parts == 1 && 16 % N != 0) continue;      // (samples that straddle column quads)
        const int upg = (!rl && t->parts > 1) ? 4 * t->parts * Q : (Q * N + 3) / 4;
        const int s1 = (!rl && t->parts == 1) ? 4 * upg / N : Q;
        long long gmax = rl ? h->rl_max_cols / (Q > 1 ? 4 * upg : N) : std::max(t->cq_max_quads, t->dq_max_quads) / upg;
        if (Q == 1) gmax = std::min<long long>(gmax, t->num_cu / upg);
        if (h->opt.has(O_PCOF_BATCH_MAX)) gmax = std::min<long long>(gmax, h->opt.get(O_PCOF_BATCH_MAX));
        gmax = std::min<long long>(gmax, npcof);
        if (gmax < 1) continue;
        bool ok = true;
        for (int G : {(int)gmax, npcof % (int)gmax}) {
            if (G == 0) continue;
            GateHold hold;
            BatchPlan p;
            if (plan_batch(eval_target(h, G * s1, false), G * s1, adjoint, false, hold, &p, G) != JQ_OK) return *why = "the batch plan refuses this evaluation (the single call reports why)", 0;
            if (G == (int)gmax) *family = (int)p.family;
            ok = ok && p.groups == G && p.upg == upg && p.family == (rl ? KF_ROWLANE : KF_CQ);
        }
        if (!ok) continue;
        *spg = s1;
        *why = rl ? "row-lane kernels: a control vector per wave(s)" : "cooperative-quad kernels: a control vector per column quad(s)";
        return (int)gmax;
    }
    return 0;
}

// npcof control vectors over ONE set of nquad nodes (nodes == weights == NULL, nquad == 1: the unperturbed sample) on this (single-device)
// handle: launches of at most `per` vectors as grouped batches where the plan allows (pcof_batch_per_launch; results do not depend on the
// round a vector runs in), else -- every route without grouped streams -- one plain evaluation per vector, the very request of the single call.
// put(i, res, g0, g1): column i of the caller's outputs from the records of its nquad samples and its gradients (g0: adjoint only, g1:
// objFuncType != 1 as well).  Timing: sums over the launches; every other field is the last launch's.
// What differs between the groups is the parameter: control vectors (drifts == NULL: pcofs holds npcof of them) or drift Hamiltonians
// (drifts: [Ntot x Ntot x npcof] members that drifts_prepare has tested against the plan, pcofs: ONE vector, nquad == 1).  A grouped launch
// of members hands run_eval their drifts; the sequential routes make member after member the handle's drift (apply_hconst: operator images
// only, no re-plan) for the single call's request and put the handle's own drift back at the end.
// ... and control mixes (mixes: [Nc x Nc x npcof], alone or together with drifts; pcofs: ONE vector, nquad == 1): a grouped launch hands
// run_eval the mixes of its members, the sequential routes give the single evaluation its member's mix -- no operator is swapped for a mix.
template <typename Put>
static int pcof_batch(jq_handle* h, const double* pcofs, int ncoeff, int npcof, const double* drifts, const double* mixes, const double* nodes,
                      const double* weights, int nquad, const double* shift, bool adjoint, Put&& put)
{
    int spg = 1, family = -1;
    const char* why = "";
    const int per = pcof_batch_per_launch(h, npcof, nquad, adjoint, &spg, &family, &why);
    const int step = per > 0 ? per : 1;
    const bool members = drifts || mixes;
    if (members) h->mb_mode = per > 0 ? "grouped" : "sequential", h->mb_why = why, h->mb_family = family, h->mb_per_launch = step, h->mb_drifts = drifts != nullptr, h->mb_mix = mixes != nullptr;
    if (drifts && !mixes) h->db_mode = per > 0 ? "grouped" : "sequential", h->db_why = why, h->db_family = family, h->db_per_launch = step;
    if (!members) h->pb_mode = per > 0 ? "grouped" : "sequential", h->pb_why = why, h->pb_family = family, h->pb_per_launch = step, h->pb_nodes = nquad;
    EvalRequest rq;
    rq.ncoeff = ncoeff, rq.nsamples = nquad, rq.eps = nodes, rq.wgt = weights, rq.shift = shift, rq.adjoint = adjoint;
    if (per > 0) rq.spg = spg, rq.nodes = nquad;
    const size_t nn = (size_t)h->Ntot * h->Ntot, ncnc = (size_t)h->Nc * h->Nc;
    const bool swap = drifts && per == 0;
    const std::vector<double> own = swap ? h->Hconst : std::vector<double>();
    struct Restore {      // (also when a member's evaluation fails)
        jq_handle* h;
        const std::vector<double>* own;
        ~Restore() { if (own) (void)apply_hconst(h, own->data()); }
    } restore{h, swap ? &own : nullptr};
    jq_timing tsum = {};
    for (int i0 = 0; i0 < npcof; i0 += step) {
        const int G = std::min(step, npcof - i0);      // (sequential: one vector, spg == 1)
        rq.pcof = members ? pcofs : pcofs + (size_t)ncoeff * i0;
        if (mixes) rq.mix = mixes + ncnc * i0;
        if (per > 0) rq.groups = G, rq.nsamples = G * spg;
        if (drifts && per > 0) rq.drifts = drifts + nn * i0;
        if (swap)
            if (int rc = apply_hconst(h, drifts + nn * i0)) return rc;
        EvalOut o;
        if (int rc = run_eval(h, rq, &o)) return rc;
        for (int g = 0; g < G; ++g)
            put(i0 + g, o.res.data() + (size_t)4 * g * spg, adjoint ? o.grad0.data() + (size_t)ncoeff * g : nullptr,
                (adjoint && h->objFuncType != 1) ? o.grad1.data() + (size_t)ncoeff * g : nullptr);
        timing_add(h->timing, tsum);      // (this launch's record + the sums so far)
        tsum = h->timing;
    }
    h->timing.ms_shard_min = h->timing.ms_shard_max = h->timing.ms_total;
    return JQ_OK;
}

extern "C" int jq_traceobjgrad_batch(jq_handle* h, const double* pcofs, int32_t ncoeff, int32_t npcof, int32_t evaladjoint, double* out4,
                                     double* totalgrad, double* infidelgrad, double* leakgrad)
{
    if (!h) return JQ_EINVAL;
    if (!pcofs || !out4) return fail(h, JQ_EINVAL, "jq_traceobjgrad_batch: NULL pointer");
    if (evaladjoint && (!totalgrad || !infidelgrad || !leakgrad))
        return fail(h, JQ_EINVAL, "jq_traceobjgrad_batch: gradient outputs are required when evaladjoint != 0");
    if (npcof < 1) return fail(h, JQ_EINVAL, "jq_traceobjgrad_batch: npcof must be >= 1");
    if (!h->subs.empty()) return multi_traceobjgrad_batch(h, pcofs, ncoeff, npcof, evaladjoint, out4, totalgrad, infidelgrad, leakgrad);
    if (int rc = check_ncoeff(h, ncoeff)) return rc;      // (before anything is written)
    return pcof_batch(h, pcofs, ncoeff, npcof, nullptr, nullptr, nullptr, nullptr, 1, nullptr, evaladjoint != 0, [&](int i, const double* res, const double* g0, const double* g1) {
        const size_t off = (size_t)ncoeff * i;
        out_record(out4 + (size_t)4 * i, res);
        if (evaladjoint) out_grads(h, ncoeff, g0, g1, totalgrad + off, infidelgrad + off, leakgrad + off);
    });
}

// An ensemble of nmember members under ONE control vector on a single-device handle: member i has the drift Hconsts[:, :, i] (NULL: the
// handle's) and the control mix ctrl_mix[:, :, i] (NULL: identity).  The two drifts calls are the ctrl_mix == NULL case.
// prepared: the caller has tested the member drifts against the plan -- a multi-device handle tests ALL members on every device before it
// shards them, so that the devices keep one plan
static int traceobjgrad_members_single(jq_handle* h, const double* pcof, int ncoeff, const double* Hconsts, const double* ctrl_mix, int nmember,
                                       int evaladjoint, bool prepared, double* out4, double* totalgrad, double* infidelgrad, double* leakgrad)
{
    if (int rc = check_ncoeff(h, ncoeff)) return rc;      // (before anything is written or re-planned)
    if (Hconsts && !prepared)
        if (int rc = drifts_prepare(h, Hconsts, nmember)) return rc;
    return pcof_batch(h, pcof, ncoeff, nmember, Hconsts, ctrl_mix, nullptr, nullptr, 1, nullptr, evaladjoint != 0, [&](int i, const double* res, const double* g0, const double* g1) {
        const size_t off = (size_t)ncoeff * i;
        out_record(out4 + (size_t)4 * i, res);
        if (evaladjoint) out_grads(h, ncoeff, g0, g1, totalgrad + off, infidelgrad + off, leakgrad + off);
    });
}

// the argument rules of the member entry points (who: the entry point's name; need_drifts: the drifts calls require Hconsts)
static int members_args(jq_handle* h, const char* who, bool need_drifts, const void* pcof, const double* Hconsts, const double* ctrl_mix, int nmember, const void* out)
{
    const std::string w(who);
    if (!pcof || !out || (need_drifts && !Hconsts)) return fail(h, JQ_EINVAL, (w + ": NULL pointer").c_str());
    if (!Hconsts && !ctrl_mix) return fail(h, JQ_EINVAL, (w + ": Hconsts and ctrl_mix are both NULL (the plain evaluation: jq_traceobjgrad)").c_str());
    if (nmember < 1) return fail(h, JQ_EINVAL, (w + ": the member count must be >= 1").c_str());
    if (ctrl_mix) {
        const int Nc = h->subs.empty() ? h->Nc : h->subs[0]->Nc;
        for (size_t e = 0; e < (size_t)Nc * Nc * nmember; ++e)
            if (!std::isfinite(ctrl_mix[e])) return fail(h, JQ_EINVAL, (w + ": a control mix entry is not finite").c_str());
    }
    return JQ_OK;
}

static int traceobjgrad_members(jq_handle* h, const char* who, bool need_drifts, const double* pcof, int ncoeff, const double* Hconsts, const double* ctrl_mix,
                                int nmember, int evaladjoint, double* out4, double* totalgrad, double* infidelgrad, double* leakgrad)
{
    if (int rc = members_args(h, who, need_drifts, pcof, Hconsts, ctrl_mix, nmember, out4)) return rc;
    if (evaladjoint && (!totalgrad || !infidelgrad || !leakgrad))
        return fail(h, JQ_EINVAL, (std::string(who) + ": gradient outputs are required when evaladjoint != 0").c_str());
    if (!h->subs.empty()) return multi_traceobjgrad_members(h, pcof, ncoeff, Hconsts, ctrl_mix, nmember, evaladjoint, out4, totalgrad, infidelgrad, leakgrad);
    return traceobjgrad_members_single(h, pcof, ncoeff, Hconsts, ctrl_mix, nmember, evaladjoint, false, out4, totalgrad, infidelgrad, leakgrad);
}

// the weighted sums of eval_f_g_grad! (src/ipopt_interface.jl:48-59) over the members of an ensemble instead of over eps-nodes: the
// members' columns from traceobjgrad_members, summed on the host in member order
static int eval_f_g_grad_members(jq_handle* h, const char* who, bool need_drifts, const double* pcof, int ncoeff, const double* Hconsts, const double* ctrl_mix,
                                 const double* weights, int nmember, int compute_adjoint, double* out2, double* infid_grad, double* leak_grad, double* member_out)
{
    if (!weights) return fail(h, JQ_EINVAL, (std::string(who) + ": NULL pointer").c_str());
    if (int rc = members_args(h, who, need_drifts, pcof, Hconsts, ctrl_mix, nmember, out2)) return rc;
    if (compute_adjoint && (!infid_grad || !leak_grad))
        return fail(h, JQ_EINVAL, (std::string(who) + ": gradient outputs are required when compute_adjoint != 0").c_str());
    if (int rc = check_ncoeff(h->subs.empty() ? h : h->subs[0], ncoeff)) {      // (before the temporaries are sized by it)
        if (!h->subs.empty()) h->err = h->subs[0]->err;
        return rc;
    }
    const size_t ng = compute_adjoint ? (size_t)ncoeff * nmember : 0;
    std::vector<double> rec((size_t)4 * nmember), tg(ng), ig(ng), lg(ng);
    const int rc = traceobjgrad_members(h, who, need_drifts, pcof, ncoeff, Hconsts, ctrl_mix, nmember, compute_adjoint, rec.data(), tg.data(), ig.data(), lg.data());
    if (rc) return rc;
    double inf = 0.0, leak = 0.0;
    for (int i = 0; i < nmember; ++i) {
        inf += rec[(size_t)4 * i + 1] * weights[i];      // (primaryobjf, secondaryobjf of the member's record)
        leak += rec[(size_t)4 * i + 2] * weights[i];
    }
    out2[0] = inf, out2[1] = leak;
    if (member_out) std::copy(rec.begin(), rec.end(), member_out);
    if (compute_adjoint) {
        std::fill_n(infid_grad, ncoeff, 0.0);
        std::fill_n(leak_grad, ncoeff, 0.0);
        for (int i = 0; i < nmember; ++i)
            for (int k = 0; k < ncoeff; ++k) {
                infid_grad[k] += weights[i] * ig[(size_t)ncoeff * i + k];
                leak_grad[k] += weights[i] * lg[(size_t)ncoeff * i + k];
            }
    }
    return JQ_OK;
}

extern "C" int jq_traceobjgrad_drifts(jq_handle* h, const double* pcof, int32_t ncoeff, const double* Hconsts, int32_t ndrift, int32_t evaladjoint,
                                      double* out4, double* totalgrad, double* infidelgrad, double* leakgrad)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_traceobjgrad_drifts", [&]() -> int {
        return traceobjgrad_members(h, "jq_traceobjgrad_drifts", true, pcof, ncoeff, Hconsts, nullptr, ndrift, evaladjoint, out4, totalgrad, infidelgrad, leakgrad);
    });
}

extern "C" int jq_eval_f_g_grad_drifts(jq_handle* h, const double* pcof, int32_t ncoeff, const double* Hconsts, const double* weights, int32_t ndrift,
                                       int32_t compute_adjoint, double* out2, double* infid_grad, double* leak_grad, double* member_out)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_eval_f_g_grad_drifts", [&]() -> int {
        return eval_f_g_grad_members(h, "jq_eval_f_g_grad_drifts", true, pcof, ncoeff, Hconsts, nullptr, weights, ndrift, compute_adjoint, out2, infid_grad, leak_grad, member_out);
    });
}

extern "C" int jq_traceobjgrad_members(jq_handle* h, const double* pcof, int32_t ncoeff, const double* Hconsts, const double* ctrl_mix, int32_t nmember,
                                       int32_t evaladjoint, double* out4, double* totalgrad, double* infidelgrad, double* leakgrad)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_traceobjgrad_members", [&]() -> int {
        return traceobjgrad_members(h, "jq_traceobjgrad_members", false, pcof, ncoeff, Hconsts, ctrl_mix, nmember, evaladjoint, out4, totalgrad, infidelgrad, leakgrad);
    });
}

extern "C" int jq_eval_f_g_grad_members(jq_handle* h, const double* pcof, int32_t ncoeff, const double* Hconsts, const double* ctrl_mix, const double* weights,
                                        int32_t nmember, int32_t compute_adjoint, double* out2, double* infid_grad, double* leak_grad, double* member_out)
{
    if (!h) return JQ_EINVAL;
    return abi_guard(h, "jq_eval_f_g_grad_members", [&]() -> int {
        return eval_f_g_grad_members(h, "jq_eval_f_g_grad_members", false, pcof, ncoeff, Hconsts, ctrl_mix, weights, nmember, compute_adjoint, out2, infid_grad, leak_grad, member_out);
    });
}

extern "C" int jq_state_history(jq_handle* h, const double* pcof, int32_t ncoeff, double* ur, double* ui)
{
    return jq_traceobj_verbose(h, pcof, ncoeff, nullptr, ur, ui);
}

extern "C" int jq_traceobj_verbose(jq_handle* h, const double* pcof, int32_t ncoeff, double* out4, double* ur, double* ui)
{
    if (!h) return JQ_EINVAL;
    if (!pcof || !ur || !ui) return fail(h, JQ_EINVAL, "jq_state_history: NULL pointer");
    JQ_ON_FIRST(h, jq_traceobj_verbose(s0_, pcof, ncoeff, out4, ur, ui))
    HIPCHK(h, hipSetDevice(h->device));
    const size_t len = (size_t)h->Ntot * h->N * (h->nsteps + 1);
    double *d_r = nullptr, *d_i = nullptr;
    HIPCHK(h, hipMalloc((void**)&d_r, len * sizeof(double)));
    if (hipMalloc((void**)&d_i, len * sizeof(double)) != hipSuccess) {
        (void)hipFree(d_r);
        return fail(h, JQ_ENOMEM, "jq_state_history: out of device memory");
    }
    (void)hipMemset(d_r, 0, len * sizeof(double));
    (void)hipMemset(d_i, 0, len * sizeof(double));
    EvalOut o;
    EvalRequest rq;
    rq.pcof = pcof, rq.ncoeff = ncoeff, rq.hist_r = d_r, rq.hist_i = d_i;
    int rc = run_eval(h, rq, &o);
    if (rc == JQ_OK) {
        if (hipMemcpy(ur, d_r, len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(ui, d_i, len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(h, JQ_EHIP, "jq_state_history: copy back failed");
        // usaver[:,:,1] = Uinit ; usavei[:,:,1] = -vi = 0 (src/evalobjgrad.jl:679-680)
        for (size_t i = 0; i < (size_t)h->Ntot * h->N && rc == JQ_OK; ++i) {
            ur[i] = h->Uinit[i];
            ui[i] = -0.0;
        }
        if (out4 && rc == JQ_OK) out_record(out4, o.res.data());   // the objective of the same forward sweep (src/evalobjgrad.jl:759-792)
    }
    (void)hipFree(d_r);
    (void)hipFree(d_i);
    return rc;
}

extern "C" int jq_state_populations(jq_handle* h, const double* pcof, int32_t ncoeff, const int32_t* group_of_row,
                                    int32_t ngroups, int32_t every, int32_t nout, double* pop, double* maxpop)
{
    if (!h) return JQ_EINVAL;
    if (!pcof) return fail(h, JQ_EINVAL, "jq_state_populations: NULL pointer");
    if (!pop && !maxpop) return fail(h, JQ_EINVAL, "jq_state_populations: pop and maxpop are both NULL");
    JQ_ON_FIRST(h, jq_state_populations(s0_, pcof, ncoeff, group_of_row, ngroups, every, nout, pop, maxpop))
    if (pop) {
        if (every < 1 || nout != h->nsteps / every + 1)
            return fail(h, JQ_EINVAL, "jq_state_populations: need every >= 1 and nout == nsteps/every + 1");
        if (ngroups < 1 || (!group_of_row && ngroups != h->Ntot))
            return fail(h, JQ_EINVAL, "jq_state_populations: ngroups must be Ntot when group_of_row is NULL");
        if (group_of_row)
            for (int r = 0; r < h->Ntot; ++r)
                if (group_of_row[r] >= ngroups) return fail(h, JQ_EINVAL, "jq_state_populations: group index >= ngroups");
    }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t len = (size_t)h->Ntot * h->N * (h->nsteps + 1);
    const size_t npop = pop ? (size_t)ngroups * h->N * nout : 0;
    double *d_r = nullptr, *d_i = nullptr, *d_pop = nullptr, *d_max = nullptr;
    int* d_grp = nullptr;
    int rc = JQ_OK;
    auto cleanup = [&]() {
        (void)hipFree(d_r); (void)hipFree(d_i); (void)hipFree(d_pop); (void)hipFree(d_max); (void)hipFree(d_grp);
    };
    if (hipMalloc((void**)&d_r, len * sizeof(double)) != hipSuccess || hipMalloc((void**)&d_i, len * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&d_pop, std::max<size_t>(npop, 1) * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&d_max, (size_t)h->Ntot * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&d_grp, (size_t)h->Ntot * sizeof(int)) != hipSuccess) {
        cleanup();
        return fail(h, JQ_ENOMEM, "jq_state_populations: out of device memory");
    }
    (void)hipMemset(d_r, 0, len * sizeof(double));
    (void)hipMemset(d_i, 0, len * sizeof(double));
    EvalOut o;
    EvalRequest rq;
    rq.pcof = pcof, rq.ncoeff = ncoeff, rq.hist_r = d_r, rq.hist_i = d_i;
    rc = run_eval(h, rq, &o);
    if (rc == JQ_OK) {
        // usaver[:,:,1] = Uinit ; usavei[:,:,1] = 0 (src/evalobjgrad.jl:679-680)
        bool ok = hipMemcpy(d_r, h->Uinit.data(), (size_t)h->Ntot * h->N * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
        if (pop && ok) {
            if (group_of_row) ok = hipMemcpy(d_grp, group_of_row, (size_t)h->Ntot * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
            const long long nthr = (long long)h->N * nout;
            hipLaunchKernelGGL(k_pop_groups, dim3((unsigned)((nthr + 127) / 128)), dim3(128), 0, h->stream, d_r, d_i, h->Ntot, h->N,
                               every, nout, group_of_row ? d_grp : nullptr, ngroups, d_pop);
        }
        if (maxpop && ok)
            hipLaunchKernelGGL(k_pop_max, dim3(h->Ntot), dim3(256), 0, h->stream, d_r, d_i, h->Ntot,
                               (long long)h->N * (h->nsteps + 1), d_max);
        ok = ok && hipStreamSynchronize(h->stream) == hipSuccess && hipGetLastError() == hipSuccess;
        if (pop && ok) ok = hipMemcpy(pop, d_pop, npop * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
        if (maxpop && ok) ok = hipMemcpy(maxpop, d_max, (size_t)h->Ntot * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
        if (!ok) rc = fail(h, JQ_EHIP, "jq_state_populations: device reduction or copy failed");
    }
    cleanup();
    return rc;
}

extern "C" int jq_eval_f_g_grad(jq_handle* h, const double* pcof, int32_t ncoeff, const double* nodes, const double* weights,
                                int32_t nquad, const double* shift, int32_t compute_adjoint, double* out2, double* infid_grad,
                                double* leak_grad)
{
    if (!h) return JQ_EINVAL;
    if (!pcof || !nodes || !weights || !out2) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad: NULL pointer");
    if (nquad < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad: nquad must be >= 1");
    if (compute_adjoint && (!infid_grad || !leak_grad))
        return fail(h, JQ_EINVAL, "jq_eval_f_g_grad: gradient outputs are required when compute_adjoint != 0");
    if (!h->subs.empty())
        return multi_eval_f_g_grad(h, pcof, ncoeff, nodes, weights, nquad, shift, compute_adjoint != 0, out2, infid_grad, leak_grad);
    EvalRequest rq;
    rq.pcof = pcof, rq.ncoeff = ncoeff, rq.nsamples = nquad, rq.eps = nodes, rq.wgt = weights, rq.shift = shift, rq.adjoint = compute_adjoint != 0;
    EvalOut o;
    int rc = run_eval(h, rq, &o);
    if (rc) return rc;
    double inf = 0.0, leak = 0.0;
    for (int i = 0; i < nquad; ++i) {  // src/ipopt_interface.jl:58-59
        inf += o.res[(size_t)i * 4 + 0] * weights[i];
        leak += o.res[(size_t)i * 4 + 1] * weights[i];
    }
    out2[0] = inf;
    out2[1] = leak;
    if (compute_adjoint) out_grads(h, ncoeff, o.grad0.data(), o.grad1.data(), nullptr, infid_grad, leak_grad);
    return JQ_OK;
}

extern "C" int jq_eval_f_g_grad_dev(jq_handle* h, const double* pcof, int32_t ncoeff, const double* nodes, const double* weights,
                                    int32_t nquad, const double* shift, int32_t compute_adjoint, void* d_packed)
{
    if (!h) return JQ_EINVAL;
    if (!pcof || !nodes || !weights || !d_packed) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_dev: NULL pointer");
    if (nquad < 0) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_dev: nquad must be >= 0");
    if (!h->subs.empty())
        return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_dev: multi-device handles reduce inside jq_eval_f_g_grad; use that entry");
    {   // the packed vector must live on the handle's GPU (a tensor allocated on torch's current device of a process that
        // created the handle on another one would hand k_pack a peer pointer)
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, d_packed) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_dev: d_packed is not a device pointer");
        }
        if (at.type != hipMemoryTypeDevice || at.device != h->device) {
            char buf[160];
            snprintf(buf, sizeof buf, "jq_eval_f_g_grad_dev: d_packed lives on device %d, the handle on device %d", at.device, h->device);
            return fail(h, JQ_EINVAL, buf);
        }
    }
    if (nquad == 0) {     // a rank without a shard contributes zeros to the all-reduce
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipMemsetAsync(d_packed, 0, (2 + 2 * (size_t)ncoeff) * sizeof(double), h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->timing = jq_timing{};
        return JQ_OK;
    }
    EvalRequest rq;
    rq.pcof = pcof, rq.ncoeff = ncoeff, rq.nsamples = nquad, rq.eps = nodes, rq.wgt = weights, rq.shift = shift, rq.adjoint = compute_adjoint != 0;
    rq.d_packed = (double*)d_packed;
    EvalOut o;
    return run_eval(h, rq, &o);
}

extern "C" int jq_traceobj_sweep(jq_handle* h, const double* pcof, int32_t ncoeff, const double* nodes, int32_t nquad,
                                 const double* shift, double* out)
{
    if (!h) return JQ_EINVAL;
    if (!pcof || !nodes || !out) return fail(h, JQ_EINVAL, "jq_traceobj_sweep: NULL pointer");
    if (nquad < 1) return fail(h, JQ_EINVAL, "jq_traceobj_sweep: nquad must be >= 1");
    if (!h->subs.empty()) return multi_traceobj_sweep(h, pcof, ncoeff, nodes, nquad, shift, out);
    EvalRequest rq;
    rq.pcof = pcof, rq.ncoeff = ncoeff, rq.nsamples = nquad, rq.eps = nodes, rq.shift = shift;
    EvalOut o;
    int rc = run_eval(h, rq, &o);
    if (rc) return rc;
    for (int i = 0; i < nquad; ++i) out_record(out + (size_t)i * 4, o.res.data() + (size_t)i * 4);
    return JQ_OK;
}

// jq_eval_f_g_grad for npcof control vectors and ONE set of nodes: grouped launches of G vectors x nquad nodes where the plan allows
// (pcof_batch_per_launch), else one ensemble evaluation per vector -- the very calls jq_eval_f_g_grad makes.
extern "C" int jq_eval_f_g_grad_batch(jq_handle* h, const double* pcofs, int32_t ncoeff, int32_t npcof, const double* nodes,
                                      const double* weights, int32_t nquad, const double* shift, int32_t compute_adjoint, double* out2,
                                      double* infid_grad, double* leak_grad, double* node_out)
{
    if (!h) return JQ_EINVAL;
    if (!pcofs || !nodes || !weights || !out2) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_batch: NULL pointer");
    if (npcof < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_batch: npcof must be >= 1");
    if (nquad < 1) return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_batch: nquad must be >= 1");
    if (compute_adjoint && (!infid_grad || !leak_grad))
        return fail(h, JQ_EINVAL, "jq_eval_f_g_grad_batch: gradient outputs are required when compute_adjoint != 0");
    if (!h->subs.empty())
        return multi_eval_f_g_grad_batch(h, pcofs, ncoeff, npcof, nodes, weights, nquad, shift, compute_adjoint, out2, infid_grad, leak_grad, node_out);
    if (int rc = check_ncoeff(h, ncoeff)) return rc;      // (before anything is written)
    // column i of the outputs from the records of its nquad samples (the sums in node order: src/ipopt_interface.jl:58-59)
    return pcof_batch(h, pcofs, ncoeff, npcof, nullptr, nullptr, nodes, weights, nquad, shift, compute_adjoint != 0, [&](int i, const double* res, const double* g0, const double* g1) {
        double inf = 0.0, leak = 0.0;
        for (int q = 0; q < nquad; ++q) {
            inf += res[(size_t)q * 4 + 0] * weights[q];
            leak += res[(size_t)q * 4 + 1] * weights[q];
            if (node_out) out_record(node_out + ((size_t)i * nquad + q) * 4, res + (size_t)q * 4);      // (the record of jq_traceobj_sweep)
        }
        out2[(size_t)2 * i] = inf, out2[(size_t)2 * i + 1] = leak;
        if (compute_adjoint) out_grads(h, ncoeff, g0, g1, nullptr, infid_grad + (size_t)ncoeff * i, leak_grad + (size_t)ncoeff * i);
    });
}

#include "jq_host_tl.h"      // what the drivers of the tangent-linear sweeps share: budgeting, stream generation, trace reduction, timing
#include "jq_host_jvp.h"      // jq_traceobj_jvp: the tangent of the forward map along directions of coefficient space
#include "jq_host_hvp.h"      // jq_traceobjgrad_hvp: the derivative of the gradient along directions of coefficient space
#include "jq_host_ens_hvp.h"      // jq_eval_f_g_grad_hvp: the same over the nodes of a risk-neutral ensemble (lane / row-lane kernels: one launch per chunk)
#include "jq_host_samples.h"      // controls given as samples on the time grid: the objective of a table pq, its gradient per entry, and (through the drivers above) Hessian-vector products along direction tables
#include "jq_host_samples_batch.h"      // ... in batches of tables and over member ensembles (drifts, control mixes) in one call
#include "jq_host_multi.h"      // multi-device handles: one process, N GPUs, one RCCL all-reduce
#include "jq_host_info.h"      // options of a live handle, plan and timing introspection
#ifdef JQ_DUMP_SELECTION
#include "jq_dump_selection.h"      // build/dump_selection: main() prints what every select_* function picks (no HIP call)
#endif
