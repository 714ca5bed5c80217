// jq_host_select.h -- part of the host side of libjuqbox_hip.so (included by juqbox_hip.hip, ONE translation unit; not a stand-alone header):
// the kernel instantiations (compiled in their own translation units, listed in jq_inst_list.h) and the functions that pick one.
// ---------------------------------------------------------------------------------------------
typedef void (*prop_kernel_t)(PropArgs);

// templates whose definitions the host does not include (jq_cq_kernels.h, jq_cq_split_kernels.h, jq_quad_split_kernels.h, jq_quad_imr_kernels.h,
// jq_cq_imr_kernels.h; jq_coop_imr_kernels.h; jq_quad_tl_kernels.h, whose kernels need the quad layout's row type)
template <int NT> __global__ void k_forward_quad_tl(PropArgs);
template <int NT> __global__ void k_backward_quad_tl(PropArgs);
template <int NT, bool MODD, int NS, bool WLR = false, bool DN = false> __global__ void k_forward_cq(PropArgs);
template <int NT, bool MODD, bool ORD, bool WLR = false, bool DN = false> __global__ void k_backward_cq(PropArgs);
template <int NT, bool MODD, bool ORD, int NR = 3, bool WLR = false, bool DN = false> __global__ void k_backward_cq3(PropArgs);
template <int NT, bool ORD, int QW, bool RIDE = false> __global__ void k_backward_qsplit(PropArgs);
template <int NT, int SPW> __global__ void k_forward_quad_imr(PropArgs);
template <int NT, int SPW> __global__ void k_backward_quad_imr(PropArgs);
template <int NT, bool DN = false> __global__ void k_forward_cq_imr(PropArgs);
template <int NT, bool DN = false> __global__ void k_backward_cq_imr(PropArgs);
template <int NT> __global__ void k_backward_cq_imr2(PropArgs);
template <int NT, bool DN = false> __global__ void k_backward_cq_imr3(PropArgs);
template <int NT, int BW, bool HBM> __global__ void k_forward_coop_imr(PropArgs);
template <int NT, int BW, bool HBM> __global__ void k_backward_coop_imr(PropArgs);
template <int NT, int BW, bool HBM> __global__ void k_forward_coop_imr_parts(PropArgs);
template <int NT, int BW, bool HBM> __global__ void k_backward_coop_imr_parts(PropArgs);

// Every instantiation of the list is compiled in its own object: declared here, so that none is instantiated into this translation unit ...
#define JQ_EXT(name, ...) extern template __global__ void name<__VA_ARGS__>(PropArgs);
#define JQ_EXT_FAMILY(letter, SIZES, INST) SIZES(INST, JQ_EXT)
JQ_OBJECT_FAMILIES(JQ_EXT_FAMILY)

// ... and a row of g_inst: its spelling, its template, the values of its template arguments (those left out: false) and the kernel.  A
// row without a kernel starts the rows of the objects with the letter it names.
struct KernelInst {
    const char *spelling, *name;
    int arg[8];
    prop_kernel_t fn;
};
#define JQ_ROW(name, ...) {#name "<" #__VA_ARGS__ ">", #name, {__VA_ARGS__}, name<__VA_ARGS__>},
#define JQ_ROW_FAMILY(letter, SIZES, INST) {nullptr, #letter, {}, nullptr}, SIZES(INST, JQ_ROW)
static const KernelInst g_inst[] = {JQ_OBJECT_FAMILIES(JQ_ROW_FAMILY)};

// What select_* chose (KernelSel, juqbox_hip.hip; jq_plan_info "last_kernels"): the objects (csrc/Makefile tags) of the two kernels and
// their compile-time variant.  pick() is the only way to a kernel: the instantiation name<args...> of the list -- none other can be
// named -- and, from the same row, the tag "<letter>_<a>[_<b>]" of the object that holds it; nullptr (tag untouched) when the list
// has no such instantiation.  A select_* function sets the flags of its record and picks by the very same values.
static void sel_tag(char* dst, char prefix, int a, int b)
{
    if (b >= 0) snprintf(dst, JQ_SEL_TAG, "%c_%d_%d", prefix, a, b);
    else snprintf(dst, JQ_SEL_TAG, "%c_%d", prefix, a);
}
static prop_kernel_t pick(char* tag, int a, int b, const char* name, std::initializer_list<int> args)
{
    int want[8] = {};
    std::copy(args.begin(), args.end(), want);
    char letter = 0;
    for (const KernelInst& r : g_inst) {
        if (!r.fn) letter = r.name[0];
        else if (strcmp(r.name, name) == 0 && std::equal(want, want + 8, r.arg)) return sel_tag(tag, letter, a, b), r.fn;
    }
    return nullptr;
}
static KernelSel sel_start()
{
    KernelSel s;
    s.set = true;
    return s;
}

static int select_kernels(jq_handle* h, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    const bool jac = (h->solver_id == 2), wlr = h->wrank > 0;      // (wlr: the low-rank full leakage weights compiled in, objects w_ / x_)
    *s = sel_start(), s->wlr = wlr;
    *fwd = pick(s->fwd, h->NT, h->BW, "k_forward", {h->NT, h->BW, JQ_MINW_OF(h->NT), jac, wlr});
    *bwd = pick(s->bwd, h->NT, h->BW, "k_backward", {h->NT, h->BW, JQ_MINW_OF(h->NT), jac, wlr});
    if (*fwd && *bwd && h->BW != JQ_BW_T4Q) return JQ_OK;      // (the quad layout is no band of a plan: select_quad_kernels)
    return fail(h, JQ_EUNSUPPORTED, wlr ? "full leakage weights (jq_update_wmat): no kernels with the low-rank terms for this plan (row-lane kernels "
                                          "disabled, or cooperative kernels that do not fit the LDS)"
                                        : "unsupported Hilbert dimension / band width");
}

// cooperative-quad (latency) kernels.  fwd2: the forward kernel with two column quads per workgroup (grid = 2 * nslabs); bwd_nr: workgroups
// per quad in the backward sweep (0 / 1: one; 2, 3: k_backward_cq3); wlr: full (real, low-rank) leakage weights; dense: no structure, NT = 2.
// (Instantiated for even and odd numbers of Neumann terms: the parities of the LDS exchange are compile-time constants.)
static int select_cq_kernels(jq_handle* h, bool fwd2, int bwd_nr, bool wlr, bool dense, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    const int nr = bwd_nr == 3 ? 3 : bwd_nr == 2 ? 2 : 1, ns = (fwd2 && !wlr) ? 2 : 1;
    const bool modd = (h->m > 0 ? h->m : 0) & 1;
    if (dense && (h->NT != 2 || wlr || fwd2)) return fail(h, JQ_EHIP, "internal error: dense cooperative-quad kernels selected for a plan they do not exist for");
    const bool ord = h->Nc <= 3 && !h->opt.on(O_CQ_GENERIC_TRACES) && ctrl_per_subsystem(h);      // (more than JQ_MAXNC controls: generic traces per group)
    *s = sel_start(), s->modd = modd, s->ord = ord && !dense, s->wlr = wlr, s->fwd2 = ns == 2, s->bwd_wgs = nr;
    *fwd = pick(s->fwd, h->NT, JQ_BW_T4Q, "k_forward_cq", {h->NT, modd, ns, wlr, dense});
    *bwd = nr == 1 ? pick(s->bwd, h->NT, JQ_BW_T4Q, "k_backward_cq", {h->NT, modd, s->ord, wlr, dense})
                   : pick(s->bwd, h->NT, JQ_BW_T4Q, "k_backward_cq3", {h->NT, modd, s->ord, nr, wlr, dense});
    return (*fwd && *bwd) ? JQ_OK : fail(h, JQ_EUNSUPPORTED, "unsupported Hilbert dimension");
}

static int select_quad_imr_kernels(jq_handle* h, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    *s = sel_start(), s->spw = 1;
    *fwd = pick(s->fwd, h->NT, JQ_BW_T4Q, "k_forward_quad_imr", {h->NT, s->spw});
    *bwd = pick(s->bwd, h->NT, JQ_BW_T4Q, "k_backward_quad_imr", {h->NT, s->spw});
    return (*fwd && *bwd) ? JQ_OK : fail(h, JQ_EUNSUPPORTED, "unsupported Hilbert dimension");
}

// three: the backward sweep on three workgroups per evaluation (as k_backward_cq3); two: with the state and the adjoint chain on two sets
// of waves (NT <= 6, LDS permitting; option imr_cq2=0: the one-set kernel of round 3)
static int select_cq_imr_kernels(jq_handle* h, bool two, bool three, bool dense, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    if (dense && (h->NT != 2 || two)) return fail(h, JQ_EHIP, "internal error: dense implicit-midpoint cooperative-quad kernels selected for a plan they do not exist for");
    *s = sel_start(), s->bwd_wgs = three ? 3 : 1;
    *fwd = pick(s->fwd, h->NT, JQ_BW_T4Q, "k_forward_cq_imr", {h->NT, dense});
    *bwd = three ? pick(s->bwd, h->NT, JQ_BW_T4Q, "k_backward_cq_imr3", {h->NT, dense}) : two ? pick(s->bwd, h->NT, JQ_BW_T4Q, "k_backward_cq_imr2", {h->NT}) : nullptr;
    s->imr_two = !three && *bwd;      // (no two-set kernel at NT = 7: the one-set kernel)
    if (!three && !*bwd) *bwd = pick(s->bwd, h->NT, JQ_BW_T4Q, "k_backward_cq_imr", {h->NT, dense});
    return (*fwd && *bwd) ? JQ_OK : fail(h, JQ_EUNSUPPORTED, "unsupported Hilbert dimension");
}

// quad-layout kernels of the JQ_BW_T4 structure (jq_kernels.h JQ_BW_T4Q): small batches, Neumann solver
// (spw: slabs per workgroup = waves per SIMD: workgroups of 4 spw waves)
static int select_quad_kernels(jq_handle* h, int spw, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    // one ensemble sample per wave (four columns of a slab): N a multiple of 4 (N <= 16 divides the slab into whole samples), or N > 16.
    // Only the twelve-wave BACKWARD kernel has a UNI variant: folding the shift into the MFMA's A operand adds a dependent FMA in front
    // of every MFMA, which three waves per SIMD hide (- 1.2 %) and one or two do not (measured: forward sweep + 1.2 %, one / two slabs
    // per workgroup + 1.6 ... 3.4 %)
    const bool uni = (h->N % 4 == 0 || h->parts > 1) && !h->opt.on(O_NO_UNI);
    // ... and its ORD variant when control q acts on subsystem q only (like the cooperative-quad kernels, select_cq_kernels)
    const bool ord = uni && h->Nc >= 2 && h->Nc <= 3 && !h->opt.on(O_NO_ORD) && ctrl_per_subsystem(h);
    // ... and, three slabs per workgroup, the SC variants when the plan's S images are uniform (s_image_uniform; option s_compact=0: the kernels
    // with the full operand, bit-identical): the forward kernel, and the ORD backward kernel
    const bool sc = spw == 3 && h->s_uniform && h->opt.on(O_S_COMPACT);
    *s = sel_start(), s->spw = spw == 3 ? 3 : spw == 2 ? 2 : 1;
    s->uni = spw == 3 && (ord || uni), s->ord = spw == 3 && ord, s->sc_fwd = sc, s->sc_bwd = sc && ord;
    *fwd = pick(s->fwd, h->NT, JQ_BW_T4Q, "k_forward", {h->NT, JQ_BW_T4Q, s->spw, false, false, false, s->sc_fwd});
    *bwd = pick(s->bwd, h->NT, JQ_BW_T4Q, "k_backward", {h->NT, JQ_BW_T4Q, s->spw, false, false, s->uni, s->ord, s->sc_bwd});
    return (*fwd && *bwd) ? JQ_OK : fail(h, JQ_EUNSUPPORTED, "unsupported Hilbert dimension");
}

// ... backward sweep with the state and the adjoint chain of a column quad on two waves, one time step apart (jq_quad_split_kernels.h):
// mid-size ensembles -- at most one column quad per SIMD (qw = 4 quads per workgroup: two waves per SIMD) or per two SIMDs (qw = 2).
// The backward kernel of a plan whose forward kernel select_quad_kernels / select_cq_kernels has recorded in *s.
static int select_qsplit_kernel(jq_handle* h, int qw, prop_kernel_t* bwd, KernelSel* s)
{
    // control q acts on subsystem q only (like select_quad_kernels / select_cq_kernels): compile-time trace modes
    const bool ord = h->Nc >= 2 && h->Nc <= 3 && !h->opt.on(O_NO_ORD) && ctrl_per_subsystem(h);
    // ... and with exactly three of them every trace product rides along in a pass of the adjoint step (RIDE; option qs_ride=0: separate passes)
    // -- where the adjoint wave is alone on its SIMD (qw = 2: - 6 %); with two waves per SIMD and the adjoint wave first in the issue
    // arbitration the rides buy nothing (248.9 ms without, 250.0 with): qw = 4 keeps the separate passes (bit-identical to the one-wave
    // kernel); option qs_ride=1 forces the rides there too
    const bool ride_set = h->opt.has(O_QS_RIDE);
    const long long ride_v = h->opt.get(O_QS_RIDE);
    const bool ride = ord && h->Nc == 3 && !(ride_set && ride_v == 0) && (qw == 2 || (ride_set && ride_v == 1));
    *bwd = pick(s->bwd, h->NT, JQ_BW_T4Q, "k_backward_qsplit", {h->NT, ride || ord, qw == 4 ? 4 : 2, ride});
    if (!*bwd) return fail(h, JQ_EUNSUPPORTED, "unsupported Hilbert dimension");
    s->qs_qw = qw == 4 ? 4 : 2, s->ord = ride || ord, s->ride = ride, s->uni = s->sc_bwd = false, s->bwd_wgs = 0;
    return JQ_OK;
}

// ... with the low-rank full leakage weights compiled in (jq_update_wmat; one slab per workgroup)
static int select_quad_w_kernels(jq_handle* h, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    *s = sel_start(), s->spw = 1, s->wlr = true;
    *fwd = pick(s->fwd, h->NT, JQ_BW_T4Q, "k_forward", {h->NT, JQ_BW_T4Q, s->spw, false, s->wlr});
    *bwd = pick(s->bwd, h->NT, JQ_BW_T4Q, "k_backward", {h->NT, JQ_BW_T4Q, s->spw, false, s->wlr});
    return (*fwd && *bwd) ? JQ_OK : fail(h, JQ_EUNSUPPORTED, "unsupported Hilbert dimension");
}

static int select_coop_kernels(jq_handle* h, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    *s = sel_start();
    if (h->huge) {      // (run-time sizes: compiled with the host code, no object of their own)
        *fwd = k_forward_huge, *bwd = k_backward_huge;
        snprintf(s->fwd, JQ_SEL_TAG, "host"), snprintf(s->bwd, JQ_SEL_TAG, "host");
        return JQ_OK;
    }
    *fwd = pick(s->fwd, h->NT, h->BWc, "k_forward_coop", {h->NT, h->BWc});
    *bwd = pick(s->bwd, h->NT, h->BWc, "k_backward_coop", {h->NT, h->BWc});
    return (*fwd && *bwd) ? JQ_OK : fail(h, JQ_EUNSUPPORTED, "no cooperative kernel for this Hilbert dimension / band width");
}

// lane kernels (one lane per column), NP = padded Hilbert dimension
static int select_lane_kernels(jq_handle* h, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    *s = sel_start();
    *fwd = pick(s->fwd, h->lane_np, -1, "k_forward_lane", {h->lane_np});
    *bwd = pick(s->bwd, h->lane_np, -1, "k_backward_lane", {h->lane_np});
    return (*fwd && *bwd) ? JQ_OK : fail(h, JQ_EUNSUPPORTED, "no lane kernel for this Hilbert dimension");
}

// row-lane kernels (one lane per (row, column)), NPJ = padded row length.  split: waves of the backward sweep (1, 2, 3)
static int select_rowlane_kernels(jq_handle* h, int split, bool hist, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    const int np = h->rl_npj;
    *s = sel_start(), s->wlr = h->wrank > 0;
    *fwd = pick(s->fwd, np, -1, "k_forward_rowlane", {np, s->wlr, s->wlr || hist});      // (full weights: the history if asked for)
    *bwd = s->wlr ? pick(s->bwd, np, -1, "k_backward_rowlane", {np, true}) : split == 3 ? pick(s->bwd, np, -1, "k_backward_rowlane3", {np})
         : split == 2 ? pick(s->bwd, np, -1, "k_backward_rowlane2", {np}) : pick(s->bwd, np, -1, "k_backward_rowlane", {np});
    return (*fwd && *bwd) ? JQ_OK : fail(h, JQ_EUNSUPPORTED, "no row-lane kernel for this Hilbert dimension");
}

static int select_rowlane_imr_kernels(jq_handle* h, bool split, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    *s = sel_start(), s->imr_two = split;
    *fwd = pick(s->fwd, h->rl_npj, -1, "k_forward_rowlane_imr", {h->rl_npj});
    *bwd = pick(s->bwd, h->rl_npj, -1, split ? "k_backward_rowlane_imr2" : "k_backward_rowlane_imr", {h->rl_npj});
    return (*fwd && *bwd) ? JQ_OK : fail(h, JQ_EUNSUPPORTED, "no implicit-midpoint kernel for this Hilbert dimension");
}

// cooperative kernels of the implicit-midpoint integrator; parts: N > 16, one workgroup per evaluation; hbm: dense 96 x 96 with the images
// read from HBM / L2 (i_6_5); <1, 0>: Ntot <= 16 with N > 4 (one wave per slab, the evaluation's columns in one wave)
static int select_coop_imr(jq_handle* h, bool parts, bool hbm, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s)
{
    const int nt = hbm ? 6 : h->NT, bw = hbm ? 5 : h->BWc;
    *s = sel_start();
    *fwd = pick(s->fwd, nt, bw, parts ? "k_forward_coop_imr_parts" : "k_forward_coop_imr", {nt, bw, hbm || nt > 6});
    *bwd = pick(s->bwd, nt, bw, parts ? "k_backward_coop_imr_parts" : "k_backward_coop_imr", {nt, bw, hbm || nt > 6});
    return (*fwd && *bwd) ? JQ_OK : fail(h, JQ_EUNSUPPORTED, "no cooperative implicit-midpoint kernel for this Hilbert dimension / band width");
}
static int select_coop_imr_parts_kernels(jq_handle* h, bool hbm, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s) { return select_coop_imr(h, true, hbm, fwd, bwd, s); }
static int select_coop_imr_kernels(jq_handle* h, bool hbm, prop_kernel_t* fwd, prop_kernel_t* bwd, KernelSel* s) { return select_coop_imr(h, false, hbm, fwd, bwd, s); }
