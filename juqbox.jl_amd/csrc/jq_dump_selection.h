// jq_dump_selection.h -- main() of build/dump_selection (juqbox_hip.hip compiled with -DJQ_DUMP_SELECTION; csrc/Makefile): the selection
// as data.  Calls every select_* function of jq_host_select.h with every combination of its arguments and of the handle fields and options
// it reads, on a handle filled by hand -- no HIP call, no device -- and prints what it picked.  tests/test_selection_table.py holds the
// output equal to profiles/selection_table.txt (profiles/README.md).
//
// Per function a line "# <function>: <names of its inputs>", then one line per RUN of combinations, in the order of the loops below (the
// last input varies fastest), that give the same outcome (a line per combination would be 37 000 lines):
//   <function> <inputs of the first combination of the run> x<combinations in the run> -> rc=<return code> fwd=<object> <instantiation>
//   bwd=<object> <instantiation> <the fields of the KernelSel record that are not zero>
// (the record and the kernels are printed for rc = 0 only).  The instantiation is the spelling of jq_inst_list.h, found by the kernel's
// pointer in g_inst; a pointer that no row holds prints as UNLISTED and the program exits with 1.
// `dump_selection --objects` prints the tag of every object the list names instead.
// JQ_DUMP_PARENT: select_* functions that leave their record in jq_handle::sel instead of taking it as their last argument.
#ifdef JQ_DUMP_PARENT
#define JQ_SELECT(s, fn, ...) (h.sel = s, dump_rc = fn(&h, __VA_ARGS__), s = h.sel, dump_rc)
#else
#define JQ_SELECT(s, fn, ...) fn(&h, __VA_ARGS__, &s)
#endif
static int dump_rc = 0, dump_unlisted = 0;

static const char* dump_spelling(const void* fn)
{
#define JQ_DUMP_ROW(name, ...) {#name "<" #__VA_ARGS__ ">", (const void*)name<__VA_ARGS__>},
    static const struct { const char* spelling; const void* fn; } other[] = {
        JQ_INST_HOST(JQ_DUMP_ROW)
        {"k_forward_huge", (const void*)k_forward_huge}, {"k_backward_huge", (const void*)k_backward_huge}};
#undef JQ_DUMP_ROW
    for (const KernelInst& r : g_inst)
        if (r.fn && (const void*)r.fn == fn) return r.spelling;
    for (const auto& r : other)
        if (r.fn == fn) return r.spelling;
    ++dump_unlisted;
    return "UNLISTED";
}

// a run of equal outcomes: printed when the outcome changes (or with `first` empty: flush)
static void dump_line(const std::string& first, const char* names, const std::string& outcome)
{
    static std::string run_first, run_outcome;
    static long run = 0;
    const bool same_fn = first.substr(0, first.find(' ')) == run_first.substr(0, run_first.find(' '));
    if (run && same_fn && outcome == run_outcome) {
        ++run;
        return;
    }
    if (run) printf("%s x%ld -> %s\n", run_first.c_str(), run, run_outcome.c_str());
    if (!same_fn && !first.empty()) printf("# %s: %s\n", first.substr(0, first.find(' ')).c_str(), names);
    run_first = first, run_outcome = outcome, run = first.empty() ? 0 : 1;
}
static void dump(const char* inputs, const char* names, int rc, const KernelSel& s, const void* fwd, const void* bwd)
{
    std::string o = "rc=" + std::to_string(rc);
    if (rc == 0) {
        if (fwd) o += std::string(" fwd=") + s.fwd + " " + dump_spelling(fwd);
        o += std::string(" bwd=") + s.bwd + " " + dump_spelling(bwd);
        const std::pair<const char*, int> ints[] = {{"spw", s.spw}, {"qs_qw", s.qs_qw}, {"bwd_wgs", s.bwd_wgs}};
        for (const auto& f : ints)
            if (f.second) o += std::string(" ") + f.first + "=" + std::to_string(f.second);
        const std::pair<const char*, bool> flags[] = {{"set", s.set}, {"uni", s.uni}, {"ord", s.ord}, {"sc_fwd", s.sc_fwd}, {"sc_bwd", s.sc_bwd},
                                                      {"ride", s.ride}, {"modd", s.modd}, {"fwd2", s.fwd2}, {"wlr", s.wlr}, {"imr_two", s.imr_two}};
        for (const auto& f : flags)
            if (f.second) o += std::string(" ") + f.first;
    }
    dump_line(inputs, names, o);
}

struct DumpSize { int a, b; };
#define JQ_DUMP_SIZE(A, ...) {__VA_ARGS__},
static void dump_controls(jq_handle& h, int Nc, bool single)      // single: control q acts on subsystem q only (ctrl_per_subsystem)
{
    h.Nc = Nc;
    h.bw_trace.assign(Nc, 7);
    for (int q = 0; q < Nc && single; ++q) h.bw_trace[q] = 1 << q;
}

static void dump_objects()
{
#define JQ_DUMP_TAG(letter, ...) { const int v[] = {__VA_ARGS__}; if (sizeof v > sizeof(int)) printf("%s_%d_%d\n", letter, v[0], v[1]); else printf("%s_%d\n", letter, v[0]); }
#define JQ_DUMP_TAG_FAMILY(letter, SIZES, INST) SIZES(JQ_DUMP_TAG, #letter)
    JQ_OBJECT_FAMILIES(JQ_DUMP_TAG_FAMILY)
}

int main(int argc, char** argv)
{
    if (argc > 1 && strcmp(argv[1], "--objects") == 0) return dump_objects(), 0;
    // (every size of the lists, and one that no object is built for; slab kernels: also the quad layout's code, which is no band of a plan)
    static const DumpSize slab[] = {JQ_SIZES_SLAB(JQ_DUMP_SIZE, ) {9, 1}, {8, JQ_BW_T4Q}}, coop[] = {JQ_SIZES_C(JQ_DUMP_SIZE, ) {1, 0}}, coop_imr[] = {JQ_SIZES_I(JQ_DUMP_SIZE, ) {17, 1}};
    static const DumpSize lane[] = {JQ_SIZES_LANE(JQ_DUMP_SIZE, ) {3, 0}}, rowlane[] = {JQ_SIZES_ROWLANE(JQ_DUMP_SIZE, ) {3, 0}};
    const long long ride_values[] = {JQ_OPT_UNSET, 0, 1};
    char in[256];
    prop_kernel_t f, b;
    jq_handle h;
    KernelSel s;
    for (const DumpSize& z : slab)
        for (int solver = 1; solver <= 2; ++solver)
            for (int wrank = 0; wrank <= 1; ++wrank) {
                h.NT = z.a, h.BW = z.b, h.solver_id = solver, h.wrank = wrank, s = KernelSel();
                const int rc = JQ_SELECT(s, select_kernels, &f, &b);
                snprintf(in, sizeof in, "select_kernels %d %d %d %d", z.a, z.b, solver, wrank);
                dump(in, "NT BW solver_id wrank", rc, s, (const void*)f, (const void*)b);
            }
    h = jq_handle();
    for (int NT = 1; NT <= 8; ++NT)
        for (int dense = 0; dense <= 1; ++dense)
            for (int wlr = 0; wlr <= 1; ++wlr)
                for (int fwd2 = 0; fwd2 <= 1; ++fwd2)
                    for (int nr = 0; nr <= 3; ++nr)
                        for (int m = 0; m <= 1; ++m)
                            for (int generic = 0; generic <= 1; ++generic)
                                for (int single = 0; single <= 1; ++single)
                                    for (int Nc = 1; Nc <= 4; ++Nc) {
                                        h.NT = NT, h.m = m, h.opt.v[O_CQ_GENERIC_TRACES] = generic, s = KernelSel();
                                        dump_controls(h, Nc, single);
                                        const int rc = JQ_SELECT(s, select_cq_kernels, fwd2, nr, wlr, dense, &f, &b);
                                        snprintf(in, sizeof in, "select_cq_kernels %d %d %d %d %d %d %d %d %d",
                                                 NT, dense, wlr, fwd2, nr, m, generic, single, Nc);
                                        dump(in, "NT dense wlr fwd2 bwd_nr m cq_generic_traces single_subsystem Nc", rc, s, (const void*)f, (const void*)b);
                                    }
    h = jq_handle();
    for (int NT = 1; NT <= 9; ++NT) {
        h.NT = NT, s = KernelSel();
        const int rc = JQ_SELECT(s, select_quad_imr_kernels, &f, &b);
        snprintf(in, sizeof in, "select_quad_imr_kernels %d", NT);
        dump(in, "NT", rc, s, (const void*)f, (const void*)b);
    }
    for (int NT = 1; NT <= 8; ++NT)
        for (int dense = 0; dense <= 1; ++dense)
            for (int three = 0; three <= 1; ++three)
                for (int two = 0; two <= 1; ++two) {
                    h.NT = NT, s = KernelSel();
                    const int rc = JQ_SELECT(s, select_cq_imr_kernels, two, three, dense, &f, &b);
                    snprintf(in, sizeof in, "select_cq_imr_kernels %d %d %d %d", NT, dense, three, two);
                    dump(in, "NT dense three two", rc, s, (const void*)f, (const void*)b);
                }
    for (int NT = 1; NT <= 9; ++NT)
        for (int spw = 1; spw <= 3; ++spw)
            for (int s_uniform = 0; s_uniform <= 1; ++s_uniform)
                for (int s_compact = 0; s_compact <= 1; ++s_compact)
                    for (int no_uni = 0; no_uni <= 1; ++no_uni)
                        for (int N = 3; N <= 4; ++N)
                            for (int parts = 1; parts <= 2; ++parts)
                                for (int no_ord = 0; no_ord <= 1; ++no_ord)
                                    for (int single = 0; single <= 1; ++single)
                                        for (int Nc = 1; Nc <= 4; ++Nc) {
                                            h.NT = NT, h.N = N, h.parts = parts, h.s_uniform = s_uniform, s = KernelSel();
                                            h.opt.v[O_NO_UNI] = no_uni, h.opt.v[O_NO_ORD] = no_ord, h.opt.v[O_S_COMPACT] = s_compact;
                                            dump_controls(h, Nc, single);
                                            const int rc = JQ_SELECT(s, select_quad_kernels, spw, &f, &b);
                                            snprintf(in, sizeof in, "select_quad_kernels %d %d %d %d %d %d %d %d %d %d",
                                                     NT, spw, s_uniform, s_compact, no_uni, N % 4, parts, no_ord, single, Nc);
                                            dump(in, "NT spw s_uniform s_compact no_uni N%4 parts no_ord single_subsystem Nc", rc, s, (const void*)f, (const void*)b);
                                        }
    h = jq_handle();
    for (int NT = 1; NT <= 7; ++NT)
        for (int qw = 2; qw <= 4; qw += 2)
            for (long long ride : ride_values)
                for (int no_ord = 0; no_ord <= 1; ++no_ord)
                    for (int single = 0; single <= 1; ++single)
                        for (int Nc = 1; Nc <= 4; ++Nc) {
                            h.NT = NT, h.opt.v[O_NO_ORD] = no_ord, h.opt.v[O_QS_RIDE] = ride;
                            dump_controls(h, Nc, single);
                            // (amends the record of the plan's forward kernel: here one with every field it resets set)
                            s = KernelSel(), s.set = s.uni = s.sc_bwd = true, s.bwd_wgs = 1, snprintf(s.fwd, JQ_SEL_TAG, "fwd"), snprintf(s.bwd, JQ_SEL_TAG, "bwd");
                            const int rc = JQ_SELECT(s, select_qsplit_kernel, qw, &b);
                            snprintf(in, sizeof in, "select_qsplit_kernel %d %d %s %d %d %d", NT, qw, ride == JQ_OPT_UNSET ? "unset" : ride ? "1" : "0",
                                     no_ord, single, Nc);
                            dump(in, "NT qw qs_ride no_ord single_subsystem Nc", rc, s, nullptr, (const void*)b);
                        }
    h = jq_handle();
    for (int NT = 1; NT <= 9; ++NT) {
        h.NT = NT, s = KernelSel();
        const int rc = JQ_SELECT(s, select_quad_w_kernels, &f, &b);
        snprintf(in, sizeof in, "select_quad_w_kernels %d", NT);
        dump(in, "NT", rc, s, (const void*)f, (const void*)b);
    }
    for (int huge = 0; huge <= 1; ++huge)
        for (const DumpSize& z : coop) {
            h.NT = z.a, h.BWc = z.b, h.huge = huge, s = KernelSel();
            const int rc = JQ_SELECT(s, select_coop_kernels, &f, &b);
            snprintf(in, sizeof in, "select_coop_kernels %d %d %d", huge, z.a, z.b);
            dump(in, "huge NT BWc", rc, s, (const void*)f, (const void*)b);
        }
    for (const DumpSize& z : lane) {
        h.lane_np = z.a, s = KernelSel();
        const int rc = JQ_SELECT(s, select_lane_kernels, &f, &b);
        snprintf(in, sizeof in, "select_lane_kernels %d", z.a);
        dump(in, "lane_np", rc, s, (const void*)f, (const void*)b);
    }
    for (const DumpSize& z : rowlane)
        for (int wrank = 0; wrank <= 1; ++wrank)
            for (int split = 1; split <= 3; ++split)
                for (int hist = 0; hist <= 1; ++hist) {
                    h.rl_npj = z.a, h.wrank = wrank, s = KernelSel();
                    const int rc = JQ_SELECT(s, select_rowlane_kernels, split, hist, &f, &b);
                    snprintf(in, sizeof in, "select_rowlane_kernels %d %d %d %d", z.a, wrank, split, hist);
                    dump(in, "rl_npj wrank split hist", rc, s, (const void*)f, (const void*)b);
                }
    for (const DumpSize& z : rowlane)
        for (int split = 0; split <= 1; ++split) {
            h.rl_npj = z.a, s = KernelSel();
            const int rc = JQ_SELECT(s, select_rowlane_imr_kernels, split, &f, &b);
            snprintf(in, sizeof in, "select_rowlane_imr_kernels %d %d", z.a, split);
            dump(in, "rl_npj split", rc, s, (const void*)f, (const void*)b);
        }
    for (int parts = 0; parts <= 1; ++parts)
        for (int hbm = 0; hbm <= 1; ++hbm)
            for (const DumpSize& z : coop_imr) {
                h.NT = z.a, h.BWc = z.b, s = KernelSel();
                const int rc = parts ? JQ_SELECT(s, select_coop_imr_parts_kernels, hbm, &f, &b) : JQ_SELECT(s, select_coop_imr_kernels, hbm, &f, &b);
                snprintf(in, sizeof in, "%s %d %d %d", parts ? "select_coop_imr_parts_kernels" : "select_coop_imr_kernels", hbm, z.a, z.b);
                dump(in, "hbm NT BWc", rc, s, (const void*)f, (const void*)b);
            }
    dump_line("", "", "");
    if (dump_unlisted) fprintf(stderr, "dump_selection: %d kernel pointer(s) that jq_inst_list.h does not list\n", dump_unlisted);
    return dump_unlisted ? 1 : 0;
}
