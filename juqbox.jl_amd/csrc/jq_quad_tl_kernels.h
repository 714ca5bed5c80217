// jq_quad_tl_kernels.h -- tangent-linear twins of the quad-layout kernels (jq_kernels.h, JQ_BW_T4Q) for jq_eval_f_g_grad_hvp:
// Hessian-vector products of risk-neutral ensembles on the 4 x 4 x n structure at Ntot > 16 (NT = 2 .. 6 blocks of 16 rows), four
// columns per wave, one 16-row block per register, Arr<NT> per vector, one grid row per direction.
//
// hv(alpha; d) = d/d eps grad(alpha + eps d) at eps = 0 of the gradient the Stormer-Verlet sweeps compute, obtained by differentiating
// the step line by line, exactly as jq_lane_tl_kernels.h and jq_rowlane_tl_kernels.h do (their kernels are the template of the
// algorithm): truncation of the Neumann series included, not symmetrised.
//
// Geometry: a wave = one quad of four columns (column = ensemble node x initial condition, consecutive -- a node's columns may share a
// quad with another node's; padding columns carry eps 0, weight 0 and a zero state), lane 16 i + 4 b + j <-> row 16 mt + 4 b + i of
// block mt, column j of the quad (the operand layout of v_mfma_f64_4x4x4_4b, mm_t4q).  blockIdx.y = the direction.  A workgroup is
// blockDim.x / 64 (1 .. JQ_QUAD_TL_WAVES) consecutive quads of ONE direction: quad blockIdx.x * waves + wave; a wave past the last
// quad only takes part in the staging.
// The chunk holds P + gridDim.y operator streams of T4 images (P = a.nprimal), a.stream_gstride doubles apart: groups 0 .. P - 1 at
// pcof (one per member of a drift ensemble, a.group_units quads each, a workgroup holds quads of one member; P = 1: one stream for
// every quad), group P + j generated
// by k_ctrl / k_stream with direction j as the coefficient vector and a zero drift image -- the controls are linear in the
// coefficients, so that stream IS the derivative of the primal one.  Members with a control mix (a.tl_dirs_per_member) bring the streams of
// their own directions: P + P gridDim.y streams, member g's direction j at P + g gridDim.y + j.  Every product is mm_t4q on an image of one of the two, and
//     y = c + M x   has the tangent   yd = cd + M xd + Md x      (two more mm_t4q).
// The node shift does not depend on the coefficients and differs between the columns of a quad: it is applied per lane to the
// results (cw = c eps ws[row], as QuadImr::cw), never folded into the MFMA operand; its tangent term is cw xd.  The Horner chain is
// differentiated inside its loop.  The trace images Hsym_q, Hanti_q are constant (yd = M xd) and multiplied in the T4 mode of their
// control (a.bw_trace).  A direction reads its own stream and its own block of the state file and nothing else, and a wave's
// arithmetic does not depend on the workgroup it sits in: a direction's bits do not depend on the launch or round it rides in.
//
// Operator images.  Both streams are the same for every quad of a direction (the shift is not in them), so the quads of a workgroup
// share ONE pair of rings in LDS: per stream three time points of (K, S) -- the integer points t_n, t_n+1 in two alternating slots and
// the half point between them -- filled at the top of a step by the workgroup's own global -> LDS DMA (1 KiB pieces dealt round
// robin to its waves), and every product reads its A operands and coefficient records from LDS where it stands, as the gradient
// kernels do.  Reading them from the streams instead would put an L2 round trip in front of each of the ~ 140 products of a
// backward step.  A deeper ring (a step ahead, as RlRing) does not fit next to the constant images at NT = 6 with four controls
// (5 points x 2 streams x 12 KiB + 48 KiB > 160 KiB); three points and the constants are 120 KiB, so a step opens with the DMA of
// its two new time points (48 pieces, ~ 2 us against a step of several tens of us) between two barriers.
// Dynamic LDS: [ring of the primal stream | ring of the direction's stream | constant images Hsym_q, Hanti_q (backward sweep)].
//
// State file of one direction (a.state_stride doubles, [row][quad][64 lanes] in the lane order above):
//     U, V, MU, NB | Ud, Vd, MUd, NBd (NT rows each) | carry[JQ_MAXNC] | d(carry)[JQ_MAXNC] | leak
// Trace records: [direction][quad][step][Ncoupled JQ_NTR], the primal one first, the tangents' one gridDim.y a.nslabs rows behind
// it; both in the layout k_trace_reduce / k_gradacc read.
#pragma once

#define JQ_QUAD_TL_WAVES 4                                            // most quads per workgroup (one wave per SIMD: 512 registers)
#define JQ_QUAD_TL_ROWS(nt) (8 * (nt) + 2 * JQ_MAXNC + 1)             // rows of 64 doubles per quad in one direction's state file
#define JQ_QUAD_TL_RINGS(stride) ((size_t)2 * 3 * 2 * (stride) * sizeof(double))      // bytes of both rings; the backward sweep adds 2 Nc images

#if defined(JQ_BW) && JQ_BW == 7
#include "jq_kernels.h"

// the two rings of a workgroup: [primal stream of its member | direction blockIdx.y], slots [t even | t odd | half point] of [K | S] each
template <int NT>
struct QtlRings {
    static constexpr int IMG = JQ_T4_ELEMS(NT), PIECES = IMG / 128, SLOT_B = 2 * IMG * 8, RING_B = 3 * SLOT_B;
    static_assert(IMG % 128 == 0, "a T4 image is a whole number of 1 KiB pieces");
    const double* lds;      // the primal ring with this lane's offset; the direction's ring 6 IMG doubles behind it
    unsigned lds0;          // ... as an LDS address (M0 of the DMA)
    unsigned lo16;          // 16 x lane
    const char *srcp, *srcd;
    int wave, nwv;

    __device__ __forceinline__ void dma(unsigned dst, const char* s) const
    {
        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(dst), "v"(lo16), "s"(s) : "memory");
    }
    // time point tp of both streams -> slot: this wave's share of the 2 PIECES pieces
    __device__ __forceinline__ void issue(int tp, int slot) const
    {
        const size_t so = (size_t)tp * SLOT_B;
        const unsigned ro = lds0 + (unsigned)slot * SLOT_B;
        for (int p = wave; p < 2 * PIECES; p += nwv) {
            dma(ro + p * 1024u, srcp + so + (size_t)p * 1024);
            dma(ro + RING_B + p * 1024u, srcd + so + (size_t)p * 1024);
        }
    }
    __device__ __forceinline__ void init(const PropArgs& a, double* ring, int lane, int wave_, int nwv_)
    {
        lds = ring + lane;
        lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) char*)ring;
        lo16 = 16u * lane;
        // (the workgroup's quads belong to ONE member: a.group_units is a multiple of the quads per workgroup)
        srcp = (const char*)jq_group_stream(a, (int)blockIdx.x * nwv_);
        srcd = (const char*)jq_tl_dir_stream(a, (int)blockIdx.x * nwv_);
        wave = wave_, nwv = nwv_;
        issue(0, 0);
    }
    // top of step n: every wave is through step n - 1; the time points 2n + 1, 2n + 2 of both streams land before anybody reads them
    __device__ __forceinline__ void issue_step(int n) const
    {
        __syncthreads();
        issue(2 * n + 1, 2);
        issue(2 * n + 2, (n + 1) & 1);
    }
    __device__ __forceinline__ void land() const
    {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    __device__ __forceinline__ void begin_step(int n) const
    {
        issue_step(n);
        land();
    }
};
// the six operator images of step n of one stream (the member names of RowOps), lane offset applied
struct QtlOps {
    const double *Kn0, *S0, *Kp05, *S05, *Kn1, *S1;
    template <int NT>
    __device__ __forceinline__ QtlOps(const QtlRings<NT>& r, int n, int stream)
    {
        constexpr int IMG = QtlRings<NT>::IMG;
        const double* b = r.lds + stream * (6 * IMG);
        const double *e0 = b + (n & 1) * (2 * IMG), *e1 = b + ((n + 1) & 1) * (2 * IMG), *o = b + 4 * IMG;
        Kn0 = e0, S0 = e0 + IMG, Kp05 = o, S05 = o + IMG, Kn1 = e1, S1 = e1 + IMG;
    }
};

__device__ __forceinline__ void qtl_phase() { __builtin_amdgcn_sched_barrier(0); }
#define JQ_QTL_FULL (JQ_T4_DIAG | JQ_T4_RTERMS | JQ_T4_MTERMS)

// A right-hand side enters every product as a fresh value: left alone the compiler shares the lane-shifted copies of a vector (mm_t4q:
// two per block) between all the products it enters and keeps them from one to the next -- three times the registers of the step.
template <int NT>
__device__ __forceinline__ Arr<NT> qtl_fresh(const Arr<NT>& x)
{
    Arr<NT> r = x;
#pragma unroll
    for (int i = 0; i < NT; ++i) asm volatile("" : "+v"(r.t[i][0]));
    return r;
}
// ... and an image is read anew by every product: the images of a step do not change between its products, so the compiler would keep the
// operands of all twelve (60 registers each at NT = 6) from one use to the next.  (An opaque ZERO offset, not an opaque pointer: the
// pointers must stay visibly LDS addresses -- ds_read, not flat loads; QuadImr::apply.)
__device__ __forceinline__ const double* qtl_anew(const double* M)
{
    int z = 0;
    asm volatile("" : "+v"(z));
    return M + z;
}
// D = M x with a constant image in the T4 mode of its control
template <int NT, int MODE>
__device__ __forceinline__ void qmz(Arr<NT>& D, const double* M, const Arr<NT>& x)
{
    const Arr<NT> xo = qtl_fresh(x);
    mm_t4q<NT, true, MODE>(D, D, qtl_anew(M), xo);
}
// y = c + M x ; yd = cd + M xd + Md x   (the tangent is formed from the old x first: y, yd may be the variables c, cd or x, xd came from)
template <int NT, bool ZEROC>
__device__ __forceinline__ void qmv2(Arr<NT>& y, Arr<NT>& yd, const Arr<NT>& c, const Arr<NT>& cd, const double* M, const double* Md,
                                     const Arr<NT>& x, const Arr<NT>& xd)
{
    const Arr<NT> xo = qtl_fresh(x), xdo = qtl_fresh(xd);
    Arr<NT> t;
    mm_t4q<NT, ZEROC, JQ_QTL_FULL>(t, cd, qtl_anew(M), xdo);
    qtl_phase();
    mm_t4q<NT, false, JQ_QTL_FULL>(t, t, qtl_anew(Md), xo);
    qtl_phase();
    mm_t4q<NT, ZEROC, JQ_QTL_FULL>(y, c, qtl_anew(M), xo);
    qtl_phase();
    yd = t;
}
// y += (+-) cw .* x and its tangent (cw: this lane's c eps ws[row] or forcing weight per block; no tangent of its own)
template <int NT, bool NEG>
__device__ __forceinline__ void qaxpy2(Arr<NT>& y, Arr<NT>& yd, const double* cw, const Arr<NT>& x, const Arr<NT>& xd)
{
    a_axpy_cw<NT, NEG>(y, cw, x);
    a_axpy_cw<NT, NEG>(yd, cw, xd);
}
// out = bpa + sum_{j=1..m} S^j A and its tangent
template <int NT>
__device__ __forceinline__ void qhorner2(Arr<NT>& out, Arr<NT>& outd, const Arr<NT>& bpa, const Arr<NT>& bpad, const Arr<NT>& A, const Arr<NT>& Ad,
                                         const double* S, const double* Sd, int m)
{
    if (m <= 0) {
        out = bpa;
        outd = bpad;
        return;
    }
    Arr<NT> Y = A, Yd = Ad;
    for (int j = 1; j < m; ++j) qmv2<NT, false>(Y, Yd, A, Ad, S, Sd, Y, Yd);
    qmv2<NT, false>(out, outd, bpa, bpad, S, Sd, Y, Yd);
}
template <int NT>
__device__ __forceinline__ void qsum(Arr<NT>& s, const Arr<NT>& x, const Arr<NT>& y)
{
#pragma unroll
    for (int i = 0; i < NT; ++i) s.t[i] = x.t[i] + y.t[i];
}
template <int NT>
__device__ __forceinline__ void qtl_load(Arr<NT>& x, const double* st, size_t rs, int arr)
{
#pragma unroll
    for (int i = 0; i < NT; ++i) x.t[i][0] = st[(size_t)(arr * NT + i) * rs];
}
template <int NT>
__device__ __forceinline__ void qtl_store(const Arr<NT>& x, double* st, size_t rs, int arr)
{
#pragma unroll
    for (int i = 0; i < NT; ++i) st[(size_t)(arr * NT + i) * rs] = x.t[i][0];
}

// the Stormer-Verlet state step and its tangent (row_state_tl in the quad layout; o: the primal images, od: the direction's)
template <int NT>
__device__ __forceinline__ void quad_state_tl(int m, const QtlOps& o, const QtlOps& od, const double* cw, const Arr<NT>& u, const Arr<NT>& v,
                                              const Arr<NT>& ud, const Arr<NT>& vd, Arr<NT>& un, Arr<NT>& v05, Arr<NT>& vnew, Arr<NT>& und,
                                              Arr<NT>& v05d, Arr<NT>& vnewd)
{
    Arr<NT> A, Ad, b, bd;
    qmv2<NT, true>(A, Ad, u, ud, o.Kp05, od.Kp05, u, ud);
    qaxpy2<NT, false>(A, Ad, cw, u, ud);
    qmv2<NT, false>(A, Ad, A, Ad, o.S05, od.S05, v, vd);
    qsum(b, v, A);
    qsum(bd, vd, Ad);
    qhorner2<NT>(v05, v05d, b, bd, A, Ad, o.S05, od.S05, m);
    qmv2<NT, false>(vnew, vnewd, v05, v05d, o.S05, od.S05, v05, v05d);      // vN
    qtl_phase();
    qmv2<NT, false>(un, und, u, ud, o.Kn0, od.Kn0, v05, v05d);
    qaxpy2<NT, true>(un, und, cw, v05, v05d);
    qmv2<NT, false>(un, und, un, und, o.S0, od.S0, u, ud);
    qmv2<NT, true>(A, Ad, u, ud, o.Kn1, od.Kn1, v05, v05d);
    qaxpy2<NT, true>(A, Ad, cw, v05, v05d);
    qtl_phase();
    qmv2<NT, false>(A, Ad, A, Ad, o.S1, od.S1, un, und);
    qsum(b, un, A);
    qsum(bd, und, Ad);
    qhorner2<NT>(un, und, b, bd, A, Ad, o.S1, od.S1, m);
    qmv2<NT, false>(vnew, vnewd, vnew, vnewd, o.Kp05, od.Kp05, un, und);
    qaxpy2<NT, false>(vnew, vnewd, cw, un, und);
    qtl_phase();
}

#define JQ_QUAD_TL_PROLOGUE                                                                                                       \
    extern __shared__ __attribute__((aligned(16))) double lds_qtl[];                                                              \
    const int lane = threadIdx.x & 63;                                                                                            \
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;                                     \
    const long long nw = a.nslabs, w = (long long)blockIdx.x * nwv + wave;                                                        \
    const bool active = w < nw;                                                                                                   \
    const long long col = 4 * (active ? w : 0) + (lane & 3);                                                                      \
    const int rowb = 4 * ((lane >> 2) & 3) + (lane >> 4);      /* this lane's row in a block */                                   \
    const size_t rs = (size_t)nw * 64;                         /* doubles per row of the state file */                            \
    double* st = a.state + (size_t)blockIdx.y * (size_t)a.state_stride + (size_t)(active ? w : 0) * 64 + lane;                    \
    const double ceps = (active && a.use_shift) ? 0.5 * a.h * a.colinfo[col] : 0.0;                                               \
    double wdr[NT], cw[NT];                                                                                                       \
    _Pragma("unroll") for (int i = 0; i < NT; ++i)                                                                                \
    {                                                                                                                             \
        wdr[i] = a.tabs[16 * i + rowb];                                                                                           \
        cw[i] = ceps * a.tabs[16 * NT + 16 * i + rowb];                                                                           \
    }                                                                                                                             \
    QtlRings<NT> rings;                                                                                                           \
    rings.init(a, lds_qtl, lane, wave, nwv);

// Forward sweep of (state, tangent) over one chunk.  grid = (ceil(quads / waves), directions), block = 64 waves
template <int NT>
__global__ __launch_bounds__(64 * JQ_QUAD_TL_WAVES) void k_forward_quad_tl(PropArgs a)
{
    JQ_QUAD_TL_PROLOGUE
    constexpr int LEAK = JQ_QUAD_TL_ROWS(NT) - 1;
    Arr<NT> u, v, ud, vd;
    a_zero(u), a_zero(v), a_zero(ud), a_zero(vd);
    double leak = 0.0;
    if (active) {
        qtl_load(u, st, rs, 0), qtl_load(v, st, rs, 1), qtl_load(ud, st, rs, 4), qtl_load(vd, st, rs, 5);
        leak = st[(size_t)LEAK * rs];
    }
    for (int n = 0; n < a.nsteps_chunk; ++n) {
        rings.begin_step(n);
        if (!active) continue;      // (a wave without a quad only takes part in the staging)
        const QtlOps o(rings, n, 0), od(rings, n, 1);
        Arr<NT> un, v05, vnew, und, v05d, vnewd;
#pragma unroll
        for (int i = 0; i < NT; ++i) leak = fma(wdr[i], u.t[i][0] * u.t[i][0], leak);
        quad_state_tl<NT>(a.m, o, od, cw, u, v, ud, vd, un, v05, vnew, und, v05d, vnewd);
        u = un, v = vnew, ud = und, vd = vnewd;
#pragma unroll
        for (int i = 0; i < NT; ++i) leak = fma(wdr[i], u.t[i][0] * u.t[i][0] + 2.0 * v05.t[i][0] * v05.t[i][0], leak);
    }
    if (!active) return;
    qtl_store(u, st, rs, 0), qtl_store(v, st, rs, 1), qtl_store(ud, st, rs, 4), qtl_store(vd, st, rs, 5);
    st[(size_t)LEAK * rs] = leak;
}

// per-lane partial of tr(x' y) over this lane's rows
template <int NT>
__device__ __forceinline__ double qdot(const Arr<NT>& x, const Arr<NT>& y)
{
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) s = fma(x.t[i][0], y.t[i][0], s);
    return s;
}
// The trace scalars of the controls and their tangents (product rule on the two state factors; the images are constant), in two stages,
// each as soon as its factors exist, so that u, ud leave the registers before the adjoint chain: stage A (after X) t1, t2, t3, stage B
// (after the adjoint step) t4 with the carry and t5.  Per-lane parts, weighted and summed over the wave; MODE: the control's T4 mode.
template <int NT, int MODE>
__device__ __forceinline__ void quad_traces_a(const double* Hs, const double* Ha, const Arr<NT>& X, const Arr<NT>& Xd, const Arr<NT>& u,
                                              const Arr<NT>& ud, const Arr<NT>& un, const Arr<NT>& und, const Arr<NT>& v05, const Arr<NT>& v05d,
                                              double* out)
{
    Arr<NT> Y, Yd;
    qmz<NT, MODE>(Y, Ha, X);
    qmz<NT, MODE>(Yd, Ha, Xd);
    out[0] = qdot(u, Y), out[3] = qdot(ud, Y) + qdot(u, Yd);
    out[2] = qdot(un, Y), out[5] = qdot(und, Y) + qdot(un, Yd);
    qtl_phase();
    qmz<NT, MODE>(Y, Hs, X);
    qmz<NT, MODE>(Yd, Hs, Xd);
    out[1] = qdot(v05, Y), out[4] = qdot(v05d, Y) + qdot(v05, Yd);
    qtl_phase();
}
template <int NT, int MODE>
__device__ __forceinline__ void quad_traces_b(const double* Hs, const double* Ha, const Arr<NT>& nb, const Arr<NT>& nbd, const Arr<NT>& nbn,
                                              const Arr<NT>& nbnd, const Arr<NT>& un, const Arr<NT>& und, const Arr<NT>& v05, const Arr<NT>& v05d,
                                              double* out)
{
    Arr<NT> Y, Yd;
    {
        Arr<NT> B;
        qsum(B, nb, nbn);
        qmz<NT, MODE>(Y, Ha, B);
        qsum(B, nbd, nbnd);
        qmz<NT, MODE>(Yd, Ha, B);
    }
    out[1] = -qdot(v05, Y), out[3] = -(qdot(v05d, Y) + qdot(v05, Yd));      // t5
    qtl_phase();
    qmz<NT, MODE>(Y, Hs, nbn);
    qmz<NT, MODE>(Yd, Hs, nbnd);
    out[0] = -qdot(un, Y), out[2] = -(qdot(und, Y) + qdot(un, Yd));         // p4
    qtl_phase();
}
#define JQ_QTL_BY_MODE(mode, fn, ...)                                       \
    switch (mode) {                                                         \
    case JQ_T4_DIAG: fn<NT, JQ_T4_DIAG>(__VA_ARGS__); break;                \
    case JQ_T4_RTERMS: fn<NT, JQ_T4_RTERMS>(__VA_ARGS__); break;            \
    case JQ_T4_MTERMS: fn<NT, JQ_T4_MTERMS>(__VA_ARGS__); break;            \
    default: fn<NT, JQ_QTL_FULL>(__VA_ARGS__); break;                       \
    }

// Backward sweep of (state, adjoint) and their tangents over one chunk: the backward step of the quad-layout kernels in dual-number
// arithmetic, in the order k_backward_rowlane_tl spells it out.  The constant images Hsym_q, Hanti_q (a.cimg) live in LDS behind the rings.
template <int NT>
__global__ __launch_bounds__(64 * JQ_QUAD_TL_WAVES) void k_backward_quad_tl(PropArgs a)
{
    JQ_QUAD_TL_PROLOGUE
    constexpr int IMG = QtlRings<NT>::IMG, CARRY0 = 8 * NT;
    const int Nc = a.Ncoupled;
    const int modes = a.bw_trace[0] | (a.bw_trace[1] << 4) | (a.bw_trace[2] << 8) | (a.bw_trace[3] << 12);
    double* lds_c = lds_qtl + 12 * IMG;
    for (int i = threadIdx.x; i < 2 * Nc * IMG; i += blockDim.x) lds_c[i] = a.cimg[i];
    __syncthreads();
    const double* cl = lds_c + lane;
    const double wgt = active ? a.colinfo[4 * nw + col] : 0.0;
    const double cf = a.forced ? 0.5 * a.h * a.tinv : 0.0;
    double cfw[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) cfw[i] = cf * wdr[i];
    // (v, vd are not carried in registers: a step reads them from the state file while its operator images land and writes the new ones
    //  back as soon as the state step has them -- 24 registers at NT = 6 that the adjoint chain and the traces need)
    Arr<NT> u, mu, nb, ud, mud, nbd;
    a_zero(u), a_zero(mu), a_zero(nb), a_zero(ud), a_zero(mud), a_zero(nbd);
    double carry[JQ_MAXNC] = {0.0, 0.0, 0.0, 0.0}, carryd[JQ_MAXNC] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        qtl_load(u, st, rs, 0), qtl_load(mu, st, rs, 2), qtl_load(nb, st, rs, 3);
        qtl_load(ud, st, rs, 4), qtl_load(mud, st, rs, 6), qtl_load(nbd, st, rs, 7);
#pragma unroll
        for (int q = 0; q < JQ_MAXNC; ++q)
            if (q < Nc) {
                carry[q] = st[(size_t)(CARRY0 + q) * rs];
                carryd[q] = st[(size_t)(CARRY0 + JQ_MAXNC + q) * rs];
            }
    }
    const size_t ntr = (size_t)Nc * JQ_NTR;
    double* trw = a.traces + (((size_t)blockIdx.y * nw + (active ? w : 0)) * a.nsteps_chunk) * ntr;
    double* trwd = trw + (size_t)gridDim.y * nw * a.nsteps_chunk * ntr;

    if (a.first_chunk && active) {
        // per-lane part of carry_q = tr(vr' Hsym_q lambdai) at t = T (see k_backward) and of its tangent; summed with the traces
#pragma unroll
        for (int q = 0; q < JQ_MAXNC; ++q)
            if (q < Nc) {
                Arr<NT> T, Td;
                qmz<NT, JQ_QTL_FULL>(T, cl + (size_t)q * IMG, nb);
                qmz<NT, JQ_QTL_FULL>(Td, cl + (size_t)q * IMG, nbd);
                carry[q] = -qdot(u, T);
                carryd[q] = -(qdot(ud, T) + qdot(u, Td));
            }
    }

    for (int n = 0; n < a.nsteps_chunk; ++n) {
        rings.issue_step(n);
        Arr<NT> v, vd;
        a_zero(v), a_zero(vd);
        if (active) qtl_load(v, st, rs, 1), qtl_load(vd, st, rs, 5);
        rings.land();
        if (!active) continue;      // (a wave without a quad only takes part in the staging)
        const QtlOps o(rings, n, 0), od(rings, n, 1);
        Arr<NT> un, v05, und, v05d;
        {
            Arr<NT> vnew, vnewd;
            quad_state_tl<NT>(a.m, o, od, cw, u, v, ud, vd, un, v05, vnew, und, v05d, vnewd);
            qtl_store(vnew, st, rs, 1), qtl_store(vnewd, st, rs, 5);
        }
        double* tr = trw + (size_t)n * ntr;
        double* trd = trwd + (size_t)n * ntr;
        // adjoint step and its tangent
        Arr<NT> X, Xd, nbn, nbnd;
        {
            Arr<NT> R, Rd, b, bd;
            qmv2<NT, true>(R, Rd, nb, nbd, o.Kp05, od.Kp05, nb, nbd);
            qaxpy2<NT, false>(R, Rd, cw, nb, nbd);
            qmv2<NT, false>(R, Rd, R, Rd, o.S0, od.S0, mu, mud);
            qaxpy2<NT, false>(R, Rd, cfw, u, ud);
            qsum(b, mu, R);
            qsum(bd, mud, Rd);
            qhorner2<NT>(X, Xd, b, bd, R, Rd, o.S0, od.S0, a.m);
        }
        qtl_phase();
        // traces, stage A: t1, t2, t3 of every control in ONE reduction each for the values and the tangents (lane 16 r: the r-th sum)
#pragma unroll 1
        for (int q = 0; q < Nc; ++q) {
            const double *Hs = cl + (size_t)q * IMG, *Ha = cl + (size_t)(Nc + q) * IMG;
            double t[6];
            JQ_QTL_BY_MODE((modes >> (4 * q)) & 15, quad_traces_a, Hs, Ha, X, Xd, u, ud, un, und, v05, v05d, t)
            const double ts = wave_sum4_rows(t[0] * wgt, t[1] * wgt, t[2] * wgt, 0.0);
            const double tsd = wave_sum4_rows(t[3] * wgt, t[4] * wgt, t[5] * wgt, 0.0);
            if ((lane & 15) == 0 && lane < 48) {
                tr[q * JQ_NTR + (lane >> 4)] = ts;
                trd[q * JQ_NTR + (lane >> 4)] = tsd;
            }
        }
        qtl_phase();
        {
            Arr<NT> L, Ld, Qv, Qd, P, Pd;
            qmv2<NT, true>(L, Ld, X, Xd, o.Kn0, od.Kn0, X, Xd);
            qaxpy2<NT, true>(L, Ld, cw, X, Xd);
            qmv2<NT, true>(Qv, Qd, X, Xd, o.Kn1, od.Kn1, X, Xd);
            qaxpy2<NT, true>(Qv, Qd, cw, X, Xd);
            qmv2<NT, true>(P, Pd, nb, nbd, o.S05, od.S05, nb, nbd);
            qaxpy2<NT, true>(P, Pd, cfw, v05, v05d);
            a_add(L, P), a_add(Ld, Pd);
            a_add(Qv, P), a_add(Qd, Pd);
            qtl_phase();
            qmv2<NT, false>(Qv, Qd, Qv, Qd, o.S05, od.S05, L, Ld);
            qsum(P, nb, L);
            qsum(Pd, nbd, Ld);
            a_add(P, Qv), a_add(Pd, Qd);
            qhorner2<NT>(nbn, nbnd, P, Pd, Qv, Qd, o.S05, od.S05, a.m);
        }
        qtl_phase();
        // (mu <- G = X + K05 nbn + S1 X + forcing: X, Xd end here)
        qmv2<NT, false>(mu, mud, X, Xd, o.Kp05, od.Kp05, nbn, nbnd);
        qaxpy2<NT, false>(mu, mud, cw, nbn, nbnd);
        qmv2<NT, false>(mu, mud, mu, mud, o.S1, od.S1, X, Xd);
        qaxpy2<NT, false>(mu, mud, cfw, un, und);
        qtl_phase();
        // traces, stage B: t4 (with the carry) and t5 of a control and their tangents in one reduction (lanes 0, 16 | 32, 48)
#pragma unroll 1
        for (int q = 0; q < Nc; ++q) {
            const double *Hs = cl + (size_t)q * IMG, *Ha = cl + (size_t)(Nc + q) * IMG;
            double t[4];
            JQ_QTL_BY_MODE((modes >> (4 * q)) & 15, quad_traces_b, Hs, Ha, nb, nbd, nbn, nbnd, un, und, v05, v05d, t)
            double cq = 0.0, cqd = 0.0;
#pragma unroll
            for (int k = 0; k < JQ_MAXNC; ++k) {
                cq = (q == k) ? carry[k] : cq;
                cqd = (q == k) ? carryd[k] : cqd;
            }
            const double ts = wave_sum4_rows((t[0] + cq) * wgt, t[1] * wgt, (t[2] + cqd) * wgt, t[3] * wgt);
#pragma unroll
            for (int k = 0; k < JQ_MAXNC; ++k) {
                carry[k] = (q == k) ? t[0] : carry[k];
                carryd[k] = (q == k) ? t[2] : carryd[k];
            }
            if ((lane & 15) == 0) (lane < 32 ? tr : trd)[q * JQ_NTR + 3 + ((lane >> 4) & 1)] = ts;
        }
        u = un, nb = nbn;
        ud = und, nbd = nbnd;
    }
    if (!active) return;
    qtl_store(u, st, rs, 0), qtl_store(mu, st, rs, 2), qtl_store(nb, st, rs, 3);
    qtl_store(ud, st, rs, 4), qtl_store(mud, st, rs, 6), qtl_store(nbd, st, rs, 7);
#pragma unroll
    for (int q = 0; q < JQ_MAXNC; ++q)
        if (q < Nc) {
            st[(size_t)(CARRY0 + q) * rs] = carry[q];
            st[(size_t)(CARRY0 + JQ_MAXNC + q) * rs] = carryd[q];
        }
}
#endif
