// jq_tl_kernels.h -- tangent-linear Stormer-Verlet forward sweep (jq_traceobj_jvp): correctness first.
//
// The pair (state, tangent) = ((u, v), (ud, vd)) goes through the forward step of k_forward_huge (jq_huge_kernels.h)
// in dual-number arithmetic: every update D = C + M x of the state step is accompanied by Dd = Cd + M xd + Md x, where Md is the operator
// derivative along a direction d of coefficient space at the same time point.  p_k, q_k and the uncoupled ft are linear in the
// coefficients, so the pre-scaled images of Md are exactly the tile stream k_ctrl + k_stream generate from the coefficient vector d with
// an all-zero drift image: the launch reads TWO streams in lock-step, the primal one (group 0 of the chunk, shared by every workgroup) and
// the one of its direction (group 1 + dir, stream_gstride doubles apart).  The Horner form of the Neumann series is differentiated as it
// is executed (y_k = A + S y_{k+1}  ->  yd_k = Ad + Sd y_{k+1} + S yd_{k+1}), so the tangent is the exact derivative of what the device
// computes, truncated series included.  Three MFMAs per MFMA of the state step.
//
// Geometry and data placement are the run-time-size kernels': the tile-row count NT is a run-time number, one workgroup of 16 waves per
// 16-column slab (N > 16: `parts` slabs per direction), wave w owns the tile rows w, w + 16, ..., the vectors of a step are [KT][64]
// arrays in a per-slab work area in global memory, operators are dense v_mfma_f64_16x16x4 tiles read from the tile stream, two workgroup
// barriers per product.  The primal state is recomputed per direction: a direction's arithmetic does not depend on how many directions a
// launch carries.  Neumann solver and Diagonal weights only (the host refuses everything else); no ensemble shift.
#pragma once
#include "jq_huge_kernels.h"

enum { TV_UN, TV_V05, TV_VN, TV_A, TV_Y, TV_YB, TV_SPARE, TV_COUNT };      // work-area vectors per slab: TV_COUNT primal, then TV_COUNT tangent
#define JQ_TL_STATE_ROWS(KT) (4 * (KT) + 2)      // 64-double rows of a slab's state file: u, v, ud, vd [KT] each, leak, d(leak)

struct Tl {
    int NT, KT, wave, lane, g, m;
    double* work;               // this slab's work area: primal vector i at work + i KT 64, its tangent TV_COUNT vectors behind
    OpCursor cur, curd;         // primal stream, stream of this workgroup's direction
    const double *M, *Md;       // current operator image and its derivative (lane offset applied): tile (mt, kk) at (mt KT + kk) 64
    const double* wd;           // [16 NT] diagonal leakage weights in natural row order
    __device__ __forceinline__ double* vec(int i) const { return work + (size_t)i * KT * 64; }
    __device__ __forceinline__ double* dvec(int i) const { return work + (size_t)(TV_COUNT + i) * KT * 64; }
    template <class F>
    __device__ __forceinline__ void each(F f) const
    {
        for (int mt = wave; mt < NT; mt += JQ_HUGE_WAVES)
#pragma unroll
            for (int r = 0; r < 4; ++r) f((size_t)(4 * mt + r) * 64 + lane, 16 * mt + 4 * r + g);
    }
    __device__ __forceinline__ void next_op() { M = cur.next(), Md = curd.next(); }
    // D = C + M x ; Dd = Cd + M xd + Md x  (C == nullptr: no C, Cd).  D, Dd must not be x, xd; C may be D, Cd may be Dd.
    // Barriers: x, xd complete on entry, all reads done on exit.
    __device__ __forceinline__ void mm2(double* D, double* Dd, const double* C, const double* Cd, const double* x, const double* xd) const
    {
        __syncthreads();
        for (int mt = wave; mt < NT; mt += JQ_HUGE_WAVES) {
            d4 acc = {0.0, 0.0, 0.0, 0.0}, accd = {0.0, 0.0, 0.0, 0.0};
            if (C)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc[r] = C[(size_t)(4 * mt + r) * 64 + lane];
                    accd[r] = Cd[(size_t)(4 * mt + r) * 64 + lane];
                }
            const double *Mr = M + (size_t)mt * KT * 64, *Mdr = Md + (size_t)mt * KT * 64;
            for (int kk = 0; kk < KT; ++kk) {
                const double a = Mr[(size_t)kk * 64], ad = Mdr[(size_t)kk * 64], b = x[(size_t)kk * 64 + lane], bd = xd[(size_t)kk * 64 + lane];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                accd = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bd, accd, 0, 0, 0);
                accd = __builtin_amdgcn_mfma_f64_16x16x4f64(ad, b, accd, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                D[(size_t)(4 * mt + r) * 64 + lane] = acc[r];
                Dd[(size_t)(4 * mt + r) * 64 + lane] = accd[r];
            }
        }
        __syncthreads();
    }
    // sum over this lane's own elements of wd[row] a[e] b[e]
    __device__ __forceinline__ double wdot(const double* a, const double* b) const
    {
        double s = 0.0;
        each([&](size_t e, int row) { s += wd[row] * (a[e] * b[e]); });
        return s;
    }
    // out = bpa + sum_{j=1..m} S^j A with the current operator, in Huge::horner's Horner form, and its tangent.  out may be bpa; out, bpa
    // must not be A or a work vector Y, YB, SPARE (the same for the tangents).
    __device__ __forceinline__ void horner2(double* out, double* outd, const double* bpa, const double* bpad, const double* A, const double* Ad)
    {
        if (m <= 0) {
            if (out != bpa) each([&](size_t e, int) { out[e] = bpa[e]; outd[e] = bpad[e]; });
            return;
        }
        const double *src = A, *srcd = Ad;
        int dst = TV_Y;
        for (int j = 1; j < m; ++j) {
            mm2(vec(dst), dvec(dst), A, Ad, src, srcd);
            src = vec(dst), srcd = dvec(dst);
            dst = (dst == TV_Y) ? TV_YB : TV_Y;
        }
        mm2(vec(TV_SPARE), dvec(TV_SPARE), bpa, bpad, src, srcd);
        const double *res = vec(TV_SPARE), *resd = dvec(TV_SPARE);
        each([&](size_t e, int) { out[e] = res[e]; outd[e] = resd[e]; });
    }
    // one time step of (state, tangent): the seven operator uses Kp05 S05 Kn0 Kn1 S0 S1 Kp05 of the cooperative forward schedule
    //   in: u, v, ud, vd   out: vectors TV_UN, TV_V05, TV_VN (= the new u, v05, the new v) and their tangents
    __device__ __forceinline__ void step(const double* u, const double* v, const double* ud, const double* vd)
    {
        double *un = vec(TV_UN), *v05 = vec(TV_V05), *vN = vec(TV_VN), *A = vec(TV_A);
        double *und = dvec(TV_UN), *v05d = dvec(TV_V05), *vNd = dvec(TV_VN), *Ad = dvec(TV_A);
        next_op();      // use 0: Kp05 -- A = c K05 u
        mm2(A, Ad, nullptr, nullptr, u, ud);
        next_op();      // use 1: S05 -- A = c (K05 u + S05 v) ; v05 = v + sum_j S^j A ; vN = v05 + S05 v05
        mm2(A, Ad, A, Ad, v, vd);
        each([&](size_t e, int) { v05[e] = v[e] + A[e]; v05d[e] = vd[e] + Ad[e]; });
        horner2(v05, v05d, v05, v05d, A, Ad);
        mm2(vN, vNd, v05, v05d, v05, v05d);
        next_op();      // use 2: Kn0 -- un = u - c K0 v05
        mm2(un, und, u, ud, v05, v05d);
        next_op();      // use 3: Kn1 -- A = -c K1 v05
        mm2(A, Ad, nullptr, nullptr, v05, v05d);
        next_op();      // use 4: S0 -- un = u + c (S0 u - K0 v05)
        mm2(un, und, un, und, u, ud);
        next_op();      // use 5: S1 -- A = c (S1 un - K1 v05) ; un += sum_j S^j A
        mm2(A, Ad, A, Ad, un, und);
        each([&](size_t e, int) { un[e] += A[e]; und[e] += Ad[e]; });
        horner2(un, und, un, und, A, Ad);
        next_op();      // use 6: Kp05 -- v(t+h) = v05 + c (K05 u_new + S05 v05)
        mm2(vN, vNd, vN, vNd, un, und);
    }
};

// Forward sweep of (state, tangent) over one chunk: workgroup b = slab b % parts of direction b / parts.
//   a.stream: the chunk's tile streams, group 0 primal, group 1 + dir the direction's; a.state: [workgroups][JQ_TL_STATE_ROWS(KT)][64];
//   a.park: work areas [workgroups][2 TV_COUNT][KT][64]; a.tabs: wd[16 NT]
// (a template with one instantiation, WAVES = JQ_HUGE_WAVES, so that jq_inst_list.h can name it like every other propagator kernel)
template <int WAVES = JQ_HUGE_WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_forward_tl(PropArgs a)
{
    static_assert(WAVES == JQ_HUGE_WAVES, "Tl strides the tile rows by JQ_HUGE_WAVES");
    __shared__ double scratch[WAVES * 64];
    Tl tl;
    tl.NT = (a.Ntot + 15) / 16;
    tl.KT = 4 * tl.NT;
    tl.lane = threadIdx.x & 63;
    tl.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    tl.g = tl.lane >> 4;
    tl.m = a.m;
    tl.work = a.park + (size_t)blockIdx.x * 2 * TV_COUNT * tl.KT * 64;
    tl.cur.init(nullptr, a, 0, 0, 0);
    tl.curd.init(nullptr, a, 0, 0, 0);
    tl.curd.stream = a.stream + (size_t)(1 + (int)blockIdx.x / a.parts) * (size_t)a.stream_gstride;
    tl.M = tl.Md = nullptr;
    tl.wd = a.tabs;
    const int KT = tl.KT;
    double* st = a.state + (size_t)blockIdx.x * a.state_stride;
    double *u = st, *v = st + (size_t)KT * 64, *ud = st + (size_t)2 * KT * 64, *vd = st + (size_t)3 * KT * 64;
    const double *un = tl.vec(TV_UN), *v05 = tl.vec(TV_V05), *vN = tl.vec(TV_VN);
    const double *und = tl.dvec(TV_UN), *v05d = tl.dvec(TV_V05), *vNd = tl.dvec(TV_VN);
    double leak = 0.0, dleak = 0.0;
    for (int n = 0; n < a.nsteps_chunk; ++n) {
        leak += tl.wdot(u, u);      // trapezoidal part at t_n (src/evalobjgrad.jl:700) and its derivative
        dleak += 2.0 * tl.wdot(u, ud);
        tl.step(u, v, ud, vd);
        tl.each([&](size_t e, int) { u[e] = un[e]; v[e] = vN[e]; ud[e] = und[e]; vd[e] = vNd[e]; });
        leak += tl.wdot(u, u) + 2.0 * tl.wdot(v05, v05);      // (:716, penalf2a :2170-2180)
        dleak += 2.0 * tl.wdot(u, ud) + 4.0 * tl.wdot(v05, v05d);
    }
    huge_wg_sum_store(leak, scratch, &st[(size_t)(4 * KT) * 64], tl.wave, tl.lane, true);
    huge_wg_sum_store(dleak, scratch, &st[(size_t)(4 * KT + 1) * 64], tl.wave, tl.lane, true);
}

// state files <- (Uinit, 0, 0, 0, 0, 0); grid = workgroups of the sweep, block = 64.  uimg: the handle's slab image of Uinit, whose
// columns beyond N repeat the first N when N <= 16 (parts == 1): here they stay zero, a slab holds ONE copy of the evaluation.
__global__ void k_init_tl(double* state, long long stride, const double* __restrict__ uimg, int KT, int parts, int N)
{
    double* st = state + (size_t)blockIdx.x * stride;
    const int lane = threadIdx.x;
    const bool on = parts > 1 || (lane & 15) < N;
    uimg += (size_t)(blockIdx.x % parts) * KT * 64;
    for (int kk = 0; kk < KT; ++kk) {
        st[kk * 64 + lane] = on ? uimg[kk * 64 + lane] : 0.0;
        st[(KT + kk) * 64 + lane] = 0.0;
        st[(2 * KT + kk) * 64 + lane] = 0.0;
        st[(3 * KT + kk) * 64 + lane] = 0.0;
    }
    st[(4 * KT) * 64 + lane] = 0.0;
    st[(4 * KT + 1) * 64 + lane] = 0.0;
}

// Objective, its directional derivative and the final tangent of one direction per workgroup (grid = directions, block = 64):
//   s = tr(Vtg' V)/N, sd = tr(Vtg' Vd)/N through the fixed-order sums of k_terminal_parts (per lane over parts and tiles, then over the
//   lanes); primaryobjf = 1 - |s|^2, d(primaryobjf) = -2 Re(conj(s) sd); secondaryobjf and its derivative from the two leak rows.
//   res[dir][8] = { primaryobjf, secondaryobjf, Re s, Im s, d primaryobjf, d secondaryobjf, Re sd, Im sd }
//   wr, wi (nullptr: not wanted): [dir][N][Ntot] real and imaginary part of d(vr - i vi) = (ud, -vd)
// vtr_img, vti_img: the handle's target images [parts][KT][64] (columns a slab does not hold meet zeros of the state)
__global__ void __launch_bounds__(64) k_terminal_tl(const double* __restrict__ state, long long stride, const double* __restrict__ vtr_img,
                                                    const double* __restrict__ vti_img, int KT, int Ntot, int N, int parts, double leak_scale,
                                                    double* res, double* wr, double* wi)
{
    __shared__ double part[6][64];
    const int lane = threadIdx.x, dir = blockIdx.x;
    double re = 0.0, im = 0.0, dre = 0.0, dim = 0.0, lk = 0.0, dlk = 0.0;
    for (int p = 0; p < parts; ++p) {
        const double* st = state + ((size_t)dir * parts + p) * stride;
        const double *tr = vtr_img + (size_t)p * KT * 64, *ti = vti_img + (size_t)p * KT * 64;
        const int col = 16 * p + (lane & 15);
        for (int kk = 0; kk < KT; ++kk) {
            const double u = st[kk * 64 + lane], v = st[(KT + kk) * 64 + lane];
            const double ud = st[(2 * KT + kk) * 64 + lane], vd = st[(3 * KT + kk) * 64 + lane];
            re += jq_det2(u, tr[kk * 64 + lane], v, ti[kk * 64 + lane]);
            im += jq_dot2(u, ti[kk * 64 + lane], v, tr[kk * 64 + lane]);
            dre += jq_det2(ud, tr[kk * 64 + lane], vd, ti[kk * 64 + lane]);
            dim += jq_dot2(ud, ti[kk * 64 + lane], vd, tr[kk * 64 + lane]);
            const int row = 4 * kk + (lane >> 4);
            if (wr && row < Ntot && col < N) {
                wr[((size_t)dir * N + col) * Ntot + row] = ud;
                wi[((size_t)dir * N + col) * Ntot + row] = -vd;
            }
        }
        lk += st[(4 * KT) * 64 + lane];
        dlk += st[(4 * KT + 1) * 64 + lane];
    }
    part[0][lane] = re, part[1][lane] = im, part[2][lane] = dre, part[3][lane] = dim, part[4][lane] = lk, part[5][lane] = dlk;
    __syncthreads();
    if (lane != 0) return;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int l = 0; l < 64; ++l)
        for (int k = 0; k < 6; ++k) s[k] += part[k][l];
    for (int k = 0; k < 4; ++k) s[k] /= N;
    double* r = res + (size_t)dir * 8;
    r[0] = 1.0 - jq_dot2(s[0], s[0], s[1], s[1]);
    r[1] = leak_scale * s[4];
    r[2] = s[0], r[3] = s[1];
    r[4] = -2.0 * jq_dot2(s[0], s[2], s[1], s[3]);
    r[5] = leak_scale * s[5];
    r[6] = s[2], r[7] = s[3];
}
