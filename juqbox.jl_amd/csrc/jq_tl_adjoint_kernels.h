// jq_tl_adjoint_kernels.h -- tangent of the Stormer-Verlet adjoint sweep (jq_traceobjgrad_hvp): correctness first.
//
// hv(alpha; d) = d/d eps totalgrad(alpha + eps d) at eps = 0: the exact derivative of the gradient THIS LIBRARY returns, obtained by
// differentiating the backward sweep as it executes, the way k_forward_tl (jq_tl_kernels.h) differentiates the forward sweep.  It is the
// Hessian of the discrete objective only as far as the gradient is its gradient: the adjoint step is the exact transpose of the forward
// step for exact linear solves, with a truncated Neumann series gradient and Jacobian deviate at truncation level and the operator is
// not symmetric (|e.Jd - d.Je| / |e.Jd| on random 7-step problems: order 0 1e-1 .. 7e-1, order 1 1e-3 .. 2e-2, order 4 4e-7 .. 4e-4,
// order 20 1e-15 .. 3e-14).  Callers who need a symmetric operator symmetrise it or raise the order; nothing here symmetrises silently.
//
// k_backward_tl is the step of k_backward_huge (jq_huge_kernels.h) in dual-number arithmetic: the state re-integration with h < 0 is
// Tl::step on (u, v, ud, vd), every vector of the adjoint step (mu, nb and R, X, L, Q, P, nbn, Bq, G, T) has a tangent twin, every
// product with a time-dependent operator is Tl::mm2 on the primal stream and the stream of the workgroup's direction in lock-step, every
// Neumann chain Tl::horner2, the leak forcing cfw wd u gets cfw wd ud.  The trace images Hsym_q, Hanti_q are constant: T = H X,
// Td = H Xd are two MFMAs per tile (mmc), what the direction's stream holds at those schedule slots is not read.  Every trace scalar
// t1 .. t5 gets its tangent dot(ud, T) + dot(u, Td) in a second trace record of the layout k_trace_reduce reads; the controls are linear
// in the coefficients, so k_gradacc on the tangent record assembles the derivative of the gradient.  No ensemble shift (the tangent-
// linear sweeps have no ensemble nodes), no low-rank weight terms (the host refuses full weights).
#pragma once
#include "jq_tl_kernels.h"

// work area of a slab: the 2 TV_COUNT vectors of Tl, then TB_COUNT primal and TB_COUNT tangent vectors of the adjoint step
enum { TB_R, TB_X, TB_L, TB_Q, TB_P, TB_NBN, TB_BQ, TB_G, TB_T, TB_COUNT };
#define JQ_TLB_WORK_VECS (2 * (TV_COUNT + TB_COUNT))
// 64-double rows of a slab's state file: u, v, ud, vd [KT] each, leak, d(leak) (the file of the forward sweep, JQ_TL_STATE_ROWS), then
// mu, nb, mud, nbd [KT] each, carry[JQ_MAXNC], d(carry)[JQ_MAXNC]
#define JQ_TLB_STATE_ROWS(KT) (8 * (KT) + 2 + 2 * JQ_MAXNC)

struct TlB : Tl {
    __device__ __forceinline__ double* bvec(int i) const { return work + (size_t)(2 * TV_COUNT + i) * KT * 64; }
    __device__ __forceinline__ double* bdvec(int i) const { return work + (size_t)(2 * TV_COUNT + TB_COUNT + i) * KT * 64; }
    // D = M x ; Dd = M xd with the current (constant) operator.  D, Dd must not be x, xd.  Barriers as mm2.
    __device__ __forceinline__ void mmc(double* D, double* Dd, const double* x, const double* xd) const
    {
        __syncthreads();
        for (int mt = wave; mt < NT; mt += JQ_HUGE_WAVES) {
            d4 acc = {0.0, 0.0, 0.0, 0.0}, accd = {0.0, 0.0, 0.0, 0.0};
            const double* Mr = M + (size_t)mt * KT * 64;
            for (int kk = 0; kk < KT; ++kk) {
                const double a = Mr[(size_t)kk * 64];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, x[(size_t)kk * 64 + lane], acc, 0, 0, 0);
                accd = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xd[(size_t)kk * 64 + lane], accd, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                D[(size_t)(4 * mt + r) * 64 + lane] = acc[r];
                Dd[(size_t)(4 * mt + r) * 64 + lane] = accd[r];
            }
        }
        __syncthreads();
    }
    // sum over this lane's own elements of a[e] b[e]
    __device__ __forceinline__ double dot(const double* a, const double* b) const
    {
        double s = 0.0;
        each([&](size_t e, int) { s += a[e] * b[e]; });
        return s;
    }
    // ... and of its derivative ad[e] b[e] + a[e] bd[e]
    __device__ __forceinline__ double ddot(const double* a, const double* ad, const double* b, const double* bd) const
    {
        double s = 0.0;
        each([&](size_t e, int) { s += ad[e] * b[e] + a[e] * bd[e]; });
        return s;
    }
};

// Backward sweep of (state, adjoint) and their tangents over one chunk: workgroup b = slab b % parts of direction b / parts.
//   a.stream: the chunk's tile streams (generated with -dt and the backward schedule), group 0 primal, group 1 + dir the direction's;
//   a.cimg: [Hsym_q | Hanti_q] of the sweep's control group; a.state: [workgroups][JQ_TLB_STATE_ROWS(KT)][64];
//   a.park: work areas [workgroups][JQ_TLB_WORK_VECS][KT][64]; a.tabs: wd[16 NT];
//   a.traces: [workgroups 16 + wave][nsteps_chunk][Ncoupled JQ_NTR] primal trace scalars per wave, the tangents' record of the same
//   shape a.nslabs 16 rows behind it
// (a template with one instantiation, like k_forward_tl)
template <int WAVES = JQ_HUGE_WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_backward_tl(PropArgs a)
{
    static_assert(WAVES == JQ_HUGE_WAVES, "Tl strides the tile rows by JQ_HUGE_WAVES");
    __shared__ double scratch[WAVES * 64];
    TlB tl;
    tl.NT = (a.Ntot + 15) / 16;
    tl.KT = 4 * tl.NT;
    tl.lane = threadIdx.x & 63;
    tl.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    tl.g = tl.lane >> 4;
    tl.m = a.m;
    tl.work = a.park + (size_t)blockIdx.x * JQ_TLB_WORK_VECS * tl.KT * 64;
    tl.cur.init(nullptr, a, 0, 0, 0);
    tl.curd.init(nullptr, a, 0, 0, 0);
    tl.curd.stream = a.stream + (size_t)(1 + (int)blockIdx.x / a.parts) * (size_t)a.stream_gstride;
    tl.M = tl.Md = nullptr;
    tl.wd = a.tabs;
    const int KT = tl.KT, lane = tl.lane, wave = tl.wave, Nc = a.Ncoupled;
    double* st = a.state + (size_t)blockIdx.x * a.state_stride;
    double *u = st, *v = st + (size_t)KT * 64, *ud = st + (size_t)2 * KT * 64, *vd = st + (size_t)3 * KT * 64;
    double* ad = st + (size_t)(4 * KT + 2) * 64;
    double *mu = ad, *nb = ad + (size_t)KT * 64, *mud = ad + (size_t)2 * KT * 64, *nbd = ad + (size_t)3 * KT * 64;
    double* cr = ad + (size_t)4 * KT * 64;      // carry[JQ_MAXNC], d(carry)[JQ_MAXNC]
    const double *un = tl.vec(TV_UN), *v05 = tl.vec(TV_V05), *vN = tl.vec(TV_VN);
    const double *und = tl.dvec(TV_UN), *v05d = tl.dvec(TV_V05), *vNd = tl.dvec(TV_VN);
    double *R = tl.bvec(TB_R), *X = tl.bvec(TB_X), *L = tl.bvec(TB_L), *Qv = tl.bvec(TB_Q), *P = tl.bvec(TB_P), *nbn = tl.bvec(TB_NBN);
    double *Bq = tl.bvec(TB_BQ), *G = tl.bvec(TB_G), *T = tl.bvec(TB_T);
    double *Rd = tl.bdvec(TB_R), *Xd = tl.bdvec(TB_X), *Ld = tl.bdvec(TB_L), *Qd = tl.bdvec(TB_Q), *Pd = tl.bdvec(TB_P), *nbnd = tl.bdvec(TB_NBN);
    double *Bqd = tl.bdvec(TB_BQ), *Gd = tl.bdvec(TB_G), *Td = tl.bdvec(TB_T);
    const double cfw = a.forced ? 0.5 * a.h * a.tinv : 0.0;
    const double* wd = a.tabs;
    double carry[JQ_MAXNC], carryd[JQ_MAXNC];
    for (int q = 0; q < JQ_MAXNC; ++q) {
        carry[q] = (q < Nc) ? cr[(size_t)q * 64 + lane] / JQ_HUGE_WAVES : 0.0;
        carryd[q] = (q < Nc) ? cr[(size_t)(JQ_MAXNC + q) * 64 + lane] / JQ_HUGE_WAVES : 0.0;
    }
    const size_t ntr = (size_t)Nc * JQ_NTR;
    double* trw = a.traces + ((size_t)blockIdx.x * JQ_HUGE_WAVES + wave) * a.nsteps_chunk * ntr;
    double* trwd = trw + (size_t)a.nslabs * JQ_HUGE_WAVES * a.nsteps_chunk * ntr;

    if (a.first_chunk) {      // carry_q = tr(vr' Hsym_q lambdai) at t = T
        for (int q = 0; q < JQ_MAXNC; ++q)
            if (q < Nc) {
                tl.next_op();
                tl.mmc(T, Td, nb, nbd);
                carry[q] = -tl.dot(u, T);      // nb = -lambda_i
                carryd[q] = -tl.ddot(u, ud, T, Td);
            }
    }
    for (int n = 0; n < a.nsteps_chunk; ++n) {
        tl.step(u, v, ud, vd);      // uses 0 .. 6: the state step with h < 0 -- un, v05, vN
        tl.mm2(R, Rd, nullptr, nullptr, nb, nbd);      // (still use 6: Kp05) R = c K05 nb
        tl.next_op();      // use 7: S0 -- R = c (S0 mu - K05 li + hr0) ; X = mu + sum_j S^j R
        tl.mm2(R, Rd, R, Rd, mu, mud);
        tl.each([&](size_t e, int row) { R[e] += (cfw * wd[row]) * u[e]; Rd[e] += (cfw * wd[row]) * ud[e]; });
        tl.each([&](size_t e, int) { X[e] = mu[e] + R[e]; Xd[e] = mud[e] + Rd[e]; });
        tl.horner2(X, Xd, X, Xd, R, Rd);
        // early traces with X: t1 = tr(vr0' Hanti_q X), t3 = tr(vr' Hanti_q X)
        for (int q = 0; q < JQ_MAXNC; ++q)
            if (q < Nc) {
                tl.next_op();
                tl.mmc(T, Td, X, Xd);
                const double t1 = wave_sum(tl.dot(u, T)), t3 = wave_sum(tl.dot(un, T));
                const double t1d = wave_sum(tl.ddot(u, ud, T, Td)), t3d = wave_sum(tl.ddot(un, und, T, Td));
                if (lane == 0) {
                    trw[(size_t)n * ntr + q * JQ_NTR + 0] = t1, trwd[(size_t)n * ntr + q * JQ_NTR + 0] = t1d;
                    trw[(size_t)n * ntr + q * JQ_NTR + 2] = t3, trwd[(size_t)n * ntr + q * JQ_NTR + 2] = t3d;
                }
            }
        tl.next_op();      // use 8: Kn0 -- L = -c K0 X
        tl.mm2(L, Ld, nullptr, nullptr, X, Xd);
        tl.next_op();      // use 9: Kn1 -- Q = -c K1 X
        tl.mm2(Qv, Qd, nullptr, nullptr, X, Xd);
        tl.next_op();      // use 10: S05 -- L = -c l2 ; Q = -c (...) ; nb_new = nb + L + sum_j S^j Q
        tl.mm2(P, Pd, nullptr, nullptr, nb, nbd);
        tl.each([&](size_t e, int row) { P[e] -= (cfw * wd[row]) * v05[e]; Pd[e] -= (cfw * wd[row]) * v05d[e]; });
        tl.each([&](size_t e, int) { L[e] += P[e]; Qv[e] += P[e]; Ld[e] += Pd[e]; Qd[e] += Pd[e]; });
        tl.mm2(Qv, Qd, Qv, Qd, L, Ld);
        tl.each([&](size_t e, int) { nbn[e] = (nb[e] + L[e]) + Qv[e]; nbnd[e] = (nbd[e] + Ld[e]) + Qd[e]; });
        tl.horner2(nbn, nbnd, nbn, nbnd, Qv, Qd);
        tl.each([&](size_t e, int) { Bq[e] = nb[e] + nbn[e]; Bqd[e] = nbd[e] + nbnd[e]; });      // -(li0 + li)
        tl.next_op();      // use 11: Kp05 -- G = X + c K05 nb_new
        tl.mm2(G, Gd, X, Xd, nbn, nbnd);
        tl.next_op();      // use 12: S1 -- lambda_r_new = X + c (S1 X - K05 li_new + hr1)
        tl.mm2(G, Gd, G, Gd, X, Xd);
        tl.each([&](size_t e, int row) { G[e] += (cfw * wd[row]) * un[e]; Gd[e] += (cfw * wd[row]) * und[e]; });
        // late traces: t5 = tr(vi05' Hanti (li0+li)), t2 = tr(vi05' Hsym X), t4 = tr(vr' Hsym li) + carry
        for (int q = 0; q < JQ_MAXNC; ++q)
            if (q < Nc) {
                tl.next_op();      // Hanti_q
                tl.mmc(T, Td, Bq, Bqd);
                const double t5 = wave_sum(-tl.dot(v05, T)), t5d = wave_sum(-tl.ddot(v05, v05d, T, Td));
                tl.next_op();      // Hsym_q
                tl.mmc(T, Td, X, Xd);
                const double t2 = wave_sum(tl.dot(v05, T)), t2d = wave_sum(tl.ddot(v05, v05d, T, Td));
                tl.mmc(T, Td, nbn, nbnd);
                const double p4 = -tl.dot(un, T), p4d = -tl.ddot(un, und, T, Td);
                const double t4 = wave_sum(p4 + carry[q]), t4d = wave_sum(p4d + carryd[q]);
                carry[q] = p4, carryd[q] = p4d;
                if (lane == 0) {
                    trw[(size_t)n * ntr + q * JQ_NTR + 4] = t5, trwd[(size_t)n * ntr + q * JQ_NTR + 4] = t5d;
                    trw[(size_t)n * ntr + q * JQ_NTR + 1] = t2, trwd[(size_t)n * ntr + q * JQ_NTR + 1] = t2d;
                    trw[(size_t)n * ntr + q * JQ_NTR + 3] = t4, trwd[(size_t)n * ntr + q * JQ_NTR + 3] = t4d;
                }
            }
        tl.each([&](size_t e, int) {
            u[e] = un[e], v[e] = vN[e], ud[e] = und[e], vd[e] = vNd[e];
            mu[e] = G[e], nb[e] = nbn[e], mud[e] = Gd[e], nbd[e] = nbnd[e];
        });
    }
    for (int q = 0; q < JQ_MAXNC; ++q)
        if (q < Nc) {
            huge_wg_sum_store(carry[q], scratch, &cr[(size_t)q * 64], wave, lane, false);
            huge_wg_sum_store(carryd[q], scratch, &cr[(size_t)(JQ_MAXNC + q) * 64], wave, lane, false);
        }
}

// Terminal condition of the adjoint and of its tangent, one direction per workgroup (grid = directions, block = 64), from the final
// (u, v, ud, vd) k_forward_tl left in the state files: s = tr(Vtg' V)/N, sd = tr(Vtg' Vd)/N through the fixed-order sums of
// k_terminal_tl; lambda(T) = s conj(Vtg)/N (k_terminal_parts, mode 1) and its tangent sd conj(Vtg)/N go to mu, nb = -lambda_i and
// mud, nbd of every slab of the direction, the carries are cleared (k_backward_tl's first_chunk branch forms them).
//   res[dir][4] = { primaryobjf, secondaryobjf, Re s, Im s }
// N <= 16 (parts == 1): the target image repeats its first N columns, a slab holds ONE copy of the evaluation (k_init_tl) -- the
// columns beyond N get a zero adjoint.
__global__ void __launch_bounds__(64) k_terminal_hvp(double* state, long long stride, const double* __restrict__ vtr_img,
                                                     const double* __restrict__ vti_img, int KT, int N, int parts, double leak_scale, double* res)
{
    __shared__ double part[5][64];
    const int lane = threadIdx.x, dir = blockIdx.x;
    double re = 0.0, im = 0.0, dre = 0.0, dim = 0.0, lk = 0.0;
    for (int p = 0; p < parts; ++p) {
        const double* st = state + ((size_t)dir * parts + p) * stride;
        const double *tr = vtr_img + (size_t)p * KT * 64, *ti = vti_img + (size_t)p * KT * 64;
        for (int kk = 0; kk < KT; ++kk) {
            const double u = st[kk * 64 + lane], v = st[(KT + kk) * 64 + lane];
            const double ud = st[(2 * KT + kk) * 64 + lane], vd = st[(3 * KT + kk) * 64 + lane];
            re += jq_det2(u, tr[kk * 64 + lane], v, ti[kk * 64 + lane]);
            im += jq_dot2(u, ti[kk * 64 + lane], v, tr[kk * 64 + lane]);
            dre += jq_det2(ud, tr[kk * 64 + lane], vd, ti[kk * 64 + lane]);
            dim += jq_dot2(ud, ti[kk * 64 + lane], vd, tr[kk * 64 + lane]);
        }
        lk += st[(4 * KT) * 64 + lane];
    }
    part[0][lane] = re, part[1][lane] = im, part[2][lane] = dre, part[3][lane] = dim, part[4][lane] = lk;
    __syncthreads();
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int l = 0; l < 64; ++l)
        for (int k = 0; k < 5; ++k) s[k] += part[k][l];
    for (int k = 0; k < 4; ++k) s[k] /= N;
    const bool on = parts > 1 || (lane & 15) < N;
    for (int p = 0; p < parts; ++p) {
        double* ad = state + ((size_t)dir * parts + p) * stride + (size_t)(4 * KT + 2) * 64;
        const double *tr = vtr_img + (size_t)p * KT * 64, *ti = vti_img + (size_t)p * KT * 64;
        for (int kk = 0; kk < KT; ++kk) {
            const double r = tr[kk * 64 + lane], i = ti[kk * 64 + lane];
            ad[kk * 64 + lane] = on ? jq_dot2(s[1], i, s[0], r) / N : 0.0;                      // lambdar
            ad[(KT + kk) * 64 + lane] = on ? -(jq_det2(s[1], r, s[0], i) / N) : 0.0;            // nb = -lambdai
            ad[(2 * KT + kk) * 64 + lane] = on ? jq_dot2(s[3], i, s[2], r) / N : 0.0;
            ad[(3 * KT + kk) * 64 + lane] = on ? -(jq_det2(s[3], r, s[2], i) / N) : 0.0;
        }
        for (int q = 0; q < 2 * JQ_MAXNC; ++q) ad[(4 * KT + q) * 64 + lane] = 0.0;
    }
    if (lane != 0) return;
    double* r = res + (size_t)dir * 4;
    r[0] = 1.0 - jq_dot2(s[0], s[0], s[1], s[1]);
    r[1] = leak_scale * s[4];
    r[2] = s[0], r[3] = s[1];
}
