// jq_aux_kernels.h -- the small kernels around the propagators: on-device control evaluation
// (bcarrier2), K(t)/S(t) tile-stream generation, state initialisation, fidelity + adjoint terminal
// condition, trace reduction and gradient assembly (gradbcarrier2! as an 18-entry scatter); the siblings of the control evaluation and
// of the assembly for controls given as samples on the time grid (k_ctrl_samples, k_gradsamples) and their batched forms for the
// tangent-linear sweeps (k_ctrl_samples_grouped, k_gradsamples_grouped).
#pragma once
#include "jq_kernels.h"
#include "jq_rowlane_kernels.h"
#include "jq_rowlane_tl_kernels.h"
#include "jq_quad_tl_kernels.h"

struct SplineArgs {
    const double* pcof;   // [nCoeff]
    const double* cfreq;  // [Ncoupled x Nfreq] column-major
    int D1, Nfreq, Ncoupled, nCoeff;
    double dtknot;        // T/(D1-2)            (bcparams, src/bsplines.jl:174)
    const double* rfreq;  // uncoupled controls: params.Rfreq [Ncoupled] (Ncoupled then counts them); nullptr otherwise
};

// knot index k (1-based) of bcarrier2 / gradbcarrier2! (src/bsplines.jl:224-225, :335-336)
__device__ __forceinline__ int knot_index(double t, double dtknot, int D1)
{
    int k = (int)ceil(t / dtknot + 2.0);
    k = k < 3 ? 3 : k;
    k = k > D1 ? D1 : k;
    return k;
}

// bcarrier2(t, params, func): src/bsplines.jl:211-304
__device__ double bcarrier2_dev(const SplineArgs& s, double t, int func)
{
    const int osc = func >> 1, q_func = func & 1;
    const double width = 3.0 * s.dtknot;
    const int k = knot_index(t, s.dtknot, s.D1);
    double f = 0.0;
    for (int freq = 0; freq < s.Nfreq; ++freq) {
        const int offset1 = 2 * osc * s.Nfreq * s.D1 + freq * 2 * s.D1;
        const int offset2 = offset1 + s.D1;
        double fbs1 = 0.0, fbs2 = 0.0, tc, tau, b;
        tc = s.dtknot * ((double)k - 1.5);           // tcenter[k]   (:175, :238)
        tau = (t - tc) / width;
        b = 9.0 / 8.0 + 4.5 * tau + 4.5 * tau * tau;
        fbs1 += s.pcof[offset1 + k - 1] * b;
        fbs2 += s.pcof[offset2 + k - 1] * b;
        tc = s.dtknot * ((double)(k - 1) - 1.5);     // tcenter[k-1] (:244)
        tau = (t - tc) / width;
        b = 0.75 - 9.0 * tau * tau;
        fbs1 += s.pcof[offset1 + k - 2] * b;
        fbs2 += s.pcof[offset2 + k - 2] * b;
        tc = s.dtknot * ((double)(k - 2) - 1.5);     // tcenter[k-2] (:250)
        tau = (t - tc) / width;
        b = 9.0 / 8.0 - 4.5 * tau + 4.5 * tau * tau;
        fbs1 += s.pcof[offset1 + k - 3] * b;
        fbs2 += s.pcof[offset2 + k - 3] * b;
        const double om = s.cfreq[osc + freq * s.Ncoupled];
        double sn, cs;
        sincos(om * t, &sn, &cs);
        if (q_func)
            f += fbs1 * sn + fbs2 * cs;   // :258
        else
            f += fbs1 * cs - fbs2 * sn;   // :260
    }
    return f;
}

// time of stream point j of a chunk: t_n (j even) or t_n + h/2 (j odd); t_n is read from the
// host-accumulated table (t = t + h, src/StormerVerlet.jl:502; the backward table starts at exactly T,
// src/evalobjgrad.jl:811) so that knot indices match the reference to the ulp.
__device__ __forceinline__ double stream_time(const double* tt, int n0, int j, double h)
{
    const double t = tt[n0 + (j >> 1)];
    return (j & 1) ? t + 0.5 * h : t;
}

// pq[j][2*Ncoupled] = (p_1, q_1, p_2, q_2, ...)(t_j)   -- KS!'s controlfunc calls (src/evalobjgrad.jl:2366-2367)
// grid.y = control vectors of a grouped batch (jq_traceobjgrad_batch): vector g reads the coefficient block g of s.pcof and writes the
// pq block g ([g][ntp][2 Ncoupled]); one vector is the launch it always was
// mix (jq_traceobjgrad_members; nullptr: none, the launch it always was): [groups][Ncoupled x Ncoupled] column-major real mixing matrices.
// What reaches operator l of group g is sum_k C_g[l, k] (p_k, q_k) -- every control keeps its own carriers and coefficients.  The thread
// parks its unmixed values in row j of `raw` (the layout of pq; read back by the thread that wrote them) and writes the mixed ones to pq.
// Zero entries of C are skipped and the first term is the product alone, so C = I writes the bits of the unmixed launch.
__global__ void k_ctrl(SplineArgs s, const double* tt, int n0, int ntp, double h, double* pq, const double* __restrict__ mix, double* raw)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ntp) return;
    const int Nc = s.Ncoupled;
    s.pcof += (size_t)blockIdx.y * s.nCoeff;
    pq += ((size_t)blockIdx.y * ntp + j) * 2 * Nc;
    double* const val = mix ? raw + ((size_t)blockIdx.y * ntp + j) * 2 * Nc : pq;      // (the unmixed values of this time point)
    const double t = stream_time(tt, n0, j, h);
    if (s.rfreq) {
        // uncoupled controls (src/evalobjgrad.jl:2373-2387): ft = 2 (p cos(2 pi Rfreq t) - q sin(2 pi Rfreq t)) multiplies
        // Hunc_ops[q], which sits in the symmetric OR the antisymmetric slot of pair q (the other slot is zero)
        for (int q = 0; q < Nc; ++q) {
            const double pt = bcarrier2_dev(s, t, 2 * q), qt = bcarrier2_dev(s, t, 2 * q + 1);
            const double ft = 2.0 * (pt * cos(2.0 * M_PI * s.rfreq[q] * t) - qt * sin(2.0 * M_PI * s.rfreq[q] * t));
            val[2 * q] = ft;
            val[2 * q + 1] = ft;
        }
    } else {
        for (int f = 0; f < 2 * Nc; ++f) val[f] = bcarrier2_dev(s, t, f);
    }
    if (!mix) return;
    const double* C = mix + (size_t)blockIdx.y * Nc * Nc;
    for (int l = 0; l < Nc; ++l) {
        double pm = 0.0, qm = 0.0;
        bool first = true;
        for (int k = 0; k < Nc; ++k) {
            const double c = C[l + Nc * k];
            if (c == 0.0) continue;
            const double pk = c * val[2 * k], qk = c * val[2 * k + 1];
            pm = first ? pk : pm + pk;
            qm = first ? qk : qm + qk;
            first = false;
        }
        pq[2 * l] = pm;
        pq[2 * l + 1] = qm;
    }
}

// KS!: K = Hconst + sum_q p_q Hsym_q ; S = sum_q q_q Hanti_q  (src/evalobjgrad.jl:2354-2370), evaluated
// on the MFMA tile images and stored pre-scaled for the accumulate-in-place step formulation
// (jq_kernels.h): with c = h/2, K -> +c K at the half time points (odd j), -c K at the integer
// time points (even j); S -> c S.   grid = (mat_elems/256, ntp, control vectors)
// (grouped batch: vector g = blockIdx.z reads the pq block g and writes its own stream, gstride doubles behind the one before)
// h0: the drift image (image 0) of group 0, group g's h0_gstride doubles behind it -- himg and 0 for every launch whose groups share the
// handle's drift (the launch it always was); a drift ensemble (jq_traceobjgrad_drifts) passes its members' images [groups][mat_elems].
// The control images 1 .. 2 Ncoupled are read from himg in either case.
__global__ void k_stream(const double* __restrict__ himg, const double* __restrict__ h0, long long h0_gstride, const double* __restrict__ pq,
                         int Ncoupled, long long mat_elems, double c, double* __restrict__ stream, long long gstride)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (e >= mat_elems) return;
    stream += (size_t)blockIdx.z * (size_t)gstride;
    h0 += (size_t)blockIdx.z * (size_t)h0_gstride;
    const double* ctl = pq + ((size_t)blockIdx.z * gridDim.y + j) * 2 * Ncoupled;
    double K = h0[e], S = 0.0;
    for (int q = 0; q < Ncoupled; ++q) {
        K += ctl[2 * q] * himg[(size_t)(1 + q) * mat_elems + e];
        S += ctl[2 * q + 1] * himg[(size_t)(1 + Ncoupled + q) * mat_elems + e];
    }
    stream[(size_t)(2 * j) * mat_elems + e] = ((j & 1) ? c : -c) * K;
    stream[(size_t)(2 * j + 1) * mat_elems + e] = c * S;
}

// state file <- (Uinit, 0, 0, 0, extras 0); grid = nslabs, block = 64  (N > 16: slab sl holds part sl % parts of its sample)
__global__ void k_init_state(double* state, long long stride, const double* __restrict__ uimg, int KT, int parts)
{
    double* st = state + (size_t)blockIdx.x * stride;
    const int lane = threadIdx.x;
    uimg += (size_t)(blockIdx.x % parts) * KT * 64;
    for (int kk = 0; kk < KT; ++kk) {
        st[kk * 64 + lane] = uimg[kk * 64 + lane];
        st[(KT + kk) * 64 + lane] = 0.0;
        st[(2 * KT + kk) * 64 + lane] = 0.0;
        st[(3 * KT + kk) * 64 + lane] = 0.0;
    }
    for (int r = 0; r < JQ_STATE_EXTRA; ++r) st[(JQ_STATE_ARRAYS * KT + r) * 64 + lane] = 0.0;
}

// Fidelity, leak integral and adjoint terminal condition per sample.
//   s = tr(Vtg' V)/N with ur = vr, ui = -vi (tracefidcomplex, src/evalobjgrad.jl:2078-2084)
//   primaryobjf = 1 - |s|^2 (:759) ; secondaryobjf = dt/2 * tinv * sum(leak partials) (:716-718)
//   lambda(T) (init_adjoint!, :2029-2042)
// res[sample][4] = { primaryobjf, secondaryobjf, Re s, Im s }.   grid = nslabs, block = 64
// mode (wave-uniform; JQ_SV_*, include/juqbox_hip.h): which of the target T (vtr_img, vti_img) and dVds D (dvr_img, dvi_img: the same
// layout; read only when mode != 1) the adjoint starts from (src/evalobjgrad.jl:815-844), with s_X = tr(X' V)/N:
//   1: lambda(T) = s_T conj(T)/N    2: s_T conj(D)/N    3: s_D conj(T)/N    4: (s_T conj(D) + s_D conj(T))/N
// res[] is taken against the target in every mode.  Mode 1 executes the instructions it always did, on the same data; the second trace of
// modes 3, 4 goes through the same fixed-order sums as the first (part[3], part[4]).
__global__ void k_terminal(double* state, long long stride, const double* __restrict__ vtr_img,
                           const double* __restrict__ vti_img, int KT, int N, int sps, int nsamples, double leak_scale,
                           double* res, const double* __restrict__ dvr_img, const double* __restrict__ dvi_img, int mode)
{
    __shared__ double part[5][64];
    double* st = state + (size_t)blockIdx.x * stride;
    const int lane = threadIdx.x;
    const int col = lane & 15;
    const int sl = (col < sps * N) ? col / N : -1;
    double re = 0.0, im = 0.0;
    for (int kk = 0; kk < KT; ++kk) {
        const double u = st[kk * 64 + lane], v = st[(KT + kk) * 64 + lane];
        const double tr = vtr_img[kk * 64 + lane], ti = vti_img[kk * 64 + lane];
        re += jq_det2(u, tr, v, ti);
        im += jq_dot2(u, ti, v, tr);
    }
    part[0][lane] = re;
    part[1][lane] = im;
    part[2][lane] = st[(JQ_STATE_ARRAYS * KT + JQ_MAXNC) * 64 + lane];
    if (mode >= 3) {      // s_D: the same sums against the dVds image
        double dre = 0.0, dim = 0.0;
        for (int kk = 0; kk < KT; ++kk) {
            const double u = st[kk * 64 + lane], v = st[(KT + kk) * 64 + lane];
            const double tr = dvr_img[kk * 64 + lane], ti = dvi_img[kk * 64 + lane];
            dre += jq_det2(u, tr, v, ti);
            dim += jq_dot2(u, ti, v, tr);
        }
        part[3][lane] = dre;
        part[4][lane] = dim;
    }
    __syncthreads();
    double sre = 0.0, sim = 0.0, slk = 0.0;
    for (int l = 0; l < 64; ++l) {
        const int c2 = l & 15;
        const int s2 = (c2 < sps * N) ? c2 / N : -1;
        if (s2 == sl && sl >= 0) {
            sre += part[0][l];
            sim += part[1][l];
            slk += part[2][l];
        }
    }
    sre /= N;
    sim /= N;
    double dre = 0.0, dim = 0.0;
    if (mode >= 3) {
        for (int l = 0; l < 64; ++l) {
            const int c2 = l & 15;
            const int s2 = (c2 < sps * N) ? c2 / N : -1;
            if (s2 == sl && sl >= 0) {
                dre += part[3][l];
                dim += part[4][l];
            }
        }
        dre /= N;
        dim /= N;
    }
    // lambda(T) = a conj(X)/N  (+ s_D conj(T)/N in mode 4): a = s_D in mode 3, X = D in modes 2 and 4
    const double are = (mode == 3) ? dre : sre, aim = (mode == 3) ? dim : sim;
    const bool from_d = (mode == 2 || mode == 4);
    const double *xr_img = from_d ? dvr_img : vtr_img, *xi_img = from_d ? dvi_img : vti_img;
    for (int kk = 0; kk < KT; ++kk) {
        const double tr = xr_img[kk * 64 + lane], ti = xi_img[kk * 64 + lane];
        double lr = jq_dot2(are, tr, aim, ti) / N, nb = -(jq_det2(aim, tr, are, ti) / N);
        if (mode == 4) {
            const double yr = vtr_img[kk * 64 + lane], yi = vti_img[kk * 64 + lane];
            lr += jq_dot2(dre, yr, dim, yi) / N;
            nb += -(jq_det2(dim, yr, dre, yi) / N);
        }
        st[(2 * KT + kk) * 64 + lane] = (sl >= 0) ? lr : 0.0;  // lambdar
        st[(3 * KT + kk) * 64 + lane] = (sl >= 0) ? nb : 0.0;  // nb = -lambdai
    }
    const int sample = blockIdx.x * sps + sl;
    if (sl >= 0 && (col % N) == 0 && (lane >> 4) == 0 && sample < nsamples) {
        res[(size_t)sample * 4 + 0] = 1.0 - jq_dot2(sre, sre, sim, sim);
        res[(size_t)sample * 4 + 1] = leak_scale * slk;
        res[(size_t)sample * 4 + 2] = sre;
        res[(size_t)sample * 4 + 3] = sim;
    }
}

// k_terminal for N > 16: the columns of a sample are spread over `parts` consecutive slabs (16 columns each); the trace
// fidelity couples them (the only cross-column coupling of an evaluation, src/evalobjgrad.jl:818, :2029-2041).
// grid = nsamples, block = 64; sums over lanes and parts in a fixed order.
// imr != 0: the implicit-midpoint convention of k_terminal_imr (lambda(T) = -2/N (...), the true lambda_i in slot NU)
// mode, dvr_img, dvi_img: see k_terminal (Stormer-Verlet only: imr != 0 is launched with mode 1)
// (one wave per block, declared: under the default bound of 1024 threads the unrolled 64-term sums spilled to scratch)
__global__ void __launch_bounds__(64) k_terminal_parts(double* state, long long stride, const double* __restrict__ vtr_img,
                                 const double* __restrict__ vti_img, int KT, int N, int parts, double leak_scale, double* res, int imr,
                                 const double* __restrict__ dvr_img, const double* __restrict__ dvi_img, int mode)
{
    __shared__ double part[5][64];
    const int lane = threadIdx.x;
    double re = 0.0, im = 0.0, lk = 0.0;
    for (int p = 0; p < parts; ++p) {
        const double* st = state + ((size_t)blockIdx.x * parts + p) * stride;
        const double *tr = vtr_img + (size_t)p * KT * 64, *ti = vti_img + (size_t)p * KT * 64;
        for (int kk = 0; kk < KT; ++kk) {           // (columns beyond N hold zeros in state and target images)
            const double u = st[kk * 64 + lane], v = st[(KT + kk) * 64 + lane];
            re += jq_det2(u, tr[kk * 64 + lane], v, ti[kk * 64 + lane]);
            im += jq_dot2(u, ti[kk * 64 + lane], v, tr[kk * 64 + lane]);
        }
        lk += st[(JQ_STATE_ARRAYS * KT + JQ_MAXNC) * 64 + lane];
    }
    part[0][lane] = re;
    part[1][lane] = im;
    part[2][lane] = lk;
    if (mode >= 3) {      // s_D: the same sums against the dVds image
        double dre = 0.0, dim = 0.0;
        for (int p = 0; p < parts; ++p) {
            const double* st = state + ((size_t)blockIdx.x * parts + p) * stride;
            const double *tr = dvr_img + (size_t)p * KT * 64, *ti = dvi_img + (size_t)p * KT * 64;
            for (int kk = 0; kk < KT; ++kk) {
                const double u = st[kk * 64 + lane], v = st[(KT + kk) * 64 + lane];
                dre += jq_det2(u, tr[kk * 64 + lane], v, ti[kk * 64 + lane]);
                dim += jq_dot2(u, ti[kk * 64 + lane], v, tr[kk * 64 + lane]);
            }
        }
        part[3][lane] = dre;
        part[4][lane] = dim;
    }
    __syncthreads();
    double sre = 0.0, sim = 0.0, slk = 0.0;
    for (int l = 0; l < 64; ++l) {
        sre += part[0][l];
        sim += part[1][l];
        slk += part[2][l];
    }
    sre /= N;
    sim /= N;
    double dre = 0.0, dim = 0.0;
    if (mode >= 3) {
        for (int l = 0; l < 64; ++l) {
            dre += part[3][l];
            dim += part[4][l];
        }
        dre /= N;
        dim /= N;
    }
    const double are = (mode == 3) ? dre : sre, aim = (mode == 3) ? dim : sim;
    const bool from_d = (mode == 2 || mode == 4);
    for (int p = 0; p < parts; ++p) {
        double* st = state + ((size_t)blockIdx.x * parts + p) * stride;
        const double *tr = (from_d ? dvr_img : vtr_img) + (size_t)p * KT * 64, *ti = (from_d ? dvi_img : vti_img) + (size_t)p * KT * 64;
        for (int kk = 0; kk < KT; ++kk) {
            if (imr) {
                st[(2 * KT + kk) * 64 + lane] = -2.0 / N * jq_dot2(sim, ti[kk * 64 + lane], sre, tr[kk * 64 + lane]);    // lambdar
                st[(3 * KT + kk) * 64 + lane] = -2.0 / N * jq_det2(sim, tr[kk * 64 + lane], sre, ti[kk * 64 + lane]);   // lambdai
            } else {
                double lr = jq_dot2(aim, ti[kk * 64 + lane], are, tr[kk * 64 + lane]) / N;        // lambdar
                double nb = -(jq_det2(aim, tr[kk * 64 + lane], are, ti[kk * 64 + lane]) / N);   // nb = -lambdai
                if (mode == 4) {
                    const double yr = vtr_img[(size_t)p * KT * 64 + kk * 64 + lane], yi = vti_img[(size_t)p * KT * 64 + kk * 64 + lane];
                    lr += jq_dot2(dim, yi, dre, yr) / N;
                    nb += -(jq_det2(dim, yr, dre, yi) / N);
                }
                st[(2 * KT + kk) * 64 + lane] = lr;
                st[(3 * KT + kk) * 64 + lane] = nb;
            }
        }
    }
    if (lane == 0) {
        res[(size_t)blockIdx.x * 4 + 0] = 1.0 - jq_dot2(sre, sre, sim, sim);
        res[(size_t)blockIdx.x * 4 + 1] = leak_scale * slk;
        res[(size_t)blockIdx.x * 4 + 2] = sre;
        res[(size_t)blockIdx.x * 4 + 3] = sim;
    }
}

// Implicit-midpoint variant of k_terminal (src/evalobjgrad.jl:1221-1271): lambda(T) = -2/N (re Vtr + im Vti),
// -2/N (-re Vti + im Vtr) with the true lambda_i in slot NU; secondaryobjf = dt*tinv/4 * sum(penal_m) (leak_scale).
// Fidelity, leak integral and adjoint terminal condition per sample.
//   s = tr(Vtg' V)/N with ur = vr, ui = -vi (tracefidcomplex, src/evalobjgrad.jl:2078-2084)
//   primaryobjf = 1 - |s|^2 (:759) ; secondaryobjf = dt/2 * tinv * sum(leak partials) (:716-718)
//   lambda(T) (init_adjoint!, :2029-2042)
// res[sample][4] = { primaryobjf, secondaryobjf, Re s, Im s }.   grid = nslabs, block = 64
__global__ void k_terminal_imr(double* state, long long stride, const double* __restrict__ vtr_img,
                           const double* __restrict__ vti_img, int KT, int N, int sps, int nsamples, double leak_scale,
                           double* res)
{
    __shared__ double part[3][64];
    double* st = state + (size_t)blockIdx.x * stride;
    const int lane = threadIdx.x;
    const int col = lane & 15;
    const int sl = (col < sps * N) ? col / N : -1;
    double re = 0.0, im = 0.0;
    for (int kk = 0; kk < KT; ++kk) {
        const double u = st[kk * 64 + lane], v = st[(KT + kk) * 64 + lane];
        const double tr = vtr_img[kk * 64 + lane], ti = vti_img[kk * 64 + lane];
        re += u * tr - v * ti;
        im += u * ti + v * tr;
    }
    part[0][lane] = re;
    part[1][lane] = im;
    part[2][lane] = st[(JQ_STATE_ARRAYS * KT + JQ_MAXNC) * 64 + lane];
    __syncthreads();
    double sre = 0.0, sim = 0.0, slk = 0.0;
    for (int l = 0; l < 64; ++l) {
        const int c2 = l & 15;
        const int s2 = (c2 < sps * N) ? c2 / N : -1;
        if (s2 == sl && sl >= 0) {
            sre += part[0][l];
            sim += part[1][l];
            slk += part[2][l];
        }
    }
    sre /= N;
    sim /= N;
    for (int kk = 0; kk < KT; ++kk) {
        const double tr = vtr_img[kk * 64 + lane], ti = vti_img[kk * 64 + lane];
        st[(2 * KT + kk) * 64 + lane] = (sl >= 0) ? -2.0 / N * (sre * tr + sim * ti) : 0.0;   // lambdar
        st[(3 * KT + kk) * 64 + lane] = (sl >= 0) ? -2.0 / N * (-sre * ti + sim * tr) : 0.0;  // lambdai
    }
    const int sample = blockIdx.x * sps + sl;
    if (sl >= 0 && (col % N) == 0 && (lane >> 4) == 0 && sample < nsamples) {
        res[(size_t)sample * 4 + 0] = 1.0 - (sre * sre + sim * sim);
        res[(size_t)sample * 4 + 1] = leak_scale * slk;
        res[(size_t)sample * 4 + 2] = sre;
        res[(size_t)sample * 4 + 3] = sim;
    }
}

// R[m][k] = sum_slab traces[slab][m][k] in slab order (deterministic).  thread per (m,k)
// Grouped batch: grid.y = control vectors, `nslabs` = trace rows of ONE vector; R[g][m][k] sums the rows g nslabs .. (g + 1) nslabs - 1 in
// row order -- the order a single evaluation of that vector sums them in.
// mix (jq_traceobjgrad_members; nullptr: none, the launch it always was): [groups][Nc x Nc] column-major mixing matrices C, and the sweep
// computed the traces of the operators [q0, q0 + ntr / JQ_NTR).  R then holds rows for ALL Nc controls, [g][m][Nc][JQ_NTR]: the row of
// control k is sum_{l in the sweep's group} C[l, k] (row of operator l) -- by linearity what k_gradacc needs to assemble the gradient of k's
// coefficients with k's own carrier and spline window (launched with q0 = 0, ng = Nc), the other operator groups add theirs in their
// sweeps.  Zero entries of C are skipped and the first term is the product alone: C = I gives the unmixed rows bit for bit and exact
// zeros elsewhere; a zero column of C an exactly zero gradient block.   thread per (m, control, scalar), grid.x sized for Nc controls
__global__ void k_trace_reduce(const double* __restrict__ traces, int nslabs, int nsteps_chunk, int ntr, double* R,
                               const double* __restrict__ mix, int Nc, int q0)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long tot = (long long)nsteps_chunk * ntr;
    traces += (size_t)blockIdx.y * nslabs * tot;
    if (mix) {
        const long long tot_out = (long long)nsteps_chunk * Nc * JQ_NTR;
        if (i >= tot_out) return;
        const int m = (int)(i / (Nc * JQ_NTR)), rem = (int)(i - (long long)m * Nc * JQ_NTR);
        const int k = rem / JQ_NTR, t = rem - k * JQ_NTR;
        const double* C = mix + (size_t)blockIdx.y * Nc * Nc + (size_t)Nc * k + q0;      // column k, rows q0 ..
        double acc = 0.0;
        bool first = true;
        for (int l = 0; l < ntr / JQ_NTR; ++l) {
            const double c = C[l];
            if (c == 0.0) continue;
            double s = 0.0;
            for (int sl = 0; sl < nslabs; ++sl) s += traces[(size_t)sl * tot + (size_t)m * ntr + l * JQ_NTR + t];
            acc = first ? c * s : acc + c * s;
            first = false;
        }
        R[(size_t)blockIdx.y * tot_out + i] = acc;
        return;
    }
    if (i >= tot) return;
    R += (size_t)blockIdx.y * tot;
    double s = 0.0;
    for (int sl = 0; sl < nslabs; ++sl) s += traces[(size_t)sl * tot + i];
    R[i] = s;
}

// Gradient assembly for one chunk of backward steps: adjoint_grad_calc! + gradbcarrier2!
// (src/evalobjgrad.jl:2581-2618, src/bsplines.jl:321-415) + gradobjfadj += dt*tr_adj (:898).
// One workgroup (JQ_GRADACC_THREADS threads) per coefficient: the threads stride over the steps of the chunk,
// each (step, time point) contributes only when its knot window covers the coefficient; fixed-order tree
// reduction, so the result is deterministic (the summation order differs from the reference's serial
// `gradobjfadj += dt*tr_adj`, a ~1e-16 relative effect).
#define JQ_GRADACC_THREADS 256
__global__ __launch_bounds__(JQ_GRADACC_THREADS) void k_gradacc(SplineArgs s, const double* __restrict__ R,
                                                                const double* __restrict__ tb, int n0, int nsteps_chunk,
                                                                double h, double* grad, int q0, int ng, long long grad_gstride)
{
    // (q0, ng): the control group [q0, q0 + ng) this backward sweep computed the traces of (R rows: [ng][JQ_NTR] per step);
    // the grid covers the coefficients of those controls only
    // grid.y = control vectors of a grouped batch: vector g assembles R[g] into its own gradient, grad_gstride doubles behind the one
    // before (gradbcarrier2! does not depend on the coefficient values: the same code per vector)
    __shared__ double red[JQ_GRADACC_THREADS];
    R += (size_t)blockIdx.y * nsteps_chunk * (ng * JQ_NTR);
    grad += (size_t)blockIdx.y * (size_t)grad_gstride;
    const int per_osc = 2 * s.Nfreq * s.D1;
    const int idx = blockIdx.x + q0 * per_osc;
    const int q = idx / per_osc;
    const int rem = idx - q * per_osc;
    const int freq = rem / (2 * s.D1);
    const int rem2 = rem - freq * 2 * s.D1;
    const int part = rem2 / s.D1;          // 0: offset1 block (alpha_1), 1: offset2 block (alpha_2)
    const int kc = rem2 - part * s.D1 + 1; // 1-based coefficient number within the block
    const double om = s.cfreq[q + freq * s.Ncoupled];
    const double width = 3.0 * s.dtknot;
    const double tc = s.dtknot * ((double)kc - 1.5);
    const int ntr = ng * JQ_NTR;
    double acc = 0.0;
    for (int m = threadIdx.x; m < nsteps_chunk; m += JQ_GRADACC_THREADS) {
        const double t0 = tb[n0 + m];
        const double* r = R + (size_t)m * ntr + (q - q0) * JQ_NTR;
        double step_acc = 0.0;
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const double tau_t = (w == 0) ? t0 : (w == 1 ? t0 + h : t0 + 0.5 * h);
            const int k = knot_index(tau_t, s.dtknot, s.D1);
            const int jj = k - kc;
            if (jj < 0 || jj > 2) continue;
            double P, Q;
            if (w == 0) {
                P = -r[1];
                Q = -r[0];
            } else if (w == 1) {
                P = -r[1];
                Q = -r[2];
            } else {
                P = r[3];
                Q = -r[4];
            }
            if (s.rfreq) {
                // uncoupled control: Hunc_ops[q] sits in ONE slot of pair q (the other image is zero, its traces too) and is
                // applied with ft = 2 (p cos(2 pi Rfreq t) - q sin(2 pi Rfreq t)): grad ft = 2 cos(.) grad p - 2 sin(.) grad q
                const double B = P + Q;
                double sr, cr;
                sincos(2.0 * M_PI * s.rfreq[q] * tau_t, &sr, &cr);
                P = 2.0 * cr * B;
                Q = -2.0 * sr * B;
            }
            const double tau = (tau_t - tc) / width;
            double b;
            if (jj == 0)
                b = 9.0 / 8.0 + 4.5 * tau + 4.5 * tau * tau;
            else if (jj == 1)
                b = 0.75 - 9.0 * tau * tau;
            else
                b = 9.0 / 8.0 - 4.5 * tau + 4.5 * tau * tau;
            double sn, cs;
            sincos(om * tau_t, &sn, &cs);
            step_acc += b * (part == 0 ? (P * cs + Q * sn) : (-P * sn + Q * cs));
        }
        acc += h * step_acc;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = JQ_GRADACC_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) grad[idx] += red[0];
}

// ---------------------------------------------------------------------------------------------
// Controls given as samples on the time grid (jq_traceobjgrad_samples): the siblings of k_ctrl and k_gradacc without a basis.
// S[J][2 Nc] = (p_1, q_1, p_2, q_2, ...) at the half-step index J = 0 .. 2 nsteps of the FORWARD grid (jq_sample_times), nt = 2 nsteps + 1
// rows; G has the same layout.  A chunk of a sweep maps its stream point j to J = J0 + dir j:
//   forward chunk at step n0:            J0 = 2 n0,             dir = +1
//   backward chunk at backward step n0:  J0 = 2 (nsteps - n0),  dir = -1
// One number per time point serves both sweeps (the spline path evaluates the backward sweep at the times of its own table, which
// differ from the forward ones in the last place).

// pq[j][2 Nc] = S[J0 + dir j][2 Nc]; the layout and the launch geometry over ntp of k_ctrl, no mix, no uncoupled branch
__global__ void k_ctrl_samples(const double* __restrict__ S, int nt, int J0, int dir, int ntp, int Nc, double* __restrict__ pq)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ntp) return;
    const int J = J0 + dir * j;
    if (J < 0 || J >= nt) return;
    for (int f = 0; f < 2 * Nc; ++f) pq[(size_t)j * 2 * Nc + f] = S[(size_t)J * 2 * Nc + f];
}

// Gradient with respect to the samples from the trace records of one chunk of backward steps: the assembly of k_gradacc before the
// basis.  R[m][ng][JQ_NTR] are the rows of the sweep's control group [q0, q0 + ng); with r the row of step m and h = -dt, the step gives
//   its point 2 m:      dJ/dp = h (-r[1]),  dJ/dq = h (-r[0])
//   its point 2 m + 2:  dJ/dp = h (-r[1]),  dJ/dq = h (-r[2])
//   its point 2 m + 1:  dJ/dp = h   r[3],   dJ/dq = h (-r[4])
// -- the (w = 0, 1, 2) cases of k_gradacc.  One thread per (chunk point j, control, p or q): an even point adds the contribution of
// step j / 2 and then that of step j / 2 - 1, where the chunk has them, and does ONE += into G[J0 - j][2 q + {0: p, 1: q}].  A point on
// the boundary of two chunks gets its halves from two launches in stream order, so the result is deterministic.  The implicit-midpoint
// kernels fill r[3], r[4] only: their integer-point entries stay exact zeros.
__global__ void k_gradsamples(const double* __restrict__ R, int nsteps_chunk, double h, double* G, int nt, int J0, int Nc, int q0, int ng)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ntp = 2 * nsteps_chunk + 1;
    if (i >= (long long)ntp * ng * 2) return;
    const int j = (int)(i / (2 * ng)), rem = (int)(i - (long long)j * 2 * ng);
    const int c = rem >> 1, isq = rem & 1;
    const int J = J0 - j;
    if (J < 0 || J >= nt) return;
    const int ntr = ng * JQ_NTR;
    double acc = 0.0;
    if (j & 1) {
        const double* r = R + (size_t)(j >> 1) * ntr + c * JQ_NTR;
        acc = h * (isq ? -r[4] : r[3]);
    } else {
        const int m = j >> 1;
        bool first = true;
        if (m < nsteps_chunk) {      // point 2 m of step m
            const double* r = R + (size_t)m * ntr + c * JQ_NTR;
            acc = h * (isq ? -r[0] : -r[1]);
            first = false;
        }
        if (m >= 1) {                // point 2 (m - 1) + 2 of step m - 1
            const double* r = R + (size_t)(m - 1) * ntr + c * JQ_NTR;
            const double v = h * (isq ? -r[2] : -r[1]);
            acc = first ? v : acc + v;
        }
    }
    G[(size_t)J * 2 * Nc + 2 * (q0 + c) + isq] += acc;
}

// The batched forms for the tangent-linear sweeps (jq_eval_f_g_grad_samples_hvp, jq_host_tl.h): siblings, so that the two launches of
// run_eval above stay the code they were.  A table is linear in itself: the tangent stream of a direction table V is the stream of V
// with a zero drift image, and the assembly of the tangent records is the assembly of the primal ones.

// grid.y = the streams [primal table | direction table ...]: table g is read tstride doubles behind the one before and written to the pq
// block g ([g][ntp][2 Nc], what k_stream reads for a grouped chunk); index map and bounds of k_ctrl_samples
__global__ void k_ctrl_samples_grouped(const double* __restrict__ S, long long tstride, int nt, int J0, int dir, int ntp, int Nc, double* __restrict__ pq)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ntp) return;
    const int J = J0 + dir * j;
    if (J < 0 || J >= nt) return;
    S += (size_t)blockIdx.y * (size_t)tstride;
    pq += (size_t)blockIdx.y * ntp * 2 * Nc;
    for (int f = 0; f < 2 * Nc; ++f) pq[(size_t)j * 2 * Nc + f] = S[(size_t)J * 2 * Nc + f];
}

// grid.y = the gradient blocks [primal | direction ...]: block g assembles record g of R ([g][nsteps_chunk][ng][JQ_NTR], k_trace_reduce's
// grouped output) with ONE += into its own table, gstride doubles behind the one before; arithmetic, order and bounds of k_gradsamples
__global__ void k_gradsamples_grouped(const double* __restrict__ R, int nsteps_chunk, double h, double* G, long long gstride, int nt, int J0, int Nc, int q0, int ng)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ntp = 2 * nsteps_chunk + 1;
    if (i >= (long long)ntp * ng * 2) return;
    const int j = (int)(i / (2 * ng)), rem = (int)(i - (long long)j * 2 * ng);
    const int c = rem >> 1, isq = rem & 1;
    const int J = J0 - j;
    if (J < 0 || J >= nt) return;
    const int ntr = ng * JQ_NTR;
    R += (size_t)blockIdx.y * nsteps_chunk * ntr;
    G += (size_t)blockIdx.y * (size_t)gstride;
    double acc = 0.0;
    if (j & 1) {
        const double* r = R + (size_t)(j >> 1) * ntr + c * JQ_NTR;
        acc = h * (isq ? -r[4] : r[3]);
    } else {
        const int m = j >> 1;
        bool first = true;
        if (m < nsteps_chunk) {      // point 2 m of step m
            const double* r = R + (size_t)m * ntr + c * JQ_NTR;
            acc = h * (isq ? -r[0] : -r[1]);
            first = false;
        }
        if (m >= 1) {                // point 2 (m - 1) + 2 of step m - 1
            const double* r = R + (size_t)(m - 1) * ntr + c * JQ_NTR;
            const double v = h * (isq ? -r[2] : -r[1]);
            acc = first ? v : acc + v;
        }
    }
    G[(size_t)J * 2 * Nc + 2 * (q0 + c) + isq] += acc;
}

// Sample tables in a grouped batch of run_eval (jq_traceobjgrad_samples_batch / _members, jq_host_samples_batch.h): siblings again, so
// that every launch above stays the code it was.

// grid.y = groups: group g reads its table tstride doubles behind the one before (0: every group reads the ONE shared table of a member
// ensemble) and writes the pq block g ([g][ntp][2 Nc], what k_stream reads for a grouped chunk); index map and bounds of k_ctrl_samples.
// mix (nullptr: none): [groups][Nc x Nc] column-major mixing matrices, applied with the loop of k_ctrl -- zero entries of C are skipped
// and the first term is the product alone, so C = I writes the table's bits.  The table IS the unmixed value: no `raw` area.
__global__ void k_ctrl_samples_members(const double* __restrict__ S, long long tstride, int nt, int J0, int dir, int ntp, int Nc,
                                       const double* __restrict__ mix, double* __restrict__ pq)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ntp) return;
    const int J = J0 + dir * j;
    if (J < 0 || J >= nt) return;
    const double* val = S + (size_t)blockIdx.y * (size_t)tstride + (size_t)J * 2 * Nc;
    pq += ((size_t)blockIdx.y * ntp + j) * 2 * Nc;
    if (!mix) {
        for (int f = 0; f < 2 * Nc; ++f) pq[f] = val[f];
        return;
    }
    const double* C = mix + (size_t)blockIdx.y * Nc * Nc;
    for (int l = 0; l < Nc; ++l) {
        double pm = 0.0, qm = 0.0;
        bool first = true;
        for (int k = 0; k < Nc; ++k) {
            const double c = C[l + Nc * k];
            if (c == 0.0) continue;
            const double pk = c * val[2 * k], qk = c * val[2 * k + 1];
            pm = first ? pk : pm + pk;
            qm = first ? qk : qm + qk;
            first = false;
        }
        pq[2 * l] = pm;
        pq[2 * l + 1] = qm;
    }
}

// The ensemble gradient of jq_eval_f_g_grad_samples_members on the device: A <- ((A + w_0 T_0) + w_1 T_1) + ... over the `groups`
// finished sample gradients T_g of a launch ([g] tstride doubles apart, k_gradsamples_grouped's tables) in member order, one thread per
// entry and ONE store.  The sum starts from A and runs in member order over whole gradients, so the bits of the ensemble gradient do not
// depend on how many members share a launch, whatever the chunking; the members' tables stay on the device.
__global__ void k_gradsamples_wsum(const double* __restrict__ T, long long tstride, int groups, const double* __restrict__ w, double* __restrict__ A, long long len)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= len) return;
    double acc = A[e];
    for (int g = 0; g < groups; ++g) acc = acc + w[g] * T[(size_t)g * (size_t)tstride + e];
    A[e] = acc;
}

// Packed result of an ensemble evaluation, left on the device for the collective that sums it over GPUs (one all-reduce):
//   out = [ sum_i w_i primaryobjf_i, sum_i w_i secondaryobjf_i, infidelity gradient [ncoeff], leak gradient [ncoeff] ]
// (src/ipopt_interface.jl:48-59; grad = the weighted gradient sums of the forced [0] and unforced [1] backward sweeps:
// objFuncType == 1: infidelgrad = totalgrad, no leak gradient; else leakgrad = totalgrad - infidelgrad, src/evalobjgrad.jl:947).
// One workgroup, fixed summation order (deterministic).  wq == nullptr: unit weights.
__global__ __launch_bounds__(256) void k_pack(const double* __restrict__ res, const double* __restrict__ wq, int nsamples,
                                              const double* __restrict__ grad, int ncoeff, int adjoint, int two_pass,
                                              double* __restrict__ out)
{
    __shared__ double r0[256], r1[256];
    const int t = threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int i = t; i < nsamples; i += 256) {
        const double w = wq ? wq[i] : 1.0;
        s0 += w * res[(size_t)i * 4 + 0];
        s1 += w * res[(size_t)i * 4 + 1];
    }
    r0[t] = s0;
    r1[t] = s1;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            r0[t] += r0[t + w];
            r1[t] += r1[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[0] = r0[0];
        out[1] = r1[0];
    }
    for (int i = t; i < ncoeff; i += 256) {
        const double g0 = adjoint ? grad[i] : 0.0;
        const double g1 = (adjoint && two_pass) ? grad[(size_t)ncoeff + i] : 0.0;
        out[2 + i] = two_pass ? g1 : g0;
        out[2 + (size_t)ncoeff + i] = two_pass ? g0 - g1 : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------
// Consumers of the state history on the device (jq_state_populations).  hist_r/hist_i: [Ntot][N][nsteps+1]
// column-major (row fastest).
// pop[g + ngroups*(q + N*k)] = sum_{rows r: group(r) == g} |psi[r, q, k*every]|^2.   thread per (q, k)
__global__ void k_pop_groups(const double* __restrict__ hr, const double* __restrict__ hi, int Ntot, int N, int every,
                             int nout, const int* __restrict__ group_of_row, int ngroups, double* __restrict__ pop)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * nout) return;
    const int q = (int)(i % N);
    const long long k = i / N;
    const size_t src = ((size_t)k * every * N + q) * Ntot;
    double* out = pop + (size_t)ngroups * i;
    for (int g = 0; g < ngroups; ++g) out[g] = 0.0;
    for (int r = 0; r < Ntot; ++r) {
        const int g = group_of_row ? group_of_row[r] : r;
        if (g < 0) continue;
        const double a = hr[src + r], b = hi[src + r];
        out[g] += a * a + b * b;       // rows of a group are summed in increasing row order, like the reference
    }
}

// maxpop[r] = max_{q, step} |psi[r, q, step]|^2.   block per row
__global__ __launch_bounds__(256) void k_pop_max(const double* __restrict__ hr, const double* __restrict__ hi, int Ntot,
                                                 long long ncolsteps, double* __restrict__ maxpop)
{
    __shared__ double red[256];
    const int r = blockIdx.x;
    double m = 0.0;
    for (long long j = threadIdx.x; j < ncolsteps; j += 256) {
        const double a = hr[(size_t)j * Ntot + r], b = hi[(size_t)j * Ntot + r];
        m = fmax(m, a * a + b * b);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) maxpop[r] = red[0];
}

// ---------------------------------------------------------------------------------------------
// Column-layout state files (lane, row-lane and tangent-linear quad kernels): initial state and terminal condition.  A sample's N columns
// may lie anywhere in the file, so the terminal kernel is a thread per sample that walks them through a column map -- where element
// (array, row, column) of a layout lives.  Arrays 0 .. 3 are U, V, MU, NB, arrays 4 .. 7 their tangents (tangent-linear files).
//   at(arr, R, col)  offset of row R, column col of state array arr
//   leak(col, k)     the k-th of the column's nleak leak partials, k < nleak
//   target(ic, R)    offset of element (R, ic) in the target / dVds images of the layout
//   nrows            rows summed per column
// (The slab-layout kernels above -- k_init_state, k_terminal, k_terminal_parts, k_terminal_imr -- and k_init_tl / k_terminal_tl /
// k_terminal_hvp are a different algorithm: a workgroup per slab or sample that reduces across its lanes through LDS, in another order.)

// lane kernels (jq_lane_kernels.h, jq_lane_tl_kernels.h): [array][row][column] with the column fastest; images [N][NP]
struct LaneMap {
    static constexpr int nleak = 1;
    int nrows;              // NP
    long long ncols;        // padded columns
    int leak_row;           // the last row of the file
    __device__ __forceinline__ size_t at(int arr, int R, long long col) const { return ((size_t)arr * nrows + R) * ncols + col; }
    __device__ __forceinline__ size_t leak(long long col, int) const { return (size_t)leak_row * ncols + col; }
    __device__ __forceinline__ size_t target(int ic, int R) const { return ic * nrows + R; }
};
// row-lane kernels (jq_rowlane_kernels.h, jq_rowlane_tl_kernels.h, jq_rowlane_imr_kernels.h): [array][wave][16 column + row]; images [N][16].
// Column packing: every `cpw` consecutive columns start at a fresh group of `wpg` waves and fill its 4 wpg slots from the front.
// wpg = 1: columns per wave (4, or N*floor(4/N) in the sample-aligned packing of the implicit-midpoint kernels); grouped batches: cpw = the
// columns of one control vector (a multiple of N), wpg = the waves it owns, so that no wave holds the columns of two.  (The implicit-midpoint
// route has no grouped batches: its plan sets wpg = 1, jq_host_plan.h, and init and terminal kernel both take the plan's value.)
struct RowlaneMap {
    static constexpr int nleak = 16, nrows = 16;
    long long nw;           // waves
    int cpw, wpg, leak_row;
    __device__ __forceinline__ size_t at(int arr, int R, long long col) const
    {
        return (size_t)arr * nw * 64 + (size_t)(col / cpw) * wpg * 64 + (size_t)(col % cpw) * 16 + R;
    }
    __device__ __forceinline__ size_t leak(long long col, int k) const { return at(leak_row, k, col); }
    __device__ __forceinline__ size_t target(int ic, int R) const { return ic * 16 + R; }
};
// tangent-linear quad-layout kernels (jq_quad_tl_kernels.h): [row][quad][lane 16 i + 4 b + j <-> row 16 mt + 4 b + i, column j], NT rows of
// 64 doubles per array; the handle's slab images are read where they are (element (R, c) of an Ntot x N array:
// ((c / 16) KT + R / 4) 64 + 16 (R % 4) + c % 16, KT = 4 NT)
struct QuadMap {
    static constexpr int nleak = 16;
    int nrows;              // Ntot
    int NT;
    long long nq;           // quads
    int leak_row;
    size_t astride;         // NT nq 64, the doubles of an array.  (A member: spelled NT * nq * 64 in at(), hipcc folds the array index into the
                            // row term -- (arr NT + R / 16) nq 64 -- and forms every array's offset anew with a 64-bit multiply per row.)
    __device__ __forceinline__ size_t elem(int R, long long col) const
    {
        return (size_t)(R / 16) * ((size_t)nq * 64) + (size_t)(col / 4) * 64 + 16 * (R % 4) + 4 * ((R % 16) / 4) + (size_t)(col % 4);
    }
    __device__ __forceinline__ size_t at(int arr, int R, long long col) const { return arr * astride + elem(R, col); }
    __device__ __forceinline__ size_t leak(long long col, int k) const { return (size_t)leak_row * ((size_t)nq * 64) + elem(k, col); }
    __device__ __forceinline__ size_t target(int ic, int R) const { return ((size_t)(ic / 16) * 4 * NT + R / 4) * 64 + 16 * (R % 4) + ic % 16; }
};

// A drift ensemble's tangent-linear files (jq_eval_f_g_grad_drifts_hvp): a member's N columns start at a fresh group of `cpg` column slots
// -- whole waves, a wave propagates with one member's operators -- so sample s, column ic is column slot s cpg + ic of the base layout.
template <class Base>
struct MemberMap {
    static constexpr int nleak = Base::nleak;
    Base b;
    int nrows, N;
    long long cpg;
    __device__ __forceinline__ long long slot(long long col) const { return (col / N) * cpg + col % N; }
    __device__ __forceinline__ size_t at(int arr, int R, long long col) const { return b.at(arr, R, slot(col)); }
    __device__ __forceinline__ size_t leak(long long col, int k) const { return b.leak(slot(col), k); }
    __device__ __forceinline__ size_t target(int ic, int R) const { return b.target(ic, R); }
};

// state files <- (Uinit, 0 ...): one file per grid row, dstride doubles apart (the directions of jq_eval_f_g_grad_hvp; an evaluation has one).
// uinit: [N][NP] (column ic of Uinit, zero padded); rows: rows of the file.  thread per column, grid = (columns / 64, files)
// Every group of cpg column slots holds ncols_used columns in front (one group of all the slots: the packed columns of an evaluation or of
// an ensemble over eps-nodes; a group per member of a drift ensemble: MemberMap).
__global__ void k_init_lane(double* state, long long ncols, int NP, int rows, long long dstride, const double* __restrict__ uinit, int N,
                            long long ncols_used, long long cpg)
{
    const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncols) return;
    double* st = state + (size_t)blockIdx.y * (size_t)dstride;
    const long long c = col % cpg;
    const int ic = (int)(c % N);
    for (int r = 0; r < rows; ++r) st[(size_t)r * ncols + col] = (r < NP && c < ncols_used) ? uinit[ic * NP + r] : 0.0;
}

// ... in the row-lane layout.  uinit: [N][16]; cpw, wpg: the column packing (RowlaneMap).  grid = (waves, files), block = 64
__global__ void k_init_rowlane(double* state, long long nw, int rows, long long dstride, const double* __restrict__ uinit, int N,
                               long long ncols_used, int cpw, int wpg)
{
    const int lane = threadIdx.x;
    const long long w = blockIdx.x;
    const int c = 4 * (int)(w % wpg) + (lane >> 4);      // slot inside the group
    const long long col = (w / wpg) * cpw + c;
    double* st = state + (size_t)blockIdx.y * (size_t)dstride + w * 64 + lane;
    const bool used = c < cpw && col < ncols_used;
    for (int r = 0; r < rows; ++r) st[(size_t)r * nw * 64] = (r == 0 && used) ? uinit[(col % N) * 16 + (lane & 15)] : 0.0;
}

// ... in the tangent-linear quad layout.  uimg: the slab image of Uinit; cpg: the column slots of a group (k_init_lane).
// grid = (quads, directions), block = 64
__global__ __launch_bounds__(64) void k_init_quad_tl(double* state, long long nq, long long dstride, const double* __restrict__ uimg, int NT,
                                                     int N, long long ncols_used, long long cpg)
{
    const int lane = threadIdx.x;
    const long long w = blockIdx.x;
    const long long col = (4 * w + (lane & 3)) % cpg;
    const int rowb = 4 * ((lane >> 2) & 3) + (lane >> 4);
    double* st = state + (size_t)blockIdx.y * (size_t)dstride + w * 64 + lane;
    const bool used = col < ncols_used;
    const int c = (int)(col % N);
    for (int r = 0; r < JQ_QUAD_TL_ROWS(NT); ++r) {
        const int R = 16 * r + rowb;
        st[(size_t)r * nq * 64] = (r < NT && used) ? uimg[((size_t)(c / 16) * 4 * NT + R / 4) * 64 + 16 * (R % 4) + c % 16] : 0.0;
    }
}

// Fidelity, leak integral and adjoint terminal condition per sample (see k_terminal), thread per sample; grid = (ceil(samples / 64), files),
// block = 64.  File blockIdx.y lies dstride doubles behind the one before and writes res[blockIdx.y][sample][4].  vtr, vti (dvr, dvi:
// the dVds image, read only when mode != 1): the images of the map's layout.
//   EP_SV   Stormer-Verlet, mode 1 .. 4 as in k_terminal
//   EP_IMR  implicit midpoint (src/evalobjgrad.jl:1221-1271): secondaryobjf = dt * tinv / 4 * sum(penal_m) (leak_scale),
//           lambda(T) = -2/N^2 (s1 Vtr + s2 Vti),  -2/N^2 (-s1 Vti + s2 Vtr)  with s1 + i s2 = N s  (true lambda_i, not negated)
//   EP_TL   tangent-linear files: mode 1 and its derivative, sd = tr(Vtg' Vd) / N and the tangent sd conj(Vtg) / N of lambda(T) in arrays 6, 7
// Every sum is a serial chain over the sample's columns in order and their rows in order.
enum { EP_SV, EP_IMR, EP_TL };
template <class Map, int FLAVOR>
__global__ __launch_bounds__(64) void k_terminal_cols(Map m, double* state, long long dstride, const double* __restrict__ vtr,
                                                      const double* __restrict__ vti, const double* __restrict__ dvr,
                                                      const double* __restrict__ dvi, int mode, int N, int nsamples, double leak_scale,
                                                      double* res)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nsamples) return;
    state += (size_t)blockIdx.y * (size_t)dstride;
    res += ((size_t)blockIdx.y * nsamples + s) * 4;
    constexpr bool TL = FLAVOR == EP_TL;
    if (FLAVOR != EP_SV) mode = 1;
    // the second trace (dre, dim): the tangent state against the target (EP_TL), the state against the dVds image (s_D, modes 3 and 4)
    // (the nest is compiled with and without it: tested at run time inside the row loop, it keeps hipcc from merging a column's loads)
    double re = 0.0, im = 0.0, lk = 0.0, dre = 0.0, dim = 0.0;
    auto sums = [&](auto second) {
        for (int ic = 0; ic < N; ++ic) {
            const long long col = (long long)s * N + ic;
            for (int R = 0; R < m.nrows; ++R) {
                const double u = state[m.at(0, R, col)], v = state[m.at(1, R, col)];
                const double tr = vtr[m.target(ic, R)], ti = vti[m.target(ic, R)];
                re += jq_det2(u, tr, v, ti);
                im += jq_dot2(u, ti, v, tr);
                if constexpr (decltype(second)::value) {
                    const double a = TL ? state[m.at(4, R, col)] : u, b = TL ? state[m.at(5, R, col)] : v;
                    const double xr = TL ? tr : dvr[m.target(ic, R)], xi = TL ? ti : dvi[m.target(ic, R)];
                    dre += jq_det2(a, xr, b, xi);
                    dim += jq_dot2(a, xi, b, xr);
                }
            }
            for (int k = 0; k < Map::nleak; ++k) lk += state[m.leak(col, k)];
        }
    };
    if (TL || mode >= 3) sums(std::true_type{});
    else sums(std::false_type{});
    re /= N, im /= N, dre /= N, dim /= N;
    // lambda(T) = a conj(X)/N  (+ s_D conj(T)/N in mode 4): a = s_D in mode 3, X = D in modes 2 and 4
    const double are = (mode == 3) ? dre : re, aim = (mode == 3) ? dim : im;
    const bool from_d = (mode == 2 || mode == 4);
    const double *xr = from_d ? dvr : vtr, *xi = from_d ? dvi : vti;
    for (int ic = 0; ic < N; ++ic) {
        const long long col = (long long)s * N + ic;
        for (int R = 0; R < m.nrows; ++R) {
            const double tr = xr[m.target(ic, R)], ti = xi[m.target(ic, R)];
            double lr = jq_dot2(aim, ti, are, tr), nb = jq_det2(aim, tr, are, ti);
            if constexpr (FLAVOR == EP_IMR) {
                // (k_terminal_rowlane_imr spelled these and the sums above a b + c d and left the fusion to the compiler; its code object fused
                // u tr and v tr of the trace, re tr and im tr here and im im of |s|^2, and rounded the other product: the calls of the other flavours)
                lr = -2.0 / N * lr;      // lambda_r
                nb = -2.0 / N * nb;      // the true lambda_i
            } else {
                lr = lr / N;             // lambda_r
                nb = -(nb / N);          // nb = -lambda_i
            }
            if (mode == 4) {
                const double yr = vtr[m.target(ic, R)], yi = vti[m.target(ic, R)];
                lr += jq_dot2(dim, yi, dre, yr) / N;
                nb += -(jq_det2(dim, yr, dre, yi) / N);
            }
            state[m.at(2, R, col)] = lr;
            state[m.at(3, R, col)] = nb;
            if constexpr (TL) {
                state[m.at(6, R, col)] = jq_dot2(dim, ti, dre, tr) / N;
                state[m.at(7, R, col)] = -(jq_det2(dim, tr, dre, ti) / N);
            }
        }
    }
    res[0] = 1.0 - jq_dot2(re, re, im, im);
    res[1] = leak_scale * lk;
    res[2] = re;
    res[3] = im;
}
