// One translation unit per (NT, BW, variant) object of the propagator kernels (parallel builds, and the MFMA register form can be
// chosen per object -- see Makefile).  What an object instantiates is listed in jq_inst_list.h; this file applies the list.
//   JQ_VARIANT 0: slab kernels, Neumann   1: slab kernels, Jacobi   2: cooperative (row-split) kernels
//              3: lane kernels (one lane per column; JQ_NT = padded Hilbert dimension NP, JQ_BW unused) and their tangent-linear twins
//              6: cooperative kernels of the implicit-midpoint integrator
//              7: quad-layout kernels of the implicit-midpoint integrator (JQ_BW = 7)
//              8: quad-layout slab kernels with 1 and 2 slabs per workgroup (JQ_BW = 7; variant 0 holds the 3-slab ones)
//              5: row-lane kernels of the implicit-midpoint integrator (JQ_NT = NPJ)
//              9: cooperative-quad kernels (one 16-row block per wave; single evaluations / small ensembles; JQ_BW = 7)
//              4: row-lane kernels (one lane per (row, column); JQ_NT = padded row length NPJ, JQ_BW unused)
//             11: kernels with the low-rank full leakage weights compiled in: quad layout with one slab per workgroup (JQ_BW = 7),
//                 slab kernels (other JQ_BW; built for <1, 0> and <6, 5>, which have no cooperative sibling)
//             13: variant 11's slab kernels with the Jacobi solver
//             14: tangent-linear twins of the quad-layout kernels (JQ_BW = 7; jq_eval_f_g_grad_hvp at Ntot > 16)
//             12: quad-layout backward sweep with the state and the adjoint chain of a column quad on two waves (JQ_BW = 7)
#if !defined(JQ_NT) || !defined(JQ_BW) || !defined(JQ_VARIANT)
#error "compile with -DJQ_NT=<tiles> -DJQ_BW=<band> -DJQ_VARIANT=<0..14>"
#endif
#include "jq_inst_list.h"
#define JQ_DEF(name, ...) template __global__ void name<__VA_ARGS__>(PropArgs);
#if JQ_VARIANT == 9     // cooperative-quad (latency) kernels of the JQ_BW_T4 structure (JQ_BW = 7)
#include "jq_cq_split_kernels.h"
JQ_INST_U(JQ_DEF, JQ_NT, JQ_BW)
#if JQ_NT == 2
JQ_INST_U_DENSE(JQ_DEF, JQ_NT, JQ_BW)
#endif
#elif JQ_VARIANT == 12  // quad layout, backward sweep split over two waves per column quad (mid-size ensembles)
#include "jq_quad_split_kernels.h"
JQ_INST_P(JQ_DEF, JQ_NT, JQ_BW)
#elif JQ_VARIANT == 14  // quad layout, tangent-linear twins: column quads x directions
#include "jq_quad_tl_kernels.h"
JQ_INST_T(JQ_DEF, JQ_NT, JQ_BW)
#if JQ_NT >= 2                    // (JQ_SIZES_QUAD_TL: NT = 1 is Ntot <= 16, which has the lane and row-lane kernels' twins)
JQ_INST_T_TL(JQ_DEF, JQ_NT, JQ_BW)
#endif
#elif JQ_VARIANT == 10  // cooperative-quad kernels of the implicit-midpoint integrator (JQ_BW = 7, N = 4)
#include "jq_cq_imr_kernels.h"
JQ_INST_V(JQ_DEF, JQ_NT, JQ_BW)
#if JQ_NT <= 6
JQ_INST_V_IMR2(JQ_DEF, JQ_NT, JQ_BW)
#endif
#if JQ_NT == 2
JQ_INST_V_DENSE(JQ_DEF, JQ_NT, JQ_BW)
#endif
#elif JQ_VARIANT == 7
#include "jq_quad_imr_kernels.h"
JQ_INST_Q(JQ_DEF, JQ_NT, JQ_BW)
// (SPW = 2 -- two slabs per workgroup, two waves per SIMD, operators re-read from LDS per application -- was measured in round 3:
//  cnot3 x 3 072 samples 0.323 s against 0.225 s for three rounds of SPW = 1: the 36 LDS reads per application saturate the
//  LDS port with eight waves per CU; not instantiated)
#elif JQ_VARIANT == 6
#include "jq_coop_imr_kernels.h"
JQ_INST_I(JQ_DEF, JQ_NT, JQ_BW)
#if JQ_NT >= 2                    // N > 16 columns per evaluation (needs Ntot > 16): one workgroup per evaluation, its parts in turn
JQ_INST_I_PARTS(JQ_DEF, JQ_NT, JQ_BW)
#endif
#if JQ_NT == 6 && JQ_BW == 5      // dense 96 x 96: both images of a step do not fit the LDS -- read from HBM / L2 per product
JQ_INST_I_HBM(JQ_DEF, JQ_NT, JQ_BW)
#endif
#elif JQ_VARIANT == 5
#include "jq_rowlane_imr_kernels.h"
JQ_INST_M(JQ_DEF, JQ_NT)
#elif JQ_VARIANT == 4
#include "jq_rowlane_tl_kernels.h"
JQ_INST_R(JQ_DEF, JQ_NT)
#if JQ_NT >= 12                   // (JQ_SIZES_ROWLANE_TL: Ntot <= 6 has the lane kernels' twins, Ntot 7 and 8 run on the sequential route)
JQ_INST_R_TL(JQ_DEF, JQ_NT)
#endif
#elif JQ_VARIANT == 3
#include "jq_lane_tl_kernels.h"
JQ_INST_L(JQ_DEF, JQ_NT)
#if JQ_NT <= 6                    // (JQ_SIZES_LANE_TL: NP = 8 spills; jq_eval_f_g_grad_hvp runs it on the sequential route)
JQ_INST_L_TL(JQ_DEF, JQ_NT)
#endif
#elif JQ_VARIANT == 2
#include "jq_coop_kernels.h"
JQ_INST_C(JQ_DEF, JQ_NT, JQ_BW)
#else
#include "jq_kernels.h"
#if JQ_BW == 7 && JQ_VARIANT == 11  // quad layout, one slab per workgroup, full leakage weights (jq_update_wmat)
JQ_INST_WQ(JQ_DEF, JQ_NT, JQ_BW)
#elif JQ_VARIANT == 11              // slab kernels with the full leakage weights
JQ_INST_W(JQ_DEF, JQ_NT, JQ_BW)
#elif JQ_VARIANT == 13              // ... with the Jacobi solver too (ABI 5)
JQ_INST_X(JQ_DEF, JQ_NT, JQ_BW)
#elif JQ_BW == 7 && JQ_VARIANT == 8   // quad layout, workgroups of 4 / 8 waves (1 / 2 slabs): built with the max-ILP scheduler (Makefile)
JQ_INST_S(JQ_DEF, JQ_NT, JQ_BW)
#elif JQ_BW == 7                    // quad layout, workgroups of 12 waves (3 slabs, 168 registers per wave): default scheduler
JQ_INST_KQ(JQ_DEF, JQ_NT, JQ_BW)
#elif JQ_VARIANT == 1
JQ_INST_J(JQ_DEF, JQ_NT, JQ_BW)
#else
JQ_INST_K(JQ_DEF, JQ_NT, JQ_BW)
#endif
#endif
