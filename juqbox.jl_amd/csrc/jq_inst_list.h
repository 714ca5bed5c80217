// jq_inst_list.h -- THE list of the propagator-kernel instantiations of libjuqbox_hip.so.  Macros only; includes nothing.
//
// Every instantiation is named here once, as X(<template>, <template arguments>): jq_kernel_inst.hip defines it in its object
// (template __global__ void ...), jq_host_select.h declares it (extern template ...) and builds the tables its select_* functions
// look kernels up in, jq_dump_selection.h maps kernel pointers back to spellings.  Trailing template arguments that are left out
// are the templates' defaults, all of them `false`.
//
// JQ_INST_<list>(X, nt, bw) / (X, np): the instantiations one object holds, in the order the object defines them (the order of
// the code in the object; keep it).  (nt, bw) / np are the -DJQ_NT / -DJQ_BW of the object (csrc/Makefile).
// JQ_SIZES_<list>(L, A): the objects of a list -- L(A, nt, bw) / L(A, np) for each, e.g. JQ_SIZES_U(JQ_INST_U, X).
// JQ_OBJECT_FAMILIES(Y): Y(<object letter>, <size list>, <instantiation list>) for every pair of the two.
// ---------------------------------------------------------------------------------------------
#define JQ_MINW_OF(nt) (((nt) <= JQ_MINW_MAXNT) ? 2 : 1)

// k_ / j_: slab kernels, Neumann / Jacobi solver
#define JQ_INST_K(X, nt, bw) X(k_forward, nt, bw, JQ_MINW_OF(nt), false) X(k_backward, nt, bw, JQ_MINW_OF(nt), false)
#define JQ_INST_J(X, nt, bw) X(k_forward, nt, bw, JQ_MINW_OF(nt), true) X(k_backward, nt, bw, JQ_MINW_OF(nt), true)
// k_<nt>_7: quad layout (bw = JQ_BW_T4Q), three slabs per workgroup -- <.., JAC, WLR, UNI, ORD, SC> (k_forward: <.., JAC, WLR, UNI, SC>)
#define JQ_INST_KQ(X, nt, bw)                                                                                           \
    X(k_forward, nt, bw, 3, false) X(k_backward, nt, bw, 3, false)                                                      \
    X(k_backward, nt, bw, 3, false, false, true)                   /* UNI: one ensemble sample per wave */              \
    X(k_backward, nt, bw, 3, false, false, true, true)             /* UNI + ORD: control q on subsystem q only */       \
    X(k_forward, nt, bw, 3, false, false, false, true)             /* SC: uniform S images, compact S operands */       \
    X(k_backward, nt, bw, 3, false, false, true, true, true)       /* UNI + ORD + SC */
// s_: quad layout, one / two slabs per workgroup
#define JQ_INST_S(X, nt, bw) \
    X(k_forward, nt, bw, 1, false) X(k_backward, nt, bw, 1, false) X(k_forward, nt, bw, 2, false) X(k_backward, nt, bw, 2, false)
// w_<nt>_7: quad layout, one slab per workgroup, low-rank full leakage weights (jq_update_wmat)
#define JQ_INST_WQ(X, nt, bw) X(k_forward, nt, bw, 1, false, true) X(k_backward, nt, bw, 1, false, true)
// w_ / x_: slab kernels with the full leakage weights, Neumann / Jacobi solver (<1, 0> and <6, 5>: no cooperative sibling)
#define JQ_INST_W(X, nt, bw) X(k_forward, nt, bw, JQ_MINW_OF(nt), false, true) X(k_backward, nt, bw, JQ_MINW_OF(nt), false, true)
#define JQ_INST_X(X, nt, bw) X(k_forward, nt, bw, JQ_MINW_OF(nt), true, true) X(k_backward, nt, bw, JQ_MINW_OF(nt), true, true)
// u_: cooperative-quad (latency) kernels -- k_forward_cq<NT, MODD, NS, WLR, DN>, k_backward_cq<NT, MODD, ORD, WLR, DN>,
// k_backward_cq3<NT, MODD, ORD, NR, WLR, DN>.  MODD: odd number of Neumann terms; NS: column quads per workgroup; ORD: control q
// acts on subsystem q only; NR: workgroups per column quad; WLR: full leakage weights (real, rank <= 4); DN: the dense policy
#define JQ_INST_U(X, nt, bw)                                                                                            \
    X(k_forward_cq, nt, false, 1) X(k_backward_cq, nt, false, false) X(k_backward_cq, nt, false, true)                  \
    X(k_forward_cq, nt, true, 1) X(k_forward_cq, nt, false, 2) X(k_forward_cq, nt, true, 2)                             \
    X(k_backward_cq, nt, true, false) X(k_backward_cq, nt, true, true)                                                  \
    X(k_forward_cq, nt, false, 1, true) X(k_forward_cq, nt, true, 1, true)                                              \
    X(k_backward_cq, nt, false, false, true) X(k_backward_cq, nt, false, true, true)                                    \
    X(k_backward_cq, nt, true, false, true) X(k_backward_cq, nt, true, true, true)                                      \
    X(k_backward_cq3, nt, false, false, 3) X(k_backward_cq3, nt, false, true, 3)                                        \
    X(k_backward_cq3, nt, true, false, 3) X(k_backward_cq3, nt, true, true, 3)                                          \
    X(k_backward_cq3, nt, false, false, 2) X(k_backward_cq3, nt, false, true, 2)                                        \
    X(k_backward_cq3, nt, true, false, 2) X(k_backward_cq3, nt, true, true, 2)                                          \
    X(k_backward_cq3, nt, false, false, 3, true) X(k_backward_cq3, nt, false, true, 3, true)                            \
    X(k_backward_cq3, nt, true, false, 3, true) X(k_backward_cq3, nt, true, true, 3, true)                              \
    X(k_backward_cq3, nt, false, false, 2, true) X(k_backward_cq3, nt, false, true, 2, true)                            \
    X(k_backward_cq3, nt, true, false, 2, true) X(k_backward_cq3, nt, true, true, 2, true)
// ... u_2_7 also: the dense policy (17 .. 32 levels without the 4 x 4 x n structure)
#define JQ_INST_U_DENSE(X, nt, bw)                                                                                      \
    X(k_forward_cq, nt, false, 1, false, true) X(k_forward_cq, nt, true, 1, false, true)                                \
    X(k_backward_cq, nt, false, false, false, true) X(k_backward_cq, nt, true, false, false, true)                      \
    X(k_backward_cq3, nt, false, false, 3, false, true) X(k_backward_cq3, nt, true, false, 3, false, true)              \
    X(k_backward_cq3, nt, false, false, 2, false, true) X(k_backward_cq3, nt, true, false, 2, false, true)
// p_: quad layout, backward sweep split over two waves per column quad -- k_backward_qsplit<NT, ORD, QW, RIDE>
#define JQ_INST_P(X, nt, bw)                                                                                            \
    X(k_backward_qsplit, nt, false, 4) X(k_backward_qsplit, nt, true, 4) X(k_backward_qsplit, nt, false, 2)             \
    X(k_backward_qsplit, nt, true, 2) X(k_backward_qsplit, nt, true, 4, true) X(k_backward_qsplit, nt, true, 2, true)
// t_: tangent-linear twins of the quad-layout kernels (jq_quad_tl_kernels.h; jq_eval_f_g_grad_hvp at Ntot > 16): column quads x directions.
// (JQ_INST_T: what every t_ object of the Makefile's QUAD list holds -- nothing: t_1_7 is empty)
#define JQ_INST_T(X, nt, bw)
#define JQ_INST_T_TL(X, nt, bw) X(k_forward_quad_tl, nt) X(k_backward_quad_tl, nt)
// v_: cooperative-quad kernels of the implicit-midpoint integrator -- <NT, DN>; imr3: three workgroups per evaluation; imr2: state and
// adjoint chain on two sets of waves (NT <= 6); v_2_7 also: the dense policy
#define JQ_INST_V(X, nt, bw) X(k_forward_cq_imr, nt) X(k_backward_cq_imr, nt) X(k_backward_cq_imr3, nt)
#define JQ_INST_V_IMR2(X, nt, bw) X(k_backward_cq_imr2, nt)
#define JQ_INST_V_DENSE(X, nt, bw) X(k_forward_cq_imr, nt, true) X(k_backward_cq_imr, nt, true) X(k_backward_cq_imr3, nt, true)
// q_: quad-layout kernels of the implicit-midpoint integrator -- <NT, SPW>
#define JQ_INST_Q(X, nt, bw) X(k_forward_quad_imr, nt, 1) X(k_backward_quad_imr, nt, 1)
// i_: cooperative kernels of the implicit-midpoint integrator -- <NT, BW, HBM>; parts: N > 16, one workgroup per evaluation (NT >= 2);
// i_6_5 also: dense 96 x 96 with the images read from HBM / L2
#define JQ_INST_I(X, nt, bw) X(k_forward_coop_imr, nt, bw, (nt > 6)) X(k_backward_coop_imr, nt, bw, (nt > 6))
#define JQ_INST_I_PARTS(X, nt, bw) X(k_forward_coop_imr_parts, nt, bw, (nt > 6)) X(k_backward_coop_imr_parts, nt, bw, (nt > 6))
#define JQ_INST_I_HBM(X, nt, bw)                                                                                        \
    X(k_forward_coop_imr, nt, bw, true) X(k_backward_coop_imr, nt, bw, true)                                            \
    X(k_forward_coop_imr_parts, nt, bw, true) X(k_backward_coop_imr_parts, nt, bw, true)
// m_ / r_: row-lane kernels (np = padded row length NPJ), implicit midpoint / Stormer-Verlet -- k_forward_rowlane<NPJ, WF, HIST>,
// k_backward_rowlane<NPJ, WF>; rowlane2 / rowlane3 / imr2: the backward sweep on two / three waves
#define JQ_INST_M(X, np) X(k_forward_rowlane_imr, np) X(k_backward_rowlane_imr, np) X(k_backward_rowlane_imr2, np)
#define JQ_INST_R(X, np)                                                                                                \
    X(k_forward_rowlane, np) X(k_forward_rowlane, np, false, true) X(k_backward_rowlane, np) X(k_backward_rowlane2, np) \
    X(k_backward_rowlane3, np) X(k_forward_rowlane, np, true, true) X(k_backward_rowlane, np, true)
// ... and the tangent-linear twins of the one-wave kernels (jq_rowlane_tl_kernels.h; jq_eval_f_g_grad_hvp at Ntot 9 .. 16): waves x directions
#define JQ_INST_R_TL(X, np) X(k_forward_rowlane_tl, np) X(k_backward_rowlane_tl, np)
// l_: lane kernels (np = padded Hilbert dimension NP)
#define JQ_INST_L(X, np) X(k_forward_lane, np) X(k_backward_lane, np)
// ... and their tangent-linear twins (jq_lane_tl_kernels.h; jq_eval_f_g_grad_hvp): columns x directions
#define JQ_INST_L_TL(X, np) X(k_forward_lane_tl, np) X(k_backward_lane_tl, np)
// c_: cooperative (row-split) kernels
#define JQ_INST_C(X, nt, bw) X(k_forward_coop, nt, bw) X(k_backward_coop, nt, bw)

// ---- the objects (csrc/Makefile: INST, COOP, BIG, QUAD, QUADBIG, LANE, ROWLANE and the loose ones) ----------------------------------
#define JQ_SIZES_SLAB(L, A)                                                                                             \
    L(A, 1, 0) L(A, 2, 0) L(A, 2, 1) L(A, 3, 0) L(A, 3, 1) L(A, 3, 2) L(A, 4, 0) L(A, 4, 1) L(A, 4, 2) L(A, 4, 3)       \
    L(A, 5, 0) L(A, 5, 1) L(A, 5, 2) L(A, 5, 4) L(A, 6, 0) L(A, 6, 1) L(A, 6, 2) L(A, 6, 5) L(A, 2, 9) L(A, 3, 9)       \
    L(A, 4, 9) L(A, 5, 9) L(A, 6, 9) L(A, 1, 8) L(A, 2, 8) L(A, 3, 8) L(A, 4, 8) L(A, 5, 8) L(A, 6, 8) L(A, 7, 8) L(A, 8, 8)
#define JQ_SIZES_COOP(L, A)                                                                                             \
    L(A, 2, 0) L(A, 2, 1) L(A, 3, 0) L(A, 3, 1) L(A, 3, 2) L(A, 4, 0) L(A, 4, 1) L(A, 4, 2) L(A, 4, 3) L(A, 5, 0)       \
    L(A, 5, 1) L(A, 5, 2) L(A, 5, 4) L(A, 6, 0) L(A, 6, 1) L(A, 6, 2) L(A, 6, 5) L(A, 2, 9) L(A, 3, 9) L(A, 4, 9)       \
    L(A, 5, 9) L(A, 6, 9)
// (Ntot > 96, NT = 7 .. 16: block band 1, 2 or dense -- band code 15 for every NT; operators read from HBM)
#define JQ_SIZES_BIG(L, A)                                                                                              \
    L(A, 7, 1) L(A, 7, 2) L(A, 7, 15) L(A, 8, 1) L(A, 8, 2) L(A, 8, 15) L(A, 9, 1) L(A, 9, 2) L(A, 9, 15) L(A, 10, 1)   \
    L(A, 10, 2) L(A, 10, 15) L(A, 11, 1) L(A, 11, 2) L(A, 11, 15) L(A, 12, 1) L(A, 12, 2) L(A, 12, 15) L(A, 13, 1)      \
    L(A, 13, 2) L(A, 13, 15) L(A, 14, 1) L(A, 14, 2) L(A, 14, 15) L(A, 15, 1) L(A, 15, 2) L(A, 15, 15) L(A, 16, 1)      \
    L(A, 16, 2) L(A, 16, 15)
#define JQ_SIZES_QUAD(L, A) L(A, 1, 7) L(A, 2, 7) L(A, 3, 7) L(A, 4, 7) L(A, 5, 7) L(A, 6, 7)
#define JQ_SIZES_QUADBIG(L, A) L(A, 7, 7) L(A, 8, 7)
// (the tangent-linear kernels of the t_ objects: none at NT = 1 -- Ntot <= 16, the lane and row-lane routes -- and none at NT = 7, 8, whose
// backward kernels do not build without scratch)
#define JQ_SIZES_QUAD_TL(L, A) L(A, 2, 7) L(A, 3, 7) L(A, 4, 7) L(A, 5, 7) L(A, 6, 7)
#define JQ_SIZES_LANE(L, A) L(A, 2) L(A, 4) L(A, 6) L(A, 8)
// (the tangent-linear kernels of the l_ objects: none at NP = 8, whose backward kernel does not fit the 512 registers of a wave without scratch)
#define JQ_SIZES_LANE_TL(L, A) L(A, 2) L(A, 4) L(A, 6)
#define JQ_SIZES_ROWLANE(L, A) L(A, 2) L(A, 4) L(A, 6) L(A, 8) L(A, 12) L(A, 16)
// (the tangent-linear kernels of the r_ objects: the row lengths jq_eval_f_g_grad_hvp has no lane kernel for; none at NPJ = 8, Ntot 7 and 8)
#define JQ_SIZES_ROWLANE_TL(L, A) L(A, 12) L(A, 16)
#define JQ_SIZES_QUAD8(L, A) JQ_SIZES_QUAD(L, A) JQ_SIZES_QUADBIG(L, A)      // k_<nt>_7, s_, q_, w_<nt>_7
#define JQ_SIZES_QUAD7(L, A) JQ_SIZES_QUAD(L, A) L(A, 7, 7)                  // u_, v_
#define JQ_SIZES_DENSE(L, A) L(A, 2, 7)                                      // the dense policy of u_ / v_
#define JQ_SIZES_WX(L, A) L(A, 1, 0) L(A, 6, 5)                              // w_ / x_ slab objects
#define JQ_SIZES_C(L, A) JQ_SIZES_COOP(L, A) JQ_SIZES_BIG(L, A)              // c_, the parts kernels of i_
#define JQ_SIZES_I(L, A) JQ_SIZES_C(L, A) L(A, 1, 0)                         // i_
#define JQ_SIZES_HBM(L, A) L(A, 6, 5)                                        // the HBM variants of i_6_5

#define JQ_OBJECT_FAMILIES(Y)                                                                                           \
    Y(k, JQ_SIZES_SLAB, JQ_INST_K) Y(j, JQ_SIZES_SLAB, JQ_INST_J) Y(k, JQ_SIZES_QUAD8, JQ_INST_KQ)                      \
    Y(s, JQ_SIZES_QUAD8, JQ_INST_S) Y(w, JQ_SIZES_QUAD8, JQ_INST_WQ) Y(w, JQ_SIZES_WX, JQ_INST_W)                       \
    Y(x, JQ_SIZES_WX, JQ_INST_X) Y(u, JQ_SIZES_QUAD7, JQ_INST_U) Y(u, JQ_SIZES_DENSE, JQ_INST_U_DENSE)                  \
    Y(p, JQ_SIZES_QUAD, JQ_INST_P) Y(t, JQ_SIZES_QUAD, JQ_INST_T) Y(t, JQ_SIZES_QUAD_TL, JQ_INST_T_TL)                  \
    Y(v, JQ_SIZES_QUAD7, JQ_INST_V) Y(v, JQ_SIZES_QUAD, JQ_INST_V_IMR2)                                                 \
    Y(v, JQ_SIZES_DENSE, JQ_INST_V_DENSE) Y(q, JQ_SIZES_QUAD8, JQ_INST_Q) Y(i, JQ_SIZES_I, JQ_INST_I)                   \
    Y(i, JQ_SIZES_C, JQ_INST_I_PARTS) Y(i, JQ_SIZES_HBM, JQ_INST_I_HBM) Y(m, JQ_SIZES_ROWLANE, JQ_INST_M)               \
    Y(r, JQ_SIZES_ROWLANE, JQ_INST_R) Y(r, JQ_SIZES_ROWLANE_TL, JQ_INST_R_TL) Y(l, JQ_SIZES_LANE, JQ_INST_L)            \
    Y(l, JQ_SIZES_LANE_TL, JQ_INST_L_TL)                                                                                \
    Y(c, JQ_SIZES_C, JQ_INST_C)
// the host translation unit's own propagator kernels beyond those of jq_huge_kernels.h: the tangent-linear forward sweep of
// jq_tl_kernels.h and the tangent of the adjoint sweep of jq_tl_adjoint_kernels.h (run-time size like them; every other instantiation
// has its object)
#define JQ_INST_HOST(X) X(k_forward_tl) X(k_backward_tl)
