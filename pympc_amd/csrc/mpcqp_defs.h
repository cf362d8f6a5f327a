// mpcqp_defs.h -- part of libmpcqp_hip: the constants both translation units share.
//   mpcqp.hip     host side, C ABI and every kernel with 256-thread workgroups (NT = 256, four waves: one per SIMD)
//   mpcqp_w8.hip  the same device headers compiled once more with NT = 512 (eight waves: two per SIMD) inside namespace w8, for the
//                 kernels of the latency backend at one instance per compute unit (MODE_BCRT, mpcqp_latw.h): a lone instance is bound by
//                 the stalls of its in-order waves -- dependent MFMAs (44 cycles), LDS round trips, double-precision vector
//                 instructions (32 cycles dependent) -- and a second wave on the same SIMD issues into them
#pragma once

#ifndef NT
#define NT 256                 // threads per workgroup (one workgroup = one MPC instance)
#endif
#define NWAVES (NT / 64)
#define QP_INFTY 1e30
#define MIN_SCALING 1e-4
#define MAX_SCALING 1e4
#define RHO_MIN 1e-6
#define RHO_MAX 1e6
#define RHO_EQ_OVER_RHO_INEQ 1e3
#define RHO_TOL 1e-4

// Which k_mpc_run<NB, LDSS, NXT, NUT, MODE, LOOP> instantiation a handle runs (run_kernel_id in mpcqp_plan.h decides; LOOP is the launch's: closed
// loop or solve); w8: the 512-thread one of mpcqp_w8.hip.  The two tables below are ALL instantiations of the library, each row for LOOP false and true:
// the launch dispatches over them, mpcqp_kernel_name prints the same id.  (MODE_*: mpcqp_phases.h.)
struct RunKernelId { int nb; bool ldss; int nxt, nut, mode; bool w8; };
constexpr bool same_kernel(const RunKernelId &a, const RunKernelId &b) {
    return a.nb == b.nb && a.ldss == b.ldss && a.nxt == b.nxt && a.nut == b.nut && a.mode == b.mode && a.w8 == b.w8;
}
//  X(NB, LDSS, NXT, NUT, MODE)
#define MPCQP_RUN_KERNELS_256(X) \
    X(16, true, 0, 0, MODE_DENSE) \
    X(16, true, 12, 4, MODE_BCRT + 31) X(16, true, 0, 0, MODE_BCRT + 31) X(16, true, 0, 0, MODE_BCRT + 21) X(16, true, 0, 0, MODE_BCRT + 11) \
    X(16, true, 12, 4, MODE_BCR + 31) X(16, true, 0, 0, MODE_BCR + 31) X(16, true, 0, 0, MODE_BCR + 21) X(16, true, 0, 0, MODE_BCR + 11) \
    X(16, true, 12, 4, MODE_CHAIN) X(32, false, 20, 8, MODE_CHAIN) \
    X(16, false, 4, 1, MODE_BORDER) X(16, false, 4, 1, MODE_CHAIN) \
    X(16, true, 0, 0, MODE_BORDER) X(16, true, 0, 0, MODE_CHAIN) X(16, false, 0, 0, MODE_BORDER) X(16, false, 0, 0, MODE_CHAIN) \
    X(32, true, 0, 0, MODE_BORDER) X(32, true, 0, 0, MODE_CHAIN) X(32, false, 0, 0, MODE_BORDER) X(32, false, 0, 0, MODE_CHAIN) \
    X(64, false, 0, 0, MODE_BORDER) X(64, false, 0, 0, MODE_CHAIN) X(128, false, 0, 0, MODE_BORDER) X(128, false, 0, 0, MODE_CHAIN)
// 512 threads: ONE long-horizon controller on grouped stages with the round staged in LDS (the reference's cart pole -- its notebook and Kalman
// examples -- with compile-time dimensions, any other nx + nu <= 8 through the generic instantiation), and the cyclic reduction with a dense top.
// (The order of the rows is the order of the kernels in the code object: where a kernel's code lands moved the headline rate by ~ 1 %, LAB_NOTES.md.)
#define MPCQP_RUN_KERNELS_512(X) \
    X(16, false, 4, 1, MODE_BORDER) X(16, false, 4, 1, MODE_CHAIN) X(16, false, 0, 0, MODE_BORDER) X(16, false, 0, 0, MODE_CHAIN) \
    X(16, true, 12, 4, MODE_BCRT + 31) X(16, true, 0, 0, MODE_BCRT + 31) X(16, true, 0, 0, MODE_BCRT + 21) X(16, true, 0, 0, MODE_BCRT + 11)

#ifdef MPCQP_LAT_ONLY
constexpr bool kLatOnly = true;    // this translation unit instantiates the latency kernels only: the other backends' code is parsed, never instantiated
#else
constexpr bool kLatOnly = false;
#endif
