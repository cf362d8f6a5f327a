// mpcqp.hip -- hand-written HIP (gfx950 / MI355X) implementation of pyMPC's QP hot path:
//   * construction of the MPC quadratic program from (Ad,Bd,Qx,QxN,Qu,QDu,bounds)   [mpc.py:386-608]
//   * OSQP-style ADMM solve of that program, one persistent workgroup per MPC instance [mpc.py:266,369,454]
//
// Design:
//   - the QP matrices are never stored; P, A, A' are applied matrix-free from the stage data
//     (row "visitors" below enumerate the nonzeros of one row exactly as the reference lays them out);
//   - the ADMM linear system is the reduced KKT matrix  K = c P + sigma D^-2 + A' diag(rho E^2) A
//     (OSQP's quasi-definite KKT with the constraint block eliminated, expressed in UNSCALED variables:
//     Ruiz scaling D,E,c enters only through the metric vectors  s = sigma/D^2  and  omega = rho E^2);
//     with the slack variables eliminated it is block tridiagonal along the horizon with (nx+nu)^2 blocks
//     and is factored by a block LDL' whose factor, stored in FP64-MFMA operand order, streams from HBM/L2
//     every iteration;
//   - one 256-thread workgroup owns one instance for the whole solve (or K closed-loop steps): iterate in LDS,
//     two waves run the sequential block forward/backward half-sweeps of the twisted factorization on the matrix
//     cores (v_mfma_f64_4x4x4_4b_f64, stage output registers = next stage's B operand), all waves run the
//     stage-parallel parts.
//
//   - that is the bandwidth backend (any size, large batches).  Further KKT backends, chosen per handle at mpcqp_create (DESIGN.md
//     section 3): block cyclic reduction with the factor resident on the compute unit for 16 x 16 stages at small batches -- on 512-thread
//     workgroups with a dense top (mpcqp_latw.h, compiled in mpcqp_w8.hip; mpcqp_bcr.h, mpcqp_lat.h: the 256-thread original) --, an explicit K^-1
//     held in registers for the reference's own small examples (mpcqp_dense.h, mpcqp_tiny.h), grouped small stages for long horizons
//     (mpcqp_group.h), and plain vector-ALU block LDL' for stages wider than 32 (mpcqp_wide.h, mpcqp_huge.h).
//
// This file: host side and C ABI (include/mpcqp.h).  Device code: mpcqp_layout.h, mpcqp_qp.h, mpcqp_factor.h, mpcqp_sweeps.h,
// mpcqp_group.h, mpcqp_bcr.h, mpcqp_wide.h, mpcqp_huge.h, mpcqp_dense.h, mpcqp_border.h, mpcqp_phases.h, mpcqp_tiny.h, mpcqp_lat.h, mpcqp_latw.h,
// mpcqp_kernels.h (the last block also compiled at 512 threads per workgroup by mpcqp_w8.hip); host only:
// mpcqp_plan.h (what mpcqp_create decides before it allocates -- backend, LDS layout, solve kernel -- and the getters' arithmetic on it:
// no HIP call, runs without a GPU), mpcqp_csc.h (one translation unit).  The solve kernels' instantiations: the two tables of mpcqp_defs.h.
//
// FP64 throughout.  No CPU fallback exists in this library.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sched.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/mpcqp.h"
#include "../../include/mpcqp_polish.h"
#include "../../include/mpcqp_model.h"
#include "../../include/mpcqp_adjoint.h"
#include "../../include/mpcqp_adjoint_model.h"
#include "../../include/mpcqp_rollout.h"
#include "../../include/mpcqp_rollout_est.h"
#include "../../include_ext/mpcqp_rollout_tv.h"
#include "../../include_ext2/mpcqp_rollout_tv_est.h"
#include "../../include/mpcqp_adjoint_bounds.h"
#include "../../include_ext4/mpcqp_affine.h"
#include "../../include_ext5/mpcqp_rollout_affine.h"

#include "mpcqp_defs.h"

// one polite spin of a host-side busy wait
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#else
    __asm__ __volatile__("" ::: "memory");
#endif
}

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
int mpcqp_set_error(int code, const char *msg) { return fail(code, msg); }      // the way of mpcqp_riccati.hip to mpcqp_last_error
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    return fail(MPCQP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

#include "mpcqp_layout.h"
#include "mpcqp_qp.h"
#include "mpcqp_factor.h"
#include "mpcqp_sweeps.h"
#include "mpcqp_group.h"
#include "mpcqp_bcr.h"
#include "mpcqp_wide.h"
#include "mpcqp_huge.h"
#include "mpcqp_dense.h"
#include "mpcqp_border.h"
#include "mpcqp_phases.h"
#include "mpcqp_run.h"
#include "mpcqp_tiny.h"
#include "mpcqp_lat.h"
#include "mpcqp_latw.h"
#include "mpcqp_kernels.h"
#include "mpcqp_latw_check.h"
#include "mpcqp_plan.h"
#include "mpcqp_kpol.h"
#include "mpcqp_polish.h"
#include "mpcqp_adjoint.h"
#include "mpcqp_adjoint_model.h"
#include "mpcqp_adjoint_bounds.h"
#include "mpcqp_rollout.h"
#include "mpcqp_affine.h"
#include "mpcqp_csc.h"

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// mpcqp_w8.hip: the second translation unit (NT = 512).  kargs: this unit's RunKArgs, byte for byte the other's.
int mpcqp_w8_launch(const void *kargs, size_t kargs_bytes, const RunKernelId &id, int loop, int grid, size_t smem, hipStream_t stream);
#ifdef MPCQP_RUN_TIMING
void mpcqp_w8_ticks(unsigned long long *out16, unsigned long long *outw48, unsigned long long *outb128);
#endif
constexpr int BALANCE_EVERY = 16;  // solves between two rebuilds of the workgroup -> instance map
constexpr int QUEUE_ITEMS_PER_SLOT = 16;   // persistent closed-loop launches: queue items per resident workgroup slot (run_kernel_args)
constexpr int BALANCE_FIRST = 4;   // ... before the first one (an instance shows its character within a few solves; a short run should not end unbalanced)

struct PackItem { const double *src; double *dst; int w, stride; };
struct PackArgs { PackItem it[24]; int n, batch; };
struct mpcqp_handle : Plan {       // the plan (mpcqp_plan.h: ncu, batch, L, lds_state, smem, fsz, kernel) and what runs it on a device
    int device = 0;
    Ptrs P = {};
    mpcqp_settings S;
    hipStream_t stream = nullptr;
    bool own_stream = false, is_setup = false;
    std::vector<void *> allocs;
    double *u0_dev = nullptr;
    int *pending_dev = nullptr, *npending_dev = nullptr;   // two-launch solve: instances that need more than the first round
    int *perm_dev = nullptr;      // [batch] workgroup -> instance map (P.perm points here once a map has been built)
    int *qperm_dev = nullptr; bool qperm_set = false;     // [batch] the queue order of persistent launches (longest expected work first), once a map has been built
    int *vcur_dev = nullptr, *vdone_dev = nullptr; unsigned *vqueue_dev = nullptr;   // persistent launches: [slots] map entry each workgroup is working on; [batch] closed-loop steps done; the queue position
    std::vector<double> work_ema; // per instance: smoothed ADMM iterations per balancing interval (host)
    int solves_since_balance = 0, auto_balance = 1;
    int loop_parts = 0;           // queue-item parts per instance of the last persistent closed-loop launch (0: not persistent; mpcqp_dev_carry_stats)
    void *run_buf = nullptr; size_t run_bytes = 0;     // staging of mpcqp_mpc_run (disturbances, plant, trajectories)
    bool profiling = false;
    hipEvent_t ev0[MAXEV], ev1[MAXEV];   // ring of event pairs around the solve-kernel launches
    long long ev_count = 0;
    double run_ms = 0.0;
    long long run_launches = 0;
    int nevents = 0;                     // event pairs created so far (a partially built handle is destroyed cleanly)
    bool warm_x_pending = false;         // mpcqp_warm_start replaced x: the next solve starts from z = A x (osqp_warm_start)
    // mpcqp_step_host: mapped, coherent host memory the kernel reads its step data from and writes its results to
    double *pin_in = nullptr, *pin_out = nullptr; void *pin_in_dev = nullptr, *pin_out_dev = nullptr;
    unsigned *done_dev = nullptr; unsigned long long host_seq = 0; int pin_stride = 0; bool pin_tried = false;
    PackArgs pack = {};                  // device-resident sources of put() waiting for flush_puts
    CscSeam *csc = nullptr;              // patterns of P and A of a handle made by mpcqp_create_csc
    double *vec_buf = nullptr;           // staging of mpcqp_update_vectors' host arrays [q | l | u], allocated on first use, kept
    bool step_blank = false;             // set up through mpcqp_setup_qp: the step blob holds no x0 / u_{-1} / xref yet
    int *fown_dev = nullptr; unsigned *nshared_dev = nullptr;   // mpcqp_share_factor: [batch] factor slot per instance (P.fown points here while sharing is on); how many share
    mpcqp_polish_settings pol;           // mpcqp_set_polish (include/mpcqp_polish.h)
    PolishArgs pq = {};                  // the polish's buffers (pq.status null until first use)
    mpcqp_adjoint_settings adj;          // mpcqp_set_adjoint (include/mpcqp_adjoint.h)
    AdjointArgs aq = {};                 // the adjoint's buffers (aq.status null until first use)
    double *adj_gw = nullptr, *adj_gu0 = nullptr;      // staging of the caller's seeds [batch][n], [batch][nu]
    double *um1_used = nullptr; bool um1_moved = false;    // mpcqp_mpc_step: the u_{-1} its solve was made with, [batch][nu]; true while the step data hold the applied input instead
    double *adj_step = nullptr;          // the adjoint's copy of the step data with that u_{-1} put back [batch][step_sz] (null until first needed)
    double *adjm_out = nullptr, *adjm_sum = nullptr;   // mpcqp_adjoint_model: the per-instance model gradients (field-major, AdjointModelArgs::out) and their batch sum; null until first use
    double *adjb_out = nullptr, *adjb_sum = nullptr;   // mpcqp_adjoint_bounds: the per-instance bound gradients (field-major, AdjointBoundsArgs::out: the tail of adjm_out's block, where the sweep expects them) and their batch sum; null until first use
    RolloutTape tape = {}; void *tape_buf = nullptr; size_t tape_bytes = 0;      // mpcqp_rollout (include/mpcqp_rollout.h): the tape, one device block (null until the first rollout)
    int tape_ny = 0;                                           // > 0: the tape is one of the output-feedback loop (mpcqp_rollout_est, include/mpcqp_rollout_est.h)
    RolloutSlots tape_slots = {};                              // nslots > 0: the tape is one of the loop under a model schedule (mpcqp_rollout_tv, include_ext/mpcqp_rollout_tv.h) and carries its models
    RolloutGains tape_gains = {};                              // Lg non-null: the tape is one of the output-feedback loop under a schedule (mpcqp_rollout_tv_est, include_ext2/mpcqp_rollout_tv_est.h): nslots > 0 and tape_ny > 0 both
    int tape_xref_rows = 1; bool tape_valid = false;           // the reference shape of its entries; false once the model blob or the scaling the tape was made under is replaced
    const mpcqp_affine_traj *loop_aff = nullptr; size_t loop_aff_k0 = 0;      // mpcqp_mpc_loop_affine: the schedule of affine terms of the call in progress and the first step of its next launch (loop_run)
    double *aff_out = nullptr;           // mpcqp_adjoint_affine: the gradient of the term [batch][Np * nx] (null until first use)
    double *aff_gain = nullptr;          // mpcqp_gains_affine: K_d [batch][nu][Np * nx] (null until first use)
    RolloutAffine tape_aff = {};         // nslots > 0: the tape is one of mpcqp_rollout_affine (include_ext5/mpcqp_rollout_affine.h) and carries the terms it was made under
    bool has_solve = false;              // a solve has been launched and nothing k_adjoint reads (step data, model, iterate) was replaced since: what mpcqp_adjoint differentiates
};

extern "C" void mpcqp_default_settings(mpcqp_settings *s) {
    s->rho = 0.1; s->sigma = 1e-6; s->alpha = 1.6;
    s->eps_abs = 1e-3; s->eps_rel = 1e-3; s->eps_prim_inf = 1e-4; s->eps_dual_inf = 1e-4;
    s->adaptive_rho_tolerance = 5.0;
    s->max_iter = 4000; s->check_termination = 25; s->scaling = 10;
    s->adaptive_rho = 1; s->adaptive_rho_interval = 0; s->warm_start = 1; s->soft_constraints = 1;
    s->backend = MPCQP_BACKEND_AUTO; s->tuning = 0;
}

extern "C" const char *mpcqp_status_string(int status) {
    switch (status) {
        case MPCQP_SOLVED: return "solved";
        case MPCQP_SOLVED_INACCURATE: return "solved inaccurate";
        case MPCQP_MAX_ITER_REACHED: return "maximum iterations reached";
        case MPCQP_PRIMAL_INFEASIBLE: return "primal infeasible";
        case MPCQP_PRIMAL_INFEASIBLE_INACCURATE: return "primal infeasible inaccurate";
        case MPCQP_DUAL_INFEASIBLE: return "dual infeasible";
        case MPCQP_DUAL_INFEASIBLE_INACCURATE: return "dual infeasible inaccurate";
        case MPCQP_NON_CVX: return "problem non convex";
        default: return "unsolved";
    }
}

extern "C" const char *mpcqp_last_error(void) { return g_err.c_str(); }

extern "C" int mpcqp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

template <class T>
static int dalloc(mpcqp_handle *h, T **p, size_t count) {
    void *q = nullptr;
    HIPCHK(hipMalloc(&q, count * sizeof(T) + 16));
    HIPCHK(hipMemsetAsync(q, 0, count * sizeof(T) + 16, h->stream));
    h->allocs.push_back(q);
    *p = (T *)q;
    return 0;
}

// Four steps: argument checks; device and stream; the plan (mpcqp_plan.h) for the device's compute units; allocation.
extern "C" int mpcqp_create(mpcqp_handle **out, int device, int batch, int nx, int nu, int Np, int Nc, const mpcqp_settings *s) {
    std::string why;
    if (!out) return fail(MPCQP_ERR_ARG, "mpcqp_create: bad dimensions");
    if (int rc = plan_check_dims(batch, nx, nu, Np, Nc, &why)) return fail(rc, why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MPCQP_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(MPCQP_ERR_ARG, "mpcqp_create: bad device index");
    HIPCHK(hipSetDevice(device));
    mpcqp_handle *h = new mpcqp_handle();
    mpcqp_polish_default_settings(&h->pol);
    mpcqp_adjoint_default_settings(&h->adj);
    h->device = device;
    if (s) h->S = *s; else mpcqp_default_settings(&h->S);
    // (every failure from here on releases what has been created so far: mpcqp_destroy copes with a partial handle)
    auto hip_fail = [&](hipError_t e, const char *what) { std::string msg = std::string(what) + ": " + hipGetErrorString(e); mpcqp_destroy(h); return fail(MPCQP_ERR_HIP, msg); };
    { hipError_t e = hipStreamCreate(&h->stream); if (e != hipSuccess) { h->stream = nullptr; return hip_fail(e, "hipStreamCreate"); } }
    h->own_stream = true;
    for (int i = 0; i < MAXEV; ++i) {
        hipError_t e = hipEventCreate(&h->ev0[i]); if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
        e = hipEventCreate(&h->ev1[i]); if (e != hipSuccess) { hipEventDestroy(h->ev0[i]); return hip_fail(e, "hipEventCreate"); }
        h->nevents = i + 1;
    }
    int ncu = 0;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess) ncu = prop.multiProcessorCount; }
    if (int rc = make_plan(ncu, batch, nx, nu, Np, Nc, h->S, h, &why)) { mpcqp_destroy(h); return fail(rc, why); }
    const Lay &L = h->L;
    Ptrs &P = h->P;
    const size_t B = (size_t)batch;
    P.fsz = h->fsz;
    int rc = 0;
    rc |= dalloc(h, &P.model, B * L.model_sz); rc |= dalloc(h, &P.step, B * L.step_sz);
    rc |= dalloc(h, &P.D, B * L.n); rc |= dalloc(h, &P.E, B * L.m); rc |= dalloc(h, &P.c, B);
    rc |= dalloc(h, &P.omega, B * L.m); rc |= dalloc(h, &P.s, B * L.n); rc |= dalloc(h, &P.rho, B);
    rc |= dalloc(h, &P.F, (B + 1) * (size_t)P.fsz);      // (slot B: the shared factor of mpcqp_share_factor)
    rc |= dalloc(h, &h->fown_dev, B); rc |= dalloc(h, &h->nshared_dev, 4);
    rc |= dalloc(h, &P.x, B * L.n); rc |= dalloc(h, &P.z, B * L.m); rc |= dalloc(h, &P.y, B * L.m);
    rc |= dalloc(h, &P.xo, B * L.n); rc |= dalloc(h, &P.yo, B * L.m);
    rc |= dalloc(h, &P.dx, B * L.n); rc |= dalloc(h, &P.dy, B * L.m);
    rc |= dalloc(h, &P.qv, B * (size_t)(L.n_x + L.n_u));
    if (L.bcr) rc |= dalloc(h, &P.bws, B * (size_t)L.bcr * BcrFmt::WSTAGE);
    if (L.NB == 128) rc |= dalloc(h, &P.bws, B * (size_t)HugeFmt::GWS);      // (the factorization's work matrices of 128-wide stages)
    if (L.border) { rc |= dalloc(h, &P.Bb, B * (size_t)L.nu * L.N * L.NB); rc |= dalloc(h, &P.Zb, B * (size_t)L.nu * L.N * L.NB); rc |= dalloc(h, &P.Sig, B * (size_t)L.nu * L.nu); }
    rc |= dalloc(h, &P.Dt, B * L.n); rc |= dalloc(h, &P.Et, B * L.m);
    rc |= dalloc(h, &P.ctype, B * L.m); rc |= dalloc(h, &P.info, B); rc |= dalloc(h, &P.stats, 10);
    rc |= dalloc(h, &h->u0_dev, B * L.nu); rc |= dalloc(h, &h->um1_used, B * L.nu);
    rc |= dalloc(h, &P.work, B); rc |= dalloc(h, &h->perm_dev, B);
    rc |= dalloc(h, &h->vcur_dev, (size_t)std::max(4 * h->ncu, 1)); rc |= dalloc(h, &h->vqueue_dev, 4); rc |= dalloc(h, &h->vdone_dev, B); rc |= dalloc(h, &h->qperm_dev, B);
    rc |= dalloc(h, &P.tstamp, (size_t)TS_STRIDE * B);
    rc |= dalloc(h, &h->pending_dev, B); rc |= dalloc(h, &h->npending_dev, 4);
    if (h->S.tuning & MPCQP_TUNE_NO_BALANCE) h->auto_balance = 0;
    if (rc) { std::string msg = g_err; mpcqp_destroy(h); return fail(MPCQP_ERR_HIP, msg); }
    *out = h;
    return MPCQP_OK;
}

extern "C" void mpcqp_destroy(mpcqp_handle *h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (void *p : h->allocs) hipFree(p);
    if (h->run_buf) hipFree(h->run_buf);
    if (h->tape_buf) hipFree(h->tape_buf);
    delete h->csc;
    if (h->vec_buf) hipFree(h->vec_buf);
    if (h->pin_in) hipHostFree(h->pin_in);
    if (h->pin_out) hipHostFree(h->pin_out);
    for (int e = 0; e < h->nevents; ++e) { hipEventDestroy(h->ev0[e]); hipEventDestroy(h->ev1[e]); }
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    delete h;
}

extern "C" int mpcqp_set_stream(mpcqp_handle *h, void *hip_stream) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->own_stream) hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)hip_stream; h->own_stream = false;
    return MPCQP_OK;
}

extern "C" int mpcqp_synchronize(mpcqp_handle *h) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

// true if p points to device memory (results copied there are stream-ordered: the call need not wait for them)
static bool is_device_ptr(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice;
}

// Device scratch of one call: freed when the call returns, on every path.
struct Scratch {
    std::vector<void *> ptrs;
    ~Scratch() { for (void *p : ptrs) hipFree(p); }
    template <class T> hipError_t get(T **out, size_t count) {
        void *q = nullptr; hipError_t e = hipMalloc(&q, count * sizeof(T)); if (e == hipSuccess) { ptrs.push_back(q); *out = (T *)q; } return e;
    }
};

// strided upload: src [batch][w] -> dst [batch][stride] at column offset off.  Host sources: one 2-D copy each.  DEVICE sources (a caller that keeps its
// data on the GPU: bench.py, the RCCL shards) are collected and moved by ONE kernel launch (flush_puts) -- a device-to-device hipMemcpy2DAsync costs
// ~ 0.2 ms of host time each, and setup() issues seventeen of them: 4 of the 5.2 ms a cold setup() of 1024 instances took.
__global__ __launch_bounds__(256) void k_pack_rows(PackArgs A) {
    for (int i = 0; i < A.n; ++i) {
        const PackItem t = A.it[i];
        const int total = A.batch * t.w;
        for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
            const int b = idx / t.w, c = idx - b * t.w;
            t.dst[(size_t)b * t.stride + c] = t.src[idx];
        }
    }
}
static int flush_puts(mpcqp_handle *h) {
    PackArgs &A = h->pack;
    if (A.n == 0) return 0;
    A.batch = h->batch;
    int most = 1;
    for (int i = 0; i < A.n; ++i) most = std::max(most, A.it[i].w);
    const int grid = std::max(1, std::min(1024, (h->batch * most + 255) / 256));
    hipLaunchKernelGGL(k_pack_rows, dim3(grid), dim3(256), 0, h->stream, A);
    A.n = 0;
    HIPCHK(hipGetLastError());
    return 0;
}
static int put(mpcqp_handle *h, double *dst, int stride, int off, const double *src, int w) {
    if (is_device_ptr(src)) {
        if (h->pack.n == 24 && flush_puts(h)) return MPCQP_ERR_HIP;
        h->pack.it[h->pack.n++] = PackItem{src, dst + off, w, stride};
        return 0;
    }
    HIPCHK(hipMemcpy2DAsync(dst + off, sizeof(double) * (size_t)stride, src, sizeof(double) * (size_t)w,
                            sizeof(double) * (size_t)w, (size_t)h->batch, hipMemcpyDefault, h->stream));
    return 0;
}

#define DISPATCH_NB(NBV, EXPR) switch (NBV) { \
    case 16: { constexpr int NB = 16; EXPR; } break; \
    case 32: { constexpr int NB = 32; EXPR; } break; \
    case 64: { constexpr int NB = 64; EXPR; } break; \
    default: { constexpr int NB = 128; EXPR; } break; }

template <class K>
static int set_smem(K kernel, size_t bytes) {
    if (bytes > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

static int step_upload(mpcqp_handle *h, const double *x0, const double *um1, const double *xref, int xref_rows) {
    const Lay &L = h->L;
    h->has_solve = false;                           // (the bounds and the linear cost no longer belong to the iterate: mpcqp_adjoint waits for the next solve)
    if (x0 && put(h, h->P.step, L.step_sz, 0, x0, L.nx)) return MPCQP_ERR_HIP;
    if (um1 && put(h, h->P.step, L.step_sz, L.nx, um1, L.nu)) return MPCQP_ERR_HIP;
    if (xref) {
        if (xref_rows != 1 && xref_rows != L.N) return fail(MPCQP_ERR_ARG, "xref_rows must be 1 or Np+1");
        h->L.xref_rows = xref_rows;
        if (put(h, h->P.step, L.step_sz, L.nx + L.nu, xref, xref_rows * L.nx)) return MPCQP_ERR_HIP;
    }
    return flush_puts(h) ? MPCQP_ERR_HIP : 0;
}

static int share_factor_async(mpcqp_handle *h);
// setup's two launches (mpcqp_phases.h): equilibration, rho vector and cold start with a lean LDS block; then the first factorization
// keep: no cold start -- the iterate, the reported solution and the last mpcqp_info stay (mpcqp_update_model)
static int launch_setup(mpcqp_handle *h, bool keep = false) {
    const Lay &L = h->L;
    h->P.fown = nullptr;                            // (every instance factors into its own slot: sharing is off until mpcqp_share_factor is asked again)
    h->has_solve = false;                           // (a cold start or a new model: nothing to differentiate until the next solve, include/mpcqp_adjoint.h)
    h->tape_valid = false;                          // (the model blob and the scaling a rollout's tape was made under are about to be replaced, include/mpcqp_rollout.h)
    if (flush_puts(h)) return MPCQP_ERR_HIP;
    const size_t lean = sizeof(double) * (size_t)(smem_common_doubles(L) - L.tsz);      // (the work area T is carved last and not touched by k_setup)
    const size_t de = sizeof(double) * (size_t)(L.n + L.m);
    const int lds_de = lean + de <= 96 * 1024 ? 1 : 0;      // (cfg-5: 91 KB -- one workgroup per compute unit, still well ahead of two walking memory)
    if (set_smem(k_setup, lean + (lds_de ? de : 0))) return MPCQP_ERR_HIP;
    hipLaunchKernelGGL(k_setup, dim3(h->batch), dim3(NT), lean + (lds_de ? de : 0), h->stream, h->L, h->P, h->S, lds_de, keep ? 1 : 0);
    // the cyclic reduction's factorization at 256 threads uses the work area only as far as BcrFmt::lds_doubles says (three workgroups per compute unit at (12,4,30)
    // where the solve kernel's block -- iterate, top inverse -- would allow one); everything else factors in the block it solves in
    if (L.NB == 16 && L.bcr) {
        const size_t fac = lean + sizeof(double) * (size_t)BcrFmt::lds_doubles(NT / 64, L.m + L.n, L.bcrtop);
        if (set_smem(k_setup_factor_bcr, fac)) return MPCQP_ERR_HIP;
        hipLaunchKernelGGL(k_setup_factor_bcr, dim3(h->batch), dim3(NT), fac, h->stream, h->L, h->P);
    } else {
        DISPATCH_NB(L.NB, {
            if (set_smem(k_setup_factor<NB>, h->smem)) return MPCQP_ERR_HIP;
            hipLaunchKernelGGL(k_setup_factor<NB>, dim3(h->batch), dim3(NT), h->smem, h->stream, h->L, h->P);
        });
    }
    HIPCHK(hipGetLastError());
    // a batch of copies of ONE controller (the reference's one-model-many-states caller) is detected here: instances whose factorization inputs equal
    // instance 0's share one copy of its factor from the start (mpcqp_share_factor says what that means; one map kernel and a 0.5 MB copy per setup)
    if (h->batch > 1 && !(h->S.tuning & MPCQP_TUNE_NO_SHARE)) return share_factor_async(h);
    return MPCQP_OK;
}

extern "C" int mpcqp_setup(mpcqp_handle *h, const mpcqp_model *M, const double *x0, const double *um1, const double *xref, int xref_rows) {
    if (!h || !M || !x0 || !um1 || !xref) return fail(MPCQP_ERR_ARG, "mpcqp_setup: null argument");
    if (!M->Ad || !M->Bd || !M->Qx || !M->QxN || !M->Qu || !M->QDu || !M->xmin || !M->xmax || !M->umin || !M->umax ||
        !M->Dumin || !M->Dumax || !M->uref || !M->eps_feas) return fail(MPCQP_ERR_ARG, "mpcqp_setup: null model field");
    HIPCHK(hipSetDevice(h->device));
    const Lay &L = h->L; const int nx = L.nx, nu = L.nu, ms = L.model_sz;
    double *mb = h->P.model;
    int rc = 0;
    h->pack.n = 0;                                  // (nothing left over from a call that failed half-way)
    rc |= put(h, mb, ms, L.oAd, M->Ad, nx * nx); rc |= put(h, mb, ms, L.oBd, M->Bd, nx * nu);
    rc |= put(h, mb, ms, L.oxmin, M->xmin, nx); rc |= put(h, mb, ms, L.oxmax, M->xmax, nx);
    rc |= put(h, mb, ms, L.oumin, M->umin, nu); rc |= put(h, mb, ms, L.oumax, M->umax, nu);
    rc |= put(h, mb, ms, L.oDumin, M->Dumin, nu); rc |= put(h, mb, ms, L.oDumax, M->Dumax, nu);
    rc |= put(h, mb, ms, L.ouref, M->uref, nu); rc |= put(h, mb, ms, L.oeps, M->eps_feas, 1);
    rc |= put(h, mb, ms, L.oQx, M->Qx, nx * nx); rc |= put(h, mb, ms, L.oQxN, M->QxN, nx * nx);
    rc |= put(h, mb, ms, L.oQu, M->Qu, nu * nu); rc |= put(h, mb, ms, L.oQDu, M->QDu, nu * nu);
    if (rc) return MPCQP_ERR_HIP;
    h->L.d_rows = 0;                                // (no affine term until mpcqp_set_affine: include_ext4/mpcqp_affine.h)
    if ((rc = step_upload(h, x0, um1, xref, xref_rows))) return rc;
    if ((rc = launch_setup(h))) return rc;
    h->is_setup = true;
    return MPCQP_OK;
}

// ---- include/mpcqp_model.h: a new model under a handle that is in use
// The given fields into the model blob (device sources through put's pack list: one k_pack_rows launch for all of them).
static int merge_model(mpcqp_handle *h, const mpcqp_model *M) {
    const Lay &L = h->L; const int nx = L.nx, nu = L.nu, ms = L.model_sz;
    const struct { const double *src; int off, w; } f[14] = {
        {M->Ad, L.oAd, nx * nx}, {M->Bd, L.oBd, nx * nu}, {M->xmin, L.oxmin, nx}, {M->xmax, L.oxmax, nx}, {M->umin, L.oumin, nu}, {M->umax, L.oumax, nu},
        {M->Dumin, L.oDumin, nu}, {M->Dumax, L.oDumax, nu}, {M->uref, L.ouref, nu}, {M->eps_feas, L.oeps, 1},
        {M->Qx, L.oQx, nx * nx}, {M->QxN, L.oQxN, nx * nx}, {M->Qu, L.oQu, nu * nu}, {M->QDu, L.oQDu, nu * nu}};
    h->pack.n = 0;                                  // (nothing left over from a call that failed half-way)
    for (int i = 0; i < 14; ++i)
        if (f[i].src && put(h, h->P.model, ms, f[i].off, f[i].src, f[i].w)) return MPCQP_ERR_HIP;
    return MPCQP_OK;
}
static bool model_is_empty(const mpcqp_model *M) {
    return !M->Ad && !M->Bd && !M->Qx && !M->QxN && !M->Qu && !M->QDu && !M->xmin && !M->xmax && !M->umin && !M->umax && !M->Dumin && !M->Dumax && !M->uref && !M->eps_feas;
}
extern "C" int mpcqp_update_model(mpcqp_handle *h, const mpcqp_model *M) {
    if (!h || !M) return fail(MPCQP_ERR_ARG, "mpcqp_update_model: null argument");
    if (model_is_empty(M)) return fail(MPCQP_ERR_ARG, "mpcqp_update_model: no model field given");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_update_model before mpcqp_setup");
    HIPCHK(hipSetDevice(h->device));
    int rc = merge_model(h, M);
    if (rc) return rc;
    if ((rc = launch_setup(h, true))) return rc;   // (flushes the pack list first)
    h->warm_x_pending = true;                       // the next solve begins from z = A_new x
    return MPCQP_OK;
}

extern "C" int mpcqp_update(mpcqp_handle *h, const double *x0, const double *um1, const double *xref, int xref_rows) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_update before mpcqp_setup");
    if (h->step_blank && (!x0 || !um1 || !xref)) return fail(MPCQP_ERR_STATE, "mpcqp_update: the handle was set up from raw q, l, u and holds no x0 / u_{-1} / xref yet: give all three");
    HIPCHK(hipSetDevice(h->device));
    h->step_blank = false;
    h->L.raw = 0;                                   // q, l, u are rebuilt from (x0, u_{-1}, xref) again
    h->pack.n = 0;
    return step_upload(h, x0, um1, xref, xref_rows);
}

// The caller's q, l, u reach the decode kernel in place if they are device memory, else through the handle's staging block
// (allocated once; copies and kernel are stream-ordered, so the next call may reuse it without waiting).
static int upload_vectors(mpcqp_handle *h, const double *q, const double *l, const double *u) {
    const Lay &L = h->L; const size_t B = (size_t)h->batch;
    const double *src[3] = {q, l, u}; const size_t cnt[3] = {B * L.n, B * L.m, B * L.m};
    const double *dev[3] = {nullptr, nullptr, nullptr};
    size_t off = 0;
    for (int i = 0; i < 3; ++i) {
        if (src[i] && !is_device_ptr(src[i])) {
            if (!h->vec_buf) HIPCHK(hipMalloc((void **)&h->vec_buf, sizeof(double) * B * (L.n + 2 * (size_t)L.m)));
            HIPCHK(hipMemcpyAsync(h->vec_buf + off, src[i], cnt[i] * sizeof(double), hipMemcpyHostToDevice, h->stream));
            dev[i] = h->vec_buf + off;
        } else dev[i] = src[i];
        off += cnt[i];
    }
    hipLaunchKernelGGL(k_decode_vectors, dim3(h->batch), dim3(64), 0, h->stream, h->L, h->P, dev[0], dev[1], dev[2], h->batch);
    HIPCHK(hipGetLastError());
    return MPCQP_OK;
}

extern "C" int mpcqp_update_vectors(mpcqp_handle *h, const double *q, const double *l, const double *u) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_update_vectors before setup");
    if ((l == nullptr) != (u == nullptr)) return fail(MPCQP_ERR_ARG, "mpcqp_update_vectors: give l and u together (the equality rows l[:nx] == u[:nx] carry x0)");
    HIPCHK(hipSetDevice(h->device));
    h->has_solve = false;                           // (as in step_upload)
    if (l) h->L.d_rows = 0;                         // (the caller's l, u replace the bounds, an affine term with them: include_ext4/mpcqp_affine.h)
    if (l) h->tape_valid = false;                   // (k_decode_vectors writes the boxes of l, u into the model blob, which a rollout's reverse sweep reads from the handle)
    if (!h->L.raw) {
        // entering raw mode: the vectors that are NOT given now must keep describing the current problem, so the
        // tables behind them are materialised once from the controller data (q from (xref, uref, u_{-1}); du0 from u_{-1})
        if (!q || !l || !u) {
            DISPATCH_NB(h->L.NB, {
                if (set_smem(k_export<NB>, h->smem)) return MPCQP_ERR_HIP;
                hipLaunchKernelGGL(k_export<NB>, dim3(h->batch), dim3(NT), h->smem, h->stream, h->L, h->P, (double *)nullptr, (double *)nullptr, (double *)nullptr, (double *)nullptr, (double *)nullptr);
            });
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_keep_du0, dim3((h->batch * h->L.nu + 255) / 256), dim3(256), 0, h->stream, h->L, h->P, h->batch);
            HIPCHK(hipGetLastError());
        }
        h->L.raw = 1;
    }
    return upload_vectors(h, q, l, u);
}

extern "C" int mpcqp_setup_qp(mpcqp_handle *h, const mpcqp_model *M, const double *q, const double *l, const double *u) {
    if (!h || !M || !q || !l || !u) return fail(MPCQP_ERR_ARG, "mpcqp_setup_qp: null argument");
    if (!M->Ad || !M->Bd || !M->Qx || !M->QxN || !M->Qu || !M->QDu || !M->eps_feas) return fail(MPCQP_ERR_ARG, "mpcqp_setup_qp: null model field");
    HIPCHK(hipSetDevice(h->device));
    const Lay &L = h->L; const int nx = L.nx, nu = L.nu, ms = L.model_sz;
    double *mb = h->P.model;
    int rc = 0;
    h->pack.n = 0;                                  // (nothing left over from a call that failed half-way)
    rc |= put(h, mb, ms, L.oAd, M->Ad, nx * nx); rc |= put(h, mb, ms, L.oBd, M->Bd, nx * nu);
    rc |= put(h, mb, ms, L.oeps, M->eps_feas, 1);
    if (M->uref) rc |= put(h, mb, ms, L.ouref, M->uref, nu);          // (only output()'s u_failure reads it; zeros otherwise)
    rc |= put(h, mb, ms, L.oQx, M->Qx, nx * nx); rc |= put(h, mb, ms, L.oQxN, M->QxN, nx * nx);
    rc |= put(h, mb, ms, L.oQu, M->Qu, nu * nu); rc |= put(h, mb, ms, L.oQDu, M->QDu, nu * nu);
    if (rc) return MPCQP_ERR_HIP;
    h->L.raw = 1; h->step_blank = true; h->L.d_rows = 0;
    if ((rc = upload_vectors(h, q, l, u))) return rc;
    if ((rc = launch_setup(h))) return rc;
    h->is_setup = true;
    return MPCQP_OK;
}

// ---- the seam with the caller's matrices (mpc.py:266), see mpcqp_csc.h
extern "C" int mpcqp_create_csc(mpcqp_handle **out, int device, int batch, int n, int m, const int64_t *P_colptr, const int32_t *P_rowidx,
                                const int64_t *A_colptr, const int32_t *A_rowidx, int nx_hint, int nu_hint, const mpcqp_settings *s) {
    if (!out || !P_colptr || !P_rowidx || !A_colptr || !A_rowidx || n < 1 || m < 1) return fail(MPCQP_ERR_ARG, "mpcqp_create_csc: null argument");
    CscSeam *seam = new CscSeam();
    CscPattern &c = seam->pat;
    c.n = n; c.m = m;
    c.Pp.assign(P_colptr, P_colptr + n + 1); c.Ap.assign(A_colptr, A_colptr + n + 1);
    bool cp_ok = c.Pp[0] == 0 && c.Ap[0] == 0;
    for (int j = 0; j < n && cp_ok; ++j) cp_ok = c.Pp[j] <= c.Pp[j + 1] && c.Ap[j] <= c.Ap[j + 1];      // non-decreasing from 0: every entry is within [0, colptr[n]]
    if (!cp_ok) { delete seam; return fail(MPCQP_ERR_ARG, "mpcqp_create_csc: bad column pointers (must start at 0 and be non-decreasing)"); }
    c.Pi.assign(P_rowidx, P_rowidx + c.Pp[n]); c.Ai.assign(A_rowidx, A_rowidx + c.Ap[n]);
    for (int32_t r : c.Pi) if (r < 0 || r >= n) { delete seam; return fail(MPCQP_ERR_ARG, "mpcqp_create_csc: P row index out of range"); }
    for (int32_t r : c.Ai) if (r < 0 || r >= m) { delete seam; return fail(MPCQP_ERR_ARG, "mpcqp_create_csc: A row index out of range"); }
    int nx, nu, Np, Nc, soft; std::string why;
    if (csc_dims(c, nx_hint, nu_hint, &nx, &nu, &Np, &Nc, &soft, &why)) { delete seam; return fail(MPCQP_ERR_UNSUPPORTED, "mpcqp_create_csc: not an MPC QP of pyMPC: " + why); }
    mpcqp_settings st; if (s) st = *s; else mpcqp_default_settings(&st);
    st.soft_constraints = soft;                     // (slack columns or not: read off the pattern by csc_dims)
    const int rc = mpcqp_create(out, device, batch, nx, nu, Np, Nc, &st);
    if (rc) { delete seam; return rc; }
    (*out)->csc = seam;
    return MPCQP_OK;
}

extern "C" int mpcqp_setup_csc(mpcqp_handle *h, const double *P_val, const double *A_val, const double *q, const double *l, const double *u) {
    if (!h || !P_val || !A_val || !q || !l || !u) return fail(MPCQP_ERR_ARG, "mpcqp_setup_csc: null argument");
    if (!h->csc) return fail(MPCQP_ERR_STATE, "mpcqp_setup_csc: the handle was not made by mpcqp_create_csc");
    const CscPattern &c = h->csc->pat; const Lay &L = h->L;
    const size_t B = (size_t)h->batch, nnzP = (size_t)c.Pp[c.n], nnzA = (size_t)c.Ap[c.n];
    const int nx = L.nx, nu = L.nu;
    std::vector<double> Ad(B * nx * nx), Bd(B * nx * nu), Qx(B * nx * nx), QxN(B * nx * nx), Qu(B * nu * nu), QDu(B * nu * nu), ef(B), lc(B * c.m), uc(B * c.m);
    for (size_t b = 0; b < B; ++b) {
        MpcBlocks blk; std::string why;
        if (csc_recover(c, nx, nu, L.Np, L.Nc, L.soft, P_val + b * nnzP, A_val + b * nnzA, q + b * c.n, l + b * c.m, u + b * c.m, &blk, &why))
            return fail(MPCQP_ERR_UNSUPPORTED, "mpcqp_setup_csc: instance " + std::to_string(b) + ": " + why);
        std::copy(blk.Ad.begin(), blk.Ad.end(), Ad.begin() + b * nx * nx); std::copy(blk.Bd.begin(), blk.Bd.end(), Bd.begin() + b * nx * nu);
        std::copy(blk.Qx.begin(), blk.Qx.end(), Qx.begin() + b * nx * nx); std::copy(blk.QxN.begin(), blk.QxN.end(), QxN.begin() + b * nx * nx);
        std::copy(blk.Qu.begin(), blk.Qu.end(), Qu.begin() + b * nu * nu); std::copy(blk.QDu.begin(), blk.QDu.end(), QDu.begin() + b * nu * nu);
        ef[b] = blk.eps_feas;
    }
    for (size_t i = 0; i < B * c.m; ++i) { lc[i] = std::min(std::max(l[i], -QP_INFTY), QP_INFTY); uc[i] = std::min(std::max(u[i], -QP_INFTY), QP_INFTY); }      // (osqp's wrapper clips to +-1e30)
    mpcqp_model M; memset(&M, 0, sizeof(M));
    M.Ad = Ad.data(); M.Bd = Bd.data(); M.Qx = Qx.data(); M.QxN = QxN.data(); M.Qu = Qu.data(); M.QDu = QDu.data(); M.eps_feas = ef.data();
    const int rc = mpcqp_setup_qp(h, &M, q, lc.data(), uc.data());
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));        // (the host staging vectors above die with this call)
    return MPCQP_OK;
}

extern "C" int mpcqp_update_settings(mpcqp_handle *h, const mpcqp_settings *s) {
    if (!h || !s) return fail(MPCQP_ERR_ARG, "null argument");
    double rho = h->S.rho, sigma = h->S.sigma; int scaling = h->S.scaling, backend = h->S.backend, tuning = h->S.tuning;
    h->S = *s;
    h->S.rho = rho; h->S.sigma = sigma; h->S.scaling = scaling;   // fixed at setup (they shape the factorization)
    h->S.soft_constraints = h->L.soft;                            // fixed at creation (it shapes the problem)
    h->S.backend = backend; h->S.tuning = tuning;                 // ... as are the backend and its tuning flags
    return MPCQP_OK;
}

// The kernel arguments of a launch and its grid: one workgroup per instance, or -- batches beyond the resident workgroup slots -- the PERSISTENT form:
// as many workgroups as there are slots, each taking instances off a queue (k_mpc_run in mpcqp_kernels.h says what that buys).
// nsteps: closed-loop steps of the launch (0: a solve).
// Fewer slots than fit for the bandwidth kernel of 32 x 32 stages with its iterate in memory (BASELINE configs[4]) where a closed-loop launch would otherwise hold
// (nearly) every instance resident at once: such a launch ends with its slowest instance, which -- sharing the memory system with 511 others -- runs at 104 us per
// iteration where it could run at 75.  Three quarters of the slots and a queue of (instance, step range) items, longest expected work first: the stragglers start
// first and run faster all along, the memory system stays saturated.  Measured (50-step launches, k solves/s, 4 / 5 / 6 / 7 / 8 quarters of a workgroup per unit):
// 512 instances 121 / 138 / 148-150 / 141-144 / 137-138; 768 instances - / - / 153 / - / 145; 1024 instances 119 / - / 153 / 166 / 177 (two full rounds: all slots).
static int run_grid(const mpcqp_handle *h, int nsteps) {
    const Lay &L = h->L;
    const int occ = plan_occupancy(*h);
    const int full = h->ncu * occ;
    const int q = (h->S.tuning >> MPCQP_TUNE_SLOTS_SHIFT) & 0x1F;      // (development: resident workgroups in eighths of a workgroup per compute unit)
    if (q) return std::max(1, std::min(full, h->ncu * q / 8));
    if (L.NB == 32 && occ == 2 && !h->lds_state && !L.lstage && nsteps >= 8 && 2 * h->batch <= 3 * full && 4 * h->batch > 3 * full && !(h->S.tuning & MPCQP_TUNE_NO_QUEUE)) return 3 * full / 4;
    return full;
}
static RunKArgs run_kernel_args(mpcqp_handle *h, const RunArgs &R0, int *grid) {
    RunKArgs A; A.L = h->L; A.P = h->P; A.S = h->S; A.R = R0;
    *grid = h->batch;
    const int slots = run_grid(h, R0.nsteps);
    if (h->ncu > 0 && h->batch > slots && h->vcur_dev && !R0.pin_in && !R0.pub && (R0.nsteps > 0 || (h->S.tuning & (MPCQP_TUNE_QUEUE_SOLVES | MPCQP_TUNE_ONE_LAUNCH_SOLVES))) && !(h->S.tuning & MPCQP_TUNE_NO_QUEUE)) {
        A.R.vcur = h->vcur_dev; A.R.vperm = ((R0.nsteps > 0 || (R0.part == 0 && (h->S.tuning & MPCQP_TUNE_ONE_LAUNCH_SOLVES))) && h->qperm_set) ? h->qperm_dev : h->P.perm;      /* (a solve's second launch walks the pending list: P.perm) */ A.R.vqueue = h->vqueue_dev;
        A.P.perm = h->vcur_dev;
        *grid = slots;
        // closed loop: an instance's steps in parts, about QUEUE_ITEMS_PER_SLOT items per slot in all (a launch ends within half an item of its ideal
        // length; an item costs a kernel prologue, ~ 10 us)
        if (R0.nsteps > 1 && !(h->S.tuning & MPCQP_TUNE_NO_PARTS)) {
            const int ov = (h->S.tuning >> MPCQP_TUNE_ITEMS_SHIFT) & 0x7F;      // (bits 16..22: development override)
            const int per_slot = ov ? ov : QUEUE_ITEMS_PER_SLOT;
            const int parts = std::min(R0.nsteps, (per_slot * slots + h->batch - 1) / h->batch);
            if (parts > 1) {
                // part lengths fall off towards the end of the loop (each takes about 2 / (parts left + 1) of what is left: 20 steps in 4 parts = 8, 6, 4, 2): the
                // launch's end is as fine-grained as many small parts would make it, for the prologues of few
                const int np = std::min(parts, 16);
                int off = 0;
                for (int p = 0; p < np; ++p) {
                    A.R.voff[p] = off;
                    const int left = R0.nsteps - off, pl = np - p;
                    const int len = pl == 1 ? left : std::max(1, std::min(left - (pl - 1), (2 * left + pl) / (pl + 1)));
                    off += len;
                }
                A.R.voff[np] = R0.nsteps; A.R.vparts = np; A.R.vdone = h->vdone_dev;
            }
        }
    }
    if (R0.nsteps > 0) h->loop_parts = A.R.vcur ? std::max(1, A.R.vparts) : 0;
    return A;
}
template <int NB, bool LDSS, int NXT, int NUT, int MODE>
static int launch_run_t(mpcqp_handle *h, const RunKArgs &A, int grid) {
    auto kernel = A.R.nsteps > 0 ? k_mpc_run<NB, LDSS, NXT, NUT, MODE, true> : k_mpc_run<NB, LDSS, NXT, NUT, MODE, false>;
    if (set_smem(kernel, h->smem)) return MPCQP_ERR_HIP;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), h->smem, h->stream, A);
    return 0;
}

// Load balancing across CUs.  All workgroups of a launch are resident at once (a few per CU) and an instance keeps its
// character -- one that needs two ADMM rounds per solve mostly keeps needing them -- so CUs that happen to host several
// slow instances finish last and set the launch time.  Every now and then the per-instance iteration counts are read
// back, smoothed, and the workgroup -> instance map is rebuilt: instances sorted by expected work, dealt to the CUs in
// snake order (blocks b, b + #CU, b + 2 #CU, ... share a CU: dispatch is round-robin over XCDs and CUs), so that every CU
// gets a similar total.  Pure scheduling: which workgroup handles which instance never changes a result.
// Must be called with the stream idle.
static bool balance_due(const mpcqp_handle *h) {
    if (!h->auto_balance || h->ncu <= 0 || h->batch <= h->ncu) return false;      // (nothing to balance: no call waits for the stream on this account)
    return h->solves_since_balance >= (h->work_ema.empty() ? BALANCE_FIRST : BALANCE_EVERY);
}
static int rebalance(mpcqp_handle *h) {
    const int B = h->batch, ncu = h->ncu;
    h->solves_since_balance = 0;
    if (!h->auto_balance || ncu <= 0 || B <= ncu) return MPCQP_OK;
    std::vector<unsigned> work(B);
    HIPCHK(hipMemcpyAsync(work.data(), h->P.work, sizeof(unsigned) * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemsetAsync(h->P.work, 0, sizeof(unsigned) * (size_t)B, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));       // (the handle's own stream only: no implicit device-wide sync)
    if (h->work_ema.empty()) h->work_ema.assign(B, 0.0);
    bool any = false;
    const double decay = 0.75;                             // (anything from 0.5 to 0.95 measured the same)
    for (int i = 0; i < B; ++i) { h->work_ema[i] = decay * h->work_ema[i] + (double)work[i]; any |= work[i] != 0; }
    if (!any) return MPCQP_OK;
    std::vector<int> order(B), perm(B);
    for (int i = 0; i < B; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return h->work_ema[a] > h->work_ema[b]; });
    // One workgroup per compute unit at a time (the latency kernels, wide stages): workgroups start in index order as compute units come
    // free, so the map is the longest-expected-work-first list -- the classic greedy schedule, makespan within one instance of the mean.
    const int occ = kernel_occupancy(h->kernel);      // (by __launch_bounds__, whatever the LDS block leaves room for)
    const bool one_at_a_time = occ == 1;
    const int full_rows = B / ncu;
    for (int j = 0; j < B; ++j) {
        const int row = j / ncu, pos = j % ncu;
        const bool reversed = !one_at_a_time && (row & 1) && row < full_rows;      // a partial last row keeps forward order
        perm[row * ncu + (reversed ? ncu - 1 - pos : pos)] = order[j];
    }
    // (the closed loop's persistent launches take instances off a QUEUE: for them the longest-expected-work-first list itself, whatever the kernel)
    HIPCHK(hipMemcpyAsync(h->qperm_dev, order.data(), sizeof(int) * (size_t)B, hipMemcpyHostToDevice, h->stream));
    h->qperm_set = true;
    // Pacing (development switch, off unless mpcqp_settings.tuning bits 8..15 ask for it): in the bandwidth kernels with a global-memory iterate whose
    // instances are ALL resident at once (B <= slots) the launch ends with its slowest instance.  Every instance that is NOT expected to need more than
    // 1.15 x the median's iterations idles `units` x 3.5 us in each of its iterations, leaving its share of the memory system to the stragglers.
    {
        const int units = std::min((h->S.tuning >> 8) & 0xFF, 64);
        if (units && !one_at_a_time && !h->lds_state && !h->L.lstage && B <= occ * ncu) {
            const double wmed = h->work_ema[order[B / 2]];
            for (int j = 0; j < B; ++j) {
                const int inst = perm[j] & PERM_INST_MASK;
                perm[j] = inst | ((h->work_ema[inst] > 1.15 * wmed ? 0 : units) << PERM_PACE_SHIFT);
            }
        }
    }
    HIPCHK(hipMemcpyAsync(h->perm_dev, perm.data(), sizeof(int) * (size_t)B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                          // (perm is a stack-lifetime host buffer)
    h->P.perm = h->perm_dev;
    return MPCQP_OK;
}

// One launch of the solve / closed-loop kernel on the handle's stream (asynchronous).  Specialisations with
// compile-time nx, nu for the BASELINE configurations; generic kernels otherwise.
static int launch_run(mpcqp_handle *h, RunArgs R, int plain_iters) {
    const Lay &L = h->L; const mpcqp_settings &S = h->S;
    R.plain = plain_iters > 0;
    R.warm_x = (h->warm_x_pending && R.part != 2 && R.part != 3) ? 1 : 0;
    if (R.part != 3) { h->has_solve = true; h->um1_moved = false; }
    if (R.part == 0 || R.part == 2) h->warm_x_pending = false;      // (a two-launch solve begins in its first launch only; mpcqp_refactor, part 3, is not a solve)
    R.max_iter = R.plain ? plain_iters : S.max_iter;
    R.chk = R.plain ? 0 : S.check_termination;
    R.rho_every = (!R.plain && S.adaptive_rho) ? (S.adaptive_rho_interval ? S.adaptive_rho_interval : (R.chk ? 4 * R.chk : 100)) : 0;
    R.batch = h->batch;
    h->solves_since_balance = std::min(h->solves_since_balance + (R.nsteps > 0 ? R.nsteps : 1), 1 << 20);
    const int e = h->ev_count % MAXEV;
    if (h->profiling) {
        if (h->ev_count >= MAXEV) {                 // ring full: bank the oldest pair first
            float ms = 0.f; HIPCHK(hipEventSynchronize(h->ev1[e])); HIPCHK(hipEventElapsedTime(&ms, h->ev0[e], h->ev1[e]));
            h->run_ms += ms; h->run_launches += 1;
        }
        HIPCHK(hipEventRecord(h->ev0[e], h->stream));
    }
    int grid, rc = MPCQP_ERR_STATE;
    const RunKArgs A = run_kernel_args(h, R, &grid);
    if (A.R.vdone) HIPCHK(hipMemsetAsync(h->vdone_dev, 0, sizeof(int) * (size_t)h->batch, h->stream));
    const RunKernelId &id = h->kernel;
    if (id.w8) {                                    // 512-thread workgroups: the other translation unit
        if (mpcqp_w8_launch(&A, sizeof(A), id, R.nsteps > 0, grid, h->smem, h->stream)) return fail(MPCQP_ERR_HIP, "mpcqp_w8_launch failed");
        rc = 0;
    }
#define X(NB, LDSS, NXT, NUT, MODE) else if (same_kernel(id, RunKernelId{NB, LDSS, NXT, NUT, MODE, false})) rc = launch_run_t<NB, LDSS, NXT, NUT, MODE>(h, A, grid);
    MPCQP_RUN_KERNELS_256(X)
#undef X
    if (rc == MPCQP_ERR_STATE) return fail(rc, "launch_run: the planned solve kernel is not in the table");
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    if (h->profiling) { HIPCHK(hipEventRecord(h->ev1[e], h->stream)); h->ev_count += 1; }
    return MPCQP_OK;
}

// Collect the pending event pairs (synchronises on them).
static int drain_events(mpcqp_handle *h) {
    const int pending = h->ev_count < MAXEV ? h->ev_count : MAXEV;
    for (int i = 0; i < pending; ++i) {
        const int e = (h->ev_count - pending + i) % MAXEV;
        float ms = 0.f; HIPCHK(hipEventSynchronize(h->ev1[e])); HIPCHK(hipEventElapsedTime(&ms, h->ev0[e], h->ev1[e]));
        h->run_ms += ms; h->run_launches += 1;
    }
    h->ev_count = 0;
    return MPCQP_OK;
}

// One solve of every instance.  Batches larger than the number of CUs are solved in two launches: begin + first ADMM
// round + check for everybody, then the instances that are not finished (typically 40 %) are continued by a second launch
// whose workgroup -> instance map is the list the first one compiled -- the dispatcher spreads them evenly over the CUs,
// whereas staying put would leave some CUs with four running workgroups and others with none (the launch would last as
// long as two fully contended rounds).  Both launches are asynchronous; no host round trip in between.
static int launch_solve(mpcqp_handle *h, int plain_iters) {
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "solve before mpcqp_setup");
    HIPCHK(hipSetDevice(h->device));
    RunArgs R; memset(&R, 0, sizeof(R));
    const bool split = plain_iters == 0 && h->auto_balance && h->ncu > 0 && h->batch > h->ncu && !(h->S.tuning & MPCQP_TUNE_ONE_LAUNCH_SOLVES);
    if (!split) return launch_run(h, R, plain_iters);
    R.pending = h->pending_dev; R.npending = h->npending_dev;
    HIPCHK(hipMemsetAsync(h->npending_dev, 0, sizeof(int), h->stream));
    R.part = 1;
    int rc = launch_run(h, R, 0);
    if (rc) return rc;
    R.part = 2;
    const int *perm = h->P.perm;
    h->P.perm = h->pending_dev;                     // the follow-up launch walks the pending list
    h->solves_since_balance -= 1;                   // (one solve, two launches)
    rc = launch_run(h, R, 0);
    h->P.perm = perm;
    return rc;
}

// ---- solution polishing (include/mpcqp_polish.h, mpcqp_polish.h) --------------------------------------------------------------
extern "C" void mpcqp_polish_default_settings(mpcqp_polish_settings *s) {
    if (!s) return;
    memset(s, 0, sizeof(*s));
    s->struct_size = (int32_t)sizeof(mpcqp_polish_settings); s->polish = 0; s->delta = 1e-6; s->polish_refine_iter = 3;
}
extern "C" int mpcqp_set_polish(mpcqp_handle *h, const mpcqp_polish_settings *s) {
    if (!h || !s) return fail(MPCQP_ERR_ARG, "null argument");
    if (s->struct_size != (int32_t)sizeof(mpcqp_polish_settings)) return fail(MPCQP_ERR_ARG, "mpcqp_set_polish: struct_size is not sizeof(mpcqp_polish_settings) (take the struct from mpcqp_polish_default_settings)");
    if ((s->polish != 0 && s->polish != 1) || !(s->delta > 0.0) || !(s->delta < 1e30) || s->polish_refine_iter < 0)
        return fail(MPCQP_ERR_ARG, "mpcqp_set_polish: polish must be 0 or 1, delta > 0, polish_refine_iter >= 0");
    h->pol = *s;
    return MPCQP_OK;
}
// What a K_pol kernel (k_polish, k_adjoint) is launched with: the layout of mpcqp_kpol.h (taken from the handle's Lay at every launch:
// it changes with raw-vector mode and the reference shape), workgroup b = instance b, a factor of the kernel's own, and the LDS of that layout.
struct KpolLaunch { Lay G; Ptrs P; size_t smem; };
static KpolLaunch kpol_launch(const mpcqp_handle *h) {
    KpolLaunch v{polish_layout(h->L), h->P, 0};
    v.P.perm = nullptr; v.P.fown = nullptr;
    v.smem = sizeof(double) * (size_t)smem_common_doubles(v.G);
    return v;
}
// The buffers of K_pol: the factor in the generic block format, the metric, the active set, the border and workspace of the factorization.
static int kpol_alloc(mpcqp_handle *h, KpolBufs *K, const char *what) {
    const KpolLaunch v = kpol_launch(h);
    const Lay &G = v.G;
    if (v.smem > 160 * 1024) return fail(MPCQP_ERR_UNSUPPORTED, std::string(what) + ": problem too large for one workgroup's LDS");
    const size_t B = (size_t)h->batch;
    K->fsz = polish_factor_doubles(G);
    int rc = 0;
    rc |= dalloc(h, &K->F, B * (size_t)K->fsz);
    rc |= dalloc(h, &K->om, B * G.m); rc |= dalloc(h, &K->s, B * G.n); rc |= dalloc(h, &K->act, B * G.m);
    if (G.border) { rc |= dalloc(h, &K->Bb, B * (size_t)G.nu * G.N * G.NB); rc |= dalloc(h, &K->Zb, B * (size_t)G.nu * G.N * G.NB); rc |= dalloc(h, &K->Sig, B * (size_t)G.nu * G.nu); }
    if (G.NB == 128) rc |= dalloc(h, &K->gws, B * (size_t)HugeFmt::GWS);
    return rc ? MPCQP_ERR_HIP : MPCQP_OK;      // (what was allocated stays in h->allocs: freed by mpcqp_destroy)
}
// The polish's buffers, on first use: K_pol, the polished point, the sweep vectors, the targets of the active rows, status_polish.
static int polish_alloc(mpcqp_handle *h) {
    if (h->pq.status) return MPCQP_OK;
    PolishArgs Q; memset(&Q, 0, sizeof(Q));
    int rc = kpol_alloc(h, &Q.K, "mpcqp_polish");
    if (rc) return rc;
    const Lay &L = h->L; const size_t B = (size_t)h->batch;
    rc |= dalloc(h, &Q.x, B * L.n); rc |= dalloc(h, &Q.z, B * L.m); rc |= dalloc(h, &Q.y, B * L.m);
    rc |= dalloc(h, &Q.r, B * L.n); rc |= dalloc(h, &Q.d, B * L.n); rc |= dalloc(h, &Q.e, B * L.n); rc |= dalloc(h, &Q.dd, B * L.n);
    rc |= dalloc(h, &Q.bt, B * L.m);
    int *status = nullptr;
    rc |= dalloc(h, &status, B);
    if (rc) return MPCQP_ERR_HIP;
    Q.status = status; Q.batch = h->batch;
    h->pq = Q;
    return MPCQP_OK;
}
// Polish the last solve of every instance (k_polish; pub: mpcqp_step_host's mapped result block and flag, else null).
static int launch_polish(mpcqp_handle *h, double *pub = nullptr, unsigned *done = nullptr, unsigned long long seq = 0) {
    int rc = polish_alloc(h);
    if (rc) return rc;
    if (flush_puts(h)) return MPCQP_ERR_HIP;
    PolishArgs Q = h->pq;
    Q.delta = h->pol.delta; Q.refine = h->pol.polish_refine_iter; Q.pub = pub; Q.done = done; Q.seq = seq;
    const KpolLaunch v = kpol_launch(h);
    DISPATCH_NB(v.G.NB, {
        if (set_smem(k_polish<NB>, v.smem)) return MPCQP_ERR_HIP;
        hipLaunchKernelGGL(k_polish<NB>, dim3(h->batch), dim3(NT), v.smem, h->stream, v.G, v.P, Q);
    });
    HIPCHK(hipGetLastError());
    return MPCQP_OK;
}
// After a solve: polish it (polish on), or record 'not performed' where an earlier solve left a status_polish behind.
static int after_solve(mpcqp_handle *h) {
    if (h->pol.polish) return launch_polish(h);
    if (h->pq.status) HIPCHK(hipMemsetAsync(h->pq.status, 0, sizeof(int) * (size_t)h->batch, h->stream));
    return MPCQP_OK;
}
extern "C" int mpcqp_polish(mpcqp_handle *h) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_polish before mpcqp_setup");
    HIPCHK(hipSetDevice(h->device));
    return launch_polish(h);
}
extern "C" int mpcqp_get_polish_info(mpcqp_handle *h, int32_t *status_polish) {
    if (!h || !status_polish) return fail(MPCQP_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    if (!h->pq.status) { HIPCHK(hipStreamSynchronize(h->stream)); memset(status_polish, 0, sizeof(int32_t) * (size_t)h->batch); return MPCQP_OK; }
    HIPCHK(hipMemcpyAsync(status_polish, h->pq.status, sizeof(int32_t) * (size_t)h->batch, hipMemcpyDefault, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

extern "C" int mpcqp_solve(mpcqp_handle *h) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    const int rc = launch_solve(h, 0);
    return rc ? rc : after_solve(h);
}
extern "C" int mpcqp_refactor(mpcqp_handle *h) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_refactor before mpcqp_setup");
    HIPCHK(hipSetDevice(h->device));
    RunArgs R; memset(&R, 0, sizeof(R));
    R.part = 3;
    const int since = h->solves_since_balance;
    const bool prof = h->profiling;
    h->profiling = false;                           // (not a solve: keep it out of the k_mpc_run timing and the balancing clock)
    const int rc = launch_run(h, R, 0);
    h->profiling = prof; h->solves_since_balance = since;
    return rc;
}
// One model, many states (test_scripts/example_mpc_function.py:105-111): instances whose factorization inputs are bit-identical to instance 0's solve with ONE
// copy of its factor -- a streamed factor then comes out of L2 instead of HBM.  k_share_map decides per instance; results cannot change: the factorization is a
// deterministic function of (model, rho vector, scaling, cost scale), and an instance that refactors (rho update, changed constraint types) leaves the shared
// slot for its own before it writes.
__global__ __launch_bounds__(NT) void k_share_map(Lay L, Ptrs P, int *fown, unsigned *nshared, int batch) {
    const int b = blockIdx.x, tid = threadIdx.x;
    typedef const unsigned long long cu64;
    int diff = 0;
    auto cmp = [&](const double *base, size_t len) {
        cu64 *a = (cu64 *)(base + (size_t)b * len), *r = (cu64 *)base;
        for (size_t i = tid; i < len; i += NT) diff |= a[i] != r[i];
    };
    cmp(P.model, L.model_sz); cmp(P.omega, L.m); cmp(P.s, L.n); cmp(P.c, 1);
    if (P.info[b].status == MPCQP_NON_CVX && P.info[b].iter == 0) diff = 1;      // (a factorization k_setup reported bad stays where it is)
    diff = __syncthreads_or(diff);
    if (tid == 0) { fown[b] = diff ? b : batch; if (!diff) atomicAdd(nshared, 1u); }
}
static int share_factor_async(mpcqp_handle *h) {
    h->P.fown = nullptr;
    // the register-resident backends read their factor once per launch (nothing to gain); the shared slot holds instance 0's factor as of NOW
    if (h->L.dense || h->L.bcr) return MPCQP_OK;
    if (flush_puts(h)) return MPCQP_ERR_HIP;
    HIPCHK(hipMemcpyAsync(h->P.F + (size_t)h->batch * h->P.fsz, h->P.F, sizeof(double) * (size_t)h->P.fsz, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->nshared_dev, 0, sizeof(unsigned), h->stream));
    hipLaunchKernelGGL(k_share_map, dim3(h->batch), dim3(NT), 0, h->stream, h->L, h->P, h->fown_dev, h->nshared_dev, h->batch);
    HIPCHK(hipGetLastError());
    h->P.fown = h->fown_dev;
    return MPCQP_OK;
}
extern "C" int mpcqp_share_factor(mpcqp_handle *h, int *nshared) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_share_factor before mpcqp_setup");
    HIPCHK(hipSetDevice(h->device));
    if (nshared) *nshared = 0;
    const int rc = share_factor_async(h);
    if (rc) return rc;
    if (nshared && h->P.fown) {
        unsigned n = 0;
        HIPCHK(hipMemcpyAsync(&n, h->nshared_dev, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        *nshared = (int)n;
    }
    return MPCQP_OK;
}
extern "C" int mpcqp_iterate(mpcqp_handle *h, int iters) {
    if (!h || iters < 1) return fail(MPCQP_ERR_ARG, "mpcqp_iterate: bad argument");
    return launch_solve(h, iters);
}

static int get(mpcqp_handle *h, void *dst, const void *src, size_t bytes) {
    if (!dst) return 0;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, h->stream));
    return 0;
}

// ---- adjoint derivatives (include/mpcqp_adjoint.h, mpcqp_adjoint.h) ------------------------------------------------------------
extern "C" void mpcqp_adjoint_default_settings(mpcqp_adjoint_settings *s) {
    if (!s) return;
    memset(s, 0, sizeof(*s));
    s->struct_size = (int32_t)sizeof(mpcqp_adjoint_settings); s->refine_iter = 3; s->delta = 1e-6; s->weak_tol = 1e-6; s->extra_iter = 60;
}
extern "C" int mpcqp_set_adjoint(mpcqp_handle *h, const mpcqp_adjoint_settings *s) {
    if (!h || !s) return fail(MPCQP_ERR_ARG, "null argument");
    if (s->struct_size != (int32_t)sizeof(mpcqp_adjoint_settings)) return fail(MPCQP_ERR_ARG, "mpcqp_set_adjoint: struct_size is not sizeof(mpcqp_adjoint_settings) (take the struct from mpcqp_adjoint_default_settings)");
    if (!(s->delta > 0.0) || !(s->delta < 1e30) || s->refine_iter < 0 || !(s->weak_tol >= 0.0) || s->extra_iter < 0)
        return fail(MPCQP_ERR_ARG, "mpcqp_set_adjoint: delta > 0, refine_iter >= 0, weak_tol >= 0, extra_iter >= 0");
    h->adj = *s;
    return MPCQP_OK;
}
// The adjoint's buffers, on first use: K_pol, r_w / r_y and the sweep vectors, the seed, the staged seeds, the outputs for up to nu seeds,
// the three info vectors.
static int adjoint_alloc(mpcqp_handle *h) {
    if (h->aq.status) return MPCQP_OK;
    AdjointArgs Q; memset(&Q, 0, sizeof(Q));
    int rc = kpol_alloc(h, &Q.K, "mpcqp_adjoint");
    if (rc) return rc;
    const Lay &L = h->L; const size_t B = (size_t)h->batch, S = (size_t)L.nu;
    const size_t C = ADJOINT_COLS;      // (the vectors of a seed in progress: one per column of a solve)
    rc |= dalloc(h, &Q.x, B * C * L.n); rc |= dalloc(h, &Q.y, B * C * L.m); rc |= dalloc(h, &Q.g, B * C * L.n);
    rc |= dalloc(h, &Q.r, B * C * L.n); rc |= dalloc(h, &Q.d, B * C * L.n); rc |= dalloc(h, &Q.e, B * C * L.n); rc |= dalloc(h, &Q.dd, B * C * L.n);
    rc |= dalloc(h, &Q.gt, B * C * L.m);
    rc |= dalloc(h, &h->adj_gw, B * L.n); rc |= dalloc(h, &h->adj_gu0, B * L.nu);
    rc |= dalloc(h, &Q.ox0, B * S * L.nx); rc |= dalloc(h, &Q.oum1, B * S * L.nu); rc |= dalloc(h, &Q.ouref, B * S * L.nu);
    rc |= dalloc(h, &Q.oxref, B * S * (size_t)L.N * L.nx);
    rc |= dalloc(h, &Q.oq, B * L.n); rc |= dalloc(h, &Q.ol, B * L.m); rc |= dalloc(h, &Q.ou, B * L.m);
    int *status = nullptr;
    rc |= dalloc(h, &Q.nact, B); rc |= dalloc(h, &Q.nweak, B); rc |= dalloc(h, &status, B);
    if (rc) return MPCQP_ERR_HIP;
    Q.status = status;
    h->aq = Q;
    return MPCQP_OK;
}
// One launch of k_adjoint: nseeds seeds per instance against one factorization (gw / gu0: the staged seeds of mpcqp_adjoint; both null: the
// unit seeds of mpcqp_gains); raw: the d_q, d_l, d_u outputs are wanted.
// dst = the step data with u_{-1} replaced by the one the last solve was made with
__global__ __launch_bounds__(256) void k_adjoint_step(Lay L, const double *step, const double *um1_used, double *dst, int batch) {
    const size_t total = (size_t)batch * L.step_sz;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int b = (int)(idx / L.step_sz), i = (int)(idx - (size_t)b * L.step_sz);
        dst[idx] = (i >= L.nx && i < L.nx + L.nu) ? um1_used[(size_t)b * L.nu + (i - L.nx)] : step[idx];
    }
}
// The adjoint's buffers with the handle's settings (mpcqp_set_adjoint) filled in: what every kernel that runs the K_pol core on a solve starts from.
static AdjointArgs adjoint_args(const mpcqp_handle *h) {
    AdjointArgs Q = h->aq;
    Q.delta = h->adj.delta; Q.refine = h->adj.refine_iter; Q.extra = h->adj.extra_iter; Q.weak_tol = h->adj.weak_tol;
    return Q;
}
// od: the gradient of the affine term per seed [batch][nseeds][d_rows nx] (mpcqp_gains_affine), or null.
static int launch_adjoint(mpcqp_handle *h, int nseeds, const double *gw, const double *gu0, bool raw_out, double *od = nullptr) {
    if (flush_puts(h)) return MPCQP_ERR_HIP;
    // mpcqp_mpc_step has left the applied input in the step data as the NEXT u_{-1}, while the iterate belongs to the one before (um1_used):
    // the bounds of the first Delta-u rows (the active set) and the QDu gradient need that one, so the kernels read a copy with it put back.
    if (h->um1_moved) {
        const size_t total = (size_t)h->batch * h->L.step_sz;
        if (!h->adj_step && dalloc(h, &h->adj_step, total)) return MPCQP_ERR_HIP;
        hipLaunchKernelGGL(k_adjoint_step, dim3((unsigned)std::min<size_t>(1024, (total + 255) / 256)), dim3(256), 0, h->stream, h->L, h->P.step, h->um1_used, h->adj_step, h->batch);
    }
    AdjointArgs Q = adjoint_args(h);
    Q.nseeds = nseeds; Q.gw = gw; Q.gu0 = gu0; Q.chain = h->L.raw ? 0 : 1; Q.od = od;
    if (!raw_out) { Q.oq = nullptr; Q.ol = nullptr; Q.ou = nullptr; }
    KpolLaunch v = kpol_launch(h);
    Lay &G = v.G;
    if (h->um1_moved) v.P.step = h->adj_step;
    // Several seeds against stages of at most 32 go four to a solve (kkt_core_cols): the work area then holds four row vectors and four stage-major
    // vectors, these two doubles further apart than their length so that the four lanes of a row position do not all meet in one LDS bank.  Where that does
    // not fit a workgroup's LDS the kernel loops over the seeds one at a time.
    Q.ncol = 1; Q.cs = 0;
    if (nseeds > 1 && G.NB <= 32) {
        const int cs = G.N * G.NB + 2;
        Lay W = G; W.tsz = std::max(G.tsz, ADJOINT_COLS * (G.m + cs));      // (the row scratch of the passes around the solves, then the columns)
        const size_t wide = sizeof(double) * (size_t)smem_common_doubles(W);
        if (wide <= 160 * 1024) { G = W; v.smem = wide; Q.ncol = ADJOINT_COLS; Q.cs = cs; }
    }
    DISPATCH_NB(G.NB, {
        if (set_smem(k_adjoint<NB>, v.smem)) return MPCQP_ERR_HIP;
        hipLaunchKernelGGL(k_adjoint<NB>, dim3(h->batch), dim3(NT), v.smem, h->stream, G, v.P, Q);
    });
    HIPCHK(hipGetLastError());
    return MPCQP_OK;
}
// The model-gradient outputs of a call, taken once from its mpcqp_adjoint_model_io (null: none): the seven pointers in field order (Ad, Bd, Qx,
// QxN, Qu, QDu, eps_feas), whether any is given, and batch_sum as the caller wrote it (each call refuses a bad one where it did before).
struct ModelOut { double *out[ADJM_FIELDS]; bool any; int batch_sum; };
static int model_out(const mpcqp_adjoint_model_io *mo, const std::string &what, ModelOut *m) {
    *m = ModelOut{};
    if (!mo) return MPCQP_OK;
    if (mo->struct_size != (int32_t)sizeof(mpcqp_adjoint_model_io)) return fail(MPCQP_ERR_ARG, what + ": struct_size is not sizeof(mpcqp_adjoint_model_io)");
    double *const out[ADJM_FIELDS] = {mo->d_Ad, mo->d_Bd, mo->d_Qx, mo->d_QxN, mo->d_Qu, mo->d_QDu, mo->d_eps_feas};
    for (int f = 0; f < ADJM_FIELDS; ++f) { m->out[f] = out[f]; if (out[f]) m->any = true; }
    m->batch_sum = mo->batch_sum;
    return MPCQP_OK;
}
// The end of a call that copies to or from the caller's arrays (null: not given; m: its model-gradient outputs too): wait, unless every one is a device pointer -- then the
// call is stream-ordered throughout and there is nothing to wait for.
static int sync_unless_all_device(mpcqp_handle *h, std::initializer_list<const void *> ptrs, const ModelOut *m = nullptr) {
    bool host = false;
    for (const void *q : ptrs) host = host || (q && !is_device_ptr(q));
    if (m) for (const double *q : m->out) host = host || (q && !is_device_ptr(q));
    if (host) HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}
static int adjoint_ready(mpcqp_handle *h, const char *what, bool chain) {
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, std::string(what) + " before mpcqp_setup");
    if (!h->has_solve) return fail(MPCQP_ERR_STATE, std::string(what) + ": no solve since the last setup, update, model update or warm start: there is no solution of the current problem to differentiate");
    if (chain && h->L.raw) return fail(MPCQP_ERR_STATE, std::string(what) + ": the handle works from raw q, l, u (mpcqp_setup_qp / mpcqp_update_vectors), where only d_q, d_l, d_u are defined");
    return MPCQP_OK;
}
// Entries of the model gradients of one instance, field by field (Ad, Bd, Qx, QxN, Qu, QDu, eps_feas), as prefix sums.
static void adjoint_model_offsets(const Lay &L, int *off) {
    const int sz[ADJM_FIELDS] = {L.nx * L.nx, L.nx * L.nu, L.nx * L.nx, L.nx * L.nx, L.nu * L.nu, L.nu * L.nu, 1};
    off[0] = 0;
    for (int f = 0; f < ADJM_FIELDS; ++f) off[f + 1] = off[f] + sz[f];
}
// The per-instance model gradients [batch][E] and their batch sum [E], on first use, like the adjoint's other buffers.
// The bound gradients (mpcqp_adjoint_bounds.h) live behind the model's in the same block: adjb_out = adjm_out + batch E.
static int adjoint_model_alloc(mpcqp_handle *h, size_t E) {
    if (h->adjm_out) return MPCQP_OK;
    const size_t EB = (size_t)adjoint_bounds_entries(h->L);
    if (dalloc(h, &h->adjm_out, (size_t)h->batch * (E + EB)) || dalloc(h, &h->adjm_sum, E) || dalloc(h, &h->adjb_sum, EB)) return MPCQP_ERR_HIP;
    h->adjb_out = h->adjm_out + (size_t)h->batch * E;
    return MPCQP_OK;
}
// adjm_sum = adjm_out added over the batch (off: adjoint_model_offsets); or, given both, `sum` = the field-major buffer `out` (off: its own table)
static void launch_adjoint_model_sum(mpcqp_handle *h, const int *off, double *out = nullptr, double *sum = nullptr) {
    AdjointModelArgs M; memset(&M, 0, sizeof(M));
    std::copy(off, off + ADJM_FIELDS + 1, M.off);
    M.out = out ? out : h->adjm_out; M.batch = h->batch;
    if (M.off[ADJM_FIELDS] < 1) return;
    hipLaunchKernelGGL(k_adjoint_model_sum, dim3((unsigned)((M.off[ADJM_FIELDS] + 15) / 16)), dim3(256), 0, h->stream, M, sum ? sum : h->adjm_sum);
}
// Every field the caller asked for, from adjm_sum (one set) or adjm_out (one per instance).
static int get_model_out(mpcqp_handle *h, const ModelOut &m, const int *off) {
    const size_t B = (size_t)h->batch;
    for (int f = 0; f < ADJM_FIELDS; ++f) {
        const size_t sz = (size_t)(off[f + 1] - off[f]);
        const double *src = m.batch_sum ? h->adjm_sum + off[f] : h->adjm_out + B * (size_t)off[f];
        if (get(h, m.out[f], src, (m.batch_sum ? 1 : B) * sz * sizeof(double))) return MPCQP_ERR_HIP;
    }
    return MPCQP_OK;
}
// k_adjoint_model behind the k_adjoint launch of the same call, k_adjoint_model_sum behind it where the batch sum is wanted.
static int launch_adjoint_model(mpcqp_handle *h, bool batch_sum) {
    const Lay G = polish_layout(h->L);
    AdjointModelArgs M; memset(&M, 0, sizeof(M));
    adjoint_model_offsets(G, M.off);
    if (adjoint_model_alloc(h, (size_t)M.off[ADJM_FIELDS])) return MPCQP_ERR_HIP;
    M.rw = h->aq.x; M.ry = h->aq.y; M.w = h->P.x; M.y = h->P.y; M.model = h->P.model; M.step = h->um1_moved ? h->adj_step : h->P.step; M.status = h->aq.status;      // (the step data k_adjoint just read)
    M.out = h->adjm_out; M.batch = h->batch;
    const size_t staged = sizeof(double) * ((size_t)NT + 2 * (size_t)G.n + 2 * (size_t)G.n_x);
    M.staged = staged <= 64 * 1024 ? 1 : 0;                  // (beyond that the vectors are read where they are)
    const size_t smem = M.staged ? staged : sizeof(double) * (size_t)NT;
    if (set_smem(k_adjoint_model, smem)) return MPCQP_ERR_HIP;
    hipLaunchKernelGGL(k_adjoint_model, dim3(h->batch), dim3(NT), smem, h->stream, G, M);
    if (batch_sum) launch_adjoint_model_sum(h, M.off);
    HIPCHK(hipGetLastError());
    return MPCQP_OK;
}
// ---- the bound gradients (include/mpcqp_adjoint_bounds.h, mpcqp_adjoint_bounds.h) ----------------------------------------------
// The bound-gradient outputs of a call, taken once from its mpcqp_adjoint_bounds_io (null: none): the six pointers in field order (xmin, xmax,
// umin, umax, Dumin, Dumax), whether any is given, and batch_sum.
struct BoundsOut { double *out[ADJB_FIELDS]; bool any; int batch_sum; };
static int bounds_out(const mpcqp_adjoint_bounds_io *bo, const std::string &what, BoundsOut *o) {
    *o = BoundsOut{};
    if (!bo) return MPCQP_OK;
    if (bo->struct_size != (int32_t)sizeof(mpcqp_adjoint_bounds_io)) return fail(MPCQP_ERR_ARG, what + ": struct_size is not sizeof(mpcqp_adjoint_bounds_io)");
    if (bo->batch_sum != 0 && bo->batch_sum != 1) return fail(MPCQP_ERR_ARG, what + ": batch_sum of mpcqp_adjoint_bounds_io is 0 or 1");
    double *const out[ADJB_FIELDS] = {bo->d_xmin, bo->d_xmax, bo->d_umin, bo->d_umax, bo->d_Dumin, bo->d_Dumax};
    for (int f = 0; f < ADJB_FIELDS; ++f) { o->out[f] = out[f]; if (out[f]) o->any = true; }
    o->batch_sum = bo->batch_sum;
    return MPCQP_OK;
}
// Entries of the bound gradients of one instance, field by field, as prefix sums -- in the table k_adjoint_model_sum reads: the fields beyond the sixth are empty.
static void adjoint_bounds_offsets(const Lay &L, int *off) {
    const int sz[ADJB_FIELDS] = {L.nx, L.nx, L.nu, L.nu, L.nu, L.nu};
    off[0] = 0;
    for (int f = 0; f < ADJM_FIELDS; ++f) off[f + 1] = off[f] + (f < ADJB_FIELDS ? sz[f] : 0);
}
// The per-instance bound gradients [batch][E] and their batch sum [E], on first use: one block with the model's (adjoint_model_alloc).
static int adjoint_bounds_alloc(mpcqp_handle *h) {
    int off[ADJM_FIELDS + 1]; adjoint_model_offsets(h->L, off);
    return adjoint_model_alloc(h, (size_t)off[ADJM_FIELDS]);
}
// The batch sum where it is wanted, then every field the caller asked for, from adjb_sum (one set) or adjb_out (one per instance).
static int get_bounds_out(mpcqp_handle *h, const BoundsOut &o) {
    int off[ADJM_FIELDS + 1]; adjoint_bounds_offsets(h->L, off);
    if (o.batch_sum) { launch_adjoint_model_sum(h, off, h->adjb_out, h->adjb_sum); HIPCHK(hipGetLastError()); }
    const size_t B = (size_t)h->batch;
    for (int f = 0; f < ADJB_FIELDS; ++f) {
        const size_t sz = (size_t)(off[f + 1] - off[f]);
        const double *src = o.batch_sum ? h->adjb_sum + off[f] : h->adjb_out + B * (size_t)off[f];
        if (get(h, o.out[f], src, (o.batch_sum ? 1 : B) * sz * sizeof(double))) return MPCQP_ERR_HIP;
    }
    return MPCQP_OK;
}
// k_adjoint_bounds behind the k_adjoint launch of the same call: the rows of seed 0 reduced to the bounds.
static int launch_adjoint_bounds(mpcqp_handle *h) {
    if (adjoint_bounds_alloc(h)) return MPCQP_ERR_HIP;
    AdjointBoundsArgs M; memset(&M, 0, sizeof(M));
    M.act = h->aq.K.act; M.ry = h->aq.y; M.status = h->aq.status; M.out = h->adjb_out; M.batch = h->batch;
    hipLaunchKernelGGL(k_adjoint_bounds, dim3(h->batch), dim3(NT), 0, h->stream, h->L, M);
    HIPCHK(hipGetLastError());
    return MPCQP_OK;
}
static bool any_host(const BoundsOut &o) {
    for (const double *q : o.out) if (q && !is_device_ptr(q)) return true;
    return false;
}
// mpcqp_adjoint (mo, bo null), mpcqp_adjoint_model (bo null) and mpcqp_adjoint_bounds: one k_adjoint launch, the model kernels behind it where
// mo asks for anything, the bound kernel where bo does.
static int adjoint_call(mpcqp_handle *h, const mpcqp_adjoint_io *io, const mpcqp_adjoint_model_io *mo, const char *what, const mpcqp_adjoint_bounds_io *bo = nullptr) {
    const std::string w(what);
    if (io->struct_size != (int32_t)sizeof(mpcqp_adjoint_io)) return fail(MPCQP_ERR_ARG, w + ": struct_size is not sizeof(mpcqp_adjoint_io)");
    ModelOut m;
    if (model_out(mo, w, &m)) return MPCQP_ERR_ARG;
    BoundsOut bd;
    if (bounds_out(bo, w, &bd)) return MPCQP_ERR_ARG;
    if (!io->g_w && !io->g_u0) return fail(MPCQP_ERR_ARG, w + ": give g_w, g_u0 or both");
    if ((io->d_l == nullptr) != (io->d_u == nullptr)) return fail(MPCQP_ERR_ARG, w + ": d_l and d_u go together");
    const bool model = m.any;
    const bool chain = io->d_x0 || io->d_uminus1 || io->d_xref || io->d_uref;
    if (mo) {
        if (m.batch_sum != 0 && m.batch_sum != 1) return fail(MPCQP_ERR_ARG, w + ": batch_sum is 0 or 1");
    }
    if ((mo || bo) && !model && !bd.any && !chain && !io->d_q && !io->d_l) return fail(MPCQP_ERR_ARG, w + ": no output asked for");
    int rc = adjoint_ready(h, what, chain || model || bd.any);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    if ((rc = adjoint_alloc(h))) return rc;
    const Lay &L = h->L; const size_t B = (size_t)h->batch, db = sizeof(double);
    if (io->g_w) HIPCHK(hipMemcpyAsync(h->adj_gw, io->g_w, B * L.n * db, hipMemcpyDefault, h->stream));
    if (io->g_u0) HIPCHK(hipMemcpyAsync(h->adj_gu0, io->g_u0, B * L.nu * db, hipMemcpyDefault, h->stream));
    if ((rc = launch_adjoint(h, 1, io->g_w ? h->adj_gw : nullptr, io->g_u0 ? h->adj_gu0 : nullptr, io->d_q || io->d_l))) return rc;
    if (model && (rc = launch_adjoint_model(h, m.batch_sum != 0))) return rc;
    if (bd.any && (rc = launch_adjoint_bounds(h))) return rc;
    const AdjointArgs &Q = h->aq;
    if (get(h, io->d_x0, Q.ox0, B * L.nx * db) || get(h, io->d_uminus1, Q.oum1, B * L.nu * db) || get(h, io->d_uref, Q.ouref, B * L.nu * db) ||
        get(h, io->d_xref, Q.oxref, B * (size_t)L.xref_rows * L.nx * db) || get(h, io->d_q, Q.oq, B * L.n * db) ||
        get(h, io->d_l, Q.ol, B * L.m * db) || get(h, io->d_u, Q.ou, B * L.m * db)) return MPCQP_ERR_HIP;
    if (model) {
        int off[ADJM_FIELDS + 1]; adjoint_model_offsets(L, off);
        if (get_model_out(h, m, off)) return MPCQP_ERR_HIP;
    }
    if (bd.any && get_bounds_out(h, bd)) return MPCQP_ERR_HIP;
    if (any_host(bd)) HIPCHK(hipStreamSynchronize(h->stream));
    return sync_unless_all_device(h, {io->g_w, io->g_u0, io->d_x0, io->d_uminus1, io->d_xref, io->d_uref, io->d_q, io->d_l, io->d_u}, &m);
}
extern "C" int mpcqp_adjoint(mpcqp_handle *h, const mpcqp_adjoint_io *io) {
    if (!h || !io) return fail(MPCQP_ERR_ARG, "null argument");
    return adjoint_call(h, io, nullptr, "mpcqp_adjoint");
}
extern "C" int mpcqp_adjoint_model(mpcqp_handle *h, const mpcqp_adjoint_io *io, const mpcqp_adjoint_model_io *mo) {
    if (!h || !io) return fail(MPCQP_ERR_ARG, "null argument");
    return adjoint_call(h, io, mo, mo ? "mpcqp_adjoint_model" : "mpcqp_adjoint");
}
extern "C" int mpcqp_adjoint_bounds(mpcqp_handle *h, const mpcqp_adjoint_io *io, const mpcqp_adjoint_model_io *mo, const mpcqp_adjoint_bounds_io *bo) {
    if (!h || !io) return fail(MPCQP_ERR_ARG, "null argument");
    return adjoint_call(h, io, mo, bo ? "mpcqp_adjoint_bounds" : mo ? "mpcqp_adjoint_model" : "mpcqp_adjoint", bo);
}
extern "C" int mpcqp_gains(mpcqp_handle *h, double *K_x0, double *K_uminus1, double *K_xref, double *K_uref) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    int rc = adjoint_ready(h, "mpcqp_gains", true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    if ((rc = adjoint_alloc(h))) return rc;
    const Lay &L = h->L; const size_t B = (size_t)h->batch, db = sizeof(double), S = (size_t)L.nu;
    if ((rc = launch_adjoint(h, L.nu, nullptr, nullptr, false))) return rc;
    const AdjointArgs &Q = h->aq;
    if (get(h, K_x0, Q.ox0, B * S * L.nx * db) || get(h, K_uminus1, Q.oum1, B * S * L.nu * db) || get(h, K_uref, Q.ouref, B * S * L.nu * db) ||
        get(h, K_xref, Q.oxref, B * S * (size_t)L.xref_rows * L.nx * db)) return MPCQP_ERR_HIP;
    return sync_unless_all_device(h, {K_x0, K_uminus1, K_xref, K_uref});
}
// mpcqp_gains that also returns K_d = d u_0 / d d (include_ext5/mpcqp_rollout_affine.h): the same launch -- one factorization, the nu unit seeds, four to a solve where
// mpcqp_gains does that -- in which k_adjoint writes each seed's row of the term's gradient beside its other outputs.
extern "C" int mpcqp_gains_affine(mpcqp_handle *h, double *K_x0, double *K_uminus1, double *K_xref, double *K_uref, double *K_d) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (h->is_setup && !h->L.d_rows) return fail(MPCQP_ERR_STATE, "mpcqp_gains_affine: the handle has no affine term (mpcqp_set_affine); mpcqp_gains is the call without one");
    int rc = adjoint_ready(h, "mpcqp_gains_affine", true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    if ((rc = adjoint_alloc(h))) return rc;
    const Lay &L = h->L; const size_t B = (size_t)h->batch, db = sizeof(double), S = (size_t)L.nu;
    if (!h->aff_gain && dalloc(h, &h->aff_gain, B * S * (size_t)L.Np * L.nx)) return MPCQP_ERR_HIP;
    if ((rc = launch_adjoint(h, L.nu, nullptr, nullptr, false, h->aff_gain))) return rc;
    const AdjointArgs &Q = h->aq;
    if (get(h, K_x0, Q.ox0, B * S * L.nx * db) || get(h, K_uminus1, Q.oum1, B * S * L.nu * db) || get(h, K_uref, Q.ouref, B * S * L.nu * db) ||
        get(h, K_xref, Q.oxref, B * S * (size_t)L.xref_rows * L.nx * db) || get(h, K_d, h->aff_gain, B * S * (size_t)L.d_rows * L.nx * db)) return MPCQP_ERR_HIP;
    return sync_unless_all_device(h, {K_x0, K_uminus1, K_xref, K_uref, K_d});
}
extern "C" int mpcqp_get_adjoint_info(mpcqp_handle *h, int32_t *n_active, int32_t *n_weak, int32_t *status) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = sizeof(int32_t) * (size_t)h->batch;
    int32_t *dst[3] = {n_active, n_weak, status};
    const int *src[3] = {h->aq.nact, h->aq.nweak, h->aq.status};
    for (int i = 0; i < 3; ++i) {
        if (!dst[i]) continue;
        if (h->aq.status) HIPCHK(hipMemcpyAsync(dst[i], src[i], bytes, hipMemcpyDefault, h->stream));
        else if (is_device_ptr(dst[i])) HIPCHK(hipMemsetAsync(dst[i], 0, bytes, h->stream));      // (no adjoint call yet)
        else memset(dst[i], 0, bytes);
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

// what mpcqp_mpc_loop refuses (before anything is launched or changed)
static int loop_check(mpcqp_handle *h, int nsteps, const mpcqp_loop *io) {
    if (!h || !io || nsteps < 1) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop: bad argument");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_mpc_loop before mpcqp_setup");
    if (h->pol.polish) return fail(MPCQP_ERR_UNSUPPORTED, "mpcqp_mpc_loop / mpcqp_mpc_run: solution polishing inside the device closed loop is not implemented; switch polish off (mpcqp_set_polish) or step with mpcqp_mpc_step");
    if ((io->Ap == nullptr) != (io->Bp == nullptr)) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop: give both Ap and Bp or neither");
    const int ny = io->ny;
    if (ny < 0 || ny > 64) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop: ny must be in 0..64");
    if (ny && (!io->C || !io->Lgain || !io->x_true)) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop: output feedback needs C, Lgain and x_true");
    if (io->xref_traj && io->xref_rows != 0 && io->xref_rows != 1 && io->xref_rows != h->L.N)
        return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop: xref_rows must be 0 (as last uploaded), 1 or Np+1");
    HIPCHK(hipSetDevice(h->device));
    if (h->L.raw) return fail(MPCQP_ERR_STATE, "mpcqp_mpc_loop: the handle holds raw q, l, u (mpcqp_update_vectors); call mpcqp_update first");
    return MPCQP_OK;
}
// balance: the call may end with a wait for the stream and a rebuild of the workgroup -> instance map when one is due (not between the segments of
// mpcqp_mpc_loop_tv, which does it once at its end)
static int loop_run(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, bool balance) {
    const int ny = io->ny;
    if (io->xref_traj && io->xref_rows) h->L.xref_rows = io->xref_rows;     // update(x, u, xref_k) with this reference shape
    const Lay &L = h->L;
    const size_t B = (size_t)h->batch, K = (size_t)nsteps, nx = L.nx, nu = L.nu;
    const size_t xblk = (size_t)L.xref_rows * nx;
    // Buffers the caller keeps in DEVICE memory are used in place (the kernel reads and writes them directly, the call is
    // stream-ordered and returns without waiting); host buffers go through one staging block on the device: inputs are
    // copied in before the launch, outputs copied out after it, and the call returns when they have arrived.
    struct Part { const void *src; void *dst; size_t bytes; size_t off; bool direct; };
    Part parts[16]; int np = 0; size_t total = 0; bool any_host = false;      // (fifteen parts are added below)
    auto add = [&](const void *src, void *dst, size_t bytes) {
        const void *user = src ? src : dst;
        const bool direct = bytes && user && is_device_ptr(user);
        parts[np] = Part{src, dst, bytes, total, direct};
        if (bytes && !direct) { total += (bytes + 15) & ~size_t(15); any_host = true; }      // (a host INPUT must stay valid until its staged copy has been made: the call waits for that too)
        return np++;
    };
    const int iw = add(io->w, nullptr, io->w ? 8 * K * B * nx : 0);
    const int iA = add(io->Ap, nullptr, io->Ap ? 8 * B * nx * nx : 0), iB = add(io->Bp, nullptr, io->Bp ? 8 * B * nx * nu : 0);
    const int ir = add(io->xref_traj, nullptr, io->xref_traj ? 8 * K * B * xblk : 0);
    // mpcqp_mpc_loop_affine: the entries this launch's steps k0 .. k0 + K - 1 use, e0 .. e1 of the schedule
    const mpcqp_affine_traj *at = h->loop_aff;
    const size_t dblk = at ? (size_t)at->rows * nx : 0, e0 = at ? h->loop_aff_k0 / (size_t)at->hold : 0, e1 = at ? (h->loop_aff_k0 + K - 1) / (size_t)at->hold : 0;
    const int id = add(at ? at->d + e0 * B * dblk : nullptr, nullptr, at ? 8 * (e1 - e0 + 1) * B * dblk : 0);
    const int iC = add(io->C, nullptr, ny ? 8 * B * ny * nx : 0), iL = add(io->Lgain, nullptr, ny ? 8 * B * nx * ny : 0);
    const int iv = add(io->v, nullptr, (ny && io->v) ? 8 * K * B * ny : 0);
    const int ixt = add(io->x_true, io->x_true, ny ? 8 * B * nx : 0);
    const int ox = add(nullptr, io->x_traj, 8 * (K + 1) * B * nx), oxh = add(nullptr, io->xhat_traj, ny ? 8 * (K + 1) * B * nx : 0);
    const int oy = add(nullptr, io->y_traj, ny ? 8 * K * B * ny : 0), ou = add(nullptr, io->u_traj, 8 * K * B * nu);
    const int os = add(nullptr, io->status_traj, 4 * K * B), oi = add(nullptr, io->iter_traj, 4 * K * B);
    if (total > h->run_bytes) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->run_buf) hipFree(h->run_buf);
        h->run_buf = nullptr; h->run_bytes = 0;
        HIPCHK(hipMalloc(&h->run_buf, total));
        h->run_bytes = total;
    }
    char *base = (char *)h->run_buf;
    auto dev = [&](int i) -> void * {
        if (!parts[i].bytes) return nullptr;
        if (parts[i].direct) return parts[i].src ? const_cast<void *>(parts[i].src) : parts[i].dst;
        return base + parts[i].off;
    };
    for (int i = 0; i < np; ++i)
        if (parts[i].src && parts[i].bytes && !parts[i].direct) HIPCHK(hipMemcpyAsync(dev(i), parts[i].src, parts[i].bytes, hipMemcpyDefault, h->stream));
    RunArgs R; memset(&R, 0, sizeof(R));
    R.nsteps = nsteps;
    R.w = (const double *)dev(iw); R.Ap = (const double *)dev(iA); R.Bp = (const double *)dev(iB);
    R.xref_traj = (const double *)dev(ir); R.xref_blk = (int)xblk;
    R.d_traj = (const double *)dev(id); R.d_blk = (int)dblk; R.d_hold = at ? at->hold : 1; R.d_k0 = at ? (int)(h->loop_aff_k0 - e0 * (size_t)at->hold) : 0;
    R.ny = ny; R.C = (const double *)dev(iC); R.Lg = (const double *)dev(iL); R.v = (const double *)dev(iv); R.x_true = (double *)dev(ixt);
    R.x_traj = (double *)dev(ox); R.xhat_traj = (double *)dev(oxh); R.y_traj = (double *)dev(oy); R.u_traj = (double *)dev(ou);
    R.status_traj = (int *)dev(os); R.iter_traj = (int *)dev(oi);
    // a schedule's shape is the handle's from this launch on (every solve of the launch follows a step: none is made with the term the handle held
    // before) -- set once the staging above has succeeded, and taken back if the launch is refused: a call that fails changes nothing
    const int d_rows_before = h->L.d_rows;
    if (at) h->L.d_rows = at->rows;
    int rc = launch_run(h, R, 0);
    if (rc) { h->L.d_rows = d_rows_before; return rc; }
    if (h->pq.status) HIPCHK(hipMemsetAsync(h->pq.status, 0, sizeof(int) * B, h->stream));      // (the last solve of the loop: not polished)
    for (int i = 0; i < np; ++i)
        if (parts[i].dst && parts[i].bytes && !parts[i].direct && get(h, parts[i].dst, dev(i), parts[i].bytes)) return MPCQP_ERR_HIP;
    const bool due = balance && balance_due(h);
    if (!due && !any_host) return MPCQP_OK;                   // every buffer is device memory: stream-ordered, nothing to wait for
    HIPCHK(hipStreamSynchronize(h->stream));
    return due ? rebalance(h) : MPCQP_OK;
}
extern "C" int mpcqp_mpc_loop(mpcqp_handle *h, int nsteps, const mpcqp_loop *io) {
    const int rc = loop_check(h, nsteps, io);
    return rc ? rc : loop_run(h, nsteps, io, true);
}

// io with every trajectory buffer advanced to step k0 (row k0 of x_traj and xhat_traj is written again: the state the steps before ended in).
// The estimator's buffers move only where there is one (io->ny > 0).
static mpcqp_loop loop_at(const mpcqp_handle *h, const mpcqp_loop *io, size_t k0) {
    const Lay &L = h->L;
    const size_t B = (size_t)h->batch, nx = L.nx, nu = L.nu, ny = (size_t)io->ny;
    const size_t xblk = (size_t)(io->xref_traj && io->xref_rows ? io->xref_rows : L.xref_rows) * nx;
    mpcqp_loop seg = *io;
    if (seg.w) seg.w += k0 * B * nx;
    if (seg.xref_traj) seg.xref_traj += k0 * B * xblk;
    if (seg.x_traj) seg.x_traj += k0 * B * nx;
    if (seg.u_traj) seg.u_traj += k0 * B * nu;
    if (seg.status_traj) seg.status_traj += k0 * B;
    if (seg.iter_traj) seg.iter_traj += k0 * B;
    if (ny) {
        if (seg.v) seg.v += k0 * B * ny;
        if (seg.xhat_traj) seg.xhat_traj += k0 * B * nx;
        if (seg.y_traj) seg.y_traj += k0 * B * ny;
    }
    return seg;
}
// The refusals a schedule adds to a loop's, in mpcqp_mpc_loop_tv's order.  est: the call is one of include_ext2/mpcqp_rollout_tv_est.h (an
// estimator is expected, et: its gain schedule or null); otherwise an estimator is refused.  Sets *nseg.
static int schedule_check(const std::string &what, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt, bool est, const mpcqp_est_traj *et, int *nseg) {
    if (mt->struct_size != (int32_t)sizeof(mpcqp_model_traj)) return fail(MPCQP_ERR_ARG, what + ": struct_size is not sizeof(mpcqp_model_traj)");
    if (mt->hold < 1) return fail(MPCQP_ERR_ARG, what + ": hold must be >= 1");
    *nseg = (nsteps + mt->hold - 1) / mt->hold;
    if (mt->nmodels < *nseg) return fail(MPCQP_ERR_ARG, what + ": fewer than ceil(nsteps / hold) model entries");
    if (!mt->Ad && !mt->Bd) return fail(MPCQP_ERR_ARG, what + ": give Ad, Bd or both");
    if (!est && io->ny > 0) return fail(MPCQP_ERR_UNSUPPORTED, what + ": output feedback with a model schedule is " + what + "_est (include_ext2/mpcqp_rollout_tv_est.h)");
    if (est && io->ny == 0) return fail(MPCQP_ERR_ARG, what + ": ny must be > 0 (without an estimator the call is the one without _est)");
    if (et && et->struct_size != (int32_t)sizeof(mpcqp_est_traj)) return fail(MPCQP_ERR_ARG, what + ": struct_size is not sizeof(mpcqp_est_traj)");
    if (et && et->nentries < *nseg) return fail(MPCQP_ERR_ARG, what + ": fewer than ceil(nsteps / hold) gain entries");
    return MPCQP_OK;
}
// The device loop under a schedule of models (include/mpcqp_model.h): per entry, mpcqp_update_model and one closed-loop launch of the steps it holds for.
// et (mpcqp_mpc_loop_tv_est): the gain of entry s, where the schedule has gains, is the estimator's during segment s.
static int loop_tv(mpcqp_handle *h, int nsteps, const mpcqp_loop *io_in, const mpcqp_model_traj *mt, const std::string &what, bool est, const mpcqp_est_traj *et) {
    int nseg = 0;
    int rc = schedule_check(what, nsteps, io_in, mt, est, et, &nseg);
    if (rc) return rc;
    const double *Lt = et ? et->Lgain_traj : nullptr;
    mpcqp_loop first = *io_in;
    if (Lt) first.Lgain = Lt;                       // (a gain schedule stands in for io->Lgain, which may then be null)
    const mpcqp_loop *io = &first;
    if ((rc = loop_check(h, nsteps, io))) return rc;
    const Lay &L = h->L;
    const size_t B = (size_t)h->batch, nx = L.nx, nu = L.nu;
    for (int s = 0; s < nseg; ++s) {
        const size_t k0 = (size_t)s * mt->hold;
        mpcqp_model M; memset(&M, 0, sizeof(M));
        if (mt->Ad) M.Ad = mt->Ad + (size_t)s * B * nx * nx;
        if (mt->Bd) M.Bd = mt->Bd + (size_t)s * B * nx * nu;
        if ((rc = mpcqp_update_model(h, &M))) return rc;
        mpcqp_loop seg = loop_at(h, io, k0);
        h->loop_aff_k0 = k0;
        if (Lt) seg.Lgain = Lt + (size_t)s * B * nx * (size_t)io->ny;
        if ((rc = loop_run(h, std::min(mt->hold, nsteps - (int)k0), &seg, s == nseg - 1))) return rc;
    }
    return MPCQP_OK;
}
extern "C" int mpcqp_mpc_loop_tv(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt) {
    if (!mt) return mpcqp_mpc_loop(h, nsteps, io);
    if (!h || !io || nsteps < 1) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop_tv: bad argument");
    return loop_tv(h, nsteps, io, mt, "mpcqp_mpc_loop_tv", false, nullptr);
}
// The output-feedback loop under a schedule of models and, optionally, of observer gains (include_ext2/mpcqp_rollout_tv_est.h).
extern "C" int mpcqp_mpc_loop_tv_est(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt, const mpcqp_est_traj *et) {
    if (!h || !io || !mt || nsteps < 1) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop_tv_est: bad argument");
    return loop_tv(h, nsteps, io, mt, "mpcqp_mpc_loop_tv_est", true, et);
}

// ---- the affine term of the prediction model (include_ext4/mpcqp_affine.h; device side: affine_bound in mpcqp_qp.h, mpcqp_affine.h) ----
// The term lives in the step blob behind du0 (Lay::od, Np nx doubles) and is in force while Lay::d_rows > 0.
extern "C" int mpcqp_set_affine(mpcqp_handle *h, const double *d, int d_rows) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_set_affine before mpcqp_setup");
    if (h->L.raw || h->step_blank || h->csc) return fail(MPCQP_ERR_STATE, "mpcqp_set_affine: the handle works from raw q, l, u (mpcqp_setup_qp / _csc, mpcqp_update_vectors): the dynamics rows' bounds are the caller's there");
    if (d_rows != 0 && d_rows != 1 && d_rows != h->L.Np) return fail(MPCQP_ERR_ARG, "mpcqp_set_affine: d_rows must be 0 (clear), 1 or Np");
    HIPCHK(hipSetDevice(h->device));
    h->has_solve = false;                           // (the bounds no longer belong to the iterate: mpcqp_adjoint waits for the next solve)
    if (!d || d_rows == 0) { h->L.d_rows = 0; return MPCQP_OK; }
    h->pack.n = 0;
    if (put(h, h->P.step, h->L.step_sz, h->L.od, d, d_rows * h->L.nx)) return MPCQP_ERR_HIP;
    h->L.d_rows = d_rows;
    return flush_puts(h) ? MPCQP_ERR_HIP : MPCQP_OK;
}
extern "C" int mpcqp_get_affine(mpcqp_handle *h, double *d, int *d_rows) {
    if (!h || !d_rows) return fail(MPCQP_ERR_ARG, "mpcqp_get_affine: null argument");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_get_affine before mpcqp_setup");
    *d_rows = h->L.d_rows;
    if (!d || !h->L.d_rows) return MPCQP_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t w = sizeof(double) * (size_t)h->L.d_rows * h->L.nx;
    HIPCHK(hipMemcpy2DAsync(d, w, h->P.step + h->L.od, sizeof(double) * (size_t)h->L.step_sz, w, (size_t)h->batch, hipMemcpyDefault, h->stream));
    return sync_unless_all_device(h, {d});
}
extern "C" int mpcqp_mpc_loop_affine(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt, const mpcqp_affine_traj *at) {
    if (!at) return mpcqp_mpc_loop_tv(h, nsteps, io, mt);
    if (!h || !io || nsteps < 1) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop_affine: bad argument");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_mpc_loop_affine before mpcqp_setup");
    if (at->struct_size != (int32_t)sizeof(mpcqp_affine_traj)) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop_affine: struct_size is not sizeof(mpcqp_affine_traj)");
    if (at->hold < 1) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop_affine: hold must be >= 1");
    if (at->nentries < (nsteps + at->hold - 1) / at->hold) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop_affine: fewer than ceil(nsteps / hold) entries");
    if (at->rows != 1 && at->rows != h->L.Np) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop_affine: rows must be 1 or Np");
    if (!at->d) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_loop_affine: no entries given (at == NULL runs the loop with the handle's own term)");
    if (io->ny > 0) return fail(MPCQP_ERR_UNSUPPORTED, "mpcqp_mpc_loop_affine: output feedback under a schedule of affine terms is not implemented");
    h->loop_aff = at; h->loop_aff_k0 = 0;           // (read by loop_run; what mt's schedule and the loop refuse, they refuse before anything is launched or changed)
    int rc = mt ? loop_tv(h, nsteps, io, mt, "mpcqp_mpc_loop_affine", false, nullptr) : loop_check(h, nsteps, io);
    if (!mt && !rc) rc = loop_run(h, nsteps, io, true);
    h->loop_aff = nullptr; h->loop_aff_k0 = 0;
    return rc;
}
extern "C" int mpcqp_adjoint_affine(mpcqp_handle *h, const mpcqp_adjoint_io *io, double *d_d) {
    if (!h || !io || !d_d) return fail(MPCQP_ERR_ARG, "mpcqp_adjoint_affine: null argument");
    if (h->is_setup && !h->L.d_rows) return fail(MPCQP_ERR_STATE, "mpcqp_adjoint_affine: the handle has no affine term (mpcqp_set_affine)");
    int rc = adjoint_call(h, io, nullptr, "mpcqp_adjoint_affine");
    if (rc) return rc;
    const Lay &L = h->L; const size_t B = (size_t)h->batch, w = (size_t)L.d_rows * L.nx;
    if (!h->aff_out && dalloc(h, &h->aff_out, B * (size_t)L.Np * L.nx)) return MPCQP_ERR_HIP;
    hipLaunchKernelGGL(k_affine_grad, dim3(h->batch), dim3(NT), 0, h->stream, L, (const double *)h->aq.y, (const int *)h->aq.status, h->aff_out);      // (behind k_adjoint: r_y of seed 0 as it left it)
    HIPCHK(hipGetLastError());
    if (get(h, d_d, h->aff_out, B * w * sizeof(double))) return MPCQP_ERR_HIP;
    return sync_unless_all_device(h, {d_d});
}

// ---- a rollout with a tape and its reverse sweep (include/mpcqp_rollout.h, mpcqp_rollout.h) ------------------------------------
// The tape and the sweep's staging are ONE device block: a rollout that cannot get it changes nothing, and releasing it is one call.
// base null: sizes only.  Returns the bytes of the block.
// ny > 0: a tape of the output-feedback loop -- the plant states, measurements, C, L and the estimator's seeds and gradients behind the rest.
// nslots > 0: a tape of the loop under a model schedule -- the model slots and their gradients behind the rest (V).
// both: the gain of every schedule entry and the estimator path's per-entry gradients behind those (X).
// aslots > 0: a tape of mpcqp_rollout_affine -- its affine area (mpcqp_rollout.h: header, the gradient per slot, the terms per slot) RIGHT BEHIND the
// block of T.nact, where the sweep looks for it; a tape without one has the layout and the size it always had.
static size_t tape_carve(const Lay &L, int batch, int nsteps, int xref_rows, int ny, char *base, RolloutTape *T, int nslots = 0, int hold = 0, RolloutSlots *V = nullptr,
                         RolloutGains *X = nullptr, int aslots = 0, int arows = 0, int ahold = 0, RolloutAffine *F = nullptr) {
    const size_t B = (size_t)batch, K = (size_t)nsteps, nx = L.nx, nu = L.nu, xw = (size_t)xref_rows * nx, db = sizeof(double);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += (bytes + 255) & ~size_t(255); return q; };
    RolloutTape t; memset(&t, 0, sizeof(t));
    t.x = (double *)take(K * B * L.n * db); t.z = (double *)take(K * B * L.m * db); t.y = (double *)take(K * B * L.m * db);
    t.step = (double *)take(K * B * L.step_sz * db); t.u = (double *)take(K * B * nu * db); t.status = (int *)take(K * B * sizeof(int));
    t.Ap = (double *)take(B * nx * nx * db); t.Bp = (double *)take(B * nx * nu * db);
    t.gx = (double *)take((K + 1) * B * nx * db); t.gu = (double *)take(K * B * nu * db); t.lam = (double *)take((K + 1) * B * nx * db);
    t.dxref = (double *)take(K * B * xw * db); t.dum1 = (double *)take(B * nu * db); t.duref = (double *)take(B * nu * db);
    t.dAp = (double *)take(B * nx * nx * db); t.dBp = (double *)take(B * nx * nu * db);
    t.carry = (double *)take(B * (size_t)rollout_carry_doubles(L, ny) * db);
    t.nact = (int *)take((3 * K * B + B) * sizeof(int)); t.nweak = t.nact + K * B; t.st = t.nweak + K * B; t.nfactor = t.st + K * B;
    t.nsteps = nsteps; t.batch = batch;
    RolloutAffine f; memset(&f, 0, sizeof(f));
    if (aslots > 0) {
        const size_t per = (size_t)aslots * B * (size_t)arows * nx * db;
        f.nslots = aslots; f.rows = arows; f.hold = ahold;
        f.header = (int *)take(ROLLOUT_AFFINE_HEADER); f.dgrad = (double *)take(per); f.dval = (double *)take(per);
    }
    if (F) *F = f;
    if (ny > 0) {
        const size_t q = (size_t)ny;
        t.ny = ny;
        t.xp = (double *)take((K + 1) * B * nx * db); t.ym = (double *)take(K * B * q * db);
        t.C = (double *)take(B * q * nx * db); t.Lg = (double *)take(B * nx * q * db); t.xt = (double *)take(B * nx * db);
        t.gxh = (double *)take((K + 1) * B * nx * db); t.gy = (double *)take(K * B * q * db);
        t.eta = (double *)take((K + 1) * B * nx * db); t.dv = (double *)take(K * B * q * db);
        t.dC = (double *)take(B * q * nx * db); t.dL = (double *)take(B * nx * q * db);
        t.dAe = (double *)take(B * nx * nx * db); t.dBe = (double *)take(B * nx * nu * db);
    }
    RolloutSlots v; memset(&v, 0, sizeof(v));
    if (nslots > 0) {
        const size_t S = (size_t)nslots;
        v.nslots = nslots; v.hold = hold;
        v.model = (double *)take(S * B * L.model_sz * db); v.D = (double *)take(S * B * L.n * db); v.E = (double *)take(S * B * L.m * db); v.c = (double *)take(S * B * db);
        v.dAd = (double *)take(S * B * nx * nx * db); v.dBd = (double *)take(S * B * nx * nu * db);
        v.dAp = (double *)take((S - 1) * B * nx * nx * db); v.dBp = (double *)take((S - 1) * B * nx * nu * db);
    }
    RolloutGains x; memset(&x, 0, sizeof(x));
    if (nslots > 0 && ny > 0) {
        const size_t S1 = (size_t)nslots - 1, q = (size_t)ny;
        x.Lg = (double *)take(S1 * B * nx * q * db); x.dL = (double *)take(S1 * B * nx * q * db);
        x.dAe = (double *)take(S1 * B * nx * nx * db); x.dBe = (double *)take(S1 * B * nx * nu * db);
    }
    if (T) *T = t;
    if (V) *V = v;
    if (X) *X = x;
    return off;
}
extern "C" int mpcqp_rollout_tape_bytes(mpcqp_handle *h, int nsteps, int64_t *bytes) {
    if (!h || !bytes || nsteps < 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_tape_bytes: bad argument");
    *bytes = (int64_t)tape_carve(h->L, h->batch, nsteps, h->L.xref_rows, 0, nullptr, nullptr);
    return MPCQP_OK;
}
extern "C" int mpcqp_rollout_release(mpcqp_handle *h) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    if (h->tape_buf) { HIPCHK(hipStreamSynchronize(h->stream)); hipFree(h->tape_buf); }
    h->tape_buf = nullptr; h->tape_bytes = 0; h->tape_valid = false; h->tape_ny = 0;
    memset(&h->tape, 0, sizeof(h->tape)); memset(&h->tape_slots, 0, sizeof(h->tape_slots)); memset(&h->tape_gains, 0, sizeof(h->tape_gains));
    memset(&h->tape_aff, 0, sizeof(h->tape_aff));
    return MPCQP_OK;
}
// What the calls that read the tape back refuse: no tape, for the estimator's part a tape without one, an entry k (null: the call takes none) out of range.
static int tape_guard(const mpcqp_handle *h, const std::string &fn, bool est, const int *k) {
    if (!h->tape_buf || h->tape.nsteps < 1) return fail(MPCQP_ERR_STATE, fn + ": the handle holds no tape (call " + (est ? "mpcqp_rollout_est" : "mpcqp_rollout") + " first)");
    if (est && h->tape_ny == 0) return fail(MPCQP_ERR_STATE, fn + ": the tape is one of mpcqp_rollout (no estimator)");
    if (k && (*k < 0 || *k >= h->tape.nsteps)) return fail(MPCQP_ERR_ARG, fn + ": k must be in 0 .. nsteps - 1");
    return MPCQP_OK;
}
// The taped loop behind mpcqp_rollout (io->ny == 0) and mpcqp_rollout_est (io->ny > 0): the refusals, the tape's one allocation and its
// invalidation, k_rollout_tape and one closed-loop launch per step with the trajectory buffers advanced to that step.  With an estimator C, L,
// the plant and x_true are read from the tape's copies, and x_k, x_{k+1}, y_k are written straight onto the tape (x_traj, y_traj of the step).
// mt (mpcqp_rollout_tv): the loop is mpcqp_mpc_loop_tv's -- at a boundary step the tape's copy, then mpcqp_update_model with the entry, then a
// copy of what the handle holds now (model blob, D, E, c) into the entry's slot, then the step; slot 0 is what it held when the call began.
// est (mpcqp_rollout_tv_est): both at once -- the tape keeps the gain of every entry too (et's, or io->Lgain over and over), and the step of
// entry e runs with its gain.
// affine (mpcqp_rollout_affine, include_ext5/mpcqp_rollout_affine.h): the loop is mpcqp_mpc_loop_affine's -- every step's launch takes its term from the
// schedule `at` (null: the handle's own term throughout), and the tape keeps the terms as slots: slot 0 what the handle held when the call began (zeros,
// written here, where it held none -- into entry 0's step data too, which the sweep reads under the tape's d_rows), slot e + 1 schedule entry e.
static int rollout_forward(mpcqp_handle *h, int nsteps, const mpcqp_loop *io_in, const std::string &what, const mpcqp_model_traj *mt = nullptr,
                           bool est = false, const mpcqp_est_traj *et = nullptr, bool affine = false, const mpcqp_affine_traj *at = nullptr) {
    int nseg = 0, rc = 0;
    if (mt && (rc = schedule_check(what, nsteps, io_in, mt, est, et, &nseg))) return rc;      // (the refusals of mpcqp_mpc_loop_tv, in its order)
    const int nslots = mt ? nseg + 1 : 0, hold = mt ? mt->hold : 0;
    const double *Lt = et ? et->Lgain_traj : nullptr;
    mpcqp_loop first = *io_in;
    if (Lt) first.Lgain = Lt;                       // (a gain schedule stands in for io->Lgain, which may then be null)
    const mpcqp_loop *io = &first;
    if ((rc = loop_check(h, nsteps, io))) return rc;
    if (!affine && h->L.d_rows) return fail(MPCQP_ERR_UNSUPPORTED, what + ": the handle has an affine term (include_ext4/mpcqp_affine.h: mpcqp_set_affine), which the taped rollouts and their reverse sweeps do not carry; clear it (mpcqp_set_affine(h, NULL, 0)) or run mpcqp_mpc_loop_affine");
    if (affine && !at && !h->L.d_rows) return fail(MPCQP_ERR_STATE, what + ": no schedule of terms given and the handle has no affine term (mpcqp_set_affine): mpcqp_rollout is the taped loop without one");
    if (!h->has_solve) return fail(MPCQP_ERR_STATE, what + ": no solve since the last setup, update, model update or warm start: the iterate does not belong to the step data of tape entry 0");
    if (io->xref_traj && io->xref_rows && io->xref_rows != h->L.xref_rows)
        return fail(MPCQP_ERR_UNSUPPORTED, what + ": xref_traj must have the reference shape of the last upload (the entries of a tape have one shape)");
    const Lay &L = h->L;
    const size_t B = (size_t)h->batch, nx = L.nx, nu = L.nu, ny = (size_t)io->ny, db = sizeof(double);
    const int arows = !affine ? 0 : at ? at->rows : L.d_rows, ahold = at ? at->hold : 0, aslots = affine ? rollout_affine_nslots(nsteps, ahold) : 0;
    const int rows_before = L.d_rows;               // (the handle's own term, if any: slot 0)
    const size_t bytes = tape_carve(L, h->batch, nsteps, L.xref_rows, io->ny, nullptr, nullptr, nslots, hold, nullptr, nullptr, aslots, arows, ahold);
    if (!h->tape_buf || bytes > h->tape_bytes) {
        void *q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(MPCQP_ERR_HIP, what + ": the tape could not be allocated (" + what + "_tape_bytes says how much it takes)"); }
        if (h->tape_buf) { HIPCHK(hipStreamSynchronize(h->stream)); hipFree(h->tape_buf); }
        h->tape_buf = q; h->tape_bytes = bytes;
    }
    h->tape_valid = false;
    RolloutTape T; RolloutSlots V; RolloutGains X; RolloutAffine F;
    tape_carve(L, h->batch, nsteps, L.xref_rows, io->ny, (char *)h->tape_buf, &T, nslots, hold, &V, &X, aslots, arows, ahold, &F);
    memset(&h->tape_aff, 0, sizeof(h->tape_aff));   // (not an affine tape until this call has made one)
    if (affine) {                                   // the header the sweep reads, the terms of every slot, a zero gradient until a sweep writes one
        const size_t aw = (size_t)arows * nx * db;
        HIPCHK(hipMemsetAsync(F.header, 0, ROLLOUT_AFFINE_HEADER, h->stream));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)F.header, ahold, 1, h->stream));
        HIPCHK(hipMemsetAsync(F.dgrad, 0, (size_t)aslots * B * aw, h->stream));
        if (rows_before) HIPCHK(hipMemcpy2DAsync(F.dval, aw, h->P.step + L.od, db * (size_t)L.step_sz, aw, B, hipMemcpyDeviceToDevice, h->stream));
        else HIPCHK(hipMemsetAsync(F.dval, 0, B * aw, h->stream));
        if (at) HIPCHK(hipMemcpyAsync(F.dval + B * (size_t)arows * nx, at->d, (size_t)(aslots - 1) * B * aw, hipMemcpyDefault, h->stream));
    }
    auto keep_slot = [&](int s) -> int {                   // what the handle holds now, as slot s
        const size_t sB = (size_t)s * B;
        HIPCHK(hipMemcpyAsync(const_cast<double *>(V.model) + sB * L.model_sz, h->P.model, B * L.model_sz * db, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(const_cast<double *>(V.D) + sB * L.n, h->P.D, B * L.n * db, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(const_cast<double *>(V.E) + sB * L.m, h->P.E, B * L.m * db, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(const_cast<double *>(V.c) + sB, h->P.c, B * db, hipMemcpyDeviceToDevice, h->stream));
        return MPCQP_OK;
    };
    if (mt && (rc = keep_slot(0))) return rc;
    if (io->Ap) {
        HIPCHK(hipMemcpyAsync(T.Ap, io->Ap, B * nx * nx * db, hipMemcpyDefault, h->stream));
        HIPCHK(hipMemcpyAsync(T.Bp, io->Bp, B * nx * nu * db, hipMemcpyDefault, h->stream));
    } else { T.Ap = nullptr; T.Bp = nullptr; }
    if (ny) {                                       // (a host x_true makes one round trip per call, not per step)
        HIPCHK(hipMemcpyAsync(T.C, io->C, B * ny * nx * db, hipMemcpyDefault, h->stream));
        HIPCHK(hipMemcpyAsync(T.Lg, io->Lgain, B * nx * ny * db, hipMemcpyDefault, h->stream));
        HIPCHK(hipMemcpyAsync(T.xt, io->x_true, B * nx * db, hipMemcpyDefault, h->stream));
        if (mt && Lt) HIPCHK(hipMemcpyAsync(const_cast<double *>(X.Lg), Lt, (size_t)nseg * B * nx * ny * db, hipMemcpyDefault, h->stream));
        else if (mt) for (int e = 0; e < nseg; ++e) HIPCHK(hipMemcpyAsync(const_cast<double *>(X.Lg) + (size_t)e * B * nx * ny, T.Lg, B * nx * ny * db, hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(hipMemsetAsync(T.nact, 0, (3 * (size_t)nsteps * B + B) * sizeof(int), h->stream));      // (mpcqp_get_rollout_info before a sweep: all zero)
    h->tape = T; h->tape_slots = V; h->tape_gains = X; h->tape_xref_rows = L.xref_rows; h->tape_ny = io->ny;
    struct AffGuard { mpcqp_handle *h; ~AffGuard() { h->loop_aff = nullptr; h->loop_aff_k0 = 0; } } aff_guard{h};      // (loop_run reads them; cleared however the call ends)
    const size_t per = (size_t)L.n + 2 * (size_t)L.m + L.step_sz + nu + 1;
    const unsigned grid = (unsigned)std::min<size_t>(1024, (B * per + 255) / 256);
    for (int k = 0; k < nsteps; ++k) {
        hipLaunchKernelGGL(k_rollout_tape, dim3(grid), dim3(256), 0, h->stream, h->L, h->P, T, k, (const double *)(h->um1_moved ? h->um1_used : nullptr));
        HIPCHK(hipGetLastError());
        const size_t k0 = (size_t)k;
        if (affine && k == 0 && !rows_before)       // entry 0 was solved without a term: zeros under the tape's d_rows, not whatever the blob held there
            HIPCHK(hipMemset2DAsync(T.step + L.od, db * (size_t)L.step_sz, 0, (size_t)arows * nx * db, B, h->stream));
        if (mt && k % hold == 0) {                  // a boundary step: the entry replaces the model under the iterate the tape has just copied
            const size_t e = (size_t)(k / hold);
            mpcqp_model M; memset(&M, 0, sizeof(M));
            if (mt->Ad) M.Ad = mt->Ad + e * B * nx * nx;
            if (mt->Bd) M.Bd = mt->Bd + e * B * nx * nu;
            if ((rc = mpcqp_update_model(h, &M)) || (rc = keep_slot((int)e + 1))) return rc;
        }
        mpcqp_loop seg = loop_at(h, io, k0);
        if (ny) {                                   // (the estimator's loop reads and writes the tape's own copies)
            seg.Ap = T.Ap; seg.Bp = T.Bp; seg.C = T.C; seg.Lgain = T.Lg; seg.x_true = T.xt;
            seg.x_traj = T.xp + k0 * B * nx; seg.y_traj = T.ym + k0 * B * ny;
            if (mt) seg.Lgain = X.Lg + (size_t)(k / hold) * B * nx * ny;
        }
        h->loop_aff = at; h->loop_aff_k0 = k0;      // (null: the handle's own term stays in force)
        if ((rc = loop_run(h, 1, &seg, k == nsteps - 1))) return rc;
    }
    if (affine) h->tape_aff = F;
    if (ny && (get(h, io->x_traj, T.xp, ((size_t)nsteps + 1) * B * nx * db) || get(h, io->y_traj, T.ym, (size_t)nsteps * B * ny * db) ||
               get(h, io->x_true, T.xt, B * nx * db))) return MPCQP_ERR_HIP;
    h->tape_valid = true;
    return ny ? sync_unless_all_device(h, {io->x_traj, io->y_traj, io->x_true, io->C, io->Lgain, io->Ap, io->Bp}) : MPCQP_OK;      // (io->Lgain: the gain schedule where there is one)
}
extern "C" int mpcqp_rollout(mpcqp_handle *h, int nsteps, const mpcqp_loop *io) {
    if (!h || !io || nsteps < 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout: bad argument");
    if (io->ny > 0) return fail(MPCQP_ERR_UNSUPPORTED, "mpcqp_rollout: output feedback in a taped rollout is mpcqp_rollout_est (include/mpcqp_rollout_est.h)");
    return rollout_forward(h, nsteps, io, "mpcqp_rollout");
}
// ---- the taped rollout of the loop under a model schedule (include_ext/mpcqp_rollout_tv.h) ------------------------------------------
extern "C" int mpcqp_rollout_tv(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt) {
    if (!h || !io || nsteps < 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_tv: bad argument");
    if (!mt) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_tv: no model schedule given (mpcqp_rollout is the taped loop on one model)");
    return rollout_forward(h, nsteps, io, "mpcqp_rollout_tv", mt);
}
extern "C" int mpcqp_rollout_tv_tape_bytes(mpcqp_handle *h, int nsteps, int hold, int64_t *bytes) {
    if (!h || !bytes || nsteps < 1 || hold < 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_tv_tape_bytes: bad argument");
    *bytes = (int64_t)tape_carve(h->L, h->batch, nsteps, h->L.xref_rows, 0, nullptr, nullptr, (nsteps + hold - 1) / hold + 1, hold);
    return MPCQP_OK;
}
extern "C" int mpcqp_rollout_tv_get_slot(mpcqp_handle *h, int s, double *model, double *D, double *E, double *c) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    const int rc = tape_guard(h, "mpcqp_rollout_tv_get_slot", false, nullptr);
    if (rc) return rc;
    const RolloutSlots &V = h->tape_slots;
    if (V.nslots < 1) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_tv_get_slot: the tape is not one of mpcqp_rollout_tv (no model schedule, no slots)");
    if (s < 0 || s >= V.nslots) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_tv_get_slot: s must be in 0 .. nseg");
    HIPCHK(hipSetDevice(h->device));
    const Lay &L = h->L;
    const size_t B = (size_t)h->batch, sB = (size_t)s * B, db = sizeof(double);
    if (get(h, model, V.model + sB * L.model_sz, B * L.model_sz * db) || get(h, D, V.D + sB * L.n, B * L.n * db) ||
        get(h, E, V.E + sB * L.m, B * L.m * db) || get(h, c, V.c + sB, B * db)) return MPCQP_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}
// ---- the taped rollout with an affine term in the prediction model (include_ext5/mpcqp_rollout_affine.h) ----------------------------------
extern "C" int mpcqp_rollout_affine(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt, const mpcqp_affine_traj *at) {
    if (!h || !io || nsteps < 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine: bad argument");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_affine before mpcqp_setup");
    if (at && h->L.d_rows && h->L.d_rows != at->rows)
        return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine: the handle's term and the schedule's entries differ in their rows (the entries of a tape have one shape): set the term in the schedule's shape, or clear it");
    if (at) {                                       // (mpcqp_mpc_loop_affine's refusals, in its order: output feedback last)
        if (at->struct_size != (int32_t)sizeof(mpcqp_affine_traj)) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine: struct_size is not sizeof(mpcqp_affine_traj)");
        if (at->hold < 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine: hold must be >= 1");
        if (at->nentries < (nsteps + at->hold - 1) / at->hold) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine: fewer than ceil(nsteps / hold) entries");
        if (at->rows != 1 && at->rows != h->L.Np) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine: rows must be 1 or Np");
        if (!at->d) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine: no entries given (at == NULL runs the loop with the handle's own term)");
    }
    if (io->ny > 0) return fail(MPCQP_ERR_UNSUPPORTED, "mpcqp_rollout_affine: output feedback with an affine term is not implemented (the estimator's model has no offset)");
    return rollout_forward(h, nsteps, io, "mpcqp_rollout_affine", mt, false, nullptr, true, at);
}
extern "C" int mpcqp_rollout_affine_tape_bytes(mpcqp_handle *h, int nsteps, int model_hold, int d_hold, int rows, int64_t *bytes) {
    if (!h || !bytes || nsteps < 1 || model_hold < 0 || d_hold < 0) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine_tape_bytes: bad argument");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_affine_tape_bytes before mpcqp_setup");
    if (rows != 1 && rows != h->L.Np) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine_tape_bytes: rows must be 1 or Np");
    *bytes = (int64_t)tape_carve(h->L, h->batch, nsteps, h->L.xref_rows, 0, nullptr, nullptr, model_hold ? (nsteps + model_hold - 1) / model_hold + 1 : 0, model_hold,
                                 nullptr, nullptr, rollout_affine_nslots(nsteps, d_hold), rows, d_hold);
    return MPCQP_OK;
}
extern "C" int mpcqp_rollout_affine_get_slot(mpcqp_handle *h, int s, double *d) {
    if (!h || !d) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine_get_slot: null argument");
    const int rc = tape_guard(h, "mpcqp_rollout_affine_get_slot", false, nullptr);
    if (rc) return rc;
    const RolloutAffine &F = h->tape_aff;
    if (F.nslots < 1) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_affine_get_slot: the tape is not one of mpcqp_rollout_affine (no term slots)");
    if (s < 0 || s >= F.nslots) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine_get_slot: s must be in 0 .. nslots - 1");
    HIPCHK(hipSetDevice(h->device));
    const size_t per = (size_t)h->batch * (size_t)F.rows * h->L.nx;
    if (get(h, d, F.dval + (size_t)s * per, per * sizeof(double))) return MPCQP_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}
extern "C" int mpcqp_rollout_affine_get_tape(mpcqp_handle *h, int k, double *d) {
    if (!h || !d) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_affine_get_tape: null argument");
    const int rc = tape_guard(h, "mpcqp_rollout_affine_get_tape", false, &k);
    if (rc) return rc;
    const RolloutAffine &F = h->tape_aff;
    if (F.nslots < 1) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_affine_get_tape: the tape is not one of mpcqp_rollout_affine");
    HIPCHK(hipSetDevice(h->device));
    const Lay &L = h->L;
    const size_t B = (size_t)h->batch, w = sizeof(double) * (size_t)F.rows * L.nx;
    HIPCHK(hipMemcpy2DAsync(d, w, h->tape.step + (size_t)k * B * L.step_sz + L.od, sizeof(double) * (size_t)L.step_sz, w, B, hipMemcpyDefault, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}
// ---- the taped rollout of the output-feedback loop under a model schedule (include_ext2/mpcqp_rollout_tv_est.h) --------------------------
extern "C" int mpcqp_rollout_tv_est(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt, const mpcqp_est_traj *et) {
    if (!h || !io || !mt || nsteps < 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_tv_est: bad argument");
    return rollout_forward(h, nsteps, io, "mpcqp_rollout_tv_est", mt, true, et);
}
extern "C" int mpcqp_rollout_tv_est_tape_bytes(mpcqp_handle *h, int nsteps, int hold, int ny, int64_t *bytes) {
    if (!h || !bytes || nsteps < 1 || hold < 1 || ny < 1 || ny > 64) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_tv_est_tape_bytes: bad argument");
    *bytes = (int64_t)tape_carve(h->L, h->batch, nsteps, h->L.xref_rows, ny, nullptr, nullptr, (nsteps + hold - 1) / hold + 1, hold);
    return MPCQP_OK;
}
extern "C" int mpcqp_rollout_tv_est_get_gain(mpcqp_handle *h, int e, double *Lg) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    const int rc = tape_guard(h, "mpcqp_rollout_tv_est_get_gain", false, nullptr);
    if (rc) return rc;
    const RolloutGains &X = h->tape_gains;
    if (!X.Lg) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_tv_est_get_gain: the tape is not one of mpcqp_rollout_tv_est (no gain entries)");
    if (e < 0 || e >= h->tape_slots.nslots - 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_tv_est_get_gain: e must be in 0 .. nseg - 1");
    HIPCHK(hipSetDevice(h->device));
    const size_t per = (size_t)h->batch * h->L.nx * (size_t)h->tape_ny;
    if (get(h, Lg, X.Lg + (size_t)e * per, per * sizeof(double))) return MPCQP_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}
// ---- the taped rollout of the output-feedback loop (include/mpcqp_rollout_est.h) ---------------------------------------------------
extern "C" int mpcqp_rollout_est_tape_bytes(mpcqp_handle *h, int nsteps, int ny, int64_t *bytes) {
    if (!h || !bytes || nsteps < 1 || ny < 1 || ny > 64) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_est_tape_bytes: bad argument");
    *bytes = (int64_t)tape_carve(h->L, h->batch, nsteps, h->L.xref_rows, ny, nullptr, nullptr);
    return MPCQP_OK;
}
extern "C" int mpcqp_rollout_est(mpcqp_handle *h, int nsteps, const mpcqp_loop *io) {
    if (!h || !io || nsteps < 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_est: bad argument");
    if (io->ny == 0) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_est: ny must be > 0 (mpcqp_rollout is the taped loop without an estimator)");
    return rollout_forward(h, nsteps, io, "mpcqp_rollout_est");
}
extern "C" int mpcqp_rollout_get_tape_est(mpcqp_handle *h, int k, double *x_plant, double *y_meas) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    const int rc = tape_guard(h, "mpcqp_rollout_get_tape_est", true, &k);
    if (rc) return rc;
    const RolloutTape &T = h->tape;
    HIPCHK(hipSetDevice(h->device));
    const size_t B = (size_t)h->batch, kB = (size_t)k * B, db = sizeof(double);
    if (get(h, x_plant, T.xp + kB * h->L.nx, B * h->L.nx * db) || get(h, y_meas, T.ym + kB * (size_t)h->tape_ny, B * (size_t)h->tape_ny * db)) return MPCQP_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}
// A seed of the sweep into its place on the tape; one that is not given is zero.
static int put_seed(mpcqp_handle *h, double *dst, const double *src, size_t bytes) {
    if (src) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, h->stream));
    else HIPCHK(hipMemsetAsync(dst, 0, bytes, h->stream));
    return MPCQP_OK;
}
// eo: the estimator's seeds and gradients (mpcqp_rollout_adjoint_est), or null.  est: the call is mpcqp_rollout_adjoint_est.
// bo: the bound gradients (mpcqp_rollout_adjoint_bounds), or null.
// tv: the call is mpcqp_rollout_adjoint_tv; to: its per-slot outputs, or null.
// tve: the call is mpcqp_rollout_adjoint_tv_est (tv and est are set too); xo: its per-entry estimator outputs, or null.
// aff: the call is mpcqp_rollout_adjoint_affine (tv: it was given a `to`, as a scheduled tape needs); ao: the gradient of the terms per slot, or null.
static int rollout_sweep(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_rollout_est_io *eo, const mpcqp_adjoint_model_io *mo, bool est,
                         const mpcqp_adjoint_bounds_io *bo = nullptr, bool tv = false, const mpcqp_rollout_tv_io *to = nullptr,
                         bool tve = false, const mpcqp_rollout_tv_est_io *xo = nullptr, bool aff = false, const mpcqp_rollout_affine_io *ao = nullptr) {
    if (!h || !io) return fail(MPCQP_ERR_ARG, "null argument");
    if (ao && ao->struct_size != (int32_t)sizeof(mpcqp_rollout_affine_io)) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint_affine: struct_size is not sizeof(mpcqp_rollout_affine_io)");
    if (xo && xo->struct_size != (int32_t)sizeof(mpcqp_rollout_tv_est_io)) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint_tv_est: struct_size is not sizeof(mpcqp_rollout_tv_est_io)");
    if (tve && eo && (eo->d_L || eo->d_Ae || eo->d_Be))
        return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint_tv_est: d_L, d_Ae, d_Be are per entry under a schedule: ask for them in mpcqp_rollout_tv_est_io");
    if (to && to->struct_size != (int32_t)sizeof(mpcqp_rollout_tv_io)) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint_tv: struct_size is not sizeof(mpcqp_rollout_tv_io)");
    if (tv && (io->d_Ap || io->d_Bp || (mo && (mo->d_Ad || mo->d_Bd))))
        return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint_tv: d_Ap, d_Bp, d_Ad, d_Bd are per slot under a schedule: ask for them in mpcqp_rollout_tv_io");
    if (io->struct_size != (int32_t)sizeof(mpcqp_rollout_adjoint_io)) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint: struct_size is not sizeof(mpcqp_rollout_adjoint_io)");
    ModelOut m;                                     // (its refusals say mpcqp_rollout_adjoint on the _est path too)
    if (model_out(mo, "mpcqp_rollout_adjoint", &m)) return MPCQP_ERR_ARG;
    BoundsOut bd;
    if (bounds_out(bo, "mpcqp_rollout_adjoint_bounds", &bd)) return MPCQP_ERR_ARG;
    if (bo) {
        const bool other = io->lam || io->d_uminus1 || io->d_uref || io->d_xref || io->d_Ap || io->d_Bp || m.any ||
                           (eo && (eo->eta || eo->d_C || eo->d_L || eo->d_v || eo->d_Ae || eo->d_Be));
        if (!tv && !aff && !bd.any && !other) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint_bounds: no output asked for");
        if (bd.any && m.any && bd.batch_sum != m.batch_sum) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint_bounds: batch_sum of mo and of bo differ");
    }
    if (eo && eo->struct_size != (int32_t)sizeof(mpcqp_rollout_est_io)) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint_est: struct_size is not sizeof(mpcqp_rollout_est_io)");
    if (!est && !io->G_x && !io->G_u) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint: give G_x, G_u or both");
    if (est && !io->G_x && !io->G_u && !(eo && (eo->G_xhat || eo->G_y))) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint_est: give at least one of G_x, G_u, G_xhat, G_y");
    if (io->no_reuse != 0 && io->no_reuse != 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint: no_reuse is 0 or 1");
    if (m.batch_sum != 0 && m.batch_sum != 1) return fail(MPCQP_ERR_ARG, "mpcqp_rollout_adjoint: batch_sum is 0 or 1");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint before mpcqp_setup");
    const RolloutAffine &F = h->tape_aff;            // (nslots > 0: a tape of mpcqp_rollout_affine, which has every term it needs on it)
    const bool aff_tape = h->tape_buf && h->tape.nsteps >= 1 && F.nslots > 0;
    if (h->L.d_rows && !aff_tape && !aff) return fail(MPCQP_ERR_UNSUPPORTED, "mpcqp_rollout_adjoint: the handle has an affine term (include_ext4/mpcqp_affine.h: mpcqp_set_affine), which the taped rollouts and their reverse sweeps do not carry");
    if (!h->tape_buf || h->tape.nsteps < 1) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint: the handle holds no tape (call mpcqp_rollout first)");
    if (!h->tape_valid) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint: the model or the scaling the tape was made under has been replaced (mpcqp_setup*, mpcqp_update_model, mpcqp_update_vectors with l, u) or its rollout failed: roll out again");
    const RolloutSlots &V = h->tape_slots;
    const RolloutGains &X = h->tape_gains;
    if (!aff && aff_tape) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint: the tape is one of mpcqp_rollout_affine (an affine term in the prediction model); use mpcqp_rollout_adjoint_affine (include_ext5/mpcqp_rollout_affine.h)");
    if (aff && !aff_tape) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint_affine: the tape is not one of mpcqp_rollout_affine; use the sweep of the call that made it");
    if (aff && tv != (V.nslots > 0)) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint_affine: pass a mpcqp_rollout_tv_io exactly when the tape has a model schedule");
    if (!tve && X.Lg) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint: the tape is one of mpcqp_rollout_tv_est (an estimator under a model schedule); use mpcqp_rollout_adjoint_tv_est");
    if (tve && !X.Lg) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint_tv_est: the tape is not one of mpcqp_rollout_tv_est; use the sweep of the call that made it");
    if (!tv && V.nslots > 0) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint: the tape is one of mpcqp_rollout_tv (a model schedule); use mpcqp_rollout_adjoint_tv");
    if (tv && V.nslots < 1) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint_tv: the tape is not one of mpcqp_rollout_tv (no model schedule); use mpcqp_rollout_adjoint");
    if (est && h->tape_ny == 0) return fail(MPCQP_ERR_STATE, "mpcqp_rollout_adjoint_est: the tape is one of mpcqp_rollout (no estimator); use mpcqp_rollout_adjoint");
    HIPCHK(hipSetDevice(h->device));
    int rc = adjoint_alloc(h);
    if (rc) return rc;
    const RolloutTape &T = h->tape;
    KpolLaunch v = kpol_launch(h);
    Lay &G = v.G;
    G.raw = 0; G.xref_rows = h->tape_xref_rows;     // (the tape's entries, whatever the handle has been given since)
    G.d_rows = aff_tape ? F.rows : 0;               // (likewise the shape of their affine term: every entry reads its own, step + Lay::od)
    RolloutSweep W; memset(&W, 0, sizeof(W));
    adjoint_model_offsets(G, W.off);
    const size_t B = (size_t)h->batch, K = (size_t)T.nsteps, nx = G.nx, nu = G.nu, db = sizeof(double);
    if (adjoint_model_alloc(h, (size_t)W.off[ADJM_FIELDS])) return MPCQP_ERR_HIP;      // (the sweep writes its model terms there whether or not they are asked for)
    const size_t ny = (size_t)h->tape_ny;
    if (put_seed(h, T.gx, io->G_x, (K + 1) * B * nx * db) || put_seed(h, T.gu, io->G_u, K * B * nu * db)) return MPCQP_ERR_HIP;
    if (ny && (put_seed(h, T.gxh, eo ? eo->G_xhat : nullptr, (K + 1) * B * nx * db) || put_seed(h, T.gy, eo ? eo->G_y : nullptr, K * B * ny * db))) return MPCQP_ERR_HIP;
    AdjointArgs Q = adjoint_args(h);
    Q.nseeds = 1; Q.gw = nullptr; Q.gu0 = nullptr; Q.chain = 1; Q.ncol = 1; Q.cs = 0;
    const bool slot_model = tv && to && (to->d_Ad_slots || to->d_Bd_slots);      // (the Ad, Bd gradients of a scheduled tape are asked for in `to`, not in mo)
    W.mout = h->adjm_out; W.no_reuse = io->no_reuse; W.want_model = ((m.any || slot_model) ? ROLLOUT_WANT_MODEL : 0) | (bd.any ? ROLLOUT_WANT_BOUNDS : 0) |
                                                                      (aff && ao && ao->d_d_slots ? ROLLOUT_WANT_AFFINE : 0);
    const size_t with_carry = v.smem + db * (size_t)rollout_carry_doubles(G, (int)ny);
    W.carry_lds = with_carry <= 160 * 1024 ? 1 : 0;         // (lam, mu, g behind the common block, or in the tape's few doubles of global memory)
    const size_t smem = W.carry_lds ? with_carry : v.smem;
    if (tve) {
        DISPATCH_NB(G.NB, {
            if (set_smem(k_rollout_adjoint_tv_est<NB>, smem)) return MPCQP_ERR_HIP;
            hipLaunchKernelGGL(k_rollout_adjoint_tv_est<NB>, dim3(h->batch), dim3(NT), smem, h->stream, G, v.P, Q, T, W, V, X);
        });
    } else if (tv) {
        DISPATCH_NB(G.NB, {
            if (set_smem(k_rollout_adjoint_tv<NB>, smem)) return MPCQP_ERR_HIP;
            hipLaunchKernelGGL(k_rollout_adjoint_tv<NB>, dim3(h->batch), dim3(NT), smem, h->stream, G, v.P, Q, T, W, V);
        });
    } else {
        DISPATCH_NB(G.NB, {
            const auto kernel = ny ? k_rollout_adjoint_est<NB> : k_rollout_adjoint<NB>;      // (one sweep, with and without the estimator: mpcqp_rollout.h)
            if (set_smem(kernel, smem)) return MPCQP_ERR_HIP;
            hipLaunchKernelGGL(kernel, dim3(h->batch), dim3(NT), smem, h->stream, G, v.P, Q, T, W);
        });
    }
    HIPCHK(hipGetLastError());
    if (tv && to) {
        const size_t S = (size_t)V.nslots;
        if (get(h, to->d_Ad_slots, V.dAd, S * B * nx * nx * db) || get(h, to->d_Bd_slots, V.dBd, S * B * nx * nu * db) ||
            get(h, to->d_Ap_entries, V.dAp, (S - 1) * B * nx * nx * db) || get(h, to->d_Bp_entries, V.dBp, (S - 1) * B * nx * nu * db)) return MPCQP_ERR_HIP;
    }
    if (aff && ao && get(h, ao->d_d_slots, F.dgrad, (size_t)F.nslots * B * (size_t)F.rows * nx * db)) return MPCQP_ERR_HIP;
    if (tve && xo) {
        const size_t S1 = (size_t)V.nslots - 1;
        if (get(h, xo->d_Ae_entries, X.dAe, S1 * B * nx * nx * db) || get(h, xo->d_Be_entries, X.dBe, S1 * B * nx * nu * db) ||
            get(h, xo->d_L_entries, X.dL, S1 * B * nx * ny * db)) return MPCQP_ERR_HIP;
    }
    const size_t xw = (size_t)G.xref_rows * nx;
    if (get(h, io->lam, T.lam, (K + 1) * B * nx * db) || get(h, io->d_uminus1, T.dum1, B * nu * db) || get(h, io->d_uref, T.duref, B * nu * db) ||
        get(h, io->d_xref, T.dxref, K * B * xw * db) || get(h, io->d_Ap, T.dAp, B * nx * nx * db) || get(h, io->d_Bp, T.dBp, B * nx * nu * db)) return MPCQP_ERR_HIP;
    if (ny && eo && (get(h, eo->eta, T.eta, (K + 1) * B * nx * db) || get(h, eo->d_v, T.dv, K * B * ny * db) || get(h, eo->d_C, T.dC, B * ny * nx * db) ||
                     get(h, eo->d_L, T.dL, B * nx * ny * db) || get(h, eo->d_Ae, T.dAe, B * nx * nx * db) || get(h, eo->d_Be, T.dBe, B * nx * nu * db))) return MPCQP_ERR_HIP;
    if (m.any) {
        if (m.batch_sum) { launch_adjoint_model_sum(h, W.off); HIPCHK(hipGetLastError()); }
        if (get_model_out(h, m, W.off)) return MPCQP_ERR_HIP;
    }
    if (bd.any && get_bounds_out(h, bd)) return MPCQP_ERR_HIP;
    if (any_host(bd)) HIPCHK(hipStreamSynchronize(h->stream));
    return sync_unless_all_device(h, {io->G_x, io->G_u, io->lam, io->d_uminus1, io->d_uref, io->d_xref, io->d_Ap, io->d_Bp,
                                      eo ? eo->G_xhat : nullptr, eo ? eo->G_y : nullptr, eo ? eo->eta : nullptr, eo ? eo->d_C : nullptr, eo ? eo->d_L : nullptr,
                                      eo ? eo->d_v : nullptr, eo ? eo->d_Ae : nullptr, eo ? eo->d_Be : nullptr,
                                      to ? to->d_Ad_slots : nullptr, to ? to->d_Bd_slots : nullptr, to ? to->d_Ap_entries : nullptr, to ? to->d_Bp_entries : nullptr,
                                      xo ? xo->d_Ae_entries : nullptr, xo ? xo->d_Be_entries : nullptr, xo ? xo->d_L_entries : nullptr,
                                      ao ? ao->d_d_slots : nullptr}, &m);
}
extern "C" int mpcqp_rollout_adjoint_tv(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_adjoint_model_io *mo,
                                        const mpcqp_adjoint_bounds_io *bo, const mpcqp_rollout_tv_io *to) {
    return rollout_sweep(h, io, nullptr, mo, false, bo, true, to);
}
extern "C" int mpcqp_rollout_adjoint_tv_est(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_rollout_est_io *eo, const mpcqp_adjoint_model_io *mo,
                                            const mpcqp_adjoint_bounds_io *bo, const mpcqp_rollout_tv_io *to, const mpcqp_rollout_tv_est_io *xo) {
    return rollout_sweep(h, io, eo, mo, true, bo, true, to, true, xo);
}
extern "C" int mpcqp_rollout_adjoint_affine(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_adjoint_model_io *mo,
                                            const mpcqp_adjoint_bounds_io *bo, const mpcqp_rollout_tv_io *to, const mpcqp_rollout_affine_io *ao) {
    return rollout_sweep(h, io, nullptr, mo, false, bo, to != nullptr, to, false, nullptr, true, ao);
}
extern "C" int mpcqp_rollout_adjoint(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_adjoint_model_io *mo) {
    return rollout_sweep(h, io, nullptr, mo, false);
}
extern "C" int mpcqp_rollout_adjoint_est(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_rollout_est_io *eo, const mpcqp_adjoint_model_io *mo) {
    return rollout_sweep(h, io, eo, mo, true);
}
extern "C" int mpcqp_rollout_adjoint_bounds(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_rollout_est_io *eo,
                                            const mpcqp_adjoint_model_io *mo, const mpcqp_adjoint_bounds_io *bo) {
    return rollout_sweep(h, io, eo, mo, eo != nullptr, bo);
}
extern "C" int mpcqp_get_rollout_info(mpcqp_handle *h, int32_t *n_active, int32_t *n_weak, int32_t *status, int32_t *n_factor) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    const int rc = tape_guard(h, "mpcqp_get_rollout_info", false, nullptr);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const RolloutTape &T = h->tape;
    const size_t kb = sizeof(int32_t) * (size_t)T.nsteps * (size_t)h->batch;
    if (get(h, n_active, T.nact, kb) || get(h, n_weak, T.nweak, kb) || get(h, status, T.st, kb) ||
        get(h, n_factor, T.nfactor, sizeof(int32_t) * (size_t)h->batch)) return MPCQP_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}
extern "C" int mpcqp_rollout_get_tape(mpcqp_handle *h, int k, double *x, double *z, double *y, double *step, int32_t *status) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    const int rc = tape_guard(h, "mpcqp_rollout_get_tape", false, &k);
    if (rc) return rc;
    const RolloutTape &T = h->tape;
    HIPCHK(hipSetDevice(h->device));
    const Lay &L = h->L;
    const size_t B = (size_t)h->batch, kB = (size_t)k * B, db = sizeof(double);
    if (get(h, x, T.x + kB * L.n, B * L.n * db) || get(h, z, T.z + kB * L.m, B * L.m * db) || get(h, y, T.y + kB * L.m, B * L.m * db) ||
        get(h, status, T.status + kB, B * sizeof(int32_t))) return MPCQP_ERR_HIP;
    if (step) {
        const size_t w = db * (size_t)(L.nx + L.nu + h->tape_xref_rows * L.nx);
        HIPCHK(hipMemcpy2DAsync(step, w, T.step + kB * L.step_sz, db * (size_t)L.step_sz, w, B, hipMemcpyDefault, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}


extern "C" int mpcqp_mpc_run(mpcqp_handle *h, int nsteps, const double *w, const double *Ap, const double *Bp,
                             double *x_traj, double *u_traj, int32_t *status_traj, int32_t *iter_traj) {
    mpcqp_loop io; memset(&io, 0, sizeof(io));
    io.w = w; io.Ap = Ap; io.Bp = Bp; io.x_traj = x_traj; io.u_traj = u_traj; io.status_traj = status_traj; io.iter_traj = iter_traj;
    return mpcqp_mpc_loop(h, nsteps, &io);
}

// The equality-constrained QP of the handle's problem (dynamics rows only) by at most `sweeps` multiplier sweeps in residual form, see k_eq_solve.
extern "C" int mpcqp_eq_solve(mpcqp_handle *h, int sweeps, int cold, double tol, double *res) {
    if (!h || sweeps < 0) return fail(MPCQP_ERR_ARG, "mpcqp_eq_solve: bad argument");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_eq_solve before mpcqp_setup");
    HIPCHK(hipSetDevice(h->device));
    double *dres = nullptr;
    Scratch sc;
    HIPCHK(sc.get(&dres, (size_t)h->batch * 5));
    DISPATCH_NB(h->L.NB, {
        if (set_smem(k_eq_solve<NB>, h->smem)) return MPCQP_ERR_HIP;
        hipLaunchKernelGGL(k_eq_solve<NB>, dim3(h->batch), dim3(NT), h->smem, h->stream, h->L, h->P, sweeps, cold, tol, dres);
    });
    HIPCHK(hipGetLastError());
    if (h->pq.status) HIPCHK(hipMemsetAsync(h->pq.status, 0, sizeof(int) * (size_t)h->batch, h->stream));      // (the polish setting is ignored here)
    h->has_solve = true; h->um1_moved = false;
    if (res) HIPCHK(hipMemcpyAsync(res, dres, sizeof(double) * 5 * (size_t)h->batch, hipMemcpyDefault, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

extern "C" int mpcqp_get_solution(mpcqp_handle *h, double *x, double *y, mpcqp_info *info) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    size_t B = (size_t)h->batch;
    if (get(h, x, h->P.xo, B * h->L.n * sizeof(double)) || get(h, y, h->P.yo, B * h->L.m * sizeof(double)) ||
        get(h, info, h->P.info, B * sizeof(mpcqp_info))) return MPCQP_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

extern "C" int mpcqp_get_u0(mpcqp_handle *h, double *u0) {
    if (!h || !u0) return fail(MPCQP_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    int tot = h->batch * h->L.nu;
    hipLaunchKernelGGL(k_gather_u0, dim3((tot + 255) / 256), dim3(256), 0, h->stream, h->L, h->P.xo, h->u0_dev, h->batch);
    HIPCHK(hipGetLastError());
    if (get(h, u0, h->u0_dev, sizeof(double) * (size_t)tot)) return MPCQP_ERR_HIP;
    const bool due = balance_due(h);
    if (!due && is_device_ptr(u0)) return MPCQP_OK;           // device destination: stream-ordered, no need to wait
    HIPCHK(hipStreamSynchronize(h->stream));
    return due ? rebalance(h) : MPCQP_OK;
}

extern "C" int mpcqp_mpc_step(mpcqp_handle *h, const double *x0, const double *uminus1, const double *xref, int xref_rows, double *u_out) {
    if (!h || !x0 || !u_out) return fail(MPCQP_ERR_ARG, "mpcqp_mpc_step: null argument");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_mpc_step before mpcqp_setup");
    if (h->step_blank && (!uminus1 || !xref)) return fail(MPCQP_ERR_STATE, "mpcqp_mpc_step: the handle was set up from raw q, l, u and holds no u_{-1} / xref yet: give them");
    HIPCHK(hipSetDevice(h->device));
    h->step_blank = false;
    h->L.raw = 0;
    int rc = step_upload(h, x0, uminus1, xref, xref_rows);
    if (rc) return rc;
    if ((rc = launch_solve(h, 0))) return rc;
    if ((rc = after_solve(h))) return rc;
    const int tot = h->batch * h->L.nu;
    hipLaunchKernelGGL(k_output_u, dim3((tot + 255) / 256), dim3(256), 0, h->stream, h->L, h->P, h->u0_dev, h->batch, 1, h->um1_used);
    HIPCHK(hipGetLastError());
    h->um1_moved = true;                            // (the step data now hold the NEXT u_{-1}; this solve's is in um1_used)
    if (get(h, u_out, h->u0_dev, sizeof(double) * (size_t)tot)) return MPCQP_ERR_HIP;
    const bool due = balance_due(h);
    if (!due && is_device_ptr(u_out)) return MPCQP_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    return due ? rebalance(h) : MPCQP_OK;
}

// One control step with HOST data and the lowest latency the library can offer (the drop-in class's update(): mpc.py:338-375
// = prob.update(l, u, q) + prob.solve() + reading res.x): x0 / u_{-1} / xref are placed in mapped host memory the kernel reads
// itself, the solution comes back the same way, and the call waits on a flag in that memory -- ONE kernel launch, no copy calls, no
// stream synchronisation.  Falls back to mpcqp_update + mpcqp_solve + mpcqp_get_solution where the batch is solved in two launches.
static int ensure_pinned(mpcqp_handle *h) {
    if (h->pin_tried) return h->pin_in && h->pin_out ? 0 : 1;
    h->pin_tried = true;
    const Lay &L = h->L; const size_t B = (size_t)h->batch;
    h->pin_stride = L.nx + L.nu + L.N * L.nx;
    const size_t in_bytes = sizeof(double) * B * h->pin_stride, out_bytes = sizeof(double) * B * (L.n + L.m) + sizeof(mpcqp_info) * B + 64;
    const unsigned flags = hipHostMallocMapped | hipHostMallocCoherent;
    if (hipHostMalloc((void **)&h->pin_in, in_bytes, flags) != hipSuccess) { h->pin_in = nullptr; (void)hipGetLastError(); return 1; }
    if (hipHostMalloc((void **)&h->pin_out, out_bytes, flags) != hipSuccess) { hipHostFree(h->pin_in); h->pin_in = h->pin_out = nullptr; (void)hipGetLastError(); return 1; }
    memset(h->pin_out, 0, out_bytes);
    if (hipHostGetDevicePointer(&h->pin_in_dev, h->pin_in, 0) != hipSuccess || hipHostGetDevicePointer(&h->pin_out_dev, h->pin_out, 0) != hipSuccess) {
        hipHostFree(h->pin_in); hipHostFree(h->pin_out); h->pin_in = h->pin_out = nullptr; (void)hipGetLastError(); return 1;
    }
    return 0;
}

extern "C" int mpcqp_step_host(mpcqp_handle *h, const double *x0, const double *uminus1, const double *xref, int xref_rows,
                               double *x, double *y, mpcqp_info *info) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "mpcqp_step_host before mpcqp_setup");
    if (xref && xref_rows != 1 && xref_rows != h->L.N) return fail(MPCQP_ERR_ARG, "xref_rows must be 1 or Np+1");
    if (h->step_blank && (!x0 || !uminus1 || !xref)) return fail(MPCQP_ERR_STATE, "mpcqp_step_host: the handle was set up from raw q, l, u and holds no x0 / u_{-1} / xref yet: give all three");
    HIPCHK(hipSetDevice(h->device));
    const bool split = h->auto_balance && h->ncu > 0 && h->batch > h->ncu;
    if (split || ensure_pinned(h)) {
        int rc = mpcqp_update(h, x0, uminus1, xref, xref_rows);      // (clears step_blank once the step data is in)
        if (rc) return rc;
        if ((rc = mpcqp_solve(h))) return rc;
        return mpcqp_get_solution(h, x, y, info);
    }
    const Lay &L = h->L; const size_t B = (size_t)h->batch;
    h->L.raw = 0;
    if (xref) h->L.xref_rows = xref_rows;
    const int nxr = xref ? xref_rows * L.nx : 0;
    const bool inl = B == 1 && x0 && uminus1 && xref && L.nx + L.nu + nxr <= 32;      // (a single controller's few doubles travel in the kernel arguments instead)
    for (size_t b = 0; b < B && !inl; ++b) {
        double *dst = h->pin_in + b * h->pin_stride;
        if (x0) memcpy(dst, x0 + b * L.nx, sizeof(double) * L.nx);
        if (uminus1) memcpy(dst + L.nx, uminus1 + b * L.nu, sizeof(double) * L.nu);
        if (xref) memcpy(dst + L.nx + L.nu, xref + b * nxr, sizeof(double) * nxr);
    }
    RunArgs R; memset(&R, 0, sizeof(R));
    if (inl) {
        memcpy(R.inl, x0, sizeof(double) * L.nx); memcpy(R.inl + L.nx, uminus1, sizeof(double) * L.nu); memcpy(R.inl + L.nx + L.nu, xref, sizeof(double) * nxr);
        R.inl_n = L.nx + L.nu + nxr;
    }
    R.pin_in = (!inl && (x0 || uminus1 || xref)) ? (const double *)h->pin_in_dev : nullptr;
    R.pin_stride = h->pin_stride; R.pin_mask = (x0 ? 1 : 0) | (uminus1 ? 2 : 0) | (xref ? 4 : 0); R.pin_xref = nxr;
    R.pub = (double *)h->pin_out_dev; R.done = (unsigned *)h->npending_dev + 2; R.seq = ++h->host_seq;
    if (h->pq.status && !h->pol.polish) HIPCHK(hipMemsetAsync(h->pq.status, 0, sizeof(int) * B, h->stream));
    if (h->pol.polish) R.pub = nullptr;                        // (polishing: the second launch, k_polish, publishes the results and raises the flag)
    int rc = launch_run(h, R, 0);
    if (!rc && h->pol.polish) rc = launch_polish(h, (double *)h->pin_out_dev, (unsigned *)h->npending_dev + 2, h->host_seq);
    if (rc) return rc;
    h->step_blank = false;                                     // the step data has been accepted (a failed launch leaves the handle demanding it again)
    volatile unsigned long long *flag = (volatile unsigned long long *)((char *)h->pin_out + sizeof(double) * B * (L.n + L.m) + sizeof(mpcqp_info) * B);
    // Poll the flag: a short busy wait (a small solve is done within tens of microseconds), then yield the core between polls -- a long
    // solve (iteration limit, a long horizon) does not keep a CPU core spinning.
    for (unsigned long long spins = 0; *flag != h->host_seq; ++spins) {
        if (spins < 20000) cpu_relax(); else sched_yield();
        if ((spins & 0xfffff) == 0xfffff) {                    // every ~million polls: has the stream died?
            hipError_t e = hipStreamQuery(h->stream);
            if (e != hipSuccess && e != hipErrorNotReady) return fail(MPCQP_ERR_HIP, std::string("mpcqp_step_host: ") + hipGetErrorString(e));
            if (e == hipSuccess && *flag != h->host_seq) { HIPCHK(hipStreamSynchronize(h->stream)); break; }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (x) memcpy(x, h->pin_out, sizeof(double) * B * L.n);
    if (y) memcpy(y, h->pin_out + B * L.n, sizeof(double) * B * L.m);
    if (info) memcpy(info, h->pin_out + B * (L.n + L.m), sizeof(mpcqp_info) * B);
    return MPCQP_OK;
}

// Development and tests, not part of the C ABI of include/mpcqp.h (the CPU twin does not have it): the closed loop's carry inside the latency round
// since creation / the last reset of mpcqp_get_stats -- out3 = { steps whose transition the round made itself, of those the steps handed back to the
// kernel's begin because a constraint type changed, queue-item parts per instance of the last persistent closed-loop launch (0 = not persistent) }.
extern "C" int mpcqp_dev_carry_stats(mpcqp_handle *h, uint64_t *out3) {
    if (!h || !out3) return fail(MPCQP_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out3, h->P.stats + 8, 2 * sizeof(uint64_t), hipMemcpyDefault, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    out3[2] = (uint64_t)h->loop_parts;
    return MPCQP_OK;
}

extern "C" int mpcqp_get_stats(mpcqp_handle *h, uint64_t *out4, int reset) {
    if (!h || !out4) return fail(MPCQP_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out4, h->P.stats, 4 * sizeof(uint64_t), hipMemcpyDefault, h->stream));
#ifdef MPCQP_RUN_TIMING
    { uint64_t t[4]; hipMemcpy(t, h->P.stats + 4, sizeof(t), hipMemcpyDeviceToHost); fprintf(stderr, "phase wall-clock ticks: begin %llu admm %llu check %llu body %llu\n", (unsigned long long)t[0], (unsigned long long)t[1], (unsigned long long)t[2], (unsigned long long)t[3]);
      unsigned long long g[16]; hipMemcpyFromSymbol(g, HIP_SYMBOL(g_ticks), sizeof(g)); unsigned long long z[16] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_ticks), z, sizeof(z));
      unsigned long long gw[48]; hipMemcpyFromSymbol(gw, HIP_SYMBOL(g_wticks), sizeof(gw)); unsigned long long zw[48] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_wticks), zw, sizeof(zw));
      unsigned long long gb[128]; hipMemcpyFromSymbol(gb, HIP_SYMBOL(g_bticks), sizeof(gb)); unsigned long long zb[128] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_bticks), zb, sizeof(zb));
      if (h->L.nw == 8) mpcqp_w8_ticks(g, gw, gb);      // (the 512-thread kernels count in their own translation unit)
      // the boundary between two rounds of the latency round, section by section (mpcqp_layout.h: BTICK): one group per section, one number per wave
      { char line[2048]; int n = snprintf(line, sizeof line, "boundary cycles (lane 0 of each wave, summed over rounds):");
        for (int k = 0; k < 10; ++k) { n += snprintf(line + n, sizeof line - n, " s%d", k); for (int w = 0; w < 8; ++w) n += snprintf(line + n, sizeof line - n, " %llu", gb[8 * k + w]); }
        fprintf(stderr, "%s\n", line); }
      // the latency round's barriers as every wave's lane 0 reaches them (mpcqp_layout.h: WTICK): one group per barrier, one number per wave
      { char line[1024]; int n = snprintf(line, sizeof line, "wave barrier cycles (lane 0 of each wave, summed over iterations):");
        for (int k = 0; k < 5; ++k) { n += snprintf(line + n, sizeof line - n, " b%d", k); for (int w = 0; w < 8; ++w) n += snprintf(line + n, sizeof line - n, " %llu", gw[8 * k + w]); }
        fprintf(stderr, "%s\n", line); }
      { double tot = 0; for (int i = 0; i < 7; ++i) tot += (double)g[i]; if (tot <= 0) tot = 1;
        fprintf(stderr, "iteration cycles (thread 0, summed over workgroups): rhs %.1f%% fwd %.1f%% middle %.1f%% bwd %.1f%% t4 %.1f%% t5 %.1f%% t6 %.1f%% total %.3g;  outside the iterations (same unit): t7 %.3g t8 %.3g t9 %.3g;  check: setup+tail %.3g rows %.3g vars %.3g reduce %.3g decide %.3g\n",
                100 * g[0] / tot, 100 * g[1] / tot, 100 * g[2] / tot, 100 * g[3] / tot, 100 * g[4] / tot, 100 * g[5] / tot, 100 * g[6] / tot, tot, (double)g[7], (double)g[8], (double)g[9], (double)g[10], (double)g[11], (double)g[12], (double)g[13], (double)g[14]); } }
#endif
    if (reset) HIPCHK(hipMemsetAsync(h->P.stats, 0, 10 * sizeof(uint64_t), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

extern "C" int mpcqp_get_launch_times(mpcqp_handle *h, uint64_t *out, int nsteps) {
    if (!h || !out || nsteps < 0 || nsteps > TS_STEPS) return fail(MPCQP_ERR_ARG, "mpcqp_get_launch_times: bad argument (0 <= nsteps <= 64)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy2DAsync(out, sizeof(uint64_t) * (size_t)(2 + nsteps), h->P.tstamp, sizeof(uint64_t) * (size_t)TS_STRIDE, sizeof(uint64_t) * (size_t)(2 + nsteps),
                            (size_t)h->batch, hipMemcpyDefault, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

extern "C" int mpcqp_profile(mpcqp_handle *h, int enable, double *run_ms, int64_t *run_launches, int reset) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    int rc = drain_events(h);
    if (rc) return rc;
    if (enable >= 0) h->profiling = enable != 0;
    if (run_ms) *run_ms = h->run_ms;
    if (run_launches) *run_launches = h->run_launches;
    if (reset) { h->run_ms = 0.0; h->run_launches = 0; }
    return MPCQP_OK;
}

extern "C" int mpcqp_get_shape(mpcqp_handle *h, int *nx, int *nu, int *Np, int *Nc) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (nx) *nx = h->L.nx;
    if (nu) *nu = h->L.nu;
    if (Np) *Np = h->L.Np;
    if (Nc) *Nc = h->L.Nc;
    return MPCQP_OK;
}

// Arithmetic on the handle's plan: mpcqp_plan.h says what each figure counts.
extern "C" int mpcqp_get_dims(mpcqp_handle *h, int *n, int *m, int64_t *factor_doubles, int64_t *nnzL) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    plan_dims(*h, n, m, factor_doubles, nnzL);
    return MPCQP_OK;
}

extern "C" int mpcqp_get_stream_bytes(mpcqp_handle *h, int64_t *per_iter, int64_t *per_round, int64_t *per_solve) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    plan_stream_bytes(*h, per_iter, per_round, per_solve);
    return MPCQP_OK;
}

extern "C" int mpcqp_get_work(mpcqp_handle *h, int64_t *mfma_per_iter) {
    if (!h || !mfma_per_iter) return fail(MPCQP_ERR_ARG, "null argument");
    *mfma_per_iter = plan_mfma_per_iter(*h);
    return MPCQP_OK;
}

extern "C" int mpcqp_get_occupancy(mpcqp_handle *h, int *workgroups_per_cu, int *compute_units, int *threads_per_workgroup) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (workgroups_per_cu) *workgroups_per_cu = plan_occupancy(*h);
    if (compute_units) *compute_units = h->ncu;
    if (threads_per_workgroup) *threads_per_workgroup = plan_threads(*h);
    return MPCQP_OK;
}

// Name of the k_mpc_run instantiation the handle's solves (loop = 0) or closed-loop runs (loop = 1) launch: the id launch_run dispatches on.
extern "C" int mpcqp_kernel_name(mpcqp_handle *h, int loop, char *buf, int buflen) {
    if (!h || !buf || buflen < 1) return fail(MPCQP_ERR_ARG, "null argument");
    run_kernel_name(h->kernel, loop != 0, buf, (size_t)buflen);
    return MPCQP_OK;
}

extern "C" int mpcqp_warm_start(mpcqp_handle *h, const double *x, const double *y) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "warm_start before setup");
    HIPCHK(hipSetDevice(h->device));
    size_t B = (size_t)h->batch;
    if (x || y) h->has_solve = false;               // (the iterate mpcqp_adjoint takes its active set from is replaced)
    if (x) { HIPCHK(hipMemcpyAsync(h->P.x, x, B * h->L.n * sizeof(double), hipMemcpyDefault, h->stream)); h->warm_x_pending = true; }
    if (y) { HIPCHK(hipMemcpyAsync(h->P.y, y, B * h->L.m * sizeof(double), hipMemcpyDefault, h->stream)); }
    return MPCQP_OK;
}

extern "C" int mpcqp_export_qp(mpcqp_handle *h, double *Pm, double *Am, double *q, double *l, double *u) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "export before setup");
    HIPCHK(hipSetDevice(h->device));
    const Lay &L = h->L; size_t B = (size_t)h->batch;
    double *dP = nullptr, *dA = nullptr, *dq = nullptr, *dl = nullptr, *du = nullptr;
    Scratch sc;
    if (Pm) { HIPCHK(sc.get(&dP, B * L.n * L.n)); HIPCHK(hipMemsetAsync(dP, 0, B * L.n * L.n * sizeof(double), h->stream)); }
    if (Am) { HIPCHK(sc.get(&dA, B * L.m * L.n)); HIPCHK(hipMemsetAsync(dA, 0, B * L.m * L.n * sizeof(double), h->stream)); }
    if (q) HIPCHK(sc.get(&dq, B * L.n));
    if (l && u) { HIPCHK(sc.get(&dl, B * L.m)); HIPCHK(sc.get(&du, B * L.m)); }
    DISPATCH_NB(L.NB, {
        if (set_smem(k_export<NB>, h->smem)) return MPCQP_ERR_HIP;
        hipLaunchKernelGGL(k_export<NB>, dim3(h->batch), dim3(NT), h->smem, h->stream, h->L, h->P, dP, dA, dq, dl, du);
    });
    HIPCHK(hipGetLastError());
    int rc = 0;
    rc |= get(h, Pm, dP, B * L.n * L.n * sizeof(double)); rc |= get(h, Am, dA, B * L.m * L.n * sizeof(double));
    rc |= get(h, q, dq, B * L.n * sizeof(double));
    if (l && u) { rc |= get(h, l, dl, B * L.m * sizeof(double)); rc |= get(h, u, du, B * L.m * sizeof(double)); }
    HIPCHK(hipStreamSynchronize(h->stream));
    return rc ? MPCQP_ERR_HIP : MPCQP_OK;
}

extern "C" int mpcqp_get_scaling(mpcqp_handle *h, double *D, double *E, double *c, double *rho) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    size_t B = (size_t)h->batch;
    if (get(h, D, h->P.D, B * h->L.n * sizeof(double)) || get(h, E, h->P.E, B * h->L.m * sizeof(double)) ||
        get(h, c, h->P.c, B * sizeof(double)) || get(h, rho, h->P.rho, B * sizeof(double))) return MPCQP_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

extern "C" int mpcqp_get_iterate(mpcqp_handle *h, double *x, double *z, double *y) {
    if (!h) return fail(MPCQP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    size_t B = (size_t)h->batch;
    if (get(h, x, h->P.x, B * h->L.n * sizeof(double)) || get(h, z, h->P.z, B * h->L.m * sizeof(double)) ||
        get(h, y, h->P.y, B * h->L.m * sizeof(double))) return MPCQP_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

extern "C" int mpcqp_debug_kkt_solve(mpcqp_handle *h, const double *rhs, double *sol) {
    if (!h || !rhs || !sol) return fail(MPCQP_ERR_ARG, "null argument");
    if (!h->is_setup) return fail(MPCQP_ERR_STATE, "kkt_solve before setup");
    HIPCHK(hipSetDevice(h->device));
    const Lay &L = h->L; size_t bytes = (size_t)h->batch * L.n * sizeof(double);
    double *dr = nullptr, *ds = nullptr;
    Scratch sc;
    HIPCHK(sc.get(&dr, (size_t)h->batch * L.n)); HIPCHK(sc.get(&ds, (size_t)h->batch * L.n));
    HIPCHK(hipMemcpyAsync(dr, rhs, bytes, hipMemcpyDefault, h->stream));
    DISPATCH_NB(L.NB, {
        if (set_smem(k_kkt_solve<NB>, h->smem)) return MPCQP_ERR_HIP;
        hipLaunchKernelGGL(k_kkt_solve<NB>, dim3(h->batch), dim3(NT), h->smem, h->stream, h->L, h->P, dr, ds);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sol, ds, bytes, hipMemcpyDefault, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}
