// mpcqp_riccati.hip -- third translation unit of libmpcqp_hip.so: batched discrete algebraic Riccati equations and their adjoint
// (include/mpcqp_riccati.h), and the Riccati difference equation with its adjoint (include_ext3/mpcqp_riccati_traj.h; device code:
// mpcqp_riccati_traj.h, k_dre<NB> / k_dre_adjoint<NB>, at the end of this file).  A unit of its own so that mpcqp.hip and mpcqp_w8.hip compile exactly as they did without it.  The calls take
// no handle; device code: mpcqp_riccati.h.  Host side: argument checks, one staging block for whatever pointers are in host memory, one
// kernel launch (k_dare<NB> / k_dare_adjoint<NB>, NB = 16 or 32 by max(n, m)), one workgroup per instance.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/mpcqp_riccati.h"
#include "../../include_ext3/mpcqp_riccati_traj.h"

#include "mpcqp_riccati.h"
#include "mpcqp_riccati_traj.h"

int mpcqp_set_error(int code, const char *msg);          // mpcqp.hip: what mpcqp_last_error returns

static int ric_fail(int code, const std::string &msg) { return mpcqp_set_error(code, msg.c_str()); }
#define RIC_HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    return ric_fail(MPCQP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

extern "C" void mpcqp_riccati_default_settings(mpcqp_riccati_settings *s) {
    if (!s) return;
    s->struct_size = (int32_t)sizeof(mpcqp_riccati_settings);
    s->max_iter = 50;
    s->gain_form = 0;
    s->reserved = 0;
    s->tol = 1e-15;
}

namespace {

bool on_device(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice;
}

// The arrays of one call.  Those in host memory get a place in ONE device block (inputs copied in before the launch, outputs copied back
// after it, then the call waits and frees the block); those in device memory are used where they are.
struct Staging {
    struct Item { void **slot; size_t bytes; bool out; void *host; };
    std::vector<Item> items;
    char *block = nullptr;
    int prev_device = -1;
    ~Staging() { if (block) (void)hipFree(block); if (prev_device >= 0) (void)hipSetDevice(prev_device); }
    template <class T> void in(const T **slot, size_t count) { items.push_back({(void **)slot, count * sizeof(T), false, nullptr}); }
    template <class T> void out(T **slot, size_t count) { items.push_back({(void **)slot, count * sizeof(T), true, nullptr}); }
    static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
    hipError_t begin(hipStream_t st) {
        size_t total = 0;
        for (Item &it : items) if (*it.slot && !on_device(*it.slot)) { it.host = *it.slot; total += pad(it.bytes); }
        if (total == 0) return hipSuccess;
        hipError_t e = hipMalloc((void **)&block, total);
        if (e != hipSuccess) return e;
        size_t off = 0;
        for (Item &it : items) if (it.host) {
            *it.slot = block + off;
            off += pad(it.bytes);
            if (!it.out && (e = hipMemcpyAsync(*it.slot, it.host, it.bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        }
        return hipSuccess;
    }
    hipError_t end(hipStream_t st) {
        if (!block) return hipSuccess;
        hipError_t e;
        for (Item &it : items) if (it.host && it.out && (e = hipMemcpyAsync(it.host, *it.slot, it.bytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        return hipStreamSynchronize(st);
    }
};

int check_sizes(const char *fn, int batch, int n, int m, const mpcqp_riccati_settings *s, mpcqp_riccati_settings *use) {
    const std::string f(fn);
    if (batch < 1 || n < 1 || m < 1) return ric_fail(MPCQP_ERR_ARG, f + ": batch, n and m must be at least 1");
    if (n > 32 || m > 32) return ric_fail(MPCQP_ERR_UNSUPPORTED, f + ": n > 32 or m > 32 is not implemented (an instance lives in one workgroup's LDS)");
    mpcqp_riccati_default_settings(use);
    if (s) {
        if (s->struct_size != (int32_t)sizeof(mpcqp_riccati_settings)) return ric_fail(MPCQP_ERR_ARG, f + ": mpcqp_riccati_settings.struct_size is not sizeof(mpcqp_riccati_settings)");
        *use = *s;
    }
    if (use->max_iter < 1 || !(use->tol >= 0.0) || (use->gain_form != 0 && use->gain_form != 1))
        return ric_fail(MPCQP_ERR_ARG, f + ": max_iter must be >= 1, tol >= 0 and gain_form 0 or 1");
    return MPCQP_OK;
}

// make `device` the current one for the rest of the call (the Staging's destructor puts the previous one back)
int enter_device(const char *fn, int device, Staging *sg) {
    const std::string f(fn);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return ric_fail(MPCQP_ERR_NO_DEVICE, "no HIP device available"); }
    if (device < 0 || device >= ndev) return ric_fail(MPCQP_ERR_ARG, f + ": bad device index");
    int prev = 0;
    RIC_HIPCHK(hipGetDevice(&prev));
    if (prev != device) { RIC_HIPCHK(hipSetDevice(device)); sg->prev_device = prev; }
    return MPCQP_OK;
}

template <class Kernel, class Args>
int launch(Kernel kernel, const Args &a, int batch, size_t lds, hipStream_t st) {
    RIC_HIPCHK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(RIC_NT), lds, st, a);
    RIC_HIPCHK(hipGetLastError());
    return MPCQP_OK;
}

}  // namespace

extern "C" int mpcqp_dare(int device, void *stream, int batch, int n, int m, const mpcqp_riccati_settings *s,
                          const double *A, const double *B, const double *Q, const double *R,
                          double *X, double *K, int32_t *status, int32_t *iters, double *res) {
    Staging sg;
    mpcqp_riccati_settings use;
    if (int rc = check_sizes("mpcqp_dare", batch, n, m, s, &use)) return rc;
    if (!A || !B || !Q || !R || !X || !status) return ric_fail(MPCQP_ERR_ARG, "mpcqp_dare: A, B, Q, R, X and status must be given");
    if (int rc = enter_device("mpcqp_dare", device, &sg)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = (size_t)batch;
    sg.in(&A, nb * n * n); sg.in(&B, nb * n * m); sg.in(&Q, nb * n * n); sg.in(&R, nb * m * m);
    sg.out(&X, nb * n * n); sg.out(&K, nb * m * n); sg.out(&status, nb); sg.out(&iters, nb); sg.out(&res, nb);
    RIC_HIPCHK(sg.begin(st));
    RicArgs a{n, m, use.max_iter, use.gain_form, use.tol, A, B, Q, R, X, K, status, iters, res};
    const int rc = (n <= 16 && m <= 16) ? launch(k_dare<16>, a, batch, ric_dare_lds<16>(), st) : launch(k_dare<32>, a, batch, ric_dare_lds<32>(), st);
    if (rc) return rc;
    RIC_HIPCHK(sg.end(st));
    return MPCQP_OK;
}

extern "C" int mpcqp_dare_adjoint(int device, void *stream, int batch, int n, int m, const mpcqp_riccati_settings *s,
                                  const double *A, const double *B, const double *Q, const double *R,
                                  const double *X, const double *K, const int32_t *status,
                                  const double *G_X, const double *G_K,
                                  double *d_A, double *d_B, double *d_Q, double *d_R, int32_t *iters) {
    Staging sg;
    mpcqp_riccati_settings use;
    if (int rc = check_sizes("mpcqp_dare_adjoint", batch, n, m, s, &use)) return rc;
    if (!A || !B || !Q || !R || !X || !K) return ric_fail(MPCQP_ERR_ARG, "mpcqp_dare_adjoint: A, B, Q, R, X and K must be given");
    if (!G_X && !G_K) return ric_fail(MPCQP_ERR_ARG, "mpcqp_dare_adjoint: give a seed, G_X or G_K");
    if (!d_A && !d_B && !d_Q && !d_R) return ric_fail(MPCQP_ERR_ARG, "mpcqp_dare_adjoint: no gradient asked for");
    if (int rc = enter_device("mpcqp_dare_adjoint", device, &sg)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = (size_t)batch;
    sg.in(&A, nb * n * n); sg.in(&B, nb * n * m); sg.in(&R, nb * m * m); sg.in(&X, nb * n * n); sg.in(&K, nb * m * n);
    sg.in(&status, nb); sg.in(&G_X, nb * n * n); sg.in(&G_K, nb * m * n);
    sg.out(&d_A, nb * n * n); sg.out(&d_B, nb * n * m); sg.out(&d_Q, nb * n * n); sg.out(&d_R, nb * m * m); sg.out(&iters, nb);
    RIC_HIPCHK(sg.begin(st));
    RicAdjArgs a{n, m, use.max_iter, use.gain_form, use.tol, A, B, R, X, K, status, G_X, G_K, d_A, d_B, d_Q, d_R, iters};      // (Q itself does not enter the derivative)
    const int rc = (n <= 16 && m <= 16) ? launch(k_dare_adjoint<16>, a, batch, ric_adjoint_lds<16>(), st)
                                        : launch(k_dare_adjoint<32>, a, batch, ric_adjoint_lds<32>(), st);
    if (rc) return rc;
    RIC_HIPCHK(sg.end(st));
    return MPCQP_OK;
}

// ---- the Riccati difference equation (include_ext3/mpcqp_riccati_traj.h) ---------------------------------------------------------------
namespace {

int check_traj(const char *fn, int batch, int n, int m, int T, int A_steps, int B_steps, const mpcqp_riccati_settings *s, int *gain_form) {
    const std::string f(fn);
    if (batch < 1 || n < 1 || m < 1 || T < 1) return ric_fail(MPCQP_ERR_ARG, f + ": batch, n, m and T must be at least 1");
    if (n > 32 || m > 32) return ric_fail(MPCQP_ERR_UNSUPPORTED, f + ": n > 32 or m > 32 is not implemented (an instance lives in one workgroup's LDS)");
    if ((A_steps != T && A_steps != 1) || (B_steps != T && B_steps != 1)) return ric_fail(MPCQP_ERR_ARG, f + ": A_steps and B_steps must each be T (a trajectory) or 1 (one matrix)");
    *gain_form = 0;
    if (s) {
        if (s->struct_size != (int32_t)sizeof(mpcqp_riccati_settings)) return ric_fail(MPCQP_ERR_ARG, f + ": mpcqp_riccati_settings.struct_size is not sizeof(mpcqp_riccati_settings)");
        if (s->gain_form != 0 && s->gain_form != 1) return ric_fail(MPCQP_ERR_ARG, f + ": gain_form must be 0 or 1");
        *gain_form = s->gain_form;
    }
    return MPCQP_OK;
}

}  // namespace

extern "C" int mpcqp_dre(int device, void *stream, int batch, int n, int m, int T, const mpcqp_riccati_settings *s,
                         const double *A, int A_steps, const double *B, int B_steps, const double *Q, const double *R, const double *X0,
                         double *X_traj, double *K_traj, int32_t *status, int32_t *first_bad) {
    Staging sg;
    int gf = 0;
    if (int rc = check_traj("mpcqp_dre", batch, n, m, T, A_steps, B_steps, s, &gf)) return rc;
    if (!A || !B || !Q || !R || !X0 || !X_traj || !status) return ric_fail(MPCQP_ERR_ARG, "mpcqp_dre: A, B, Q, R, X0, X_traj and status must be given");
    if (int rc = enter_device("mpcqp_dre", device, &sg)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = (size_t)batch, a_tv = A_steps == T && T > 1, b_tv = B_steps == T && T > 1;
    sg.in(&A, (size_t)A_steps * nb * n * n); sg.in(&B, (size_t)B_steps * nb * n * m); sg.in(&Q, nb * n * n); sg.in(&R, nb * m * m); sg.in(&X0, nb * n * n);
    sg.out(&X_traj, (size_t)(T + 1) * nb * n * n); sg.out(&K_traj, (size_t)T * nb * m * n); sg.out(&status, nb); sg.out(&first_bad, nb);
    RIC_HIPCHK(sg.begin(st));
    DreArgs a{n, m, T, gf, (int)a_tv, (int)b_tv, batch, A, B, Q, R, X0, X_traj, K_traj, status, first_bad};
    const int rc = (n <= 16 && m <= 16) ? launch(k_dre<16>, a, batch, ric_dre_lds<16>(), st) : launch(k_dre<32>, a, batch, ric_dre_lds<32>(), st);
    if (rc) return rc;
    RIC_HIPCHK(sg.end(st));
    return MPCQP_OK;
}

extern "C" int mpcqp_dre_adjoint(int device, void *stream, int batch, int n, int m, int T, const mpcqp_riccati_settings *s,
                                 const double *A, int A_steps, const double *B, int B_steps, const double *Q, const double *R, const double *X0,
                                 const double *X_traj, const int32_t *status, const double *G_X, const double *G_K,
                                 double *d_A, double *d_B, double *d_Q, double *d_R, double *d_X0) {
    (void)Q; (void)X0;                                   // (they do not enter the derivative)
    Staging sg;
    int gf = 0;
    if (int rc = check_traj("mpcqp_dre_adjoint", batch, n, m, T, A_steps, B_steps, s, &gf)) return rc;
    if (!A || !B || !R || !X_traj) return ric_fail(MPCQP_ERR_ARG, "mpcqp_dre_adjoint: A, B, R and X_traj must be given");
    if (!G_X && !G_K) return ric_fail(MPCQP_ERR_ARG, "mpcqp_dre_adjoint: give a seed, G_X or G_K");
    if (!d_A && !d_B && !d_Q && !d_R && !d_X0) return ric_fail(MPCQP_ERR_ARG, "mpcqp_dre_adjoint: no gradient asked for");
    if (int rc = enter_device("mpcqp_dre_adjoint", device, &sg)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = (size_t)batch, a_tv = A_steps == T && T > 1, b_tv = B_steps == T && T > 1;
    sg.in(&A, (size_t)A_steps * nb * n * n); sg.in(&B, (size_t)B_steps * nb * n * m); sg.in(&R, nb * m * m); sg.in(&X_traj, (size_t)(T + 1) * nb * n * n);
    sg.in(&status, nb); sg.in(&G_X, (size_t)(T + 1) * nb * n * n); sg.in(&G_K, (size_t)T * nb * m * n);
    sg.out(&d_A, (size_t)A_steps * nb * n * n); sg.out(&d_B, (size_t)B_steps * nb * n * m); sg.out(&d_Q, nb * n * n); sg.out(&d_R, nb * m * m); sg.out(&d_X0, nb * n * n);
    RIC_HIPCHK(sg.begin(st));
    DreAdjArgs a{n, m, T, gf, (int)a_tv, (int)b_tv, batch, A, B, R, X_traj, status, G_X, G_K, d_A, d_B, d_Q, d_R, d_X0};
    const int rc = (n <= 16 && m <= 16) ? launch(k_dre_adjoint<16>, a, batch, ric_dre_adjoint_lds<16>(), st)
                                        : launch(k_dre_adjoint<32>, a, batch, ric_dre_adjoint_lds<32>(), st);
    if (rc) return rc;
    RIC_HIPCHK(sg.end(st));
    return MPCQP_OK;
}
