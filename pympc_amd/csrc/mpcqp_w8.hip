// mpcqp_w8.hip -- second translation unit of libmpcqp_hip.so: the solve / closed-loop kernel of the latency backend with 512-THREAD workgroups
// (eight waves, two per SIMD) for handles with at most one instance per compute unit (mpcqp_plan.h: Lay::nw = 8; mpcqp_latw.h says why).
//
// The device code of this library is written against the compile-time workgroup size NT (mpcqp_defs.h): here the same headers are compiled once
// more with NT = 512, inside namespace w8 so that nothing collides with the 256-thread instantiations of mpcqp.hip.  Only k_mpc_run of the
// cyclic-reduction modes with a dense top (MODE_BCRT + 11 / 21 / 31) is instantiated -- and, for ONE controller of the reference's cart pole on a
// long horizon (grouped stages, round staged in LDS), the sweeps kernel: half of its iteration is owner passes that eight waves run faster than
// four; their begin / check / factorization phases are the common ones at 512 threads.  Setup, export and the verification kernels of such a handle run from mpcqp.hip at 256 threads -- every phase sizes
// its loops by NT, and the data in memory does not know how many threads wrote it.
// What is instantiated here is the table MPCQP_RUN_KERNELS_512 of mpcqp_defs.h, every row for LOOP false and true, and nothing else.
// Host side: one function, called by launch_run in mpcqp.hip with the RunKernelId the handle's plan chose (run_kernel_id in mpcqp_plan.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>

#include "../../include/mpcqp.h"

#define NT 512
#define MPCQP_LAT_ONLY 1
#include "mpcqp_defs.h"

namespace w8 {
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

template <int NB, bool LDSS, int NXT, int NUT, int MODE>
static int launch(const RunKArgs &A, bool loop, int grid, size_t smem, hipStream_t stream) {
    auto kernel = loop ? k_mpc_run<NB, LDSS, NXT, NUT, MODE, true> : k_mpc_run<NB, LDSS, NXT, NUT, MODE, false>;
    if (smem > 48 * 1024 && hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return 1;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), smem, stream, A);
    return 0;
}
}  // namespace w8

// id: a row of MPCQP_RUN_KERNELS_512 (mpcqp_defs.h), chosen by run_kernel_id in mpcqp_plan.h.  3: not one of this unit's kernels.
int mpcqp_w8_launch(const void *kargs, size_t kargs_bytes, const RunKernelId &id, int loop, int grid, size_t smem, hipStream_t stream) {
    using namespace w8;
    if (kargs_bytes != sizeof(RunKArgs)) return 2;
    RunKArgs A; memcpy(&A, kargs, sizeof(A));
#define X(NB, LDSS, NXT, NUT, MODE) if (same_kernel(id, RunKernelId{NB, LDSS, NXT, NUT, MODE, true})) return launch<NB, LDSS, NXT, NUT, MODE>(A, loop != 0, grid, smem, stream);
    MPCQP_RUN_KERNELS_512(X)
#undef X
    return 3;
}

#ifdef MPCQP_RUN_TIMING
// development build: this unit's phase clocks (mpcqp_get_stats prints them beside its own)
void mpcqp_w8_ticks(unsigned long long *out16, unsigned long long *outw48, unsigned long long *outb128) {
    hipMemcpyFromSymbol(out16, HIP_SYMBOL(w8::g_ticks), 16 * sizeof(unsigned long long));
    hipMemcpyFromSymbol(outw48, HIP_SYMBOL(w8::g_wticks), 48 * sizeof(unsigned long long));
    hipMemcpyFromSymbol(outb128, HIP_SYMBOL(w8::g_bticks), 128 * sizeof(unsigned long long));
    unsigned long long z[128] = {0};
    hipMemcpyToSymbol(HIP_SYMBOL(w8::g_ticks), z, 16 * sizeof(unsigned long long));
    hipMemcpyToSymbol(HIP_SYMBOL(w8::g_wticks), z, 48 * sizeof(unsigned long long));
    hipMemcpyToSymbol(HIP_SYMBOL(w8::g_bticks), z, sizeof(z));
}
#endif
