// plan_driver.hip -- stand-alone host program of tests/test_plan.py: pympc_amd/csrc/mpcqp_plan.h without a GPU.
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 tests/plan_driver.hip -o plan_driver
//   plan_driver <cases file>
// The cases file: the compute-unit count on its first line, then one case per line: batch nx nu Np Nc soft backend tuning.
// Prints one JSON line per case (the fields scripts/record_plan_table.py records through the library's getters), then one line with
// both tables of solve kernels (mpcqp_defs.h), every row named for LOOP false and true.
// The same header chain as pympc_amd/csrc/mpcqp.hip, up to and including mpcqp_plan.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/mpcqp.h"
#include "../include/mpcqp_polish.h"
#include "../include/mpcqp_model.h"
#include "../include/mpcqp_adjoint.h"
#include "../include/mpcqp_adjoint_model.h"
#include "../include/mpcqp_rollout.h"
#include "../include/mpcqp_rollout_est.h"

#include "../pympc_amd/csrc/mpcqp_defs.h"
#include "../pympc_amd/csrc/mpcqp_layout.h"
#include "../pympc_amd/csrc/mpcqp_qp.h"
#include "../pympc_amd/csrc/mpcqp_factor.h"
#include "../pympc_amd/csrc/mpcqp_sweeps.h"
#include "../pympc_amd/csrc/mpcqp_group.h"
#include "../pympc_amd/csrc/mpcqp_bcr.h"
#include "../pympc_amd/csrc/mpcqp_wide.h"
#include "../pympc_amd/csrc/mpcqp_huge.h"
#include "../pympc_amd/csrc/mpcqp_dense.h"
#include "../pympc_amd/csrc/mpcqp_border.h"
#include "../pympc_amd/csrc/mpcqp_phases.h"
#include "../pympc_amd/csrc/mpcqp_run.h"
#include "../pympc_amd/csrc/mpcqp_tiny.h"
#include "../pympc_amd/csrc/mpcqp_lat.h"
#include "../pympc_amd/csrc/mpcqp_latw.h"
#include "../pympc_amd/csrc/mpcqp_kernels.h"
#include "../pympc_amd/csrc/mpcqp_latw_check.h"
#include "../pympc_amd/csrc/mpcqp_plan.h"

static std::string quoted_name(const RunKernelId &k, bool loop) {
    char buf[128];
    run_kernel_name(k, loop, buf, sizeof(buf));
    return std::string("\"") + buf + "\"";
}

int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: plan_driver <cases file>\n"); return 2; }
    int ncu = 0;
    if (fscanf(f, "%d", &ncu) != 1) return 2;
    int batch, nx, nu, Np, Nc, soft, backend, tuning;
    while (fscanf(f, "%d %d %d %d %d %d %d %d", &batch, &nx, &nu, &Np, &Nc, &soft, &backend, &tuning) == 8) {
        mpcqp_settings S;
        memset(&S, 0, sizeof(S));       // (the plan reads soft_constraints, backend and tuning only)
        S.soft_constraints = soft; S.backend = backend; S.tuning = tuning;
        Plan p;
        std::string why;
        const int rc = make_plan(ncu, batch, nx, nu, Np, Nc, S, &p, &why);
        if (rc) { printf("{\"rc\": %d, \"error\": \"%s\"}\n", rc, why.c_str()); continue; }     // (no message holds a character JSON escapes)
        int n, m; int64_t fd, nnzL, it, rd, sv;
        plan_dims(p, &n, &m, &fd, &nnzL);
        plan_stream_bytes(p, &it, &rd, &sv);
        printf("{\"rc\": 0, \"kernel\": [%s, %s], \"occupancy\": [%d, %d, %d], \"dims\": [%d, %d, %lld, %lld], \"stream_bytes\": [%lld, %lld, %lld], \"work\": %lld}\n",
               quoted_name(p.kernel, false).c_str(), quoted_name(p.kernel, true).c_str(), plan_occupancy(p), p.ncu, plan_threads(p),
               n, m, (long long)fd, (long long)nnzL, (long long)it, (long long)rd, (long long)sv, (long long)plan_mfma_per_iter(p));
    }
    fclose(f);
    std::string t256, t512;
#define X(NB, LDSS, NXT, NUT, MODE) for (int loop = 0; loop < 2; ++loop) t256 += (t256.empty() ? "" : ", ") + quoted_name(RunKernelId{NB, LDSS, NXT, NUT, MODE, false}, loop != 0);
    MPCQP_RUN_KERNELS_256(X)
#undef X
#define X(NB, LDSS, NXT, NUT, MODE) for (int loop = 0; loop < 2; ++loop) t512 += (t512.empty() ? "" : ", ") + quoted_name(RunKernelId{NB, LDSS, NXT, NUT, MODE, true}, loop != 0);
    MPCQP_RUN_KERNELS_512(X)
#undef X
    printf("{\"kernels_256\": [%s], \"kernels_512\": [%s]}\n", t256.c_str(), t512.c_str());
    return 0;
}
