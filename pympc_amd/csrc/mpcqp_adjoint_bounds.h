// mpcqp_adjoint_bounds.h -- part of libmpcqp_hip (included by mpcqp.hip, one translation unit; C ABI in include/mpcqp_adjoint_bounds.h).
// The bound half of the adjoint derivatives: dL/db = r_y on the active rows, chained into xmin, xmax, umin, umax, Dumin, Dumax -- row_bounds
// (mpcqp_qp.h) read backwards.  Every inequality row's bound is one of the six (the first Delta-u rows' plus u_{-1}, whose own path is
// adjoint_outputs'), so entry e of an instance's gradients is a sum of r_y over the rows of one component that are active on one side.
//   sweeps        rollout_adjoint_body (mpcqp_rollout.h) adds adjoint_bounds_entry of every differentiated tape entry onto a per-instance
//                 accumulator, under RolloutSweep::want_bounds, beside the sums of adjoint_model_entry.
//   single solve  k_adjoint_bounds runs on the handle's stream BEHIND k_adjoint -- which is not touched -- and reads what that left: the active
//                 set (KpolBufs::act) and column 0 of its work area, r_y of seed 0 in the unscaled units the outputs need (k_adjoint's own
//                 ol / ou are y on the rows with act 1 / 2).  One 256-thread workgroup per instance, a thread per entry.
// The per-instance gradients are field-major like the model's (field f of instance b: out + batch off[f] + b (off[f + 1] - off[f])), so that
// k_adjoint_model_sum (mpcqp_adjoint_model.h) adds them over the batch: the six fields and an empty seventh.
#pragma once

constexpr int ADJB_FIELDS = 6;      // xmin, xmax, umin, umax, Dumin, Dumax
static_assert(ADJB_FIELDS <= ADJM_FIELDS, "the batch sum of the bound gradients goes through k_adjoint_model_sum's offset table");

// Entries of the bound gradients of one instance: [xmin | xmax | umin | umax | Dumin | Dumax]
__host__ __device__ inline int adjoint_bounds_entries(const Lay &L) { return 2 * L.nx + 4 * L.nu; }

// Entry e in [0, 2 nx + 4 nu) of one solve: the sum of r_y over the rows of its component that are active on its side (act 1: lower or
// equality, 2: upper), in ascending row order.  A clipped (infinite) bound is never active: the sum is empty, exactly 0.
__device__ __forceinline__ double adjoint_bounds_entry(const Lay &L, const int *act, const double *ry, int e) {
    int side, row, stride, count;
    if (e < 2 * L.nx) {                                  // the state box: N stages of nx rows
        const int f = e >= L.nx ? 1 : 0;
        side = f + 1; row = L.rs + (e - f * L.nx); stride = L.nx; count = L.N;
    } else {
        const int e2 = e - 2 * L.nx, f = e2 / L.nu, j = e2 - f * L.nu;
        side = (f & 1) + 1; stride = L.nu;
        if (f < 2) { row = L.ri + j; count = L.Nc; }     // the input box: Nc stages of nu rows
        else { row = L.rdu + j; count = L.Nc + 1; }      // the Delta-u rows: Nc + 1 blocks of nu rows, the first (bounds + u_{-1}) included
    }
    double acc = 0.0;
    for (int k = 0; k < count; ++k, row += stride)
        if (act[row] == side) acc += ry[row];
    return acc;
}

struct AdjointBoundsArgs {
    const int *act;               // [batch][m] KpolBufs::act as k_adjoint left it
    const double *ry;             // [batch][ADJOINT_COLS][m] AdjointArgs::y (column 0 is read)
    const int *status;            // [batch] AdjointArgs::status: anything but 1 gives zeros
    double *out;                  // field-major per-instance gradients (see above)
    int batch;
};

__global__ __launch_bounds__(NT) void k_adjoint_bounds(Lay L, AdjointBoundsArgs M) {
    const int b = blockIdx.x, nx = L.nx, nu = L.nu, E = adjoint_bounds_entries(L);
    const bool ok = M.status[b] == 1;                    // (uniform over the workgroup)
    const int *act = M.act + (size_t)b * L.m;
    const double *ry = M.ry + (size_t)b * ADJOINT_COLS * L.m;
    for (int e = threadIdx.x; e < E; e += NT) {
        const int f = e < 2 * nx ? e / nx : 2 + (e - 2 * nx) / nu, sz = f < 2 ? nx : nu, off = f < 2 ? f * nx : 2 * nx + (f - 2) * nu;
        M.out[(size_t)M.batch * off + (size_t)b * sz + (e - off)] = ok ? adjoint_bounds_entry(L, act, ry, e) : 0.0;
    }
}
