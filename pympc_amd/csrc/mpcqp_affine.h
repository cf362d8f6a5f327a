// mpcqp_affine.h -- part of libmpcqp_hip (included by mpcqp.hip, one translation unit; C ABI in include_ext4/mpcqp_affine.h).
// The affine term d of the prediction model x_{k+1} = Ad x_k + Bd u_k + d_k.  It lives in the step blob (Lay::od, Np nx doubles, in force while
// Lay::d_rows > 0) and enters the QP as the bound 0.0 - d_k of dynamics row block k + 1: affine_bound (mpcqp_qp.h) is the one statement of that
// rule -- row_bounds for setup, begin, residuals, polish, adjoint, eq_solve and export; the owners' bound registers of the hot rounds (own_load,
// gown_update, admm_tiny, admm_lat, admm_latw).  Here: the rule read backwards.
//   single solve  k_affine_grad runs on the handle's stream BEHIND k_adjoint -- which is not touched -- and reads column 0 of its work area,
//                 r_y of seed 0 in unscaled units (k_adjoint's own d_x0 is -r_y of row block 0; every equality row is in its active set).
#pragma once

// out [batch][d_rows nx]: d_rows = Np: entry (k, i) = -r_y[(k + 1) nx + i]; d_rows = 1: entry i = the sum of those over k, in ascending k.
// status: AdjointArgs::status, anything but 1 gives zeros.
__global__ __launch_bounds__(NT) void k_affine_grad(Lay L, const double *ry_all, const int *status, double *out) {
    const int b = blockIdx.x, w = L.d_rows * L.nx;
    const bool ok = status[b] == 1;                      // (uniform over the workgroup)
    const double *ry = ry_all + (size_t)b * ADJOINT_COLS * L.m + L.nx;      // (row block 1 onwards)
    for (int e = threadIdx.x; e < w; e += NT) {
        double acc = 0.0;
        if (ok) {
            if (L.d_rows > 1) acc = -ry[e];
            else for (int k = 0; k < L.Np; ++k) acc -= ry[k * L.nx + e];
        }
        out[(size_t)b * w + e] = acc;
    }
}
