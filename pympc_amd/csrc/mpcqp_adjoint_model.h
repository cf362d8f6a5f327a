// mpcqp_adjoint_model.h -- part of libmpcqp_hip (included by mpcqp.hip, one translation unit; C ABI in include/mpcqp_adjoint_model.h).
// The matrix half of the adjoint derivatives: dL/dP = -sym(r_w w*'), dL/dA = -(y* r_w' + r_y w*') chained into Ad, Bd, Qx, QxN, Qu, QDu and
// eps_feas (the row visitors of mpcqp_qp.h read backwards).  k_adjoint_model runs on the handle's stream BEHIND k_adjoint and reads what
// that left: column 0 of its work area -- r_w, r_y of seed 0, in the UNSCALED units the outputs need (k_adjoint's sweeps solve
// c (g - P x) - A' (c y + ..) = 0 with the unscaled P and A of the row visitors, the scaling enters through the metric of K_pol alone; its
// own outputs are oq = -x, ol / ou = y as they stand) -- the ADMM iterate w*, y* (unscaled), the model blob and the step data.  r_y is zero
// on inactive rows; only the dynamics rows, always active, are read here.  (After mpcqp_mpc_step the step data are the
// adjoint's copy with the u_{-1} that solve was made with: launch_adjoint in mpcqp.hip.)
// One 256-thread workgroup per instance, plain vector FP64: Np + 1 small outer products per output.  The five vectors go through LDS where
// they fit in 64 KB and are read from global memory where they do not (n = 2920 at (20, 8, 60)).  Where the instance has fewer output
// entries than the workgroup has threads (65 at (4, 2, 200)) the sum over the stages is split into S = NT / entries contiguous ranges, one
// per thread, and the S partial sums of an entry are added in range order: a fixed order, the same bits every time.
// Entry (i, j) of a weight gradient is formed from (min, max) of its indices, so the gradient is symmetric to the bit.
// k_adjoint_model_sum adds the per-instance gradients over the batch (mpcqp_adjoint_model_io.batch_sum): sixteen lanes per entry each add
// every sixteenth instance in ascending order, then a binary tree over the sixteen in LDS -- no atomics, a fixed order.
#pragma once

constexpr int ADJM_FIELDS = 7;      // Ad, Bd, Qx, QxN, Qu, QDu, eps_feas

struct AdjointModelArgs {
    const double *rw, *ry;        // [batch][ADJOINT_COLS][n], [batch][ADJOINT_COLS][m]: AdjointArgs::x, ::y (column 0 is read)
    const double *w, *y;          // [batch][n], [batch][m] the iterate (Ptrs::x, ::y)
    const double *model, *step;
    const int *status;            // [batch] AdjointArgs::status: anything but 1 gives zeros
    double *out;                  // field f of instance b: out + batch off[f] + b (off[f + 1] - off[f])
    int off[ADJM_FIELDS + 1];     // entries of the fields before f; off[ADJM_FIELDS]: entries of one instance
    int batch, staged;            // staged: the vectors are copied into LDS first
};

// Entry e of an instance's gradients, summed over range s of S of its stages.
__device__ __forceinline__ double adjoint_model_entry(const Lay &L, const AdjointModelArgs &M, const double *W, const double *RW, const double *Y, const double *RY,
                                                      const double *model, const double *step, int e, int s, int S) {
    int f = 0;
    while (e >= M.off[f + 1]) ++f;
    const int idx = e - M.off[f];
    const int K = f <= 2 ? L.Np : f == 3 ? 1 : f <= 5 ? L.Nc : (L.soft ? L.n_x : 0);
    const int chunk = (K + S - 1) / S, k0 = s * chunk, k1 = min(K, k0 + chunk);
    double acc = 0.0;
    if (f == 0) {                                        // Ad: dynamics rows of stage k + 1 against x_k
        const int i = idx / L.nx, j = idx - i * L.nx;
        for (int k = k0; k < k1; ++k) acc += Y[(k + 1) * L.nx + i] * RW[k * L.nx + j] + RY[(k + 1) * L.nx + i] * W[k * L.nx + j];
        return -acc;
    }
    if (f == 1) {                                        // Bd: ... against u_{min(k, Nc - 1)}
        const int i = idx / L.nu, j = idx - i * L.nu;
        for (int k = k0; k < k1; ++k) {
            const int col = L.ou + min(k, L.Nc - 1) * L.nu + j;
            acc += Y[(k + 1) * L.nx + i] * RW[col] + RY[(k + 1) * L.nx + i] * W[col];
        }
        return -acc;
    }
    if (f <= 3) {                                        // Qx (k < Np), QxN (k = Np): P_X and q_X[k] = -Q_k xref_k
        const int i = idx / L.nx, j = idx - i * L.nx, lo = min(i, j), hi = max(i, j);
        const double *xref = step + L.nx + L.nu;
        for (int k = k0; k < k1; ++k) {
            const int kk = f == 3 ? L.Np : k, base = kk * L.nx;
            const double *xr = L.xref_rows == 1 ? xref : xref + base;
            acc += RW[base + lo] * (W[base + hi] - xr[hi]) + RW[base + hi] * (W[base + lo] - xr[lo]);
        }
        return -0.5 * acc;
    }
    if (f == 4) {                                        // Qu: iU_k Qu on the diagonal blocks and q_U[k] = -iU_k Qu uref
        const int i = idx / L.nu, j = idx - i * L.nu, lo = min(i, j), hi = max(i, j);
        const double *uref = model + L.ouref;
        for (int k = k0; k < k1; ++k) {
            const int base = L.ou + k * L.nu;
            const double iu = (k == L.Nc - 1) ? (double)(L.Np - L.Nc + 1) : 1.0;
            acc += iu * (RW[base + lo] * (W[base + hi] - uref[hi]) + RW[base + hi] * (W[base + lo] - uref[lo]));
        }
        return -0.5 * acc;
    }
    if (f == 5) {                                        // QDu: the differences u_k - u_{k-1}, u_{-1} from the step data
        const int i = idx / L.nu, j = idx - i * L.nu, lo = min(i, j), hi = max(i, j);
        const double *um1 = step + L.nx;
        for (int k = k0; k < k1; ++k) {
            const int base = L.ou + k * L.nu;
            const double rl = RW[base + lo] - (k > 0 ? RW[base - L.nu + lo] : 0.0), rh = RW[base + hi] - (k > 0 ? RW[base - L.nu + hi] : 0.0);
            const double ul = W[base + lo] - (k > 0 ? W[base - L.nu + lo] : um1[lo]), uh = W[base + hi] - (k > 0 ? W[base - L.nu + hi] : um1[hi]);
            acc += rl * uh + rh * ul;
        }
        return -0.5 * acc;
    }
    for (int k = k0; k < k1; ++k) acc += RW[L.oe + k] * W[L.oe + k];      // eps_feas I on the slack variables
    return -acc;
}

__global__ __launch_bounds__(NT) void k_adjoint_model(Lay L, AdjointModelArgs M) {
    extern __shared__ __attribute__((aligned(16))) double sh[];
    const int b = blockIdx.x, tid = threadIdx.x, E = M.off[ADJM_FIELDS];
    auto dst = [&](int e) -> double & {
        int f = 0;
        while (e >= M.off[f + 1]) ++f;
        return M.out[(size_t)M.batch * M.off[f] + (size_t)b * (M.off[f + 1] - M.off[f]) + (e - M.off[f])];
    };
    if (M.status[b] != 1) {                                  // not computed: every output is zero (uniform over the workgroup)
        for (int e = tid; e < E; e += NT) dst(e) = 0.0;
        return;
    }
    const double *W = M.w + (size_t)b * L.n, *Y = M.y + (size_t)b * L.m;
    const double *RW = M.rw + (size_t)b * ADJOINT_COLS * L.n, *RY = M.ry + (size_t)b * ADJOINT_COLS * L.m;
    const double *model = M.model + (size_t)b * L.model_sz, *step = M.step + (size_t)b * L.step_sz;
    double *part = sh;                                       // [NT] the partial sums of the split stage loop
    if (M.staged) {                                          // [ part | w | r_w | y (dynamics rows) | r_y (dynamics rows) ]
        double *w = sh + NT, *rw = w + L.n, *y = rw + L.n, *ry = y + L.n_x;
        for (int i = tid; i < L.n; i += NT) { w[i] = W[i]; rw[i] = RW[i]; }
        for (int i = tid; i < L.n_x; i += NT) { y[i] = Y[i]; ry[i] = RY[i]; }
        __syncthreads();
        W = w; RW = rw; Y = y; RY = ry;
    }
    const int S = E < NT ? NT / E : 1;
    if (S == 1) {
        for (int e = tid; e < E; e += NT) dst(e) = adjoint_model_entry(L, M, W, RW, Y, RY, model, step, e, 0, 1);
        return;
    }
    if (tid < E * S) part[tid] = adjoint_model_entry(L, M, W, RW, Y, RY, model, step, tid % E, tid / E, S);      // (E S <= NT)
    __syncthreads();
    if (tid < E) {
        double v = part[tid];
        for (int s = 1; s < S; ++s) v += part[s * E + tid];
        dst(tid) = v;
    }
}

// sum[off[f] + idx] = sum over b of field f, entry idx: 16 entries by 16 lanes per workgroup
__global__ __launch_bounds__(256) void k_adjoint_model_sum(AdjointModelArgs M, double *sum) {
    __shared__ double part[16][17];
    const int tx = threadIdx.x & 15, r = threadIdx.x >> 4, e = blockIdx.x * 16 + tx, E = M.off[ADJM_FIELDS];
    double v = 0.0;
    if (e < E) {
        int f = 0;
        while (e >= M.off[f + 1]) ++f;
        const int sz = M.off[f + 1] - M.off[f];
        const double *src = M.out + (size_t)M.batch * M.off[f] + (e - M.off[f]);
        for (int b = r; b < M.batch; b += 16) v += src[(size_t)b * sz];
    }
    part[r][tx] = v;
    __syncthreads();
    for (int h = 8; h >= 1; h >>= 1) {
        if (r < h) part[r][tx] += part[r + h][tx];
        __syncthreads();
    }
    if (r == 0 && e < E) sum[e] = part[0][tx];
}
