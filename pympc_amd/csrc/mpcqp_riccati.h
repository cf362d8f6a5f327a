// mpcqp_riccati.h -- device code of mpcqp_riccati.hip (include/mpcqp_riccati.h): one 256-thread workgroup solves one discrete algebraic
// Riccati equation, or the adjoint of one, entirely in LDS.
//
// Every matrix is an NB x NB block of doubles in LDS (NB = 16 or 32), zero-padded beyond its n or m rows and columns, so that every
// product is a whole number of 16 x 16 tiles of v_mfma_f64_16x16x4_f64 (one tile per wave and instruction, four steps of K; lane l feeds
// A[l & 15][l >> 4] and B[l >> 4][l & 15] and receives C[(l >> 4) + 4 v][l & 15], v = 0..3 -- the operand map of mpcqp_factor.h).  One tile on
// wave 0 at NB = 16, four tiles on the four waves at NB = 32.  A product takes its operands by (pointer, row stride, column stride): a
// transposed operand is the same block read with the strides swapped, a block of the augmented matrix of the LU a pointer into it.
// Every loop is bounded by max_iter, n, m or NB; no atomics; nothing here looks at another workgroup; an instance's arithmetic depends on
// its own data alone, so its result has the same bits wherever it sits in whatever batch.
#pragma once

#define RIC_NT 256
typedef double ric_d4 __attribute__((ext_vector_type(4)));

struct RicArgs {                       // mpcqp_dare
    int n, m, max_iter, gain_form;
    double tol;
    const double *A, *B, *Q, *R;
    double *X, *K;
    int32_t *status, *iters;
    double *res;
};

struct RicAdjArgs {                    // mpcqp_dare_adjoint
    int n, m, max_iter, gain_form;
    double tol;
    const double *A, *B, *R, *X, *K;
    const int32_t *status;
    const double *G_X, *G_K;
    double *d_A, *d_B, *d_Q, *d_R;
    int32_t *iters;
};

// C = alpha A B + beta C on the matrix cores.  Element (i, k) of A is A[i * sai + k * sak], element (k, j) of B is B[k * sbk + j * sbj], C has
// row stride ldc.  Called by every thread; C may be one of the operands (the products are in registers before anything is written).
template <int NB>
__device__ __forceinline__ void ric_mm(double *C, int ldc, const double *A, int sai, int sak, const double *B, int sbk, int sbj,
                                       double alpha, double beta, int tid) {
    constexpr int TW = NB / 16;
    const int wv = tid >> 6, ln = tid & 63, ti = wv / TW, tj = wv % TW, lr = ln & 15, lk = ln >> 4;
    const bool on = wv < TW * TW;                        // (uniform per wave)
    ric_d4 acc = {0.0, 0.0, 0.0, 0.0};
    if (on) {
#pragma unroll
        for (int kk = 0; kk < NB / 4; ++kk)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(16 * ti + lr) * sai + (4 * kk + lk) * sak], B[(4 * kk + lk) * sbk + (16 * tj + lr) * sbj], acc, 0, 0, 0);
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            double *c = C + (16 * ti + lk + 4 * v) * ldc + 16 * tj + lr;
            *c = beta != 0.0 ? fma(beta, *c, alpha * acc[v]) : alpha * acc[v];
        }
    }
    __syncthreads();
}

// |M|_max over `count` contiguous doubles for every thread; +inf if any of them is not finite.  red: 4 doubles of LDS.
__device__ __forceinline__ double ric_absmax(const double *M, int count, double *red, int tid) {
    double v = 0.0;
    for (int e = tid; e < count; e += RIC_NT) {
        const double a = fabs(M[e]);
        v = a <= 1.7976931348623157e308 ? fmax(v, a) : INFINITY;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    const double r = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return r;
}

// dst (NB x NB, zero-padded) = the rows x cols matrix src in global memory (null: zeros), transposed if `tr` (src is then cols x rows)
template <int NB>
__device__ __forceinline__ void ric_load(double *dst, const double *src, int rows, int cols, bool tr, int tid) {
    for (int e = tid; e < NB * NB; e += RIC_NT) {
        const int i = e / NB, j = e % NB;
        dst[e] = (src != nullptr && i < rows && j < cols) ? (tr ? src[j * rows + i] : src[i * cols + j]) : 0.0;
    }
}

template <int NB>
__device__ __forceinline__ void ric_store(double *dst, const double *src, int rows, int cols, int tid) {
    if (dst == nullptr) return;
    for (int e = tid; e < rows * cols; e += RIC_NT) dst[e] = src[(e / cols) * NB + e % cols];
}

__device__ __forceinline__ void ric_zero(double *dst, int count, int tid) {
    if (dst == nullptr) return;
    for (int e = tid; e < count; e += RIC_NT) dst[e] = 0.0;
}

// In-place Cholesky factorization M = L L' of the leading m x m block (row stride NB; L in the lower triangle).  Returns 1, or at the first
// pivot that is not > 0: -1 (it is <= 0) or 0 (it is not a number).  The same for every thread.  M must be visible (a barrier behind it).
template <int NB>
__device__ __forceinline__ int ric_chol(double *M, int m, int tid) {
    for (int j = 0; j < m; ++j) {
        const double d = M[j * NB + j];
        if (!(d > 0.0)) return d <= 0.0 ? -1 : 0;
        const double l = sqrt(d);
        __syncthreads();
        for (int i = j + tid; i < m; i += RIC_NT) M[i * NB + j] = i == j ? l : M[i * NB + j] / l;
        __syncthreads();
        const int w = m - j - 1;
        for (int e = tid; e < w * w; e += RIC_NT) {
            const int i = j + 1 + e / w, c = j + 1 + e % w;
            if (c <= i) M[i * NB + c] -= M[i * NB + j] * M[c * NB + j];
        }
        __syncthreads();
    }
    return 1;
}

// column c of the m-row block Rhs (row stride ld): Rhs = L^-1 Rhs, then with `full` Rhs = L'^-1 Rhs (together (L L')^-1 Rhs); one thread per column
template <int NB>
__device__ __forceinline__ void ric_chol_solve_col(const double *L, int m, double *Rhs, int ld, int c, bool full) {
    for (int i = 0; i < m; ++i) {
        double s = Rhs[i * ld + c];
        for (int j = 0; j < i; ++j) s -= L[i * NB + j] * Rhs[j * ld + c];
        Rhs[i * ld + c] = s / L[i * NB + i];
    }
    if (!full) return;
    for (int i = m - 1; i >= 0; --i) {
        double s = Rhs[i * ld + c];
        for (int j = i + 1; j < m; ++j) s -= L[j * NB + i] * Rhs[j * ld + c];
        Rhs[i * ld + c] = s / L[i * NB + i];
    }
}

// E = [W | R1 | R2] (NB rows, row stride 3 NB): the two right-hand blocks become W^-1 R1, W^-1 R2 by LU with partial pivoting over the leading
// n x n block of W (beyond it W is the identity and the right-hand sides are zero).  A zero pivot leaves inf / NaN behind, which the caller's
// norm sees.  E must be visible.
template <int NB>
__device__ __forceinline__ void ric_lu_solve(double *E, int n, int tid) {
    constexpr int LD = 3 * NB;
    for (int p = 0; p < n; ++p) {
        int piv = p;
        double best = fabs(E[p * LD + p]);
        for (int i = p + 1; i < n; ++i) {                // (every thread finds the same pivot row: broadcast reads)
            const double a = fabs(E[i * LD + p]);
            if (a > best) { best = a; piv = i; }
        }
        __syncthreads();
        if (piv != p && tid < LD) { const double t = E[p * LD + tid]; E[p * LD + tid] = E[piv * LD + tid]; E[piv * LD + tid] = t; }
        __syncthreads();
        const double dinv = 1.0 / E[p * LD + p];
        const int w = LD - p - 1;
        for (int e = tid; e < (n - p - 1) * w; e += RIC_NT) {
            const int i = p + 1 + e / w, c = p + 1 + e % w;
            E[i * LD + c] -= (E[i * LD + p] * dinv) * E[p * LD + c];
        }
        __syncthreads();
    }
    if (tid < 2 * NB) {
        const int c = NB + tid;
        for (int i = n - 1; i >= 0; --i) {
            double s = E[i * LD + c];
            for (int j = i + 1; j < n; ++j) s -= E[i * LD + j] * E[j * LD + c];
            E[i * LD + c] = s / E[i * LD + i];
        }
    }
    __syncthreads();
}

template <int NB> constexpr size_t ric_dare_lds() { return sizeof(double) * (9 * NB * NB + 4); }
template <int NB> constexpr size_t ric_adjoint_lds() { return sizeof(double) * (13 * NB * NB + 4); }

template <int NB>
__global__ void __launch_bounds__(RIC_NT) k_dare(RicArgs a) {
    extern __shared__ double ric_lds[];
    constexpr int NN = NB * NB, LD = 3 * NB;
    double *Ab = ric_lds, *Gb = Ab + NN, *Hb = Gb + NN, *E = Hb + NN, *T1 = E + 3 * NN, *T2 = T1 + NN, *T3 = T2 + NN, *red = T3 + NN;
    const int tid = threadIdx.x, n = a.n, m = a.m;
    const size_t b = blockIdx.x;
    const double *Ag = a.A + b * n * n, *Bg = a.B + b * n * m, *Qg = a.Q + b * n * n, *Rg = a.R + b * m * m;
    auto finish = [&](int st, int it, double res) {      // the per-instance outcome; zeros in X and K unless converged (they are stored before)
        if (st != 1) { ric_zero(a.X + b * n * n, n * n, tid); ric_zero(a.K ? a.K + b * m * n : nullptr, m * n, tid); }
        if (tid == 0) {
            a.status[b] = st;
            if (a.iters) a.iters[b] = it;
            if (a.res) a.res[b] = st == 1 ? res : 0.0;
        }
    };

    // G_0 = B R^-1 B' = Y'Y, Y = L^-1 B' with R = L L'
    ric_load<NB>(T1, Rg, m, m, false, tid);
    ric_load<NB>(T2, Bg, m, n, true, tid);
    __syncthreads();
    int st = ric_chol<NB>(T1, m, tid);
    if (st != 1) { finish(st, 0, 0.0); return; }
    if (tid < n) ric_chol_solve_col<NB>(T1, m, T2, NB, tid, false);
    __syncthreads();
    ric_mm<NB>(Gb, NB, T2, 1, NB, T2, NB, 1, 1.0, 0.0, tid);
    ric_load<NB>(Ab, Ag, n, n, false, tid);
    ric_load<NB>(Hb, Qg, n, n, false, tid);
    __syncthreads();

    int it = 0;
    bool conv = false;
    while (it < a.max_iter) {
        // E = [I + G H | A | G]
        ric_mm<NB>(E, LD, Gb, NB, 1, Hb, NB, 1, 1.0, 0.0, tid);
        for (int e = tid; e < NN; e += RIC_NT) {
            const int i = e / NB, j = e % NB;
            if (i == j) E[i * LD + j] += 1.0;
            E[i * LD + NB + j] = Ab[e];
            E[i * LD + 2 * NB + j] = Gb[e];
        }
        __syncthreads();
        ric_lu_solve<NB>(E, n, tid);
        const double *Z1 = E + NB, *Z2 = E + 2 * NB;     // W^-1 A, W^-1 G
        ric_mm<NB>(T1, NB, Ab, NB, 1, Z2, LD, 1, 1.0, 0.0, tid);          // A W^-1 G
        ric_mm<NB>(T2, NB, Hb, NB, 1, Z1, LD, 1, 1.0, 0.0, tid);          // H W^-1 A
        ric_mm<NB>(T3, NB, Ab, NB, 1, Z1, LD, 1, 1.0, 0.0, tid);          // A_{k+1}
        ric_mm<NB>(E, LD, T1, NB, 1, Ab, 1, NB, 1.0, 0.0, tid);           // (A W^-1 G) A'   (the W block of E is free)
        for (int e = tid; e < NN; e += RIC_NT) { const int i = e / NB, j = e % NB; Gb[e] += 0.5 * (E[i * LD + j] + E[j * LD + i]); }
        __syncthreads();
        ric_mm<NB>(E, LD, Ab, 1, NB, T2, NB, 1, 1.0, 0.0, tid);           // A' (H W^-1 A)
        for (int e = tid; e < NN; e += RIC_NT) {
            const int i = e / NB, j = e % NB;
            const double d = 0.5 * (E[i * LD + j] + E[j * LD + i]);
            T1[e] = d;
            Hb[e] += d;
            Ab[e] = T3[e];
        }
        __syncthreads();
        ++it;
        const double dmax = ric_absmax(T1, NN, red, tid), hmax = ric_absmax(Hb, NN, red, tid);
        const double omax = fmax(ric_absmax(Gb, NN, red, tid), ric_absmax(Ab, NN, red, tid));
        if (!(fmax(fmax(dmax, hmax), omax) < INFINITY)) break;            // overflow or NaN: not converged, and no reason to go on
        if (dmax <= a.tol * fmax(1.0, hmax)) { conv = true; break; }
    }
    if (!conv) { finish(0, it, 0.0); return; }

    // X = H;  M = R + B'XB,  P = B'XA;  K = M^-1 P,  F = M^-1 B'X;  the residual from the given A, B, Q, R
    double *E0 = E, *E1 = E + NN, *E2 = E + 2 * NN;       // (three plain NB x NB blocks from here on)
    ric_load<NB>(Ab, Ag, n, n, false, tid);
    ric_load<NB>(Gb, Bg, n, m, false, tid);
    __syncthreads();
    ric_mm<NB>(T1, NB, Hb, NB, 1, Gb, NB, 1, 1.0, 0.0, tid);              // X B
    ric_mm<NB>(T2, NB, Hb, NB, 1, Ab, NB, 1, 1.0, 0.0, tid);              // X A
    ric_mm<NB>(T3, NB, Gb, 1, NB, T1, NB, 1, 1.0, 0.0, tid);              // B' X B
    for (int e = tid; e < NN; e += RIC_NT) {
        const int i = e / NB, j = e % NB;
        E0[e] = (i < m && j < m ? Rg[i * m + j] : 0.0) + 0.5 * (T3[e] + T3[j * NB + i]);
        E2[e] = T1[j * NB + i];                                           // (X B)' = B'X
    }
    ric_mm<NB>(E1, NB, Gb, 1, NB, T2, NB, 1, 1.0, 0.0, tid);              // P = B' X A   (its barriers cover the loop above)
    for (int e = tid; e < NN; e += RIC_NT) T3[e] = E1[e];                 // P is needed again for the residual
    st = ric_chol<NB>(E0, m, tid);
    if (st != 1) { finish(st, it, 0.0); return; }
    if (tid < 2 * NB) ric_chol_solve_col<NB>(E0, m, tid < NB ? E1 : E2, NB, tid & (NB - 1), true);
    __syncthreads();
    ric_mm<NB>(E0, NB, Ab, 1, NB, T2, NB, 1, 1.0, 0.0, tid);              // A' X A
    ric_mm<NB>(E0, NB, T3, 1, NB, E1, NB, 1, -1.0, 1.0, tid);             // - P' K
    for (int e = tid; e < NN; e += RIC_NT) {
        const int i = e / NB, j = e % NB;
        if (i < n && j < n) E0[e] += Qg[i * n + j] - Hb[e];
    }
    __syncthreads();
    const double rmax = ric_absmax(E0, NN, red, tid), xmax = ric_absmax(Hb, NN, red, tid);
    const double kmax = ric_absmax(E1, 2 * NN, red, tid);
    if (!(fmax(fmax(rmax, xmax), kmax) < INFINITY)) { finish(0, it, 0.0); return; }
    ric_store<NB>(a.X + b * n * n, Hb, n, n, tid);
    ric_store<NB>(a.K ? a.K + b * m * n : nullptr, a.gain_form == 0 ? E1 : E2, m, n, tid);
    finish(1, it, rmax / fmax(1.0, xmax));
}

template <int NB>
__global__ void __launch_bounds__(RIC_NT) k_dare_adjoint(RicAdjArgs a) {
    extern __shared__ double ric_lds[];
    constexpr int NN = NB * NB;
    double *Ab = ric_lds, *Bb = Ab + NN, *Xb = Bb + NN, *Kg = Xb + NN, *K0 = Kg + NN, *Tb = K0 + NN, *Mb = Tb + NN, *Lb = Mb + NN, *Sb = Lb + NN,
           *Acl = Sb + NN, *U1 = Acl + NN, *U2 = U1 + NN, *U3 = U2 + NN, *red = U3 + NN;
    const int tid = threadIdx.x, n = a.n, m = a.m;
    const size_t b = blockIdx.x;
    const bool gf0 = a.gain_form == 0;
    double *dA = a.d_A ? a.d_A + b * n * n : nullptr, *dB = a.d_B ? a.d_B + b * n * m : nullptr;
    double *dQ = a.d_Q ? a.d_Q + b * n * n : nullptr, *dR = a.d_R ? a.d_R + b * m * m : nullptr;
    auto zeros = [&](int it) {
        ric_zero(dA, n * n, tid); ric_zero(dB, n * m, tid); ric_zero(dQ, n * n, tid); ric_zero(dR, m * m, tid);
        if (tid == 0 && a.iters) a.iters[b] = it;
    };
    if (a.status != nullptr && a.status[b] != 1) { zeros(0); return; }

    ric_load<NB>(Ab, a.A + b * n * n, n, n, false, tid);
    ric_load<NB>(Bb, a.B + b * n * m, n, m, false, tid);
    ric_load<NB>(Xb, a.X + b * n * n, n, n, false, tid);
    ric_load<NB>(Kg, a.K + b * m * n, m, n, false, tid);
    ric_load<NB>(Tb, a.G_K ? a.G_K + b * m * n : nullptr, m, n, false, tid);
    ric_load<NB>(Lb, a.G_X ? a.G_X + b * n * n : nullptr, n, n, false, tid);
    __syncthreads();
    // M = R + B'XB = L L';  T = M^-1 G_K;  Mb = -T K'  (K: the gain in the form given);  K0 = the gain of form 0
    ric_mm<NB>(U1, NB, Xb, NB, 1, Bb, NB, 1, 1.0, 0.0, tid);              // X B   (kept to the end)
    ric_mm<NB>(U2, NB, Bb, 1, NB, U1, NB, 1, 1.0, 0.0, tid);
    const double *Rg = a.R + b * m * m;
    for (int e = tid; e < NN; e += RIC_NT) {
        const int i = e / NB, j = e % NB;
        U3[e] = (i < m && j < m ? Rg[i * m + j] : 0.0) + 0.5 * (U2[e] + U2[j * NB + i]);
    }
    __syncthreads();
    if (ric_chol<NB>(U3, m, tid) != 1) { zeros(0); return; }
    if (tid < n) ric_chol_solve_col<NB>(U3, m, Tb, NB, tid, true);
    __syncthreads();
    if (gf0) {
        for (int e = tid; e < NN; e += RIC_NT) K0[e] = Kg[e];
        __syncthreads();
    } else {
        ric_mm<NB>(K0, NB, Kg, NB, 1, Ab, NB, 1, 1.0, 0.0, tid);          // K = F A
    }
    ric_mm<NB>(Mb, NB, Tb, NB, 1, Kg, 1, NB, -1.0, 0.0, tid);
    // Xb = sym(G_X + B T A' + B Mb B')          (form 1: sym(G_X + sym(B T) + B sym(Mb) B'))
    ric_mm<NB>(U2, NB, Bb, NB, 1, Tb, NB, 1, 1.0, 0.0, tid);              // B T
    if (gf0) {
        ric_mm<NB>(Sb, NB, U2, NB, 1, Ab, 1, NB, 1.0, 0.0, tid);          // B T A'
        ric_mm<NB>(U2, NB, Bb, NB, 1, Mb, NB, 1, 1.0, 0.0, tid);          // B Mb
    } else {
        for (int e = tid; e < NN; e += RIC_NT) {
            const int i = e / NB, j = e % NB;
            Sb[e] = 0.5 * (U2[e] + U2[j * NB + i]);
            Acl[e] = 0.5 * (Mb[e] + Mb[j * NB + i]);
        }
        __syncthreads();
        ric_mm<NB>(U2, NB, Bb, NB, 1, Acl, NB, 1, 1.0, 0.0, tid);         // B sym(Mb)
    }
    ric_mm<NB>(Sb, NB, U2, NB, 1, Bb, 1, NB, 1.0, 1.0, tid);              // + (B Mb) B'
    for (int e = tid; e < NN; e += RIC_NT) U3[e] = Lb[e] + Sb[e];
    __syncthreads();
    for (int e = tid; e < NN; e += RIC_NT) { const int i = e / NB, j = e % NB; Lb[e] = 0.5 * (U3[e] + U3[j * NB + i]); }
    // Acl = A - B K0;  Lambda = Acl Lambda Acl' + Xb by Smith doubling: Lambda += S Lambda S', S <- S S
    ric_mm<NB>(Acl, NB, Bb, NB, 1, K0, NB, 1, -1.0, 0.0, tid);
    for (int e = tid; e < NN; e += RIC_NT) { Acl[e] += Ab[e]; Sb[e] = Acl[e]; }
    __syncthreads();
    int it = 0;
    bool conv = false;
    while (it < a.max_iter) {
        ric_mm<NB>(U2, NB, Sb, NB, 1, Lb, NB, 1, 1.0, 0.0, tid);
        ric_mm<NB>(U3, NB, U2, NB, 1, Sb, 1, NB, 1.0, 0.0, tid);          // S Lambda S'
        for (int e = tid; e < NN; e += RIC_NT) {
            const int i = e / NB, j = e % NB;
            const double d = 0.5 * (U3[e] + U3[j * NB + i]);
            U2[e] = d;
            Lb[e] += d;
        }
        ric_mm<NB>(Sb, NB, Sb, NB, 1, Sb, NB, 1, 1.0, 0.0, tid);          // (its barriers cover the loop above)
        ++it;
        const double dmax = ric_absmax(U2, NN, red, tid), lmax = ric_absmax(Lb, NN, red, tid), smax = ric_absmax(Sb, NN, red, tid);
        if (!(fmax(fmax(dmax, lmax), smax) < INFINITY)) break;
        if (dmax <= a.tol * fmax(1.0, lmax)) { conv = true; break; }
    }
    if (!conv) { zeros(it); return; }
    if (tid == 0 && a.iters) a.iters[b] = it;

    ric_store<NB>(dQ, Lb, n, n, tid);                                     // d_Q = Lambda
    ric_mm<NB>(U2, NB, Acl, NB, 1, Lb, NB, 1, 1.0, 0.0, tid);
    ric_mm<NB>(U3, NB, Xb, NB, 1, U2, NB, 1, 1.0, 0.0, tid);              // X Acl Lambda   (kept to the end)
    // d_A = X B T + 2 X Acl Lambda               (form 1: the direct term vanishes)
    if (dA != nullptr) {
        if (gf0) ric_mm<NB>(Sb, NB, U1, NB, 1, Tb, NB, 1, 1.0, 0.0, tid);
        for (int e = tid; e < NN; e += RIC_NT) Sb[e] = (gf0 ? Sb[e] : 0.0) + 2.0 * U3[e];
        __syncthreads();
        ric_store<NB>(dA, Sb, n, n, tid);
        __syncthreads();
    }
    // d_R = sym(Mb) + K0 Lambda K0'
    if (dR != nullptr) {
        ric_mm<NB>(U2, NB, K0, NB, 1, Lb, NB, 1, 1.0, 0.0, tid);
        ric_mm<NB>(Sb, NB, U2, NB, 1, K0, 1, NB, 1.0, 0.0, tid);
        for (int e = tid; e < m * m; e += RIC_NT) {
            const int i = e / m, j = e % m;
            dR[e] = 0.5 * (Mb[i * NB + j] + Mb[j * NB + i]) + 0.5 * (Sb[i * NB + j] + Sb[j * NB + i]);
        }
        __syncthreads();
    }
    // d_B = X A T' + X B (Mb + Mb') - 2 X Acl Lambda K0'          (form 1: the direct term is X T')
    if (dB != nullptr) {
        if (gf0) {
            ric_mm<NB>(U2, NB, Xb, NB, 1, Ab, NB, 1, 1.0, 0.0, tid);
            ric_mm<NB>(Sb, NB, U2, NB, 1, Tb, 1, NB, 1.0, 0.0, tid);
        } else {
            ric_mm<NB>(Sb, NB, Xb, NB, 1, Tb, 1, NB, 1.0, 0.0, tid);
        }
        for (int e = tid; e < NN; e += RIC_NT) { const int i = e / NB, j = e % NB; Acl[e] = Mb[e] + Mb[j * NB + i]; }
        __syncthreads();
        ric_mm<NB>(Sb, NB, U1, NB, 1, Acl, NB, 1, 1.0, 1.0, tid);
        ric_mm<NB>(Sb, NB, U3, NB, 1, K0, 1, NB, -2.0, 1.0, tid);
        ric_store<NB>(dB, Sb, n, m, tid);
    }
}
