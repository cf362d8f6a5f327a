// mpcqp_riccati_traj.h -- device code of the Riccati DIFFERENCE equation (include_ext3/mpcqp_riccati_traj.h), compiled in mpcqp_riccati.hip
// behind mpcqp_riccati.h, whose building blocks it uses (ric_mm, ric_chol, ric_chol_solve_col, ric_absmax, ric_store, ric_zero): one
// 256-thread workgroup runs one instance's recursion
//
//     S_t = R + B_t'X_t B_t,   K_t = S_t^-1 B_t'X_t A_t,   F_t = S_t^-1 B_t'X_t,   X_{t+1} = sym(A_t'X_t A_t - A_t'X_t B_t K_t + Q)
//
// over all T steps with X in LDS throughout, or the adjoint of it backwards over the forward's X trajectory.
// Every matrix is an NB x NB block in LDS as in mpcqp_riccati.h; the trajectory entries of the NEXT step travel from global memory into
// registers (RicRegs) while the step computes and reach LDS behind the step's last barrier.  Every loop is bounded by T, n, m or NB; no
// atomics; an instance's arithmetic depends on its own data alone; every sum over t runs in the one order of the walk.
#pragma once

struct DreArgs {                       // mpcqp_dre
    int n, m, T, gain_form, a_tv, b_tv;                  // a_tv / b_tv: A / B is a trajectory [T][batch][.][.] (else [batch][.][.])
    int batch;
    const double *A, *B, *Q, *R, *X0;
    double *X, *K;                                       // [T + 1][batch][n][n], [T][batch][m][n] (K: may be null)
    int32_t *status, *first_bad;
};

struct DreAdjArgs {                    // mpcqp_dre_adjoint
    int n, m, T, gain_form, a_tv, b_tv;
    int batch;
    const double *A, *B, *R, *X;
    const int32_t *status;
    const double *G_X, *G_K;                             // [T + 1][batch][n][n], [T][batch][m][n]; either may be null
    double *d_A, *d_B, *d_Q, *d_R, *d_X0;                // d_A, d_B: per entry where the input was a trajectory, else the sum over t
};

// one NB x NB block's share of a thread: element e = tid + k RIC_NT
template <int NB> struct RicRegs { double v[NB * NB / RIC_NT]; };

template <int NB>
__device__ __forceinline__ void ric_fetch(RicRegs<NB> &r, const double *src, int rows, int cols, int tid) {
#pragma unroll
    for (int k = 0; k < NB * NB / RIC_NT; ++k) {
        const int e = tid + k * RIC_NT, i = e / NB, j = e % NB;
        r.v[k] = (src != nullptr && i < rows && j < cols) ? src[i * cols + j] : 0.0;
    }
}

template <int NB>
__device__ __forceinline__ void ric_put(double *dst, const RicRegs<NB> &r, int tid) {
#pragma unroll
    for (int k = 0; k < NB * NB / RIC_NT; ++k) dst[tid + k * RIC_NT] = r.v[k];
}

// What a step of either walk needs of X_t, A_t, B_t (LDS) and R (global, m x m):  U1 = X B,  U2 = X A,  Sb = the Cholesky factor of
// S = R + sym(B'XB),  K0 = S^-1 B'XA,  Fb = S^-1 B'X,  with Tb (null: not there) <- S^-1 Tb and Pb (null: not wanted) = B'XA.
// Returns ric_chol's status.  The same instructions in both kernels: the adjoint's S, K, F are the forward's to the bit.
template <int NB>
__device__ __forceinline__ int dre_gains(const double *Xb, const double *Ab, const double *Bb, const double *Rg, double *U1, double *U2,
                                         double *Sb, double *K0, double *Fb, double *Pb, double *Tb, int n, int m, int tid) {
    constexpr int NN = NB * NB;
    ric_mm<NB>(U1, NB, Xb, NB, 1, Bb, NB, 1, 1.0, 0.0, tid);              // X B
    ric_mm<NB>(U2, NB, Xb, NB, 1, Ab, NB, 1, 1.0, 0.0, tid);              // X A
    ric_mm<NB>(K0, NB, Bb, 1, NB, U2, NB, 1, 1.0, 0.0, tid);              // B'XA
    ric_mm<NB>(Fb, NB, Bb, 1, NB, U1, NB, 1, 1.0, 0.0, tid);              // B'XB
    for (int e = tid; e < NN; e += RIC_NT) {
        const int i = e / NB, j = e % NB;
        Sb[e] = (i < m && j < m ? Rg[i * m + j] : 0.0) + 0.5 * (Fb[e] + Fb[j * NB + i]);
        if (Pb != nullptr) Pb[e] = K0[e];
    }
    __syncthreads();
    for (int e = tid; e < NN; e += RIC_NT) Fb[e] = U1[(e % NB) * NB + e / NB];      // B'X = (X B)'
    __syncthreads();
    const int st = ric_chol<NB>(Sb, m, tid);
    if (st != 1) return st;
    if (tid < (Tb != nullptr ? 3 : 2) * NB) ric_chol_solve_col<NB>(Sb, m, tid < NB ? K0 : (tid < 2 * NB ? Fb : Tb), NB, tid & (NB - 1), true);
    __syncthreads();
    return 1;
}

template <int NB> constexpr size_t ric_dre_lds() { return sizeof(double) * (11 * NB * NB + 4); }
template <int NB> constexpr size_t ric_dre_adjoint_lds() { return sizeof(double) * (19 * NB * NB + 4); }
static_assert(ric_dre_lds<32>() <= 160 * 1024 && ric_dre_adjoint_lds<32>() <= 160 * 1024, "an instance must fit one workgroup's LDS (160 KB on gfx950)");

template <int NB>
__global__ void __launch_bounds__(RIC_NT) k_dre(DreArgs a) {
    extern __shared__ double ric_lds[];
    constexpr int NN = NB * NB;
    double *Xb = ric_lds, *Ab = Xb + NN, *Bb = Ab + NN, *Qb = Bb + NN, *U1 = Qb + NN, *U2 = U1 + NN, *Sb = U2 + NN, *K0 = Sb + NN, *Fb = K0 + NN,
           *Pb = Fb + NN, *T3 = Pb + NN, *red = T3 + NN;
    const int tid = threadIdx.x, n = a.n, m = a.m, T = a.T;
    const size_t b = blockIdx.x, nb = (size_t)a.batch;
    const double *Rg = a.R + b * m * m;
    auto Aof = [&](int t) { return a.A + ((a.a_tv ? (size_t)t * nb : 0) + b) * n * n; };
    auto Bof = [&](int t) { return a.B + ((a.b_tv ? (size_t)t * nb : 0) + b) * n * m; };
    auto Xof = [&](int t) { return a.X + ((size_t)t * nb + b) * n * n; };
    auto Kof = [&](int t) { return a.K ? a.K + ((size_t)t * nb + b) * m * n : nullptr; };
    auto finish = [&](int st, int bad) {                 // an instance that ended early: zeros in the whole of both trajectories
        if (st != 1) {
            for (int t = 0; t <= T; ++t) ric_zero(Xof(t), n * n, tid);
            for (int t = 0; t < T; ++t) ric_zero(Kof(t), m * n, tid);
        }
        if (tid == 0) {
            a.status[b] = st;
            if (a.first_bad) a.first_bad[b] = bad;
        }
    };

    RicRegs<NB> ra, rb;
    ric_fetch<NB>(ra, a.X0 + b * n * n, n, n, tid);
    ric_put<NB>(U1, ra, tid);
    ric_fetch<NB>(ra, a.Q + b * n * n, n, n, tid);
    ric_put<NB>(Qb, ra, tid);
    ric_fetch<NB>(ra, Aof(0), n, n, tid);
    ric_put<NB>(Ab, ra, tid);
    ric_fetch<NB>(rb, Bof(0), n, m, tid);
    ric_put<NB>(Bb, rb, tid);
    __syncthreads();
    for (int e = tid; e < NN; e += RIC_NT) Xb[e] = 0.5 * (U1[e] + U1[(e % NB) * NB + e / NB]);
    __syncthreads();
    ric_store<NB>(Xof(0), Xb, n, n, tid);

    for (int t = 0; t < T; ++t) {
        const bool more = t + 1 < T;
        if (more && a.a_tv) ric_fetch<NB>(ra, Aof(t + 1), n, n, tid);     // in flight while the step computes
        if (more && a.b_tv) ric_fetch<NB>(rb, Bof(t + 1), n, m, tid);
        const int st = dre_gains<NB>(Xb, Ab, Bb, Rg, U1, U2, Sb, K0, Fb, Pb, nullptr, n, m, tid);
        if (st != 1) { finish(st, t); return; }
        ric_mm<NB>(T3, NB, Ab, 1, NB, U2, NB, 1, 1.0, 0.0, tid);          // A'XA
        ric_mm<NB>(T3, NB, Pb, 1, NB, K0, NB, 1, -1.0, 1.0, tid);         // - (B'XA)'K
        for (int e = tid; e < NN; e += RIC_NT) {
            const int et = (e % NB) * NB + e / NB;
            Xb[e] = 0.5 * ((T3[e] + Qb[e]) + (T3[et] + Qb[et]));
        }
        __syncthreads();
        const double xmax = ric_absmax(Xb, NN, red, tid), kmax = ric_absmax(K0, 2 * NN, red, tid);       // (K0 and Fb are neighbours)
        if (!(fmax(xmax, kmax) < INFINITY)) { finish(0, t); return; }
        ric_store<NB>(Xof(t + 1), Xb, n, n, tid);
        ric_store<NB>(Kof(t), a.gain_form == 0 ? K0 : Fb, m, n, tid);
        if (more && a.a_tv) ric_put<NB>(Ab, ra, tid);
        if (more && a.b_tv) ric_put<NB>(Bb, rb, tid);
        __syncthreads();
    }
    finish(1, -1);
}

// Backwards over t = T-1 .. 0 for the loss sum_t <G_X[t], X_t> + sum_t <G_K[t], gain_t>, Lambda = dL/dX_{t+1} (symmetric) carried in LDS.
// With T = S^-1 G_K[t], Mb = -T gain', Acl = A - B K:
//     Qbar += Lambda      Rbar += sym(Mb) + sym(K Lambda K')
//     d_A_t = 2 X Acl Lambda + X B T                                  (form 1: no direct term)
//     d_B_t = -2 X Acl Lambda K' + X B (Mb + Mb') + X A T'            (form 1: the last term is X T')
//     Lambda <- sym(G_X[t] + Acl Lambda Acl' + B T A' + B Mb B')      (form 1: sym(B T) + B sym(Mb) B' for the last two)
template <int NB>
__global__ void __launch_bounds__(RIC_NT) k_dre_adjoint(DreAdjArgs a) {
    extern __shared__ double ric_lds[];
    constexpr int NN = NB * NB;
    double *Ab = ric_lds, *Bb = Ab + NN, *Xb = Bb + NN, *K0 = Xb + NN, *Fb = K0 + NN, *Tb = Fb + NN, *Mb = Tb + NN, *Sb = Mb + NN, *Lam = Sb + NN,
           *Acl = Lam + NN, *U1 = Acl + NN, *U2 = U1 + NN, *U3 = U2 + NN, *U4 = U3 + NN, *U5 = U4 + NN, *Qa = U5 + NN, *Ra = Qa + NN, *dAa = Ra + NN,
           *dBa = dAa + NN, *red = dBa + NN;
    const int tid = threadIdx.x, n = a.n, m = a.m, T = a.T;
    const size_t b = blockIdx.x, nb = (size_t)a.batch;
    const bool gf0 = a.gain_form == 0, gk = a.G_K != nullptr;
    const double *Rg = a.R + b * m * m;
    const double *Kg = gf0 ? K0 : Fb;                    // the gain in the form the seed belongs to
    auto Aof = [&](int t) { return a.A + ((a.a_tv ? (size_t)t * nb : 0) + b) * n * n; };
    auto Bof = [&](int t) { return a.B + ((a.b_tv ? (size_t)t * nb : 0) + b) * n * m; };
    auto Xof = [&](int t) { return a.X + ((size_t)t * nb + b) * n * n; };
    auto GXof = [&](int t) { return a.G_X ? a.G_X + ((size_t)t * nb + b) * n * n : nullptr; };
    auto GKof = [&](int t) { return a.G_K ? a.G_K + ((size_t)t * nb + b) * m * n : nullptr; };
    auto dAof = [&](int t) { return a.d_A ? a.d_A + ((a.a_tv ? (size_t)t * nb : 0) + b) * n * n : nullptr; };
    auto dBof = [&](int t) { return a.d_B ? a.d_B + ((a.b_tv ? (size_t)t * nb : 0) + b) * n * m : nullptr; };
    double *dQ = a.d_Q ? a.d_Q + b * n * n : nullptr, *dR = a.d_R ? a.d_R + b * m * m : nullptr, *dX0 = a.d_X0 ? a.d_X0 + b * n * n : nullptr;
    auto zeros = [&]() {
        for (int t = 0; t < (a.a_tv ? T : 1); ++t) ric_zero(dAof(t), n * n, tid);
        for (int t = 0; t < (a.b_tv ? T : 1); ++t) ric_zero(dBof(t), n * m, tid);
        ric_zero(dQ, n * n, tid); ric_zero(dR, m * m, tid); ric_zero(dX0, n * n, tid);
    };
    if (a.status != nullptr && a.status[b] != 1) { zeros(); return; }

    RicRegs<NB> ra, rb, rx, rg, rt;                      // A, B, X, G_X, G_K of the step to come
    ric_fetch<NB>(rg, GXof(T), n, n, tid);
    ric_put<NB>(U1, rg, tid);
    ric_fetch<NB>(ra, Aof(T - 1), n, n, tid);
    ric_fetch<NB>(rb, Bof(T - 1), n, m, tid);
    ric_fetch<NB>(rx, Xof(T - 1), n, n, tid);
    ric_fetch<NB>(rg, GXof(T - 1), n, n, tid);
    ric_fetch<NB>(rt, GKof(T - 1), m, n, tid);
    ric_put<NB>(Ab, ra, tid); ric_put<NB>(Bb, rb, tid); ric_put<NB>(Xb, rx, tid); ric_put<NB>(Tb, rt, tid);
    for (int e = tid; e < NN; e += RIC_NT) Qa[e] = Ra[e] = dAa[e] = dBa[e] = Mb[e] = U5[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < NN; e += RIC_NT) Lam[e] = 0.5 * (U1[e] + U1[(e % NB) * NB + e / NB]);
    __syncthreads();

    for (int t = T - 1; t >= 0; --t) {
        const bool more = t > 0;
        const RicRegs<NB> gx = rg;                       // G_X[t]: used at the end of the step
        if (more) {
            if (a.a_tv) ric_fetch<NB>(ra, Aof(t - 1), n, n, tid);
            if (a.b_tv) ric_fetch<NB>(rb, Bof(t - 1), n, m, tid);
            ric_fetch<NB>(rx, Xof(t - 1), n, n, tid);
            ric_fetch<NB>(rg, GXof(t - 1), n, n, tid);
            if (gk) ric_fetch<NB>(rt, GKof(t - 1), m, n, tid);
        }
        if (dre_gains<NB>(Xb, Ab, Bb, Rg, U1, U2, Sb, K0, Fb, nullptr, gk ? Tb : nullptr, n, m, tid) != 1) { zeros(); return; }
        if (gk) ric_mm<NB>(Mb, NB, Tb, NB, 1, Kg, 1, NB, -1.0, 0.0, tid);                  // Mb = -T gain'
        for (int e = tid; e < NN; e += RIC_NT) Acl[e] = Ab[e];
        __syncthreads();
        ric_mm<NB>(Acl, NB, Bb, NB, 1, K0, NB, 1, -1.0, 1.0, tid);        // Acl = A - B K
        ric_mm<NB>(U4, NB, Acl, NB, 1, Lam, NB, 1, 1.0, 0.0, tid);        // Acl Lambda
        ric_mm<NB>(U3, NB, Xb, NB, 1, U4, NB, 1, 1.0, 0.0, tid);          // X Acl Lambda   (kept to the end of the step)
        ric_mm<NB>(Sb, NB, U4, NB, 1, Acl, 1, NB, 1.0, 0.0, tid);         // Acl Lambda Acl'   (the factor of S is done with)
        if (dR != nullptr) {
            ric_mm<NB>(U4, NB, K0, NB, 1, Lam, NB, 1, 1.0, 0.0, tid);
            ric_mm<NB>(U5, NB, U4, NB, 1, K0, 1, NB, 1.0, 0.0, tid);      // K Lambda K'
        }
        for (int e = tid; e < NN; e += RIC_NT) {
            const int et = (e % NB) * NB + e / NB;
            Qa[e] += Lam[e];
            if (dR != nullptr) Ra[e] += 0.5 * (Mb[e] + Mb[et]) + 0.5 * (U5[e] + U5[et]);
        }
        __syncthreads();
        if (a.d_A != nullptr) {
            if (gf0 && gk) ric_mm<NB>(U4, NB, U1, NB, 1, Tb, NB, 1, 1.0, 0.0, tid);        // X B T
            for (int e = tid; e < NN; e += RIC_NT) {
                const double g = (gf0 && gk ? U4[e] : 0.0) + 2.0 * U3[e];
                if (a.a_tv) U4[e] = g; else dAa[e] += g;
            }
            __syncthreads();
            if (a.a_tv) { ric_store<NB>(dAof(t), U4, n, n, tid); __syncthreads(); }
        }
        if (a.d_B != nullptr) {
            ric_mm<NB>(U5, NB, U3, NB, 1, K0, 1, NB, -2.0, 0.0, tid);     // -2 X Acl Lambda K'
            if (gk) {
                if (gf0) ric_mm<NB>(U5, NB, U2, NB, 1, Tb, 1, NB, 1.0, 1.0, tid);          // + X A T'
                else ric_mm<NB>(U5, NB, Xb, NB, 1, Tb, 1, NB, 1.0, 1.0, tid);              // + X T'
                for (int e = tid; e < NN; e += RIC_NT) U4[e] = Mb[e] + Mb[(e % NB) * NB + e / NB];
                __syncthreads();
                ric_mm<NB>(U5, NB, U1, NB, 1, U4, NB, 1, 1.0, 1.0, tid);  // + X B (Mb + Mb')
            }
            if (a.b_tv) { ric_store<NB>(dBof(t), U5, n, m, tid); __syncthreads(); }
            else { for (int e = tid; e < NN; e += RIC_NT) dBa[e] += U5[e]; __syncthreads(); }
        }
        // U5 = the gain seed's direct term in Xbar_t (zero without one)
        if (gk) {
            ric_mm<NB>(U4, NB, Bb, NB, 1, Tb, NB, 1, 1.0, 0.0, tid);      // B T
            if (gf0) {
                ric_mm<NB>(U5, NB, U4, NB, 1, Ab, 1, NB, 1.0, 0.0, tid);  // B T A'
                ric_mm<NB>(U4, NB, Bb, NB, 1, Mb, NB, 1, 1.0, 0.0, tid);  // B Mb
            } else {
                for (int e = tid; e < NN; e += RIC_NT) {
                    const int et = (e % NB) * NB + e / NB;
                    U5[e] = 0.5 * (U4[e] + U4[et]);
                    U2[e] = 0.5 * (Mb[e] + Mb[et]);                       // (X A is done with)
                }
                __syncthreads();
                ric_mm<NB>(U4, NB, Bb, NB, 1, U2, NB, 1, 1.0, 0.0, tid);  // B sym(Mb)
            }
            ric_mm<NB>(U5, NB, U4, NB, 1, Bb, 1, NB, 1.0, 1.0, tid);      // + (B Mb) B'
        }
#pragma unroll
        for (int k = 0; k < NN / RIC_NT; ++k) { const int e = tid + k * RIC_NT; U4[e] = gx.v[k] + (gk ? U5[e] : 0.0) + Sb[e]; }
        __syncthreads();
        for (int e = tid; e < NN; e += RIC_NT) Lam[e] = 0.5 * (U4[e] + U4[(e % NB) * NB + e / NB]);
        if (more) {
            if (a.a_tv) ric_put<NB>(Ab, ra, tid);
            if (a.b_tv) ric_put<NB>(Bb, rb, tid);
            ric_put<NB>(Xb, rx, tid);
            if (gk) ric_put<NB>(Tb, rt, tid);
        }
        __syncthreads();
    }
    const double lmax = fmax(fmax(ric_absmax(Lam, NN, red, tid), ric_absmax(Qa, 2 * NN, red, tid)), ric_absmax(dAa, 2 * NN, red, tid));
    if (!(lmax < INFINITY)) { zeros(); return; }         // (per-entry gradients that are not finite go with it)
    ric_store<NB>(dX0, Lam, n, n, tid);
    ric_store<NB>(dQ, Qa, n, n, tid);
    ric_store<NB>(dR, Ra, m, m, tid);
    if (!a.a_tv) ric_store<NB>(dAof(0), dAa, n, n, tid);
    if (!a.b_tv) ric_store<NB>(dBof(0), dBa, n, m, tid);
}
