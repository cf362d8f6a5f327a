// mpcqp_kpol.h -- part of libmpcqp_hip (included by mpcqp.hip, one translation unit).
// The regularized active-set KKT matrix that solution polishing (k_polish, mpcqp_polish.h) and the adjoint derivatives (k_adjoint,
// mpcqp_adjoint.h) both factor and solve with -- everything the two kernels share, written once:
//   K_pol = [P~ + delta I, A~r'; A~r, -delta I] with the constraint block eliminated and written in unscaled variables: the matrix the ADMM
//   factor has (K = c P + diag(s) + A' diag(omega) A, mpcqp.hip) with  s = delta / D^2  and  omega = E^2 / delta  on the active rows, 0 elsewhere.
// What the kernels do NOT share is around it: their multiplier sweeps against the unregularized system and when those stop.
#pragma once

constexpr int POLISH_INNER = 8;     // inner refinement steps of one KKT solve, at most
constexpr int ADJOINT_COLS = 4;     // right-hand sides of one solve: the columns of a 4x4x4 matrix instruction

// K_pol of every instance: the polish and the adjoint each own a set (kpol_alloc, mpcqp.hip)
struct KpolBufs {
    double *F;                    // [batch][fsz] the factor (generic block format)
    long long fsz;
    double *om, *s;               // [batch][m], [batch][n] the metric
    int *act;                     // [batch][m] state of a row: 0 inactive, 1 lower-active (the adjoint: or equality), 2 upper-active
    double *Bb, *Zb, *Sig, *gws;  // the held input's border (Nc < Np) and the 128-wide factorization's workspace
};
// K_pol of one instance, factored: what a solve takes
struct Kpol { const double *om, *sv, *F; BorderPtrs bp; };

// Host side: the layout K_pol is factored and solved in -- the handle's, with the register-resident and grouped formats off (they have no
// generic kkt_solve path) and a work area that holds the generic factorization's workspace and the solve's stage vectors.
static Lay polish_layout(const Lay &L) {
    Lay G = L;
    G.dense = 0; G.bcr = 0; G.bcrtop = 0; G.grp = 0; G.lstage = 0; G.nw = NWAVES;
    G.fstage = L.NB == 16 ? FactorFmt<16>::STAGE : L.NB == 32 ? FactorFmt<32>::STAGE : L.NB == 64 ? WideFmt::STAGE : HugeFmt::STAGE;
    G.fhead = L.NB == 16 ? FactorFmt<16>::HEAD : L.NB == 32 ? FactorFmt<32>::HEAD : 0;
    G.ffwd = L.NB == 16 ? FactorFmt<16>::FWD : L.NB == 32 ? FactorFmt<32>::FWD : L.NB == 64 ? WideFmt::NN : HugeFmt::NN;
    G.ftab = L.NB == 16 ? FactorFmt<16>::TAB : L.NB == 32 ? FactorFmt<32>::TAB : 0;
    const int fws = L.NB == 16 ? FactorCfg<16>::WS : L.NB == 32 ? FactorCfg<32>::WS : L.NB == 64 ? WideFmt::WS : HugeFmt::WS;
    G.tsz = std::max(std::max(L.m + L.N * L.NB * (L.NB >= 64 ? 2 : 1), fws), L.border ? 2 * L.nu * L.nu : 0);
    G.hot_lds = L.hot_sz;
    return G;
}
static long long polish_factor_doubles(const Lay &G) { return (long long)G.fhead + (long long)G.N * G.fstage; }

// OSQP's rule for row i in the scaled space, (z~, y~) = (E z, c y / E), (l~, u~) = (E l, E u): lower-active if z~ - l~ < -y~, else upper-active
// if u~ - z~ < y~; eq_always: a row with l == u is lower-active whatever its multiplier.  Returns the row's state, omega its weight in K_pol.
__device__ __forceinline__ int kpol_row(double e, double z, double y, double lo, double hi, double cc, double delta, bool eq_always, double &omega) {
    const double zs = e * z, ys = cc * y / e;
    const bool low = (eq_always && lo == hi) || zs - e * lo < -ys, upp = !low && (e * hi - zs < ys);
    omega = (low || upp) ? e * e / delta : 0.0;
    return low ? 1 : upp ? 2 : 0;
}

// Factor K_pol of instance b with the metric om, sv (the instance's slices of Q.om, Q.s, filled and visible) into Q's buffers; k: what the
// solves take.  False: a non-positive pivot.
template <int NB>
__device__ __forceinline__ bool kpol_factor(const Ctx &c, const KpolBufs &Q, int b, const double *om, const double *sv, double cc, const Smem &S, Kpol &k) {
    const Lay &L = c.L;
    BorderPtrs bp; bp.red = S.red;
    const size_t npb = (size_t)L.nu * L.N * L.NB;
    bp.Bb = L.border ? Q.Bb + b * npb : nullptr; bp.Zb = L.border ? Q.Zb + b * npb : nullptr;
    bp.Sig = L.border ? Q.Sig + (size_t)b * L.nu * L.nu : nullptr;
    bp.gws = NB == 128 ? Q.gws + (size_t)b * HugeFmt::GWS : nullptr;
    double *F = Q.F + (size_t)b * Q.fsz;
    k.om = om; k.sv = sv; k.F = F; k.bp = bp;
    return factor_all<NB>(c, om, sv, cc, F, S.T, S.iflag, bp) == 0;
}

// e = r - K_pol d, K_pol d = c P d + s . d + A' (omega . (A d)) matrix-free, for C right-hand sides at a time (C = 1, or ADJOINT_COLS with the
// columns in `mask` live): column col of a vector of n doubles lies col n further on; a row's coefficients are walked once for all its
// columns.  T: LDS, C m doubles.
template <int C>
__device__ __forceinline__ void kpol_residual(const Ctx &c, const double *om, const double *sv, double cc, unsigned mask, const double *ds, const double *rs,
                                              double *T, double *es) {
    const Lay &L = c.L;
    for (int i = threadIdx.x; i < L.m; i += NT) {
        double a[C];
#pragma unroll
        for (int col = 0; col < C; ++col) a[col] = 0.0;
        const double o = om[i];
        if (o != 0.0) A_row(c, i, [&](double co, int idx) {
#pragma unroll
            for (int col = 0; col < C; ++col) a[col] += co * ds[(size_t)col * L.n + idx];
        });
#pragma unroll
        for (int col = 0; col < C; ++col) if ((mask >> col) & 1u) T[col * L.m + i] = o * a[col];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < L.n; j += NT) {
        double pv[C], at[C];
#pragma unroll
        for (int col = 0; col < C; ++col) { pv[col] = 0.0; at[col] = 0.0; }
        P_row(c, j, [&](double co, int idx) {
#pragma unroll
            for (int col = 0; col < C; ++col) pv[col] += co * ds[(size_t)col * L.n + idx];
        });
        AT_row(c, j, [&](double co, int row) {
#pragma unroll
            for (int col = 0; col < C; ++col) at[col] += co * T[col * L.m + row];
        });
#pragma unroll
        for (int col = 0; col < C; ++col) {
            if (!((mask >> col) & 1u)) continue;
            const double kd = cc * pv[col] + sv[j] * ds[(size_t)col * L.n + j] + at[col];
            es[(size_t)col * L.n + j] = rs[(size_t)col * L.n + j] - kd;
        }
    }
    __syncthreads();
}

// kkt_solve (mpcqp_border.h) for the columns in `mask`: right-hand sides rg + col n -> solutions out + col n, through one pass of the
// column solve.  Tc: LDS, ADJOINT_COLS columns cs doubles apart (a column outside the mask is solved from zero and not read back).
template <int NB>
__device__ __forceinline__ void kkt_solve_cols(const Ctx &c, const double *om, const double *sv, double cc, const double *F,
                                               const double *rg, double *Tc, double *out, BorderPtrs bp, double *ubar, int cs, unsigned mask) {
    const Lay &L = c.L;
    const double cef = cc * c.eps_feas();
    for (int idx = threadIdx.x; idx < L.N * NB; idx += NT) {
        const int k = idx / NB, a = idx % NB;
        const bool isx = a < L.nx, isu = !isx && a < L.nb && k < L.Nc;
        const int e = isx ? k * L.nx + a : isu ? L.ou + k * L.nu + (a - L.nx) : 0;
        const double ws = isx ? om[L.rs + e] : 0.0, den = (isx && L.soft) ? cef + sv[L.oe + e] + ws : 1.0;
#pragma unroll
        for (int col = 0; col < ADJOINT_COLS; ++col) {
            const double *rc = rg + (size_t)col * L.n;
            double v = 0.0;
            if ((mask >> col) & 1u) {
                if (isx) {
                    double te = 0.0;
                    if (L.soft) { te = rc[L.oe + e] / den; out[(size_t)col * L.n + L.oe + e] = te; }
                    v = rc[e] - ws * te;
                } else if (isu) v = rc[e];
            }
            Tc[col * cs + idx] = v;
        }
    }
    __syncthreads();
    if (L.border) for (int col = 0; col < ADJOINT_COLS; ++col) if ((mask >> col) & 1u) border_pre<NB>(L, bp.Bb, bp.Zb, bp.Sig, Tc + col * cs, ubar + col * L.nu, bp.red);
    kkt_core_cols<NB>(core_args(L, F, om), Tc, cs);
    if (L.border) for (int col = 0; col < ADJOINT_COLS; ++col) if ((mask >> col) & 1u) border_post(L, NB, Tc + col * cs, ubar + col * L.nu);
    for (int idx = threadIdx.x; idx < L.N * NB; idx += NT) {
        const int k = idx / NB, a = idx % NB;
        const bool isx = a < L.nx, isu = !isx && a < L.nb && k < L.Nc;
        if (!isx && !isu) continue;
        const int e = isx ? k * L.nx + a : L.ou + k * L.nu + (a - L.nx);
        const double ws = isx ? om[L.rs + e] : 0.0, den = (isx && L.soft) ? cef + sv[L.oe + e] + ws : 1.0;
#pragma unroll
        for (int col = 0; col < ADJOINT_COLS; ++col) {
            if (!((mask >> col) & 1u)) continue;
            double *oc = out + (size_t)col * L.n;
            const double xe = Tc[col * cs + idx];
            oc[e] = xe;
            if (isx && L.soft) oc[L.oe + e] -= (ws / den) * xe;
        }
    }
    __syncthreads();
}

// The refined solve: ds = K~^-1 rs through the stored factor, then ds += K~^-1 (rs - K_pol ds) for at most POLISH_INNER steps, a column leaving
// when its correction is negligible (1e-13 of the solution), no longer halves, or is NaN (a broken factor: the caller sees it in ds).  For the
// columns in `mask` (C = 1: mask 1); es, dds: scratch vectors like ds; T: the LDS work area (C m doubles of rows, then the solve's stage
// vectors, for C > 1 cs doubles apart).  Every test is on reduced values: uniform over the workgroup.
template <int NB, int C>
__device__ __forceinline__ void kpol_solve(const Ctx &c, const Kpol &k, double cc, unsigned mask, const double *rs, double *ds, double *es, double *dds,
                                           const Smem &S, int cs) {
    const Lay &L = c.L;
    auto solve = [&](const double *rhs, double *sol, unsigned cols) {
        if constexpr (C > 1) kkt_solve_cols<NB>(c, k.om, k.sv, cc, k.F, rhs, S.T + C * L.m, sol, k.bp, S.tv, cs, cols);
        else kkt_solve<NB>(c, k.om, k.sv, cc, k.F, rhs, S.T + L.m, sol, k.bp, S.tv);
    };
    solve(rs, ds, mask);
    unsigned inl = mask;                          // the columns still being refined
    double last[C];
#pragma unroll
    for (int col = 0; col < C; ++col) last[col] = 0.0;
    for (int it = 0; it < POLISH_INNER && inl; ++it) {
        kpol_residual<C>(c, k.om, k.sv, cc, inl, ds, rs, S.T, es);
        solve(es, dds, inl);
        double mx[2 * C], dsm[C];
#pragma unroll
        for (int col = 0; col < C; ++col) { mx[2 * col] = 0.0; mx[2 * col + 1] = 0.0; dsm[col] = 0.0; }
        for (int j = threadIdx.x; j < L.n; j += NT) {
#pragma unroll
            for (int col = 0; col < C; ++col) {
                if (!((inl >> col) & 1u)) continue;
                const double dv = dds[(size_t)col * L.n + j], v = ds[(size_t)col * L.n + j] + dv;
                ds[(size_t)col * L.n + j] = v; mx[2 * col] = fmax(mx[2 * col], fabs(dv)); mx[2 * col + 1] = fmax(mx[2 * col + 1], fabs(v)); dsm[col] += dv;
            }
        }
        block_reduce<2 * C, C>(mx, dsm, S.red);
#pragma unroll
        for (int col = 0; col < C; ++col) {
            if (!((inl >> col) & 1u)) continue;
            if (dsm[col] != dsm[col] || mx[2 * col] <= 1e-13 * mx[2 * col + 1] || (it > 0 && mx[2 * col] > 0.5 * last[col])) inl &= ~(1u << col);
            last[col] = mx[2 * col];
        }
    }
}
