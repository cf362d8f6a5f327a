// mpcqp_adjoint.h -- part of libmpcqp_hip (included by mpcqp.hip, one translation unit; C ABI in include/mpcqp_adjoint.h).
// Adjoint derivatives of the QP solution: a sibling of k_polish (mpcqp_polish.h) -- the same active-set rule, the same regularized matrix
// K_pol in the same generic block format, the same refined solves -- with another right-hand side and a chain rule behind it.
// One 256-thread workgroup per instance, FP64, in the handle's SCALED space:
//   active set   from the ADMM iterate by polishing's rule, plus every equality row (l == u) whatever its multiplier; n_weak counts the rows
//                with l != u that sit on a bound with a zero multiplier (unscaled units: include/mpcqp_adjoint.h);
//   K_pol        s = delta / D^2, omega = E^2 / delta on the active rows, 0 elsewhere, factored ONCE by factor_all into the adjoint's own buffers;
//   per seed g   [P, A_a'; A_a, 0] [r_w; r_y] = [g; 0]: one solve from zero, then `refine` sweeps in residual form against the unregularized
//                system (the multiplier sweep of k_eq_solve / k_polish with q = -g and every target 0), each KKT solve refined against K_pol
//                itself, applied matrix-free, until its correction stalls (polish_kmul: K_pol is conditioned 1e9 .. 1e12).  Where the
//                last of them still moved the answer (nearly dependent active rows: three sweeps left r_y 2e-6 off on random_5_3_8, 5e-7
//                on the 200-step cart pole; rows held by a slack variable contract by about 0.5 a sweep) up to extra_iter more follow,
//                until the correction is negligible or stops shrinking;
//   results      dL/dq = -r_w, dL/db = r_y, and the chain rule into x0, u_{-1}, xref, uref (build_q / row_bounds read backwards): reductions
//                over the stage blocks with Qx, QxN, Qu, QDu from the model blob.
// mpcqp_gains runs the nu unit seeds of the u_0 block against the one factor.  For stages of at most 32 (NB = 16, 32) they go FOUR TO A SOLVE:
// in a mat-vec the generic solve's matrix instructions carry the stage vector replicated over their four right-hand-side columns, and
// the column variant of the solve (kkt_core_cols, mpcqp_sweeps.h) puts a seed into each of them -- the work area holds four stage-major
// vectors, lane j sweeps column j.  The residuals, K_pol products and updates around the solves walk each row's coefficients once for all
// four columns; a column whose correction has converged or stalled is frozen while the others go on.  Wider stages (NB = 64, 128: another solve, no idle column) and work areas
// that four columns would push past a workgroup's LDS loop over the seeds one at a time.
// Nothing of the handle is written: not the iterate, the solution, info, the factor, rho, the polish's buffers or the counters.
#pragma once

constexpr int ADJOINT_COLS = 4;     // right-hand sides of one solve: the columns of a 4x4x4 matrix instruction

struct AdjointArgs {
    double *F;                    // [batch][fsz] the factor of K_pol (generic block format)
    long long fsz;
    double *om, *s;               // [batch][m], [batch][n] the metric of K_pol
    double *x, *y;                // [batch][COLS][n], [batch][COLS][m] r_w, r_y of the seeds in progress
    double *r, *d, *e, *dd;       // [batch][COLS][n] x4 residual / correction of a sweep, and of the inner refinement of its KKT solve
    double *gt;                   // [batch][COLS][m] c y + omega (A x) of the active rows as the sweep's residual saw it
    double *g;                    // [batch][COLS][n] the seeds in progress
    int *act;                     // [batch][m] 0 inactive, 1 lower-active or equality, 2 upper-active
    double *Bb, *Zb, *Sig, *gws;  // the held input's border (Nc < Np) and the 128-wide factorization's workspace, of K_pol
    const double *gw, *gu0;       // [batch][n], [batch][nu] the caller's seeds (either may be null); gains: both null, seed j = unit vector of u_0[j]
    double *ox0, *oum1, *oxref, *ouref;      // [batch][nseeds][nx | nu | xref_rows nx | nu] chained gradients (chain = 1)
    double *oq, *ol, *ou;         // [batch][n], [batch][m] x2 raw gradients of seed 0 (null: not wanted)
    int *nact, *nweak, *status;   // [batch]
    double delta, weak_tol; int refine, extra, nseeds, chain;      // (extra: sweeps beyond refine, at most)
    int ncol, cs;                 // seeds per solve (1 or ADJOINT_COLS) and the distance of their columns in the work area
};

// The passes around the solves, for C seeds at a time (C = 1, or ADJOINT_COLS with the columns in `mask` live): column col of a vector of
// n (m) doubles lies col n (col m) further on; a row's coefficients are walked once for all its columns.  T: LDS, C m doubles.
// gt = c y + omega (A x) on the active rows, 0 elsewhere (mm_row_residual with every target 0), kept in gts for the multiplier update;
// r = c (g - P x) - A' gt: mm_var_residual with q = -g over ALL n variables (a seed may touch the slack variables, whose linear cost
// the solver never carries)
template <int C>
__device__ __forceinline__ void adjoint_residual(const Ctx &c, const int *act, const double *om, double cc, unsigned mask, const double *xs, const double *ys,
                                                 const double *gs, double *T, double *gts, double *rs) {
    const Lay &L = c.L;
    for (int i = threadIdx.x; i < L.m; i += NT) {
        double ax[C];
#pragma unroll
        for (int col = 0; col < C; ++col) ax[col] = 0.0;
        const bool on = act[i] != 0;
        if (on) A_row(c, i, [&](double co, int idx) {
#pragma unroll
            for (int col = 0; col < C; ++col) ax[col] += co * xs[(size_t)col * L.n + idx];
        });
#pragma unroll
        for (int col = 0; col < C; ++col) {
            if (!((mask >> col) & 1u)) continue;
            const double v = on ? cc * ys[(size_t)col * L.m + i] + om[i] * ax[col] : 0.0;
            T[col * L.m + i] = v; gts[(size_t)col * L.m + i] = v;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < L.n; j += NT) {
        double px[C], atg[C];
#pragma unroll
        for (int col = 0; col < C; ++col) { px[col] = 0.0; atg[col] = 0.0; }
        P_row(c, j, [&](double co, int idx) {
#pragma unroll
            for (int col = 0; col < C; ++col) px[col] += co * xs[(size_t)col * L.n + idx];
        });
        AT_row(c, j, [&](double co, int row) {
#pragma unroll
            for (int col = 0; col < C; ++col) atg[col] += co * T[col * L.m + row];
        });
#pragma unroll
        for (int col = 0; col < C; ++col)
            if ((mask >> col) & 1u) rs[(size_t)col * L.n + j] = cc * (gs[(size_t)col * L.n + j] - px[col]) - atg[col];
    }
    __syncthreads();
}
// e = r - K_pol d, K_pol d = c P d + s . d + A' (omega . (A d)) matrix-free (polish_kmul and the subtraction behind it)
template <int C>
__device__ __forceinline__ void adjoint_kres(const Ctx &c, const double *om, const double *sv, double cc, unsigned mask, const double *ds, const double *rs,
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

template <int NB>
__global__ __launch_bounds__(NT) void k_adjoint(Lay L, Ptrs P, AdjointArgs Q) {
    extern __shared__ __attribute__((aligned(16))) double sh[];
    double *p = sh; Smem S; smem_common(L, P, p, S);       // (P.perm is null: workgroup b works on instance b)
    const int b = blockIdx.x, tid = threadIdx.x, ns = Q.nseeds;
    const mpcqp_info inf = P.info[b];
    const int xw = L.xref_rows * L.nx;
    double *ox0 = Q.ox0 + (size_t)b * ns * L.nx, *oum1 = Q.oum1 + (size_t)b * ns * L.nu, *ouref = Q.ouref + (size_t)b * ns * L.nu;
    double *oxref = Q.oxref + (size_t)b * ns * xw;
    double *oq = Q.oq ? Q.oq + (size_t)b * L.n : nullptr, *ol = Q.ol ? Q.ol + (size_t)b * L.m : nullptr, *ou = Q.ou ? Q.ou + (size_t)b * L.m : nullptr;
    int st = 0, nact = 0, nweak = 0;
    if (inf.status == MPCQP_SOLVED) {
        const double *model = P.model + (size_t)b * L.model_sz, *step = P.step + (size_t)b * L.step_sz;
        load_common(L, model, step, S);
        Ctx c{L, S.hot, model + L.hot_sz};
        const double *D = P.D + (size_t)b * L.n, *E = P.E + (size_t)b * L.m;
        const double cc = P.c[b], delta = Q.delta;
        const double *za = P.z + (size_t)b * L.m, *ya = P.y + (size_t)b * L.m;      // the ADMM iterate (unscaled)
        double *om = Q.om + (size_t)b * L.m, *sv = Q.s + (size_t)b * L.n;
        int *act = Q.act + (size_t)b * L.m;
        const size_t vn = (size_t)b * ADJOINT_COLS * L.n, vm = (size_t)b * ADJOINT_COLS * L.m;      // (column col of a vector: + col n, + col m)
        double *xs = Q.x + vn, *ys = Q.y + vm, *gs = Q.g + vn, *gts = Q.gt + vm;
        double *rs = Q.r + vn, *ds = Q.d + vn, *es = Q.e + vn, *dds = Q.dd + vn;
        // 1. active set (polishing's rule in the scaled space; equality rows always), weak rows, the metric of K_pol
        double ymx[1] = {0.0}, cnt[2] = {0.0, 0.0};
        for (int i = tid; i < L.m; i += NT) ymx[0] = fmax(ymx[0], fabs(ya[i]));
        block_reduce<1, 2>(ymx, cnt, S.red);
        const double ytol = Q.weak_tol * fmax(1.0, ymx[0]);
        for (int i = tid; i < L.m; i += NT) {
            double lo, hi; row_bounds(c, S.x0s, S.du0, i, lo, hi);
            const double ev = E[i], zv = za[i], yv = ya[i], zs = ev * zv, ys = cc * yv / ev;
            const bool eq = lo == hi;
            const bool low = eq || zs - ev * lo < -ys, upp = !low && (ev * hi - zs < ys);
            act[i] = low ? 1 : upp ? 2 : 0;
            om[i] = (low || upp) ? ev * ev / delta : 0.0;
            if (low || upp) cnt[0] += 1.0;
            if (!eq && fmin(zv - lo, hi - zv) <= Q.weak_tol * fmax(1.0, fabs(zv)) && fabs(yv) <= ytol) cnt[1] += 1.0;
        }
        for (int j = tid; j < L.n; j += NT) sv[j] = delta / (D[j] * D[j]);
        block_reduce<1, 2>(ymx, cnt, S.red);             // (ends with a barrier: act, om, sv are visible)
        nact = (int)cnt[0]; nweak = (int)cnt[1];
        // 2. factor K_pol once (generic block format, own buffers)
        BorderPtrs bp; bp.red = S.red;
        const size_t npb = (size_t)L.nu * L.N * L.NB;
        bp.Bb = L.border ? Q.Bb + b * npb : nullptr; bp.Zb = L.border ? Q.Zb + b * npb : nullptr;
        bp.Sig = L.border ? Q.Sig + (size_t)b * L.nu * L.nu : nullptr;
        bp.gws = NB == 128 ? Q.gws + (size_t)b * HugeFmt::GWS : nullptr;
        double *F = Q.F + (size_t)b * Q.fsz;
        bool bad = factor_all<NB>(c, om, sv, cc, F, S.T, S.iflag, bp) != 0;
        // 3. the seeds, C to a solve: one solve from zero, then the refinement sweeps against the unregularized system
        auto seeds = [&](auto ctag) {
            constexpr int C = decltype(ctag)::value;
            auto solve = [&](const double *rhs, double *sol, unsigned mask) {      // the columns in `mask` of rhs -> sol
                if constexpr (C > 1) kkt_solve_cols<NB>(c, om, sv, cc, F, rhs, S.T + C * L.m, sol, bp, S.tv, Q.cs, mask);
                else kkt_solve<NB>(c, om, sv, cc, F, rhs, S.T + L.m, sol, bp, S.tv);
            };
            for (int s0 = 0; s0 < ns && !bad; s0 += C) {
                const int nc = min(C, ns - s0);
                for (int j = tid; j < L.n; j += NT) {
#pragma unroll
                    for (int col = 0; col < C; ++col) {
                        double v = 0.0;
                        if (!Q.gw && !Q.gu0) v = (j == L.ou + s0 + col) ? 1.0 : 0.0;
                        else {
                            if (Q.gw) v = Q.gw[(size_t)b * L.n + j];
                            if (Q.gu0 && j >= L.ou && j < L.ou + L.nu) v += Q.gu0[(size_t)b * L.nu + (j - L.ou)];
                        }
                        gs[(size_t)col * L.n + j] = v; xs[(size_t)col * L.n + j] = 0.0;      // (a column beyond the last seed is filled and never swept)
                    }
                }
                for (int i = tid; i < C * L.m; i += NT) ys[i] = 0.0;
                __syncthreads();
                double lastrel[C];
#pragma unroll
                for (int col = 0; col < C; ++col) lastrel[col] = 0.0;
                unsigned live = (1u << nc) - 1u;                 // the columns still sweeping (uniform over the workgroup: every test is on reduced values)
                for (int sw = 0; sw <= Q.refine + Q.extra && live && !bad; ++sw) {
                    adjoint_residual<C>(c, act, om, cc, live, xs, ys, gs, S.T, gts, rs);
                    solve(rs, ds, live);
                    unsigned inl = live;                          // the columns whose KKT solve is still being refined
                    double last[C];
#pragma unroll
                    for (int col = 0; col < C; ++col) last[col] = 0.0;
                    for (int it = 0; it < POLISH_INNER && inl; ++it) {     // d += K~^-1 (r - K_pol d) until the correction is negligible or stops shrinking
                        adjoint_kres<C>(c, om, sv, cc, inl, ds, rs, S.T, es);
                        solve(es, dds, inl);
                        double mx[2 * C], dsm[C];
#pragma unroll
                        for (int col = 0; col < C; ++col) { mx[2 * col] = 0.0; mx[2 * col + 1] = 0.0; dsm[col] = 0.0; }
                        for (int j = tid; j < L.n; j += NT) {
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
                    double dsum[C], cm[4 * C];                    // per column |d|, |x|, |dy|, |y|
#pragma unroll
                    for (int col = 0; col < C; ++col) { dsum[col] = 0.0; cm[4 * col] = 0.0; cm[4 * col + 1] = 0.0; cm[4 * col + 2] = 0.0; cm[4 * col + 3] = 0.0; }
                    for (int j = tid; j < L.n; j += NT) {
#pragma unroll
                        for (int col = 0; col < C; ++col) {
                            if (!((live >> col) & 1u)) continue;
                            const double dv = ds[(size_t)col * L.n + j], v = xs[(size_t)col * L.n + j] + dv;
                            xs[(size_t)col * L.n + j] = v; dsum[col] += dv; cm[4 * col] = fmax(cm[4 * col], fabs(dv)); cm[4 * col + 1] = fmax(cm[4 * col + 1], fabs(v));
                        }
                    }
                    __syncthreads();
                    // y += (omega / c) A (x + d) on the active rows, formed as (gt + omega A d) / c: A x is taken as the residual took it and only A d,
                    // whose rounding is that of the small correction, is evaluated anew -- so the multiplier is the one the solve just made
                    // stationary.  (mm_dual_update's fresh A (x + d) differs from it by the rounding of A x times omega / c = E^2 / (c delta), up to
                    // 1e8: 1.5e-8 of r_y on random_12_4_30, 2e-9 on quadcopter_nodu.)
                    for (int i = tid; i < L.m; i += NT) {
                        if (!act[i]) continue;
                        double ad[C];
#pragma unroll
                        for (int col = 0; col < C; ++col) ad[col] = 0.0;
                        A_row(c, i, [&](double co, int idx) {
#pragma unroll
                            for (int col = 0; col < C; ++col) ad[col] += co * ds[(size_t)col * L.n + idx];
                        });
#pragma unroll
                        for (int col = 0; col < C; ++col) {
                            if (!((live >> col) & 1u)) continue;
                            const double v = (gts[(size_t)col * L.m + i] + om[i] * ad[col]) / cc, dy = v - ys[(size_t)col * L.m + i];
                            ys[(size_t)col * L.m + i] = v; cm[4 * col + 2] = fmax(cm[4 * col + 2], fabs(dy)); cm[4 * col + 3] = fmax(cm[4 * col + 3], fabs(v));
                        }
                    }
                    if constexpr (C == 1) block_reduce<4, 1>(cm, dsum, S.red);
                    else { double none[1] = {0.0}; block_reduce<8, C>(cm, dsum, S.red); block_reduce<4 * C - 8, 1>(cm + 8, none, S.red); }
                    // refine_iter sweeps at least; then on while the correction is neither negligible (1e-12 of the solution, 1e-10 of r_y) nor stalled --
                    // nearly dependent active rows contract r_y by only 1e-2 .. 1e-1 a sweep, rows held by a slack variable (a violated soft state box:
                    // eps_feas against delta) by about 0.5: "stalled" is a correction that no longer shrinks by a tenth, not one that fails to halve.
                    // r_w's correction is measured against the whole solution (|r_w|, c |r_y|, both scaled): where the seed's input sits on a bound r_w is
                    // zero but for rounding and its own relative change says nothing.  A column that is done keeps what it has.
#pragma unroll
                    for (int col = 0; col < C; ++col) {
                        if (!((live >> col) & 1u)) continue;
                        if (dsum[col] != dsum[col]) bad = true;        // (a NaN correction: a broken factor)
                        const double rel = fmax(cm[4 * col] / fmax(fmax(cm[4 * col + 1], cc * cm[4 * col + 3]), 1e-300), 1e-2 * cm[4 * col + 2] / fmax(cm[4 * col + 3], 1e-300));
                        if (sw >= Q.refine && (rel <= 1e-12 || rel > 0.9 * lastrel[col])) live &= ~(1u << col);
                        lastrel[col] = rel;
                    }
                }
                if (bad) break;
                // 4. dL/dq, dL/dl, dL/du and the chain rule into the controller's parameters
                for (int col = 0; col < nc; ++col) {
                    const int sd = s0 + col;
                    const double *x = xs + (size_t)col * L.n, *y = ys + (size_t)col * L.m;
                    if (sd == 0) {
                        if (oq) for (int j = tid; j < L.n; j += NT) oq[j] = -x[j];
                        if (ol && ou) for (int i = tid; i < L.m; i += NT) { const int a = act[i]; ol[i] = a == 1 ? y[i] : 0.0; ou[i] = a == 2 ? y[i] : 0.0; }
                    }
                    if (Q.chain) {
                        const double *Qu = c.Qu(), *QDu = c.QDu();
                        for (int i = tid; i < L.nx; i += NT) ox0[sd * L.nx + i] = -y[i];      // l[:nx] = u[:nx] = -x0
                        for (int l = tid; l < L.nu; l += NT) {
                            double a = y[L.rdu + l];                  // the first Delta-u rows' bounds are Dumin / Dumax + u_{-1} (0 where the row is inactive)
                            for (int jj = 0; jj < L.nu; ++jj) a += QDu[jj * L.nu + l] * x[L.ou + jj];      // q_U[0:nu] += -QDu u_{-1}
                            oum1[sd * L.nu + l] = a;
                            double ur = 0.0;                          // q_U[k] = -iU_k Qu uref
                            for (int k = 0; k < L.Nc; ++k) {
                                const double iu = (k == L.Nc - 1) ? (double)(L.Np - L.Nc + 1) : 1.0;
                                double t = 0.0;
                                for (int jj = 0; jj < L.nu; ++jj) t += Qu[jj * L.nu + l] * x[L.ou + k * L.nu + jj];
                                ur += iu * t;
                            }
                            ouref[sd * L.nu + l] = ur;
                        }
                        if (L.xref_rows == 1) {                       // q_X[k] = -Q_k xref
                            for (int l = tid; l < L.nx; l += NT) {
                                double a = 0.0;
                                for (int k = 0; k < L.N; ++k) {
                                    const double *Qk = (k < L.Np) ? c.Qx() : c.QxN();
                                    for (int i = 0; i < L.nx; ++i) a += Qk[i * L.nx + l] * x[k * L.nx + i];
                                }
                                oxref[sd * xw + l] = a;
                            }
                        } else {                                      // q_X[k] = -(xref_k' Q_k)'
                            for (int idx = tid; idx < L.N * L.nx; idx += NT) {
                                const int k = idiv(idx, L.rnx), l = idx - k * L.nx;
                                const double *Qk = (k < L.Np) ? c.Qx() : c.QxN();
                                double a = 0.0;
                                for (int i = 0; i < L.nx; ++i) a += Qk[l * L.nx + i] * x[k * L.nx + i];
                                oxref[sd * xw + idx] = a;
                            }
                        }
                    }
                }
                __syncthreads();
            }
        };
        if (!bad) {
            if constexpr (NB <= 32) { if (Q.ncol > 1) seeds(std::integral_constant<int, ADJOINT_COLS>{}); else seeds(std::integral_constant<int, 1>{}); }
            else seeds(std::integral_constant<int, 1>{});
        }
        st = bad ? -1 : 1;
    }
    if (st != 1) {                                            // not computed: every output is zero
        if (oq) for (int j = tid; j < L.n; j += NT) oq[j] = 0.0;
        if (ol && ou) for (int i = tid; i < L.m; i += NT) { ol[i] = 0.0; ou[i] = 0.0; }
        if (Q.chain) {
            for (int i = tid; i < ns * L.nx; i += NT) ox0[i] = 0.0;
            for (int i = tid; i < ns * L.nu; i += NT) { oum1[i] = 0.0; ouref[i] = 0.0; }
            for (int i = tid; i < ns * xw; i += NT) oxref[i] = 0.0;
        }
    }
    if (tid == 0) { Q.status[b] = st; Q.nact[b] = nact; Q.nweak[b] = nweak; }
}
