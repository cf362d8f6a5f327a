// mpcqp_adjoint.h -- part of libmpcqp_hip (included by mpcqp.hip, one translation unit; C ABI in include/mpcqp_adjoint.h).
// Adjoint derivatives of the QP solution: a sibling of k_polish (mpcqp_polish.h) on the same K_pol (mpcqp_kpol.h: the active-set rule kpol_row,
// the factorization kpol_factor, the refined solve kpol_solve) -- with another right-hand side and a chain rule behind it.
// One 256-thread workgroup per instance, FP64, in the handle's SCALED space:
//   active set   from the ADMM iterate by polishing's rule, plus every equality row (l == u) whatever its multiplier; n_weak counts the rows
//                with l != u that sit on a bound with a zero multiplier (unscaled units: include/mpcqp_adjoint.h);
//   K_pol        s = delta / D^2, omega = E^2 / delta on the active rows, 0 elsewhere, factored ONCE into the adjoint's own buffers;
//   per seed g   [P, A_a'; A_a, 0] [r_w; r_y] = [g; 0]: one solve from zero, then `refine` sweeps in residual form against the unregularized
//                system (the multiplier sweep of k_eq_solve / k_polish with q = -g and every target 0), each KKT solve refined against K_pol
//                itself, applied matrix-free, until its correction stalls (kpol_solve: K_pol is conditioned 1e9 .. 1e12).  Where the
//                last of them still moved the answer (nearly dependent active rows: three sweeps left r_y 2e-6 off on random_5_3_8, 5e-7
//                on the 200-step cart pole; rows held by a slack variable contract by about 0.5 a sweep) up to extra_iter more follow,
//                until the correction is negligible or stops shrinking (adjoint_update);
//   results      dL/dq = -r_w, dL/db = r_y, and the chain rule into x0, u_{-1}, xref, uref (build_q / row_bounds read backwards): reductions
//                over the stage blocks with Qx, QxN, Qu, QDu from the model blob (adjoint_outputs); zeros where nothing was computed
//                (adjoint_zero).
// mpcqp_gains runs the nu unit seeds of the u_0 block against the one factor.  For stages of at most 32 (NB = 16, 32) they go FOUR TO A SOLVE:
// in a mat-vec the generic solve's matrix instructions carry the stage vector replicated over their four right-hand-side columns, and
// the column variant of the solve (kkt_core_cols, mpcqp_sweeps.h) puts a seed into each of them -- the work area holds four stage-major
// vectors, lane j sweeps column j.  The residuals, K_pol products and updates around the solves walk each row's coefficients once for all
// four columns; a column whose correction has converged or stalled is frozen while the others go on.  Wider stages (NB = 64, 128: another solve, no idle column) and work areas
// that four columns would push past a workgroup's LDS loop over the seeds one at a time.
// Nothing of the handle is written: not the iterate, the solution, info, the factor, rho, the polish's buffers or the counters.
#pragma once

struct AdjointArgs {
    KpolBufs K;                   // K_pol: factor, metric, active set (equality rows count as lower-active)
    double *x, *y;                // [batch][COLS][n], [batch][COLS][m] r_w, r_y of the seeds in progress
    double *r, *d, *e, *dd;       // [batch][COLS][n] x4 residual / correction of a sweep, and of the inner refinement of its KKT solve
    double *gt;                   // [batch][COLS][m] c y + omega (A x) of the active rows as the sweep's residual saw it
    double *g;                    // [batch][COLS][n] the seeds in progress
    const double *gw, *gu0;       // [batch][n], [batch][nu] the caller's seeds (either may be null); gains: both null, seed j = unit vector of u_0[j]
    double *ox0, *oum1, *oxref, *ouref;      // [batch][nseeds][nx | nu | xref_rows nx | nu] chained gradients (chain = 1)
    double *oq, *ol, *ou;         // [batch][n], [batch][m] x2 raw gradients of seed 0 (null: not wanted)
    int *nact, *nweak, *status;   // [batch]
    double delta, weak_tol; int refine, extra, nseeds, chain;      // (extra: sweeps beyond refine, at most)
    int ncol, cs;                 // seeds per solve (1 or ADJOINT_COLS) and the distance of their columns in the work area
    double *od;                   // [batch][nseeds][d_rows nx] the gradient of the affine term per seed (mpcqp_gains_affine, include_ext5/mpcqp_rollout_affine.h), or null:
                                  // the work area keeps only the last group of seeds, so K_d is written where the group's other outputs are
};

// Seed sd's r_y = y into its row of the term's gradient: k_affine_grad's rule (mpcqp_affine.h) -- -r_y of row blocks 1 .. Np, d_rows = 1: summed in ascending order
__device__ __forceinline__ void adjoint_affine_out(const Lay &L, const double *y, double *o) {
    const int w = L.d_rows * L.nx;
    const double *ry = y + L.nx;
    for (int e = threadIdx.x; e < w; e += NT) {
        double acc = 0.0;
        if (L.d_rows > 1) acc = -ry[e];
        else for (int k = 0; k < L.Np; ++k) acc -= ry[k * L.nx + e];
        o[e] = acc;
    }
}

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

// The seeds s0 .. s0 + C - 1 into gs: the instance's g_w [n] / g_u0 [nu] (either may be null), or with both null the unit vectors of u_0
// (the gains); xs = ys = 0.  A column beyond the last seed is filled and never swept.
template <int C>
__device__ __forceinline__ void adjoint_seeds(const Lay &L, const double *gw, const double *gu0, int s0, double *gs, double *xs, double *ys) {
    for (int j = threadIdx.x; j < L.n; j += NT) {
#pragma unroll
        for (int col = 0; col < C; ++col) {
            double v = 0.0;
            if (!gw && !gu0) v = (j == L.ou + s0 + col) ? 1.0 : 0.0;
            else {
                if (gw) v = gw[j];
                if (gu0 && j >= L.ou && j < L.ou + L.nu) v += gu0[j - L.ou];
            }
            gs[(size_t)col * L.n + j] = v; xs[(size_t)col * L.n + j] = 0.0;
        }
    }
    for (int i = threadIdx.x; i < C * L.m; i += NT) ys[i] = 0.0;
    __syncthreads();
}

// The end of a sweep for the columns in `live`: x += d, the multiplier update, and the stop rule (may_stop: refine_iter sweeps are done).
// Returns the columns that go on; bad: a NaN correction (a broken factor).  Every test is on reduced values: uniform over the workgroup.
template <int C>
__device__ __forceinline__ unsigned adjoint_update(const Ctx &c, const int *act, const double *om, double cc, unsigned live, bool may_stop, double *xs, double *ys,
                                                   const double *ds, const double *gts, double *red, double (&lastrel)[C], bool &bad) {
    const Lay &L = c.L;
    double dsum[C], cm[4 * C];                    // per column |d|, |x|, |dy|, |y|
#pragma unroll
    for (int col = 0; col < C; ++col) { dsum[col] = 0.0; cm[4 * col] = 0.0; cm[4 * col + 1] = 0.0; cm[4 * col + 2] = 0.0; cm[4 * col + 3] = 0.0; }
    for (int j = threadIdx.x; j < L.n; j += NT) {
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
    for (int i = threadIdx.x; i < L.m; i += NT) {
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
    if constexpr (C == 1) block_reduce<4, 1>(cm, dsum, red);
    else { double none[1] = {0.0}; block_reduce<8, C>(cm, dsum, red); block_reduce<4 * C - 8, 1>(cm + 8, none, red); }
    // refine_iter sweeps at least; then on while the correction is neither negligible (1e-12 of the solution, 1e-10 of r_y) nor stalled --
    // nearly dependent active rows contract r_y by only 1e-2 .. 1e-1 a sweep, rows held by a slack variable (a violated soft state box:
    // eps_feas against delta) by about 0.5: "stalled" is a correction that no longer shrinks by a tenth, not one that fails to halve.
    // r_w's correction is measured against the whole solution (|r_w|, c |r_y|, both scaled): where the seed's input sits on a bound r_w is
    // zero but for rounding and its own relative change says nothing.  A column that is done keeps what it has.
#pragma unroll
    for (int col = 0; col < C; ++col) {
        if (!((live >> col) & 1u)) continue;
        if (dsum[col] != dsum[col]) bad = true;
        const double rel = fmax(cm[4 * col] / fmax(fmax(cm[4 * col + 1], cc * cm[4 * col + 3]), 1e-300), 1e-2 * cm[4 * col + 2] / fmax(cm[4 * col + 3], 1e-300));
        if (may_stop && (rel <= 1e-12 || rel > 0.9 * lastrel[col])) live &= ~(1u << col);
        lastrel[col] = rel;
    }
    return live;
}

// One instance's outputs (q, l, u null: not wanted; the chained four are written only where the handle builds its vectors itself)
struct AdjointOut { double *x0, *um1, *xref, *uref, *q, *l, *u; };

// (made where it is used, not at the top of the kernel: seven more pointers live across the solves cost k_adjoint<16> registers it does not have)
__device__ __forceinline__ AdjointOut adjoint_out(const Lay &L, const AdjointArgs &Q, int b) {
    const size_t ns = (size_t)Q.nseeds;
    return AdjointOut{Q.ox0 + b * ns * L.nx, Q.oum1 + b * ns * L.nu, Q.oxref + b * ns * L.xref_rows * L.nx, Q.ouref + b * ns * L.nu,
                      Q.oq ? Q.oq + (size_t)b * L.n : nullptr, Q.ol ? Q.ol + (size_t)b * L.m : nullptr, Q.ou ? Q.ou + (size_t)b * L.m : nullptr};
}

// Seed sd's r_w = x, r_y = y into the outputs: dL/dq, dL/dl, dL/du (seed 0 only) and, with `chain`, the chain rule into the controller's parameters
__device__ __forceinline__ void adjoint_outputs(const Ctx &c, const int *act, const double *x, const double *y, int sd, int chain, const AdjointOut &o) {
    const Lay &L = c.L;
    const int tid = threadIdx.x, xw = L.xref_rows * L.nx;
    if (sd == 0) {
        if (o.q) for (int j = tid; j < L.n; j += NT) o.q[j] = -x[j];
        if (o.l && o.u) for (int i = tid; i < L.m; i += NT) { const int a = act[i]; o.l[i] = a == 1 ? y[i] : 0.0; o.u[i] = a == 2 ? y[i] : 0.0; }
    }
    if (!chain) return;
    const double *Qu = c.Qu(), *QDu = c.QDu();
    for (int i = tid; i < L.nx; i += NT) o.x0[sd * L.nx + i] = -y[i];      // l[:nx] = u[:nx] = -x0
    for (int l = tid; l < L.nu; l += NT) {
        double a = y[L.rdu + l];                  // the first Delta-u rows' bounds are Dumin / Dumax + u_{-1} (0 where the row is inactive)
        for (int jj = 0; jj < L.nu; ++jj) a += QDu[jj * L.nu + l] * x[L.ou + jj];      // q_U[0:nu] += -QDu u_{-1}
        o.um1[sd * L.nu + l] = a;
        double ur = 0.0;                          // q_U[k] = -iU_k Qu uref
        for (int k = 0; k < L.Nc; ++k) {
            const double iu = (k == L.Nc - 1) ? (double)(L.Np - L.Nc + 1) : 1.0;
            double t = 0.0;
            for (int jj = 0; jj < L.nu; ++jj) t += Qu[jj * L.nu + l] * x[L.ou + k * L.nu + jj];
            ur += iu * t;
        }
        o.uref[sd * L.nu + l] = ur;
    }
    if (L.xref_rows == 1) {                       // q_X[k] = -Q_k xref
        for (int l = tid; l < L.nx; l += NT) {
            double a = 0.0;
            for (int k = 0; k < L.N; ++k) {
                const double *Qk = (k < L.Np) ? c.Qx() : c.QxN();
                for (int i = 0; i < L.nx; ++i) a += Qk[i * L.nx + l] * x[k * L.nx + i];
            }
            o.xref[sd * xw + l] = a;
        }
    } else {                                      // q_X[k] = -(xref_k' Q_k)'
        for (int idx = tid; idx < L.N * L.nx; idx += NT) {
            const int k = idiv(idx, L.rnx), l = idx - k * L.nx;
            const double *Qk = (k < L.Np) ? c.Qx() : c.QxN();
            double a = 0.0;
            for (int i = 0; i < L.nx; ++i) a += Qk[l * L.nx + i] * x[k * L.nx + i];
            o.xref[sd * xw + idx] = a;
        }
    }
}

// Not computed (not solved, or a broken factor): every output of the ns seeds is zero
__device__ __forceinline__ void adjoint_zero(const Lay &L, int ns, int chain, const AdjointOut &o) {
    const int tid = threadIdx.x;
    if (o.q) for (int j = tid; j < L.n; j += NT) o.q[j] = 0.0;
    if (o.l && o.u) for (int i = tid; i < L.m; i += NT) { o.l[i] = 0.0; o.u[i] = 0.0; }
    if (!chain) return;
    for (int i = tid; i < ns * L.nx; i += NT) o.x0[i] = 0.0;
    for (int i = tid; i < ns * L.nu; i += NT) { o.um1[i] = 0.0; o.uref[i] = 0.0; }
    for (int i = tid; i < ns * L.xref_rows * L.nx; i += NT) o.xref[i] = 0.0;
}

template <int NB>
__global__ __launch_bounds__(NT) void k_adjoint(Lay L, Ptrs P, AdjointArgs Q) {
    extern __shared__ __attribute__((aligned(16))) double sh[];
    double *p = sh; Smem S; smem_common(L, P, p, S);       // (P.perm is null: workgroup b works on instance b)
    const int b = blockIdx.x, tid = threadIdx.x, ns = Q.nseeds;
    const mpcqp_info inf = P.info[b];
    int st = 0, nact = 0, nweak = 0;
    if (inf.status == MPCQP_SOLVED) {
        const double *model = P.model + (size_t)b * L.model_sz, *step = P.step + (size_t)b * L.step_sz;
        load_common(L, model, step, S);
        Ctx c{L, S.hot, model + L.hot_sz};
        const double *D = P.D + (size_t)b * L.n, *E = P.E + (size_t)b * L.m;
        const double cc = P.c[b], delta = Q.delta;
        const double *za = P.z + (size_t)b * L.m, *ya = P.y + (size_t)b * L.m;      // the ADMM iterate (unscaled)
        double *om = Q.K.om + (size_t)b * L.m, *sv = Q.K.s + (size_t)b * L.n;
        int *act = Q.K.act + (size_t)b * L.m;
        const size_t vn = (size_t)b * ADJOINT_COLS * L.n, vm = (size_t)b * ADJOINT_COLS * L.m;      // (column col of a vector: + col n, + col m)
        double *xs = Q.x + vn, *ys = Q.y + vm, *gs = Q.g + vn, *gts = Q.gt + vm;
        double *rs = Q.r + vn, *ds = Q.d + vn, *es = Q.e + vn, *dds = Q.dd + vn;
        // 1. active set (polishing's rule in the scaled space; equality rows always), weak rows, the metric of K_pol
        double ymx[1] = {0.0}, cnt[2] = {0.0, 0.0};
        for (int i = tid; i < L.m; i += NT) ymx[0] = fmax(ymx[0], fabs(ya[i]));
        block_reduce<1, 2>(ymx, cnt, S.red);
        const double ytol = Q.weak_tol * fmax(1.0, ymx[0]);
        for (int i = tid; i < L.m; i += NT) {
            double lo, hi; row_bounds(c, S.x0s, S.du0, affine_ptr(L, P, b), i, lo, hi);
            const double zv = za[i], yv = ya[i];
            const int a = kpol_row(E[i], zv, yv, lo, hi, cc, delta, true, om[i]);
            act[i] = a;
            if (a) cnt[0] += 1.0;
            if (lo != hi && fmin(zv - lo, hi - zv) <= Q.weak_tol * fmax(1.0, fabs(zv)) && fabs(yv) <= ytol) cnt[1] += 1.0;
        }
        for (int j = tid; j < L.n; j += NT) sv[j] = delta / (D[j] * D[j]);
        block_reduce<1, 2>(ymx, cnt, S.red);             // (ends with a barrier: act, om, sv are visible)
        nact = (int)cnt[0]; nweak = (int)cnt[1];
        // 2. factor K_pol once (generic block format, own buffers)
        Kpol kp;
        bool bad = !kpol_factor<NB>(c, Q.K, b, om, sv, cc, S, kp);
        // 3. the seeds, C to a solve: one solve from zero, then the refinement sweeps against the unregularized system
        auto seeds = [&](auto ctag) {
            constexpr int C = decltype(ctag)::value;
            for (int s0 = 0; s0 < ns && !bad; s0 += C) {
                const int nc = min(C, ns - s0);
                adjoint_seeds<C>(L, Q.gw ? Q.gw + (size_t)b * L.n : nullptr, Q.gu0 ? Q.gu0 + (size_t)b * L.nu : nullptr, s0, gs, xs, ys);
                double lastrel[C];
#pragma unroll
                for (int col = 0; col < C; ++col) lastrel[col] = 0.0;
                unsigned live = (1u << nc) - 1u;                 // the columns still sweeping
                for (int sw = 0; sw <= Q.refine + Q.extra && live && !bad; ++sw) {
                    adjoint_residual<C>(c, act, om, cc, live, xs, ys, gs, S.T, gts, rs);
                    kpol_solve<NB, C>(c, kp, cc, live, rs, ds, es, dds, S, Q.cs);
                    live = adjoint_update<C>(c, act, om, cc, live, sw >= Q.refine, xs, ys, ds, gts, S.red, lastrel, bad);
                }
                if (bad) break;
                // 4. dL/dq, dL/dl, dL/du and the chain rule into the controller's parameters
                const AdjointOut out = adjoint_out(L, Q, b);
                for (int col = 0; col < nc; ++col) adjoint_outputs(c, act, xs + (size_t)col * L.n, ys + (size_t)col * L.m, s0 + col, Q.chain, out);
                if (Q.od) for (int col = 0; col < nc; ++col) adjoint_affine_out(L, ys + (size_t)col * L.m, Q.od + ((size_t)b * ns + s0 + col) * L.d_rows * L.nx);
                __syncthreads();
            }
        };
        if (!bad) {
            if constexpr (NB <= 32) { if (Q.ncol > 1) seeds(std::integral_constant<int, ADJOINT_COLS>{}); else seeds(std::integral_constant<int, 1>{}); }
            else seeds(std::integral_constant<int, 1>{});
        }
        st = bad ? -1 : 1;
    }
    // 5. not computed: every output is zero
    if (st != 1) adjoint_zero(L, ns, Q.chain, adjoint_out(L, Q, b));
    if (st != 1 && Q.od) for (int e = tid; e < ns * L.d_rows * L.nx; e += NT) Q.od[(size_t)b * ns * L.d_rows * L.nx + e] = 0.0;
    if (tid == 0) { Q.status[b] = st; Q.nact[b] = nact; Q.nweak[b] = nweak; }
}
