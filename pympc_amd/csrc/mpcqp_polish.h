// mpcqp_polish.h -- part of libmpcqp_hip (included by mpcqp.hip, one translation unit; C ABI in include/mpcqp_polish.h).
// OSQP's solution polishing (OSQP 0.6 polish.c) after a solve: guess the active constraints from the iterate, solve the equality-constrained
// QP on them, keep the result if its residuals are better.  One 256-thread workgroup per instance, FP64, in the handle's SCALED space:
//   active set   (x~, z~, y~) = (x / D, E z, c y / E), (l~, u~) = (E l, E u):  lower-active if z~ - l~ < -y~, else upper-active if u~ - z~ < y~;
//   regularized  K_pol = [P~ + delta I, A~r'; A~r, -delta I] with the constraint block eliminated and written in unscaled variables, exactly
//                the matrix the ADMM factor has (K = c P + diag(s) + A' diag(omega) A, mpcqp.hip) with  s = delta / D^2  (scaled: delta I)
//                and  omega = E^2 / delta  on the active rows, 0 elsewhere (scaled: 1 / delta) -- factored by factor_all in the generic
//                block format into the polish's own buffers, whatever backend the handle runs;
//   refinement   one solve from zero, then polish_refine_iter sweeps in residual form against the UNREGULARIZED system (k_eq_solve's
//                multiplier sweep, mm_* in mpcqp_kernels.h: with omega / c = E^2 / (c delta) it is OSQP's iterative refinement step
//                  [x~; y~r] += K_pol^-1 ([-q~; b~r] - [P~, A~r'; A~r, 0] [x~; y~r])  in unscaled variables);
//   result       y = the multipliers of the active rows, 0 elsewhere; z = clip(A x, l, u); unscaled residuals and objective by the
//                termination test's own pass (check_norms_gown), accepted by OSQP 0.6's rule.
// The KKT solve of a sweep is refined against K_pol itself (applied matrix-free) until its correction stalls: the stored factor keeps explicit
// inverses of the stage Schur complements, accurate to about eps * cond, and the 1/delta rows make K_pol far worse conditioned than the ADMM
// matrix (cond 1e9 .. 1e12 on the golden fixtures) -- without it the sweeps contract too slowly to give OSQP's answer in polish_refine_iter steps.
// Accepted: the polished point replaces the solution, info's obj_val / pri_res / dua_res AND the ADMM iterate the next solve warm-starts
// from (polish.c copies pol->x, z, y into work->x, z, y).  Rejected: nothing changes.  status_polish: 1 / -1 / 0 (not solved: not tried).
// info.status, iter, rho_updates, rho, reserved, the stats counters, the handle's factor, rho and share map are never written.
#pragma once

struct PolishArgs {
    double *F;                    // [batch][fsz] the polish factor (generic block format)
    long long fsz;
    double *om, *s;               // [batch][m], [batch][n] the metric of K_pol
    double *x, *z, *y;            // [batch][n], [batch][m] x2 the polished point
    double *r, *d, *e, *dd;       // [batch][n] x4 residual / correction of a sweep, and of the inner refinement of its KKT solve
    double *bt; int *act;         // [batch][m] target of a row (l or u) and its state (0 inactive, 1 lower, 2 upper)
    double *Bb, *Zb, *Sig, *gws;  // the held input's border (Nc < Np) and the 128-wide factorization's workspace, of K_pol
    int *status;                  // [batch] status_polish
    double delta; int refine;
    double *pub; unsigned *done; unsigned long long seq;      // mpcqp_step_host: results to mapped host memory, as k_mpc_run does (pub null: off)
    int batch;
};

// Host side: the layout the polish runs in -- the handle's, with the register-resident and grouped formats off (they have no generic
// kkt_solve path) and a work area that holds the generic factorization's workspace and the solve's stage vectors.
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

constexpr int POLISH_INNER = 8;      // inner refinement steps of one KKT solve, at most

// out = K_pol v = c P v + s . v + A' (omega . (A v)), matrix-free; av: LDS scratch of m doubles
__device__ __forceinline__ void polish_kmul(const Ctx &c, const double *om, const double *sv, double cc, const double *v, double *av, double *out) {
    const Lay &L = c.L;
    for (int i = threadIdx.x; i < L.m; i += NT) {
        double a = 0.0;
        if (om[i] != 0.0) A_row(c, i, [&](double co, int idx) { a += co * v[idx]; });
        av[i] = om[i] * a;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < L.n; j += NT) {
        double pv = 0.0, at = 0.0;
        P_row(c, j, [&](double co, int idx) { pv += co * v[idx]; });
        AT_row(c, j, [&](double co, int row) { at += co * av[row]; });
        out[j] = cc * pv + sv[j] * v[j] + at;
    }
    __syncthreads();
}

template <int NB>
__global__ __launch_bounds__(NT) void k_polish(Lay L, Ptrs P, PolishArgs Q) {
    extern __shared__ __attribute__((aligned(16))) double sh[];
    double *p = sh; Smem S; smem_common(L, P, p, S);       // (P.perm is null: workgroup b polishes instance b)
    const int b = blockIdx.x, tid = threadIdx.x;
    const mpcqp_info inf = P.info[b];
    int st = 0;
    if (inf.status == MPCQP_SOLVED) {
        const double *model = P.model + (size_t)b * L.model_sz, *step = P.step + (size_t)b * L.step_sz;
        load_common(L, model, step, S);
        Ctx c{L, S.hot, model + L.hot_sz};
        if (!L.raw) build_q(c, step, S.Qv);
        const double *D = P.D + (size_t)b * L.n, *E = P.E + (size_t)b * L.m;
        const double cc = P.c[b], delta = Q.delta;
        const double *xa = P.x + (size_t)b * L.n, *za = P.z + (size_t)b * L.m, *ya = P.y + (size_t)b * L.m;      // the ADMM iterate (unscaled)
        double *om = Q.om + (size_t)b * L.m, *sv = Q.s + (size_t)b * L.n, *bt = Q.bt + (size_t)b * L.m;
        int *act = Q.act + (size_t)b * L.m;
        double *x = Q.x + (size_t)b * L.n, *z = Q.z + (size_t)b * L.m, *y = Q.y + (size_t)b * L.m;
        double *r = Q.r + (size_t)b * L.n, *d = Q.d + (size_t)b * L.n, *e = Q.e + (size_t)b * L.n, *dd = Q.dd + (size_t)b * L.n;
        // 1. active set (OSQP's rule in the scaled space) and the metric of K_pol
        for (int i = tid; i < L.m; i += NT) {
            double lo, hi; row_bounds(c, S.x0s, S.du0, i, lo, hi);
            const double e = E[i], zs = e * za[i], ys = cc * ya[i] / e;
            const bool low = zs - e * lo < -ys, upp = !low && (e * hi - zs < ys);
            act[i] = low ? 1 : upp ? 2 : 0;
            bt[i] = low ? lo : hi;
            om[i] = (low || upp) ? e * e / delta : 0.0;
            y[i] = 0.0;
        }
        for (int j = tid; j < L.n; j += NT) { sv[j] = delta / (D[j] * D[j]); x[j] = 0.0; }
        __syncthreads();
        // 2. factor K_pol (generic block format, own buffers)
        BorderPtrs bp; bp.red = S.red;
        const size_t npb = (size_t)L.nu * L.N * L.NB;
        bp.Bb = L.border ? Q.Bb + b * npb : nullptr; bp.Zb = L.border ? Q.Zb + b * npb : nullptr;
        bp.Sig = L.border ? Q.Sig + (size_t)b * L.nu * L.nu : nullptr;
        bp.gws = NB == 128 ? Q.gws + (size_t)b * HugeFmt::GWS : nullptr;
        double *F = Q.F + (size_t)b * Q.fsz;
        bool bad = factor_all<NB>(c, om, sv, cc, F, S.T, S.iflag, bp) != 0;
        // 3. one solve from zero, then the refinement sweeps against the unregularized system
        auto sel = [&](int i, double &t) { if (!act[i]) return false; t = bt[i]; return true; };
        double nrm[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int sw = 0; sw <= Q.refine && !bad; ++sw) {
            mm_row_residual(c, L.m, sel, x, y, om, cc, S.T, nrm);
            mm_var_residual(c, L.m, x, y, S.T, S.Qv, cc, r, nrm);
            kkt_solve<NB>(c, om, sv, cc, F, r, S.T + L.m, d, bp, S.tv);
            double last = 0.0;
            for (int it = 0; it < POLISH_INNER; ++it) {     // d += K~^-1 (r - K_pol d) until the correction is negligible or stops shrinking
                polish_kmul(c, om, sv, cc, d, S.T, e);
                for (int j = tid; j < L.n; j += NT) e[j] = r[j] - e[j];
                __syncthreads();
                kkt_solve<NB>(c, om, sv, cc, F, e, S.T + L.m, dd, bp, S.tv);
                double mx[2] = {0.0, 0.0}, ds[1] = {0.0};
                for (int j = tid; j < L.n; j += NT) { const double v = d[j] + dd[j]; d[j] = v; mx[0] = fmax(mx[0], fabs(dd[j])); mx[1] = fmax(mx[1], fabs(v)); ds[0] += dd[j]; }
                block_reduce<2, 1>(mx, ds, S.red);
                if (ds[0] != ds[0] || mx[0] <= 1e-13 * mx[1] || (it > 0 && mx[0] > 0.5 * last)) break;
                last = mx[0];
            }
            double dsum[1] = {0.0}, dmax[1] = {0.0};
            for (int j = tid; j < L.n; j += NT) { x[j] += d[j]; dsum[0] += d[j]; }
            block_reduce<1, 1>(dmax, dsum, S.red);
            if (dsum[0] != dsum[0]) bad = true;            // (a NaN correction: a broken factor)
            mm_dual_update(c, L.m, sel, x, om, cc, y);
        }
        // z = clip(A x, l, u); residuals and objective as the termination test evaluates them
        double pri = 0.0, dua = 0.0, obj = 0.0;
        if (!bad) {
            for (int i = tid; i < L.m; i += NT) {
                double lo, hi; row_bounds(c, S.x0s, S.du0, i, lo, hi);
                double ax = 0.0; A_row(c, i, [&](double co, int idx) { ax += co * x[idx]; });
                z[i] = fmin(fmax(ax, lo), hi);
            }
            __syncthreads();
            double vsum[1] = {0.0};
            for (int k = 0; k < 7; ++k) nrm[k] = 0.0;
            check_norms_gown(c, x, z, y, D, E, S.Qv, cc, S.T, S.tv, nrm, vsum, false);
            block_reduce<7, 1>(nrm, vsum, S.red);
            pri = nrm[0]; dua = nrm[3]; obj = vsum[0];
            if (obj != obj || pri > QP_INFTY || dua > QP_INFTY) bad = true;
        }
        // 4. accept (OSQP 0.6's rule) or reject
        const bool ok = !bad && ((pri < inf.pri_res && dua < inf.dua_res) || (pri < inf.pri_res && inf.dua_res < 1e-10) ||
                                 (dua < inf.dua_res && inf.pri_res < 1e-10));
        st = ok ? 1 : -1;
        if (ok) {
            double *xo = P.xo + (size_t)b * L.n, *yo = P.yo + (size_t)b * L.m;
            double *xg = P.x + (size_t)b * L.n, *zg = P.z + (size_t)b * L.m, *yg = P.y + (size_t)b * L.m;
            for (int j = tid; j < L.n; j += NT) { xo[j] = x[j]; xg[j] = x[j]; }
            for (int i = tid; i < L.m; i += NT) { yo[i] = y[i]; yg[i] = y[i]; zg[i] = z[i]; }
            if (tid == 0) { P.info[b].obj_val = obj; P.info[b].pri_res = pri; P.info[b].dua_res = dua; }
        }
        __syncthreads();
    }
    if (tid == 0) Q.status[b] = st;
    if (Q.pub) {                                 // mpcqp_step_host: the results to the caller's mapped memory; the last workgroup raises the flag
        double *px = Q.pub + (size_t)b * L.n, *py = Q.pub + (size_t)Q.batch * L.n + (size_t)b * L.m;
        for (int j = tid; j < L.n; j += NT) px[j] = P.xo[(size_t)b * L.n + j];
        for (int i = tid; i < L.m; i += NT) py[i] = P.yo[(size_t)b * L.m + i];
        mpcqp_info *pi = (mpcqp_info *)(Q.pub + (size_t)Q.batch * (L.n + L.m));
        __syncthreads();
        if (tid == 0) pi[b] = P.info[b];
        __threadfence_system();
        __syncthreads();
        if (tid == 0) {
            if (atomicAdd(Q.done, 1u) == (unsigned)Q.batch - 1u) {
                *Q.done = 0;
                __threadfence_system();
                *(volatile unsigned long long *)(pi + Q.batch) = Q.seq;
            }
        }
    }
}
