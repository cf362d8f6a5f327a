// mpcqp_polish.h -- part of libmpcqp_hip (included by mpcqp.hip, one translation unit; C ABI in include/mpcqp_polish.h).
// OSQP's solution polishing (OSQP 0.6 polish.c) after a solve: guess the active constraints from the iterate, solve the equality-constrained
// QP on them, keep the result if its residuals are better.  One 256-thread workgroup per instance, FP64, in the handle's SCALED space:
//   active set   (x~, z~, y~) = (x / D, E z, c y / E), (l~, u~) = (E l, E u):  lower-active if z~ - l~ < -y~, else upper-active if u~ - z~ < y~;
//   regularized  K_pol (mpcqp_kpol.h: the rule above is kpol_row) with  s = delta / D^2,  omega = E^2 / delta  on the active rows -- factored
//                in the generic block format into the polish's own buffers (kpol_factor), whatever backend the handle runs;
//   refinement   one solve from zero, then polish_refine_iter sweeps in residual form against the UNREGULARIZED system (k_eq_solve's
//                multiplier sweep, mm_* in mpcqp_kernels.h: with omega / c = E^2 / (c delta) it is OSQP's iterative refinement step
//                  [x~; y~r] += K_pol^-1 ([-q~; b~r] - [P~, A~r'; A~r, 0] [x~; y~r])  in unscaled variables);
//   result       y = the multipliers of the active rows, 0 elsewhere; z = clip(A x, l, u); unscaled residuals and objective by the
//                termination test's own pass (check_norms_gown), accepted by OSQP 0.6's rule.
// The KKT solve of a sweep is refined against K_pol itself until its correction stalls (kpol_solve, mpcqp_kpol.h, shared with k_adjoint) --
// without it the sweeps contract too slowly to give OSQP's answer in polish_refine_iter steps.
// Accepted: the polished point replaces the solution, info's obj_val / pri_res / dua_res AND the ADMM iterate the next solve warm-starts
// from (polish.c copies pol->x, z, y into work->x, z, y).  Rejected: nothing changes.  status_polish: 1 / -1 / 0 (not solved: not tried).
// info.status, iter, rho_updates, rho, reserved, the stats counters, the handle's factor, rho and share map are never written.
#pragma once

struct PolishArgs {
    KpolBufs K;                   // K_pol: factor, metric, active set
    double *x, *z, *y;            // [batch][n], [batch][m] x2 the polished point
    double *r, *d, *e, *dd;       // [batch][n] x4 residual / correction of a sweep, and of the inner refinement of its KKT solve
    double *bt;                   // [batch][m] target of an active row (l or u)
    int *status;                  // [batch] status_polish
    double delta; int refine;
    double *pub; unsigned *done; unsigned long long seq;      // mpcqp_step_host: results to mapped host memory, as k_mpc_run does (pub null: off)
    int batch;
};

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
        double *om = Q.K.om + (size_t)b * L.m, *sv = Q.K.s + (size_t)b * L.n, *bt = Q.bt + (size_t)b * L.m;
        int *act = Q.K.act + (size_t)b * L.m;
        double *x = Q.x + (size_t)b * L.n, *z = Q.z + (size_t)b * L.m, *y = Q.y + (size_t)b * L.m;
        double *r = Q.r + (size_t)b * L.n, *d = Q.d + (size_t)b * L.n, *e = Q.e + (size_t)b * L.n, *dd = Q.dd + (size_t)b * L.n;
        // 1. active set (OSQP's rule in the scaled space) and the metric of K_pol
        for (int i = tid; i < L.m; i += NT) {
            double lo, hi; row_bounds(c, S.x0s, S.du0, affine_ptr(L, P, b), i, lo, hi);
            const int a = kpol_row(E[i], za[i], ya[i], lo, hi, cc, delta, false, om[i]);
            act[i] = a;
            bt[i] = a == 1 ? lo : hi;
            y[i] = 0.0;
        }
        for (int j = tid; j < L.n; j += NT) { sv[j] = delta / (D[j] * D[j]); x[j] = 0.0; }
        __syncthreads();
        // 2. factor K_pol (generic block format, own buffers)
        Kpol kp;
        bool bad = !kpol_factor<NB>(c, Q.K, b, om, sv, cc, S, kp);
        // 3. one solve from zero, then the refinement sweeps against the unregularized system
        auto sel = [&](int i, double &t) { if (!act[i]) return false; t = bt[i]; return true; };
        double nrm[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int sw = 0; sw <= Q.refine && !bad; ++sw) {
            mm_row_residual(c, L.m, sel, x, y, om, cc, S.T, nrm);
            mm_var_residual(c, L.m, x, y, S.T, S.Qv, cc, r, nrm);
            kpol_solve<NB, 1>(c, kp, cc, 1u, r, d, e, dd, S, 0);
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
                double lo, hi; row_bounds(c, S.x0s, S.du0, affine_ptr(L, P, b), i, lo, hi);
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
