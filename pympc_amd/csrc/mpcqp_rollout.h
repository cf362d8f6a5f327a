// mpcqp_rollout.h -- part of libmpcqp_hip (included by mpcqp.hip, one translation unit; C ABI in include/mpcqp_rollout.h).
// A closed-loop rollout with a tape, and its derivative in one reverse sweep.
//   forward   mpcqp_rollout runs the device loop one step per launch and puts k_rollout_tape in front of each: a grid-stride copy of what
//             the handle holds at that moment -- the ADMM iterate, the step data (entry 0: with the u_{-1} its solve was made with, where
//             mpcqp_mpc_step has already stored the next), the status, and the input output() is about to apply -- into tape entry k.
//   reverse   k_rollout_adjoint<NB>: ONE launch, one 256-thread workgroup per instance walking its tape from entry K-1 down to 0.  Per entry it
//             is k_adjoint (mpcqp_adjoint.h) with the pointers aimed at the tape -- kpol_row, kpol_factor, one seed through adjoint_residual /
//             kpol_solve / adjoint_update, adjoint_outputs -- followed by the sums of adjoint_model_entry (mpcqp_adjoint_model.h), with the
//             recursion of include/mpcqp_rollout.h around it.  lam, mu and g are carried in LDS behind the common block, or in a few doubles
//             of global memory where that block already fills the workgroup's LDS.  The model gradients accumulate in the per-instance
//             buffer k_adjoint_model writes (field-major: k_adjoint_model_sum adds it over the batch), the plant gradients in one of the tape's,
//             the bound gradients (ROLLOUT_WANT_BOUNDS: adjoint_bounds_entry, mpcqp_adjoint_bounds.h) behind the model's in the same buffer,
//             which is where k_adjoint_bounds writes too.
//   reuse     the metric of K_pol is s = delta / D^2 (fixed) and omega = E^2 / delta on the active rows: it follows from the active set alone.
//             The rows whose state differs from the one in place are counted while the set is written; where there is none and a factor
//             is in place, kpol_factor is skipped.  The factorization is deterministic: the same bits either way.
//   schedule  TV = true (k_rollout_adjoint_tv<NB>, include_ext/mpcqp_rollout_tv.h): the loop ran under a model schedule and the tape holds every model
//             it was made under, with its scaling, as slots (RolloutSlots).  Entry k then reads model, D, E, c of slot sigma(k) = 0 for k = 0,
//             1 + (k - 1) / hold beyond; on a change of slot the fixed half of the metric is formed again and the factor in place is dropped.
//             Without a plant of its own the step reads Ad, Bd of the slot in force, 1 + k / hold, from global memory (S.hot holds the solve's
//             slot, another one at a boundary step).  The Ad, Bd gradients land in the slot's buffer, the plant's in the schedule entry's.
//             TV = false compiles to the code without any of it.
//   estimator EST = true (k_rollout_adjoint_est<NB>, include/mpcqp_rollout_est.h): the loop ran output feedback, the entry's x0 is the estimate
//             xh_k and the tape holds the plant state x_k, the measurement y_k, C and L beside it.  The step prologue then carries eta
//             (the gradient at xh) beside lam and forms s = Ad' eta, t = L' s, r = G_y + t in three more barrier-separated phases; the
//             step's d_x0 lands on eta instead of lam.  EST = false compiles to the code without any of it.
//   both      EST and TV (k_rollout_adjoint_tv_est<NB>, include_ext2/mpcqp_rollout_tv_est.h): the output-feedback loop ran under a schedule of
//             models and, where given, of observer gains.  The estimator stepped under the slot in force, pi(k) = 1 + k / hold, so its phases
//             read Ad, Bd of that slot's blob from global memory (S.hot holds the solve's slot sigma(k), another one at every boundary step)
//             and the gain of entry k / hold (RolloutGains); d_Ae, d_Be, d_L are re-aimed per entry as the plant's d_Ap, d_Bp are.
//   affine    a RUNTIME path of the state-feedback sweeps, no instantiation of its own (mpcqp_rollout_adjoint_affine, include_ext5/mpcqp_rollout_affine.h): the loop
//             ran with an affine term in the prediction model.  Every entry reads its bounds under the term in its own step data (step + Lay::od; the
//             sweep's Lay carries the tape's d_rows), and under ROLLOUT_WANT_AFFINE -r_y of the dynamics row blocks 1 .. Np is added onto the slot
//             tau(k) the entry was solved under.  A tape without a term has d_rows = 0 and the flag clear: it executes none of it.
// Every sum over the steps is formed by the thread that owns the entry, in the order K-1 .. 0: no atomics, the same bits every time.
#pragma once

struct RolloutTape {
    double *x, *z, *y;            // [K][batch][n], [K][batch][m] x2 the iterate of entry k (unscaled)
    double *step;                 // [K][batch][step_sz] the step data its solve was made with
    double *u;                    // [K][batch][nu] the input applied at step k
    int *status;                  // [K][batch] mpcqp_info.status of entry k
    double *Ap, *Bp;              // [batch][nx nx], [batch][nx nu] the plant, or null (the controller's Ad, Bd)
    // the sweep's staging: seeds in, results out
    double *gx, *gu;              // [K+1][batch][nx], [K][batch][nu]
    double *lam;                  // [K+1][batch][nx]
    double *dxref;                // [K][batch][xref_rows nx]
    double *dum1, *duref;         // [batch][nu] x2
    double *dAp, *dBp;            // [batch][nx nx], [batch][nx nu]
    double *carry;                // [batch][rollout_carry_doubles] lam, mu, g where LDS has no room for them
    int *nact, *nweak, *st;       // [K][batch]
    int *nfactor;                 // [batch]
    int nsteps, batch;
    // output feedback (mpcqp_rollout_est; ny = 0 and null otherwise)
    int ny;
    double *xp, *ym;              // [K+1][batch][nx] the plant states, [K][batch][ny] the measurements
    double *C, *Lg;               // [batch][ny nx], [batch][nx ny]
    double *xt;                   // [batch][nx] x_true during the forward loop
    double *gxh, *gy;             // [K+1][batch][nx], [K][batch][ny] seeds
    double *eta, *dv;             // [K+1][batch][nx], [K][batch][ny]
    double *dC, *dL, *dAe, *dBe;  // [batch][ny nx], [batch][nx ny], [batch][nx nx], [batch][nx nu]
};
struct RolloutSweep {
    double *mout;                 // the model gradients, field f of instance b: mout + batch off[f] + b (off[f + 1] - off[f])  (AdjointModelArgs::out)
    int off[ADJM_FIELDS + 1];
    int no_reuse, carry_lds;
    int want_model;               // bit 0: the model gradients; bit 1 (ROLLOUT_WANT_BOUNDS): the bound gradients too, field-major (AdjointBoundsArgs::out,
                                  // mpcqp_adjoint_bounds.h) behind the model's: mout + batch off[ADJM_FIELDS].  (A flag bit and a fixed place, not two more
                                  // kernel arguments: the sweep has no scalar register to spare, and one that is not asked for bounds must cost what it did.)
};
constexpr int ROLLOUT_WANT_MODEL = 1, ROLLOUT_WANT_BOUNDS = 2;
// bit 2 (ROLLOUT_WANT_AFFINE, mpcqp_rollout_adjoint_affine, include_ext5/mpcqp_rollout_affine.h): the tape is one of mpcqp_rollout_affine and the gradient of
// its terms is wanted, per slot.  The same economy: a flag bit and a fixed place -- the tape's affine area, which tape_carve puts right behind the
// block of T.nact: 256 bytes of header (int hold; 0: one constant term, every entry under slot 0), then d_d_slots [nslots][batch][d_rows nx].  The
// term an entry was solved with needs neither: it is in the entry's own step data, read where Lay::d_rows > 0 (the sweep's Lay has the tape's).
constexpr int ROLLOUT_WANT_AFFINE = 4;
constexpr size_t ROLLOUT_AFFINE_HEADER = 256;
// The affine area as the host sees it (tape_carve; not a kernel argument).  dval: the terms themselves, for mpcqp_rollout_affine_get_slot.
struct RolloutAffine {
    int *header;                          // hold (0: one constant term)
    double *dgrad, *dval;                 // [nslots][batch][rows nx] x2
    int nslots, rows, hold;
};
__host__ __device__ inline size_t rollout_info_bytes(size_t K, size_t B) { return ((3 * K * B + B) * sizeof(int) + 255) & ~size_t(255); }
// tau(k): the term slot tape entry k was solved under; the slots a tape of K steps has (the ONE statement of both: kernel and host)
__host__ __device__ inline int rollout_affine_tau(int k, int hold) { return (k == 0 || hold == 0) ? 0 : 1 + (k - 1) / hold; }
__host__ __device__ inline int rollout_affine_nslots(int K, int hold) { return hold == 0 ? 1 : 2 + (K - 1) / hold; }      // (slot 0 and ceil(K / hold) entries)
// The model slots of a scheduled tape (mpcqp_rollout_tv, include_ext/mpcqp_rollout_tv.h): slot 0 is the model the call began under, slot e + 1
// schedule entry e.  An argument of k_rollout_adjoint_tv alone: the other two sweeps neither take nor read it.
struct RolloutSlots {
    const double *model, *D, *E, *c;      // [nslots][batch][model_sz], [..][n], [..][m], [nslots][batch]: what the handle held under slot s
    double *dAd, *dBd;                    // [nslots][batch][nx nx], [..][nx nu] the solve path of the entries made under slot s
    double *dAp, *dBp;                    // [nslots - 1][batch][nx nx], [..][nx nu] the plant path of the steps schedule entry e was in force
    int hold, nslots;
};
// The observer gains of a scheduled output-feedback tape (mpcqp_rollout_tv_est, include_ext2/mpcqp_rollout_tv_est.h) and the estimator path's
// per-entry sums.  An argument of k_rollout_adjoint_tv_est alone: the other three sweeps neither take nor read it.
struct RolloutGains {
    const double *Lg;                     // [nslots - 1][batch][nx ny] the gain of schedule entry e
    double *dAe, *dBe, *dL;               // [nslots - 1][batch][nx nx], [..][nx nu], [..][nx ny] the steps schedule entry e was in force
};

// lam | lam as the plant alone gives it | d_x0 of the step | g | mu | d_uref of the step | d_uref so far
// with an estimator (ny > 0), behind them: eta | eta before d_x0 | s | xhat[k|k] | t | r | innovation
__host__ __device__ inline int rollout_carry_doubles(const Lay &L, int ny = 0) { return 3 * L.nx + 4 * L.nu + (ny > 0 ? 4 * L.nx + 3 * ny : 0); }

// Workgroup b's row of slot 0 of the term's gradient in the tape's affine area (w = d_rows nx doubles; slot s lies s batch w further on), and the area's hold.
__device__ __forceinline__ double *rollout_affine_grad(const RolloutTape &T, int w, int &hold) {
    const char *area = (const char *)T.nact + rollout_info_bytes((size_t)T.nsteps, (size_t)T.batch);
    hold = *(const int *)area;
    return (double *)(area + ROLLOUT_AFFINE_HEADER) + (size_t)blockIdx.x * w;
}

// Entry k of the tape from what the handle holds now.  um1: the u_{-1} the current solve was made with where the step data no longer have it, else null.
__global__ __launch_bounds__(256) void k_rollout_tape(Lay L, Ptrs P, RolloutTape T, int k, const double *um1) {
    const size_t B = (size_t)T.batch, n = L.n, m = L.m, ss = L.step_sz, nu = L.nu;
    const size_t per = n + 2 * m + ss + nu + 1, total = B * per;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t b = idx / per, kb = (size_t)k * B + b;
        size_t i = idx - b * per;
        if (i < n) { T.x[kb * n + i] = P.x[b * n + i]; continue; }
        i -= n;
        if (i < m) { T.z[kb * m + i] = P.z[b * m + i]; continue; }
        i -= m;
        if (i < m) { T.y[kb * m + i] = P.y[b * m + i]; continue; }
        i -= m;
        if (i < ss) { T.step[kb * ss + i] = (um1 && i >= (size_t)L.nx && i < (size_t)(L.nx + L.nu)) ? um1[b * nu + (i - L.nx)] : P.step[b * ss + i]; continue; }
        i -= ss;
        const int status = P.info[b].status;
        if (i < nu) T.u[kb * nu + i] = status == MPCQP_SOLVED ? P.xo[b * n + L.ou + i] : P.model[b * L.model_sz + L.ouref + i];      // (output(), as k_mpc_run applies it)
        else T.status[kb] = status;
    }
}

// The sweep's body.  The estimator is a template parameter of this force-inlined function and not of the kernel: k_rollout_adjoint<NB> keeps the
// name and the one template argument it had (the build's resource remarks are read by that name, tests/test_rollout_resources.py), and is the
// EST = false instantiation; k_rollout_adjoint_est<NB> is the EST = true one.
template <int NB, bool EST, bool TV>
__device__ __forceinline__ void rollout_adjoint_body(const Lay &L, const Ptrs &P, const AdjointArgs &Q, const RolloutTape &T, const RolloutSweep &W, const RolloutSlots &V,
                                                     const RolloutGains &X) {
    extern __shared__ __attribute__((aligned(16))) double sh[];
    double *p = sh; Smem S; smem_common(L, P, p, S);       // (P.perm is null: workgroup b works on instance b)
    const int b = blockIdx.x, tid = threadIdx.x, B = T.batch, K = T.nsteps;
    const int nx = L.nx, nu = L.nu, xw = L.xref_rows * L.nx, EN = W.off[ADJM_FIELDS];
    const int ny = EST ? T.ny : 0;
    double *lam = W.carry_lds ? p : T.carry + (size_t)b * rollout_carry_doubles(L, ny);
    double *lamn = lam + nx, *dx0 = lamn + nx, *g = dx0 + nx, *mu = g + nu, *durk = mu + nu, *dur = durk + nu;
    double *eta = dur + nu, *etan = eta + nx, *sv_e = etan + nx, *xu = sv_e + nx, *tv = xu + nx, *rv = tv + ny, *inn = rv + ny;      // (EST only)
    const double *Cm = EST ? T.C + (size_t)b * ny * nx : nullptr, *Lg = EST && !TV ? T.Lg + (size_t)b * nx * ny : nullptr;
    double *dC = EST ? T.dC + (size_t)b * ny * nx : nullptr, *dL = EST && !TV ? T.dL + (size_t)b * nx * ny : nullptr;      // (EST and TV: Lg, dL, dAe, dBe are
    double *dAe = EST && !TV ? T.dAe + (size_t)b * nx * nx : nullptr, *dBe = EST && !TV ? T.dBe + (size_t)b * nx * nu : nullptr;      // aimed at the schedule entry in force inside the loop)
    const double *model = P.model + (size_t)b * L.model_sz;
    const double *D = P.D + (size_t)b * L.n, *E = P.E + (size_t)b * L.m;
    double cc = TV ? 0.0 : P.c[b];                        // (TV: all four are aimed at the entry's slot inside the loop)
    const double delta = Q.delta;
    int slot = -1;                                       // (TV) the slot model, D, E, cc, sv belong to
    double *om = Q.K.om + (size_t)b * L.m, *sv = Q.K.s + (size_t)b * L.n;
    int *act = Q.K.act + (size_t)b * L.m;
    const size_t vn = (size_t)b * ADJOINT_COLS * L.n, vm = (size_t)b * ADJOINT_COLS * L.m;      // (column 0 of the adjoint's work area)
    double *xs = Q.x + vn, *ys = Q.y + vm, *gs = Q.g + vn, *gts = Q.gt + vm;
    double *rs = Q.r + vn, *ds = Q.d + vn, *es = Q.e + vn, *dds = Q.dd + vn;
    double *dAp = T.dAp + (size_t)b * nx * nx, *dBp = T.dBp + (size_t)b * nx * nu;
    AdjointModelArgs M;                                  // (adjoint_model_entry reads the field offsets only)
#pragma unroll
    for (int f = 0; f <= ADJM_FIELDS; ++f) M.off[f] = W.off[f];
    auto mdst = [&](int e) -> double & {
        int f = 0;
        while (e >= W.off[f + 1]) ++f;
        if constexpr (TV) if (f < 2) return (f == 0 ? V.dAd : V.dBd)[((size_t)slot * B + b) * (W.off[f + 1] - W.off[f]) + (e - W.off[f])];      // (Ad, Bd: per slot)
        return W.mout[(size_t)B * W.off[f] + (size_t)b * (W.off[f + 1] - W.off[f]) + (e - W.off[f])];
    };
    // lam_K = G_x[K], mu = 0, every sum 0; the fixed half of K_pol's metric
    for (int i = tid; i < nx; i += NT) { const double v = T.gx[((size_t)K * B + b) * nx + i]; lam[i] = v; T.lam[((size_t)K * B + b) * nx + i] = v; }
    for (int j = tid; j < nu; j += NT) { mu[j] = 0.0; dur[j] = 0.0; }
    if constexpr (TV) {
        for (int s = 0; s < V.nslots; ++s) {
            for (int e = tid; e < nx * nx; e += NT) { V.dAd[((size_t)s * B + b) * nx * nx + e] = 0.0; if (s) V.dAp[((size_t)(s - 1) * B + b) * nx * nx + e] = 0.0; }
            for (int e = tid; e < nx * nu; e += NT) { V.dBd[((size_t)s * B + b) * nx * nu + e] = 0.0; if (s) V.dBp[((size_t)(s - 1) * B + b) * nx * nu + e] = 0.0; }
        }
    }
    for (int e = tid + (TV ? W.off[2] : 0); e < EN; e += NT) mdst(e) = 0.0;
    auto bdst = [&](int e) -> double & {                 // (called under ROLLOUT_WANT_BOUNDS only)
        const int f = e < 2 * nx ? e / nx : 2 + (e - 2 * nx) / nu, sz = f < 2 ? nx : nu, off = f < 2 ? f * nx : 2 * nx + (f - 2) * nu;
        return W.mout[(size_t)B * (EN + off) + (size_t)b * sz + (e - off)];
    };
    if (W.want_model & ROLLOUT_WANT_BOUNDS) for (int e = tid; e < adjoint_bounds_entries(L); e += NT) bdst(e) = 0.0;
    for (int e = tid; e < nx * nx; e += NT) dAp[e] = 0.0;
    for (int e = tid; e < nx * nu; e += NT) dBp[e] = 0.0;
    // the affine area, found behind the flag where it is used (rollout_affine_grad: ONE statement of the place; nothing of it is kept live across the entries, the
    // sweep has no register to spare) and never in the estimator's instantiations, which no affine tape reaches
    if constexpr (!EST) if (W.want_model & ROLLOUT_WANT_AFFINE) {
        int hold;
        const int w = L.d_rows * nx;                     // every slot of the term's gradient: a slot no entry was solved under stays zero
        double *add = rollout_affine_grad(T, w, hold);
        for (int s = 0; s < rollout_affine_nslots(K, hold); ++s) for (int e = tid; e < w; e += NT) add[(size_t)s * B * w + e] = 0.0;
    }
    if (EST) {                                           // eta_K = G_xh[K]
        for (int i = tid; i < nx; i += NT) { const double v = T.gxh[((size_t)K * B + b) * nx + i]; eta[i] = v; T.eta[((size_t)K * B + b) * nx + i] = v; }
        if constexpr (TV) {
            for (int s = 0; s + 1 < V.nslots; ++s) {
                const size_t sb = (size_t)s * B + b;
                for (int e = tid; e < nx * nx; e += NT) X.dAe[sb * nx * nx + e] = 0.0;
                for (int e = tid; e < nx * nu; e += NT) X.dBe[sb * nx * nu + e] = 0.0;
                for (int e = tid; e < nx * ny; e += NT) X.dL[sb * nx * ny + e] = 0.0;
            }
            for (int e = tid; e < nx * ny; e += NT) dC[e] = 0.0;
        } else {
            for (int e = tid; e < nx * nx; e += NT) dAe[e] = 0.0;
            for (int e = tid; e < nx * nu; e += NT) dBe[e] = 0.0;
            for (int e = tid; e < nx * ny; e += NT) { dC[e] = 0.0; dL[e] = 0.0; }
        }
    }
    if constexpr (!TV) for (int j = tid; j < L.n; j += NT) sv[j] = delta / (D[j] * D[j]);
    __syncthreads();
    Kpol kp = {};
    bool have = false;                                   // a factor of the active set in act[] is in place
    int nfac = 0;
    for (int k = K - 1; k >= 0; --k) {
        const size_t kb = (size_t)k * B + b;
        const double *step = T.step + kb * L.step_sz;
        if constexpr (TV) {                              // the slot this entry's solve was made under: its model, its scaling, its metric, and no factor of another's
            const int s = k == 0 ? 0 : 1 + (k - 1) / V.hold;
            if (s != slot) {
                const size_t sb = (size_t)s * B + b;
                slot = s;
                model = V.model + sb * L.model_sz; D = V.D + sb * L.n; E = V.E + sb * L.m; cc = V.c[sb];
                for (int j = tid; j < L.n; j += NT) sv[j] = delta / (D[j] * D[j]);
                have = false;
            }
        }
        load_common(L, model, step, S);                  // (x_k, u_{-1} and the first Delta-u bounds of this entry; ends with a barrier)
        {   // g = G_u[k] + Bp' lam_{k+1} + mu;  lam_k = G_x[k] + Ap' lam_{k+1} (+ d_x0 below);  d_Ap += lam_{k+1} x_k',  d_Bp += lam_{k+1} u_k'
            const double *inforce = TV ? V.model + ((size_t)(1 + k / V.hold) * B + b) * L.model_sz : S.hot;      // (TV: the plant follows the schedule entry in force)
            const double *Ap = T.Ap ? T.Ap + (size_t)b * nx * nx : inforce + L.oAd, *Bp = T.Bp ? T.Bp + (size_t)b * nx * nu : inforce + L.oBd;
            double *dApk = TV ? V.dAp + ((size_t)(k / V.hold) * B + b) * nx * nx : dAp, *dBpk = TV ? V.dBp + ((size_t)(k / V.hold) * B + b) * nx * nu : dBp;
            const double *uk = T.u + kb * nu;
            const double *xk = EST ? T.xp + kb * nx : S.x0s;      // (the plant state; with an estimator the entry's x0 is the estimate)
            const double *estm = TV ? inforce : S.hot;            // (EST: the model the estimator stepped under, the slot in force)
            if constexpr (EST && TV) {                            // the gain and the estimator path's sums of the schedule entry in force
                const size_t eb = (size_t)(k / V.hold) * B + b;
                Lg = X.Lg + eb * nx * ny; dL = X.dL + eb * nx * ny; dAe = X.dAe + eb * nx * nx; dBe = X.dBe + eb * nx * nu;
            }
            for (int j = tid; j < nu; j += NT) {
                double a = T.gu[kb * nu + j] + mu[j];
                for (int i = 0; i < nx; ++i) a += Bp[i * nu + j] * lam[i];
                if (EST) { const double *Bd = estm + L.oBd; for (int i = 0; i < nx; ++i) a += Bd[i * nu + j] * eta[i]; }
                g[j] = a;
            }
            for (int i = tid; i < nx; i += NT) {
                double a = T.gx[kb * nx + i];
                for (int r = 0; r < nx; ++r) a += Ap[r * nx + i] * lam[r];
                lamn[i] = a;
            }
            for (int e = tid; e < nx * nx; e += NT) { const int r = e / nx; dApk[e] += lam[r] * xk[e - r * nx]; }
            for (int e = tid; e < nx * nu; e += NT) { const int r = e / nu; dBpk[e] += lam[r] * uk[e - r * nu]; }
            if (EST) {
                // s = Ad' eta_{k+1};  d_Be += eta_{k+1} u_k'
                const double *Ad = estm + L.oAd, *yk = T.ym + kb * ny;
                for (int i = tid; i < nx; i += NT) {
                    double a = 0.0;
                    for (int r = 0; r < nx; ++r) a += Ad[r * nx + i] * eta[r];
                    sv_e[i] = a;
                }
                for (int e = tid; e < nx * nu; e += NT) { const int r = e / nu; dBe[e] += eta[r] * uk[e - r * nu]; }
                __syncthreads();
                // t = L' s;  r = G_y[k] + t = d_v[k];  the innovation y_k - C xh_k
                for (int j = tid; j < ny; j += NT) {
                    double a = 0.0, yh = 0.0;
                    for (int i = 0; i < nx; ++i) { a += Lg[i * ny + j] * sv_e[i]; yh += Cm[j * nx + i] * S.x0s[i]; }
                    const double rr = T.gy[kb * ny + j] + a;
                    tv[j] = a; rv[j] = rr; inn[j] = yk[j] - yh;
                    T.dv[kb * ny + j] = rr;
                }
                __syncthreads();
                // lam_k += C' r;  eta_k = G_xh[k] + s - C' t (+ d_x0 below);  xhat[k|k];  d_L += s inn',  d_C += r x_k' - t xh_k'
                for (int i = tid; i < nx; i += NT) {
                    double a = lamn[i], c = T.gxh[kb * nx + i] + sv_e[i], x = S.x0s[i];
                    for (int j = 0; j < ny; ++j) { a += Cm[j * nx + i] * rv[j]; c -= Cm[j * nx + i] * tv[j]; x += Lg[i * ny + j] * inn[j]; }
                    lamn[i] = a; etan[i] = c; xu[i] = x;
                }
                for (int e = tid; e < nx * ny; e += NT) {
                    const int i = e / ny, j = e / nx;              // dL is [nx][ny], dC is [ny][nx]
                    dL[e] += sv_e[i] * inn[e - i * ny];
                    dC[e] += rv[j] * xk[e - j * nx] - tv[j] * S.x0s[e - j * nx];
                }
                __syncthreads();
                // d_Ae += eta_{k+1} xhat[k|k]'
                for (int e = tid; e < nx * nx; e += NT) { const int r = e / nx; dAe[e] += eta[r] * xu[e - r * nx]; }
            }
        }
        __syncthreads();
        int st = 0, nact = 0, nweak = 0;
        if (T.status[kb] == MPCQP_SOLVED) {
            Ctx c{L, S.hot, model + L.hot_sz};
            const double *wa = T.x + kb * L.n, *za = T.z + kb * L.m, *ya = T.y + kb * L.m;
            // 1. the active set of this entry (k_adjoint's step 1), and how many rows differ from the set in place
            double ymx[1] = {0.0}, cnt[3] = {0.0, 0.0, 0.0};
            for (int i = tid; i < L.m; i += NT) ymx[0] = fmax(ymx[0], fabs(ya[i]));
            block_reduce<1, 3>(ymx, cnt, S.red);
            const double ytol = Q.weak_tol * fmax(1.0, ymx[0]);
            for (int i = tid; i < L.m; i += NT) {
                double lo, hi; row_bounds(c, S.x0s, S.du0, step + L.od, i, lo, hi);      // (the term this entry was solved with, where the tape has one: L.d_rows is the tape's)
                const double zv = za[i], yv = ya[i];
                const int a = kpol_row(E[i], zv, yv, lo, hi, cc, delta, true, om[i]);
                if (a != act[i]) cnt[2] += 1.0;
                act[i] = a;
                if (a) cnt[0] += 1.0;
                if (lo != hi && fmin(zv - lo, hi - zv) <= Q.weak_tol * fmax(1.0, fabs(zv)) && fabs(yv) <= ytol) cnt[1] += 1.0;
            }
            block_reduce<1, 3>(ymx, cnt, S.red);             // (ends with a barrier: act, om are visible)
            nact = (int)cnt[0]; nweak = (int)cnt[1];
            // 2. factor K_pol, unless the factor in place belongs to this very set
            bool bad = false;
            if (!have || cnt[2] != 0.0 || W.no_reuse) { bad = !kpol_factor<NB>(c, Q.K, b, om, sv, cc, S, kp); ++nfac; }
            // 3. the seed g on the u_0 block: one solve from zero, then the refinement sweeps against the unregularized system
            if (!bad) {
                adjoint_seeds<1>(L, nullptr, g, 0, gs, xs, ys);
                double lastrel[1] = {0.0};
                unsigned live = 1u;
                for (int sw = 0; sw <= Q.refine + Q.extra && live && !bad; ++sw) {
                    adjoint_residual<1>(c, act, om, cc, live, xs, ys, gs, S.T, gts, rs);
                    kpol_solve<NB, 1>(c, kp, cc, live, rs, ds, es, dds, S, 0);
                    live = adjoint_update<1>(c, act, om, cc, live, sw >= Q.refine, xs, ys, ds, gts, S.red, lastrel, bad);
                }
            }
            have = !bad;
            if (!bad) {
                // 4. the chain rule into x_k, u_{-1}, xref, uref; 5. the model gradients of this entry onto the sums
                const AdjointOut o{dx0, mu, T.dxref + kb * xw, durk, nullptr, nullptr, nullptr};
                adjoint_outputs(c, act, xs, ys, 0, 1, o);
                if (W.want_model & ROLLOUT_WANT_MODEL) for (int e = tid; e < EN; e += NT) mdst(e) += adjoint_model_entry(L, M, wa, xs, ya, ys, model, step, e, 0, 1);
                if (W.want_model & ROLLOUT_WANT_BOUNDS)      // (dL/db = r_y of this entry onto the bounds; a sweep that is not asked runs none of it)
                    for (int e = tid; e < adjoint_bounds_entries(L); e += NT) bdst(e) += adjoint_bounds_entry(L, act, ys, e);
                if constexpr (!EST) if (W.want_model & ROLLOUT_WANT_AFFINE) {      // (k_affine_grad's rule, mpcqp_affine.h, onto the slot this entry was solved under; the thread that zeroed the element)
                    int hold;
                    const int w = L.d_rows * nx;
                    double *dd = rollout_affine_grad(T, w, hold);
                    dd += (size_t)rollout_affine_tau(k, hold) * B * w;
                    const double *ry = ys + nx;              // (row block 1 onwards)
                    for (int e = tid; e < w; e += NT) {
                        double acc = 0.0;
                        if (L.d_rows > 1) acc = -ry[e];
                        else for (int j = 0; j < L.Np; ++j) acc -= ry[j * nx + e];
                        dd[e] += acc;
                    }
                }
                __syncthreads();
                if (EST) for (int i = tid; i < nx; i += NT) { lam[i] = lamn[i]; eta[i] = etan[i] + dx0[i]; }
                else for (int i = tid; i < nx; i += NT) lam[i] = lamn[i] + dx0[i];
                for (int j = tid; j < nu; j += NT) dur[j] += durk[j];
            }
            st = bad ? -1 : 1;
        }
        if (st != 1) {                                   // u_failure = uref was applied (not solved), or nothing can be said (a broken factor)
            for (int i = tid; i < nx; i += NT) { lam[i] = lamn[i]; if (EST) eta[i] = etan[i]; }
            for (int j = tid; j < nu; j += NT) { if (st == 0) dur[j] += g[j]; mu[j] = 0.0; }
            for (int i = tid; i < xw; i += NT) T.dxref[kb * xw + i] = 0.0;
        }
        for (int i = tid; i < nx; i += NT) T.lam[kb * nx + i] = lam[i];      // (the thread that wrote lam[i])
        if (EST) for (int i = tid; i < nx; i += NT) T.eta[kb * nx + i] = eta[i];
        if (tid == 0) { T.st[kb] = st; T.nact[kb] = nact; T.nweak[kb] = nweak; }
        __syncthreads();
    }
    for (int j = tid; j < nu; j += NT) { T.dum1[(size_t)b * nu + j] = mu[j]; T.duref[(size_t)b * nu + j] = dur[j]; }
    if (tid == 0) T.nfactor[b] = nfac;
}

template <int NB>
__global__ __launch_bounds__(NT) void k_rollout_adjoint(Lay L, Ptrs P, AdjointArgs Q, RolloutTape T, RolloutSweep W) { rollout_adjoint_body<NB, false, false>(L, P, Q, T, W, RolloutSlots{}, RolloutGains{}); }
// the same sweep over a tape of the output-feedback loop (mpcqp_rollout_est)
template <int NB>
__global__ __launch_bounds__(NT) void k_rollout_adjoint_est(Lay L, Ptrs P, AdjointArgs Q, RolloutTape T, RolloutSweep W) { rollout_adjoint_body<NB, true, false>(L, P, Q, T, W, RolloutSlots{}, RolloutGains{}); }
// the same sweep over a tape of the loop under a model schedule (mpcqp_rollout_tv)
template <int NB>
__global__ __launch_bounds__(NT) void k_rollout_adjoint_tv(Lay L, Ptrs P, AdjointArgs Q, RolloutTape T, RolloutSweep W, RolloutSlots V) { rollout_adjoint_body<NB, false, true>(L, P, Q, T, W, V, RolloutGains{}); }
// the same sweep over a tape of the output-feedback loop under a model schedule (mpcqp_rollout_tv_est)
template <int NB>
__global__ __launch_bounds__(NT) void k_rollout_adjoint_tv_est(Lay L, Ptrs P, AdjointArgs Q, RolloutTape T, RolloutSweep W, RolloutSlots V, RolloutGains X) { rollout_adjoint_body<NB, true, true>(L, P, Q, T, W, V, X); }
