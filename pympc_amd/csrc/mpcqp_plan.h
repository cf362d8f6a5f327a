// mpcqp_plan.h -- part of libmpcqp_hip, HOST ONLY (included by mpcqp.hip behind the format headers; tests/plan_driver.hip runs it without a GPU).
// The plan of a handle: everything mpcqp_create decides from (compute units, batch, nx, nu, Np, Nc, settings) before it allocates --
//   which KKT backend the handle runs on, what its workgroup keeps in LDS, which k_mpc_run instantiation it launches --
// and the arithmetic the getters of include/mpcqp.h do on that decision.  Integer arithmetic only: no hip* call, no allocation, no handle.
// make_plan is a sequence of named steps, each reading the partial plan and adding its part; the ORDER matters (the work area is widened, reset and
// widened again; the waves, the staged round and the hot prefix feed each other) and is the order of make_plan's body.
#pragma once

struct Plan {
    int ncu = 0, batch = 0;       // what the plan was made for: compute units of the device (0: unknown), instances
    Lay L = {};
    bool lds_state = false;       // the iterate x, z, y lives in LDS behind the common block (owner-mapped rounds)
    size_t smem = 0;              // bytes of dynamic LDS of every kernel that gets the full block (setup's factorization, solve, export, verification)
    long long fsz = 0;            // factor doubles per instance
    RunKernelId kernel = {};      // the k_mpc_run instantiation of the handle's solves and closed-loop runs
};

constexpr size_t LDS_PER_CU = 160 * 1024;
constexpr int BCR_STAGES = 31;      // the largest stage count the register-resident cyclic reduction is instantiated for (Np = 30: the BASELINE shape)
// The static schedule of mpcqp_lat.h exists for 11, 21 and 31 stages; a problem runs the smallest one that holds its N = Np + 1 stages (the rest
// are identity padding: factor_bcr).  0: too long a horizon for this backend.
static int bcr_schedule(int N) { return N <= 11 ? 11 : N <= 21 ? 21 : N <= BCR_STAGES ? BCR_STAGES : 0; }

static Lay make_layout(int nx, int nu, int Np, int Nc, int soft) {
    Lay L; memset(&L, 0, sizeof(L));
    L.nx = nx; L.nu = nu; L.Np = Np; L.Nc = Nc; L.N = Np + 1; L.nb = nx + nu;
    L.n_x = L.N * nx; L.n_u = Nc * nu;
    L.soft = soft ? 1 : 0;
    L.n = (L.soft ? 2 : 1) * L.n_x + L.n_u; L.m = 2 * L.n_x + L.n_u + (Nc + 1) * nu;
    L.ou = L.n_x; L.oe = L.n_x + L.n_u;
    L.rs = L.n_x; L.ri = 2 * L.n_x; L.rdu = 2 * L.n_x + L.n_u;
    L.NB = L.nb <= 16 ? 16 : L.nb <= 32 ? 32 : L.nb <= 64 ? 64 : 128;
    L.border = Nc < Np ? 1 : 0;
    L.NcT = L.border ? Nc - 1 : Nc;
    L.rnx = 1.0f / (float)nx; L.rnu = 1.0f / (float)nu;
    int o = 0;
    L.oAd = o; o += nx * nx; L.oBd = o; o += nx * nu;
    L.oxmin = o; o += nx; L.oxmax = o; o += nx;
    L.oumin = o; o += nu; L.oumax = o; o += nu; L.oDumin = o; o += nu; L.oDumax = o; o += nu;
    L.ouref = o; o += nu; L.oeps = o; o += 1;
    L.hot_sz = o;
    L.oQx = o; o += nx * nx; L.oQxN = o; o += nx * nx; L.oQu = o; o += nu * nu; L.oQDu = o; o += nu * nu;
    L.model_sz = o;
    L.hot_lds = L.hot_sz;                              // (plan_hot_prefix: model_sz where the weight matrices fit in LDS beside everything else)
    L.odu0 = nx + nu + L.N * nx;
    L.od = L.odu0 + 2 * nu;
    L.step_sz = L.od + Np * nx;
    L.d_rows = 0;
    L.raw = 0;
    L.xref_rows = 1;
    L.fstage = L.NB == 16 ? FactorFmt<16>::STAGE : L.NB == 32 ? FactorFmt<32>::STAGE : L.NB == 64 ? WideFmt::STAGE : HugeFmt::STAGE;
    L.fhead = L.NB == 16 ? FactorFmt<16>::HEAD : L.NB == 32 ? FactorFmt<32>::HEAD : 0;
    L.ffwd = L.NB == 16 ? FactorFmt<16>::FWD : L.NB == 32 ? FactorFmt<32>::FWD : L.NB == 64 ? WideFmt::NN : HugeFmt::NN;      // (non-zero: the factor starts at the stages)
    L.ftab = L.NB == 16 ? FactorFmt<16>::TAB : L.NB == 32 ? FactorFmt<32>::TAB : 0;
    L.tsz = L.m + L.N * L.NB * (L.NB >= 64 ? 2 : 1);   // [W (m) | Tc (N*NB)] (+ the second stage-major vector of the wide solve); the plan widens it where the factorization needs more
    L.NR = L.N * L.nb; L.dld = L.NR | 1;               // dense mode (plan_backend): unknowns, odd LDS row stride
    L.nw = NWAVES; L.bcrtop = 0;                        // (plan_backend: eight waves and a dense top for the kernels of mpcqp_w8.hip)
    return L;
}

static size_t state_doubles(const Lay &L) { return (size_t)(L.n + 2 * L.m); }

// ---- the steps of make_plan, in its order -----------------------------------------------------------------------------------------------
// Small problems keep the iterate x, z, y in LDS behind the common block (four workgroups per CU: 40 KB each); larger ones keep it in L2/HBM.
// (an LDS-resident iterate's termination check reads the weight matrices from LDS too -- check_norms_own: behind W in the work area unless
//  they are staged with the hot prefix -- so the work area of such a handle holds at least W and them: short horizons of wide stages only)
static void plan_lds_state(Plan &p) {
    Lay &L = p.L;
    const int tsz_plain = L.tsz;
    if (L.NB <= 32) L.tsz = std::max(L.tsz, L.m + (L.model_sz - L.hot_sz));
    p.lds_state = L.NB <= 32 && sizeof(double) * ((size_t)smem_common_doubles(L) + state_doubles(L)) <= 40 * 1024 && L.m <= 4 * NT && L.N * L.NB <= 2 * NT && L.n_u + L.nu <= NT;      // (the owner map of the parallel phases: two state elements and one input element per thread)
    if (!p.lds_state) L.tsz = tsz_plain;
}

// Eligibility.  The smallest problems (the reference's own examples) solve the KKT system with a register-resident dense inverse (mpcqp_dense.h).
static bool dense_shape(const Plan &p) { return p.lds_state && p.L.NB == 16 && p.L.NR <= DenseFmt::ROWS; }      // (Nc < Np included: the dense inverse holds the held input's couplings itself)
// Block cyclic reduction, factor resident on the compute unit: 16 x 16 stages and horizons of up to 30 steps -- the BASELINE shape (12, 4, 30) with
// compile-time dimensions, anything else with nx + nu <= 16 through the generic instantiations.
static bool bcr_shape(const Plan &p) { return !p.L.dense && p.lds_state && p.L.NB == 16 && !p.L.border && bcr_schedule(p.L.N) > 0; }

// The AUTO cross-overs.
// Dense: up to six instances per compute unit -- measured on (3,1,30), (4,1,20), (2,2,12), (6,2,10), (12,4,7), device loop: ahead of both other backends by
// 1.2 - 2.3 x up to 512 instances, by 0.94 - 1.4 x at 1024, behind the bandwidth kernel by 0 - 18 % at 2048.
static bool auto_dense(const Plan &p) { return p.ncu <= 0 || p.batch <= 6 * p.ncu; }
// Cyclic reduction: up to three instances per compute unit (one resident, the others queued); larger batches stream the chain format (the bandwidth
// backend).  Measured against the bandwidth kernel (device loop and stepwise path, 1024 .. 4096 instances; LAB_NOTES.md):
//   * horizons of 21 .. 30 steps (the 31-stage schedule: every wave owns one group of four stages and the kernel runs on five barriers per iteration, mpcqp_latw.h) with
//     stages too wide for the bandwidth kernel to pack two per block (nx + nu > 8): at EVERY batch size -- (12,4,30) 1.52 / 1.66 / 1.72 M solves/s against 1.28 / 1.37 /
//     1.47 M at 1024 / 2048 / 4096 instances, (12,4,25) 1.54 / 1.69 / 1.75 against 1.43 / 1.50 / 1.68, (8,8,30) 1.93 / 2.13 / 2.20 against 1.50 / 1.72 / 1.94, (6,3,28) 1.80 /
//     1.90 / 2.02 against 1.44 / 1.77 / 1.88, (10,6,24) 1.79 / 1.88 / 1.93 against 1.60 / 1.77 / 2.01, (12,4,21) level (1.56 / 1.69 / 1.75 against 1.59 / 1.70 / 1.84);
//   * anything else it is eligible for: up to three instances per compute unit -- at 768 instances (12,4,10) 2.32 against 2.21, (6,2,20) 1.71 / 1.61; beyond that the
//     bandwidth kernel is ahead on short or padded schedules ((12,4,10) 2.63 against 2.36 at 1024, (12,4,14) 2.17 / 1.80) and on stages it packs ((6,2,20) 2.63 / 2.04 and
//     (5,1,30) 1.72 / 1.63 at 2048).
static bool auto_bcr(const Plan &p) {
    const bool any_batch = bcr_schedule(p.L.N) == 31 && p.L.N >= 22 && p.L.nb > 8;
    return p.ncu > 0 && (any_batch || p.batch <= 3 * p.ncu);
}

// Backend: mpcqp_settings.backend forces a choice -- what tests/test_gpu_backends.py runs every eligible fixture through; a forced backend the shape
// is not eligible for is refused, never silently replaced.
static int plan_backend(Plan &p, int want, std::string *why) {
    Lay &L = p.L;
    auto refuse = [&](const char *what) { *why = std::string("mpcqp_create: backend ") + what + " is not available for this shape"; return (int)MPCQP_ERR_UNSUPPORTED; };
    if (want < MPCQP_BACKEND_AUTO || want > MPCQP_BACKEND_BCRT) { *why = "mpcqp_create: unknown mpcqp_settings.backend"; return MPCQP_ERR_ARG; }
    if (want == MPCQP_BACKEND_DENSE && !dense_shape(p)) return refuse("DENSE");
    const bool dense = dense_shape(p) && (want == MPCQP_BACKEND_DENSE || (want == MPCQP_BACKEND_AUTO && auto_dense(p)));
    L.dense = dense ? 1 : 0;
    if (dense) L.tsz += DenseFmt::SCRATCH;
    const bool want_bcr = want == MPCQP_BACKEND_BCR || want == MPCQP_BACKEND_BCR8 || want == MPCQP_BACKEND_BCRT;
    if (want_bcr && !bcr_shape(p)) return refuse("BCR");
    const bool bcr = bcr_shape(p) && (want == MPCQP_BACKEND_AUTO ? auto_bcr(p) : want_bcr);
    L.bcr = bcr ? bcr_schedule(L.N) : 0;
    // What AUTO runs it on: 512-thread workgroups (two waves per SIMD) with a dense top (mpcqp_latw.h, mpcqp_w8.hip) -- 128 / 256 / 512 instances
    // 608 k / 1.03 M / 1.13 M solves/s against 506 k / 841 k / 935 k on four waves with the plain reduction (MPCQP_BACKEND_BCR, mpcqp_lat.h).
    // MPCQP_BACKEND_BCRT: the dense-top format on four waves (533 k / 890 k: what the eight waves add on top of the format).  DESIGN.md section 5b.
    const bool bcr8 = bcr && (want == MPCQP_BACKEND_BCR8 || want == MPCQP_BACKEND_AUTO);
    const bool bcrt = bcr8 || (bcr && want == MPCQP_BACKEND_BCRT);
    L.bcrtop = bcrt ? BcrFmt::top_count(L.bcr) : 0;
    L.nw = bcr8 ? 8 : NWAVES;
    return MPCQP_OK;
}

// Grouping.  Small stages (nx + nu <= 8) that neither of the register-resident backends takes: several stages per 16 x 16 block (mpcqp_group.h) -- the
// chain and the factor shrink by the group size.  (Worth it once the chain is long: at least three super-stages.)
static void plan_grouping(Plan &p, int tuning) {
    Lay &L = p.L;
    const int grp = (!L.dense && !L.bcr && L.NB == 16 && group_size(L.nb) >= 2 && group_count(L.N, group_size(L.nb)) >= 3 && !(tuning & MPCQP_TUNE_NO_GROUPING)) ? group_size(L.nb) : 0;
    L.grp = grp;
    if (grp) {
        L.fstage = GroupFmt::REC; L.fhead = 0; L.ffwd = GroupFmt::NN; L.ftab = 0;
        L.tsz += (group_count(L.N, grp) + 2) * L.NB;    // the grouped vector Tg behind Tc (+ the two slots of the middle stage's inputs)
    }
}

static long long plan_factor_doubles(const Plan &p) {
    const Lay &L = p.L;
    return L.dense ? (long long)DenseFmt::DOUBLES : L.bcr ? BcrFmt::doubles(L.bcr, L.bcrtop > 0) : L.grp ? (long long)(group_count(L.N, L.grp) + 1) * GroupFmt::REC
                   : (long long)L.fhead + (long long)L.N * L.fstage;
}

// Work-area size: returns the bytes of the full LDS block.  The factorization's workspace starts at the work area T, the last part of the common block,
// and may run on into the iterate area (dead while a factorization runs); T is widened only where even that is short.
static size_t plan_work_area(Plan &p) {
    Lay &L = p.L;
    const int NS = L.bcr;                                           // stages of the schedule (>= L.N)
    if (L.bcr) L.tsz = std::max(L.tsz + NS * L.NB, LAT_LDS_DOUBLES(NS));      // the stage-major vectors of the latency round (mpcqp_lat.h); c_e of the streaming solve
    const size_t state = p.lds_state ? state_doubles(L) : 0;
    const int toplds = L.bcrtop ? LATW_TOP_LDS(NS) + 2 : 0;      // the round's LDS copy of the top inverse, behind the iterate (+ alignment slack)
    const int fws = L.dense ? L.NR * L.dld + 2 * DenseFmt::ROWS + L.m + L.n : L.bcr ? BcrFmt::lds_doubles(L.nw, L.m + L.n, L.bcrtop)
                  : (L.NB == 16 ? FactorCfg<16>::WS : L.NB == 32 ? FactorCfg<32>::WS : L.NB == 64 ? WideFmt::WS : HugeFmt::WS);
    // (a held input, Nc < Np: border_factor also forms Sigma and its inverse, 2 nu^2 doubles, at the start of T -- more than any factorization
    //  workspace once nu is large: (30, 40, 3, 2) needs 3 200 doubles where the 128-wide factorization asks for 264)
    const int need = std::max(fws, (L.border && !L.dense) ? 2 * L.nu * L.nu : 0);
    const int avail = L.tsz + (int)state + toplds;
    if (avail < need) L.tsz += need - avail;
    return sizeof(double) * ((size_t)smem_common_doubles(L) + state + (size_t)toplds);      // every kernel gets the full block
}

// Staged round: returns the bytes it adds.  At most one instance per compute unit and an iterate that does not qualify for the LDS-resident owner map:
// stage it (with the metric vectors, the linear cost and the border matrices) into LDS for the length of a round if one workgroup's LDS holds it
// (admm_round_global).
static size_t plan_staged_round(Plan &p, int tuning) {
    Lay &L = p.L;
    const size_t stage_doubles = 2 * (size_t)L.n + 3 * (size_t)L.m + (size_t)(L.n_x + L.n_u) + (L.border ? 2 * (size_t)L.nu * L.N * L.NB + (size_t)L.nu * L.nu : 0);
    const bool specialised = L.NB == 32 && L.nx == 20 && L.nu == 8 && !L.border;      // (the BASELINE cfg-5 instantiation has compile-time dimensions and no staged round)
    const bool lstage = !p.lds_state && !L.dense && !L.bcr && !specialised && p.ncu > 0 && p.batch <= p.ncu && p.smem + sizeof(double) * stage_doubles <= 150 * 1024
                        && !(tuning & MPCQP_TUNE_NO_LSTAGE);
    L.lstage = lstage ? 1 : 0;
    if (!lstage) return 0;
    size_t more = sizeof(double) * stage_doubles;
    // ... and of those, the ones on grouped stages (nx + nu <= 8 on a long horizon: the reference's notebook (4,1,150,75) and Kalman (4,1,200,200)
    // examples with compile-time dimensions, anything else generically) run the 512-thread instantiation of the same kernel (mpcqp_w8.hip):
    // eight waves for the owner passes that are half of their iteration
    if (L.grp > 1 && !(tuning & MPCQP_TUNE_NO_W8)) {
        more += sizeof(double) * 16 * (8 - L.nw);      // (the reduction scratch grows with the waves: smem_common)
        L.nw = 8;
    }
    return more;
}

// The ONLY place that decides which k_mpc_run instantiation a handle runs: a row of MPCQP_RUN_KERNELS_256 or MPCQP_RUN_KERNELS_512 (mpcqp_defs.h).
// Compile-time nx, nu for the BASELINE configurations and the reference's cart pole (its example system, and the Kalman notebook's long horizon, in
// the global-iterate kernel); generic kernels otherwise.
static RunKernelId run_kernel_id(const Plan &p) {
    const Lay &L = p.L;
    const bool w8 = L.nw == 8, lds = p.lds_state;
    auto dims = [&](int nx, int nu) { return L.nx == nx && L.nu == nu; };
    if (L.dense) return {16, true, 0, 0, MODE_DENSE, false};
    if (L.bcr) {                                        // (w8: cyclic reduction with a dense top on eight waves)
        const int mode = (L.bcrtop ? MODE_BCRT : MODE_BCR) + L.bcr;
        return L.bcr == 31 && dims(12, 4) ? RunKernelId{16, true, 12, 4, mode, w8} : RunKernelId{16, true, 0, 0, mode, w8};
    }
    const int mode = L.border ? MODE_BORDER : MODE_CHAIN;
    const bool spec = (L.NB == 16 && !lds && dims(4, 1))                                   // (w8: one long-horizon controller on grouped stages, round staged in LDS)
                   || (!w8 && !L.border && ((L.NB == 16 && lds && dims(12, 4)) || (L.NB == 32 && !lds && dims(20, 8))));
    return {L.NB, lds, spec ? L.nx : 0, spec ? L.nu : 0, mode, w8};
}

// Workgroups of the planned kernel per compute unit by its __launch_bounds__: one for 512-thread handles, otherwise the constexpr rule of mpcqp_kernels.h.
static int kernel_occupancy(const RunKernelId &k) { return k.w8 ? 1 : run_occupancy(k.nb, k.mode); }

// Hot-prefix placement: returns the bytes it adds.  The weight matrices [Qx | QxN | Qu | QDu] ride with the hot prefix into LDS (Lay::hot_lds) where that
// costs no residency: the kernels that run one workgroup per compute unit (latency backends, 512 threads, wide stages) or two (32 x 32 stages), not the
// four-per-CU bandwidth kernel of 16 x 16 stages, whose 40 KB are spoken for.
static size_t plan_hot_prefix(Plan &p) {
    Lay &L = p.L;
    const size_t extra = sizeof(double) * (size_t)(L.model_sz - L.hot_sz);
    if ((p.smem + extra + 1024) * (size_t)kernel_occupancy(p.kernel) > LDS_PER_CU) return 0;
    L.hot_lds = L.model_sz;
    return extra;
}

static int plan_check_dims(int batch, int nx, int nu, int Np, int Nc, std::string *why) {
    if (batch < 1 || nx < 1 || nu < 1 || Np < 2 || Nc < 1 || Nc > Np) { *why = "mpcqp_create: bad dimensions"; return MPCQP_ERR_ARG; }
    if (nx + nu > 128) { *why = "mpcqp_create: nx+nu > 128 is not implemented"; return MPCQP_ERR_UNSUPPORTED; }
    return MPCQP_OK;
}

// ncu: compute units of the device the handle is for (0: unknown -- AUTO then keeps to what needs no batch-per-unit figure).
// MPCQP_OK, or MPCQP_ERR_ARG / MPCQP_ERR_UNSUPPORTED with the reason in *why.
static int make_plan(int ncu, int batch, int nx, int nu, int Np, int Nc, const mpcqp_settings &S, Plan *out, std::string *why) {
    if (int rc = plan_check_dims(batch, nx, nu, Np, Nc, why)) return rc;
    Plan p;
    p.ncu = ncu; p.batch = batch;
    p.L = make_layout(nx, nu, Np, Nc, S.soft_constraints);
    plan_lds_state(p);
    if (int rc = plan_backend(p, S.backend, why)) return rc;
    plan_grouping(p, S.tuning);
    p.smem = plan_work_area(p);
    p.fsz = plan_factor_doubles(p);
    p.smem += plan_staged_round(p, S.tuning);
    p.kernel = run_kernel_id(p);
    p.smem += plan_hot_prefix(p);
    if (p.smem > LDS_PER_CU) { *why = "problem too large for one workgroup's LDS"; return MPCQP_ERR_UNSUPPORTED; }
    // check_norms_own reads the weight matrices through LDS views (as_lds): with an LDS-resident iterate they must BE in LDS -- staged with the hot
    // prefix, or behind W in the work area.  The sizing above guarantees it; a layout change that breaks it must fail here, not give wrong residuals.
    if (p.lds_state && p.L.hot_lds == p.L.hot_sz && p.L.tsz - p.L.m < p.L.model_sz - p.L.hot_sz) {
        *why = "mpcqp_create: internal layout error: the weight matrices of an LDS-resident handle do not fit behind W"; return MPCQP_ERR_UNSUPPORTED;
    }
    *out = p;
    return MPCQP_OK;
}

// ---- what the getters of include/mpcqp.h report: arithmetic on the plan ------------------------------------------------------------------
// How many workgroups of the handle's solve kernel one compute unit holds at a time: the kernel's __launch_bounds__ occupancy, capped by what the
// dynamic LDS block leaves room for.  (bench.py's "instances in flight" -- what the memory-side cache sees -- is this times the compute units.)
static int plan_occupancy(const Plan &p) {
    const int occ = kernel_occupancy(p.kernel);
    return p.smem > 0 ? std::max(1, std::min(occ, (int)(LDS_PER_CU / p.smem))) : occ;
}
static int plan_threads(const Plan &p) { return p.kernel.w8 ? 512 : 256; }

// The name of the instantiation, spelled as rocprofv3 prints it (without spaces) -- so that bench.py and the profile summaries name the same kernel.
static void run_kernel_name(const RunKernelId &k, bool loop, char *buf, size_t buflen) {
    snprintf(buf, buflen, "%sk_mpc_run<%d,%s,%d,%d,%d,%s>", k.w8 ? "w8::" : "", k.nb, k.ldss ? "true" : "false", k.nxt, k.nut, k.mode, loop ? "true" : "false");
}

static void plan_dims(const Plan &p, int *n, int *m, int64_t *factor_doubles, int64_t *nnzL) {
    const Lay &L = p.L;
    if (n) *n = L.n;
    if (m) *m = L.m;
    if (factor_doubles) *factor_doubles = p.fsz;
    if (nnzL) {      // structural nonzeros of the block factor (diagonal included) + the eliminated eps pivots
        int64_t nb = L.nb, nx = L.nx;
        const int64_t T = L.NcT;                       // stages with an input inside the tridiagonal part
        int64_t full = T * (nb * (nb + 1) / 2) + (int64_t)(L.N - T) * (nx * (nx + 1) / 2);
        int64_t sub = (T > 0 ? (T - 1) * (nx * nb + (int64_t)L.nu * L.nu) + nx * nb : 0) + (int64_t)(L.N - 1 - T) * nx * nx;
        int64_t border = L.border ? (int64_t)L.nu * (L.n_x + T * L.nu) + (int64_t)L.nu * (L.nu + 1) / 2 : 0;
        *nnzL = full + sub + border + (L.soft ? 2 * (int64_t)L.n_x : 0);
    }
}

// Bytes one instance moves between the memory system (HBM / Infinity Cache / L2) and its compute unit BY DESIGN of these
// kernels -- the roofline numerator bench.py uses ("Roofline accounting"):
//   per ADMM iteration : the factor stream (FactorFmt, mpcqp_factor.h).  16 x 16 stages: forward matrices of N-1 stages, packed
//                        S^-1 of N stages, N-1 stage tables and [G | G'], once each; 32 x 32 stages (S^-1-only): packed S^-1
//                        twice, one table per sweep, [G | G'] by each sweeping wave.  Problems whose iterate does not fit
//                        LDS also read and write x, z, y and read omega, s, q every iteration; Nc < Np adds the two border matrices.
//   per round (check)  : residual evaluation inputs (weights, D, E, omega, s, last increments), the round's load/store of
//                        the LDS-resident iterate and of the per-thread register copies of omega, s, q.
//   per solve          : the begin phase (step data, E, constraint types, q rebuild) and the solution write-out.
//   an affine term    : (Lay::d_rows > 0) its Np nx doubles, counted once per solve (begin's type check) -- and once per ITERATION where the iterate is not
//                        LDS-resident (gown_update); nothing without one.  NOT counted: the owners of the LDS-resident rounds (own_load, admm_tiny, admm_lat,
//                        admm_latw) read their entry again at the start of every round, Np nx doubles more per round out of L2 -- beside the round's
//                        3 (n + 2 m) and more it is under 2 %, and the model leaves it out as it leaves out the x0 / bounds they re-read there.
static void plan_stream_bytes(const Plan &p, int64_t *per_iter, int64_t *per_round, int64_t *per_solve) {
    const Lay &L = p.L;
    const int64_t n = L.n, m = L.m, nq = L.n_x + L.n_u, NB = L.NB;
    const int64_t aff = L.d_rows ? (int64_t)L.Np * L.nx : 0, step_rd = L.step_sz - (int64_t)L.Np * L.nx + aff;      // (the step blob as a solve reads it)
    const int64_t sinv = L.fstage - L.ffwd - L.ftab;
    int64_t it = (L.dense || L.bcr) ? 0 /* the factor sits in registers for the round */ : !L.ffwd ? 2 * (int64_t)L.N * sinv + (int64_t)L.N * L.ftab + 2 * (int64_t)L.fhead   // S^-1-only build: S^-1 twice, one of the two tables per sweep, [G | G'] by each sweeping wave
                         : (int64_t)(L.N - 1) * L.ffwd + (int64_t)L.N * sinv + (int64_t)(L.N - 1) * L.ftab + L.fhead;   // forward matrices once, S^-1 once, the tables, G / G' once each
    if (L.NB >= 64) it = (3 * (int64_t)L.N - 2) * (int64_t)L.NB * L.NB;      // wide stages: S^-1 of every stage, M and M' of all but the last
    if (L.grp) it = (3 * (int64_t)group_count(L.N, L.grp) - 1) * GroupFmt::NN;      // grouped small stages: S^-1 of every super-stage, forward matrix and its transpose of all but the ends, the middle's second pair
    if (!p.lds_state && !L.lstage) it += (2 * n + 4 * m) /* x, z, y read + written */ + (m + L.n_x) /* omega */ + (n + L.n_x) /* s */ + nq /* q */;
    if (!p.lds_state && !L.dense && !L.bcr) it += aff;
    if (L.border && !L.dense) it += 2 * (int64_t)L.nu * L.N * NB;      // (the dense inverse holds the held input's couplings itself)
    int64_t rd = (L.model_sz - L.hot_lds) /* the weight matrices, unless they are staged with the hot prefix */ + 2 * n + 2 * m /* D, s, E, omega */ + n + m /* dx, dy */;
    if (L.dense) rd += DenseFmt::DOUBLES;               // the round's load of K^-1 into registers
    if (L.bcr && !L.bcrtop) rd += (int64_t)L.bcr * BcrFmt::REC - 4 * BcrFmt::NN;      // ... of the cyclic-reduction fragments (the two end stages have one neighbour)
    int64_t fr = 0;
    if (L.bcrtop) {                                     // ... of levels 0 and 1 (the top inverse and G, G' enter LDS once per kernel prologue: admm_latw)
        for (int l = 0; l < 2; ++l) for (int kind = 0; kind < 3; ++kind) for (int t = 0; t < lat_count(L.bcr, l, kind); ++t) fr += lat_nfr(L.bcr, l, kind, t);
        rd += fr * BcrFmt::NN;
    }
    rd += (p.lds_state || L.lstage) ? 2 * (n + 2 * m) /* iterate in and out of LDS */ + (m + L.n_x) + (n + L.n_x) + nq : (n + 2 * m);
    if (L.lstage && L.border) rd += 2 * (int64_t)L.nu * L.N * NB;      // the border matrices staged with it
    int64_t sv = L.hot_lds + step_rd + 3 * m /* E, types, omega */ + nq + 2 * (n + m) /* solution out, iterate read */;
    if (L.bcrtop && L.nw == 8 && (L.bcr + 3) / 4 <= 8 && L.hot_lds > L.hot_sz) {
        // The 512-thread latency round with its own termination test (latw_check): a round boundary moves the level fragments, the increments (written by
        // the last iteration, read back by the test) and the three scalings per lane the test clips the certificates with; the owners' registers are
        // loaded once per SOLVE (iterate, metric, linear cost), the iterate, the solution and the record written once per solve; the top inverse and the hot
        // prefix enter LDS once per kernel prologue -- per queue item of a persistent closed-loop launch, about every fifth solve (QUEUE_ITEMS_PER_SLOT).
        // (Spill traffic around the non-inlined test -- ~ 110 bytes per lane and round in the write counter -- is NOT design traffic and not in here.)
        rd = fr * BcrFmt::NN + 2 * (n + m) /* dx, dy out and back */ + 3 * 64 * 8 /* E of the owned rows */;
        sv = step_rd + 3 * m + nq                                              /* begin: E, types, omega looked at, q written */
           + (2 * n + 3 * m + nq)                                              /* the round's prologue: x, s, q, omega, z, y */
           + (n + 2 * m) + (n + m)                                             /* the solve's end: iterate, reported solution */
           + ((int64_t)L.bcrtop * L.bcrtop * BcrFmt::NN + L.hot_lds) / 5;     /* kernel prologue, amortised */
    }
    if (per_iter) *per_iter = 8 * it;
    if (per_round) *per_round = 8 * rd;
    if (per_solve) *per_solve = 8 * sv;
}

// Matrix-core instructions (v_mfma_f64_4x4x4_4b_f64, 512 flop each, a quarter of them useful in a mat-vec) one instance issues per
// ADMM iteration with this plan's backend -- the numerator of the MFMA roofline bench.py reports for the latency backend.
static int64_t plan_mfma_per_iter(const Plan &p) {
    const Lay &L = p.L;
    int64_t mv = 0;                                  // 16 x 16 mat-vecs (four MFMAs each)
    if (L.dense || L.NB >= 64) mv = 0;               // vector ALU only
    else if (L.bcr) {
        for (int l = 0; l < (L.bcrtop ? 2 : bcr_levels(L.bcr)); ++l)
            for (int kind = 0; kind < 3; ++kind) for (int t = 0; t < lat_count(L.bcr, l, kind); ++t) mv += lat_nfr(L.bcr, l, kind, t);
        // (the dense top runs on the vector ALU: 512 nt^2 flop per iteration, not counted here)
        mv += 2 * ((L.bcr + 3) / 4);                 // G v and G'W: one group per four stages each
    } else if (L.grp) mv = 3 * (int64_t)group_count(L.N, L.grp) - 1;      // forward 1, backward 2 mat-vecs per super-stage, the middle stage
    else {
        const int64_t blk = (L.NB / 16) * (L.NB / 16);
        mv = L.ffwd ? (int64_t)(L.N - 1) * blk * 3 + 3 * blk : (int64_t)(L.N - 1) * blk * 4 + 3 * blk;      // forward 1 (or 2) + backward 2 mat-vecs per stage, the middle stage
    }
    return 4 * mv;
}
