// mpcqp_latw_check.h -- part of libmpcqp_hip (included by mpcqp.hip and mpcqp_w8.hip behind mpcqp_kernels.h).
// OSQP's termination test (update_info + check_termination: what check_body of mpcqp_phases.h evaluates on the iterate's LDS copy) in the OWNER
// layout of the latency round (mpcqp_latw.h: lane (I, B, J) of wave w owns slot a = 4B + I of stage s = 4w + J -- one group of four stages per
// wave), called by admm_latw between two rounds with the owned values BY VALUE:
//   * A x and A'y are the two MFMA groups of the iteration (G v of the previous stage, G' y_dyn of the next) applied to x and y, P x a 16-long dot
//     product per lane against the weight matrices' LDS copy; the residuals, their scales and the objective meet in one block reduction of five
//     values (latw_reduce below: one barrier), and ONLY where the solve has not converged the cheap halves of both infeasibility certificates
//     (|c dy| clipped by the infinite bounds and the support function of [l, u]; |dx| and q'dx) in a second one of four;
//   * LATW_SOLVED: the solve is finished here -- iterate for the next warm start, reported solution, mpcqp_info, statistics, first input and status
//     for the closed loop on the device: everything check_body's tail writes;
//   * LATW_CARRIED: solved, and the queue item has another step: its transition (latw_carry below, inline) is made in the same call -- one entry, one
//     return, one set of kernel-argument loads, and everything the transition reads from memory was requested behind the check's first barrier;
//   * LATW_CONTINUE: not converged and neither certificate can hold: the caller starts the next round at once, fragments and owner registers
//     where they are;
//   * LATW_GENERIC: anything else (a certificate that needs its operator product, a non-finite residual, the first launch of a two-launch
//     solve): the caller writes the iterate back and the generic check does what it always did.
// A function of its own on purpose: see the head of admm_latw.  Its budget is the caller's: what the function clobbers the caller saves around the
// call.  It has 80 VGPRs; the (12,4,30) kernel's scratch stays at its 320 bytes up to 106 and is 356 at 117.  Per check of one (12,4,30) instance,
// on the boundary clocks (BTICK, scripts/lat_phase.py; mean over the waves): entry 2.6 k, exchanges 2.0 k, rows and variables 4.1 k, reduction
// 2.1 k, solved tail 1.2 k cycles -- 12 k where the solve ends, not the 4 k this comment used to claim -- and 3.4 k more for a carried transition,
// against 15 k of the generic check plus 10 k of write-back and reload around it.
#pragma once

template <int NXT, int NUT, int NST>
__device__ __forceinline__ int latw_carry(const RunKArgs &KA, Smem &S, int b, int k, int iter, double cc, double wn, double Er, int ct, int r, mpcqp_info inf);      // (below)

// The check's own block reduction: ONE barrier where block_reduce (mpcqp_qp.h) has four.  Each wave's partial results (wave_reduce_last, as there)
// go to red[G i + wv], value by value, G = NWAVES (eight in the 512-thread unit; four in the 256-thread one, which runs the check on schedules of up
// to sixteen stages); behind the barrier lane G i + w of EVERY wave reads value i of wave w -- one LDS read per wave -- and the waves' values meet
// inside the wave: a maximum over its group of G lanes in DPP steps (lane ^ 1, lane ^ 2 and, for eight, the mirror of the half row; a maximum has no
// order), a sum in wave order, v = red[w = 0]; v += red[w], w = 1 .. G - 1, by G - 1 shifts of one lane -- the order block_reduce's thread i uses:
// the same bits; v_readlane hands the K results to every lane.  (Every thread reading all G K values itself was tried first: 160 broadcast reads a
// workgroup through one LDS pipe cost 500 cycles MORE than block_reduce.)  No barrier in front and none behind: red is this reduction's alone (the
// check's two stages use disjoint parts of Smem::red), and between its last read here and its next write lie the barriers of a whole round, of the
// carried transition or of the generic check's own reduction.
typedef __attribute__((address_space(3))) double ldsw;      // (ldsd of mpcqp_phases.h, writable)
template <int KMAX, int KSUM>
__device__ __forceinline__ void latw_reduce(double *vmax, double *vsum, double *red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr int K = KMAX + KSUM, G = NWAVES;
    static_assert((G == 8 || G == 4) && G * K <= 64, "a group of G lanes per value, a lane per wave");
#pragma unroll
    for (int i = 0; i < KMAX; ++i) vmax[i] = wave_reduce_last<true>(vmax[i]);
#pragma unroll
    for (int i = 0; i < KSUM; ++i) vsum[i] = wave_reduce_last<false>(vsum[i]);
    ldsd *rl = as_lds(red);
    ldsw *rw = (ldsw *)rl;
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < KMAX; ++i) rw[G * i + wv] = vmax[i];
#pragma unroll
        for (int i = 0; i < KSUM; ++i) rw[G * (KMAX + i) + wv] = vsum[i];
    }
    __syncthreads();
    const double x = rl[lane < G * K ? lane : 0];
    double m = x;
    m = fmax(m, dpp_move_f64<0xB1>(m));             // quad_perm [1,0,3,2]
    m = fmax(m, dpp_move_f64<0x4E>(m));             // quad_perm [2,3,0,1]
    if constexpr (G == 8) m = fmax(m, dpp_move_f64<0x141>(m));      // row_half_mirror: the other quad of the group
#pragma unroll
    for (int i = 0; i < KMAX; ++i) { vmax[i] = readlane_f64(m, G * i); asm volatile("" : "+v"(vmax[i])); }      // (in a vector register from here on: the function has no scalar pair to spare)
    // (the sums: G - 1 shifts by one lane, acc = acc of the lane below + own value in EVERY lane -- lane k of a group holds the sum of the group's lanes
    //  0 .. k in that order after step k and its last lane the whole sum after the last step; what the other lanes hold meanwhile is never read)
    double acc = x;
#pragma unroll
    for (int w = 1; w < G; ++w) acc = dpp_move_f64<0x111>(acc) + x;      // row_shr:1
#pragma unroll
    for (int i = 0; i < KSUM; ++i) { vsum[i] = readlane_f64(acc, G * (KMAX + i) + G - 1); asm volatile("" : "+v"(vsum[i])); }
}
constexpr int LATW_RED1 = 0, LATW_RED2 = 5 * NWAVES, LATW_FLAG = 16 * NWAVES - 8;      // Smem::red: stage 1 (5 values a wave), stage 2 (4), latw_carry's flag word
static_assert(LATW_RED2 + 4 * NWAVES <= LATW_FLAG, "Smem::red holds 16 doubles per wave");

template <int NXT, int NUT, int NST>
__device__ __noinline__ int latw_check(double pv, double pv2, double ncq, double zA, double ysA, double omA, double zB, double ysB, double omB, double z0, double ys0, double om0,
                                       double loA, double hiA, double loB, double hiB, double cc, int iter, int binst, int *frame_pin) {
    PHASE_PIN_USE(frame_pin);
    constexpr int NB = 16, N = NST, NG = (N + 3) / 4, VS = LAT_VS(N), NTOP = BcrFmt::top_count(N);
    static_assert(NG <= NWAVES, "one group of four stages per wave");
    const RunKArgs &KA = run_kargs();
    const Lay &L = KA.L; const Ptrs &PP = KA.P; const RunArgs &R = KA.R;
    const int b = __builtin_amdgcn_readfirstlane(binst);      // (the instance travels by value: the map entry is not loaded again)
    RunSmem rs = run_smem<true>(L, PP, b);
    Smem &S = rs.S;
    const int nx = NXT ? NXT : L.nx, nu = NUT ? NUT : L.nu, NR = L.N;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double cinv = 1.0 / cc;
    const double *hot = S.hot;
    double *Tc = S.T + NB, *Cc = Tc + VS;
    const double *TopL = rs.Y + L.m + ((smem_common_doubles(L) + L.n + 2 * L.m) & 1);
    // ---- the owner map, as in admm_latw
    const int a = 4 * ((lane >> 2) & 3) + (lane >> 4), J = lane & 3;
    const bool is_x = a < nx;
    const int jj = a - nx;
    const int s = wv < NG ? 4 * wv + J : 4 * NG, sl = s * NB + a;
    const bool ok = is_x ? s < NR : (a < nx + nu && s < NR - 1);
    const int e = s * nx + a, cu = s * nu + jj;
    const int pidx = is_x ? e : L.ou + cu, aidx = is_x ? e : L.ri + cu, bidx = is_x ? L.rs + e : L.rdu + nu + cu;
    const bool u0v = wv == 0 && J == 0 && !is_x && a < nx + nu;
    const int onext = (jj + 1 < nu) ? 1 : NB - nu + 1, oprev = (jj > 0) ? -1 : -(NB - nu + 1);
    cgdouble *dxg = (cgdouble *)(PP.dx + (size_t)b * L.n), *dyg = (cgdouble *)(PP.dy + (size_t)b * L.m);
    cgdouble *Eg = (cgdouble *)(PP.E + (size_t)b * L.m);
    const double lim = QP_INFTY * MIN_SCALING;
    // x in Tc, the first rows' multipliers in Cc -- and, once G'y has been formed, the second rows' in Cc again (every slot 0 .. 4 NG - 1 has an
    // owner that writes it; slots -1 and 4 NG stay zero throughout; the iteration rewrites both vectors before it reads them)
    const double yA = ysA * (omA * cinv), yB = ysB * (omB * cinv), y0 = u0v ? ys0 * (om0 * cinv) : 0.0;
    Tc[sl] = ok ? pv : 0.0; Cc[sl] = ok ? yA : 0.0;
    __syncthreads();
    BTICK(0)
    // the closed loop on the device: may a converged solve be carried into the item's next step right here (Smem::iflag[6], [7]: run_instance's, written
    // before the round began)?  Then what that transition reads from memory -- the next step's disturbance, scaling and current type of the row this
    // thread re-types, rho -- is requested here, before the verdict is known, and consumed in latw_carry: no round trip of its own -- behind the first barrier, where the two
    // flags arrive with the exchange's own LDS reads (in front of it, at the function's entry, waiting for them cost every check 900 cycles).  (w[k + 1] only
    // where step k + 1 is inside the item: no address out of range; the other addresses are the instance's own whatever the verdict.)
    const int kc = __builtin_amdgcn_readfirstlane(S.iflag[6]), ke = __builtin_amdgcn_readfirstlane(S.iflag[7]);
    const bool more = R.nsteps > 0 && kc >= 0 && ke <= R.nsteps && kc + 1 < ke;
    const int rc = tid < nx ? tid : (tid < nx + nu ? L.rdu + (tid - nx) : -1);
    const double wn = (more && tid < nx && R.w) ? ((cgdouble *)R.w)[((size_t)(kc + 1) * R.batch + b) * nx + tid] : 0.0;
    const double Erc = Eg[rc >= 0 ? rc : 0];
    const int ctc = ((const __attribute__((address_space(1))) int *)(PP.ctype + (size_t)b * L.m))[rc >= 0 ? rc : 0];
    const double rho = PP.rho[b];
    const Ctx c{L, hot, hot + L.hot_sz};
    // STAGE 1, every check: what a verdict 'solved' needs and no more.  0 pri, 1 max(|Ax|, |z|), 2 dua, 3 max(|Px|, |A'y|, |q|); sum: the objective.
    // (|Ax| and |z| enter the test only as their maximum, |Px|, |A'y| and |q| only as theirs; a maximum of non-negative numbers is the same in any
    //  grouping, and block_reduce forms every value on its own: pri_res, dua_res, obj_val and every verdict keep their bits.)
    double nrm[4], vsum[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) nrm[i] = 0.0;
    vsum[0] = 0.0;
    auto row = [&](double ax, double z) { nrm[0] = fmax(nrm[0], fabs(ax - z)); nrm[1] = fmax(nrm[1], fmax(fabs(z), fabs(ax))); };
    auto var = [&](double px, double aty, double qj, double xj) {
        nrm[2] = fmax(nrm[2], fabs(px + qj + aty)); nrm[3] = fmax(nrm[3], fmax(fmax(fabs(qj), fabs(aty)), fabs(px)));
        vsum[0] += xj * (0.5 * px + qj);
    };
    double g = 0.0, h2 = 0.0, gt = 0.0, ht = 0.0;
    lat_mv(latw_top_frag(TopL, NTOP * NTOP, lane), Tc[sl - NB], g, h2);            // G v of the previous stage
    lat_mv(latw_top_frag(TopL, NTOP * NTOP + 1, lane), Cc[sl + NB], gt, ht);      // G' y_dyn of the next stage
    const double un = Tc[sl + onext];
    __syncthreads();
    Cc[sl] = ok ? yB : 0.0;
    __syncthreads();
    BTICK(1)
    const double qj = -ncq * cinv;
    if (ok) {
        const double xj = pv, yprev = Cc[sl + oprev];
        const double *xs = Tc + s * NB;
        if (is_x) {
            row((g + h2) - xj, zA);
            row(L.soft ? xj + pv2 : xj, zB);
            const double *Q = (s < L.Np) ? c.Qx() : c.QxN();
            double px = 0.0;
#pragma unroll 4
            for (int l = 0; l < nx; ++l) px += Q[min(a, l) * nx + max(a, l)] * xs[l];
            var(px, (gt + ht) - yA + yB, qj, xj);
            if (L.soft) var(c.eps_feas() * pv2, yB, 0.0, pv2);
        } else {
            row(xj, zA);
            row(un - xj, zB);
            const double iu = (s == L.Nc - 1) ? (double)(L.Np - L.Nc + 1) : 1.0, dk = (s == L.Nc - 1) ? 1.0 : 2.0;
            const double *Qu = c.Qu(), *QDu = c.QDu(), *us = xs + nx;
            double px = 0.0;
            for (int l = 0; l < nu; ++l) { const int lo = min(jj, l), hi = max(jj, l); px += input_weight(iu, Qu[lo * nu + hi], dk, QDu[lo * nu + hi]) * us[l]; }
            if (s + 1 < L.Nc) for (int l = 0; l < nu; ++l) px += -QDu[jj * nu + l] * us[NB + l];
            if (s > 0) for (int l = 0; l < nu; ++l) px += -QDu[l * nu + jj] * us[l - NB];
            double aty = (gt + ht) + yA - yB + yprev;
            if (u0v) { aty += y0; row(xj, z0); }
            var(px, aty, qj, xj);
        }
    }
    if (u0v) S.uo[jj] = pv;      // (the first input, should the verdict be 'solved' -- nobody reads it otherwise: published by the reduction's barriers, for latw_carry)
    BTICK(2)
    latw_reduce<4, 1>(nrm, vsum, S.red + LATW_RED1);
    BTICK(3)
    const double ea = KA.S.eps_abs, er = KA.S.eps_rel;
    const double pri_res = nrm[0], dua_res = nrm[2], obj_val = vsum[0];
    if (!(pri_res <= QP_INFTY) || !(dua_res <= QP_INFTY) || obj_val != obj_val) return LATW_GENERIC;      // (non-finite: the generic check reports it)
    const bool pc = pri_res < ea + er * nrm[1], dc = dua_res < ea + er * nrm[3];
    if (pc && dc) {
        // (what was requested behind the first barrier for the carry arrived long ago.  Its wait is taken HERE, in front of the tail's global stores:
        //  taken at the first use, behind them, it is a vmcnt count that the stores' divergent branches make the compiler put at 3 -- the plant
        //  product then waits until all but three of a dozen stores are acknowledged.)
        asm volatile("" :: "v"(wn), "v"(Erc), "v"(ctc), "v"(rho));
        // ---- solved: what check_body's tail writes (the iterate for the next warm start, the reported solution, the record)
        gdouble *gx = (gdouble *)(PP.x + (size_t)b * L.n), *gz = (gdouble *)(PP.z + (size_t)b * L.m), *gy = (gdouble *)(PP.y + (size_t)b * L.m);
        gdouble *xo = (gdouble *)(PP.xo + (size_t)b * L.n), *yo = (gdouble *)(PP.yo + (size_t)b * L.m);
        if (ok) {
            gx[pidx] = pv; xo[pidx] = pv;
            if (is_x && L.soft) { gx[pidx + L.oe] = pv2; xo[pidx + L.oe] = pv2; }
            gz[aidx] = zA; gy[aidx] = yA; yo[aidx] = yA;
            gz[bidx] = zB; gy[bidx] = yB; yo[bidx] = yB;
        }
        if (u0v) { gz[L.rdu + jj] = z0; gy[L.rdu + jj] = y0; yo[L.rdu + jj] = y0; }
        mpcqp_info inf;                                    // (thread 0's: stored ONCE, here or by the carry)
        inf.status = MPCQP_SOLVED; inf.iter = iter; inf.rho_updates = 0; inf.reserved = 0;
        inf.obj_val = obj_val; inf.pri_res = pri_res; inf.dua_res = dua_res; inf.rho = rho;
        if (tid == 0) {
            inf.rho_updates = S.iflag[1];
            const int checks = (S.iflag[3] += 1);
            S.iflag[4] = MPCQP_SOLVED;
            atomicAdd(&PP.stats[0], (unsigned long long)iter); atomicAdd(&PP.stats[1], (unsigned long long)checks);
            atomicAdd(&PP.stats[2], (unsigned long long)inf.rho_updates); atomicAdd(&PP.stats[3], 1ULL);
            atomicAdd(&PP.work[b], (unsigned)iter);      // (one writer per instance: the sum a load, an addition and a store gave, without the round trip)
        }
        if (!more) { if (tid == 0) PP.info[b] = inf; return LATW_SOLVED; }
        return latw_carry<NXT, NUT, NST>(KA, S, b, kc, iter, cc, wn, Erc, ctc, rc, inf);
    }
    // not converged: may the next round start at once?  Only if neither certificate can hold -- decided from their cheap halves
    if (R.nsteps == 0 && R.part == 1) return LATW_GENERIC;                       // (the first launch of a two-launch solve hands over after ONE round)
    // STAGE 2, only here: the cheap halves of both certificates.  0 |c dy| clipped by the infinite bounds, 1 |dx|;  sums: the support function of
    // [l, u] at c dy, q'dx -- each lane's terms in the order the one-stage check added them.
    double cn[2] = {0.0, 0.0}, cs[2] = {0.0, 0.0};
    auto cert = [&](double dy, double lo, double hi, int bits) {      // OSQP is_primal_infeasible: c dy projected on the polar of the recession cone of [l, u]
        double v = cc * dy;
        if (bits & 1) v = (bits & 2) ? 0.0 : fmin(v, 0.0);
        else if (bits & 2) v = fmax(v, 0.0);
        cn[0] = fmax(cn[0], fabs(v)); cs[0] += hi * fmax(v, 0.0) + lo * fmin(v, 0.0);
    };
    auto dvar = [&](double qv, double dxj) { cn[1] = fmax(cn[1], fabs(dxj)); cs[1] += qv * dxj; };
    // (the last iteration's increments -- each lane reads back what it stored itself for the generic check -- and the owned rows' scaling: requested
    //  HERE, by every lane at clamped addresses in one go.  Requested at the function's entry they cost every check 900 cycles of entry and this stage
    //  300 less; seven checks in ten end solved and never come here.)
    const int ip = ok ? pidx : 0;
    const double ddx = dxg[ip], dde = dxg[(ok && is_x && L.soft) ? ip + L.oe : 0], ddA = dyg[ok ? aidx : 0], ddB = dyg[ok ? bidx : 0];
    const double dd0 = dyg[L.rdu + ((jj >= 0 && jj < nu) ? jj : 0)];
    const double eA = Eg[ok ? aidx : 0], eB = Eg[ok ? bidx : 0], e0 = Eg[L.rdu + ((jj >= 0 && jj < nu) ? jj : 0)];
    if (ok) {
        // which of the owned rows' bounds are infinite on OSQP's scaled test (E hi > 1e26, E lo < -1e26: the primal infeasibility certificate clips the
        // dual increment by them) -- two bits per row: rA 0,1  rB 2,3
        int infbits = (eA * hiA > lim ? 1 : 0) | (eA * loA < -lim ? 2 : 0) | (eB * hiB > lim ? 4 : 0) | (eB * loB < -lim ? 8 : 0);
        if (u0v) cert(dd0, S.du0[jj], S.du0[nu + jj], (e0 * S.du0[nu + jj] > lim ? 1 : 0) | (e0 * S.du0[jj] < -lim ? 2 : 0));
        dvar(qj, ddx);
        if (is_x && L.soft) dvar(0.0, dde);
        cert(ddA, loA, hiA, infbits); cert(ddB, loB, hiB, infbits >> 2);
    }
    latw_reduce<2, 2>(cn, cs, S.red + LATW_RED2);
    BTICK(5)
    // (pc and dc formed again from the first stage's values: kept across the second reduction they are two scalar register pairs more than the
    //  function has, and the spill lane that takes them is a register of the caller's to save and restore around every check)
    const double epi = KA.S.eps_prim_inf, edi = KA.S.eps_dual_inf;
    double s0 = nrm[0], s1 = nrm[1], s2 = nrm[2], s3 = nrm[3];
    asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3));
    const bool pc2 = s0 < ea + er * s1, dc2 = s2 < ea + er * s3;
    if (!pc2 && cn[0] > epi && cs[0] < -epi * cn[0]) return LATW_GENERIC;     // primal infeasibility would need |A' dy|
    if (!dc2 && cn[1] > edi && cs[1] < -edi * cn[1]) return LATW_GENERIC;     // dual infeasibility would need |P dx| and A dx
    if (tid == 0) S.iflag[3] += 1;
    return LATW_CONTINUE;
}

// The closed loop on the device, between two steps of one queue item, without leaving the latency round: the tail of latw_check where the solve has
// converged and the item has another step (Smem::iflag[6] = k, the step whose solve just ended, [7] = the end of the item, 0 where the carry does not
// apply -- the kernel decides: no estimator, no reference trajectory, warm start on, not MPCQP_TUNE_NO_CARRY).  What the kernel's loop body and
// begin_body would do, in their arithmetic and summation order: the records of step k, output (u_0 of the converged solve), plant step, update of
// x0 / u_{-1} / the first Delta-u bounds and the step blob, and of what these enter -- q of stage 0's inputs (the only entries of q that change with
// a constant reference), the types of stage 0's dynamics rows and the first Delta-u rows (the only bounds that move).  It loads NOTHING from memory
// where the plant is the model's (the LDS copy): the disturbance wn, the scaling Er and type ct of row r, rho (in inf) were requested early in
// the check; S.uo was published by the check's block reduction.  Called in line, forward declared for the check above.
// Returns LATW_CARRIED: the caller starts step k + 1's solve from its owner registers, iflag[6] = k + 1, with the new -c q of stage 0's inputs
// in Tc and the new bound of stage 0's dynamics rows in Cc at their owners' slots (both vectors are rewritten by the iteration before it reads
// them).  Returns LATW_SOLVED: a type changed -- the step's transition is done, its begin (refactorization) is not: iflag[7] = -1 tells the kernel
// to run begin for step iflag[6] = k + 1.
template <int NXT, int NUT, int NST>
__device__ __forceinline__ int latw_carry(const RunKArgs &KA, Smem &S, int b, int k, int iter, double cc, double wn, double Er, int ct, int r, mpcqp_info inf) {
    BTICK(4)
#ifdef MPCQP_RUN_TIMING
    const unsigned long long tw0_ = wall_clock64();
#endif
    constexpr int NB = 16, VS = LAT_VS(NST);
    const Lay &L = KA.L; const Ptrs &P = KA.P; const RunArgs &R = KA.R;
    const int nx = NXT ? NXT : L.nx, nu = NUT ? NUT : L.nu;
    const int tid = threadIdx.x, k1 = k + 1;
    const unsigned long long tstep = wall_clock64();      // (the end of step k: asked for here, stored with the record below)
    double *step = P.step + (size_t)b * L.step_sz;
    const size_t kb = (size_t)k1 * R.batch + b;
    // ---- output (solved: the first input), plant step, update -- mpcqp_kernels.h run_instance, ny = 0
    const double *un = S.uo, *xt = S.x0s;
    double xn = 0.0;
    if (tid < nx) {
        double acc = 0.0;
        if (!R.Ap && !R.Bp) {
            // (the model's own matrices: LDS, read THROUGH LDS POINTERS.  Left generic, the compiler joins the input part of this branch with the other
            //  one's and reads Bd with FLAT loads; a FLAT load is waited for with vmcnt(0), and that wait stood right behind the solved tail's ten
            //  global stores: the plant product paid their whole acknowledgement.)
            ldsd *Ad = as_lds(S.hot + L.oAd), *Bd = as_lds(S.hot + L.oBd), *xl = as_lds(xt), *ul = as_lds(un);
            for (int j = 0; j < nx; ++j) acc += Ad[tid * nx + j] * xl[j];
            for (int j = 0; j < nu; ++j) acc += Bd[tid * nu + j] * ul[j];
        } else {
            const double *Ap = R.Ap ? R.Ap + (size_t)b * nx * nx : S.hot + L.oAd;
            const double *Bp = R.Bp ? R.Bp + (size_t)b * nx * nu : S.hot + L.oBd;
            for (int j = 0; j < nx; ++j) acc += Ap[tid * nx + j] * xt[j];
            for (int j = 0; j < nu; ++j) acc += Bp[tid * nu + j] * un[j];
        }
        xn = acc + wn;
        R.x_traj[kb * nx + tid] = xt[tid];
    }
    if (tid < nu) R.u_traj[kb * nu + tid] = un[tid];
    // has a re-typed row changed its type?  An OR has no order: the lanes that see a change store 1 into a word of Smem::red that thread 0 cleared
    // two barriers earlier, everybody reads it behind one more (__syncthreads_or is three barriers and three loads of the block's dimensions from memory)
    typedef __attribute__((address_space(3))) int ldsi;
    ldsi *chg = (ldsi *)(size_t)(unsigned)(unsigned long long)(S.red + LATW_FLAG);      // (as_lds for an int)
    if (tid == 0) *chg = 0;
    __syncthreads();
    BTICK(6)
    if (tid < nx) { S.x0s[tid] = xn; step[tid] = xn; }
    if (tid < nu) { const double u = un[tid]; S.um1s[tid] = u; step[nx + tid] = u; S.du0[tid] = S.hot[L.oDumin + tid] + u; S.du0[nu + tid] = S.hot[L.oDumax + tid] + u; }
    __syncthreads();
    // ---- begin_body for what moved: q of stage 0's inputs (memory, and -c q for their owners), stage 0's dynamics-row bounds for theirs, types
    const Ctx c{L, S.hot, S.hot + L.hot_sz};              // (hot_lds > hot_sz: the caller's fast path)
    double *Tc = S.T + NB, *Cc = Tc + VS;                  // (owner slot of stage 0's slot a: a)
    if (tid < nu) { const double qj = q_input(c, 0, tid, S.um1s, S.hot + L.ouref); S.Qv[L.n_x + tid] = qj; Tc[nx + tid] = -cc * qj; }
    if (tid < nx) Cc[tid] = -S.x0s[tid];
    if (r >= 0) { double lo, hi; row_bounds(c, S.x0s, S.du0, affine_ptr(L, P, b), r, lo, hi); if (row_type(Er, lo, hi) != ct) *chg = 1; }
    __syncthreads();
    const int changed = *chg;
    if (tid == 0) {
        R.status_traj[(size_t)k * R.batch + b] = MPCQP_SOLVED;      // (Smem::iflag[4]: the check's, a moment ago)
        R.iter_traj[(size_t)k * R.batch + b] = iter;
        if (k < TS_STEPS) P.tstamp[(size_t)TS_STRIDE * b + 2 + k] = tstep;
        S.iflag[6] = k1;
        atomicAdd(&P.stats[8], 1ULL);                      // (mpcqp_dev_carry_stats: steps carried, and of those handed back)
        if (changed) { S.iflag[7] = -1; atomicAdd(&P.stats[9], 1ULL); }      // (the record stays the solved step's)
        else {
            inf.status = MPCQP_UNSOLVED; inf.iter = 0; inf.rho_updates = 0;      // (begin_body's record)
            inf.obj_val = 0.0; inf.pri_res = 0.0; inf.dua_res = 0.0;
            S.iflag[1] = 0; S.iflag[3] = 0;
        }
        P.info[b] = inf;
    }
#ifdef MPCQP_RUN_TIMING
    if (tid == 0) atomicAdd(&P.stats[7], wall_clock64() - tw0_);      // (the loop body's clock: transitions inside the round count there too)
#endif
    return changed ? LATW_SOLVED : LATW_CARRIED;
}
