/*
 * mpcqp_rollout_tv_est.h -- the OUTPUT-FEEDBACK loop under a model schedule: the loop, a tape of it, and its derivative in one reverse sweep.
 * An extension beside the headers of include/ and include_ext/, whose declarations and structs stay as they are (mpcqp_mpc_loop_tv and
 * mpcqp_rollout_tv keep refusing io->ny > 0); exported by libmpcqp_hip.so.
 *
 * With hold and nseg = ceil(nsteps / hold) as in include_ext/mpcqp_rollout_tv.h: e(k) = k / hold is the schedule entry in force at step k,
 * pi(k) = 1 + e(k) its slot, sigma(k) = 0 for k = 0 and 1 + (k - 1) / hold beyond the slot the solve of tape entry k was made under, and L_e the
 * observer gain of entry e (the one constant io->Lgain where no gain schedule is given).  Forward, per step k (at k = e hold the input of the
 * last solve is kept, THEN entry e replaces Ad / Bd: mpcqp_mpc_loop_tv's order):
 *
 *     y_k      = C x_k + v_k
 *     u_k      = first input of the solve made under slot sigma(k) for (xh_k, u_{k-1}, xref), or uref where it is not 'solved'
 *     x_{k+1}  = Ap x_k + Bp u_k + w_k                                  (Ap, Bp given, or Ad, Bd of slot pi(k))
 *     xh_{k+1} = Ad_pi(k) (xh_k + L_e(k) (y_k - C xh_k)) + Bd_pi(k) u_k
 *
 * Reverse: the recursion of include/mpcqp_rollout_est.h with Ad, Bd -> those of slot pi(k) in the estimator terms, L -> L_e(k), and the
 * per-entry solve differentiated under slot sigma(k) with that slot's D, E, c (include_ext/mpcqp_rollout_tv.h).  The sums that were per tape
 * are per slot or per entry:
 *
 *     d_Ad_slots[sigma(k)] += d_Ad of entry k            d_Bd_slots[sigma(k)] += d_Bd of entry k
 *     d_Ap_entries[e(k)]   += lam_{k+1} x_k'              d_Bp_entries[e(k)]   += lam_{k+1} u_k'
 *     d_Ae_entries[e(k)]   += eta_{k+1} (xh_k + L_e(k) inn_k)'                  d_Be_entries[e(k)] += eta_{k+1} u_k'
 *     d_L_entries[e(k)]    += s_k inn_k'                  (s_k = Ad_pi(k)' eta_{k+1},  inn_k = y_k - C xh_k)
 *
 * d_C, d_v, eta, lam, d_uminus1, d_uref, d_xref, the five weight gradients and the six bound gradients are as they were.  The factor in place
 * is used again only where the active set and the slot are those of the entry behind it; every sum runs in the order K-1 .. 0 by the thread
 * that owns it, without atomics: two sweeps of one tape give the same bits, with reuse on or off.  For a caller with one Ad per entry the
 * gradient of entry e is d_Ad_slots[e + 1] + d_Ae_entries[e], plus d_Ap_entries[e] where the plant followed the schedule.
 */
#ifndef MPCQP_ROLLOUT_TV_EST_H
#define MPCQP_ROLLOUT_TV_EST_H

#include <stdint.h>

#include "../include/mpcqp_model.h"
#include "../include/mpcqp_rollout.h"
#include "../include/mpcqp_rollout_est.h"
#include "../include/mpcqp_adjoint_bounds.h"
#include "../include_ext/mpcqp_rollout_tv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A schedule of observer gains beside mpcqp_model_traj, with its hold: entry e is in force during steps e hold .. e hold + hold - 1. */
typedef struct {
    int32_t struct_size;          /* sizeof(mpcqp_est_traj) */
    int32_t nentries;             /* >= ceil(nsteps / hold) */
    const double *Lgain_traj;     /* [nentries][batch][nx * ny], host or device; or NULL: io->Lgain holds for every entry */
} mpcqp_est_traj;

/* mpcqp_mpc_loop_tv with io->ny > 0: per schedule entry e, mpcqp_update_model(entry e) and the output-feedback loop for min(hold, rest)
 * steps with the gain of entry e.  et may be NULL (io->Lgain throughout).  Refusals, before anything is launched or changed: everything
 * mpcqp_mpc_loop_tv refuses except the estimator, io->ny == 0 or mt == NULL: MPCQP_ERR_ARG, et->nentries < ceil(nsteps / hold) or a wrong
 * struct_size: MPCQP_ERR_ARG. */
int mpcqp_mpc_loop_tv_est(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt, const mpcqp_est_traj *et);

/* Exactly mpcqp_mpc_loop_tv_est(h, nsteps, io, mt, et) -- the same trajectories, statuses, iteration counts and handle state afterwards,
 * bit for bit -- and the tape: what mpcqp_rollout_tv keeps (nseg + 1 slots with model blob, D, E, c), what mpcqp_rollout_est keeps (x_k, y_k,
 * C and, where given, Ap, Bp) and the gain of every entry.  One closed-loop launch per step; at a boundary step k = e hold: the tape's copy
 * of entry k, mpcqp_update_model(entry e), the slot copy, then the step with the entry's gain.  Refusals, before anything is launched or
 * changed: everything mpcqp_rollout_tv and mpcqp_rollout_est refuse (but for the estimator and the schedule themselves), and those of
 * mpcqp_mpc_loop_tv_est. */
int mpcqp_rollout_tv_est(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt, const mpcqp_est_traj *et);

/* Device memory the tape of nsteps steps under a schedule with this hold and ny outputs takes, slots, gains and staging included. */
int mpcqp_rollout_tv_est_tape_bytes(mpcqp_handle *h, int nsteps, int hold, int ny, int64_t *bytes);

/* The outputs schedule and estimator add together; any may be NULL, host or device.  nseg = ceil(nsteps / hold) of the tape. */
typedef struct {
    int32_t struct_size;          /* sizeof(mpcqp_rollout_tv_est_io) */
    int32_t reserved;
    double *d_Ae_entries;         /* [nseg][batch][nx * nx] the estimator path eta_{k+1} xhat[k|k]', summed over the steps with k / hold = e */
    double *d_Be_entries;         /* [nseg][batch][nx * nu] eta_{k+1} u_k' */
    double *d_L_entries;          /* [nseg][batch][nx * ny] s_k inn_k' */
} mpcqp_rollout_tv_est_io;

/* The reverse sweep over a tape of mpcqp_rollout_tv_est, one kernel launch.  io, mo, bo, to as for mpcqp_rollout_adjoint_tv (with its refusals);
 * eo (or NULL): the estimator's seeds G_xhat, G_y and eta, d_C, d_v as for mpcqp_rollout_adjoint_est -- eo->d_L, eo->d_Ae, eo->d_Be:
 * MPCQP_ERR_ARG (the outputs of `xo` replace them); xo (or NULL): the per-entry estimator gradients.  At least one of the four seeds.
 * On any other tape: MPCQP_ERR_STATE; likewise mpcqp_rollout_adjoint, _est, _bounds and _tv on this tape. */
int mpcqp_rollout_adjoint_tv_est(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_rollout_est_io *eo, const mpcqp_adjoint_model_io *mo,
                                 const mpcqp_adjoint_bounds_io *bo, const mpcqp_rollout_tv_io *to, const mpcqp_rollout_tv_est_io *xo);

/* ---- verification surface ---- */
/* The gain of schedule entry e, 0 <= e < nseg, as the sweep reads it: L [batch][nx * ny] (host or device; synchronises).  Slots:
 * mpcqp_rollout_tv_get_slot; entries of the tape: mpcqp_rollout_get_tape and mpcqp_rollout_get_tape_est. */
int mpcqp_rollout_tv_est_get_gain(mpcqp_handle *h, int e, double *L);

#ifdef __cplusplus
}
#endif
#endif
