/*
 * mpcqp_rollout_tv.h -- a closed-loop rollout under a model schedule with a tape, and its derivative in one reverse sweep.  An extension
 * beside the headers of include/, whose declarations and structs stay as they are; exported by libmpcqp_hip.so.
 *
 * mpcqp_rollout_tv is mpcqp_mpc_loop_tv (include/mpcqp_model.h) that remembers.  That loop is, per schedule entry e,
 * mpcqp_update_model(entry e) followed by the loop for min(hold, rest) steps; update_model keeps the iterate, so the input applied at a
 * boundary step is still the one the last solve produced under the previous model.  With nseg = ceil(nsteps / hold) the tape holds
 * nseg + 1 model slots -- slot 0: the model the handle holds when the call begins; slot e + 1: schedule entry e -- each with the model
 * blob and the scaling D, E, c it was equilibrated to, and:
 *
 *     solve slot   tape entry k (the solve whose first input is applied at step k) was made under slot sigma(k) = 0 for k = 0 and
 *                  1 + (k - 1) / hold for k > 0; it is differentiated with that slot's model and scaling.
 *     plant slot   without io->Ap the plant at step k is the model in force, slot 1 + k / hold: not sigma(k) at a boundary step.
 *     last entry   its solve path covers the tape entries k > (nseg - 1) hold only: with hold = 1 it is exactly zero (its one solve is the
 *                  one for x_K, which is not on a tape).  Its plant path is not.
 *
 * The recursion is that of include/mpcqp_rollout.h with these substitutions.  The factor in place is used again only where both the active
 * set and the slot equal those of the entry behind it (the metric s = delta / D^2 follows the slot).  Every sum runs in the order
 * K-1 .. 0 without floating-point atomics: two calls on one tape give the same bits, with and without reuse.
 *
 * The tape carries its models: unlike the tape of mpcqp_rollout the sweep reads nothing of the handle's model blob or scaling.  It is
 * invalidated all the same by mpcqp_setup*, mpcqp_update_model and mpcqp_update_vectors with l, u, as that one is.
 */
#ifndef MPCQP_ROLLOUT_TV_H
#define MPCQP_ROLLOUT_TV_H

#include <stdint.h>

#include "../include/mpcqp_model.h"
#include "../include/mpcqp_rollout.h"
#include "../include/mpcqp_adjoint_bounds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Exactly mpcqp_mpc_loop_tv(h, nsteps, io, mt) -- the same trajectories, statuses, iteration counts and handle state afterwards, bit for
 * bit -- and the tape.  One closed-loop launch per step; at a boundary step k = e hold: the tape's copy of entry k, mpcqp_update_model(entry e),
 * a device copy of the handle's model blob, D, E, c into slot e + 1, then the step.  Slot 0 is copied before anything else.  With every
 * buffer in device memory the call is stream-ordered.  Refusals, before anything is launched or changed: everything mpcqp_rollout refuses,
 * everything mpcqp_mpc_loop_tv refuses (io->ny > 0: MPCQP_ERR_UNSUPPORTED), and mt == NULL: MPCQP_ERR_ARG (that is mpcqp_rollout). */
int mpcqp_rollout_tv(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt);

/* Device memory the tape of nsteps steps under a schedule with this hold takes, slots and staging included. */
int mpcqp_rollout_tv_tape_bytes(mpcqp_handle *h, int nsteps, int hold, int64_t *bytes);

/* The outputs a schedule adds to the sweep; any may be NULL, host or device.  nseg = ceil(nsteps / hold) of the tape. */
typedef struct {
    int32_t struct_size;          /* sizeof(mpcqp_rollout_tv_io) */
    int32_t reserved;
    double *d_Ad_slots;           /* [nseg+1][batch][nx * nx] the solve path, summed over the tape entries k with sigma(k) = s */
    double *d_Bd_slots;           /* [nseg+1][batch][nx * nu] */
    double *d_Ap_entries;         /* [nseg][batch][nx * nx] the plant path lam_{k+1} x_k', summed over the steps with k / hold = e */
    double *d_Bp_entries;         /* [nseg][batch][nx * nu] lam_{k+1} u_k' */
} mpcqp_rollout_tv_io;

/* The reverse sweep over a scheduled tape, one kernel launch.  io: the seeds and lam, d_uminus1, d_uref, d_xref as for mpcqp_rollout_adjoint;
 * mo (or NULL): d_Qx, d_QxN, d_Qu, d_QDu, d_eps_feas summed over all steps (the weights do not change along a schedule); bo (or NULL): the
 * six bound gradients; to (or NULL): the per-slot and per-entry model gradients.  io->d_Ap, io->d_Bp, mo->d_Ad, mo->d_Bd: MPCQP_ERR_ARG (the
 * outputs of `to` replace them).  batch_sum applies to mo and bo.  mpcqp_get_rollout_info serves this sweep too.
 * On the tape of mpcqp_rollout or mpcqp_rollout_est: MPCQP_ERR_STATE (use mpcqp_rollout_adjoint); likewise mpcqp_rollout_adjoint, _est and
 * _bounds on a scheduled tape (use mpcqp_rollout_adjoint_tv). */
int mpcqp_rollout_adjoint_tv(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_adjoint_model_io *mo,
                             const mpcqp_adjoint_bounds_io *bo, const mpcqp_rollout_tv_io *to);

/* ---- verification surface ---- */
/* Slot s, 0 <= s <= nseg, as the sweep reads it (any pointer may be NULL; host or device; synchronises): model [batch][3 nx nx + nx nu +
 * 2 nu nu + 2 nx + 5 nu + 1] the model blob = (Ad | Bd | xmin | xmax | umin | umax | Dumin | Dumax | uref | eps_feas | Qx | QxN | Qu | QDu),
 * D [batch][n], E [batch][m], c [batch].  Entries of the tape itself: mpcqp_rollout_get_tape. */
int mpcqp_rollout_tv_get_slot(mpcqp_handle *h, int s, double *model, double *D, double *E, double *c);

#ifdef __cplusplus
}
#endif
#endif
