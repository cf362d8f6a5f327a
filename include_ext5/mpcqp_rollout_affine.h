/*
 * mpcqp_rollout_affine.h -- the taped closed loop and its reverse sweep for a prediction model with an affine term,
 * x_{k+1} = Ad x_k + Bd u_k + d_k (include_ext4/mpcqp_affine.h), in the two state-feedback forms of the loop: one model, and a model schedule.
 * An extension beside the headers of include/, include_ext/ .. include_ext4/, which stay as they are; exported by libmpcqp_hip.so.
 *
 * What has changed about the "not covered" list of include_ext4/mpcqp_affine.h: the OLDER taped rollouts and sweeps answer as that header says
 * (MPCQP_ERR_UNSUPPORTED on a handle that has a term); the calls below are the ones that carry the term.  Still not covered, each refused and
 * never ignored: the two output-feedback tapes with a term (the estimator's model has no offset), raw-vector mode, polishing inside the loop.
 * mpcqp_gains itself still has no K_d: mpcqp_gains_affine below is the call that returns it.
 *
 * The tape keeps the term beside everything else: every entry's step data include it (they always did: the term is step data), and the tape
 * remembers the terms as SLOTS, the way a scheduled tape remembers its models:
 *     slot 0       the term the handle held when the call began -- zeros, written by the call, where it held none
 *     slot e + 1   schedule entry e
 * Tape entry k was solved under slot tau(k):  tau(0) = 0,  tau(k) = 1 + (k - 1) / at->hold  for k >= 1.  With at == NULL there is one slot, the
 * handle's own constant term, and tau(k) = 0 throughout.
 */
#ifndef MPCQP_ROLLOUT_AFFINE_H
#define MPCQP_ROLLOUT_AFFINE_H

#include <stdint.h>

#include "../include/mpcqp_adjoint_bounds.h"
#include "../include/mpcqp_rollout.h"
#include "../include_ext/mpcqp_rollout_tv.h"
#include "../include_ext4/mpcqp_affine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mpcqp_mpc_loop_affine(h, nsteps, io, mt, at) that keeps a tape: the same loop with the same indexing (the solve that follows step k uses
 * entry k / at->hold), one closed-loop launch per step behind a copy of what the handle holds, as mpcqp_rollout / mpcqp_rollout_tv run theirs.
 * mt: a model schedule or NULL; at: a schedule of terms or NULL (the handle's own term throughout, which must exist: MPCQP_ERR_STATE without).
 * After the call the handle holds the last entry used.  The plant is unchanged: x = Ap x + Bp u + w[k], without the offset.
 * Refused before any launch, with nothing changed, in this order: a handle term whose d_rows differs from at->rows: MPCQP_ERR_ARG; every refusal
 * of mpcqp_mpc_loop_affine, with its codes, in its order (io->ny > 0, MPCQP_ERR_UNSUPPORTED, is its last); then every refusal of mpcqp_rollout /
 * mpcqp_rollout_tv, with their codes, in their order. */
int mpcqp_rollout_affine(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt, const mpcqp_affine_traj *at);

/* Device memory the tape takes.  Before mpcqp_setup: MPCQP_ERR_STATE.  model_hold_or_0: hold of the model schedule, 0 without one; d_hold_or_0: hold of the schedule of terms, 0 for
 * at == NULL; rows: 1 or Np.  What the older *_tape_bytes calls report does not change. */
int mpcqp_rollout_affine_tape_bytes(mpcqp_handle *h, int nsteps, int model_hold_or_0, int d_hold_or_0, int rows, int64_t *bytes);

/* The reverse sweep's one more output. */
typedef struct {
    int32_t struct_size, reserved;   /* sizeof(mpcqp_rollout_affine_io); 0 */
    double *d_d_slots;               /* [nslots][batch][rows * nx], host or device, or NULL: slot s gets the sum, over the solved entries k with
                                        tau(k) = s whose factorization held, of -r_y of dynamics row blocks 1 .. Np (mpcqp_adjoint_affine's rule:
                                        rows = Np per row, rows = 1 summed over the stages in ascending order); a slot no entry used is zero */
} mpcqp_rollout_affine_io;

/* mpcqp_rollout_adjoint_bounds (to == NULL) / mpcqp_rollout_adjoint_tv (to != NULL) over the tape of a mpcqp_rollout_affine, with each entry's
 * active set and bounds read under the term that entry was solved with.  to is non-NULL exactly when the tape has a model schedule
 * (MPCQP_ERR_STATE otherwise); mo, bo, ao may be NULL.  Every sum over the steps is formed in the order K-1 .. 0 by one thread: the same bits
 * from call to call.  On a tape that is not one of mpcqp_rollout_affine: MPCQP_ERR_STATE; the four older sweeps answer MPCQP_ERR_STATE on a
 * tape of mpcqp_rollout_affine and name this call. */
int mpcqp_rollout_adjoint_affine(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_adjoint_model_io *mo,
                                 const mpcqp_adjoint_bounds_io *bo, const mpcqp_rollout_tv_io *to, const mpcqp_rollout_affine_io *ao);

/* The term of slot s as the tape remembers it, d [batch][rows * nx] (host or device).  For tests and callers.  s out of range or d NULL:
 * MPCQP_ERR_ARG; not such a tape: MPCQP_ERR_STATE. */
int mpcqp_rollout_affine_get_slot(mpcqp_handle *h, int s, double *d);

/* FOR VERIFICATION ONLY, like mpcqp_rollout_get_tape: the term in the step data of tape entry k, as the sweep reads it, d [batch][rows * nx]
 * (mpcqp_rollout_get_tape returns the step data up to the reference, as it always did).  Synchronises.  k out of range or d NULL: MPCQP_ERR_ARG; not such a tape: MPCQP_ERR_STATE. */
int mpcqp_rollout_affine_get_tape(mpcqp_handle *h, int k, double *d);

/* mpcqp_gains (include/mpcqp_adjoint.h) that also returns K_d = d u_0 / d d, [batch][nu][d_rows * nx] (host or device; any of the five may be NULL):
 * the same factorization and the same nu unit-seed solves, four to a solve where mpcqp_gains does that; row j is what mpcqp_adjoint_affine returns
 * for the seed e_j.  On a handle without a term: MPCQP_ERR_STATE.  mpcqp_gains itself is untouched. */
int mpcqp_gains_affine(mpcqp_handle *h, double *K_x0, double *K_uminus1, double *K_xref, double *K_uref, double *K_d);

#ifdef __cplusplus
}
#endif
#endif
