/*
 * mpcqp_rollout.h -- a closed-loop rollout with a tape, and its derivative in one reverse sweep.  An extension beside mpcqp.h,
 * mpcqp_adjoint.h and mpcqp_adjoint_model.h, whose declarations and structs stay as they are; exported by libmpcqp_hip.so.
 *
 * mpcqp_rollout is mpcqp_mpc_loop that remembers: for every step k = 0 .. nsteps - 1 it keeps the solve whose first input was applied at
 * that step -- the ADMM iterate (x, z, y, unscaled), the step data the solve was made with (x_k, the u_{-1} it was solved with, xref), its
 * status and the applied input u_k -- and the plant (Ap, Bp) where one was given.  The solve for x_K, whose input is never applied, is not
 * on the tape.  mpcqp_rollout_adjoint pushes a loss on the trajectory, given by G_x[k] = dL/dx_k and G_u[k] = dL/du_k, back through the loop:
 *
 *     lam_K = G_x[K];  mu = 0
 *     for k = K-1 .. 0:
 *         g      = G_u[k] + Bp' lam_{k+1} + mu
 *         (d_x0, d_um1, d_xref, d_uref, model gradients) = the adjoint of tape entry k with seed g_u0 = g   (mpcqp_adjoint.h, mpcqp_adjoint_model.h)
 *         lam_k  = G_x[k] + Ap' lam_{k+1} + d_x0
 *         mu     = d_um1
 *         d_uref += d_uref_k;   d_xref[k] = d_xref_k;   model gradients += those of step k
 *         d_Ap   += lam_{k+1} x_k';   d_Bp += lam_{k+1} u_k'
 *     d_uminus1 = mu
 *
 * A step whose solve did not end 'solved' applied u_failure = uref: it gives d_uref += g, lam_k = G_x[k] + Ap' lam_{k+1}, mu = 0 and
 * nothing else.  A step whose regularized factorization broke (status -1) passes lam through the plant alone.  Without Ap, Bp in the
 * forward call the plant was the controller's Ad, Bd: d_Ap, d_Bp are still the plant path alone, to be ADDED to d_Ad, d_Bd by a caller
 * for whom the two are one parameter.
 *
 * The sweep is one kernel launch, one workgroup per instance walking its tape backwards.  Where a step's active set equals the one the
 * regularized KKT matrix was last factored for, the factor in place is used again (the metric follows from the active set, the scaling
 * being fixed): a regulated loop settles on one active set and pays a handful of factorizations instead of nsteps.  Every sum over the
 * steps runs in the order K-1 .. 0 without floating-point atomics: two calls on one tape give the same bits, with and without reuse.
 *
 * The tape is a copy: later mpcqp_solve, mpcqp_update, mpcqp_mpc_step and mpcqp_mpc_loop calls do not touch it.  The model blob and the
 * scaling are read from the handle, so mpcqp_setup*, mpcqp_update_model and mpcqp_update_vectors with l, u (which decodes the boxes of
 * l, u into the model blob) invalidate it.  Like the other adjoint calls the sweep writes
 * nothing of the handle but the adjoint's own buffers: a solve after it is bit-identical to the same solve without it.
 */
#ifndef MPCQP_ROLLOUT_H
#define MPCQP_ROLLOUT_H

#include <stdint.h>

#include "mpcqp_adjoint_model.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Exactly mpcqp_mpc_loop(h, nsteps, io) -- the same arguments, trajectories, pointer rules and handle state afterwards -- and the tape.
 * One closed-loop launch per step with a copy kernel in front of it; with every buffer in device memory the call is stream-ordered.
 * Refusals, before anything is launched or changed: io->ny > 0 (output feedback) MPCQP_ERR_UNSUPPORTED; polishing switched on
 * MPCQP_ERR_UNSUPPORTED and raw-vector mode MPCQP_ERR_STATE, as for the loop; no solve since the last update (the iterate would not belong
 * to the step data of entry 0) MPCQP_ERR_STATE; an xref_traj whose xref_rows differs from the shape of the last upload (the entries of a
 * tape have one shape) MPCQP_ERR_UNSUPPORTED; a tape that cannot be allocated MPCQP_ERR_HIP -- an earlier tape then stays as it is. */
int mpcqp_rollout(mpcqp_handle *h, int nsteps, const mpcqp_loop *io);

/* Device memory a tape of nsteps steps takes, the staging of the sweep's seeds and outputs included. */
int mpcqp_rollout_tape_bytes(mpcqp_handle *h, int nsteps, int64_t *bytes);

/* Free the tape (mpcqp_destroy does it too).  mpcqp_rollout_adjoint is MPCQP_ERR_STATE afterwards. */
int mpcqp_rollout_release(mpcqp_handle *h);

/* Every array is a host or a device pointer; with every given pointer in device memory the call is stream-ordered and returns without
 * waiting.  nsteps, batch and xref_rows are the tape's. */
typedef struct {
    int32_t struct_size;          /* sizeof(mpcqp_rollout_adjoint_io) */
    int32_t no_reuse;             /* 0: reuse the factor across steps with equal active sets; 1: factor at every solved step (same bits) */
    const double *G_x;            /* [nsteps+1][batch][nx] dL/dx_k, or NULL */
    const double *G_u;            /* [nsteps][batch][nu] dL/du_k, or NULL (at least one of the two) */
    /* outputs, any may be NULL */
    double *lam;                  /* [nsteps+1][batch][nx] total dL/dx_k: lam[0] = dL/dx0, lam[k+1] = dL/dw[k] */
    double *d_uminus1;            /* [batch][nu] with respect to the u_{-1} of entry 0 */
    double *d_uref;               /* [batch][nu] */
    double *d_xref;               /* [nsteps][batch][xref_rows * nx]: entry k, with respect to the reference tape entry k was solved with */
    double *d_Ap;                 /* [batch][nx * nx] the plant path alone */
    double *d_Bp;                 /* [batch][nx * nu] */
} mpcqp_rollout_adjoint_io;

/* The reverse sweep over the handle's tape.  mo (or NULL): the seven model gradients of mpcqp_adjoint_model_io summed over the steps,
 * batch_sum as there.  The settings are those of mpcqp_set_adjoint.  Wrong struct_size, or neither G_x nor G_u: MPCQP_ERR_ARG.  Before any
 * rollout, after mpcqp_rollout_release, after mpcqp_setup*, mpcqp_update_model or mpcqp_update_vectors with l, u: MPCQP_ERR_STATE. */
int mpcqp_rollout_adjoint(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_adjoint_model_io *mo);

/* Of the last mpcqp_rollout_adjoint (any may be NULL; host or device; synchronises): n_active, n_weak, status [nsteps][batch] with the
 * meaning of mpcqp_get_adjoint_info per tape entry (status 0: the entry's solve did not end 'solved'), and n_factor [batch], the
 * factorizations of the regularized KKT matrix the sweep made.  Before any sweep of the current tape: all zero. */
int mpcqp_get_rollout_info(mpcqp_handle *h, int32_t *n_active, int32_t *n_weak, int32_t *status, int32_t *n_factor);

/* ---- verification surface ---- */
/* Tape entry k, 0 <= k < nsteps (any pointer may be NULL; host or device; synchronises): x [batch][n], z, y [batch][m] the iterate;
 * step [batch][nx + nu + xref_rows * nx] = (x_k | the u_{-1} the solve was made with | xref); status [batch] its mpcqp_info.status. */
int mpcqp_rollout_get_tape(mpcqp_handle *h, int k, double *x, double *z, double *y, double *step, int32_t *status);

#ifdef __cplusplus
}
#endif
#endif
