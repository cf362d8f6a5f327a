/*
 * mpcqp_rollout_est.h -- the taped rollout of the OUTPUT-FEEDBACK loop and its derivative through the estimator.  An extension beside
 * mpcqp_rollout.h, whose declarations and structs stay as they are (mpcqp_rollout itself keeps refusing ny > 0); exported by libmpcqp_hip.so.
 *
 * The forward loop is mpcqp_mpc_loop with io->ny > 0 (mpcqp.h): x the plant state, xh = xhat[k|k-1] the estimate the controller sees, the
 * estimator's model the controller's Ad, Bd, no D term:
 *
 *     y_k      = C x_k + v_k
 *     u_k      = first input of the solve made for (xh_k, u_{k-1}, xref), or uref where that solve is not 'solved'
 *     x_{k+1}  = Ap x_k + Bp u_k + w_k
 *     xh_{k+1} = Ad (xh_k + L (y_k - C xh_k)) + Bd u_k
 *
 * A loss is given by four seeds, G_x[k] = dL/dx_k and G_xh[k] = dL/dxh_k (k = 0 .. K), G_u[k] = dL/du_k and G_y[k] = dL/dy_k (k = 0 .. K-1),
 * any of them absent but not all.  The sweep is the one of mpcqp_rollout.h with the estimator in the chain:
 *
 *     lam_K = G_x[K];  eta_K = G_xh[K];  mu = 0
 *     for k = K-1 .. 0:
 *         g    = G_u[k] + Bp' lam_{k+1} + Bd' eta_{k+1} + mu
 *         s    = Ad' eta_{k+1}                 (the gradient at xhat[k|k])
 *         t    = L' s
 *         r    = G_y[k] + t                    (the gradient at y_k)
 *         lam_k = G_x[k]  + Ap' lam_{k+1} + C' r
 *         eta_k = G_xh[k] + s - C' t  (+ d_x0(g) of tape entry k, if it is 'solved')
 *         solved:        mu = d_um1(g);  d_uref += d_uref(g);  d_xref[k] = d_xref(g);  model gradients += those of entry k
 *         not solved:    mu = 0;  d_uref += g
 *         broken factor: mu = 0
 *         d_L  += s (y_k - C xh_k)'
 *         d_C  += r x_k' - t xh_k'
 *         d_v[k] = r
 *         d_Ap += lam_{k+1} x_k';   d_Bp += lam_{k+1} u_k'                         (the plant path alone)
 *         d_Ae += eta_{k+1} (xh_k + L (y_k - C xh_k))';   d_Be += eta_{k+1} u_k'   (the estimator path alone)
 *     d_uminus1 = mu;  lam_0 = dL/dx_0 (the true plant state);  eta_0 = dL/dxh_0;  lam[k+1] = dL/dw[k]
 *
 * d_x0, d_um1, d_uref, d_xref and the model gradients are the per-entry adjoint of mpcqp_rollout.h's sweep, seeded with g on the u_0 block.
 * A caller for whom Ad is one parameter adds d_Ae (and d_Ap, where the plant is the model) to d_Ad; the same holds for B -- the convention
 * mpcqp_rollout.h states for d_Ap, d_Bp.  One kernel launch, one workgroup per instance, no floating-point atomics, every sum in the order
 * K-1 .. 0: two sweeps of one tape give the same bits, with and without factor reuse.
 *
 * mpcqp_get_rollout_info, mpcqp_rollout_release, mpcqp_rollout_get_tape and the invalidation rules of mpcqp_rollout.h apply unchanged.
 */
#ifndef MPCQP_ROLLOUT_EST_H
#define MPCQP_ROLLOUT_EST_H

#include <stdint.h>

#include "mpcqp_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Exactly mpcqp_mpc_loop(h, nsteps, io) with io->ny > 0 -- the same trajectories, pointer rules (host or device) and handle state
 * afterwards -- and the tape: beside what mpcqp_rollout keeps (the entry's x0 is the estimate xh_k), the plant state x_k and the
 * measurement y_k of every step and copies of C, L and, where given, Ap, Bp.  A host x_true is copied to the device once and back once.
 * io->ny == 0: MPCQP_ERR_ARG.  The other refusals are those of mpcqp_rollout (and of the loop: C, Lgain or x_true missing MPCQP_ERR_ARG),
 * before anything is launched or changed; a tape that cannot be allocated leaves an earlier tape as it is. */
int mpcqp_rollout_est(mpcqp_handle *h, int nsteps, const mpcqp_loop *io);

/* Device memory a tape of nsteps steps with ny outputs takes, staging included.  (mpcqp_rollout_tape_bytes stays the state-feedback tape's.) */
int mpcqp_rollout_est_tape_bytes(mpcqp_handle *h, int nsteps, int ny, int64_t *bytes);

/* The estimator's half of the sweep's seeds and outputs.  Every array is a host or a device pointer, any may be NULL. */
typedef struct {
    int32_t struct_size;          /* sizeof(mpcqp_rollout_est_io) */
    const double *G_xhat;         /* [nsteps+1][batch][nx] dL/dxh_k, or NULL */
    const double *G_y;            /* [nsteps][batch][ny] dL/dy_k, or NULL */
    double *eta;                  /* [nsteps+1][batch][nx] total dL/dxh_k: eta[0] = dL/dxh_0 */
    double *d_C;                  /* [batch][ny * nx] */
    double *d_L;                  /* [batch][nx * ny] */
    double *d_v;                  /* [nsteps][batch][ny] */
    double *d_Ae;                 /* [batch][nx * nx] the estimator path alone */
    double *d_Be;                 /* [batch][nx * nu] */
} mpcqp_rollout_est_io;

/* The reverse sweep over a tape made by mpcqp_rollout_est.  io, mo as for mpcqp_rollout_adjoint; eo may be NULL.  MPCQP_ERR_ARG unless at
 * least one of io->G_x, io->G_u, eo->G_xhat, eo->G_y is given, and for a wrong struct_size.  On a tape made by mpcqp_rollout (no
 * estimator): MPCQP_ERR_STATE.  mpcqp_rollout_adjoint on an estimator tape is this sweep with eo == NULL. */
int mpcqp_rollout_adjoint_est(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_rollout_est_io *eo, const mpcqp_adjoint_model_io *mo);

/* ---- verification surface ---- */
/* Of tape entry k, 0 <= k < nsteps (either may be NULL; host or device; synchronises): x_plant [batch][nx] the plant state x_k, y_meas
 * [batch][ny] the measurement y_k.  mpcqp_rollout_get_tape gives the rest; its step data begin with the estimate xh_k. */
int mpcqp_rollout_get_tape_est(mpcqp_handle *h, int k, double *x_plant, double *y_meas);

#ifdef __cplusplus
}
#endif
#endif
