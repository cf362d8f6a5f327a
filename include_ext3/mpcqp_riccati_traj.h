/*
 * mpcqp_riccati_traj.h -- batched Riccati DIFFERENCE equations on the device, and the adjoint of their trajectories and gains.  An
 * extension beside the headers of include/, include_ext/ and include_ext2/, which stay as they are; exported by libmpcqp_hip.so.
 *
 * The stepwise companion of include/mpcqp_riccati.h: for t = 0 .. T-1, from a given symmetric X_0 >= 0,
 *
 *     S_t     = R + B_t' X_t B_t
 *     K_t     = S_t^-1 B_t' X_t A_t                         (gain_form 0)
 *     F_t     = S_t^-1 B_t' X_t                             (gain_form 1)
 *     X_{t+1} = sym(A_t' X_t A_t - A_t' X_t B_t K_t + Q)
 *
 * -- the covariance recursion of the Kalman filter of a time-varying system on the dual problem (A_t', C', Qn, Rn; X_0 = P0, L_t = F_t'),
 * and the cost-to-go of a model schedule with the schedule reversed and X_0 = QxN.  A is a trajectory [T][batch][n][n] (A_steps = T) or one
 * matrix per instance [batch][n][n] used at every step (A_steps = 1); the same for B [.][batch][n][m] and B_steps.  Q [batch][n][n] and
 * R [batch][m][m] are constant.  The calls take no handle; device, stream, host or device pointers, stream ordering and the one staging
 * block that is freed before the call returns are those of mpcqp_dare.  One workgroup runs one instance's recursion with X in LDS across
 * all steps.  mpcqp_riccati_settings is reused: gain_form as there, max_iter and tol are ignored.
 *
 * status[b]:  1 done;  -1 a Cholesky pivot of some S_t was not positive;  0 a NaN or an inf appeared.  first_bad[b]: the step t at which
 * the instance ended, -1 if it ran through.  These are outcomes, not errors (mpcqp.h).  An instance whose status is not 1 gets zeros in
 * every output of both calls.
 *
 * 1 <= n <= 32 and 1 <= m <= 32 (MPCQP_ERR_UNSUPPORTED beyond); batch < 1, n < 1, m < 1, T < 1, A_steps or B_steps that is neither T nor 1,
 * a NULL pointer that is not optional, a wrong struct_size or a gain_form that is neither 0 nor 1: MPCQP_ERR_ARG.  Both before anything is
 * launched; mpcqp_last_error explains.
 */
#ifndef MPCQP_RICCATI_TRAJ_H
#define MPCQP_RICCATI_TRAJ_H

#include <stdint.h>

#include "../include/mpcqp_riccati.h"

#ifdef __cplusplus
extern "C" {
#endif

/* s == NULL: the defaults.  Outputs: X_traj [T + 1][batch][n][n] (entry 0 is sym(X0), every entry exactly symmetric), K_traj
 * [T][batch][m][n] (the gain of every step in the form asked for), status [batch], first_bad [batch]; X_traj and status are required,
 * K_traj and first_bad may be NULL. */
int mpcqp_dre(int device, void *stream, int batch, int n, int m, int T, const mpcqp_riccati_settings *s,
              const double *A, int A_steps, const double *B, int B_steps, const double *Q, const double *R, const double *X0,
              double *X_traj, double *K_traj, int32_t *status, int32_t *first_bad);

/* The gradients of sum_t <G_X[t], X_t> + sum_t <G_K[t], gain_t> with respect to A, B, Q, R and X0, at the X_traj and status that mpcqp_dre
 * returned for the same inputs under the same gain_form.  Seeds G_X [T + 1][batch][n][n], G_K [T][batch][m][n]: either may be NULL (zero),
 * not both.  Outputs d_A [A_steps][batch][n][n] and d_B [B_steps][batch][n][m] (per entry for a trajectory, the sum over t for one matrix),
 * d_Q [batch][n][n], d_R [batch][m][m], d_X0 [batch][n][n]: any may be NULL, not all.  d_Q, d_R and d_X0 are the gradients of a SYMMETRIC
 * perturbation and are themselves exactly symmetric (the convention of mpcqp_adjoint_model.h).  Every sum over t runs in one fixed order:
 * the same bits from call to call.  Q and X0 do not enter the derivative and may be NULL; status == NULL: every instance counts as done. */
int mpcqp_dre_adjoint(int device, void *stream, int batch, int n, int m, int T, const mpcqp_riccati_settings *s,
                      const double *A, int A_steps, const double *B, int B_steps, const double *Q, const double *R, const double *X0,
                      const double *X_traj, const int32_t *status, const double *G_X, const double *G_K,
                      double *d_A, double *d_B, double *d_Q, double *d_R, double *d_X0);

#ifdef __cplusplus
}
#endif
#endif
