/*
 * mpcqp_riccati.h -- batched discrete algebraic Riccati equations on the device, and the adjoint of their solution and gain.  An
 * extension beside the other headers, which stay as they are; exported by libmpcqp_hip.so.
 *
 *     X = A'XA - A'XB (R + B'XB)^-1 B'XA + Q            A [n][n], B [n][m], Q [n][n] symmetric >= 0, R [m][m] symmetric > 0
 *
 * is what a terminal weight tied to the model (the LQR cost-to-go of (Ad, Bd, Qx, Qu)) and a stationary Kalman gain (the dual problem
 * (A', C', Qn, Rn)) are made of.  The calls take no handle: a device, a stream (a hipStream_t passed as void *, NULL = the null stream) and
 * plain [batch][...] row-major float64 arrays, each a host or a device pointer.  With every given pointer in device memory a call is
 * stream-ordered and returns without waiting; host pointers go through one staging block that is freed before the call returns.  One
 * workgroup solves one instance entirely in LDS:
 *
 *   forward   structure-preserving doubling:  G_0 = B R^-1 B', H_0 = Q, A_0 = A;  W = I + G_k H_k,
 *                 A_{k+1} = A_k W^-1 A_k,   G_{k+1} = sym(G_k + A_k W^-1 G_k A_k'),   H_{k+1} = sym(H_k + A_k' H_k W^-1 A_k)  -> X
 *             (W by LU with partial pivoting, every product on the matrix cores), stopped by |H_{k+1} - H_k|_max <= tol max(1, |H_{k+1}|_max).
 *   adjoint   of the loss <G_X, X> + <G_K, K>: one discrete Lyapunov equation Lambda = Acl Lambda Acl' + Xb, Acl = A - B K, by Smith doubling
 *             under the same stopping rule, and a handful of products around it.
 *
 * status[b]:  1 converged;  0 no convergence within max_iter (the pair is not stabilizable, not detectable on the unit circle, or the
 * iterate overflowed: a NaN or inf anywhere counts as not converged and ends the instance at once);  -1 R or R + B'XB is not positive
 * definite (a Cholesky pivot <= 0).  These are outcomes, not errors (mpcqp.h).  An instance whose status is not 1 gets zeros in X, K and
 * res, and zeros in every output of the adjoint.  iters[b]: the doubling steps taken.  For a converged instance
 *     res[b] = |X - (A'XA - A'XB (R + B'XB)^-1 B'XA + Q)|_max / max(1, |X|_max)        from the given A, B, Q, R.
 *
 * 1 <= n <= 32 and 1 <= m <= 32 (MPCQP_ERR_UNSUPPORTED beyond); batch < 1, n < 1, m < 1, a NULL input or output that is not optional, a
 * wrong struct_size, max_iter < 1 or a tol that is not >= 0: MPCQP_ERR_ARG.  mpcqp_last_error explains.
 */
#ifndef MPCQP_RICCATI_H
#define MPCQP_RICCATI_H

#include <stdint.h>

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t struct_size;   /* sizeof(mpcqp_riccati_settings) */
    int32_t max_iter;      /* doubling steps, default 50 */
    int32_t gain_form;     /* 0: K = (R+B'XB)^-1 B'X A  [m][n]  (LQR / predictor form)
                              1: F = (R+B'XB)^-1 B'X    [m][n]  (filter form: L = F' on the dual problem) */
    int32_t reserved;
    double  tol;           /* stop when |H_{k+1}-H_k|_max <= tol * max(1, |H_{k+1}|_max); default 1e-15 */
} mpcqp_riccati_settings;

void mpcqp_riccati_default_settings(mpcqp_riccati_settings *s);

/* s == NULL: the defaults.  Outputs: X [batch][n][n], K [batch][m][n] (the gain in the form asked for), status [batch], iters [batch],
 * res [batch]; X and status are required, K, iters and res may be NULL. */
int mpcqp_dare(int device, void *stream, int batch, int n, int m, const mpcqp_riccati_settings *s,
               const double *A, const double *B, const double *Q, const double *R,
               double *X, double *K, int32_t *status, int32_t *iters, double *res);

/* The gradients of <G_X, X> + <G_K, K> with respect to A, B, Q, R at the solution X, K, status of mpcqp_dare under the same settings (K in
 * the same gain_form).  Seeds G_X [batch][n][n], G_K [batch][m][n]: either may be NULL (zero), not both.  Outputs d_A [batch][n][n], d_B
 * [batch][n][m], d_Q [batch][n][n], d_R [batch][m][m] and iters [batch] (the Smith doubling steps): any may be NULL, not all four
 * gradients.  d_Q and d_R are the gradients of a SYMMETRIC perturbation, dL = <d_Q, dQ> for symmetric dQ, and are themselves exactly
 * symmetric (the convention of mpcqp_adjoint_model.h).  status == NULL: every instance counts as converged.  An instance whose status is
 * not 1, or whose Lyapunov iteration does not converge (it does wherever mpcqp_dare did), gets zeros. */
int mpcqp_dare_adjoint(int device, void *stream, int batch, int n, int m, const mpcqp_riccati_settings *s,
                       const double *A, const double *B, const double *Q, const double *R,
                       const double *X, const double *K, const int32_t *status,
                       const double *G_X, const double *G_K,
                       double *d_A, double *d_B, double *d_Q, double *d_R, int32_t *iters);

#ifdef __cplusplus
}
#endif
#endif
