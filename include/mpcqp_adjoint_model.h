/*
 * mpcqp_adjoint_model.h -- the matrix half of the adjoint derivatives (what OSQP offers as adjoint_derivative_get_mat), chained into the
 * controller's model Ad, Bd and weights Qx, QxN, Qu, QDu, eps_feas.  An extension beside mpcqp_adjoint.h, whose declarations and structs
 * stay as they are; exported by libmpcqp_hip.so.
 *
 * In the notation of mpcqp_adjoint.h ([P, A_a'; A_a, 0] [r_w; r_y] = [g; 0] on the active rows), a perturbation of the problem data moves
 * the loss by
 *     dL = -r_w' (dP w* + dq + dA' y*) + r_y' (db - dA w*),
 * so beside dL/dq = -r_w and dL/db = r_y
 *     dL/dP = -1/2 (r_w w*' + w* r_w'),     dL/dA = -(y* r_w' + r_y w*')     (non-zero on active rows only).
 * Only the dynamics rows  -x_{k+1} + Ad x_k + Bd u_{min(k, Nc-1)} = 0  of A carry the model; they are equalities, always active.  P and q
 * carry the weights as pyMPC builds them (mpc.py:482-531, 411-452): blkdiag(Qx .. Qx, QxN); iU_k Qu on the input blocks (iU_k = 1, and
 * Np - Nc + 1 on the held last input) plus the tridiagonal iDu (x) QDu; eps_feas I on the slack variables; q_X[k] = -Q_k xref_k,
 * q_U[k] = -iU_k Qu uref, q_U[0] += -QDu u_{-1}.  With X_k, U_k (RX_k, RU_k) the blocks of w* (r_w), Y_{k+1}, RY_{k+1} the blocks of y*, r_y
 * on the dynamics rows of stage k + 1, u(k) = min(k, Nc - 1) and sym M = (M + M') / 2:
 *     d_Ad  = -sum_{k<Np} ( Y_{k+1} RX_k' + RY_{k+1} X_k' )                      [nx][nx]
 *     d_Bd  = -sum_{k<Np} ( Y_{k+1} RU_{u(k)}' + RY_{k+1} U_{u(k)}' )             [nx][nu]
 *     d_Qx  = -sym sum_{k<Np} RX_k (X_k - xref_k)'                                [nx][nx]
 *     d_QxN = -sym RX_Np (X_Np - xref_Np)'                                        [nx][nx]
 *     d_Qu  = -sym sum_{k<Nc} iU_k RU_k (U_k - uref)'                             [nu][nu]
 *     d_QDu = -sym sum_{k<Nc} (RU_k - RU_{k-1}) (U_k - U_{k-1})'                  [nu][nu]    RU_{-1} = 0, U_{-1} = u_{-1} (the one the solve
 *                                                                                  was made with, also after mpcqp_mpc_step has stored the next)
 *     d_eps_feas = -sum_k REPS_k . EPS_k                                          scalar; 0 without slack variables (soft_constraints = 0)
 * The weights are symmetric (the solver reads the upper triangle of P): each weight gradient is the derivative with respect to a
 * SYMMETRIC perturbation, dL = <d_Q, dQ> for symmetric dQ, and is itself exactly symmetric.  w*, y* are the handle's ADMM iterate, the one
 * the active set is read from.  The handle always carries every cost term: a weight the caller switched off by uploading zeros still gets
 * the gradient of the term it would add.
 */
#ifndef MPCQP_ADJOINT_MODEL_H
#define MPCQP_ADJOINT_MODEL_H

#include <stdint.h>

#include "mpcqp_adjoint.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every array is [batch][...] row-major as in mpcqp_model (batch_sum = 1: [1][...], the sum over the batch), a host or a device pointer;
 * any may be NULL. */
typedef struct {
    int32_t struct_size;          /* sizeof(mpcqp_adjoint_model_io) */
    int32_t batch_sum;            /* 0: one gradient per instance; 1: their sum over the batch (one model shared by many states), formed on the
                                     device in a fixed order without floating-point atomics: two calls on the same state give the same bits */
    double *d_Ad;                 /* [batch][nx][nx] */
    double *d_Bd;                 /* [batch][nx][nu] */
    double *d_Qx;                 /* [batch][nx][nx] */
    double *d_QxN;                /* [batch][nx][nx] */
    double *d_Qu;                 /* [batch][nu][nu] */
    double *d_QDu;                /* [batch][nu][nu] */
    double *d_eps_feas;           /* [batch] */
} mpcqp_adjoint_model_io;

/* Everything mpcqp_adjoint(h, io) does -- every output pointer of io may be NULL here as long as one output of io or mo is asked for --
 * and the model gradients of the same seed from the same single factorization.  mo == NULL: exactly mpcqp_adjoint.  With every given
 * pointer in device memory the call is stream-ordered and returns without waiting.  Wrong struct_size, or nothing asked for:
 * MPCQP_ERR_ARG.  The MPCQP_ERR_STATE cases of mpcqp_adjoint carry over; in raw-vector mode any output of mo is MPCQP_ERR_STATE, as d_x0
 * is.  An instance whose adjoint status (mpcqp_get_adjoint_info, which reports on this call as on the others) is 0 or -1 gets zeros, and
 * adds zeros to a batch sum.  Like the other adjoint calls it writes nothing of the handle but the adjoint's own buffers (the per-instance
 * gradients behind a batch sum are one of them, allocated on first use): a solve after it is bit-identical to the same solve without it. */
int mpcqp_adjoint_model(mpcqp_handle *h, const mpcqp_adjoint_io *io, const mpcqp_adjoint_model_io *mo);

#ifdef __cplusplus
}
#endif
#endif
