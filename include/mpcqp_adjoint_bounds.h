/*
 * mpcqp_adjoint_bounds.h -- the adjoint derivatives chained into the controller's constraint bounds xmin, xmax, umin, umax, Dumin, Dumax:
 * for the single solve (mpcqp_adjoint / mpcqp_adjoint_model) and for the reverse sweeps over a tape (mpcqp_rollout_adjoint /
 * mpcqp_rollout_adjoint_est).  An extension beside mpcqp_adjoint.h, mpcqp_adjoint_model.h, mpcqp_rollout.h and mpcqp_rollout_est.h, whose
 * declarations and structs stay as they are; exported by libmpcqp_hip.so.
 *
 * In the notation of mpcqp_adjoint.h, dL/db_r = r_y[r] on the active rows r, and every inequality row's bound IS one of the controller's
 * bounds (pyMPC/mpc.py:551-580):
 *     state-box rows   stage k = 0 .. Np, component i:       xmin[i] <= x_k[i] (+ eps_k[i] with slack columns) <= xmax[i]
 *     input-box rows   stage k = 0 .. Nc-1, component j:     umin[j] <= u_k[j] <= umax[j]
 *     Delta-u rows     block k = 0 .. Nc, component j:       Dumin[j] <= (row of the difference operator) <= Dumax[j]; block 0 carries u_0
 *                                                            alone against Dumin[j] + u_{-1}[j], Dumax[j] + u_{-1}[j]
 * so
 *     d_xmin[i]  = sum of r_y[r] over the state-box rows r of component i that are lower-active,     d_xmax[i]: upper-active
 *     d_umin[j]  = ... over the Nc input-box rows of component j,                                      d_umax[j]
 *     d_Dumin[j] = ... over all Nc + 1 Delta-u rows of component j, the first included,                d_Dumax[j]
 * each sum in ascending row order.  A row whose two bounds are equal counts as lower-active, as in d_l / d_u: the derivative with respect
 * to the common value is in the lower name, 0 in the upper.  A bound at or beyond +-1e30 is clipped to it and never active: its gradient is
 * exactly 0.  The path of u_{-1} through the first Delta-u rows stays in d_uminus1.
 *
 * In a sweep the bounds are the handle's, constant over the tape: the gradient is the sum of the per-entry sums over the tape entries that
 * were differentiated (status 1 in mpcqp_get_rollout_info); an entry that applied u_failure or whose factorization broke adds zero.  Each
 * sum is formed by one thread in the order K-1 .. 0, without atomics: two sweeps over the same tape give the same bits.
 */
#ifndef MPCQP_ADJOINT_BOUNDS_H
#define MPCQP_ADJOINT_BOUNDS_H

#include <stdint.h>

#include "mpcqp_adjoint.h"
#include "mpcqp_adjoint_model.h"
#include "mpcqp_rollout.h"
#include "mpcqp_rollout_est.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every array is [batch][...] row-major (batch_sum = 1: [1][...], the sum over the batch), a host or a device pointer; any may be NULL. */
typedef struct {
    int32_t struct_size, batch_sum;   /* sizeof(mpcqp_adjoint_bounds_io); 0: one gradient per instance, 1: their sum over the batch (one set of
                                         bounds shared by many states), formed on the device in a fixed order without floating-point atomics */
    double *d_xmin, *d_xmax;          /* [batch][nx] */
    double *d_umin, *d_umax;          /* [batch][nu] */
    double *d_Dumin, *d_Dumax;        /* [batch][nu] */
} mpcqp_adjoint_bounds_io;

/* Everything mpcqp_adjoint_model(h, io, mo) does, and the bound gradients of the same seed from the same single factorization: a small
 * kernel on the handle's stream behind the adjoint's reduces its rows to the bounds.  bo == NULL: exactly mpcqp_adjoint_model (which with
 * mo == NULL is exactly mpcqp_adjoint).  With every given pointer in device memory the call is stream-ordered and returns without waiting.
 * Wrong struct_size, a batch_sum other than 0 or 1, or nothing asked for in any of the structs: MPCQP_ERR_ARG.  The MPCQP_ERR_STATE cases of
 * mpcqp_adjoint carry over; in raw-vector mode any output of bo is MPCQP_ERR_STATE -- there the bounds are l and u themselves, and d_l, d_u
 * are the answer.  An instance whose adjoint status is 0 or -1 gets zeros and adds zeros to a batch sum.  Like the other adjoint calls it
 * writes nothing of the handle but the adjoint's own buffers: a solve after it is bit-identical to the same solve without it. */
int mpcqp_adjoint_bounds(mpcqp_handle *h, const mpcqp_adjoint_io *io, const mpcqp_adjoint_model_io *mo, const mpcqp_adjoint_bounds_io *bo);

/* The reverse sweep over the handle's tape with the bound gradients summed over its entries.  eo == NULL: the tape is one of mpcqp_rollout
 * and the call is mpcqp_rollout_adjoint(h, io, mo) plus bo; otherwise one of mpcqp_rollout_est and the call is
 * mpcqp_rollout_adjoint_est(h, io, eo, mo) plus bo (an eo with no pointer set is allowed there as long as io carries a seed).
 * bo == NULL: exactly those calls.  Their pointer, stream-ordering, state and status rules carry over (a tape whose model was replaced:
 * MPCQP_ERR_STATE); wrong struct_size, a batch_sum other than 0 or 1 (where mo asks for a model gradient too, the two must agree), or a bo
 * given while no output is asked for in any of the structs: MPCQP_ERR_ARG.  A sweep that is not asked for bounds executes none of their code. */
int mpcqp_rollout_adjoint_bounds(mpcqp_handle *h, const mpcqp_rollout_adjoint_io *io, const mpcqp_rollout_est_io *eo,
                                 const mpcqp_adjoint_model_io *mo, const mpcqp_adjoint_bounds_io *bo);

#ifdef __cplusplus
}
#endif
#endif
