/*
 * mpcqp_adjoint.h -- adjoint derivatives of the QP solution (what OSQP offers as adjoint_derivative_compute / adjoint_derivative_get_vec)
 * for the handles of mpcqp.h, chained into the controller's parameters x0, u_{-1}, xref, uref.  An extension beside mpcqp.h, whose
 * declarations and structs stay as they are; exported by libmpcqp_hip.so.
 *
 * The QP is  min 1/2 w'P w + q'w,  l <= A w <= u,  with solution w* and multipliers y*.  Let the active rows be every equality row
 * (l == u) and every other row the iterate marks active by OSQP's polishing rule (scaled space: lower-active if z~ - l~ < -y~, else
 * upper-active if u~ - z~ < y~), and b the bound each of them sits on.  Locally w* solves
 *     [ P    A_a' ] [ w   ]   [ -q ]
 *     [ A_a   0   ] [ y_a ] = [  b ]
 * so for a seed g = dL/dw one solve of the same symmetric system with right-hand side [g; 0] gives [r_w; r_y] and
 *     dL/dq = -r_w,     dL/db_i = r_y[i] on the active rows, 0 elsewhere,
 * and the controller's parameters follow by the chain rule through the vectors they enter (pyMPC/mpc.py:386-452):
 *     dL/dx0 = -r_y[0:nx];   dL/du_{-1} = QDu' r_w[u_0] + r_y[first nu Delta-u rows];
 *     dL/dxref = sum_k Q_k' r_w[x_k] (one row) or Q_k r_w[x_k] per row k (Np+1 rows), Q_k = Qx (k < Np), QxN (k = Np);
 *     dL/duref = sum_k iU_k Qu' r_w[u_k].
 * The system is solved as polishing solves its own (mpcqp_polish.h): regularized by delta, factored into buffers of the adjoint's own,
 * then refine_iter refinement sweeps against the unregularized system.
 *
 * The gradients are those of the active set the ITERATE implies: at a loose tolerance the rule can miss a row, so solve tightly or with
 * polish = 1 where the set must be the true one.  Where a row is weakly active (on its bound with a zero multiplier) the control law has a
 * kink and no derivative: the call counts such rows (n_weak) and returns the one-sided derivative of the active set it used.
 *
 * The calls never write the solution, the iterate, mpcqp_info, the handle's factor, rho, the shared-factor map, the polish's buffers or
 * the counters of mpcqp_get_stats / mpcqp_profile: a solve after them is bit-identical to the same solve without them.
 */
#ifndef MPCQP_ADJOINT_H
#define MPCQP_ADJOINT_H

#include <stdint.h>

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t struct_size;          /* sizeof(mpcqp_adjoint_settings): mpcqp_set_adjoint refuses any other value (MPCQP_ERR_ARG) */
    int32_t refine_iter;          /* refinement sweeps after the first solve that are always made, >= 0 (default 3) */
    double delta;                 /* regularization of the active-set KKT system, > 0 (default 1e-6) */
    double weak_tol;              /* a row counts as weakly active below this, >= 0 (default 1e-6; see mpcqp_get_adjoint_info) */
    int32_t extra_iter;           /* where the last of the refine_iter sweeps still moved the answer the kernel goes on, at most this many
                                     sweeps more, >= 0 (default 60), until the correction is negligible (1e-12 of the solution, 1e-10 of r_y) or
                                     no longer shrinks by a tenth (rows held by a slack variable contract by about 0.5 a sweep and take some
                                     30).  0: exactly refine_iter sweeps, the cost of a seed is then bounded by the setting alone */
    int32_t reserved;             /* 0 */
} mpcqp_adjoint_settings;

/* Every array is [batch][...], a host or a device pointer; with every given pointer in device memory the call is stream-ordered and
 * returns without waiting. */
typedef struct {
    int32_t struct_size;          /* sizeof(mpcqp_adjoint_io) */
    int32_t reserved;             /* 0 */
    const double *g_w;            /* [batch][n] seed dL/dw, or NULL */
    const double *g_u0;           /* [batch][nu] seed dL/du_0, added into the u_0 block of g_w, or NULL (at least one of the two) */
    /* outputs, any may be NULL */
    double *d_x0;                 /* [batch][nx] */
    double *d_uminus1;            /* [batch][nu] */
    double *d_xref;               /* [batch][xref_rows * nx], in the shape of the last upload */
    double *d_uref;               /* [batch][nu] */
    double *d_q;                  /* [batch][n] */
    double *d_l, *d_u;            /* [batch][m]: a lower-active row has r_y in d_l, an upper-active one in d_u, an equality row the derivative
                                     with respect to its common value in d_l and 0 in d_u, an inactive row 0 in both */
} mpcqp_adjoint_io;

/* Defaults: struct_size set, delta = 1e-6, refine_iter = 3, weak_tol = 1e-6, extra_iter = 60.  The adjoint's own settings: mpcqp_set_polish does not
 * change them and they do not change polishing. */
void mpcqp_adjoint_default_settings(mpcqp_adjoint_settings *s);
/* Any time after mpcqp_create / mpcqp_create_csc.  The adjoint's buffers are allocated on first use. */
int mpcqp_set_adjoint(mpcqp_handle *h, const mpcqp_adjoint_settings *s);

/* Differentiate the handle's current solution (after mpcqp_solve, mpcqp_mpc_step, mpcqp_step_host or a polish).  Before the first solve
 * after a setup, and after anything that replaced what the solution belongs to without solving again -- mpcqp_update,
 * mpcqp_update_vectors, mpcqp_update_model, mpcqp_warm_start -- MPCQP_ERR_STATE: the call never pairs an iterate with bounds, costs or a
 * model it was not computed for.  (mpcqp_update_settings changes nothing the adjoint reads.)  In raw-vector mode (mpcqp_setup_qp / _csc, mpcqp_update_vectors) only d_q, d_l, d_u are defined:
 * asking for d_x0, d_uminus1, d_xref or d_uref there is MPCQP_ERR_STATE. */
int mpcqp_adjoint(mpcqp_handle *h, const mpcqp_adjoint_io *io);

/* The Jacobians of the first input u_0 of the current solution: K_x0 [batch][nu][nx], K_uminus1 [batch][nu][nu],
 * K_xref [batch][nu][xref_rows * nx], K_uref [batch][nu][nu]; any may be NULL.  One factorization per instance, nu right-hand sides (the
 * unit seeds on the u_0 block).  Raw-vector mode: MPCQP_ERR_STATE. */
int mpcqp_gains(mpcqp_handle *h, double *K_x0, double *K_uminus1, double *K_xref, double *K_uref);

/* Of the last mpcqp_adjoint / mpcqp_gains, each [batch] (any may be NULL; host or device; synchronises):
 *   n_active  rows of the active set used;
 *   n_weak    rows with l != u and, in unscaled units,  min(z - l, u - z) <= weak_tol max(1, |z_i|)  and  |y_i| <= weak_tol max(1, |y|_inf);
 *   status    1 computed; 0 not computed (the instance's last solve did not end 'solved'): its outputs are zero; -1 the factorization
 *             of the regularized system broke (non-positive pivot or NaN): its outputs are zero.
 * Before any such call: all zero. */
int mpcqp_get_adjoint_info(mpcqp_handle *h, int32_t *n_active, int32_t *n_weak, int32_t *status);

#ifdef __cplusplus
}
#endif
#endif
