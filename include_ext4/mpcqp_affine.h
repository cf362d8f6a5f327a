/*
 * mpcqp_affine.h -- an affine term in the prediction model:  x_{k+1} = Ad x_k + Bd u_k + d_k.  The offset of a linearisation away from an
 * equilibrium (c = f(xbar, ubar) - A xbar - B ubar), or a measured disturbance with a preview.  An extension beside the headers of
 * include/, include_ext/, include_ext2/ and include_ext3/, which stay as they are; exported by libmpcqp_hip.so.
 *
 * In the QP of mpcqp.h the dynamics rows are  -x_{k+1} + Ad x_k + Bd u_k = 0;  with the term, rows (k+1) nx .. (k+2) nx - 1 get
 * l = u = 0.0 - d_k and nothing else changes: P, A, the row types, the rho vector, the scaling and the KKT factor are those of the
 * d-free problem, so setting a term costs no factorization.  d is `d_rows` rows of nx per instance: d_rows = 1 is one offset used at
 * every stage, d_rows = Np gives row k to the step k -> k+1 (k = 0 .. Np-1).
 *
 * The term is step data, like xref: it stays in force across mpcqp_update, mpcqp_solve, mpcqp_mpc_step, mpcqp_step_host,
 * mpcqp_update_model and mpcqp_update_settings until it is replaced or cleared; mpcqp_setup clears it, and so do the calls that put the
 * caller's own l, u in force (mpcqp_setup_qp / _csc, mpcqp_update_vectors with l, u).  With no term set every kernel
 * computes what it computed before this header existed, bit for bit, and a term of zeros gives those bits too (0.0 - 0.0 is +0.0).
 * d must be finite: a non-finite entry changes its row's type, as a non-finite x0 does, and the solve's type check refactors for it.
 *
 * Not covered (each refused, never ignored): the taped rollouts and their reverse sweeps (include/mpcqp_rollout.h,
 * include/mpcqp_rollout_est.h, include_ext/mpcqp_rollout_tv.h, include_ext2/mpcqp_rollout_tv_est.h) answer MPCQP_ERR_UNSUPPORTED on a
 * handle that has a term; output feedback under a schedule of terms; raw-vector mode.  mpcqp_gains has no K_d, and mpcqp_eq_solve's gains
 * do not depend on the term.
 */
#ifndef MPCQP_AFFINE_H
#define MPCQP_AFFINE_H

#include <stdint.h>

#include "../include/mpcqp_adjoint.h"
#include "../include/mpcqp_model.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d: [batch][d_rows * nx], a host or a device pointer (device: the call is stream-ordered).  d == NULL or d_rows == 0 clears the term.
 * d_rows not in {0, 1, Np}: MPCQP_ERR_ARG.  Before mpcqp_setup: MPCQP_ERR_STATE.  Raw-vector mode (mpcqp_setup_qp / _csc,
 * mpcqp_update_vectors): MPCQP_ERR_STATE -- there l and u are the caller's.  Like mpcqp_update the call detaches the current solution
 * from the adjoint: mpcqp_adjoint and mpcqp_gains answer MPCQP_ERR_STATE until the next solve. */
int mpcqp_set_affine(mpcqp_handle *h, const double *d, int d_rows);

/* The term in force: *d_rows (0: none) and, if d != NULL, its [batch][d_rows * nx] doubles (host or device; a host d synchronises).
 * mpcqp_export_qp shows 0.0 - d on the dynamics rows of l and u. */
int mpcqp_get_affine(mpcqp_handle *h, double *d, int *d_rows);

/* A schedule of terms for the device loop: entry e is in force for the solves after steps e * hold .. e * hold + hold - 1. */
typedef struct {
    int32_t struct_size, hold;   /* sizeof(mpcqp_affine_traj); hold >= 1: steps per entry */
    int32_t nentries, rows;      /* nentries >= ceil(nsteps / hold); rows: 1 or Np */
    const double *d;             /* [nentries][batch][rows * nx], host or device */
} mpcqp_affine_traj;

/* mpcqp_mpc_loop_tv(h, nsteps, io, mt) (mt may be NULL: mpcqp_mpc_loop) in which the solve that follows step k uses entry k / at->hold --
 * the indexing of the model schedule's entries and, at hold = 1, of io->xref_traj[k]: one entry (A_e, B_e, c_e) per relinearisation, or
 * one preview window per step.  at == NULL: exactly mpcqp_mpc_loop_tv, with the handle's own term if it has one (a term that does not
 * change over the launch keeps the register-resident carry between steps; a schedule switches it off, as io->xref_traj does).  After the
 * run the handle holds the last entry used.
 * The PLANT of the loop does not change: x = Ap x + Bp u + w[k], and with io->Ap == NULL the plant is the model's Ad, Bd WITHOUT the
 * offset -- a caller whose plant has the offset puts it into io->w.
 * Refused before any launch, with nothing changed: wrong struct_size, hold < 1, nentries < ceil(nsteps / hold), rows neither 1 nor Np,
 * d == NULL: MPCQP_ERR_ARG; output feedback (io->ny > 0): MPCQP_ERR_UNSUPPORTED. */
int mpcqp_mpc_loop_affine(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt, const mpcqp_affine_traj *at);

/* mpcqp_adjoint(h, io), from the same factorization and solve, that also writes d_d [batch][d_rows * nx] (host or device), the gradient
 * with respect to the term in the shape it was set in: d_rows = Np: d_d[k] = -r_y of row block k + 1 (the rule that gives d_x0 for row
 * block 0); d_rows = 1: the sum of those over k.  d_d == NULL: MPCQP_ERR_ARG.  On a handle without a term: MPCQP_ERR_STATE.
 * (mpcqp_adjoint itself stays correct with a term set: it reads its bounds where every other kernel does.) */
int mpcqp_adjoint_affine(mpcqp_handle *h, const mpcqp_adjoint_io *io, double *d_d);

#ifdef __cplusplus
}
#endif
#endif
