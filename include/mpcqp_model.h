/*
 * mpcqp_model.h -- change the model of a controller that is in use: relinearised plants, scheduled weights and bounds (the LTV use of a
 * linear MPC solver; what OSQP users do with update(Px=, Ax=)).  An extension beside mpcqp.h, whose declarations and structs stay as they
 * are; exported by libmpcqp_hip.so.
 *
 * Without it the only route is: read the iterate back, mpcqp_setup again with all fourteen model fields and the step data, push the iterate
 * back with mpcqp_warm_start.  mpcqp_update_model does the same work on the device -- re-equilibration, rho vector from the current bounds
 * with rho = settings.rho, factorization with the handle's backend, shared-factor map -- and leaves the iterate where it is: it is kept in
 * unscaled units, so new scaling vectors do not touch it.
 */
#ifndef MPCQP_MODEL_H
#define MPCQP_MODEL_H

#include <stdint.h>

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Merge the given fields of M into the handle's model and rebuild everything that depends on it.  Every field is [batch][...] as in
 * mpcqp_setup, a host or a device pointer; NULL = unchanged.  M == NULL or no field given: MPCQP_ERR_ARG; before a setup call:
 * MPCQP_ERR_STATE.
 *  - No cold start: x, y and the last mpcqp_info stay readable, mpcqp_get_solution / mpcqp_get_u0 answer as before the call until the next
 *    solve.  That solve begins from z = A_new x and gives, bit for bit, what mpcqp_get_iterate, mpcqp_setup (or mpcqp_setup_qp) with the
 *    merged model and the same step data, mpcqp_warm_start(x, y), mpcqp_solve give.  rho starts from settings.rho again, as after a setup.
 *  - A non-positive pivot of the new factorization sets info.status = MPCQP_NON_CVX (iter = 0), as setup does.
 *  - Raw-vector mode (mpcqp_setup_qp / _csc, mpcqp_update_vectors) is kept, and so are q, l, u: there the bound fields of M are the tables
 *    l and u were decoded into (one period of each row block), so giving one changes those rows.
 *  - Stream-ordered: with every given field in device memory the call returns without waiting. */
int mpcqp_update_model(mpcqp_handle *h, const mpcqp_model *M);

/* A schedule of models for the device loop: entry e is in force during steps e * hold .. e * hold + hold - 1. */
typedef struct {
    int32_t struct_size, hold;   /* sizeof(mpcqp_model_traj); hold >= 1: steps per entry */
    int32_t nmodels, reserved;   /* nmodels >= ceil(nsteps / hold); 0 */
    const double *Ad;            /* [nmodels][batch][nx*nx], or NULL (Ad does not change) */
    const double *Bd;            /* [nmodels][batch][nx*nu], or NULL (Bd does not change) */
} mpcqp_model_traj;

/* mpcqp_mpc_loop with a time-varying model: at the start of every step k with k % hold == 0, entry k / hold replaces Ad and / or Bd
 * (mpcqp_update_model), then the step runs as in mpcqp_mpc_loop -- the input applied at step k is still the one the last solve produced,
 * and with io->Ap == NULL the plant is the model now in force.  The call IS, per entry, mpcqp_update_model(entry) followed by
 * mpcqp_mpc_loop(min(hold, steps left)) on the trajectory buffers advanced to the entry's first step: one pair of setup launches and one
 * closed-loop launch per entry, all stream-ordered, with no host wait in between when every buffer is device memory.
 * mt == NULL: exactly mpcqp_mpc_loop.  Wrong struct_size, hold < 1, nmodels < ceil(nsteps / hold), neither Ad nor Bd: MPCQP_ERR_ARG
 * (nothing has been changed).  io->ny > 0 (output feedback): MPCQP_ERR_UNSUPPORTED for now. */
int mpcqp_mpc_loop_tv(mpcqp_handle *h, int nsteps, const mpcqp_loop *io, const mpcqp_model_traj *mt);

#ifdef __cplusplus
}
#endif
#endif
