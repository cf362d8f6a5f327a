/*
 * mpcqp_polish.h -- OSQP's solution polishing (settings polish / delta / polish_refine_iter, OSQP 0.6) for the handles of mpcqp.h.
 * An extension beside mpcqp.h, whose declarations and structs stay as they are; exported by libmpcqp_hip.so.
 *
 * After a solve that ended 'solved', polishing guesses the active constraints from the iterate, solves the equality-constrained QP on
 * that active set once (regularized by delta, then polish_refine_iter refinement sweeps against the unregularized system) and keeps the
 * result only if its residuals are better (OSQP 0.6's rule).  With a right guess the answer is accurate to rounding error.  It runs on the
 * device, one workgroup per instance, in the handle's scaled space, with a factor of its own: the handle's KKT factor, rho and shared-factor
 * map are left as they are.
 *
 * Accepted (status_polish 1): x, y of mpcqp_get_solution and info.obj_val / pri_res / dua_res are the polished point's, and so is the
 * iterate (mpcqp_get_iterate) the next solve warm-starts from.  Rejected (-1): nothing changes.  Not performed (0): polishing off, or the
 * solve did not end 'solved'.  info.status / iter / rho_updates / rho and the counters of mpcqp_get_stats and mpcqp_profile never
 * include polishing.
 *
 * With polish = 1:  mpcqp_solve and mpcqp_mpc_step polish after the solve (stream-ordered; mpcqp_mpc_step before its output() gather),
 * mpcqp_step_host polishes before it returns; mpcqp_mpc_run / mpcqp_mpc_loop return MPCQP_ERR_UNSUPPORTED (no polishing inside the device
 * closed loop); mpcqp_eq_solve ignores the setting.
 */
#ifndef MPCQP_POLISH_H
#define MPCQP_POLISH_H

#include <stdint.h>

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t struct_size;          /* sizeof(mpcqp_polish_settings): mpcqp_set_polish refuses any other value (MPCQP_ERR_ARG) */
    int32_t polish;               /* 0 (default): off; 1: on */
    double delta;                 /* regularization of the reduced KKT system, > 0 (OSQP's default 1e-6) */
    int32_t polish_refine_iter;   /* refinement sweeps after the first solve, >= 0 (OSQP's default 3) */
    int32_t reserved;             /* 0 */
} mpcqp_polish_settings;

/* Defaults: struct_size set, polish = 0, delta = 1e-6, polish_refine_iter = 3. */
void mpcqp_polish_default_settings(mpcqp_polish_settings *s);
/* Any time after mpcqp_create / mpcqp_create_csc; applies to the solves that follow.  The polish's buffers are allocated on first use. */
int mpcqp_set_polish(mpcqp_handle *h, const mpcqp_polish_settings *s);
/* Polish the last solve of every instance now, with the handle's delta / polish_refine_iter (whether polish is on or not).
 * Stream-ordered, does not wait. */
int mpcqp_polish(mpcqp_handle *h);
/* status_polish [batch] of the last solve (1 accepted, -1 rejected, 0 not performed).  Synchronises. */
int mpcqp_get_polish_info(mpcqp_handle *h, int32_t *status_polish);

#ifdef __cplusplus
}
#endif
#endif
