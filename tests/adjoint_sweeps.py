"""numpy emulation of k_adjoint's multiplier sweeps (pympc_amd/csrc/mpcqp_adjoint.h) with exact inner solves: what the
ALGORITHM gives on an iterate, apart from the kernel's arithmetic -- to tell truncation of the sweeps from a kernel error.  Dense, in the
scaled space (D, E, c):  K_pol = c D P D + delta I + As' diag(omega) As,  omega = 1 / delta on the active rows.  Per sweep
    gt = y + omega (As x),   r = c D g - Ps x - As' gt,   d = K_pol^-1 r,   x += d,   y = gt + omega (As d)
and the stopping rule: refine_iter sweeps after the first at least, then on, at most extra_iter more, until the correction is below 1e-12
of the solution max(|x|, |y|) and 1e-10 of y, or no longer shrinks by a tenth."""
import numpy as np
import scipy.linalg as sla


def sweeps(P, A, low, upp, g, D, E, c, delta=1e-6, refine_iter=3, extra_iter=60):
    """(r_w, r_y, sweeps made) in unscaled units for one seed g."""
    P, A = np.asarray(P.toarray() if hasattr(P, 'toarray') else P), np.asarray(A.toarray() if hasattr(A, 'toarray') else A)
    n, m = P.shape[0], A.shape[0]
    act = low | upp
    Ps, As = c * (D[:, None] * P * D[None, :]), E[:, None] * A * D[None, :]
    om = np.where(act, 1.0 / delta, 0.0)
    Kpol = Ps + delta * np.eye(n) + As.T @ (om[:, None] * As)
    lu = sla.lu_factor(Kpol)
    gs, x, y, last = c * D * g, np.zeros(n), np.zeros(m), 0.0
    for sw in range(refine_iter + extra_iter + 1):
        gt = np.where(act, y + om * (As @ x), 0.0)
        r = gs - Ps @ x - As.T @ gt
        d = sla.lu_solve(lu, r)
        for _ in range(3):
            d += sla.lu_solve(lu, r - Kpol @ d)
        x = x + d
        ynew = gt + om * (As @ d)
        dy, y = np.abs(ynew - y).max(), ynew
        rel = max(np.abs(d).max() / max(np.abs(x).max(), np.abs(y).max(), 1e-300), 1e-2 * dy / max(np.abs(y).max(), 1e-300))
        if sw >= refine_iter and (rel <= 1e-12 or rel > 0.9 * last):
            break
        last = rel
    return D * x, E * y / c, sw + 1
