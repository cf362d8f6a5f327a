"""Second models and model schedules for the update_model tests (tests/test_update_model_host.py, tests/test_gpu_update_model.py)."""
import numpy as np

MODEL_FIELDS = ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu', 'xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax')


def new_model(kw, seed=1, amp=0.02):
    """Another model for the fixture ``kw``: Ad and Bd perturbed entry by entry by ``amp`` (relative, so zeros stay zeros and the QP keeps its
    sparsity pattern), other weights, a wider state box and a tighter input and input-rate box.  Returns the dict of changed fields."""
    rng = np.random.default_rng(seed)
    f = lambda k: np.array(kw[k], dtype=float)
    Ad, Bd = f('Ad'), f('Bd')
    return dict(Ad=Ad * (1.0 + amp * rng.standard_normal(Ad.shape)), Bd=Bd * (1.0 + amp * rng.standard_normal(Bd.shape)),
                Qx=1.5 * f('Qx'), QxN=2.0 * f('QxN'), Qu=1.2 * f('Qu'), QDu=0.8 * f('QDu'),
                xmin=1.1 * f('xmin'), xmax=1.1 * f('xmax'), umin=0.95 * f('umin'), umax=0.95 * f('umax'),
                Dumin=0.9 * f('Dumin'), Dumax=0.9 * f('Dumax'))


def with_model(kw, new):
    """The fixture's constructor arguments with the fields of ``new`` replaced (hidden switches in ``.attrs`` carried over)."""
    kw2 = type(kw)(kw)
    if hasattr(kw, 'attrs'):
        kw2.attrs = kw.attrs
    kw2.update(new)
    return kw2


def model_schedule(Ad, Bd, nmodels, seed=3, amp=0.03):
    """A seeded smooth schedule around (Ad, Bd): entry e = M * (1 + amp * (sin(0.7 e + phase) with a random phase per entry of M)).
    Returns (Ad [nmodels, nx, nx], Bd [nmodels, nx, nu])."""
    rng = np.random.default_rng(seed)
    Ad, Bd = np.asarray(Ad, dtype=float), np.asarray(Bd, dtype=float)
    pa, pb = rng.uniform(0, 2 * np.pi, Ad.shape), rng.uniform(0, 2 * np.pi, Bd.shape)
    e = np.arange(nmodels).reshape(-1, 1, 1)
    return Ad[None] * (1.0 + amp * np.sin(0.7 * e + pa[None])), Bd[None] * (1.0 + amp * np.sin(0.7 * e + pb[None]))
