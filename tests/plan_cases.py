"""Case table of tests/test_plan.py, tests/test_gpu_plan.py and scripts/record_plan_table.py: the handles whose plan
(pympc_amd/csrc/mpcqp_plan.h: backend, LDS layout, solve kernel, and the getters' arithmetic on them) is pinned by
tests/golden/plan_table.json, recorded through the library's public getters.  Handles are created, never set up or solved."""
import json
import os

from util import GOLDEN_DIR

TABLE = os.path.join(GOLDEN_DIR, 'plan_table.json')
NCU = 256                                   # compute units of the MI355X the table was recorded on: the AUTO cross-overs count instances per unit
AUTO, SWEEPS, DENSE, BCR, BCR8, BCRT = range(6)            # enum mpcqp_backend
NO_LSTAGE, NO_GROUPING, NO_W8 = 2, 4, 8                    # enum mpcqp_tuning

# (batch, nx, nu, Np, Nc, soft, backend, tuning)
CASES = []


def case(batch, nx, nu, Np, Nc=None, soft=1, backend=AUTO, tuning=0):
    CASES.append((batch, nx, nu, Np, Np if Nc is None else Nc, soft, backend, tuning))


# ---- every block size ----------------------------------------------------------------------------------------------------------------
case(2, 12, 4, 10, backend=SWEEPS)          # NB 16, iterate in LDS
case(4096, 12, 4, 40)                       # NB 16, iterate in memory
case(4096, 10, 3, 20, backend=SWEEPS)       # NB 16 generic, iterate in LDS
case(4096, 12, 4, 20, 10)                   # ... with a held input
case(1, 20, 8, 12)                          # NB 32: BASELINE cfg-5
case(1024, 20, 8, 12)
case(1, 20, 8, 100)
case(1024, 20, 8, 100)
case(1024, 20, 8, 12, 6)                    # NB 32 generic with a held input
case(1024, 20, 9, 20)
case(1024, 20, 8, 40, 20)                   # ... and its iterate in memory
case(2, 20, 8, 3)                           # a 32-wide shape short enough for an LDS iterate
case(2, 20, 8, 3, 2)
case(1, 40, 8, 10)                          # NB 64
case(2, 40, 8, 10, 5)
case(1, 56, 8, 5)
case(1, 100, 28, 3)                         # NB 128
case(2, 100, 28, 4, 2)
case(1, 30, 40, 3, 2)                       # a held input with large nu: Sigma and its inverse outgrow the factorization's workspace
# ---- dense ------------------------------------------------------------------------------------------------------------------------------
for shape in ((4, 1, 20), (12, 4, 7)):
    case(6 * NCU, *shape)
    case(6 * NCU + 1, *shape)
case(4096, 3, 1, 30, backend=DENSE)
case(1, 4, 1, 20, 10)                       # the dense inverse holds a held input's couplings itself
case(1, 2, 2, 12, soft=0)
# ---- cyclic reduction: the 11-, 21- and 31-stage schedules under each backend, generic and (12, 4) ---------------------------------------
for Np in (10, 20, 30):
    for backend in (BCR, BCR8, BCRT):
        case(2, 6, 3, Np, backend=backend)
        case(2, 12, 4, Np, backend=backend)
for shape in ((12, 4, 20), (6, 2, 20)):     # AUTO: up to three instances per compute unit ...
    case(3 * NCU, *shape)
    case(3 * NCU + 1, *shape)
for shape in ((12, 4, 30), (6, 3, 28)):     # ... at every batch size on the 31-stage schedule of stages wider than 8
    case(1, *shape)
    case(4096, *shape)
case(2, 12, 4, 30, backend=SWEEPS)          # (12, 4, 30) forced to SWEEPS
case(4096, 12, 4, 30, backend=SWEEPS)
case(4096, 12, 4, 30, soft=0)
# ---- grouped stages: the reference's notebook and Kalman horizons, alone and beyond one instance per compute unit ---------------------------
for tuning in (0, NO_W8, NO_GROUPING, NO_LSTAGE):
    for batch in (1, NCU + 1):
        case(batch, 4, 1, 150, 75, tuning=tuning)
        case(batch, 4, 1, 200, 200, tuning=tuning)
for batch in (1, NCU + 1):                  # a generic nx + nu <= 8 long horizon, with and without a held input
    case(batch, 5, 2, 100)
    case(batch, 5, 2, 100, 50)
# ---- the staged round, on and off, around batch == compute units ---------------------------------------------------------------------------
for shape in ((20, 9, 20), (12, 4, 40)):
    case(NCU, *shape)
    case(NCU + 1, *shape)
    case(NCU, *shape, tuning=NO_LSTAGE)
case(1, 40, 8, 10, tuning=NO_LSTAGE)
case(1, 20, 8, 12, soft=0)
case(1, 40, 8, 10, soft=0)
# ---- one shape on each side of the hot-prefix rule (smem + extra + 1024) * occ <= 160 KB, per occupancy -------------------------------------------
case(1024, 12, 4, 86); case(1024, 12, 4, 87)       # four workgroups per compute unit
case(1024, 20, 9, 90); case(1024, 20, 9, 91)       # two
case(1, 40, 8, 64); case(1, 40, 8, 65)             # one
# ---- every refusal -----------------------------------------------------------------------------------------------------------------------
case(1, 12, 4, 30, backend=DENSE)           # DENSE on 864 unknowns
case(1, 12, 4, 40, backend=BCR)             # BCR on Np = 40
case(1, 12, 4, 30, 15, backend=BCR8)        # BCR8 with Nc < Np
case(1, 12, 4, 30, backend=6)               # backend out of range
case(1, 12, 4, 30, backend=-1)
case(1, 100, 29, 5)                         # nx + nu > 128
case(1, 4, 1, 1, 1)                         # Np < 2
case(1, 40, 8, 80)                          # over 160 KB of LDS (exists well below nx + nu = 128: 48-wide stages on 81 of them)


def load_table():
    with open(TABLE) as f:
        t = json.load(f)
    assert [tuple(r['case']) for r in t['rows']] == CASES, 'tests/golden/plan_table.json is not a record of tests/plan_cases.py: record it again'
    return t


def handle_record(L, Settings, c):
    """What the library's public getters say of the handle of case c (created, never set up): the row of the table."""
    import ctypes as C
    batch, nx, nu, Np, Nc, soft, backend, tuning = c
    S = Settings()
    L.mpcqp_default_settings(C.byref(S))
    S.soft_constraints, S.backend, S.tuning = soft, backend, tuning
    h = C.c_void_p()
    rc = L.mpcqp_create(C.byref(h), 0, batch, nx, nu, Np, Nc, C.byref(S))
    if rc != 0:
        return dict(case=list(c), rc=rc, error=L.mpcqp_last_error().decode())
    try:
        names = []
        for loop in (0, 1):
            buf = C.create_string_buffer(128)
            assert L.mpcqp_kernel_name(h, loop, buf, 128) == 0
            names.append(buf.value.decode())
        occ = [C.c_int() for _ in range(3)]
        assert L.mpcqp_get_occupancy(h, *[C.byref(v) for v in occ]) == 0
        n, m, fd, nnzL = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
        assert L.mpcqp_get_dims(h, C.byref(n), C.byref(m), C.byref(fd), C.byref(nnzL)) == 0
        sb = [C.c_int64() for _ in range(3)]
        assert L.mpcqp_get_stream_bytes(h, *[C.byref(v) for v in sb]) == 0
        w = C.c_int64()
        assert L.mpcqp_get_work(h, C.byref(w)) == 0
        return dict(case=list(c), rc=0, kernel=names, occupancy=[v.value for v in occ], dims=[n.value, m.value, fd.value, nnzL.value],
                    stream_bytes=[v.value for v in sb], work=w.value)
    finally:
        L.mpcqp_destroy(h)
