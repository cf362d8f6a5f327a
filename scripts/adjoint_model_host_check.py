#!/usr/bin/env python3
"""The arithmetic and the indexing of k_adjoint_model (pympc_amd/csrc/mpcqp_adjoint_model.h) checked on the host, without a GPU.

The kernel's entry function adjoint_model_entry is cut out of the header as it stands, compiled with g++ behind a driver that reproduces
the kernel's schedule (S = NT / entries ranges of the stage sum per entry, partial sums added in range order), and
  1. run as a STAND-ALONE program under AddressSanitizer / UBSan on arrays of exactly n, m, step and model doubles, over shapes that take
     every path: (4, 2, 200), (20, 8, 60), (64, 5, 3), Nc < Np, Nc = 1, no slack variables, Np + 1 reference rows;
  2. loaded (plain build) and fed the CPU oracle's iterate and the restatement's r_w, r_y of golden fixtures: every entry against the
     numpy sums of tests/adjoint_model_ref.py, relative to the sum of the absolute values of its terms.

    python scripts/adjoint_model_host_check.py [--keep DIR]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

DRIVER_HEAD = '''
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
using std::min; using std::max;
#define __device__
#define __forceinline__ inline
constexpr int NT = 256, ADJOINT_COLS = 4;
struct Lay { int nx, nu, Np, Nc, N, n, m, n_x, n_u, ou, oe, soft, ouref, xref_rows, model_sz, step_sz; };
'''
DRIVER_TAIL = '''
extern "C" void run(const int *dims, const double *W, const double *RW, const double *Y, const double *RY, const double *model, const double *step, double *out) {
    Lay L{}; L.nx = dims[0]; L.nu = dims[1]; L.Np = dims[2]; L.Nc = dims[3]; L.soft = dims[4]; L.xref_rows = dims[5]; L.ouref = dims[6];
    L.N = L.Np + 1; L.n_x = L.N * L.nx; L.n_u = L.Nc * L.nu; L.ou = L.n_x; L.oe = L.n_x + L.n_u;
    AdjointModelArgs M{}; const int sz[7] = {L.nx * L.nx, L.nx * L.nu, L.nx * L.nx, L.nx * L.nx, L.nu * L.nu, L.nu * L.nu, 1};
    M.off[0] = 0; for (int f = 0; f < 7; ++f) M.off[f + 1] = M.off[f] + sz[f];
    const int E = M.off[7], S = E < NT ? NT / E : 1;
    for (int e = 0; e < E; ++e) {
        double v = 0.0;
        for (int s = 0; s < S; ++s) { const double p = adjoint_model_entry(L, M, W, RW, Y, RY, model, step, e, s, S); v = s ? v + p : p; }
        out[e] = v;
    }
}
#ifdef WITH_MAIN
int main() {
    const int cases[][6] = {{4,2,200,200,1,1},{20,8,60,60,1,1},{5,3,8,4,0,1},{2,1,25,10,1,26},{4,1,20,1,1,1},{64,5,3,3,1,1},{18,9,6,3,1,7},{7,7,4,4,0,1},{1,1,2,1,1,3}};
    for (auto &c : cases) {
        const int nx = c[0], nu = c[1], Np = c[2], Nc = c[3], soft = c[4], rows = c[5], N = Np + 1;
        const int n = (soft ? 2 : 1) * N * nx + Nc * nu, m = 2 * N * nx + Nc * nu + (Nc + 1) * nu;
        std::vector<double> W(n), RW(n), Y(m), RY(m), model(7 + nu), step(nx + nu + rows * nx);      // exact sizes: a read past them is reported
        for (auto *v : {&W, &RW, &Y, &RY, &model, &step}) for (auto &x : *v) x = rand() / (double)RAND_MAX - 0.5;
        const int dims[7] = {nx, nu, Np, Nc, soft, rows, 7};
        std::vector<double> out(3 * nx * nx + nx * nu + 2 * nu * nu + 1);
        run(dims, W.data(), RW.data(), Y.data(), RY.data(), model.data(), step.data(), out.data());
        printf("(%d, %d, %d) Nc %d soft %d xref rows %d: clean\\n", nx, nu, Np, Nc, soft, rows);
    }
    return 0;
}
#endif
'''


def entry_source():
    src = open(os.path.join(ROOT, 'pympc_amd', 'csrc', 'mpcqp_adjoint_model.h')).read()
    return src[src.index('constexpr int ADJM_FIELDS'):src.index('__global__ __launch_bounds__(NT) void k_adjoint_model(')]


def against_numpy(lib, name):
    import adjoint_ref as ar
    import adjoint_model_ref as am
    from adjoint_cases import solve_golden
    kw0, (P, q, A, l, u), r, (x, z, y), (D, E, c) = solve_golden(name, 1e-9)
    kw, attrs = am.full_kwargs(kw0), dict(kw0.attrs)
    g = np.random.default_rng(7).standard_normal(P.shape[0])
    res = ar.adjoint(P, A, l, u, x, z, y, D, E, c, g)
    cf, mag = am.closed_form_of(kw, attrs, x, y, res['r_w'], res['r_y'])
    nx, nu = kw['Bd'].shape
    Np = kw['Np']
    Nc = Np if kw.get('Nc') is None else kw['Nc']
    xr = np.asarray(kw['xref'], dtype=float)
    rows = 1 if xr.ndim == 1 else Np + 1
    step = np.concatenate([kw['x0'], kw['uminus1'], xr.ravel()[:rows * nx]])
    model = np.concatenate([np.zeros(7), kw['uref']])
    dims = (C.c_int * 7)(nx, nu, Np, Nc, int(attrs.get('SOFT_ON', True)), rows, 7)
    out = np.zeros(3 * nx * nx + nx * nu + 2 * nu * nu + 1)
    arrs = [np.ascontiguousarray(v, dtype=float) for v in (x, res['r_w'], y, res['r_y'], model, step)]
    lib.run(dims, *[a.ctypes.data_as(C.c_void_p) for a in arrs], out.ctypes.data_as(C.c_void_p))
    o, worst = 0, 0.0
    for k, shp in (('Ad', (nx, nx)), ('Bd', (nx, nu)), ('Qx', (nx, nx)), ('QxN', (nx, nx)), ('Qu', (nu, nu)), ('QDu', (nu, nu)), ('eps_feas', ())):
        cnt = int(np.prod(shp)) if shp else 1
        v = out[o:o + cnt].reshape(shp) if shp else out[o]
        o += cnt
        err = np.abs(v - cf[k])
        assert np.all(err <= 1e-12 * mag[k]), (name, k, float(np.max(err)))
        worst = max(worst, float(np.max(err / np.maximum(mag[k], 1e-300))))
        if k in am.WEIGHTS:
            assert np.array_equal(v, v.T), (name, k)
    print('%s: %d entries, largest |host build - numpy| / sum|terms| = %.2e' % (name, out.size, worst))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--keep', default=None, help='directory to leave the generated program in')
    a = ap.parse_args()
    d = a.keep or tempfile.mkdtemp(prefix='adjm_host_')
    os.makedirs(d, exist_ok=True)
    cpp = os.path.join(d, 'adjoint_model_host.cpp')
    open(cpp, 'w').write(DRIVER_HEAD + entry_source() + DRIVER_TAIL)
    exe, so = os.path.join(d, 'adjoint_model_host_asan'), os.path.join(d, 'adjoint_model_host.so')
    subprocess.check_call(['g++', '-O1', '-g', '-DWITH_MAIN', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe, cpp])
    subprocess.check_call([exe])
    subprocess.check_call(['g++', '-O2', '-fPIC', '-shared', '-o', so, cpp])
    lib = C.CDLL(so)
    for name in ('random_5_3_8', 'point_mass_nc', 'cart_pole_nc1', 'random_12_4_30_hard', 'small_mimo', 'random_5_3_8_nc_hard'):
        against_numpy(lib, name)
    print('ok')


if __name__ == '__main__':
    main()
