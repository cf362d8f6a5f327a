"""bench.py without --full runs the headline alone; --full adds the rest AFTER the timed steps.  Both runs of the same command time the same
steps on the same inputs: the outputs of the last timed step (--dump-outputs) are bit-identical, and only the full run carries the u*
comparison against the CPU reference.  The single-controller latency workload keeps the same split (CPU oracle beside it with --full only)."""
import json
import os

import numpy as np
import pytest

from util import run_bench

pytestmark = pytest.mark.gpu
SMALL = ['--gpus', '1', '--steps', '4', '--warmup', '2', '--batch', '64']


def _bench(tmp_path, tag, *flags):
    env = dict(os.environ, MPCQP_BENCH_LEGS=str(tmp_path / (tag + '_legs.json')))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'MPCQP_BENCH_BACKEND', 'MPCQP_BENCH_FORCE_PG'):
        env.pop(k, None)
    return run_bench(env, *flags)


@pytest.mark.timeout(600)
def test_plain_run_times_what_the_full_run_times(tmp_path):
    plain = _bench(tmp_path, 'plain', *SMALL, '--dump-outputs', str(tmp_path / 'plain'))
    full = _bench(tmp_path, 'full', *SMALL, '--dump-outputs', str(tmp_path / 'full'), '--full', '--no-cpu-baseline', '--no-other-path')
    for k in ('u_err', 'legs', 'cpu_baseline'):
        assert k not in plain, k
    assert plain['metric'] == full['metric'] and plain['unit'] == full['unit'] == 'QP-solves/s' and plain['steps'] == 4 and plain['value'] > 0
    assert plain['mean_admm_iters'] == full['mean_admm_iters'] and plain['solved_fraction_last_step'] == full['solved_fraction_last_step']
    for name in ('u', 'x', 'status', 'iters', 'instance'):
        a, b = np.load(tmp_path / 'plain' / (name + '.npy')), np.load(tmp_path / 'full' / (name + '.npy'))
        assert a.shape == b.shape and np.array_equal(a, b), name
    # what moved behind --full still runs there: the u* sample against the CPU reference, the timing of a refactorization
    assert full['u_err']['eps_0.001']['instances'] > 0
    with open(tmp_path / 'full_legs.json') as f:
        assert json.load(f)['refactorization']['ms_per_batch'] > 0
    with open(tmp_path / 'plain_legs.json') as f:
        assert json.load(f)['refactorization']['ms_per_batch'] is None


@pytest.mark.timeout(600)
def test_latency_workload_compares_with_the_oracle_only_in_full(tmp_path):
    plain = _bench(tmp_path, 'plain', '--workload', 'cfg2')
    full = _bench(tmp_path, 'full', '--workload', 'cfg2', '--full')
    assert plain['unit'] == full['unit'] == 'us' and plain['value'] > 0 and plain['higher_is_better'] is False
    assert plain['latency']['mean_admm_iters'] == full['latency']['mean_admm_iters']
    assert 'cpu_oracle_update_us_median' not in plain['latency'] and 'raw_c_abi_step_us' not in plain['latency']
    assert full['latency']['cpu_oracle_update_us_median'] > 0 and full['latency']['raw_c_abi_step_us'] > 0
