"""k_rollout_adjoint<NB> (pympc_amd/csrc/mpcqp_rollout.h) in the compiler's resource remarks of the build: every instantiation exists and
is resident.  It carries k_adjoint's state and the recursion's on top, so it may use scratch; the figures are recorded in DESIGN.md, no
number is pinned here.  k_adjoint and k_polish keep theirs (tests/test_kernel_resources.py)."""
import re

from util import kernel_resources


def test_the_rollout_kernels():
    ks = kernel_resources()
    ro = {int(m.group(1)): v for n, v in ks.items() for m in [re.match(r'_Z17k_rollout_adjointILi(\d+)EE', n)] if m}
    assert sorted(ro) == [16, 32, 64, 128], sorted(ro)
    for nb, v in ro.items():
        print('ROLLOUT_RESOURCES k_rollout_adjoint<%d>: VGPRs %s AGPRs %s scratch %s B/lane occupancy %s' % (nb, v['VGPRs'], v['AGPRs'], v['ScratchSize'], v['Occupancy']))
        assert int(v['Occupancy']) >= 1, (nb, v)
        assert int(v['VGPRs']) + int(v['AGPRs']) <= 512, (nb, v)
    assert any(n.startswith('_Z14k_rollout_tape') for n in ks), 'k_rollout_tape is not in the resource remarks'
