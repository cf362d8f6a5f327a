"""k_rollout_adjoint_tv_est<NB> (pympc_amd/csrc/mpcqp_rollout.h) in the compiler's resource remarks of the build: every instantiation
exists and is resident, and it is a kernel of its own -- the three older sweeps keep their signatures (they take no RolloutGains).  The
figures are recorded in DESIGN.md section 5l, no number is pinned here."""
import re

from util import kernel_resources


def test_the_fourth_sweep_and_the_signatures_of_the_other_three():
    ks = kernel_resources()
    new = {int(m.group(1)): (n, v) for n, v in ks.items() for m in [re.match(r'_Z24k_rollout_adjoint_tv_estILi(\d+)EE', n)] if m}
    assert sorted(new) == [16, 32, 64, 128], sorted(new)
    for nb, (n, v) in new.items():
        print('ROLLOUT_TV_EST_RESOURCES k_rollout_adjoint_tv_est<%d>: VGPRs %s AGPRs %s scratch %s B/lane occupancy %s' % (nb, v['VGPRs'], v['AGPRs'], v['ScratchSize'], v['Occupancy']))
        assert int(v['Occupancy']) >= 1 and int(v['VGPRs']) + int(v['AGPRs']) <= 512, (nb, v)
        assert n.endswith('12RolloutSlots12RolloutGains'), n
    for prefix, tail in (('_Z17k_rollout_adjointILi', '12RolloutSweep'), ('_Z21k_rollout_adjoint_estILi', '12RolloutSweep'), ('_Z20k_rollout_adjoint_tvILi', '12RolloutSlots')):
        names = [n for n in ks if n.startswith(prefix)]
        assert len(names) == 4 and all(n.endswith(tail) for n in names), (prefix, names)
