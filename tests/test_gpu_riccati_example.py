"""examples/learn_noise_through_observer.py, run as a user would run it: a fresh process, its defaults (8 copies, 10 steps).  The example
asserts on its own account that the closed-loop cost went down and that the gradient with respect to diag(Qn) agrees with central
differences through the same device path; its closing line is what is read here."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(120)
def test_learning_the_noise_covariances_through_the_observer():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'learn_noise_through_observer.py')], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r'NOISE_OK cost0 ([0-9.e+-]+) cost1 ([0-9.e+-]+) fd_err ([0-9.e+-]+)', r.stdout)
    assert m, r.stdout
    cost0, cost1, err = (float(g) for g in m.groups())
    assert cost1 < cost0 and err <= 1e-5, r.stdout
