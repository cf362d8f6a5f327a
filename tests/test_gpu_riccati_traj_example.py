"""examples/learn_noise_through_ltv_kalman.py, run as a user would run it, in a fresh process, for a handful of iterations on a small batch:
the closed-loop loss falls and the noise scale moves from the learner's first guess towards the one the recorded filter was designed for.
The full run is the example's own business; its closing line is what is read here."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(120)
def test_learning_the_noise_scale_through_the_time_varying_filter():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'learn_noise_through_ltv_kalman.py'), '--batch', '8', '--steps', '9', '--iters', '3'],
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r'LTV_KALMAN_OK loss0 ([0-9.e+-]+) loss1 ([0-9.e+-]+) q ([0-9.e+-]+)', r.stdout)
    assert m, r.stdout
    loss0, loss1, q = (float(g) for g in m.groups())
    assert loss1 < loss0 and q < 0.02, r.stdout
