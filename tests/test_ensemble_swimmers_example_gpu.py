"""examples/ensemble_swimmers.py runs to completion on the GPU (own process, as a user would start it), prints one displacement
per height and cycle, and keeps every joint as closed as the single-context example does at the same dt."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE_CONTEXT_GAP = 2.9e-4      # the largest gap examples/three_link_swimmer.py reports at dt = 0.02 (README's row of that example)


def test_the_swimmers_at_every_height_swim_and_stay_jointed():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join("examples", "ensemble_swimmers.py")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out = p.stdout
    print(out)
    assert "nan" not in out.lower()
    moved = re.findall(r"cycle 1 height +([0-9.]+): displacement ([-+0-9.e]+) along", out)
    assert [float(h) for h, _ in moved] == [2.0, 2.5, 3.0, 4.0, 6.0, 10.0]
    assert all(abs(float(d)) > 1e-4 for _, d in moved)           # every swimmer went somewhere
    gaps = re.findall(r"height +([0-9.]+): largest gap over the run ([0-9.e+-]+)", out)
    assert len(gaps) == 6 and all(float(g) < SINGLE_CONTEXT_GAP for _, g in gaps), gaps
