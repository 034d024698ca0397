"""Every code path of the kernels against the oracle, including the ones the default configuration rarely takes:
the literal contour scanner and the mid tier forced on every frame, and another grid size of k_binary."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("case", ["default", "literal", "mid", "groups2"])
def test_variant(case):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_variant_check.py"), case], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "variant ok" in r.stdout
    if case == "literal":
        assert "slow-path frames: 4" in r.stdout
    if case == "mid":
        assert "slow-path frames: 0 mid-tier frames: 4" in r.stdout
