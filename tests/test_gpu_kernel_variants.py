"""tail_kernel reads D^-1 either through one-byte codes (default) or from the vector (MGAMD_NO_DINV_CODES=1), and the level
transfers run fused into the 17^3 brick kernel (default) or as separate kernels (MGAMD_NO_FUSED_TRANSFER=1).  Every other GPU
test runs the defaults; here the alternatives are checked against them on meshes with several 17^3 bricks or many single cells
(the switches are read when the library is loaded, hence child processes)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("quadrant", 7, 4), ("hypercube", 8, 1), ("hypercube", 4, 2)]  # the first two: several bricks per persistent workgroup


def run(geo, L, p, out, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    subprocess.run([sys.executable, os.path.join(HERE, "_vcycle_dump.py"), geo, str(L), str(p), out], check=True, env=env, timeout=600)
    return np.load(out)


@pytest.mark.parametrize("geo,L,p", CASES)
def test_alternative_kernel_paths_agree(tmp_path, geo, L, p):
    ref = run(geo, L, p, str(tmp_path / "default.npz"), {})
    assert any(g[1] > 1 and p * g[0] + 1 == 17 for g in ref["groups"]), "the case must contain several 17^3-lattice bricks"
    alt = run(geo, L, p, str(tmp_path / "alt.npz"), {"MGAMD_NO_DINV_CODES": "1"})
    for key in ("ax", "step", "vcycle"):
        a, b = ref[key], alt[key]
        assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(a), key


@pytest.mark.parametrize("geo,L,p", [("quadrant", 6, 4), ("annulus", 6, 2), ("quadrant", 5, 3)])
def test_round3_kernel_paths_agree(tmp_path, geo, L, p):
    """hanging-node meshes with many single cells (and, at p = 4, 17^3 bricks with fused transfers): separate transfer kernels
    give the defaults' results to rounding"""
    ref = run(geo, L, p, str(tmp_path / "default.npz"), {})
    assert any(g[0] == 1 and g[1] > 8 for g in ref["groups"]), "the case must contain single-cell slots"
    alt = run(geo, L, p, str(tmp_path / "alt.npz"), {"MGAMD_NO_FUSED_TRANSFER": "1"})
    for key in ("ax", "step", "vcycle"):
        a, b = ref[key], alt[key]
        assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(a), key

