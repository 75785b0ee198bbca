"""CPU: conv1's tile -> occupancy-block geometry (csrc/conv1_zero_geom.h, shared by conv1_mfma_kernel) checked exhaustively by a
stand-alone host program under AddressSanitizer and UBSan (tests/host/conv1_zero_geom_main.cpp), and against the numpy census."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def host_compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.skipif(host_compiler() is None, reason="no host C++ compiler")
def test_geometry_program_under_sanitizers(tmp_path):
    exe = tmp_path / "conv1_zero_geom"
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "relativepose_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "host", "conv1_zero_geom_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "conv1_zero_geom ok: 7056 units" in r.stdout


def test_census_model_agrees_with_a_pixel_level_count():
    """tools/conv1_zero_census.unit_zero (block words) never calls a unit zero whose 3 x 3 neighbourhood holds a non-zero value, and is
    conservative by whole blocks only."""
    import conv1_zero_census as CZ
    import zero_tiles_model as Z
    rs = np.random.RandomState(7)
    x0 = np.zeros((2, 224, 224, 16), np.float32)
    for _ in range(12):
        x0[rs.randint(2), rs.randint(224), rs.randint(224), rs.randint(16)] = rs.choice([1.0, -0.0, 1e-40])
    x0[1, 100:140, 60:200, 8:16] = 1.0
    occ, _ = Z.occupancy(x0)
    z = CZ.unit_zero(occ, CZ.nonfinite_rows(x0))
    nz = (x0.view(np.uint32) & 0x7fffffff) != 0
    for q in range(6):
        s = nz[..., Z.stream_channels(q)].any(-1)
        for by in range(28):
            for tx in range(7):
                field = s[:, max(8 * by - 1, 0):8 * by + 9, max(32 * tx - 1, 0):32 * tx + 33].any((1, 2))
                wide = s[:, max(8 * by - 8, 0):8 * by + 16, max(32 * tx - 8, 0):32 * tx + 40].any((1, 2))
                assert not (z[:, q, by, tx] & field).any()
                assert np.array_equal(z[:, q, by, tx], ~wide)
