"""CPU: the SIFT detection contract's numpy model (tests/sift_model.py) and the C ABI of the HIP detector (include/relpose.h)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sift_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blob_image(h, w, centres, s=2.5, amp=180.0, base=40.0, signs=None):
    """uint8 [h, w]: flat `base` plus Gaussian blobs of std `s` px centred at (x, y) in pixel-index coordinates."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), base)
    for k, (cx, cy) in enumerate(centres):
        img += (1 if signs is None else signs[k]) * amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# the contract's output frame: pt = c * 2^o / 2 on the half-pixel-centred x2 image puts the centre of source pixel i at i + 1/4
FRAME = 0.25
BLOBS = [(40.1, 40.3), (100.2, 50.35), (60.4, 110.15), (120.3, 120.2), (30.3, 125.1)]


def test_model_finds_planted_blobs():
    img = blob_image(160, 160, BLOBS, amp=100.0, base=128.0, signs=[1, 1, -1, 1, -1])
    r = M.detect(img[None])[0]
    for cx, cy in BLOBS:
        d = np.hypot(r["x"] - (cx + FRAME), r["y"] - (cy + FRAME))
        assert d.min() < 0.05, (cx, cy, d.min())


def test_model_flat_image_has_no_keypoints():
    for v in (0, 128, 255):
        assert len(M.detect(np.full((1, 160, 160), v, np.uint8))[0]["x"]) == 0


def test_model_output_order_and_no_duplicates():
    img = blob_image(96, 128, [(30.2, 30.1), (70.3, 60.4), (100.1, 40.2)])
    r = M.detect(img[None])[0]
    a = np.stack([r["x"], r["y"], -r["size"], r["angle"], -r["response"]], 1)
    for i in range(1, len(a)):
        assert tuple(a[i - 1]) <= tuple(a[i])
        assert tuple(a[i - 1, :4]) != tuple(a[i, :4])
    assert ((r["angle"] >= 0) & (r["angle"] < 360)).all()


def test_octave_counts():
    assert M.n_octaves(160, 160) == 6
    assert M.n_octaves(320, 320) == 7
    assert M.n_octaves(480, 640) == 8


def test_tap_tables_follow_the_size_rule():
    sig = M.layer_sigmas()
    assert abs(sig[0] - np.sqrt(1.6 ** 2 - 1.0)) < 1e-12
    k = 2 ** (1 / 3)
    for i in range(1, 6):
        assert abs(sig[i] - 1.6 * k ** (i - 1) * np.sqrt(k * k - 1)) < 1e-12
    assert [M.kernel_size(s) for s in sig] == [11, 11, 13, 17, 21, 27]
    for s in sig:
        t = M.gaussian_taps(s)
        assert t.dtype == np.float32 and len(t) == (int(np.floor(8 * s + 1 + 0.5)) | 1)
        assert np.array_equal(t, t[::-1]) and abs(float(t.astype(np.float64).sum()) - 1) < 1e-6
        assert np.argmax(t) == len(t) // 2


def _header():
    return open(os.path.join(ROOT, "include", "relpose.h")).read()


def test_header_declares_the_sift_symbols():
    h = _header()
    for sym in ("relpose_sift_workspace_bytes", "relpose_sift_detect", "relpose_sift_stage_capacity"):
        assert re.search(rf"\b{sym}\s*\(", h), sym
    assert "typedef struct RelposeSiftArgs" in h and "rputil.py:152-172" in h and ":253-265" in h
    from relativepose_amd import _lib
    assert int(re.search(r"#define RELPOSE_SIFT_OVERFLOW \((-\d+)\)", h).group(1)) == _lib.SIFT_OVERFLOW
    assert int(re.search(r"#define RELPOSE_SIFT_MAX_SIDE (\d+)", h).group(1)) == _lib.SIFT_MAX_SIDE
    from relativepose_amd import build
    assert ("sift.hip", ["-ffp-contract=off"]) in build.SOURCES


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_sift_args_layout_matches_ctypes(tmp_path):
    from relativepose_amd import _lib
    fields = [f for f, _ in _lib.SiftArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "relpose.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(RelposeSiftArgs));\n' +
                   "".join(f'  printf(" %zu", offsetof(RelposeSiftArgs, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.SiftArgs)
    assert got[1:] == [getattr(_lib.SiftArgs, f).offset for f in fields]


def test_workspace_sizes_and_invalid_arguments():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    assert L.relpose_sift_workspace_bytes(64, 160, 160, 4096) > 0
    assert L.relpose_sift_workspace_bytes(64, 480, 640, 8192) > L.relpose_sift_workspace_bytes(64, 160, 160, 8192)
    for bad in ((0, 160, 160, 100), (1, 15, 160, 100), (1, 160, 2049, 100), (1, 160, 160, 0)):
        assert L.relpose_sift_workspace_bytes(*bad) == 0
    assert L.relpose_sift_stage_capacity(100) == 8192 and L.relpose_sift_stage_capacity(5000) == 32768
    a = _lib.SiftArgs()
    a.struct_size = C.sizeof(a)
    assert L.relpose_sift_detect(C.byref(a)) == -1                      # no images / outputs: RELPOSE_EINVAL before touching a device
    assert L.relpose_sift_detect(None) == -1
