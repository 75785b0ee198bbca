"""CPU codegen (hipcc only): taking the patch index from the zero-tile list costs conv_s2_tile_kernel nothing.  Every instantiation has no
spills, and its VGPR count and LDS bytes are not above the parent commit's build, whose figures -- read from that build's listing -- are
recorded in tests/golden/zero_tiles_parent_codegen.json.

Parent figures of note: the f16x3 conv2 instantiation <2, 2, 16, false, 2> spilled 4 registers (20 bytes of scratch) at 168 VGPRs in
the parent.  That instantiation alone now recomputes the index and edge flags of its halo slots 8 and 9 from the thread index where they
are used instead of keeping them (same addresses, same masks, same bits): 168 VGPRs, no spill; the other nine are untouched."""
import json
import os
import re
import subprocess

import pytest

from relativepose_amd import build as B

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
PARENT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zero_tiles_parent_codegen.json")))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    s = tmp_path_factory.mktemp("ztasm") / "scnet.s"
    extra = dict(B.SOURCES)["scnet.hip"]
    subprocess.check_call([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", *extra, "--cuda-device-only", "-S", "-o", str(s),
                           os.path.join(B.CSRC, "scnet.hip")], stderr=subprocess.DEVNULL)
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+).*?"
                         r"\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", s.read_text(), re.S):
        k = re.search(r"conv_s2_tile_kernel(I\w+?E)EvPK", m.group(2))
        if k:
            res[k.group(1)] = {"lds_bytes": int(m.group(1)), "private_bytes": int(m.group(3)), "vgpr_count": int(m.group(4)),
                               "vgpr_spill_count": int(m.group(5))}
    return res


def test_every_instantiation_is_there(kernels):
    assert sorted(kernels) == sorted(PARENT) and len(PARENT) == 10


@pytest.mark.parametrize("inst", sorted(PARENT))
def test_no_spills(kernels, inst):
    print(inst, kernels[inst], "parent", PARENT[inst])
    assert kernels[inst]["vgpr_spill_count"] == 0 and kernels[inst]["private_bytes"] == 0, (inst, kernels[inst])


@pytest.mark.parametrize("inst", sorted(PARENT))
def test_registers_and_lds_not_above_the_parent(kernels, inst):
    print(inst, kernels[inst], "parent", PARENT[inst])
    assert kernels[inst]["vgpr_count"] <= PARENT[inst]["vgpr_count"], (inst, kernels[inst], PARENT[inst])
    assert kernels[inst]["lds_bytes"] <= PARENT[inst]["lds_bytes"], (inst, kernels[inst], PARENT[inst])
    assert kernels[inst]["vgpr_spill_count"] <= PARENT[inst]["vgpr_spill_count"], (inst, kernels[inst], PARENT[inst])
