"""CPU (needs only hipcc, which cross-compiles gfx950 without a GPU): the generated code of deconv_strip_kernel<4, SPLIT>, the phase
strip kernel of SCNet's deconv4 / deconv5, and of the kernel it was modelled on.

* every instantiation (SPLIT 0, 2, 3, 4, 5) compiles without VGPR spills and without scratch memory;
* SPLIT 0 (fp32 products) stays at <= 168 VGPRs: three workgroups per CU, as conv_s2_strip_kernel<4, 0>;
* SPLIT >= 4 (three-piece bf16 rows) keeps its static LDS at <= 80 KB: two workgroups per CU;
* conv_s2_strip_kernel<4, 0> is untouched by its sibling: 164 VGPRs, no spills, 50688 bytes of LDS -- the figures of a build of the
  parent commit (the commit before deconv_strip_kernel existed), read from that build's assembly listing."""
import os
import re
import subprocess

import pytest

from relativepose_amd import build as B

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

PARENT_CONV_STRIP_F32 = {"vgpr_count": 164, "vgpr_spill_count": 0, "private_segment_fixed_size": 0, "group_segment_fixed_size": 50688}


@pytest.fixture(scope="module")
def scnet_kernels(tmp_path_factory):
    d = tmp_path_factory.mktemp("dstripasm")
    s = d / "scnet.s"
    extra = dict(B.SOURCES)["scnet.hip"]
    subprocess.check_call([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", *extra, "--cuda-device-only", "-S", "-o", str(s),
                           os.path.join(B.CSRC, "scnet.hip")], stderr=subprocess.DEVNULL)
    txt = s.read_text()
    s.unlink()
    res = {}
    # amdhsa metadata: .group_segment_fixed_size precedes the kernel-level .name (the one directly followed by .private_segment_fixed_size;
    # arguments may carry .name entries too), the register figures follow it
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n(\s+\.private_segment_fixed_size:.*?)\.wavefront_size", txt, re.S):
        r = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", m.group(3))}
        r["group_segment_fixed_size"] = int(m.group(1))
        res[m.group(2)] = r
    return res


def _one(k, part):
    hits = [n for n in k if part in n]
    assert len(hits) == 1, (part, hits)
    return k[hits[0]]


def test_deconv_strip_kernel_resources(scnet_kernels):
    k = scnet_kernels
    names = sorted(n for n in k if "deconv_strip_kernelILi" in n)
    assert len(names) == 5, names
    for sp in (0, 2, 3, 4, 5):
        r = _one(k, f"deconv_strip_kernelILi4ELi{sp}EE")
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (sp, r)
        if sp == 0:
            assert r["vgpr_count"] <= 168, r                       # 512 / 168 = 3 waves per SIMD: three 4-wave workgroups per CU
            assert 3 * r["group_segment_fixed_size"] <= 160 * 1024, r
        if sp >= 4:
            assert r["group_segment_fixed_size"] <= 80 * 1024, (sp, r)
            assert r["vgpr_count"] <= 256, (sp, r)


def test_conv_s2_strip_kernel_is_what_the_parent_built(scnet_kernels):
    r = _one(scnet_kernels, "conv_s2_strip_kernelILi4ELi0EE")
    assert {f: r[f] for f in PARENT_CONV_STRIP_F32} == PARENT_CONV_STRIP_F32, r
