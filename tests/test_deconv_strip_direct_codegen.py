"""CPU (needs only hipcc, which cross-compiles gfx950 without a GPU): the generated code of the deconv_strip_kernel<4, SPLIT>
instantiations that carry the direct-store epilogue (SPLIT 4 / 5, the three-piece bf16 modes: deconv4's unsplit launch with its fused
BatchNorm records).  The epilogue is a runtime branch (ConvDesc::ksplit == 1) inside the existing instantiations -- no new kernel names --
so what is pinned here is that the branch costs them nothing they cannot afford:

* no VGPR or SGPR spills and no scratch memory;
* static LDS <= 80 KB and <= 256 VGPRs: two workgroups per CU, as before (the float64 chains re-use the A strip's LDS);
* the float64 statistics are in SPLIT 4 / 5 only: the fp32 and f16 instantiations (fp32: 168-VGPR budget, three workgroups per CU)
  contain no float64 arithmetic at all."""
import os
import re
import subprocess

import pytest

from relativepose_amd import build as B

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    d = tmp_path_factory.mktemp("dstripdirectasm")
    s = d / "scnet.s"
    extra = dict(B.SOURCES)["scnet.hip"]
    subprocess.check_call([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", *extra, "--cuda-device-only", "-S", "-o", str(s),
                           os.path.join(B.CSRC, "scnet.hip")], stderr=subprocess.DEVNULL)
    txt = s.read_text()
    s.unlink()
    meta = {}
    # amdhsa metadata: .group_segment_fixed_size precedes the kernel-level .name (the one directly followed by .private_segment_fixed_size)
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n(\s+\.private_segment_fixed_size:.*?)\.wavefront_size", txt, re.S):
        r = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", m.group(3))}
        r["group_segment_fixed_size"] = int(m.group(1))
        meta[m.group(2)] = r
    body = {}
    for name in meta:
        if "deconv_strip_kernelILi" not in name:
            continue
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M)     # the function's label to its end label
        assert m, name
        body[name] = m.group(1)
    return meta, body


def _one(names, part):
    hits = [n for n in names if part in n]
    assert len(hits) == 1, (part, hits)
    return hits[0]


@pytest.mark.parametrize("sp", [4, 5])
def test_direct_epilogue_instantiations_fit_two_per_cu(listing, sp):
    meta, body = listing
    name = _one(meta, f"deconv_strip_kernelILi4ELi{sp}EE")
    r = meta[name]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (sp, r)
    assert r["group_segment_fixed_size"] <= 80 * 1024, (sp, r)
    assert r["vgpr_count"] <= 256, (sp, r)
    assert "scratch_" not in body[name], sp


@pytest.mark.parametrize("sp", [4, 5])
def test_direct_epilogue_is_in_the_three_piece_instantiations(listing, sp):
    meta, body = listing
    name = _one(meta, f"deconv_strip_kernelILi4ELi{sp}EE")
    # the float64 chains of the BatchNorm records are there
    assert re.search(r"^\s+v_(add|fma)_f64", body[name], re.M), sp
    assert re.search(r"^\s+v_cvt_f64_f32", body[name], re.M), sp


@pytest.mark.parametrize("sp", [0, 2, 3])
def test_other_instantiations_carry_no_statistics_code(listing, sp):
    meta, body = listing
    name = _one(meta, f"deconv_strip_kernelILi4ELi{sp}EE")
    assert not re.search(r"^\s+v_\w*f64", body[name], re.M), sp
