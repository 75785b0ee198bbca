"""CPU (needs only hipcc, which cross-compiles gfx950 without a GPU): the generated code of SCNet's two heads kernels.

* heads_kernel<S, POSE> (the streamed kernel, all four instantiations): no VGPR spills, no scratch memory, and the access shape it
  exists for -- 16-byte global loads staged into LDS with 16-byte writes, OUT leaving as 16-byte stores and never as the 8-byte
  row-per-lane stores of the kernel it replaced.
* heads_lanepix_kernel<S, POSE> (the kept lane-per-pixel kernel, the bitwise reference behind RELPOSE_TUNE_HEADS_KERNEL = 1): still
  compiles spill-free, and its mangled name does not contain `heads_kernelILi`, which tests/test_kernel_hygiene.py uses to find the
  product kernel."""
import os
import re
import subprocess

import pytest

from relativepose_amd import build as B

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def scnet_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("headsasm")
    s = d / "scnet.s"
    extra = dict(B.SOURCES)["scnet.hip"]
    subprocess.check_call([HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", *extra, "--cuda-device-only", "-S", "-o", str(s),
                           os.path.join(B.CSRC, "scnet.hip")], stderr=subprocess.DEVNULL)
    txt = s.read_text()
    s.unlink()
    return txt


def _resources(txt):
    res = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(\s+\.private_segment_fixed_size:.*?)\.wavefront_size", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", m.group(2))}
    return res


def _body(txt, name):
    i = txt.index("\n" + name + ":")
    return txt[i:txt.index("s_endpgm", i)]


def test_heads_kernels_resources_and_access_shape(scnet_asm):
    k = _resources(scnet_asm)
    streamed = sorted(n for n in k if "heads_kernelILi" in n)
    lanepix = sorted(n for n in k if "heads_lanepix_kernelILi" in n)
    assert len(streamed) == 4 and len(lanepix) == 4, (streamed, lanepix)
    for s_ in (15, 21):
        for pose in (0, 1):
            assert any(f"heads_kernelILi{s_}ELb{pose}E" in n for n in streamed), (s_, pose)
            assert any(f"heads_lanepix_kernelILi{s_}ELb{pose}E" in n for n in lanepix), (s_, pose)
    for n in streamed:
        assert k[n]["vgpr_spill_count"] == 0 and k[n]["private_segment_fixed_size"] == 0, (n, k[n])
        body = _body(scnet_asm, n)
        assert body.count("global_load_dwordx4") >= 8 * 6 and body.count("ds_write_b128") >= 8 * 6, n       # at least the six line-sets of the pose plan
        assert "global_store_dwordx4" in body and "global_store_dwordx2" not in body and "global_store_dword " not in body, n
        assert body.count("s_barrier") <= 2, n          # one workgroup barrier per path (weights in place); the line-sets are wave-private
    for n in lanepix:
        assert "heads_kernelILi" not in n
        assert k[n]["vgpr_spill_count"] == 0 and k[n]["private_segment_fixed_size"] == 0, (n, k[n])
