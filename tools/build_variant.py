"""Build relativepose_amd/librelpose_hip_<name>.so from the working tree, with extra compiler flags on every source if any are given:
a second library next to the product one, for A/B comparisons (tools/gpu_evidence.sh ab).  Use it with RELPOSE_LIB_PATH=<that file>.
The sources have no experiment switches of their own; a variant is a source change.
    python tools/build_variant.py cand [-O2 ...]"""
import os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relativepose_amd import build as b
name, flags = sys.argv[1], sys.argv[2:]
objs = []
for src, extra in b.SOURCES:
    o = f"/tmp/{src[:-4]}_{name}.o"
    subprocess.check_call(["/opt/rocm/bin/hipcc", f"--offload-arch={b.ARCH}", "-O3", "-std=c++17", "-fPIC", *extra, *flags, "-c", os.path.join(b.CSRC, src), "-o", o],
                          stderr=subprocess.DEVNULL)
    objs.append(o)
out = os.path.join(b.HERE, f"librelpose_hip_{name}.so")
subprocess.check_call(["/opt/rocm/bin/hipcc", f"--offload-arch={b.ARCH}", "-shared", "-fPIC", "-o", out] + objs)
print(out)
