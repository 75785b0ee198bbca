"""Build librelpose_hip.so (gfx950) in-tree with hipcc.  No torch involved: the
library is a plain C-ABI shared object (include/relpose.h)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librelpose_hip.so")
ARCH = "gfx950"

# (source, extra flags).  matcher/geometry must round like numpy: no FMA contraction.
SOURCES = [
    ("matcher.hip", ["-ffp-contract=off"]),
    ("affinity.hip", ["-ffp-contract=off"]),
    ("geometry.hip", ["-ffp-contract=off"]),
    ("keypoints.hip", ["-ffp-contract=off"]),
    ("sift.hip", ["-ffp-contract=off"]),          # the detector and its numpy model must round alike
    ("fgr.hip", ["-ffp-contract=off"]),           # FPFH + FGR: bins and matches must agree with tests/fgr_model.py bit for bit
    ("ransac.hip", ["-ffp-contract=off"]),        # RANSAC: draws, Horn and the validation sums must agree with tests/ransac_model.py
    ("cicp.hip", ["-ffp-contract=off"]),          # coloured ICP: voxels, correspondences and the reductions must agree with tests/cicp_model.py
    ("descriptor.hip", ["-ffp-contract=off"]),    # descriptor evaluation: the thresholds and counts must agree with tests/descriptor_model.py
    ("siftdesc.hip", ["-ffp-contract=off"]),      # SIFT descriptors: the base blur must agree with tests/sift_model.py bit for bit
    ("completion.hip", ["-ffp-contract=off"]),    # completion losses: the fp32 terms must agree with tests/completion_model.py
    ("normals.hip", ["-ffp-contract=off"]),       # depth normals: count and the nine moments must agree with tests/normals_model.py bit for bit
    ("panorama.hip", ["-ffp-contract=off"]),      # frames to panorama: the f64 geometry and the f32 gate must agree with tests/panorama_model.py bit for bit
    ("overlap.hip", ["-ffp-contract=off"]),        # overlap statistics: hits and the closest-pair distance must agree with tests/overlap_model.py bit for bit
    ("visibility.hip", ["-ffp-contract=off"]),     # visibility consistency: classes and margins must agree with tests/visibility_model.py bit for bit
    ("tsdf.hip", ["-ffp-contract=off"]),           # TSDF fusion: the integer volume and the surface must agree with tests/tsdf_model.py bit for bit
    ("mesh.hip", ["-ffp-contract=off"]),           # marching cubes: the vertices are tsdf.hip's surface bit for bit (tsdf_surf.h), the triangles tests/mesh_model.py's
    ("meshcc.hip", ["-ffp-contract=off"]),         # mesh components: labels, integer sums and the triangle areas must agree with tests/components_model.py bit for bit
    ("meshdecim.hip", ["-ffp-contract=off"]),      # mesh decimation: cells, integer sums and the means must agree with tests/decimate_model.py bit for bit
    ("tsdfalign.hip", ["-ffp-contract=off"]),      # TSDF alignment: the integer sums and the stepped poses must agree with tests/align_model.py bit for bit
    ("tsdfrender.hip", ["-ffp-contract=off"]),     # TSDF rendering: every output must agree with tests/render_model.py bit for bit
    ("posesync.hip", ["-ffp-contract=off"]),       # pose synchronisation: every f64 operation rounds as tests/sync_model.py states it
    ("scnet.hip", []),
]


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + \
              [os.path.join(os.path.dirname(HERE), "include", "relpose.h")]
    for src, extra in SOURCES:
        s = os.path.join(CSRC, src)
        if not os.path.exists(s):
            continue
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        if force or _newer(s, o) or any(_newer(h, o) for h in headers):
            cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-c", s, "-o", o] + extra + \
                  os.environ.get("RELPOSE_HIPCC_FLAGS", "").split()       # extra flags for an A/B build (tools/build_variant.py)
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        objs.append(o)
    if force or any(_newer(o, LIB) for o in objs):
        cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
