"""CPU: the contract of relpose_tsdf_render checked on its numpy model: the vectorised form (clip and skip) against the
plain per-ray loop, skip against no skip, a batch against its members, the accuracy against the analytic closed rooms (measured with the
model and pinned), the hand-built edge volume, and csrc/tsdfrender_math.h -- the very text the kernels run -- compiled for the host and
compared with the model bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_scenes as AS
import render_model as RM
import render_scenes as RS
import tsdf_scenes as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Measured with the model: median and p90 of |rendered - analytic depth| in voxels, coverage, median normal angle in degrees
MEASURED = {("closed16", "all"): (0.03807, 0.23079, 0.91634, 4.6429), ("closed32", "all"): (0.03139, 0.16614, 0.97961, 4.3479),
            ("closed16", "loo"): (0.03699, 0.24090, 0.85026, 5.0117), ("closed32", "loo"): (0.03501, 0.18704, 0.89465, 4.8048)}
MARGIN = 1.25                                       # test_align_cpu.py's margin for model-measured quantities


def loops_of(cs, v, pixels=None):
    s = int(cs["scene_of_view"][v])
    st = cs["state"]
    return RM.render_view_loops(st["tsdf_sum"][s], st["weight"][s], st["color_sum"][s], cs["origin"][s], cs["voxel"], cs["pose"][v], cs["ds"], cs["h"],
                                cs["d_min"], cs["step"], cs["n_steps"], cs["min_weight"], pixels)


# ---------------------------------------------------------------------------------------------- 1. the two forms
def test_vectorised_form_equals_the_plain_loop():
    cs = RS.case("closed16")
    m = RS.room_model("closed16", False)
    for v in range(len(cs["pose"])):
        L = loops_of(cs, v)
        assert [k for k in RM.KEYS if not TS.bits_equal(L[k], m[k][v])] == [], v
    cs = RS.case("closed32", [1])                                   # every 5th pixel of one view: the loop is slow
    m = RS.model_of(cs, skip=False)
    pix = list(range(0, 4 * 32 * 32, 5))
    L = loops_of(cs, 0, pix)
    for k in RM.KEYS:
        assert TS.bits_equal(L[k].reshape(L[k].shape[:-2] + (-1,))[..., pix], m[k][0].reshape(m[k][0].shape[:-2] + (-1,))[..., pix]), k
    e = RS.edge_case()
    m = RS.model_of(e, skip=False)
    for v in range(len(e["pose"])):
        L = loops_of(e, v)
        assert [k for k in RM.KEYS if not TS.bits_equal(L[k], m[k][v])] == [], v


def test_clip_is_conservative():
    """the clipped march gives what the unclipped one gives, n_evaluated included, from inside, from outside and from 100 m away"""
    for cs in (RS.case("closed16"), RS.batch(), RS.edge_case(), RS.edge_case("scannet")):
        for skip in (False, True):
            assert TS.differ(RS.model_of(cs, skip=skip), RS.model_of(cs, skip=skip, clip=False), RM.KEYS) == []
    b = RS.batch()
    W = AS.AM.inverse(b["pose"][2])
    k0, k1 = RM.clip_range(W, RM.rays(16, "suncg"), b["origin"][0], b["dims"], b["voxel"], 0.0, b["step"], b["n_steps"])
    assert (k0 > k1).all()                                           # 100 m away: no ray reaches the box within d_max


# ---------------------------------------------------------------------------------------------- 2. skipping
def test_skip_changes_nothing_but_the_count():
    for name in ("closed16", "closed32"):
        a, b = RS.room_model(name, True), RS.room_model(name, False)
        assert TS.differ(a, b, RM.IMAGE_KEYS) == []
        assert (a["n_evaluated"] <= b["n_evaluated"]).all()
    # closed32 (38 x 26 x 46 voxels, 5 x 4 x 6 bricks) has bricks in the room's interior: strictly fewer evaluations
    a, b = RS.room_model("closed32", True), RS.room_model("closed32", False)
    assert int(a["n_evaluated"].sum()) < int(b["n_evaluated"].sum())
    # closed16 is 22 x 16 x 26 voxels: 15 cells in y are two bricks, each holding the floor or the ceiling, so every one of its 24 bricks is
    # flagged and skip can evaluate no fewer samples there: the counts are equal
    st = RS.full_state("closed16")
    assert RM.brick_flags(st["tsdf_sum"][0], st["weight"][0]).all()
    assert np.array_equal(RS.room_model("closed16", True)["n_evaluated"], RS.room_model("closed16", False)["n_evaluated"])
    e = RS.edge_case()
    assert TS.differ(RS.model_of(e, skip=True), RS.model_of(e, skip=False), RM.IMAGE_KEYS) == []


def test_an_unflagged_cell_cannot_give_a_negative_value():
    """the step of the proof that is about rounding: the lerp of non-negative corners with 0 <= f < 1 is never negative"""
    rs = np.random.RandomState(0)
    t = rs.randint(0, 5, (200000, 8)).astype(np.float64) * rs.choice([2.0 ** -15, 1.0 / 3.0, 1e-300, 0.999], (200000, 1))
    f = rs.choice([0.0, 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53, 1.0 / 3.0], (200000, 3))
    f[::2] = rs.uniform(0, 1, (100000, 3))
    assert (RM._lerp8(t, f) >= 0.0).all()


# ---------------------------------------------------------------------------------------------- 3. the batch
def test_a_batch_equals_its_members():
    b = RS.batch()
    m = RS.model_of(b)
    for v in range(len(b["pose"])):
        one = RS.model_of(RS.batch_member(v))
        for k in RM.KEYS:
            assert TS.bits_equal(one[k][0], m[k][v]), (v, k)
    assert (m["cls"][2] == RM.MISS).all() and (m["n_evaluated"][2] == 0).all() and not m["depth"][2].any()      # 100 m away
    assert TS.bits_equal(m["depth"][0], RS.room_model("closed16")["depth"][0])
    assert not TS.bits_equal(m["depth"][0], m["depth"][3])           # the same pose against another volume


# ---------------------------------------------------------------------------------------------- 4. accuracy
@pytest.mark.parametrize("name,which", sorted(MEASURED))
def test_rendered_views_match_their_analytic_inputs(name, which):
    n = len(AS.scene(name)["R"])
    if which == "all":
        out = RS.room_model(name)
    else:
        views = [RS.loo_model(name, v) for v in range(n)]
        out = {k: np.concatenate([w[k] for w in views]) for k in ("depth", "cls", "normal")}
    med, p90, cov, ang = RS.accuracy(name, out, list(range(n)))
    print(f"render accuracy {name} {which}: median {med:.5f} p90 {p90:.5f} voxels, coverage {cov:.5f}, normal angle {ang:.4f} deg")
    m = MEASURED[(name, which)]
    assert med <= m[0] * MARGIN and p90 <= m[1] * MARGIN and cov >= m[2] / MARGIN and ang <= m[3] * MARGIN
    hit = out["cls"] == RM.HIT
    assert ((out["depth"] > 0) == hit).all() and not out["normal"][~np.repeat(hit[:, None], 3, 1)].any()     # 0 is "no data"
    nn = np.sqrt((out["normal"].astype(np.float64) ** 2).sum(1))[hit]
    assert np.abs(nn - 1.0).max() < 1e-6


# ---------------------------------------------------------------------------------------------- 5. the edge volume
@pytest.mark.parametrize("skip", [False, True])
def test_edge_volume_gets_what_the_contract_gives(skip):
    e = RS.edge_case()
    m = RS.model_of(e, skip=skip)
    at = lambda key, name: m[key][RS.EDGE_AXIS[name]]
    # t_k = 0 exactly ends nothing at the pair (1, 2); t_{k-1} = 0 gives s = 0 at the pair (2, 3): the depth is d_2, u there is an integer
    assert at("cls", "hit_s0") == RM.HIT and at("depth", "hit_s0") == np.float32(0.5)
    # the last cell (u_z = 3 and 3.5) is evaluated, one past it (u_z = 4) is not
    assert at("cls", "last_cell") == RM.MISS and (skip or at("n_evaluated", "last_cell") == 2)
    # positive, four invalid samples around a voxel of weight min_weight - 1, negative: no surface is invented
    assert at("cls", "no_bridge") == RM.MISS and at("depth", "no_bridge") == 0 and (skip or at("n_evaluated", "no_bridge") == 8)
    # the camera inside a solid: the first valid sample is negative, the pixel is a back face without data
    assert at("cls", "back_face") == RM.BACK and at("depth", "back_face") == 0
    v, r, c = RS.EDGE_AXIS["back_face"]
    assert not m["normal"][v, :, r, c].any() and not m["color"][v, :, r, c].any()
    for v in (3, 4):                                                 # NaN and inf in a pose
        assert (m["cls"][v] == RM.MISS).all() and (m["n_evaluated"][v] == 0).all()
        assert not m["depth"][v].any() and not m["normal"][v].any() and not m["color"][v].any()
    one = RS.model_of(e, skip=skip, n_steps=1)                       # n_steps = 1: no pair
    assert (one["cls"] == RM.MISS).all() and not one["depth"].any() and one["n_evaluated"].max() <= 1
    flat = RS.model_of(RS.flat_case(), skip=skip)                    # a dimension of 1: no cells
    assert (flat["cls"] == RM.MISS).all() and not flat["n_evaluated"].any() and not flat["depth"].any()
    lift = RS.model_of(e, skip=skip, min_weight=1)                   # with min_weight 1 the voxel is known and the ray hits
    assert lift["cls"][RS.EDGE_AXIS["no_bridge"]] == RM.HIT


def test_face_order_of_the_datasets():
    a, b = RS.model_of(RS.edge_case("suncg")), RS.model_of(RS.edge_case("scannet"))
    h = 4
    for s in range(4):                                               # scannet's slot s shows suncg's face (s + 3) & 3
        f = (s + 3) & 3
        assert TS.bits_equal(b["depth"][:, :, s * h:(s + 1) * h], a["depth"][:, :, f * h:(f + 1) * h])
    assert TS.bits_equal(RS.model_of(RS.edge_case("matterport"))["depth"], b["depth"])


# ---------------------------------------------------------------------------------------------- 6. the kernels' text on the host
SHIM = r'''
#include "tsdfrender_math.h"
extern "C" void t_render_view(const int* tsdf, const int* weight, const unsigned* color, const double* origin, double voxel, int nx, int ny, int nz,
                              int min_weight, const unsigned char* flags, const double* T, int suncg, int h, double d_min, double step, int n_steps,
                              int clip, float* depth, unsigned char* cls, float* normal, float* out_color, int* nev) {
    RenderVolume g;
    g.nx = nx; g.ny = ny; g.nz = nz; g.min_weight = min_weight;
    g.bx = render_bricks(nx); g.by = render_bricks(ny); g.bz = render_bricks(nz);
    g.nvox = (size_t)nx * ny * nz; g.voxel = voxel;
    for (int a = 0; a < 3; ++a) g.origin[a] = origin[a];
    g.tsdf = tsdf; g.weight = weight; g.color = color; g.flags = flags;
    double W[12];
    align_inverse(T, W);
    const int npix = 4 * h * h;
    for (int pix = 0; pix < npix; ++pix) {
        double dir[3];
        render_ray(suncg != 0, h, pix / (4 * h), pix % (4 * h), dir);
        int k0 = 0, k1 = n_steps - 1;
        if (clip) render_clip(g, W, dir, d_min, step, n_steps, k0, k1);
        RenderPixel o;
        render_march(g, W, dir, d_min, step, k0, k1, true, color != nullptr, o);
        depth[pix] = o.depth; cls[pix] = (unsigned char)o.cls; nev[pix] = o.n_evaluated;
        for (int c = 0; c < 3; ++c) { normal[c * npix + pix] = o.normal[c]; if (color) out_color[c * npix + pix] = o.color[c]; }
    }
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostrender")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "shim.so"
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I",
                           os.path.join(ROOT, "relativepose_amd", "csrc"), str(src), "-o", str(so)])
    return C.CDLL(str(so))


def host_render(shim, cs, skip, clip=True, color=True):
    st = cs["state"]
    h, V = cs["h"], len(cs["pose"])
    nx, ny, nz = cs["dims"]
    out = {"depth": np.zeros((V, h, 4 * h), np.float32), "cls": np.zeros((V, h, 4 * h), np.uint8), "normal": np.zeros((V, 3, h, 4 * h), np.float32),
           "color": np.zeros((V, 3, h, 4 * h), np.float32), "n_evaluated": np.zeros((V, h, 4 * h), np.int32)}
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for v in range(V):
        s = int(cs["scene_of_view"][v])
        ts, wt, col = (np.ascontiguousarray(st[k][s]) for k in RS.STATE_KEYS)
        flags = np.ascontiguousarray(RM.brick_flags(ts, wt, cs["min_weight"]).astype(np.uint8).reshape(-1)) if skip else None
        if flags is not None and flags.size == 0:
            flags = np.zeros(1, np.uint8)
        org, T = np.ascontiguousarray(cs["origin"][s], dtype=np.float64), np.ascontiguousarray(cs["pose"][v], dtype=np.float64)
        o = [np.ascontiguousarray(out[k][v]) for k in RM.KEYS]
        shim.t_render_view(p(ts), p(wt), p(col) if color else None, p(org), C.c_double(cs["voxel"]), nx, ny, nz, cs["min_weight"], None if flags is None else p(flags), p(T),
                           int("suncg" in cs["ds"]), h, C.c_double(cs["d_min"]), C.c_double(cs["step"]), cs["n_steps"], int(clip), *[p(a) for a in o])
        for k, a in zip(RM.KEYS, o):
            out[k][v] = a
    return out


@pytest.mark.parametrize("skip", [False, True])
def test_host_build_of_the_kernel_text_matches_the_model_bitwise(shim, skip):
    for cs in (RS.case("closed16"), RS.case("closed32", [2]), RS.case("scannet16", [1]), RS.batch(), RS.edge_case(), RS.edge_case("scannet"),
               RS.flat_case()):
        assert TS.differ(host_render(shim, cs, skip), RS.model_of(cs, skip=skip), RM.KEYS) == []
    e = RS.edge_case()
    assert TS.differ(host_render(shim, e, skip, clip=False), RS.model_of(e, skip=skip), RM.KEYS) == []
    bare = host_render(shim, RS.batch(), skip, color=False)           # without color_sum nothing is read through the NULL pointer
    assert TS.differ(bare, RS.model_of(RS.batch(), skip=skip), ("depth", "cls", "normal", "n_evaluated")) == [] and not bare["color"].any()
