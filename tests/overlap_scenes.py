"""Shared inputs of the overlap tests (test infrastructure): the three multi-view scenes, their observed clouds through the oracle and the
brute model's results, computed once per process."""
import functools

import numpy as np

import overlap_model as OM
from oracle import geom_oracle as G
from relativepose_amd import synth

SCENES = (("suncg", 32), ("suncg", 48), ("matterport", 48))
SCENE_SEED, SCENE_VIEWS = 7, 6
NO_HIT = {("suncg", 32): 12, ("suncg", 48): 12, ("matterport", 48): 16}        # of the 30 directed queries (k-d tree and brute force agree)


def observed_clouds(depth, ds):
    """depth [M,h,4h] -> (pc [M,P,3] f64, valid [M,P] u8) of the observed block in relpose_depth2pc's layout (invalid points are zeros)."""
    M, h = depth.shape[:2]
    pcs, va = [], []
    for v in range(M):
        if ds == "scannet":
            y0, y1, x0, x1 = G.kinect_box(h)
            crop = depth[v, y0:y1, x0:x1]
        else:
            crop = depth[v, :, h:2 * h]
        p, m = G.depth2pc(crop, ds)
        full = np.zeros((m.size, 3))
        full[m] = p
        pcs.append(full)
        va.append(m)
    return np.stack(pcs), np.stack(va).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene(ds, h):
    """-> dict: the rendered scene, pc, valid, the 30 directed queries (qc, rc, T) and the brute model's result `want` (read-only)."""
    sc = synth.render_scene(SCENE_SEED, SCENE_VIEWS, ds, h)
    pc, valid = observed_clouds(sc["depth"], ds)
    qc, rc, T = OM.matrix_queries(sc["R"])
    return {"scene": sc, "pc": pc, "valid": valid, "qc": qc, "rc": rc, "T": T, "want": OM.overlap(pc, valid, qc, rc, T, model="brute")}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(got, want, keys=("hits", "hit", "nn_min", "n_valid")):
    """bitwise comparison of two result dicts; returns the list of keys that differ"""
    bad = []
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        eq = np.array_equal(bits(a), bits(b)) if b.dtype == np.float64 else np.array_equal(a, b)
        if not eq:
            bad.append(k)
    return bad


def kinect_pair(h, seed=3):
    """A scannet pair whose poses are a small motion apart (the kinect crop of both views sees much of the same wall):
    -> (pc [2,P,3], valid [2,P], qc, rc, T [2,4,4]) with the two directed queries; P = the kinect box of height h."""
    rs = np.random.RandomState(seed)
    half = np.array([2.5, 2.0, 3.0])
    p0 = synth.random_rigid(rs, 0.3, 0.3)
    p1 = np.matmul(p0, synth.random_rigid(rs, 0.12, 0.15))
    _, _, depth, _ = synth.render_room(rs, "scannet", 0.01, h, poses=[p0, p1], half=half)
    pc, valid = observed_clouds(depth, "scannet")
    R = [np.linalg.inv(p0), np.linalg.inv(p1)]
    T = np.stack([np.matmul(R[1], np.linalg.inv(R[0])), np.matmul(R[0], np.linalg.inv(R[1]))])
    return pc, valid, np.array([0, 1], np.int32), np.array([1, 0], np.int32), T
