"""GPU: relpose_overlap (the grid-based overlap statistics) against the brute numpy model bit for bit, its batch
invariance, the drivers built on it against the unchanged per-pair yardstick util.point_cloud_overlap, and pair mining."""
import ctypes as C
import os

import numpy as np
import pytest

import overlap_model as OM
import overlap_scenes as OS
from cases import GEOM_CASES
from gpu_util import log
from relativepose_amd import synth

pytestmark = pytest.mark.gpu

MD = 0.08


def run(pc, valid, qc, rc, T, max_dist=MD):
    """util.overlap_dev on numpy inputs -> the model's result dict"""
    import torch
    from relativepose_amd import util
    dev = torch.device("cuda:0")
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, dtype=np.uint8)).to(dev)
    hits, nn_min, n_valid, hit = util.overlap_dev(torch.from_numpy(np.ascontiguousarray(pc, dtype=np.float64)).to(dev), v, qc, rc,
                                                  torch.from_numpy(np.ascontiguousarray(T, dtype=np.float64)).to(dev), max_dist, want_hit=True)
    return {"hits": hits.cpu().numpy(), "nn_min": nn_min.cpu().numpy(), "n_valid": n_valid.cpu().numpy(), "hit": hit.cpu().numpy()}


def check(name, pc, valid, qc, rc, T, max_dist=MD):
    """one call against the brute model, bitwise; returns the model's result"""
    want = OM.overlap(pc, valid, qc, rc, T, max_dist)
    got = run(pc, valid, qc, rc, T, max_dist)
    log("overlap_" + name, hits=got["hits"], want_hits=want["hits"], nn_min=got["nn_min"], want_nn_min=want["nn_min"])
    assert OS.same(got, want) == [], (name, got["hits"], want["hits"], got["nn_min"], want["nn_min"])
    return want


EYE = np.eye(4)


@pytest.mark.parametrize("ds,h", OS.SCENES)
def test_scene_queries_match_the_brute_model_bitwise(ds, h):
    s = OS.scene(ds, h)
    got = run(s["pc"], s["valid"], s["qc"], s["rc"], s["T"])
    want = s["want"]
    log("overlap_scene", ds=ds, h=h, hits=got["hits"], want_hits=want["hits"])
    assert OS.same(got, want) == []
    assert int((want["hits"] == 0).sum()) == OS.NO_HIT[(ds, h)]


@pytest.mark.parametrize("h", (32, 48))
def test_kinect_crop_pair_a_small_motion_apart(h):
    """The scannet kinect crop: 12 x 16 = 192 points at h = 32, 18 x 26 = 468 at h = 48 (no multiple of 64, nor of the 256-point tile)."""
    pc, valid, qc, rc, T = OS.kinect_pair(h)
    assert pc.shape[1] == {32: 192, 48: 468}[h]
    want = check("kinect", pc, valid, qc, rc, T)
    assert (want["hits"] > 0).all()                                 # hits in both directions


def _pad(points, P, fill=0.0):
    """points [k,3] -> (pc [P,3], valid [P]) with the k points first"""
    pc = np.full((P, 3), fill)
    pc[:len(points)] = points
    valid = np.zeros(P, np.uint8)
    valid[:len(points)] = 1
    return pc, valid


def test_a_query_at_exactly_max_dist_and_one_ulp_nearer():
    P = 1024
    near = np.nextafter(MD, 0.0)
    q, vq = _pad(np.array([[MD, 0, 0], [near, 0, 0], [0, -MD, 0], [0, 0, -near], [0, near, 0]]), P)
    r, vr = _pad(np.zeros((1, 3)), P)
    want = check("exact", np.stack([q, r]), np.stack([vq, vr]), [0], [1], [EYE])
    assert want["hit"][0, :5].tolist() == [0, 1, 0, 1, 1] and want["hits"][0] == 3 and want["nn_min"][0] == near


def test_queries_just_outside_the_reference_box_on_the_low_side():
    rs = np.random.RandomState(1)
    P = 1536
    ref = rs.uniform(0.0, 1.0, (P, 3))
    ref[:8] = [[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0], [0, 0, 0.7], [0, 0.3, 0], [0.9, 0, 0], [0.02, 0.02, 0.02]]
    q = ref.copy()
    for a in range(3):                                              # below the box on axis a, on two axes, on all three
        q[a * 200:(a + 1) * 200, a] = -rs.uniform(0.0, 0.1, 200)
    q[600:800, :2] = -rs.uniform(0.0, 0.07, (200, 2))
    q[800:1000] = -rs.uniform(0.0, 0.06, (200, 3))
    q[1000:1008] = ref[:8] - [0.0799, 0, 0]
    want = check("low_side", np.stack([q, ref]), None, [0], [1], [EYE])
    outside = (q < 0).any(1)
    assert 0 < want["hit"][0][outside].sum() < outside.sum()        # some of them hit, some do not


def test_three_thousand_reference_points_in_one_cell():
    rs = np.random.RandomState(2)
    P = 3072
    ref, vr = _pad(rs.uniform(0.0, 0.0799, (3000, 3)), P)
    q = rs.uniform(-0.2, 0.28, (P, 3))
    want = check("one_cell", np.stack([q, ref]), np.stack([np.ones(P, np.uint8), vr]), [0, 1], [1, 0], [EYE, EYE])
    assert 0 < want["hits"][0] < P and want["hits"][1] == 3000


def _two_blobs(rs, P, shift):
    a = rs.uniform(-1.0, 1.0, (P, 3)) * [1.0, 0.6, 0.05]             # two thin slabs, like walls
    b = rs.uniform(-1.0, 1.0, (P, 3)) * [1.0, 0.6, 0.05] + shift
    return np.stack([a, b])


def test_every_second_point_invalid():
    rs = np.random.RandomState(3)
    P = 2048
    pc = _two_blobs(rs, P, [0.5, 0.1, 0.02])
    valid = np.zeros((2, P), np.uint8)
    valid[0, ::2] = 1
    valid[1, 1::2] = 1
    want = check("alternate", pc, valid, [0, 1], [1, 0], [EYE, EYE])
    assert (want["n_valid"] == P // 2).all() and (want["hits"] > 0).all() and not want["hit"][0, 1::2].any()


def test_clouds_with_no_valid_point_and_with_one():
    rs = np.random.RandomState(4)
    P = 1024
    full = rs.uniform(-0.5, 0.5, (P, 3))
    one = full.copy()
    pc = np.stack([full, one, rs.uniform(-0.5, 0.5, (P, 3))])
    valid = np.ones((3, P), np.uint8)
    valid[1] = 0
    valid[1, 700] = 1
    valid[2] = 0
    qc, rc = [0, 1, 0, 2, 1, 2, 2], [1, 0, 2, 0, 2, 1, 2]
    want = check("empty_and_one", pc, valid, qc, rc, [EYE] * 7)
    assert want["n_valid"].tolist() == [P, 1, 0]
    assert want["hits"][1] == 1 and want["nn_min"][1] == 0.0 and want["hits"][0] >= 1
    assert (want["hits"][2:] == 0).all() and np.isposinf(want["nn_min"][2:]).all()


def test_grid_edge_cases_match_the_brute_model_bitwise():
    """The shared scan and sort (csrc/cloud_prims.h) where they can go wrong, on clouds whose invalid slots lie between the valid ones
    (fgr_scenes.voxel_edge_clouds at the grid's edge length): no valid point, 40 of them, 2500 (two full rounds of 1024 and a partial one)
    over 13 bits of keys, 2300 over 6 bits, 1500 in one cell (no sort pass: the header's buffer index stays 0)."""
    import fgr_scenes
    edge = MD * OM.EDGE_MARGIN
    names, pc, valid, _ = fgr_scenes.voxel_edge_clouds(edge)
    k = {n: i for i, n in enumerate(names)}

    def bits(name):
        p = pc[k[name]][valid[k[name]] != 0]
        return int(int((np.floor((p.max(0) - p.min(0)) / edge) + 1).prod()) - 1).bit_length()

    assert bits("sparse") == 13 and bits("dense") == 6 and bits("one_cell") == 0 and valid[k["empty"]].sum() == 0
    assert valid[k["few"]].sum() == 40 and valid[k["sparse"]].sum() == 2500
    q = [("sparse", "sparse2"), ("sparse2", "sparse"), ("dense", "sparse"), ("sparse", "dense"), ("few", "sparse"), ("sparse", "few"),
         ("one_cell", "dense"), ("dense", "one_cell"), ("empty", "sparse"), ("sparse", "empty")]
    want = check("grid_edge", pc, valid, [k[a] for a, _ in q], [k[b] for _, b in q], [EYE] * len(q))
    assert want["hits"][0] > 0 and want["hits"][2] > 0 and want["hits"][6] == 1500 and (want["hits"][8:] == 0).all()


def test_a_cloud_against_itself_under_the_identity():
    rs = np.random.RandomState(5)
    P = 1500
    pc = _two_blobs(rs, P, [3.0, 0, 0])
    want = check("self", pc, None, [0, 1], [0, 1], [EYE, EYE])
    assert (want["hits"] == P).all() and (want["nn_min"] == 0.0).all() and want["hit"].all()


def test_both_clouds_offset_by_a_kilometre():
    rs = np.random.RandomState(6)
    P = 1280
    pc = _two_blobs(rs, P, [0.3, 0.2, 0.03]) + [1000.0, -1000.0, 1000.0]
    want = check("offset", pc, None, [0, 1], [1, 0], [EYE, EYE])
    assert (want["hits"] > 0).all()
    T = synth.random_rigid(np.random.RandomState(7), 0.02, 0.05)     # and under a pose that is not the identity
    check("offset_pose", pc, None, [0, 1], [1, 0], [T, np.linalg.inv(T)])


def test_two_clouds_three_metres_apart():
    rs = np.random.RandomState(8)
    P = 2304
    pc = _two_blobs(rs, P, [0.4, -0.3, 3.0])
    want = check("apart", pc, None, [0, 1], [1, 0], [EYE, EYE])
    assert (want["hits"] == 0).all() and (want["nn_min"] > 2.8).all() and want["nn_min"][0] == want["nn_min"][1]
    T = synth.random_rigid(np.random.RandomState(9), 2.0, 1.0)
    want = check("apart_pose", pc, None, [0, 1], [1, 0], [T, np.linalg.inv(T)])
    assert np.isfinite(want["nn_min"]).all()


def test_a_nan_coordinate_among_the_valid_points():
    rs = np.random.RandomState(10)
    P = 1024
    pc = _two_blobs(rs, P, [0.2, 0.1, 0.01])
    pc[0, 5, 1] = np.nan
    pc[0, 77] = np.nan
    pc[1, 9, 0] = np.nan
    pc[1, 300, 2] = np.inf
    pc[0, 301, 0] = -np.inf
    want = check("nan", pc, None, [0, 1, 0], [1, 0, 0], [EYE, EYE, EYE])
    assert (want["n_valid"] == P).all()                             # they still count
    assert not want["hit"][0, [5, 77, 301]].any() and not want["hit"][1, [9, 300]].any() and want["hits"][2] == P - 3
    T = np.eye(4)
    T[0, 3] = np.nan                                                 # a pose that moves every point to NaN
    want = check("nan_pose", pc, None, [0], [1], [T])
    assert want["hits"][0] == 0 and np.isposinf(want["nn_min"][0])


def test_an_extent_that_cannot_be_keyed_is_an_error_and_writes_nothing():
    import torch
    from relativepose_amd import _lib
    dev = torch.device("cuda:0")
    P = 1024
    pc = np.random.RandomState(11).uniform(0, 1, (2, P, 3))
    pc[1, 3, 2] = 1.0e6                                              # 1.25e7 cells of 0.08 along z
    pcd = torch.from_numpy(pc).to(dev)
    pose = torch.eye(4, dtype=torch.float64, device=dev).repeat(2, 1, 1).contiguous()
    hits = torch.full((2,), -5, dtype=torch.int32, device=dev)
    nn_min = torch.full((2,), -5.0, dtype=torch.float64, device=dev)
    n_valid = torch.full((2,), -5, dtype=torch.int32, device=dev)
    hit = torch.full((2, P), 9, dtype=torch.uint8, device=dev)
    L = _lib.lib()
    nbytes = L.relpose_overlap_workspace_bytes(2, P, 2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    qc, rc = (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(1, 0)
    a = _lib.OverlapArgs()
    a.struct_size = C.sizeof(a)
    a.n_clouds, a.n_points, a.n_queries, a.max_dist = 2, P, 2, MD
    a.pc, a.valid, a.pose = pcd.data_ptr(), None, pose.data_ptr()
    a.query_cloud_host, a.ref_cloud_host = C.addressof(qc), C.addressof(rc)
    a.hits, a.nn_min, a.n_valid, a.hit = hits.data_ptr(), nn_min.data_ptr(), n_valid.data_ptr(), hit.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, None
    torch.cuda.synchronize()
    assert L.relpose_overlap(C.byref(a)) == _lib.OVERLAP_EXTENT
    torch.cuda.synchronize()
    assert (hits == -5).all() and (nn_min == -5.0).all() and (n_valid == -5).all() and (hit == 9).all()
    a.max_dist = 20.0                                                # 5e4 cells: the same clouds can be keyed at this radius
    assert L.relpose_overlap(C.byref(a)) == 0
    torch.cuda.synchronize()
    want = OM.overlap(pc, None, [0, 1], [1, 0], [EYE, EYE], 20.0)
    assert np.array_equal(hits.cpu().numpy(), want["hits"]) and np.array_equal(OS.bits(nn_min.cpu().numpy()), OS.bits(want["nn_min"]))


def test_a_query_does_not_depend_on_its_batch_and_runs_repeat():
    s = OS.scene("suncg", 32)
    a = run(s["pc"], s["valid"], s["qc"], s["rc"], s["T"])
    b = run(s["pc"], s["valid"], s["qc"], s["rc"], s["T"])
    assert OS.same(a, b) == []
    for k in range(len(s["qc"])):
        one = run(s["pc"], s["valid"], s["qc"][k:k + 1], s["rc"][k:k + 1], s["T"][k:k + 1])
        assert one["hits"][0] == a["hits"][k] and OS.bits(one["nn_min"])[0] == OS.bits(a["nn_min"])[k] and np.array_equal(one["hit"][0], a["hit"][k])
    # nor on the order of the queries or on clouds that nothing names
    perm = np.random.RandomState(0).permutation(len(s["qc"]))
    c = run(np.concatenate([s["pc"][:1] * 0 + 5.0, s["pc"]]), np.concatenate([s["valid"][:1], s["valid"]]), s["qc"][perm] + 1, s["rc"][perm] + 1, s["T"][perm])
    assert np.array_equal(c["hits"], a["hits"][perm]) and np.array_equal(OS.bits(c["nn_min"]), OS.bits(a["nn_min"])[perm])


def _yardstick(pc, valid, R_gt):
    """util.point_cloud_overlap, the unchanged per-pair brute-force path, pair by pair -> [B,4]"""
    from relativepose_amd import util
    out = []
    for b in range(len(R_gt)):
        out.append(util.point_cloud_overlap(pc[2 * b][valid[2 * b] != 0], pc[2 * b + 1][valid[2 * b + 1] != 0], R_gt[b]))
    return np.array(out, dtype=np.float64)


def _check_pairs_against_yardstick(pcd, vad, R_gt):
    from relativepose_amd import util
    got = np.stack([t.cpu().numpy() for t in util.point_cloud_overlap_dev(pcd, vad, R_gt)], 1)        # overlap, cam_dist, pc_dist, pc_nn
    want = _yardstick(pcd.cpu().numpy(), vad.cpu().numpy(), R_gt)
    log("overlap_pairs", got=got, want=want)
    assert np.array_equal(OS.bits(got[:, 0]), OS.bits(want[:, 0])) and np.array_equal(OS.bits(got[:, 3]), OS.bits(want[:, 3]))
    assert np.allclose(got[:, 1:3], want[:, 1:3], rtol=1e-12, atol=0)
    return got, want


@pytest.mark.parametrize("ds,mm,seed", GEOM_CASES)
def test_paired_driver_and_records_match_the_yardstick(golden_dir, ds, mm, seed):
    """The GEOM_CASES pairs at h = 160: point_cloud_overlap_dev against util.point_cloud_overlap and the goldens, and evaluate_pairs'
    records carry exactly the yardstick's values."""
    import torch
    from types import SimpleNamespace
    from relativepose_amd import evaluation as E
    from relativepose_amd import util, weights
    from relativepose_amd.model import SCNet
    from relativepose_amd.pipeline import RelativePosePipeline
    dev = torch.device("cuda:0")
    gst = np.load(os.path.join(golden_dir, "stats.npz"))
    d = synth.make_pairs(1, seed + 40, ds)
    pcd, vad = util.depth2pc_dev(torch.from_numpy(d["depth"][0]).to(dev), ds)
    R_gt = [np.matmul(d["R"][0, 1], np.linalg.inv(d["R"][0, 0]))]
    assert np.array_equal(R_gt[0], gst[f"stats_{ds}_Rgt"])
    got, want = _check_pairs_against_yardstick(pcd, vad, R_gt)
    assert np.allclose(got[0], gst[f"stats_{ds}_overlap"], rtol=1e-9, atol=1e-12)
    S = 15
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=1, outputType="rgbdnsf", snumclass=S))
    net.load_state_dict(weights.make_state_dict(7, S))
    pipe = RelativePosePipeline(net, ds, mm, alter_steps=1)
    pts, ptw = synth.make_keypoints(1, 40, seed, mm)
    rec = E.evaluate_pairs(pipe, [dict(d, pts=pts, ptw=ptw)], dev)[0]
    vals = np.array([rec["overlap"], rec["cam_dist"], rec["pc_dist"], rec["pc_nearest"]], dtype=np.float64)
    assert np.array_equal(OS.bits(vals), OS.bits(want[0]))
    sub = {k: d[k] for k in ("depth", "R")}
    rec2 = E._default_record(pipe, sub, np.eye(4)[None], dev, None, [0])[0]
    assert np.array_equal(OS.bits([rec2[k] for k in ("overlap", "cam_dist", "pc_dist", "pc_nearest")]), OS.bits(want[0]))


@pytest.fixture(scope="module")
def scene48():
    """the suncg h = 48 scene on the device: (pc, valid) through the product's own depth2pc"""
    import torch
    from relativepose_amd import util
    s = OS.scene("suncg", 48)
    pcd, vad = util.depth2pc_dev(torch.from_numpy(s["scene"]["depth"]).to("cuda:0"), "suncg")
    assert np.array_equal(pcd.cpu().numpy()[vad.cpu().numpy() != 0], s["pc"][s["valid"] != 0])
    return s, pcd, vad


def test_paired_driver_on_a_scene_matches_the_yardstick(scene48):
    import torch
    s, pcd, vad = scene48
    R = s["scene"]["R"]
    pairs = [(0, 1), (2, 3), (4, 5), (1, 4), (5, 0), (3, 0)]
    idx = torch.tensor([k for ij in pairs for k in ij], device=pcd.device)
    R_gt = [np.matmul(R[j], np.linalg.inv(R[i])) for i, j in pairs]
    got, want = _check_pairs_against_yardstick(pcd[idx].contiguous(), vad[idx].contiguous(), R_gt)
    assert (got[:, 0] > 0.1).any() and (got[:, 0] == 0).any()


def test_overlap_matrix_equals_the_paired_call_and_mining_equals_the_model(scene48):
    import torch
    from relativepose_amd import evaluation as E
    from relativepose_amd import util
    s, pcd, vad = scene48
    R, M = s["scene"]["R"], OS.SCENE_VIEWS
    frac, nn, n_valid = (t.cpu().numpy() for t in util.overlap_matrix_dev(pcd, vad, R))
    assert np.array_equal(n_valid, s["want"]["n_valid"]) and (np.diag(frac) == 1).all() and (np.diag(nn) == 0).all()
    # the paired call: its source -> target query is the matrix's (i, j) entry; its target -> source query runs under np.linalg.inv(T_ij),
    # which is not bitwise the matrix's own product R_i inv(R_j), so that direction is taken from a single query under the same inverse
    for i in range(M):
        for j in range(M):
            if i == j:
                continue
            idx = torch.tensor([i, j], device=pcd.device)
            pc2, va2 = pcd[idx].contiguous(), vad[idx].contiguous()
            T_ij = np.matmul(R[j], np.linalg.inv(R[i]))
            inv = torch.from_numpy(np.linalg.inv(T_ij)[None]).to(pcd.device)
            fwd_h, fwd_nn, nv = util.overlap_dev(pc2, va2, [0], [1], torch.from_numpy(T_ij[None]).to(pcd.device))
            assert int(fwd_h[0]) / int(nv[0]) == frac[i, j] and float(fwd_nn[0]) == nn[i, j]
            rev_h, rev_nn, _ = util.overlap_dev(pc2, va2, [1], [0], inv)
            ov, _, _, pc_nn = util.point_cloud_overlap_dev(pc2, va2, [T_ij])
            assert float(ov[0]) == max(frac[i, j], int(rev_h[0]) / int(nv[1])) and float(pc_nn[0]) == (nn[i, j] + float(rev_nn[0])) / 2
    want_frac = OM.fractions(s["want"], s["qc"], s["rc"], M)
    assert np.array_equal(frac, want_frac)
    assert np.array_equal(OS.bits(nn[~np.eye(M, dtype=bool)]), OS.bits(s["want"]["nn_min"]))
    ids = [f"v{k}" for k in range(M)]
    for mo in (None, 0.1):
        assert E.mine_pairs(s["scene"]["depth"], R, "suncg", "room7", ids, min_overlap=mo) == E.pairs_from_overlap(want_frac, "room7", ids, mo)


def test_scene_batch_fills_more_than_one_bucket(tmp_path):
    import torch
    from types import SimpleNamespace
    from relativepose_amd import evaluation as E
    from relativepose_amd import weights
    from relativepose_amd.model import SCNet
    from relativepose_amd.pipeline import RelativePosePipeline
    dev = torch.device("cuda:0")
    sb = E.SceneBatch(6, 5, "suncg", "second", 40, views=5, balanced=True, max_scenes=4)
    S = 15
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=1, outputType="rgbdnsf", snumclass=S))
    net.load_state_dict(weights.make_state_dict(7, S))
    pipe = RelativePosePipeline(net, "suncg", "second", alter_steps=1)
    batch = sb.take(range(sb.size))
    assert batch["rgb"].shape == (6, 2, 3, 160, 640) and batch["R"].shape == (6, 2, 4, 4) and len(sb.pairs) == 6
    stats = E.evaluate_pairs(pipe, [batch], dev)
    assert [r["overlap"] for r in stats] == [e["overlap"] for e in sb.pairs]       # the mined overlap is the record's
    filled = [k for k, v in E.summarize(stats).items() if v["nobs"] > 0]
    log("overlap_scene_batch", overlaps=[float(r["overlap"]) for r in stats], filled=filled)
    assert len(filled) >= 2
    p = E.save_data_list(str(tmp_path / "x.datalist"), {"test": sb.pairs})
    assert len(E.load_data_list(p, "test")) == 6


def test_full_frame_clouds():
    """One synth.make_full_res_pair pair, 307 200 points per cloud, a small motion apart.  The yardstick's O(P^2) float64 scan of the whole
    clouds is 1.9e11 distance evaluations per pair, so util.point_cloud_overlap is compared bitwise on every 8th point of both clouds
    (38 400 points each).  The call on the WHOLE clouds is checked through its per-point stage output: for every 61st query point the
    yardstick's kernel (util.nn_dist_dev) scans the whole reference cloud, and its distance decides the same hit flag; nn_min is no
    larger than the smallest of those distances."""
    import torch
    from relativepose_amd import _lib, util
    dev = torch.device("cuda:0")
    depth, _ = synth.make_full_res_pair(21)
    dd = torch.from_numpy(np.ascontiguousarray(depth[0])).to(dev)
    P = 480 * 640
    pcd = torch.empty(2, P, 3, dtype=torch.float64, device=dev)
    vad = torch.empty(2, P, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().relpose_depth2pc_full(_lib.ptr(dd), _lib.ptr(pcd), _lib.ptr(vad), 2, 480, 640, _lib.stream_ptr()), "relpose_depth2pc_full")
    T = synth.random_rigid(np.random.RandomState(22), 0.05, 0.1)
    poses = torch.from_numpy(np.stack([T, np.linalg.inv(T)])).to(dev)
    hits, nn_min, n_valid, hit = util.overlap_dev(pcd, vad, [0, 1], [1, 0], poses, want_hit=True)
    log("overlap_full_frame", hits=hits.cpu().numpy(), n_valid=n_valid.cpu().numpy(), nn_min=nn_min.cpu().numpy())
    assert torch.equal(n_valid, (vad != 0).sum(1).to(torch.int32)) and torch.equal(hits, hit.sum(1).to(torch.int32))
    assert (hits > 1000).all() and (hits < n_valid).all() and not hit[vad == 0].any()
    for k, (q, r) in enumerate(((0, 1), (1, 0))):
        sub = torch.arange(0, P, 61, device=dev)
        sub = sub[vad[q][sub] != 0]
        d = util.nn_dist_dev(pcd[q][sub].contiguous(), pcd[r], poses[k].contiguous(), None, vad[r])
        assert torch.equal(hit[k][sub] != 0, d < MD) and 0 < int((d < MD).sum()) < len(sub)
        assert 0.0 < float(nn_min[k]) <= float(d.min())
    _check_pairs_against_yardstick(pcd[:, ::8].contiguous(), vad[:, ::8].contiguous(), [T])


def test_mine_pairs_command_line(tmp_path, capsys):
    """--mine-pairs prints one JSON line and writes the data list the loaders' expression reads back."""
    import json
    from relativepose_amd import evaluation as E
    exp = str(tmp_path / "mined")
    E.main(["--mine-pairs", "--scenes", "2", "--scene-views", "4", "--dataset", "suncg", "--seed", "7", "--exp", exp])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["mine_pairs"] and (line["scenes"], line["views"], line["pairs"]) == (2, 4, 12) and sum(line["pairs_per_bucket"].values()) == 12
    assert line["data_list"] == exp + ".datalist.npy" and line["seconds"] > 0
    entries = np.load(line["data_list"], allow_pickle=True).item()["test"]
    assert len(entries) == 12 and entries[0]["base"] == "scene7" and entries[-1]["base"] == "scene8"
    assert [(e["id_src"], e["id_tgt"]) for e in entries[:6]] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    sc = synth.render_scene(7, 4, "suncg")
    assert entries[:6] == E.mine_pairs(sc["depth"], sc["R"], "suncg", "scene7")
    E.main(["--mine-pairs", "--scenes", "2", "--scene-views", "4", "--dataset", "suncg", "--seed", "7", "--min-overlap", "0.1"])
    kept = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert kept["pairs"] == sum(1 for e in entries if e["overlap"] >= 0.1) and kept["data_list"] is None
