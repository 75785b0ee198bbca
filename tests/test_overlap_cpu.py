"""CPU: the overlap contract's two numpy statements agree bit for bit on multi-view scenes whose queries hit and miss, the model's
statistics are the reference's (sklearn KDTree oracle and the stats.npz goldens), and the host layers around relpose_overlap -- pair
mining, the data-list file, operator registration, argument validation -- work without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import overlap_model as OM
import overlap_scenes as OS
from cases import GEOM_CASES
from oracle import stats_oracle as S
from relativepose_amd import synth

TOL = dict(rtol=1e-9, atol=1e-12)               # test_gpu_stats.py's


@pytest.mark.parametrize("ds,h", OS.SCENES)
def test_grid_model_equals_brute_model_bitwise(ds, h):
    s = OS.scene(ds, h)
    want = s["want"]
    got = OM.overlap(s["pc"], s["valid"], s["qc"], s["rc"], s["T"], model="grid")
    assert OS.same(got, want) == []
    Q = len(s["qc"])
    assert Q == 30
    nohit = int((want["hits"] == 0).sum())
    assert 3 * nohit >= Q and 3 * (Q - nohit) >= Q                  # both kinds of query are well represented
    assert nohit == OS.NO_HIT[(ds, h)]
    assert np.isfinite(want["nn_min"]).all() and (want["nn_min"][want["hits"] == 0] >= 0.08).all()
    assert (want["nn_min"][want["hits"] > 0] < 0.08).all()


def test_scenes_cover_all_three_overlap_buckets():
    from relativepose_amd import evaluation as E
    seen = set()
    top = 0.0
    for ds, h in OS.SCENES[1:]:                                     # h = 48
        s = OS.scene(ds, h)
        frac = OM.fractions(s["want"], s["qc"], s["rc"], OS.SCENE_VIEWS)
        sym = np.maximum(frac, frac.T)[np.triu_indices(OS.SCENE_VIEWS, 1)]
        seen |= {E.overlap_bucket(v) for v in sym}
        top = max(top, sym.max())
    assert seen == set(E.OVERLAPS) and 0.5 < top < 0.6


def test_fast_brute_model_is_the_brute_model():
    s = OS.scene("suncg", 32)
    got = OM.overlap(s["pc"], s["valid"], s["qc"], s["rc"], s["T"], model="fast")
    assert OS.same(got, s["want"]) == []


@pytest.mark.parametrize("ds,h", OS.SCENES)
def test_model_statistics_match_the_kdtree_oracle_on_scenes(ds, h):
    s = OS.scene(ds, h)
    pc, valid, R = s["pc"], s["valid"], s["scene"]["R"]
    pairs = [(0, 1), (2, 3), (4, 5), (0, 5), (1, 4)]
    pcp = np.stack([pc[k] for ij in pairs for k in ij])
    vap = np.stack([valid[k] for ij in pairs for k in ij])
    R_gt = [np.matmul(R[j], np.linalg.inv(R[i])) for i, j in pairs]
    got = OM.pair_statistics(pcp, vap, R_gt)
    for b, (i, j) in enumerate(pairs):
        want = S.point_cloud_overlap(pc[i][valid[i] != 0], pc[j][valid[j] != 0], R_gt[b])
        assert np.allclose(got[b], want, **TOL), (i, j, got[b], want)
        # the matrix queries carry the same numbers
        k_ij = [k for k in range(30) if (s["qc"][k], s["rc"][k]) == (i, j)][0]
        k_ji = [k for k in range(30) if (s["qc"][k], s["rc"][k]) == (j, i)][0]
        n = s["want"]["n_valid"]
        assert got[b][0] == max(s["want"]["hits"][k_ij] / n[i], s["want"]["hits"][k_ji] / n[j])


@pytest.mark.parametrize("ds,mm,seed", GEOM_CASES)
def test_model_statistics_match_the_oracle_and_the_goldens(golden_dir, ds, mm, seed):
    gst = np.load(os.path.join(golden_dir, "stats.npz"))
    d = synth.make_pairs(1, seed + 40, ds)
    o = S.observed_clouds(d["depth"][0], ds)
    n = max(len(o[0]), len(o[1]))
    pc, valid = np.zeros((2, n, 3)), np.zeros((2, n), np.uint8)
    for k in range(2):
        pc[k, :len(o[k])] = o[k]
        valid[k, :len(o[k])] = 1
    Rgt = gst[f"stats_{ds}_Rgt"]
    got = OM.pair_statistics(pc, valid, [Rgt], model="fast")[0]
    assert np.allclose(got, S.point_cloud_overlap(o[0], o[1], Rgt), **TOL)
    assert np.allclose(got, gst[f"stats_{ds}_overlap"], **TOL)


def test_render_scene_follows_its_recipe():
    sc = synth.render_scene(11, 3, "matterport", 16)
    rs = np.random.RandomState(11)
    half = rs.uniform(1.5, 4.0, 3)
    assert np.array_equal(sc["half"], half)
    poses = []
    for _ in range(3):
        T = synth.random_rigid(rs, np.pi, 1.0)
        T[:3, 3] = np.clip(T[:3, 3], -0.6 * half, 0.6 * half)
        poses.append(T)
    assert np.array_equal(sc["pose"], np.stack(poses))
    assert np.array_equal(sc["R"], np.stack([np.linalg.inv(T) for T in poses]))
    a = synth.render_room(rs, "matterport", 0.01, 16, poses=poses[:2], half=half)
    b = synth.render_room(rs, "matterport", 0.01, 16, poses=[poses[2], poses[2]], half=half)
    assert np.array_equal(sc["depth"][:2], a[2]) and np.array_equal(sc["depth"][2], b[2][0])
    assert np.array_equal(sc["rgb"][2], b[0][0]) and np.array_equal(sc["norm"][:2], a[1])
    assert sc["rgb"].shape == (3, 3, 16, 64) and sc["depth"].dtype == np.float32
    assert (synth.render_scene(5, 2, "suncg", 16)["depth"] != 0).all()          # suncg: no holes


def test_pairs_from_overlap():
    from relativepose_amd import evaluation as E
    frac = np.array([[1.0, 0.2, 0.05, 0.1],
                     [0.3, 1.0, 0.6, 0.0],
                     [0.0, 0.5, 1.0, 0.5],
                     [0.1000001, 0.0, 0.2, 1.0]])
    ids = [10, 11, 12, 13]
    p = E.pairs_from_overlap(frac, "room", ids)
    assert [(e['id_src'], e['id_tgt']) for e in p] == [(10, 11), (10, 12), (10, 13), (11, 12), (11, 13), (12, 13)]      # i < j, sorted by (i, j)
    assert all(set(e) == {'base', 'id_src', 'id_tgt', 'overlap'} and e['base'] == "room" for e in p)
    assert [e['overlap'] for e in p] == [0.3, 0.05, 0.1000001, 0.6, 0.0, 0.5]                                            # max of both directions
    assert p == E.pairs_from_overlap(frac.T, "room", ids)                                                                 # symmetric
    assert [E.overlap_bucket(e['overlap']) for e in p] == ['0.1-0.5', '0-0.1', '0.1-0.5', '0.5-1.0', '0-0.1', '0.1-0.5']  # 0.5 is in the middle bucket
    q = E.pairs_from_overlap(frac, "room", ids, min_overlap=0.1)
    assert [(e['id_src'], e['id_tgt']) for e in q] == [(10, 11), (10, 13), (11, 12), (12, 13)]
    frac[0, 3] = frac[3, 0] = 0.1
    assert (10, 13) in [(e['id_src'], e['id_tgt']) for e in E.pairs_from_overlap(frac, "room", ids, min_overlap=0.1)]     # the rule is ov < 0.1
    with pytest.raises(ValueError):
        E.pairs_from_overlap(frac, "room", ids[:3])


def test_data_list_round_trip(tmp_path):
    from relativepose_amd import evaluation as E
    frac = np.array([[1.0, 0.2], [0.7, 1.0]])
    lists = {"train": E.pairs_from_overlap(frac, "a", [3, 9]), "test": E.pairs_from_overlap(frac.T, "b", ["x", "y"])}
    p = E.save_data_list(str(tmp_path / "exp.datalist"), lists)
    assert p.endswith(".datalist.npy")
    for split in lists:
        back = np.load(p, allow_pickle=True).item()[split]                      # the loaders' expression (datasets/SUNCG.py:66)
        assert back == lists[split] and E.load_data_list(p, split) == lists[split]
    assert back[0] == {'base': "b", 'id_src': "x", 'id_tgt': "y", 'overlap': 0.7}


def test_operator_is_registered_with_a_meta_kernel():
    import torch
    from relativepose_amd import ops
    assert "overlap" in ops.OPS
    m = lambda *s, dt: torch.empty(*s, dtype=dt, device="meta")
    hits, nn_min, n_valid = torch.ops.relpose.overlap(m(6, 100, 3, dt=torch.float64), m(6, 100, dt=torch.uint8), m(30, dt=torch.int32),
                                                      m(30, dt=torch.int32), m(30, 4, 4, dt=torch.float64), 0.08)
    assert hits.shape == (30,) and hits.dtype == torch.int32 and nn_min.shape == (30,) and nn_min.dtype == torch.float64
    assert n_valid.shape == (6,) and n_valid.dtype == torch.int32
    hits, _, _ = torch.ops.relpose.overlap(m(2, 10, 3, dt=torch.float64), None, m(2, dt=torch.int32), m(2, dt=torch.int32), m(2, 4, 4, dt=torch.float64))
    assert hits.shape == (2,)
    with pytest.raises(Exception):                                              # no CPU kernel: loud failure, no fallback
        torch.ops.relpose.overlap(torch.zeros(2, 10, 3, dtype=torch.float64), None, torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                  torch.zeros(2, 4, 4, dtype=torch.float64))


def test_invalid_arguments_are_rejected_without_a_device():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.lib()
    EINVAL = -1
    assert lib.relpose_overlap(None) == EINVAL
    buf = (C.c_double * 64)()                      # host memory: a valid call would fault, an invalid one must not touch it
    p = C.addressof(buf)
    qc, rc = (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(1, 0)

    def call(**kw):
        a = _lib.OverlapArgs()
        a.struct_size = C.sizeof(a)
        a.n_clouds, a.n_points, a.n_queries, a.max_dist = 2, 8, 2, 0.08
        a.pc = a.valid = a.pose = a.hits = a.nn_min = a.n_valid = p
        a.query_cloud_host, a.ref_cloud_host = C.addressof(qc), C.addressof(rc)
        a.workspace, a.workspace_bytes = 256 * 1024, 1 << 30              # never dereferenced on these paths
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.relpose_overlap(C.byref(a))

    assert call(struct_size=16) == EINVAL
    assert call(struct_size=C.sizeof(_lib.OverlapArgs) - 8) == EINVAL          # the stream field is cut off
    for name in ("pc", "query_cloud_host", "ref_cloud_host", "pose", "hits", "nn_min", "n_valid", "workspace"):
        assert call(**{name: None}) == EINVAL, name
    for md in (0.0, -0.08, float("nan"), float("inf")):
        assert call(max_dist=md) == EINVAL, md
    assert call(n_clouds=0) == EINVAL and call(n_points=0) == EINVAL and call(n_queries=0) == EINVAL
    assert call(n_points=(1 << 24) + 1) == EINVAL
    assert call(n_clouds=1) == EINVAL                                          # cloud index 1 is out of range
    bad = (C.c_int32 * 2)(0, -1)
    assert call(query_cloud_host=C.addressof(bad)) == EINVAL and call(ref_cloud_host=C.addressof(bad)) == EINVAL
    bad[1] = 2
    assert call(ref_cloud_host=C.addressof(bad)) == EINVAL
    assert call(workspace_bytes=64) == EINVAL and call(workspace=256 * 1024 + 8) == EINVAL
    assert lib.relpose_overlap_workspace_bytes(2, 8, 2) > 0
    assert lib.relpose_overlap_workspace_bytes(0, 8, 2) == 0 and lib.relpose_overlap_workspace_bytes(2, 0, 2) == 0
    per_point = (lib.relpose_overlap_workspace_bytes(4, 480 * 640, 4) - lib.relpose_overlap_workspace_bytes(4, 240 * 640, 4)) / (4 * 240 * 640)
    assert 40 <= per_point <= 64                                               # O(P) per cloud: sorted keys, indices and coordinates
    assert _lib.OVERLAP_EXTENT == -7 != EINVAL


def test_cli_flags_and_their_defaults():
    from relativepose_amd import evaluation as E
    a = E._cli_parser_completion().parse_args([])
    assert (a.mine_pairs, a.pair_source, a.min_overlap, a.scenes, a.scene_views) == (False, "pairs", None, 8, 6)
    a = E._cli_parser_completion().parse_args(["--mine-pairs", "--scenes", "3", "--scene-views", "5", "--min-overlap", "0.1", "--exp", "out"])
    assert a.mine_pairs and (a.scenes, a.scene_views, a.min_overlap, a.exp) == (3, 5, 0.1, "out")
    for argv in (["--mine-pairs", "--gpus", "2"], ["--mine-pairs", "--scene-views", "1"], ["--pair-source", "scenes", "--descriptor-eval"],
                 ["--pair-source", "scenes", "--keypoint-mode", "reference"]):
        with pytest.raises(SystemExit):
            E.main(argv)
