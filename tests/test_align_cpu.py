"""CPU: the alignment contract's numpy model (tests/align_model.py) agrees with its own plain-loop statement, unprojected pixels project onto
themselves, the closed room's views converge from three starts to one pose with every direction observed, view 0 of the pinned rooms has
exactly one held direction along which nothing moves, the default eigenvalue floor lies between the two measured ranges, leave-one-out by
subtraction is direct fusion bit for bit, the quantised step stays within its pin of the unquantised one, and the host layers around
relpose_tsdf_align -- operator registration, workspace queries, argument validation, the CLI flag -- work without a GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import align_model as AM
import align_scenes as AS
import tsdf_model as TM
import tsdf_scenes as TS
import visibility_model as VM

# Measured with the model (DESIGN.md §4.19 holds the same numbers); the pins are the measured values x 1.25.
# closed room, per (h, view): the rms point displacement against the truth after 12 iterations (voxels; the largest of the three starts), and
# the largest difference between the three starts' refined pose entries.
CLOSED = {(16, 0): (0.05239, 2.62e-4), (16, 1): (0.05222, 1.03e-7), (16, 2): (0.05272, 1.51e-7),
          (32, 0): (0.02322, 2.56e-8), (32, 1): (0.02204, 6.70e-9), (32, 2): (0.02795, 1.39e-8), (32, 3): (0.02395, 5.66e-6)}
BEFORE = {(16, 0): 1.0468, (16, 1): 1.0501, (16, 2): 1.0741, (32, 0): 2.0898, (32, 1): 2.0951, (32, 2): 2.1396, (32, 3): 1.9574}
AGREE_FLOOR = 1e-6        # below this the starts differ by what 12 iterations leave of the convergence; last bits of the fixture move it freely
# pinned rooms, view 0, the largest over the three starts: |x| and |z| of the camera centre's error (voxels), rotation error (degrees)
PINNED0 = {"suncg16": (0.0065, 0.1616), "suncg32": (0.0045, 0.0426), "scannet16": (0.0055, 0.1730)}
# pinned rooms, view 1 (every direction observed): displacement after (voxels), largest over the starts
PINNED1 = {"suncg16": 0.07134, "suncg32": 0.02197, "scannet16": 0.07622}
QUANT_DELTA = 3.18e-5     # the largest difference between the quantised and the unquantised step (radians / voxels) over test 7's cases; pin x 4


def centre_error(c, v, T):
    """the camera centre's error in the world frame, voxels"""
    return (np.linalg.inv(T)[:3, 3] - np.linalg.inv(c["R"][v])[:3, 3]) / c["voxel"]


def held_columns(r, e):
    st = r["steps"][0][e]
    n = int(r["trace_sums"][0, e, AM.USED])
    return [k for k in range(6) if not (n >= 6 and st["lam"][k] > AS.EIG_MIN * n)]


# ---------------------------------------------------------------------------------------------- 1. loops = vectorised
@pytest.mark.parametrize("case", ["edge_suncg", "edge_matterport", "edge_scannet", "batch_stride3", "boundary"])
def test_loops_equal_the_vectorised_form(case):
    if case == "boundary":
        p, want = AS.boundary_points()
        rs = np.random.RandomState(2)
        ts = (rs.randint(-30000, 30000, (5, 3, 4)) * 2).astype(np.int32)
        wt = np.full((5, 3, 4), 2, np.int32)
        a = AM.accumulate(p, np.eye(4), ts, wt, [0.0, 0.0, 0.0], 1.0)
        b = AM.accumulate_loops(p, np.eye(4), ts, wt, [0.0, 0.0, 0.0], 1.0)
        assert TS.bits_equal(a, b)
        for k in (AM.OUTSIDE, AM.UNKNOWN, AM.SATURATED, AM.USED):
            assert a[k] == want.count(k)
        for q, k in zip(p, want):                                               # one by one: each point gets the class the contract gives it
            one = AM.accumulate(q[None], np.eye(4), ts, wt, [0.0, 0.0, 0.0], 1.0)
            assert one[k] == 1 and one[28:].sum() == 1, (q, k)
        return
    if case.startswith("edge_"):
        c, kw = AS.edge_case(case[5:]), dict(iters=2, min_weight=2)
    else:
        c, kw = AS.batch(), dict(iters=2, stride=3)
    a, b = AS.model_of(c, **kw), AS.model_of(c, loops=True, **kw)
    assert TS.differ(a, b, AS.OUT_KEYS + AS.TRACE_KEYS) == []
    if case.startswith("edge_"):
        n = a["trace_sums"][:, 0, 28:]
        assert (n.sum(1) == 4 * 4 * 4 - np.array([4, 0, 0])).all()              # view 0 has four pixels without data
        assert (n[1:, 0] == 64).all() and (a["held"][1:] == 6).all()            # a NaN / an inf in the pose: every point outside
        assert TS.bits_equal(a["pose"][1:], c["pose"][1:])                      # and the pose comes back bit for bit
        if case == "edge_suncg":
            assert n[0, 1] > 0 and n[0, 2] > 0 and n[0, 3] >= 6                 # unknown (min_weight - 1), saturated (|t| = 1) and used points


# ---------------------------------------------------------------------------------------------- 2. unprojection
@pytest.mark.parametrize("ds", ["suncg", "matterport", "scannet"])
def test_unprojected_pixels_project_onto_themselves(ds):
    for h in (4, 16, 22):
        depth = np.random.RandomState(h).uniform(0.3, 5.0, (h, 4 * h)).astype(np.float32)
        p, pix = AM.unproject(depth, ds)
        assert len(pix) == 4 * h * h
        back, d = VM.project(p, h, ds)
        row, px = pix // (4 * h), pix % h
        inner = (row >= 1) & (px >= 1)
        assert np.array_equal(back[inner], pix[inner])
        assert np.array_equal(d[inner], depth.reshape(-1)[pix[inner]].astype(np.float64))
        assert (back[~inner] == -1).all()                                       # xn = -1 or yn = 1: the face's open edge, which no face takes
    p, pix = AM.unproject(depth, ds, stride=3)
    assert np.array_equal(pix, np.arange(0, 4 * h * h, 3))
    depth[0, :5] = [0.0, -1.0, np.nan, np.inf, -np.inf]
    assert len(AM.unproject(depth, ds)[1]) == 4 * h * h - 5


# ---------------------------------------------------------------------------------------------- 3. the closed room
@pytest.mark.parametrize("h,v", sorted(CLOSED))
def test_closed_room_converges_from_three_starts(h, v):
    name = f"closed{h}"
    c = AS.scene(name)
    assert c["dims"] == {16: (22, 16, 26), 32: (38, 26, 46)}[h]
    runs = [AS.solo(name, v, k) for k in range(3)]
    agree = max(float(np.abs(r["pose"][0] - runs[0]["pose"][0]).max()) for r in runs)
    disp = [AS.displacement(c, v, r["pose"][0]) for r in runs]
    before = AS.displacement(c, v, AS.start_pose(c, v, 2))
    print("closed room", h, v, "displacement before", before, "after", disp, "agreement", agree, "eig", runs[2]["eig"][0])
    m_disp, m_agree = CLOSED[(h, v)]
    assert agree <= max(1.25 * m_agree, AGREE_FLOOR)
    assert max(disp) <= 1.25 * m_disp and max(disp) >= 0.75 * m_disp            # and the table in DESIGN.md is still what the model gives
    assert abs(before - BEFORE[(h, v)]) < 1e-3
    for r in runs:
        assert all(st["held"] == 0 for st in r["steps"][0]) and r["held"][0] == 0
        assert r["rms"][0, 1] <= r["rms"][0, 0]
    if h == 32:
        assert max(disp) < before / 10


# ---------------------------------------------------------------------------------------------- 4. the pinned rooms
@pytest.mark.parametrize("name", sorted(PINNED0))
def test_pinned_room_view_0_holds_its_unobservable_direction(name):
    c = AS.scene(name)
    xz, rot = [], []
    for k in range(3):
        r = AS.solo(name, 0, k)
        for e, st in enumerate(r["steps"][0]):
            held = held_columns(r, e)
            assert st["held"] == 1 and len(held) == 1
            assert st["coef"][held[0]] == 0.0                                   # the pose change's component along the held direction: exactly zero
            assert abs(st["vec"][4, held[0]]) > 0.99                            # the translation along y: this view sees no +-y wall
        assert r["held"][0] == 1
        err = centre_error(c, 0, r["pose"][0])
        xz.append(max(abs(err[0]), abs(err[2])))
        rot.append(AS.rotation_error_deg(c, 0, r["pose"][0]))
    print("pinned room", name, "view 0: |x|, |z| error (voxels)", xz, "rotation error (degrees)", rot)
    assert max(xz) <= 1.25 * PINNED0[name][0] and max(rot) <= 1.25 * PINNED0[name][1]
    # the trap the floor closes: started at the truth, the undamped step drifts along y on gradient noise; the held step stays
    drift = abs(centre_error(c, 0, AS.solo(name, 0, 0, 0.0)["pose"][0])[1])
    stay = abs(centre_error(c, 0, AS.solo(name, 0, 0)["pose"][0])[1])
    print("y error from the truth (voxels): without the floor", drift, "with it", stay)
    assert stay < 0.01 and drift > 0.1
    assert AS.solo(name, 0, 0, 0.0)["held"][0] == 0


@pytest.mark.parametrize("name", sorted(PINNED1))
def test_pinned_room_view_1_observes_every_direction(name):
    c = AS.scene(name)
    disp = []
    for k in range(3):
        r = AS.solo(name, 1, k)
        assert all(st["held"] == 0 for st in r["steps"][0])
        disp.append(AS.displacement(c, 1, r["pose"][0]))
    print("pinned room", name, "view 1: displacement after (voxels)", disp)
    assert max(disp) <= 1.25 * PINNED1[name] and max(disp) >= 0.75 * PINNED1[name]


# ---------------------------------------------------------------------------------------------- 5. the default floor
def test_default_floor_lies_between_the_measured_ranges():
    from relativepose_amd import _lib
    assert _lib.TSDF_ALIGN_EIG_MIN == AS.EIG_MIN
    unobservable, observable = [], []
    for k in range(3):
        for name in PINNED0:
            unobservable.append(AS.solo(name, 0, k)["eig"][0, 0])
            observable.append(AS.solo(name, 1, k)["eig"][0, 0])
        for h, v in CLOSED:
            observable.append(AS.solo(f"closed{h}", v, k)["eig"][0, 0])
    lo, hi = max(unobservable), min(observable)
    print("smallest eigenvalue / n_used: unobservable", min(unobservable), "..", lo, " observable", hi, "..", max(observable))
    assert lo < AS.EIG_MIN < hi
    assert hi / lo >= 3.0                                                       # the ranges are well apart
    assert abs(math.log(AS.EIG_MIN / math.sqrt(lo * hi))) < math.log(1.05)      # the default is their geometric mean, to its two digits


# ---------------------------------------------------------------------------------------------- 6. leave-one-out
@pytest.mark.parametrize("name", ["closed16", "suncg16"])
def test_leave_one_out_by_subtraction_is_direct_fusion(name):
    c = AS.scene(name)
    everything = TS.fuse_model(c)
    for v in range(len(c["depth"])):
        alone = TS.fuse_model(c, order=[v])
        direct = TS.fuse_model(c, order=[u for u in range(len(c["depth"])) if u != v])
        for k in TS.STATE_KEYS:
            assert TS.bits_equal(everything[k] - alone[k], direct[k]), (v, k)


# ---------------------------------------------------------------------------------------------- 7. quantisation
def test_quantised_step_against_the_unquantised_normal_equations():
    worst = 0.0
    for name, v in (("closed16", 0), ("closed32", 1), ("suncg16", 0), ("suncg32", 1)):
        c, st = AS.scene(name), AS.leave_one_out(name, v)
        p, _ = AM.unproject(c["depth"][v], c["ds"])
        for k in (0, 2):
            T = AS.start_pose(c, v, k)
            sums, (A, b, r2, n) = AM.accumulate(p, T, st["tsdf_sum"][0], st["weight"][0], c["origin"][0], c["voxel"], 1, exact=True)
            got = AM.step(sums, T, c["origin"][0], c["dims"], c["voxel"], AS.EIG_MIN)
            lam, V = np.linalg.eigh(A)
            keep = lam > AS.EIG_MIN * n
            assert keep.sum() == 6 - got["held"]
            want = -(V[:, keep] / lam[keep]) @ (V[:, keep].T @ b)
            worst = max(worst, float(np.abs(want - got["delta"]).max()))
            assert np.allclose(sorted(lam / n), got["eig"], rtol=1e-3)
            assert abs(AM.rms(sums) - math.sqrt(r2 / n)) < 2.0 ** -16           # the residual's quantum
    print("quantised against unquantised step, largest difference", worst)
    assert worst <= 4 * QUANT_DELTA


def test_jacobi_diagonalises_and_the_update_is_rigid():
    rs = np.random.RandomState(0)
    J = rs.randn(40, 6) * np.array([30, 30, 30, 1, 1, 1])
    A = (J.T @ J).tolist()
    lam, V = AM.jacobi(A)
    V = np.array(V)
    assert np.allclose(V.T @ V, np.eye(6), atol=1e-13)
    assert np.allclose(V @ np.diag(lam) @ V.T, np.array(A), rtol=0, atol=1e-9 * np.abs(A).max())
    assert np.allclose(sorted(lam), np.linalg.eigvalsh(np.array(A)), rtol=1e-10)
    T = AS.scene("closed16")["R"][0]
    T2 = AM.apply_delta(T, [0.1, -0.2, 0.05, 0.3, -0.1, 0.2], [-1.0, -2.0, -3.0], (22, 16, 26), 0.25)
    assert np.allclose(T2[:3, :3] @ T2[:3, :3].T, np.eye(3), atol=1e-14) and np.array_equal(T2[3], T[3])
    assert TS.bits_equal(AM.apply_delta(np.eye(4), [0.0] * 6, [-1.0, -2.0, -3.0], (22, 16, 26), 0.25), np.eye(4))


# ---------------------------------------------------------------------------------------------- 8. invalid arguments
def test_invalid_arguments_are_rejected_without_a_device():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.lib()
    EINVAL = -1
    assert lib.relpose_tsdf_align(None) == EINVAL
    buf = (C.c_double * 256)(*([-7.5] * 256))          # host memory: a valid call would fault, an invalid one must not touch it
    p = C.addressof(buf)
    host = AS.host_arrays()
    calls = AS.einval_calls()
    assert len(calls) >= 45 and len({n for n, _ in calls}) == len(calls)
    for name, kw in calls:
        assert lib.relpose_tsdf_align(C.byref(AS.align_args(_lib, p, host, kw))) == EINVAL, name
    assert buf[:] == [-7.5] * 256
    W = lib.relpose_tsdf_align_workspace_bytes
    base = W(2, 3, 4, 3, 2, 2, 1)
    assert base >= 2 * 3 * 8 + 3 * 4 + 3 * 32 * 8 and base % 256 == 0
    assert W(1, 1, 160, 128, 128, 128, 1) - W(1, 1, 160, 128, 128, 128, 2) == (100 - 50) * 32 * 8      # one slab per 1024 sampled pixels
    for a in ((0, 3, 4, 3, 2, 2, 1), (2, 0, 4, 3, 2, 2, 1), (2, 3, 5, 3, 2, 2, 1), (2, 3, 0, 3, 2, 2, 1), (2, 3, 4, 0, 2, 2, 1), (2, 3, 4, 3, 2, 2, 0),
              (2, 3, 4, 2049, 2, 2, 1), (2, 3, 4, 3, 2049, 2, 1), (2, 3, 4, 3, 2, 2049, 1), (1, 1, 1026, 3, 2, 2, 1), (2, 3, 4, 2048, 1024, 1024, 1),
              (-1, 3, 4, 3, 2, 2, 1)):
        assert W(*a) == 0, a
    assert W(1, 1, 1024, 3, 2, 2, 1) > 0 and W(1, 1, 1026, 3, 2, 2, 2) > 0       # 2^22 sampled pixels: inside the limit


# ---------------------------------------------------------------------------------------------- 9. operator and CLI
def test_operator_is_registered_with_a_meta_kernel():
    import torch
    from relativepose_amd import ops
    assert "tsdf_align" in ops.OPS
    m = lambda *s, dt: torch.empty(*s, dtype=dt, device="meta")
    ts, wt = m(3, 27, 34, 20, dt=torch.int32), m(3, 27, 34, 20, dt=torch.int32)
    a = (ts, wt, m(3, 3, dt=torch.float64), 0.25, m(5, 16, 64, dt=torch.float32), m(5, 4, 4, dt=torch.float64), m(5, dt=torch.int32), 0)
    pose, eig, held, sums, rms, tp, tsm = torch.ops.relpose.tsdf_align(*a)
    assert pose.shape == (5, 4, 4) and pose.dtype == eig.dtype == rms.dtype == torch.float64 and eig.shape == (5, 6) and rms.shape == (5, 2)
    assert held.shape == (5,) and held.dtype == torch.int32 and sums.shape == (5, 32) and sums.dtype == torch.int64
    assert tp.numel() == 0 and tsm.numel() == 0
    tp, tsm = torch.ops.relpose.tsdf_align(*a, 7, 0.0, 2, 1, True)[5:]
    assert tp.shape == (5, 8, 4, 4) and tp.dtype == torch.float64 and tsm.shape == (5, 8, 32) and tsm.dtype == torch.int64
    with pytest.raises(Exception):                                              # no CPU kernel: loud failure, no fallback
        torch.ops.relpose.tsdf_align(torch.zeros(1, 2, 2, 2, dtype=torch.int32), torch.zeros(1, 2, 2, 2, dtype=torch.int32),
                                     torch.zeros(1, 3, dtype=torch.float64), 0.5, torch.ones(1, 4, 16), torch.eye(4, dtype=torch.float64)[None],
                                     torch.zeros(1, dtype=torch.int32), 0)


def test_cli_flag_and_its_default():
    from relativepose_amd import evaluation as E
    assert E._cli_parser_completion().parse_args([]).refine == 0
    assert E._cli_parser_completion().parse_args(["--reconstruct", "--fuse", "0.125", "--refine", "2"]).refine == 2
    for argv in (["--refine", "1"], ["--reconstruct", "--refine", "1"], ["--mine-pairs", "--fuse", "0.1", "--refine", "1"],
                 ["--reconstruct", "--fuse", "0.1", "--refine", "-1"], ["--method", "fgs", "--fuse", "0.1", "--refine", "1"]):
        with pytest.raises(SystemExit):
            E.main(argv)
