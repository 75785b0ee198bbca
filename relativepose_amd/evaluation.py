"""Evaluation-side bookkeeping of the reference driver (evaluation.py:286-320): pose error metrics per scan
pair, the ``error_stats`` record list and its ``<exp>.result.npy`` container, and a batched harness that runs
the device pipeline over a stream of scan-pair batches and fills those records ("called
unchanged" is realised by the build's own eval_pairs-style harness).

  angular_distance_np     util.py:176-187
  pose_errors             evaluation.py:291-297
  result_record           evaluation.py:299-305
  save_results / load_results   evaluation.py:319-320 (np.save of the list of dicts)
  evaluate_pairs          evaluation.py:203-320 (loop over the loader, keypoints injected)
  evaluate_pairs_sharded  the same over the GPUs of a node: the reference shards by hand (--entrySplit, evaluation.py:59,
                          datasets/SUNCG.py:68-69: one process and one result file per split, merged afterwards); here every global
                          batch is cut into contiguous per-rank blocks, ONE all_gather of the poses per round, rank 0 writes ONE
                          <exp>.result.npy and resumes from an existing one in units of 100 pairs (:129-133, :319-320)

  pairs_from_overlap / mine_pairs / save_data_list / load_data_list / SceneBatch
                          the loaders' dataList ({'base','id_src','id_tgt',...} per split, datasets/SUNCG.py:66,91-93), whose generator
                          was never published: which pairs of M posed scans overlap, from util.overlap_matrix_dev
  select_pose / verify_summary / spearman / observed_depth, evaluate_pairs(verify=...)
                          no counterpart: the visibility check of an estimated pose against the partner's depth panorama
                          (util.pose_visibility_dev)
  fuse_views / reconstruction_scores / fuse_summary / wall_error, evaluate_pairs(fuse=...)
                          no counterpart: the posed views merged into a TSDF volume and its surface cloud, and what a pose error does to
                          it (util.tsdf_fuse_dev / tsdf_surface_dev)
  fuse_views(mesh=True) / mesh_stats / mesh_summary
                          no counterpart: the fused volume as an indexed triangle mesh and what kind of surface it is (util.tsdf_mesh_dev,
                          DESIGN.md 4.18)
  fuse_views(mesh=True, decimate=K) / decimate_mesh / mesh_decimate_summary
                          no counterpart: the mesh decimated by vertex clustering on the volume's grid (util.mesh_decimate_dev /
                          mesh_decimate_volume_dev)
  fuse_views(mesh=True, min_component=N) / mesh_component_stats / clean_mesh / mesh_clean_summary
                          no counterpart: the mesh's connected components and the mesh without the small ones (util.mesh_components_dev /
                          mesh_filter_dev / mesh_clean_dev)
  refine_scene / leave_one_out_state, evaluate_scenes(refine=...)
                          no counterpart: the views' poses refined against the volume the other views fuse into, frame to model
                          (util.tsdf_align_dev)
  render_views / render_scores / render_summary, evaluate_scenes(render=...)
                          no counterpart: the fused volume rendered back into depth, normal and colour panoramas from given poses and
                          compared with the scans pixel by pixel (util.tsdf_render_dev)
  synchronize_scene / absolute_pose_errors / evaluate_scenes / scenes_summary
                          no counterpart: a scene's relative poses synchronised into one pose per view, which pair estimates that
                          distrusts, and the scene fused under the result (util.pose_graph / pose_sync_dev)

The metrics are host numpy like the reference's (a handful of 3x3 products per pair); overlap and pc_nearest of a batch come from one
grid-based GPU call (util.point_cloud_overlap_dev), bitwise the values of the per-pair brute-force yardstick
util.point_cloud_overlap."""
import numpy as np

OVERLAPS = ("0-0.1", "0.1-0.5", "0.5-1.0")       # evaluation.py:68


def angular_distance_np(R_hat, R):
    """util.py:176-187 (degrees); R_hat, R: [n,3,3] or [3,3]."""
    R_hat = np.asarray(R_hat)
    R = np.asarray(R)
    if R_hat.shape == (3, 3):
        R_hat = R_hat[np.newaxis, :]
    if R.shape == (3, 3):
        R = R[np.newaxis, :]
    n = R.shape[0]
    trace = np.matmul(R_hat, R.transpose(0, 2, 1)).reshape(n, -1)[:, [0, 4, 8]].sum(1)
    return np.arccos(((trace - 1) / 2).clip(-1, 1)) / np.pi * 180.0


def pose_errors(R_hat_44, R_gt_44, pc_src):
    """evaluation.py:291-297 -> (err_ad, err_t, err_blind, err_t_blind)."""
    t_hat, R_hat = R_hat_44[:3, 3], R_hat_44[:3, :3]
    R_gt = R_gt_44[:3, :3]
    ad = angular_distance_np(R_hat, R_gt[np.newaxis, :, :])[0]
    ad_blind = angular_distance_np(R_gt[np.newaxis, :, :], np.eye(3)[np.newaxis, :, :])[0]
    tr = np.linalg.norm(np.matmul((R_hat - R_gt), np.asarray(pc_src).mean(0).reshape(3)) + t_hat - R_gt_44[:3, 3])
    tr_blind = np.linalg.norm(t_hat - R_gt_44[:3, 3])
    return ad, tr, ad_blind, tr_blind


def overlap_bucket(overlap_val):
    """evaluation.py:187-192."""
    return '0-0.1' if overlap_val <= 0.1 else ('0.1-0.5' if overlap_val <= 0.5 else '0.5-1.0')


def result_record(img_src, img_tgt, R_hat_44, R_gt_44, pc_src, overlap_val, pc_dist, cam_dist, pc_nn):
    """One ``error_stats`` entry with the reference's keys (evaluation.py:299-305)."""
    ad, tr, ad_blind, tr_blind = pose_errors(R_hat_44, R_gt_44, pc_src)
    R_pred_44 = np.eye(4)
    R_pred_44[:3, :3] = R_hat_44[:3, :3]
    R_pred_44[:3, 3] = R_hat_44[:3, 3]
    return {'img_src': img_src, 'img_tgt': img_tgt, 'err_ad': ad, 'err_t': tr, 'err_blind': ad_blind, 'err_t_blind': tr_blind,
            'overlap': overlap_val, 'pc_dist': pc_dist, 'cam_dist': cam_dist, 'pc_nearest': pc_nn, 'R_gt': np.asarray(R_gt_44),
            'R_pred_44': R_pred_44}


def save_results(path, error_stats):
    """evaluation.py:319-320: ``np.save(f"{exp_dir}/{exp}.result.npy", error_stats)`` (an object array of dicts)."""
    if not path.endswith(".npy"):
        path += ".npy"
    np.save(path, np.array(list(error_stats), dtype=object), allow_pickle=True)
    return path


def load_results(path):
    return list(np.load(path, allow_pickle=True))


def summarize(error_stats):
    """Per overlap bucket: number of pairs, mean rotation / translation error (evaluation.py:321-327)."""
    out = {}
    for ov in OVERLAPS:
        rows = [e for e in error_stats if overlap_bucket(e['overlap']) == ov]
        out[ov] = {"nobs": len(rows), "rot_mean": float(np.mean([e['err_ad'] for e in rows])) if rows else float('nan'),
                   "trans_mean": float(np.mean([e['err_t'] for e in rows])) if rows else float('nan')}
    return out


NORMAL_ERR_BINS = 18000            # 0.01 degree bins over 0..180


def normal_error_hist(est, given):
    """Histogram (NORMAL_ERR_BINS bins over 0..180 degrees, float64 counts, on the device) of the angle between two normal maps
    [n,3,h,w] over the pixels where both are non-zero, i.e. valid in both."""
    import torch
    e, g = est.double(), given.double()
    le, lg = e.norm(dim=1), g.norm(dim=1)
    both = (le > 0) & (lg > 0)
    cos = ((e * g).sum(1)[both] / (le[both] * lg[both])).clamp(-1.0, 1.0)
    return torch.histc(torch.rad2deg(torch.acos(cos)), NORMAL_ERR_BINS, 0.0, 180.0)


def hist_quantile(hist, q):
    """The upper edge, in degrees, of the bin in which the cumulative count of a normal_error_hist reaches the share q (nan if it is empty)."""
    h = np.asarray(hist, np.float64)
    if h.sum() <= 0:
        return float("nan")
    return float((np.searchsorted(np.cumsum(h), q * h.sum()) + 1) * 180.0 / len(h))


def _prepare_batch(pipe, batch, device, normals="given", normal_hist=None):
    """pipe.prepare for a DataLoader-layout batch dict under either keypoint mode: keypoints="given" reads "pts" / "ptw" (injected
    keypoints), keypoints="reference" reads "sift" = [(source detections [n,2], target detections [m,2])] * B in panorama coordinates
    (rputil.map_detections of the SIFT detector's output, rputil.py:152-172) and optionally "kp_seeds" [B][levels]: every level then derives
    its keypoints from its own feature maps, as evaluation.py:278 does through getMatchingPrimitive.
    normals="estimated": the batch's normal maps are not used; the pipeline estimates them from the depth (prepare(rgb, None, depth, ...)).
    normal_hist: a one-element list that then accumulates normal_error_hist of the estimate against the batch's own "norm"."""
    if normals not in ("given", "estimated"):
        raise ValueError("normals must be 'given' or 'estimated'")
    norm = batch["norm"] if normals == "given" else None
    if getattr(pipe, "keypoints", "given") == "reference":
        st = pipe.prepare(batch["rgb"], norm, batch["depth"], None, None, device, sift=batch["sift"], kp_seeds=batch.get("kp_seeds"),
                          rgb_full=batch.get("rgb_full"))
    else:
        st = pipe.prepare(batch["rgb"], norm, batch["depth"], batch["pts"], batch["ptw"], device)
    if norm is None and normal_hist is not None and batch.get("norm") is not None:
        import torch
        given = torch.from_numpy(np.ascontiguousarray(batch["norm"], dtype=np.float32)).to(device).reshape(st["norm"].shape)
        hist = normal_error_hist(st["norm"], given)
        normal_hist[0] = hist if normal_hist[0] is None else normal_hist[0] + hist
    return st


def _pair_overlap_stats(pcs_dev, valid_dev, R_gts):
    """overlap and pc_nearest of every pair of a batch from ONE util.point_cloud_overlap_dev call (pcs_dev [2B,P,3], valid_dev [2B,P] on
    the device, R_gts [B,4,4] host) -> two float64 numpy arrays [B], bitwise util.point_cloud_overlap's values."""
    from . import util
    ov, _, _, nn = util.point_cloud_overlap_dev(pcs_dev, valid_dev, np.asarray(R_gts, dtype=np.float64).reshape(-1, 4, 4))
    return ov.cpu().numpy(), nn.cpu().numpy()


def _host_pair_stats(pc_src, pc_tgt, R_gt_44):
    """cam_dist and pc_dist of util.point_cloud_overlap (util.py:36-39), its host expressions: (cam_dist, pc_dist)."""
    R = np.ascontiguousarray(R_gt_44, dtype=np.float64)
    src_trans = np.matmul(R[:3, :3], pc_src.T) + R[:3, 3:4]
    return np.linalg.norm(R[:3, 3]), np.linalg.norm(src_trans.mean(1) - pc_tgt.T.mean(1))


def select_pose(scores):
    """Which of K candidate poses per pair the visibility check prefers (host code): scores = util.visibility_scores' dict with entries
    [B,K] (tensors or arrays) -> int64 numpy [B], the index of the candidate with the highest agreement; ties go to the lower
    violation_rate, then to the lower index.  A NaN agreement ranks last (among NaNs: the lower violation_rate, a NaN one last, then the
    lower index)."""
    host = lambda v: np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v, dtype=np.float64)
    ag, vr = host(scores["agreement"]), host(scores["violation_rate"])
    if ag.ndim != 2 or ag.shape != vr.shape or ag.shape[1] < 1:
        raise ValueError("select_pose takes agreement and violation_rate [B,K] with K >= 1")
    key = lambda b, k: (np.isnan(ag[b, k]), 0.0 if np.isnan(ag[b, k]) else -ag[b, k], np.isnan(vr[b, k]), 0.0 if np.isnan(vr[b, k]) else vr[b, k], k)
    return np.array([min(range(ag.shape[1]), key=lambda k: key(b, k)) for b in range(ag.shape[0])], dtype=np.int64)


VERIFY_MODES = ("observed", "completed")


def _verify_depth(pipe, st, verify, kept):
    """The reference panoramas of the visibility check, [2B,h,4h] f32 on the device.  "observed": the depth under the pipeline's mask, channel 6
    of util.build_view_dev's output (zero outside the mask): only what the method itself was given.  "completed": the last level's composed
    depth (1 - m) f[6] + m observed depth, from what run(keep=...) retained."""
    import torch
    from . import synth, util
    if verify == "observed":
        return util.build_view_dev(st["rgb"], st["norm"], st["depth"], pipe.mask_method)[:, 6].contiguous()
    y0, y1, x0, x1 = synth.observed_box(pipe.mask_method, st["h"])
    m = torch.zeros_like(st["depth"][0])
    m[y0:y1, x0:x1] = 1                                    # the pipeline's mask (util.apply_mask)
    return ((1 - m) * kept[-1]["f"][:, 6] + m * st["depth"]).contiguous()


def _verify_fields(pipe, st, verify, kept, trace, pcs, valid):
    """Per pair the record fields of evaluate_pairs(verify=...): ONE util.pose_visibility_dev call scores every level's pose of every pair."""
    from . import util
    levels = np.stack([t.cpu().numpy() for t in trace], 1)                                 # [B,L,4,4]
    counts, _, sc = util.pose_visibility_dev(pcs, valid, _verify_depth(pipe, st, verify, kept), levels, pipe.dataset)
    pick = select_pose(sc)
    counts = counts.sum(2).cpu().numpy()                                                   # both directions added
    sc = {k: v.cpu().numpy() for k, v in sc.items()}
    last = levels.shape[1] - 1
    return [{'vis_agreement': float(sc["agreement"][b, last]), 'vis_violation_rate': float(sc["violation_rate"][b, last]),
             'vis_observed': float(sc["observed"][b, last]), 'vis_counts': counts[b, last].copy(), 'vis_level': int(pick[b]),
             'R_pred_44_selected': levels[b, pick[b]].copy()} for b in range(levels.shape[0])]


def evaluate_pairs(pipe, batches, device, result_path=None, names=None, normals="given", verify=None, fuse=None):
    """The reference's evaluation loop (evaluation.py:203-320) over an iterable of batches
    ``{"rgb","norm","depth","R" [B,2,4,4], "pts" [B,2,N,2], "ptw" [B,2,N]}`` (the DataLoader dict layout, batched, with the
    injected keypoints; with RelativePosePipeline(keypoints="reference") a batch carries "sift" detections instead, _prepare_batch):
    R_gt = R_t inv(R_s) (:185), overlap statistics from the observed clouds (util.parse_data +
    point_cloud_overlap), the recurrent pipeline on the GPU, then one result record per pair.
    normals="estimated": a batch needs no "norm"; the normal maps are estimated from the depth panoramas (util.depth_normals_dev).
    verify="observed" / "completed": every record gains the visibility check of its pose: the observed clouds of both views
    against the partner's reference panorama (_verify_depth) -- vis_agreement, vis_violation_rate, vis_observed, vis_counts [6] (both
    directions added) for the final pose, vis_level = the level select_pose picks among the per-level poses, R_pred_44_selected = that
    level's pose.  verify=None: the records are what they were.
    fuse=voxel: every record gains what its pose does to the reconstruction (_fuse_fields): fuse_accuracy, fuse_completeness
    (the pair's observed views fused under the estimate against the same fusion under R_gt) and fuse_points.  fuse=None: nothing changes."""
    from . import util
    if verify is not None and verify not in VERIFY_MODES:
        raise ValueError(f"verify must be None or one of {VERIFY_MODES}")
    if fuse is not None and not (np.isfinite(fuse) and fuse > 0):
        raise ValueError("fuse must be None or a voxel size > 0")
    stats = []
    k = 0
    for batch in batches:
        B = batch["rgb"].shape[0]
        st = _prepare_batch(pipe, batch, device, normals)
        kept = [] if verify == "completed" else None
        pose, status, trace = pipe.run(st, keep=kept)
        pose = pose.cpu().numpy()
        pcs, valid = util.depth2pc_dev(st["depth"], pipe.dataset)
        R_gts = [np.matmul(batch["R"][b, 1], np.linalg.inv(batch["R"][b, 0])) for b in range(B)]
        ovs, nns = _pair_overlap_stats(pcs, valid, R_gts)
        vis = _verify_fields(pipe, st, verify, kept, trace, pcs, valid) if verify is not None else None
        fus = _fuse_fields(_verify_depth(pipe, st, "observed", None), pose, R_gts, pipe.dataset, fuse) if fuse is not None else None
        pcs, valid = pcs.cpu().numpy(), valid.cpu().numpy().astype(bool)
        for b in range(B):
            R_gt_44 = R_gts[b]
            pc_src, pc_tgt = pcs[2 * b][valid[2 * b]], pcs[2 * b + 1][valid[2 * b + 1]]
            ov, pc_nn = ovs[b], nns[b]
            cam_dist, pc_dist = _host_pair_stats(pc_src, pc_tgt, R_gt_44)
            nm = names[k] if names is not None else (f"pair{k}/src", f"pair{k}/tgt")
            stats.append(result_record(nm[0], nm[1], pose[b], R_gt_44, pc_src, ov, pc_dist, cam_dist, pc_nn))
            if vis is not None:
                stats[-1].update(vis[b])
            if fus is not None:
                stats[-1].update(fus[b])
            k += 1
    if result_path is not None:
        save_results(result_path, stats)
    return stats


def spearman(a, b):
    """Spearman's rank correlation of two sequences (numpy ranks, ties averaged); pairs with a NaN are left out; NaN when fewer than two pairs
    remain or a side is constant."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    ok = ~(np.isnan(a) | np.isnan(b))
    a, b = a[ok], b[ok]
    if a.size < 2:
        return float("nan")

    def rank(x):
        order = np.argsort(x, kind="stable")
        r = np.empty(x.size)
        r[order] = np.arange(x.size, dtype=np.float64)
        _, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)
        return (np.bincount(inv, r) / cnt)[inv]

    ra, rb = rank(a) - rank(a).mean(), rank(b) - rank(b).mean()
    den = np.sqrt((ra * ra).sum() * (rb * rb).sum())
    return float((ra * rb).sum() / den) if den > 0 else float("nan")


def verify_summary(stats):
    """What the CLI reports about records that carry the visibility fields: the Spearman rank correlation of vis_agreement with err_ad and
    with err_t, and per overlap bucket the mean rotation error of the selected level next to that of the last level."""
    ag = [e['vis_agreement'] for e in stats]
    out = {"vis_spearman_rot": spearman(ag, [e['err_ad'] for e in stats]), "vis_spearman_trans": spearman(ag, [e['err_t'] for e in stats]),
           "vis_selected": {}}
    for ov in OVERLAPS:
        rows = [e for e in stats if overlap_bucket(e['overlap']) == ov]
        if rows:
            sel = [angular_distance_np(e['R_pred_44_selected'][:3, :3].reshape(1, 3, 3), e['R_gt'][:3, :3].reshape(1, 3, 3))[0] for e in rows]
            out["vis_selected"][ov] = {"nobs": len(rows), "err_ad_last": float(np.mean([e['err_ad'] for e in rows])),
                                       "err_ad_selected": float(np.mean(sel))}
    return out


def fuse_views(depth, rgb, R, dataset, voxel, trunc=None, pad=3, min_weight=1, max_points=None, view_begin=None, mesh=False, min_component=None,
               decimate=None):
    """Merge posed depth panoramas into one surface cloud per scene: depth [V,h,4h] f32 and rgb [V,3,h,4h] f32 (or None)
    CUDA tensors, R [V,4,4] host float64 world -> camera poses (the loaders' R), view_begin as util.tsdf_fuse_dev's (None: one scene).  The box
    is util.tsdf_bounds_dev's, the volume util.tsdf_fuse_dev's, the cloud util.tsdf_surface_dev's.
    -> {"points" [S,cap,3] f64, "normals", "colors" (or None), "valid" [S,cap] u8, "n_points" [S] i32, "origin", "dims", "voxel", "state"}.
    mesh=True: the same five tensors from util.tsdf_mesh_dev, and "triangles" [S,cap_tri,3] i32, "n_triangles" [S] i32.
    min_component=N (with mesh=True): the mesh without its connected components of fewer than N triangles and without unused vertices
    (util.mesh_clean_dev), "vertex_map", and "components": mesh_clean_dev's description of the mesh before the cleaning.
    decimate=K (with mesh=True, an integer >= 1): the mesh decimated by vertex clustering on the volume's grid coarsened by K
    (util.mesh_decimate_volume_dev), after the cleaning when both are given: its mesh tensors, "vertex_map", "tri_map", "count"
    and the four counters replace the mesh's (the maps are relative to the mesh that was decimated), and "decimated_from": (n_points,
    n_triangles) [S] i32 tensors of that mesh."""
    from . import util
    vb = np.array([0, int(depth.shape[0])], np.int32) if view_begin is None else view_begin
    origin, dims = util.tsdf_bounds_dev(depth, R, dataset, voxel, pad, vb)
    state = util.tsdf_fuse_dev(depth, rgb, R, vb, origin, dims, voxel, dataset, trunc)
    if mesh:
        out = util.tsdf_mesh_dev(state, min_weight, max_points)
        out.update(origin=origin, dims=dims, voxel=float(voxel), state=state)
        if min_component is not None:
            clean, comps = util.mesh_clean_dev(out, min_triangles=int(min_component))
            out.update(clean, components=comps)
        if decimate is not None:
            dec = util.mesh_decimate_volume_dev(out, state, int(decimate))
            out.update(dec, decimated_from=(out["n_points"], out["n_triangles"]))
        return out
    if min_component is not None or decimate is not None:
        raise ValueError("fuse_views: min_component and decimate apply to mesh=True")
    points, normals, colors, valid, n = util.tsdf_surface_dev(state, min_weight, max_points)
    return {"points": points, "normals": normals, "colors": colors, "valid": valid, "n_points": n, "origin": origin, "dims": dims,
            "voxel": float(voxel), "state": state}


def render_views(state, R, dataset=None, h=160, scene_of_view=None, **kw):
    """What the fused model looks like from the world -> camera poses R [V,4,4]: `state` is util.tsdf_fuse_dev's (or
    fuse_views(...)["state"]); dataset defaults to the state's; kw goes to util.tsdf_render_dev (d_min, d_max, step, min_weight, skip).
    -> {"depth" [V,h,4h] f32 (0 = no data), "normal" [V,3,h,4h] f32 (camera frame), "color" [V,3,h,4h] f32 or None, "cls" [V,h,4h] u8}: the
    triple RelativePosePipeline.prepare, util.depth_normals_dev, util.visibility_dev and util.tsdf_fuse_dev take."""
    from . import util
    depth, normal, color, cls = util.tsdf_render_dev(state, R, state["dataset"] if dataset is None else dataset, h, scene_of_view, **kw)
    return {"depth": depth, "normal": normal, "color": color, "cls": cls}


def render_scores(rendered_depth, cls, measured_depth, voxel):
    """A rendered model view against the scan it stands for, pixel by pixel: -> ((median, p90) of |rendered - measured| in voxels over the
    pixels where both have data (the render a hit, the scan finite and > 0; NaN without such a pixel), coverage = hits / measured pixels: above 1
    where the model fills more holes of the scan than it leaves)."""
    import torch
    rd = torch.as_tensor(rendered_depth)
    md, hit = torch.as_tensor(measured_depth).to(rd.device), torch.as_tensor(cls).to(rd.device) == 1
    have = torch.isfinite(md) & (md > 0)
    both = hit & have
    err = ((rd[both].double() - md[both].double()).abs() / float(voxel)).cpu().numpy()
    n = int(have.sum().item())
    med, p90 = (float(np.median(err)), float(np.percentile(err, 90))) if err.size else (float("nan"), float("nan"))
    return (med, p90), (int(hit.sum().item()) / n if n else float("nan"))


def render_summary(parts, voxel):
    """[(rendered depth, cls, measured depth)] of several scenes -> the CLI's three fields over all their pixels"""
    import torch
    if not parts:
        return {"render_depth_err_median": float("nan"), "render_depth_err_p90": float("nan"), "render_coverage": float("nan")}
    (med, p90), cov = render_scores(torch.cat([p[0].reshape(-1) for p in parts]), torch.cat([p[1].reshape(-1) for p in parts]),
                                    torch.cat([p[2].reshape(-1) for p in parts]), voxel)
    return {"render_depth_err_median": med, "render_depth_err_p90": p90, "render_coverage": cov}


def save_render(path, rv):
    """<exp>.scene<k>.render.npz: depth, normal, colour and cls of render_views"""
    np.savez(path, depth=rv["depth"].cpu().numpy(), normal=rv["normal"].cpu().numpy(), cls=rv["cls"].cpu().numpy(),
             color=np.zeros(0, np.float32) if rv["color"] is None else rv["color"].cpu().numpy())
    return path


def leave_one_out_state(state_all, state_solo):
    """tsdf_fuse_dev's state of all V views in one scene, and of every view alone (V scenes of one view, the same box) -> the state of V
    scenes, scene v = every view but v.  The sums are integers: the difference is exactly what fusing the others gives."""
    out = dict(state_solo)
    for k in ("tsdf_sum", "weight", "color_sum"):
        out[k] = None if state_solo.get(k) is None else state_all[k] - state_solo[k]
    return out


def refine_scene(depth, R, dataset, voxel, rounds=1, leave_one_out=True, iters=12, eig_min=None, stride=1, trunc=None, pad=3, min_weight=1):
    """Refine the poses of one scene's views against the volume they fuse into: depth [V,h,4h] f32 CUDA tensor, R [V,4,4]
    host float64 world -> camera.  Per round: the box (util.tsdf_bounds_dev) and one fusion of all views under the current poses; with
    leave_one_out, every view fused alone in one batched call and subtracted, so that view v is aligned to the volume of the others (a view
    aligned to a volume that holds itself is pulled to where it already is); then every view is aligned in ONE util.tsdf_align_dev call.
    -> {"pose" [V,4,4] host float64, "held" [V], "eig" [V,6], "rms" [V,2] (before the first round's first step, after the last round's last),
    "used" [V] (points used at the last evaluation)}.  rounds=0 returns the poses as given, scored."""
    import torch
    from . import util
    V = int(depth.shape[0])
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(V, 4, 4).copy()
    first = None
    for rnd in range(max(int(rounds), 1)):
        origin, dims = util.tsdf_bounds_dev(depth, R, dataset, voxel, pad)
        state = util.tsdf_fuse_dev(depth, None, R, np.array([0, V], np.int32), origin, dims, voxel, dataset, trunc)
        sov = np.zeros(V, np.int32)
        if leave_one_out and V > 1:
            solo = util.tsdf_fuse_dev(depth, None, R, np.arange(V + 1, dtype=np.int32), np.repeat(origin, V, 0), dims, voxel, dataset, trunc)
            state = leave_one_out_state(state, solo)
            sov = np.arange(V, dtype=np.int32)
        out = util.tsdf_align_dev(state, depth, R, sov, iters if rounds > 0 else 0, eig_min, stride, min_weight=min_weight)
        first = out["rms"][:, 0].cpu().numpy() if first is None else first
        R = out["pose"].cpu().numpy()
    return {"pose": R, "held": out["held"].cpu().numpy(), "eig": out["eig"].cpu().numpy(),
            "rms": np.stack([first, out["rms"][:, 1].cpu().numpy()], 1), "used": out["sums"][:, 31].cpu().numpy()}


def mesh_stats(mesh):
    """What a mesh of fuse_views(mesh=True) / util.tsdf_mesh_dev is, per scene, on the host in float64: -> a list of {"triangles", "area" (the
    sum of |(p1 - p0) x (p2 - p0)| / 2), "border_edges" (undirected edges with one triangle: the rim of the observed surface),
    "nonmanifold_edges" (undirected edges with more than two triangles, or with two that run the same way: expected 0)}."""
    host = lambda v: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    pts, tri, nt = host(mesh["points"]).astype(np.float64), host(mesh["triangles"]).astype(np.int64), host(mesh["n_triangles"])
    out = []
    for s in range(pts.shape[0]):
        t = tri[s, :min(int(nt[s]), tri.shape[1])]
        p = pts[s]
        area = float(np.linalg.norm(np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]), axis=1).sum() * 0.5) if len(t) else 0.0
        d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]) if len(t) else np.zeros((0, 2), np.int64)
        big = int(d.max()) + 1 if len(d) else 1
        und, inv, cnt = np.unique(d.min(1) * big + d.max(1), return_inverse=True, return_counts=True)
        fwd = np.bincount(inv.reshape(-1), weights=(d[:, 0] < d[:, 1]).astype(np.float64), minlength=len(und))      # of them, low -> high
        manifold = (cnt == 1) | ((cnt == 2) & (fwd == 1))
        out.append({"triangles": int(len(t)), "area": area, "border_edges": int((cnt == 1).sum()), "nonmanifold_edges": int((~manifold).sum())})
    return out


def mesh_component_stats(comps):
    """What util.mesh_components_dev / mesh_clean_dev's `comps` (or the model's dict) says per scene, on the host: -> a list of {"components",
    "largest_share": the largest component's share of the labelled triangles (nan without any), "small_triangles": the triangles outside the
    largest component}.  Needs every component's count: cap_comp >= n_components."""
    host = lambda v: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    n, ct = host(comps["n_components"]), host(comps["comp_triangles"]).astype(np.int64)
    if len(n) and int(n.max()) > ct.shape[1]:
        raise ValueError("mesh_component_stats: the statistics are truncated (cap_comp < n_components)")
    out = []
    for s in range(len(n)):
        c = ct[s, :int(n[s])]
        total, top = int(c.sum()), int(c.max()) if len(c) else 0
        out.append({"components": int(n[s]), "largest_share": top / total if total else float("nan"), "small_triangles": total - top})
    return out


def mesh_clean_summary(stats, removed):
    """the CLI's medians of mesh_component_stats and of the triangles --mesh-min-component removed, over scenes"""
    med = lambda v: float(np.nanmedian(v)) if len(v) and not np.all(np.isnan(v)) else float("nan")
    return {"mesh_components_median": med([m["components"] for m in stats]), "mesh_largest_share_median": med([m["largest_share"] for m in stats]),
            "mesh_removed_triangles_median": med(removed)}


def clean_mesh(mesh, min_component):
    """--mesh-min-component: -> (the mesh dict without its components of fewer than min_component triangles, mesh_component_stats of the mesh as
    it came, the number of triangles removed); scene 0 of a one-scene mesh"""
    from . import util
    clean, comps = util.mesh_clean_dev(mesh, min_triangles=int(min_component))
    removed = int(mesh["n_triangles"][0].item()) - int(clean["n_triangles"][0].item())
    return dict(mesh, **clean), mesh_component_stats(comps)[0], removed


def decimate_mesh(mesh, factor):
    """--mesh-decimate: -> (the mesh dict decimated on its volume's grid coarsened by factor (util.mesh_decimate_volume_dev),
    (triangles before, triangles after, dist, within)); scene 0 of a one-scene mesh of fuse_views(mesh=True).  dist: the median distance of
    the mesh's vertices to the vertex that replaced them (through vertex_map, with torch operators); within: the share of the new vertices
    with a vertex of the original surface cloud inside half a cell (one reconstruction_scores call, which is one util.overlap_dev call)."""
    import torch
    from . import util
    dec = util.mesh_decimate_volume_dev(mesh, mesh["state"], int(factor))
    nv = min(max(int(mesh["n_points"][0].item()), 0), int(mesh["points"].shape[1]))
    vm = dec["vertex_map"][0, :nv].long()
    moved = (mesh["points"][0, :nv][vm >= 0] - dec["points"][0][vm[vm >= 0]]).norm(dim=1)
    dist = float(moved.median().item()) if moved.numel() else float("nan")
    within, _ = reconstruction_scores(dec, {"points": mesh["points"], "valid": mesh["valid"]}, 0.5 * dec["decimate_cell"])
    return dict(mesh, **dec), (int(mesh["n_triangles"][0].item()), int(dec["n_triangles"][0].item()), dist, float(within[0]))


def mesh_decimate_summary(parts):
    """the CLI's medians of decimate_mesh's tuples over scenes"""
    med = lambda v: float(np.nanmedian(v)) if len(v) and not np.all(np.isnan(v)) else float("nan")
    share = [p[1] / p[0] if p[0] else float("nan") for p in parts]
    return {"mesh_decimated_triangles_median": med([float(p[1]) for p in parts]), "mesh_decimated_share_median": med(share),
            "mesh_decimated_dist_median": med([p[2] for p in parts]), "mesh_decimated_within_median": med([p[3] for p in parts])}


def mesh_summary(stats):
    """the CLI's medians of mesh_stats over scenes"""
    med = lambda k: float(np.median([m[k] for m in stats])) if stats else float("nan")
    return {"mesh_triangles_median": med("triangles"), "mesh_area_median": med("area"), "mesh_border_edges_median": med("border_edges"),
            "mesh_nonmanifold_edges": int(sum(m["nonmanifold_edges"] for m in stats))}


def reconstruction_scores(est, ref, max_dist=0.08):
    """Accuracy and completeness of fused surfaces against reference surfaces, scene by scene: est, ref = fuse_views' dicts (or any dicts
    with "points" [S,cap,3] f64 and "valid" [S,cap] u8 CUDA tensors) with the same S.  accuracy = the share of est's points with a point of
    ref within max_dist, completeness = the share of ref's points with a point of est within max_dist.  ONE util.overlap_dev call with 2 S
    directed queries under the identity pose.  -> (accuracy [S], completeness [S]) float64 numpy; NaN where the cloud divided by is empty."""
    import torch
    from . import util
    pe, ve, pr, vr = est["points"], est["valid"], ref["points"], ref["valid"]
    S = int(pe.shape[0])
    if int(pr.shape[0]) != S:
        raise ValueError("reconstruction_scores takes as many reference scenes as estimated ones")
    P = max(int(pe.shape[1]), int(pr.shape[1]))
    dev = pe.device
    pc = torch.zeros(2 * S, P, 3, dtype=torch.float64, device=dev)
    valid = torch.zeros(2 * S, P, dtype=torch.uint8, device=dev)
    pc[:S, :pe.shape[1]], valid[:S, :pe.shape[1]] = pe, ve
    pc[S:, :pr.shape[1]], valid[S:, :pr.shape[1]] = pr, vr
    q = np.arange(2 * S)
    eye = torch.eye(4, dtype=torch.float64, device=dev).repeat(2 * S, 1, 1)
    hits, _, n_valid = util.overlap_dev(pc, valid, q, (q + S) % (2 * S), eye, max_dist)
    hits, n = hits.cpu().numpy().astype(np.float64), n_valid.cpu().numpy().astype(np.float64)
    with np.errstate(all="ignore"):
        share = np.where(n > 0, hits / np.where(n > 0, n, 1.0), np.nan)
    return share[:S], share[S:]


def _fuse_fields(depth_obs, poses, R_gts, dataset, voxel, max_dist=0.08):
    """Per pair the record fields of evaluate_pairs(fuse=voxel): the pair's two observed views depth_obs [2B,h,4h] (view 2b = the source)
    fused in the target's frame -- target pose I, source pose inv(R) -- once under the estimate poses[b] and once under R_gts[b]; the
    estimate's surface is scored against the ground truth's (reconstruction_scores).  2 B scenes of 2 views in one fuse call.  A pose that
    cannot be inverted gives NaN scores."""
    import torch
    B = len(R_gts)
    R = np.empty((4 * B, 4, 4))
    bad = np.zeros(B, bool)
    for b in range(B):
        for k, T in enumerate((poses[b], R_gts[b])):
            T = np.vstack([np.asarray(T, np.float64)[:3], [0.0, 0.0, 0.0, 1.0]])
            try:
                inv = np.linalg.inv(T)
            except np.linalg.LinAlgError:
                inv = np.full((4, 4), np.nan)
            if not np.isfinite(inv).all():
                inv, bad[b] = np.eye(4), True
            s = k * B + b
            R[2 * s], R[2 * s + 1] = inv, np.eye(4)
    idx = torch.tensor([2 * (s % B) + v for s in range(2 * B) for v in range(2)], device=depth_obs.device)
    surf = fuse_views(depth_obs[idx].contiguous(), None, R, dataset, voxel, view_begin=np.arange(0, 4 * B + 1, 2, dtype=np.int32))
    half = lambda lo, hi: {"points": surf["points"][lo:hi], "valid": surf["valid"][lo:hi]}
    acc, comp = reconstruction_scores(half(0, B), half(B, 2 * B), max_dist)
    n = surf["n_points"].cpu().numpy()
    return [{'fuse_accuracy': float("nan") if bad[b] else float(acc[b]), 'fuse_completeness': float("nan") if bad[b] else float(comp[b]),
             'fuse_points': int(n[b])} for b in range(B)]


def fuse_summary(stats):
    """What the CLI reports about records that carry the fusion fields: the medians, and the Spearman rank correlation of fuse_accuracy with
    the rotation error."""
    acc, comp = [e['fuse_accuracy'] for e in stats], [e['fuse_completeness'] for e in stats]
    med = lambda v: float(np.nanmedian(v)) if len(v) and not np.all(np.isnan(v)) else float("nan")
    return {"fuse_accuracy_median": med(acc), "fuse_completeness_median": med(comp), "fuse_points_median": med([e['fuse_points'] for e in stats]),
            "fuse_spearman_rot": spearman(acc, [e['err_ad'] for e in stats])}


def wall_error(points, half, voxel):
    """Distance of points [N,3] (world frame of synth.render_scene: the room is the box |x_a| <= half_a) to the nearest wall plane, in voxels."""
    return np.abs(np.abs(np.asarray(points, np.float64)) - np.asarray(half, np.float64)[None]).min(1) / float(voxel)


def evaluate_from_frames(pipe, batches, device, Hf=480, Wf=640):
    """The pose evaluation from perspective frames alone, next to the same pairs' directly rendered panoramas: for every SyntheticBatch
    the pairs' rooms are rendered as one Hf x Wf frame per view (synth.render_frames: identity frame pose, util.SCANNET_FRAME_SCALE), the
    panoramas are built and their normals estimated on the GPU (RelativePosePipeline.prepare_frames) and the recurrent
    pipeline runs on them; the second route is prepare(rgb, None, depth, ...) on the rendered panoramas, so that the frames are the only
    difference.  Returns (records from frames, records from the rendered panoramas, relative depth errors of the built panorama against the
    rendered one over the pixels of the observed box that have data in both, float64 numpy)."""
    from . import synth, util
    recs_f, recs_d, errs = [], [], []
    y0, y1, x0, x1 = synth.observed_box(pipe.mask_method, 160)
    k = 0
    for sb in batches:
        batch = sb.take(range(sb.size))
        B = batch["rgb"].shape[0]
        fr = [synth.render_frames(None, batch["R"][b], synth.room_half(sb.seed + b), Hf, Wf) for b in range(B)]
        depth_full = np.stack([f[0][:, 0] for f in fr])
        rgb_full = np.stack([np.moveaxis(f[1][:, 0], -1, 1) for f in fr])
        st_f = pipe.prepare_frames(rgb_full, depth_full, batch["pts"], batch["ptw"], device)
        pose_f = pipe.run(st_f)[0].cpu().numpy()
        st_d = pipe.prepare(batch["rgb"], None, batch["depth"], batch["pts"], batch["ptw"], device)
        pose_d = pipe.run(st_d)[0].cpu().numpy()
        df, dd = st_f["depth"][:, y0:y1, x0:x1].double(), st_d["depth"][:, y0:y1, x0:x1].double()
        both = (df > 0) & (dd > 0)
        errs.append(((df - dd).abs() / dd.clamp(min=1e-12))[both].cpu().numpy())
        pcs, valid = util.depth2pc_dev(st_d["depth"], pipe.dataset)
        R_gts = [np.matmul(batch["R"][b, 1], np.linalg.inv(batch["R"][b, 0])) for b in range(B)]
        ovs, nns = _pair_overlap_stats(pcs, valid, R_gts)
        pcs, valid = pcs.cpu().numpy(), valid.cpu().numpy().astype(bool)
        for b in range(B):
            R_gt_44 = R_gts[b]
            pc_src, pc_tgt = pcs[2 * b][valid[2 * b]], pcs[2 * b + 1][valid[2 * b + 1]]
            ov, pc_nn = ovs[b], nns[b]
            cam_dist, pc_dist = _host_pair_stats(pc_src, pc_tgt, R_gt_44)
            for recs, pose in ((recs_f, pose_f), (recs_d, pose_d)):
                recs.append(result_record(f"pair{k}/src", f"pair{k}/tgt", pose[b], R_gt_44, pc_src, ov, pc_dist, cam_dist, pc_nn))
            k += 1
    return recs_f, recs_d, np.concatenate(errs) if errs else np.zeros(0)


class SyntheticBatch:
    """A global batch of `size` seeded synthetic scan pairs (synth.make_pairs / make_keypoints conventions: pair b of the batch comes from
    seed + b) that materialises only the pairs a rank asks for -- evaluate_pairs_sharded hands every rank the same batch list, and a rank
    should not render the other ranks' panoramas."""

    def __init__(self, size, seed, dataset, mask_method, keypoints, h=160, sift=0, sift_detector="synthetic"):
        self.size, self.seed, self.dataset, self.mask_method, self.keypoints, self.h = size, seed, dataset, mask_method, keypoints, h
        self.sift = int(sift)           # > 0: also `sift` synthetic SIFT detections per view (for RelativePosePipeline(keypoints="reference"))
        # "gpu": no synthetic detections; the pipeline runs the HIP SIFT detector on the rendered views (prepare(sift="detect"))
        self.sift_detector = sift_detector

    def take(self, idx):
        from . import synth
        parts = [synth.make_pairs(1, self.seed + int(b), self.dataset, h=self.h) for b in idx]
        # (both seeds are functions of the GLOBAL pair index seed + b only: the same pair gets the same panoramas and keypoints under any
        # --batch, so result files are comparable / resumable across batch sizes)
        kps = [synth.make_keypoints(1, self.keypoints, 7919 * (self.seed + int(b)) + 13, self.mask_method, h=self.h) for b in idx]
        out = {k: np.concatenate([p[k] for p in parts]) for k in ("rgb", "norm", "depth", "R")}
        out["pts"], out["ptw"] = np.concatenate([k[0] for k in kps]), np.concatenate([k[1] for k in kps])
        if self.sift and self.sift_detector == "gpu":
            out["sift"] = "detect"
            if self.mask_method == "kinect":
                out["rgb_full"] = synth.kinect_frames(out["rgb"], self.h)
            out["kp_seeds"] = [[31 * (self.seed + int(b)) + lvl for lvl in range(8)] for b in idx]
        elif self.sift:
            from . import rputil
            dets = [synth.make_sift_detections(1, self.sift, 15485863 * (self.seed + int(b)) + 7, self.mask_method, self.h)[0] for b in idx]
            out["sift"] = [(rputil.map_detections(a, self.mask_method, self.h), rputil.map_detections(c, self.mask_method, self.h)) for a, c in dets]
            out["kp_seeds"] = [[31 * (self.seed + int(b)) + lvl for lvl in range(8)] for b in idx]
        return out


def pairs_from_overlap(frac, base, ids, min_overlap=None):
    """The pair list of one scene from its directed overlap matrix (host code): frac [M,M] (frac[i,j] = the share of view i's points
    that view j also sees, util.overlap_matrix_dev), base = the scene's name, ids = the M view ids -> the loaders' dataList entries
    {'base', 'id_src', 'id_tgt', 'overlap'} (datasets/SUNCG.py:91-93) for i < j, sorted by (i, j); overlap = max(frac[i,j], frac[j,i]),
    the symmetric value util.point_cloud_overlap reports.  min_overlap: pairs below it are left out (the baselines' rule is 0.1,
    evaluation.py:190-191)."""
    f = np.asarray(frac, dtype=np.float64)
    M = len(ids)
    if f.shape != (M, M):
        raise ValueError("pairs_from_overlap takes frac [M,M] and M ids")
    out = []
    for i in range(M):
        for j in range(i + 1, M):
            ov = float(max(f[i, j], f[j, i]))
            if min_overlap is not None and ov < min_overlap:
                continue
            out.append({'base': base, 'id_src': ids[i], 'id_tgt': ids[j], 'overlap': ov})
    return out


def observed_depth(depth, dataset):
    """depth [n,h,4h] f32 tensor -> the same with everything outside the dataset's observed box zeroed (the kinect window for scannet, the
    second face otherwise): channel 6 of util.build_view_dev's output, the reference panorama of verify="observed"."""
    import torch
    from . import synth
    y0, y1, x0, x1 = synth.observed_box("kinect" if "scannet" in dataset else "second", depth.shape[1])
    out = torch.zeros_like(depth)
    out[:, y0:y1, x0:x1] = depth[:, y0:y1, x0:x1]
    return out


def mine_pairs(depth, R, dataset, base, ids=None, min_overlap=None, max_dist=0.08, device=None, verify=None):
    """Which pairs of M posed scans of one scene overlap, and by how much: depth [M,h,4h] float32 panoramas (numpy or a CUDA tensor),
    R [M,4,4] world -> camera poses (the loaders' convention) -> pairs_from_overlap's entries.  The observed clouds (util.depth2pc_dev),
    ONE grid-based overlap call over the M (M - 1) directed pairs (util.overlap_matrix_dev) and the host pair list.
    verify="observed": every entry gains 'vis_agreement', the visibility agreement of the pair under its poses with both directions pooled
    (util.visibility_matrix_dev on the observed clouds against the observed depth; NaN when no point of either lands on data)."""
    import torch
    from . import _lib, util
    if verify not in (None, "observed"):
        raise ValueError("mine_pairs takes verify=None or 'observed'")
    dev = device if device is not None else _lib.require_gpu()
    d = depth if isinstance(depth, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(dev)
    pc, valid = util.depth2pc_dev(d, dataset)
    frac, _, _ = util.overlap_matrix_dev(pc, valid, R, max_dist)
    M = d.shape[0]
    ids = list(range(M)) if ids is None else list(ids)
    out = pairs_from_overlap(frac.cpu().numpy(), base, ids, min_overlap)
    if verify is not None:
        counts, margin, _ = util.visibility_matrix_dev(pc, valid, observed_depth(d, dataset), R, dataset)
        ag = util.visibility_scores(counts + counts.transpose(0, 1), margin + margin.transpose(0, 1))["agreement"].cpu().numpy()
        pos = {v: k for k, v in enumerate(ids)}
        for e in out:
            e['vis_agreement'] = float(ag[pos[e['id_src']], pos[e['id_tgt']]])
    return out


def save_data_list(path, lists):
    """Write {split: [entries]} as the object file the reference's loaders read with np.load(path).item()[split]
    (datasets/SUNCG.py:66).  -> the path written (.npy appended when missing)."""
    if not path.endswith(".npy"):
        path += ".npy"
    np.save(path, {k: list(v) for k, v in lists.items()}, allow_pickle=True)
    return path


def load_data_list(path, split):
    return np.load(path, allow_pickle=True).item()[split]


class SceneBatch:
    """The take(idx) counterpart of SyntheticBatch whose pairs OVERLAP: `size` pairs mined (mine_pairs) from synth.render_scene scenes of
    `views` views each, scene after scene (scene s of the batch has seed 7919 * seed + s) in (scene, i, j) order.  balanced: equal
    numbers from the three overlap buckets instead, taken round-robin (0-0.1, 0.1-0.5, 0.5-1.0, 0-0.1, ...) in that order from as many
    scenes as it takes -- so that a synthetic summary has populated rows; at most `max_scenes` scenes are rendered, and a bucket that
    stays short is filled from the others.  The pair list is built on first use (it needs the GPU); `pairs` holds its entries, with
    'base' = the scene's seed."""

    def __init__(self, size, seed, dataset, mask_method, keypoints, h=160, views=6, balanced=False, max_scenes=64):
        self.size, self.seed, self.dataset, self.mask_method, self.keypoints, self.h = size, seed, dataset, mask_method, keypoints, h
        self.views, self.balanced, self.max_scenes = int(views), bool(balanced), int(max_scenes)
        self.pairs = None
        self._scenes = {}

    def _scene(self, s):
        from . import synth
        if s not in self._scenes:
            self._scenes[s] = synth.render_scene(7919 * self.seed + s, self.views, self.dataset, self.h)
        return self._scenes[s]

    def _mine(self):
        if self.pairs is not None:
            return
        buckets = {k: [] for k in OVERLAPS}
        flat = []
        want = -(-self.size // 3)
        for s in range(self.max_scenes):
            sc = self._scene(s)
            found = mine_pairs(sc["depth"], sc["R"], self.dataset, 7919 * self.seed + s)
            for e in found:
                e['scene'] = s
                buckets[overlap_bucket(e['overlap'])].append(e)
            flat += found
            if (not self.balanced and len(flat) >= self.size) or (self.balanced and all(len(v) >= want for v in buckets.values())):
                break
        if self.balanced:
            picked, rest = [], []
            for r in range(max(len(v) for v in buckets.values())):
                for k in OVERLAPS:
                    if r < len(buckets[k]):
                        (picked if r < want else rest).append(buckets[k][r])
            flat = picked + rest
        if len(flat) < self.size:
            raise RuntimeError(f"SceneBatch: {len(flat)} pairs from {self.max_scenes} scenes of {self.views} views, {self.size} wanted")
        self.pairs = flat[:self.size]
        used = {e['scene'] for e in self.pairs}
        self._scenes = {s: v for s, v in self._scenes.items() if s in used}

    def take(self, idx):
        from . import synth
        self._mine()
        out = {k: [] for k in ("rgb", "norm", "depth", "R")}
        for b in idx:
            e = self.pairs[int(b)]
            sc, ij = self._scene(e['scene']), [e['id_src'], e['id_tgt']]
            for k in out:
                out[k].append(sc[k][ij])
        out = {k: np.stack(v) for k, v in out.items()}
        kps = [synth.make_keypoints(1, self.keypoints, 7919 * (self.seed + int(b)) + 13, self.mask_method, h=self.h) for b in idx]
        out["pts"], out["ptw"] = np.concatenate([k[0] for k in kps]), np.concatenate([k[1] for k in kps])
        return out


def _batch_size(batch):
    return batch.size if hasattr(batch, "take") else batch["rgb"].shape[0]


def _batch_take(batch, idx):
    """The pairs `idx` of a global batch as a dict of arrays (a dict batch is sliced, a lazy one renders them)."""
    if hasattr(batch, "take"):
        return batch.take(idx)
    out = {k: v[idx] for k, v in batch.items() if isinstance(v, np.ndarray)}
    for k in ("sift", "kp_seeds"):                        # per-pair lists (keypoints="reference")
        if k in batch and isinstance(batch[k], str):      # sift="detect": the pipeline detects on the batch's own views
            out[k] = batch[k]
        elif k in batch:
            out[k] = [batch[k][int(i)] for i in idx]
    return out


def _default_record(pipe, sub, poses, device, names, ks):
    """Result records (the reference's keys, evaluation.py:286-305) of the pairs of `sub` (a _batch_take dict), given their poses
    [n,4,4] (host) and their global pair indices `ks`: overlap statistics from the observed clouds, then the error metrics."""
    from . import util
    import torch
    n = len(ks)
    depth = torch.from_numpy(np.ascontiguousarray(sub["depth"].reshape(2 * n, *sub["depth"].shape[2:]))).to(device)
    pcs, valid = util.depth2pc_dev(depth, pipe.dataset)
    R_gts = [np.matmul(sub["R"][q, 1], np.linalg.inv(sub["R"][q, 0])) for q in range(n)]
    ovs, nns = _pair_overlap_stats(pcs, valid, R_gts)
    pcs, valid = pcs.cpu().numpy(), valid.cpu().numpy().astype(bool)
    out = []
    for q in range(n):
        R_gt_44 = R_gts[q]
        pc_src, pc_tgt = pcs[2 * q][valid[2 * q]], pcs[2 * q + 1][valid[2 * q + 1]]
        ov, pc_nn = ovs[q], nns[q]
        cam_dist, pc_dist = _host_pair_stats(pc_src, pc_tgt, R_gt_44)
        nm = names[ks[q]] if names is not None else (f"pair{ks[q]}/src", f"pair{ks[q]}/tgt")
        out.append(result_record(nm[0], nm[1], poses[q], R_gt_44, pc_src, ov, pc_dist, cam_dist, pc_nn))
    return out


def evaluate_fgs(batches, device, dataset, result_path=None, max_points=None, seed=0, verify=None, fuse=None):
    """The reference's `--method fgs` loop (evaluation.py:182-203, 286-320) over batches of synthetic pairs: the observed-block clouds
    of both views (util.depth2pc_dev, as _default_record builds them), ONE batched FPFH + fast global registration call per batch
    (baselines.fast_global_registration_dev), then per pair the overlap statistics; pairs with overlap < 0.1 are skipped without a
    record (evaluation.py:190-191).  Returns the record list (the reference's keys + 'status'); written to result_path if given."""
    from . import _lib, baselines
    reg = lambda pcs, valid: baselines.fast_global_registration_dev(pcs, valid, max_points=max_points or _lib.FGR_MAX_POINTS, seed=seed)[:2]
    return _evaluate_baseline(batches, device, dataset, reg, result_path, verify=verify, fuse=fuse)


def evaluate_gs(batches, device, dataset, result_path=None, max_points=None, seed=0, verify=None, fuse=None):
    """The reference's `--method gs` loop: as evaluate_fgs, with ONE batched FPFH + RANSAC call per batch
    (baselines.global_registration_dev, baselines.py:52-81)."""
    from . import _lib, baselines
    reg = lambda pcs, valid: baselines.global_registration_dev(pcs, valid, max_points=max_points or _lib.FGR_MAX_POINTS, seed=seed)[:2]
    return _evaluate_baseline(batches, device, dataset, reg, result_path, verify=verify, fuse=fuse)


def evaluate_cgs(batches, device, dataset, result_path=None, max_points=None, seed=0, verify=None, fuse=None):
    """The reference's `--method cgs` loop: as evaluate_gs, with the RANSAC pose of every pair refined by the three coloured ICP levels
    (baselines.color_registration_dev, baselines.py:110-168).  The colours are the observed block of `rgb` in the clouds' point order,
    quantised as the reference does: clip(rgb * 255, 0, 255) to uint8 (evaluation.py:168), then / 255 (util.py:53)."""
    from . import _lib, baselines
    reg = lambda pcs, valid, colors: baselines.color_registration_dev(pcs, colors, valid, max_points=max_points or _lib.FGR_MAX_POINTS, seed=seed)[:2]
    return _evaluate_baseline(batches, device, dataset, reg, result_path, with_colors=True, verify=verify, fuse=fuse)


def observed_colors(rgb):
    """rgb [n,3,h,4h] float numpy in [0, 1] -> [n, h*h, 3] f64: the observed block (columns h:2h) in util.depth2pc_dev's point order
    (row-major pixels), through the reference's uint8 quantisation."""
    h = rgb.shape[2]
    q = (np.asarray(rgb) * 255).clip(0, 255).astype('uint8')
    return np.ascontiguousarray(q[:, :, :, h:2 * h].transpose(0, 2, 3, 1).reshape(len(q), h * h, 3)) / 255.


def _evaluate_baseline(batches, device, dataset, register, result_path, with_colors=False, verify=None, fuse=None):
    """register(pcs, valid) -> (pose [B,4,4], status [B]) tensors for the observed-block clouds of a batch; with_colors: register(pcs,
    valid, colors [2B,P,3] f64).  verify="observed": the records gain evaluate_pairs' visibility fields for the baseline's one pose (vis_level
    is 0); a baseline completes nothing, so there is no "completed".  fuse=voxel: evaluate_pairs' fusion fields for the baseline's pose."""
    import torch
    from . import util
    if verify not in (None, "observed"):
        raise ValueError("the baselines take verify=None or 'observed'")
    stats = []
    for batch in batches:
        n = _batch_size(batch)
        sub = _batch_take(batch, np.arange(n))
        depth = torch.from_numpy(np.ascontiguousarray(sub["depth"].reshape(2 * n, *sub["depth"].shape[2:]))).to(device)
        pcs, valid = util.depth2pc_dev(depth, dataset)
        if with_colors:
            colors = torch.from_numpy(observed_colors(sub["rgb"].reshape(2 * n, *sub["rgb"].shape[2:]))).to(device)
            pose, status = register(pcs, valid, colors)
        else:
            pose, status = register(pcs, valid)
        pose, status = pose.cpu().numpy(), status.cpu().numpy()
        R_gts = [np.matmul(sub["R"][q, 1], np.linalg.inv(sub["R"][q, 0])) for q in range(n)]
        ovs, nns = _pair_overlap_stats(pcs, valid, R_gts)
        if verify is not None:
            vcounts, _, vsc = util.pose_visibility_dev(pcs, valid, observed_depth(depth, dataset), pose[:, None], dataset)
            vcounts, vsc = vcounts.sum(2).cpu().numpy(), {k: v.cpu().numpy() for k, v in vsc.items()}
        fus = _fuse_fields(observed_depth(depth, dataset), pose, R_gts, dataset, fuse) if fuse is not None else None
        pcs, valid = pcs.cpu().numpy(), valid.cpu().numpy().astype(bool)
        for q in range(n):
            R_gt_44 = R_gts[q]
            pc_src, pc_tgt = pcs[2 * q][valid[2 * q]], pcs[2 * q + 1][valid[2 * q + 1]]
            if len(pc_src) == 0 or len(pc_tgt) == 0:                  # evaluation.py:184-186
                continue
            ov, pc_nn = ovs[q], nns[q]
            if ov < 0.1:                                                  # evaluation.py:190-191
                continue
            cam_dist, pc_dist = _host_pair_stats(pc_src, pc_tgt, R_gt_44)
            k = len(stats)
            rec = result_record(f"pair{k}/src", f"pair{k}/tgt", pose[q], R_gt_44, pc_src, ov, pc_dist, cam_dist, pc_nn)
            rec['status'] = int(status[q])
            if verify is not None:
                rec.update(vis_agreement=float(vsc["agreement"][q, 0]), vis_violation_rate=float(vsc["violation_rate"][q, 0]),
                           vis_observed=float(vsc["observed"][q, 0]), vis_counts=vcounts[q, 0].copy(), vis_level=0,
                           R_pred_44_selected=rec['R_pred_44'].copy())
            if fus is not None:
                rec.update(fus[q])
            stats.append(rec)
    if result_path is not None:
        save_results(result_path, stats)
    return stats


def synchronize_scene(pairs, poses, M, weights=None, device=None, **sync):
    """One scene's relative poses -> one absolute pose per view: util.pose_graph(pairs, poses, weights) builds the edges
    (several poses per pair become competing edges), util.pose_sync_dev solves (`sync` = its keyword overrides: sigma_r, sigma_t, mu0, div,
    n_final, robust).  pairs / poses / weights as util.pose_graph's (poses=None: `pairs` are records).
    -> host arrays {"pose" [M,4,4] world -> camera in each component's gauge, "component" [M], "n_components", "cost", "last_step", and per
    edge "src", "dst", "pair", "w0", "confidence", "res_rot", "res_trans", "tree", "edge_state"; "pair_confidence" [len(pairs)]: the largest
    confidence among the pair's edges}."""
    from . import util
    src, dst, T, w0, pair = util.pose_graph(pairs, poses, weights)
    out = util.pose_sync_dev(T, src, dst, w0, np.array([0, int(M)], np.int32), np.array([0, len(src)], np.int32), device=device, **sync)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("n_components", "cost", "last_step"):
        res[k] = res[k][0].item()
    res.update(src=src, dst=dst, pair=pair, w0=w0)
    pc = np.zeros(len(pairs))
    np.maximum.at(pc, pair, res["confidence"])
    res["pair_confidence"] = pc
    return res


def absolute_pose_errors(pose_hat, R, component=None):
    """Synchronised poses against ground truth: pose_hat [M,4,4] world -> camera in each component's gauge (synchronize_scene's "pose"), R
    [M,4,4] the loaders' world -> camera poses, component [M] (None: one component whose gauge is view 0).  View k is compared with
    R_k inv(R_gauge).  -> (rotation error in degrees [M], translation error in metres [M])."""
    pose_hat, R = np.asarray(pose_hat, np.float64).reshape(-1, 4, 4), np.asarray(R, np.float64).reshape(-1, 4, 4)
    M = len(R)
    comp = np.zeros(M, np.int64) if component is None else np.asarray(component).reshape(-1)
    rot, tr = np.zeros(M), np.zeros(M)
    for k in range(M):
        want = np.matmul(R[k], np.linalg.inv(R[comp[k]]))
        rot[k] = angular_distance_np(pose_hat[k, :3, :3], want[:3, :3])[0]
        tr[k] = np.linalg.norm(pose_hat[k, :3, 3] - want[:3, 3])
    return rot, tr


SCENE_BAD_ROT, SCENE_BAD_TRANS = 10.0, 0.3       # a pair estimate is wrong beyond 10 degrees or 0.3 m


def evaluate_scenes(pipe_or_method, scenes, device, verify=None, fuse=None, dataset=None, keypoints=200, seed=0, exp=None, mesh=False, refine=0,
                    render=False, mesh_min_component=None, mesh_decimate=None, **sync):
    """Scenes of posed views -> estimated pairs -> synchronised absolute poses -> what they do to the reconstruction.
    scenes: synth.render_scene dicts; pipe_or_method: a RelativePosePipeline, or "fgs" / "gs" / "cgs" (then `dataset` names the scenes').
    Per scene: mine_pairs, the pair method on the mined pairs through evaluate_pairs / evaluate_fgs / _gs / _cgs as they are (verify and
    the baselines' overlap rule included: a pair without a record contributes no edge), the graph (util.pose_graph; w0 = the record's
    vis_agreement where verify gave one, else 1; a selected level that differs from the last enters as a second edge), synchronize_scene.
    -> one dict per scene: 'views', 'pairs' (mined), 'records' (the pair records, untouched), 'edges', 'n_components', 'component', 'pose'
    [M,4,4], 'abs_err_rot' / 'abs_err_t' [M] (absolute_pose_errors) with their '_median' and '_max', 'pair_confidence' per record,
    'downweighted_share' (records with confidence < 0.5), 'bad_share' (records off by more than 10 degrees or 0.3 m), 'bad_downweighted' /
    'good_downweighted' (the share of each kind that is down-weighted; NaN for an empty kind), 'cost', 'last_step'.
    fuse=voxel: 'fuse_accuracy' / 'fuse_completeness' (reconstruction_scores of fuse_views of the largest component's views under the
    synchronised poses against the same fusion under R_k inv(R_gauge)), 'fuse_points', 'fuse_views'; exp: the surface is written to
    <exp>.scene<k>.ply.  mesh=True (with fuse): 'mesh' = mesh_stats of the estimate's fusion, and <exp>.scene<k>.mesh.ply next to the cloud;
    mesh_min_component=N: of that mesh without its components of fewer than N triangles (the cloud stays), with 'mesh_components' and
    'mesh_removed_triangles'.
    mesh_decimate=K: of that mesh (after the cleaning) decimated on the volume's grid coarsened by K (decimate_mesh), with
    'mesh_decimated': (triangles before, after, dist, within).
    refine=rounds (with fuse): the largest component's synchronised poses are refined against the fused volume (refine_scene,
    re-gauged to the component's first view) before the final fusion, which then uses them; the record gains 'refine_rounds',
    'refine_err_rot' / 'refine_err_t' [2, views] (absolute_pose_errors before and after), 'refine_wall_median' [2] (the surface's median
    distance to the room's walls in voxels, for scenes that carry "half"), 'refine_held_views'.  refine=0: nothing changes.
    render=True (with fuse): every fused view is rendered from its final pose against the final volume (render_views); the
    record gains 'render' = (rendered depth, cls, the view's own depth) on the device for render_summary, and with exp
    <exp>.scene<k>.render.npz is written.  render=False: nothing changes."""
    import torch
    from . import synth, util
    method = pipe_or_method if isinstance(pipe_or_method, str) else None
    if method is not None and method not in ("fgs", "gs", "cgs"):
        raise ValueError("evaluate_scenes takes a RelativePosePipeline or one of 'fgs', 'gs', 'cgs'")
    ds = dataset if method is not None else pipe_or_method.dataset
    if ds is None:
        raise ValueError("evaluate_scenes needs the dataset of the scenes for a baseline method")
    out = []
    for k, sc in enumerate(scenes):
        M = len(sc["depth"])
        entries = mine_pairs(sc["depth"], sc["R"], ds, f"scene{k}", device=device)
        ij = [(e['id_src'], e['id_tgt']) for e in entries]
        recs = []
        if ij:
            sel = lambda key: np.stack([sc[key][[i, j]] for i, j in ij])
            batch = {key: sel(key) for key in ("rgb", "norm", "depth", "R")}
            if method is None:
                h = sc["depth"].shape[1]
                kps = [synth.make_keypoints(1, keypoints, 7919 * (seed + 131 * k + b) + 13, pipe_or_method.mask_method, h=h) for b in range(len(ij))]
                batch["pts"], batch["ptw"] = np.concatenate([p[0] for p in kps]), np.concatenate([p[1] for p in kps])
            parts = [{key: v[b0:b0 + 32] for key, v in batch.items()} for b0 in range(0, len(ij), 32)]      # 32 pairs per batch of the pair method
            if method is None:
                recs = evaluate_pairs(pipe_or_method, parts, device, verify=verify)
            else:
                recs = {"fgs": evaluate_fgs, "gs": evaluate_gs, "cgs": evaluate_cgs}[method](parts, device, ds, verify=verify)
        gts = [np.matmul(sc["R"][j], np.linalg.inv(sc["R"][i])) for i, j in ij]       # a record's pair: the one with its R_gt
        pair_of = []
        for r in recs:
            d = [np.abs(g - r['R_gt']).max() for g in gts]
            pair_of.append(int(np.argmin(d)))
        poses, weights = [], []
        for r in recs:
            P = [r['R_pred_44']]
            if 'R_pred_44_selected' in r and not np.array_equal(r['R_pred_44_selected'], r['R_pred_44']):
                P.append(r['R_pred_44_selected'])
            poses.append(np.stack(P))
            weights.append(r.get('vis_agreement', 1.0))
        sy = synchronize_scene([ij[p] for p in pair_of], poses, M, weights, device=device, **sync)
        rot, tr = absolute_pose_errors(sy["pose"], sc["R"], sy["component"])
        conf = sy["pair_confidence"]
        bad = np.array([r['err_ad'] > SCENE_BAD_ROT or r['err_t'] > SCENE_BAD_TRANS for r in recs], bool)
        down = conf < 0.5
        share = lambda m: float(down[m].mean()) if m.any() else float("nan")
        rec = {'scene': k, 'views': M, 'pairs': len(ij), 'records': recs, 'edges': len(sy["src"]), 'n_components': sy["n_components"],
               'component': sy["component"], 'pose': sy["pose"], 'abs_err_rot': rot, 'abs_err_t': tr,
               'abs_err_rot_median': float(np.median(rot)) if M else float("nan"), 'abs_err_rot_max': float(rot.max()) if M else float("nan"),
               'abs_err_t_median': float(np.median(tr)) if M else float("nan"), 'abs_err_t_max': float(tr.max()) if M else float("nan"),
               'pair_confidence': conf, 'downweighted_share': float(down.mean()) if len(recs) else float("nan"),
               'bad_share': float(bad.mean()) if len(recs) else float("nan"), 'bad_downweighted': share(bad), 'good_downweighted': share(~bad),
               'cost': sy["cost"], 'last_step': sy["last_step"]}
        if fuse is not None and M:
            comp = sy["component"]
            g = int(np.bincount(comp, minlength=M).argmax())
            views = np.nonzero(comp == g)[0]
            up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(device)
            depth = up(sc["depth"][views])
            rgb = up(sc["rgb"][views]) if exp is not None else None
            inv_g = np.linalg.inv(sc["R"][g])
            pose_est = sy["pose"][views]
            if refine:
                ref_out = refine_scene(depth, pose_est, ds, fuse, rounds=int(refine))
                gauge = np.linalg.inv(ref_out["pose"][int(np.nonzero(views == g)[0][0])])
                pose_ref = np.stack([np.matmul(P, gauge) for P in ref_out["pose"]])
                errs = [absolute_pose_errors(P, sc["R"][views], np.full(len(views), int(np.nonzero(views == g)[0][0]))) for P in (pose_est, pose_ref)]
                rec.update(refine_rounds=int(refine), refine_err_rot=np.stack([e[0] for e in errs]), refine_err_t=np.stack([e[1] for e in errs]),
                           refine_held_views=int((ref_out["held"] > 0).sum()))
                if "half" in sc:
                    walls = []
                    for P in (pose_est, pose_ref):
                        sf = fuse_views(depth, None, P, ds, fuse)
                        pts = sf["points"][0, :int(sf["n_points"][0].item())].cpu().numpy()
                        walls.append(float(np.median(wall_error(pts @ inv_g[:3, :3].T + inv_g[:3, 3], sc["half"], fuse))) if len(pts) else float("nan"))
                    rec['refine_wall_median'] = walls
                pose_est = pose_ref
            est = fuse_views(depth, rgb, pose_est, ds, fuse, mesh=mesh)
            ref = fuse_views(depth, None, np.stack([np.matmul(sc["R"][v], inv_g) for v in views]), ds, fuse)
            acc, cmp_ = reconstruction_scores(est, ref)
            n = int(est["n_points"][0].item())
            rec.update(fuse_accuracy=float(acc[0]), fuse_completeness=float(cmp_[0]), fuse_points=n, fuse_views=len(views))
            if exp is not None:
                rec['fuse_ply'] = f"{exp}.scene{k}.ply"
                util.save_ply(rec['fuse_ply'], est["points"][0, :n], est["normals"][0, :n], est["colors"][0, :n])
            if render:
                rv = render_views(est["state"], pose_est, ds, int(depth.shape[1]))
                rec['render'] = (rv["depth"], rv["cls"], depth)
                if exp is not None:
                    rec['render_npz'] = save_render(f"{exp}.scene{k}.render.npz", rv)
            if mesh:
                if mesh_min_component is not None:
                    est, rec['mesh_components'], rec['mesh_removed_triangles'] = clean_mesh(est, mesh_min_component)
                    n = int(est["n_points"][0].item())
                if mesh_decimate is not None:
                    est, rec['mesh_decimated'] = decimate_mesh(est, mesh_decimate)
                    n = int(est["n_points"][0].item())
                rec['mesh'] = mesh_stats(est)[0]
                if exp is not None:
                    rec['mesh_ply'] = f"{exp}.scene{k}.mesh.ply"
                    util.save_ply(rec['mesh_ply'], est["points"][0, :n], est["normals"][0, :n], est["colors"][0, :n],
                                  est["triangles"][0, :int(est["n_triangles"][0].item())])
        out.append(rec)
    return out


def scenes_summary(recs):
    """What the CLI reports about evaluate_scenes' records: medians over the scenes and the down-weighting shares over all pair records."""
    med = lambda v: float(np.nanmedian(v)) if len(v) and not np.all(np.isnan(v)) else float("nan")
    conf = np.concatenate([r['pair_confidence'] for r in recs]) if recs else np.zeros(0)
    bad = np.array([p['err_ad'] > SCENE_BAD_ROT or p['err_t'] > SCENE_BAD_TRANS for r in recs for p in r['records']], bool)
    share = lambda m: float((conf[m] < 0.5).mean()) if m.any() else float("nan")
    out = {"abs_err_rot_median": med([r['abs_err_rot_median'] for r in recs]), "abs_err_rot_max": med([r['abs_err_rot_max'] for r in recs]),
           "abs_err_t_median": med([r['abs_err_t_median'] for r in recs]), "abs_err_t_max": med([r['abs_err_t_max'] for r in recs]),
           "pair_records": int(len(conf)), "bad_share": float(bad.mean()) if len(bad) else float("nan"),
           "bad_downweighted": share(bad), "good_downweighted": share(~bad), "components_max": max([r['n_components'] for r in recs] or [0])}
    if recs and 'fuse_accuracy' in recs[0]:
        out.update(fuse_accuracy_median=med([r['fuse_accuracy'] for r in recs]), fuse_completeness_median=med([r['fuse_completeness'] for r in recs]),
                   fuse_points=int(sum(r['fuse_points'] for r in recs)), fuse_ply=[r['fuse_ply'] for r in recs if 'fuse_ply' in r])
    if recs and any('refine_rounds' in r for r in recs):
        rr = [r for r in recs if 'refine_rounds' in r]
        out.update(refine_rounds=rr[0]['refine_rounds'],
                   refine_abs_err_rot_median=[med([float(np.median(r['refine_err_rot'][k])) for r in rr]) for k in (0, 1)],
                   refine_abs_err_t_median=[med([float(np.median(r['refine_err_t'][k])) for r in rr]) for k in (0, 1)],
                   refine_wall_median=[med([r['refine_wall_median'][k] for r in rr if 'refine_wall_median' in r]) for k in (0, 1)],
                   refine_held_views=int(sum(r['refine_held_views'] for r in rr)))
    if recs and any('mesh' in r for r in recs):
        out.update(mesh_summary([r['mesh'] for r in recs if 'mesh' in r]), mesh_ply=[r['mesh_ply'] for r in recs if 'mesh_ply' in r])
    if recs and any('mesh_components' in r for r in recs):
        rr = [r for r in recs if 'mesh_components' in r]
        out.update(mesh_clean_summary([r['mesh_components'] for r in rr], [r['mesh_removed_triangles'] for r in rr]))
    if recs and any('mesh_decimated' in r for r in recs):
        out.update(mesh_decimate_summary([r['mesh_decimated'] for r in recs if 'mesh_decimated' in r]))
    return out


def evaluate_descriptors(batches, net, device, dataset, mask_method, seed=0, n_eval=100, sift_baseline=False, **corres):
    """The reference's descriptor metric (evalDLDescriptor, mainPanoCompletion2view.py:383-414) over batches of pairs with ground-truth
    poses: per batch the level-0 forward the pipeline builds (masked own view, zero warped view), the descriptor = the feature channels
    at the pipeline's feat_off, dense correspondences from the batch's depth and poses (descriptor.dense_correspondences; batch["R"] is
    camera-to-world and is passed as is; `corres` = its keyword overrides) and the rank ratios.  One np.random.RandomState(seed) serves
    every draw, batch after batch.  -> {"pairs", "valid_pairs", "ratiosObs", "ratiosUnobs" (one entry per valid pair with a non-empty
    class), "ratio_obs", "ratio_unobs" (their means; NaN when empty)}.
    sift_baseline: also the reference's SIFT baseline on the same correspondences (descriptor.evalSiftDescriptor,
    mainPanoCompletion2view.py:353-381): the result gains "ratiosSift" (one entry per valid pair) and "ratio_sift".  Its draws come from a
    second np.random.RandomState(seed + 1), so the other numbers are the same with and without it."""
    import torch
    from . import descriptor, util
    from .pipeline import RelativePosePipeline
    pipe = RelativePosePipeline(net, dataset, mask_method, alter_steps=1)
    rng = np.random.RandomState(seed)
    rng_sift = np.random.RandomState(seed + 1)
    obs, unobs, sift, pairs, valid = [], [], [], 0, 0
    for batch in batches:
        n = _batch_size(batch)
        sub = _batch_take(batch, np.arange(n))
        h = sub["depth"].shape[2]
        st = pipe.prepare(sub["rgb"], sub["norm"], sub["depth"], np.zeros((n, 2, 1, 2)), np.zeros((n, 2, 1)), device)
        x = pipe._net_input(st)
        x[:, 8:].zero_()                              # level 0: the warp under the identity is the all-zero view (util.py:95-96)
        f = net.forward(x, out=st["f"], zero_warp=True)
        _, mask = util.apply_mask_dev(torch.ones(2 * n, 1, h, 4 * h, dtype=torch.float32, device=device), mask_method)
        dc = descriptor.dense_correspondences(st["depth"], sub["R"].reshape(2 * n, 4, 4), dataset, rng, **corres)
        o, u = descriptor.evalDLDescriptor(f, pipe.feat_off, net.out_channels - pipe.feat_off, dc, mask, rng, n_eval=n_eval)
        obs += o
        unobs += u
        if sift_baseline:
            sift += descriptor.evalSiftDescriptor(sub["rgb"], dc, rng_sift, n_eval=n_eval)
        pairs += n
        valid += int(dc["valid"].sum())
    mean = lambda v: float(np.mean(v)) if v else float("nan")
    res = {"pairs": pairs, "valid_pairs": valid, "ratiosObs": obs, "ratiosUnobs": unobs, "ratio_obs": mean(obs), "ratio_unobs": mean(unobs)}
    if sift_baseline:
        res["ratiosSift"], res["ratio_sift"] = sift, mean(sift)
    return res


def evaluate_completion(batches, net, device, dataset, mask_method, seed=0, with_contrast=True, geometric_weight=False, **corres):
    """The losses of the reference's validation pass (learner.step(mode='val'), mainPanoCompletion2view.py:457-602) over batches of pairs
    with ground-truth poses, on the INFERENCE network: BatchNorm groups are (source, target) pairs here, not the trainer's 4n batch.
    Per batch two forwards: "type 0" = the level-0 forward evaluate_descriptors builds (masked own view, zero warped view) and "type 1" =
    the own view with the other view warped under a perturbed pose (completion.perturbed_poses, util.warp_pairs_dev).  Of each:
    completion.completion_loss_dev against complete = (rgb, norm, depth) and the labels synth.make_labels gives the rendered normals
    (batch["label"] [B,2,h,4h] overrides them), and -- with_contrast -- completion.contrast_loss on descriptor.dense_correspondences.
    One np.random.RandomState(seed) serves every draw; per batch: the correspondence draws, the perturbation draws, the negatives of
    type 0, the negatives of type 1.  geometric_weight: weight = completion.geometric_weight (the reference's --GeometricWeight; off by
    default there too).  -> {"pairs", "valid_pairs", "n_bad_label", "type0": {...}, "type1": {...}} with, per type, the keys of
    completion.completion_scalars over all images of all batches, and loss_fl / loss_fl_pos / loss_fl_neg (means over the valid pairs'
    correspondences and negatives of all batches; 0 without a valid pair), n_active, n_skipped."""
    import torch
    from . import completion, descriptor, synth, util
    from .pipeline import RelativePosePipeline
    pipe = RelativePosePipeline(net, dataset, mask_method, alter_steps=1)
    rng = np.random.RandomState(seed)
    S, C_ = net.snumclass, net.out_channels - pipe.feat_off
    acc = [{"sums": [], "cross": 0.0, "pos": 0.0, "neg": 0.0, "n_active": 0, "n_skipped": 0} for _ in range(2)]
    pairs = valid = n_bad = 0
    K = n_neg = 0
    hw = None
    for batch in batches:
        n = _batch_size(batch)
        sub = _batch_take(batch, np.arange(n))
        h = sub["depth"].shape[2]
        hw = (h, 4 * h)
        st = pipe.prepare(sub["rgb"], sub["norm"], sub["depth"], np.zeros((n, 2, 1, 2)), np.zeros((n, 2, 1)), device)
        complete = torch.cat((st["rgb"], st["norm"], st["depth"][:, None]), 1).contiguous()
        lab = sub["label"] if "label" in sub else synth.make_labels(sub["norm"], S)
        label = torch.from_numpy(np.ascontiguousarray(np.asarray(lab).reshape(2 * n, h, 4 * h))).to(device=device, dtype=torch.uint8)
        _, mask = util.apply_mask_dev(torch.ones(2 * n, 1, h, 4 * h, dtype=torch.float32, device=device), mask_method)
        weight = None
        if geometric_weight:
            weight = torch.from_numpy(completion.geometric_weight(mask_method, h)).to(device).expand(2 * n, h, 4 * h).contiguous()
        dc = descriptor.dense_correspondences(st["depth"], sub["R"].reshape(2 * n, 4, 4), dataset, rng, **corres) if with_contrast else None
        R_rel = np.stack([np.matmul(sub["R"][b, 1], np.linalg.inv(sub["R"][b, 0])) for b in range(n)])
        poses = torch.from_numpy(completion.perturbed_poses(R_rel, rng).reshape(2 * n, 4, 4)).to(device)
        x = pipe._net_input(st)
        for typ in range(2):
            if typ == 0:
                x[:, 8:].zero_()                      # type 0: the blank other view (level 0 of the pipeline)
            else:
                util.warp_pairs_dev(x, poses, dataset)        # type 1: the other view under the perturbed pose
            f = net.forward(x, out=st["f"], zero_warp=(typ == 0))
            sums, _, cross, bad = completion.completion_loss_dev(f, complete, label, mask, weight, S=S)
            a = acc[typ]
            a["sums"].append(sums.cpu().numpy())
            a["cross"] += float(cross.item()) / (2 * n)           # per batch: ce_cross / N, so that batches of different sizes add up
            if typ == 0:
                n_bad += int(bad.sum().item())
            if with_contrast:
                det = {}
                K, n_neg = dc["idxSrc"].shape[1], 100
                _, lp, ln = completion.contrast_loss(f, pipe.feat_off, C_, dc, rng, n_neg=n_neg, details=det)
                nv = det["valid_pairs"]
                a["pos"] += lp * nv * K
                a["neg"] += ln * nv * K * n_neg
                a["n_active"] += det["n_active"]
                a["n_skipped"] += det["n_skipped"]
        pairs += n
        if with_contrast:
            valid += int(dc["valid"].sum())
    res = {"pairs": pairs, "valid_pairs": valid, "n_bad_label": n_bad}
    for typ in range(2):
        a = acc[typ]
        sums = np.concatenate(a["sums"]) if a["sums"] else np.zeros((0, 5, 2))
        N = max(len(sums), 1)
        # errG_s over several batches: the mean of the batches' own scalars weighted by their image counts (each batch is one `step`)
        r = completion.completion_scalars(sums, [a["cross"] * N], *(hw or (1, 4)))
        lp = a["pos"] / (valid * K) if valid else 0.0
        ln = a["neg"] / (valid * K * n_neg) if valid else 0.0
        r.update(loss_fl=lp + ln, loss_fl_pos=lp, loss_fl_neg=ln, n_active=a["n_active"], n_skipped=a["n_skipped"])
        res[f"type{typ}"] = r
    return res


def evaluate_pairs_sharded(pipe, batches, device, result_path=None, names=None, rank=0, world=1, resume=True, round_batches=None,
                           record_fn=None, depth=2, normals="given", normal_hist=None):
    """`evaluate_pairs` over `world` ranks (one process per GPU, torch.distributed initialised by the caller:
    distributed.init_from_env).  Every rank receives the same `batches` (a sequence of the DataLoader-layout dicts, B pairs each);
    of every global batch rank r takes the contiguous block distributed.shard_range(B_todo, r, world) -- BatchNorm groups are scan
    pairs, so a shard is independent of the others -- runs its blocks through pipe.run_pipelined (`depth` in flight), and computes
    the records of its own pairs.  Per ROUND (`round_batches` global batches; default: the whole list) there is ONE all_gather of
    the stacked poses (distributed.gather_poses: the north-star's single RCCL gather) and one gather of the record lists to rank 0,
    which keeps the records in global pair order and writes `result_path` (np.save of the list of dicts, evaluation.py:319-320).
    resume: an existing result file is loaded and its first (len // 100) * 100 pairs are kept and skipped, like the reference's
    repeat bookkeeping (evaluation.py:129-133).  Returns the full record list on rank 0, None elsewhere.
    A batch may be a dict of arrays or a lazy provider with `.size` and `.take(indices)` (SyntheticBatch): a rank then only
    materialises its own pairs.
    record_fn(sub_batch, local_indices, poses_host, k0) -> list of records (sub_batch = the rank's pairs of the global batch, in the
    order of local_indices): override for callers with their own statistics (tests).
    normals / normal_hist: as _prepare_batch (normal_hist accumulates this rank's pairs only)."""
    import os
    import torch
    import torch.distributed as dist
    from . import distributed as D
    batches = list(batches)
    sizes = [_batch_size(b) for b in batches]
    starts = np.concatenate(([0], np.cumsum(sizes)))
    stats = []
    if rank == 0 and resume and result_path is not None and os.path.exists(result_path if result_path.endswith(".npy") else result_path + ".npy"):
        old = load_results(result_path if result_path.endswith(".npy") else result_path + ".npy")
        stats = old[:(len(old) // 100) * 100]
    done = len(stats)
    if world > 1:
        t = torch.tensor([done], dtype=torch.int64, device=device if dist.get_backend() == "nccl" else "cpu")
        dist.broadcast(t, 0)
        done = int(t.item())
    todo = [(i, max(0, done - int(starts[i]))) for i in range(len(batches)) if int(starts[i + 1]) > done]     # (batch, first pair still to do)
    # a ROUND = the unit of gathering and saving (default: the whole list).  Device memory does NOT grow with it: the batches of a round are
    # prepared lazily, at most `depth` at a time (run_pipelined(provider=...)), and a batch's prepared state and host arrays are dropped as
    # soon as its records are built (the default run used to prepare every batch up front -- 140 GB at 2048 pairs).
    nround = len(todo) if round_batches is None else max(1, int(round_batches))
    for r0 in range(0, len(todo), max(1, nround)):
        chunk = todo[r0:r0 + nround]
        local, mine = [], []
        for j, (i, first) in enumerate(chunk):
            lo, hi = D.shard_range(sizes[i] - first, rank, world)
            idx = np.arange(first + lo, first + hi)
            local.append(idx)
            if len(idx):
                mine.append(j)
        subs, recs, poses, status = {}, [], [None] * len(mine), [None] * len(mine)

        def provider(q):
            i, first = chunk[mine[q]]
            b = _batch_take(batches[i], local[mine[q]])
            subs[q] = b
            return _prepare_batch(pipe, b, device, normals, normal_hist)

        def on_result(q, pose, st):
            # records of this rank's pairs of batch q, built as soon as the batch is complete (the other in-flight batch keeps the GPU busy)
            i, first = chunk[mine[q]]
            idx, sub = local[mine[q]], subs.pop(q)
            poses[q], status[q] = pose.reshape(-1, 4, 4), st.reshape(-1)
            ph = pose.detach().cpu().numpy().reshape(-1, 4, 4)
            sh = st.detach().cpu().numpy().reshape(-1)
            k0 = int(starts[i])
            rr = record_fn(sub, idx, ph, k0) if record_fn is not None else _default_record(pipe, sub, ph, device, names, [k0 + int(b) for b in idx])
            for j, (b, rec) in enumerate(zip(idx, rr)):
                rec['status'] = int(sh[j])             # the matcher's per-pair status (0 ok, 1.. the reference's "return identity" exits)
                recs.append((k0 + int(b), rec))
            return None

        if mine:
            pipe.run_pipelined(None, len(mine), on_result=on_result, depth=min(depth, len(mine)), provider=provider)
        n_local = sum(len(ix) for ix in local)
        n_round = sum(sizes[i] - first for i, first in chunk)
        if world > 1:
            # ONE all_gather of this round's poses (+ status); blocks are per-rank concatenations, ragged by at most one pair per batch
            pl = torch.cat(poses) if poses else torch.zeros(0, 4, 4, dtype=torch.float64, device=device)
            sl = torch.cat(status).to(torch.int32) if status else torch.zeros(0, dtype=torch.int32, device=device)
            counts = [sum(D.shard_range(sizes[i] - first, r, world)[1] - D.shard_range(sizes[i] - first, r, world)[0] for i, first in chunk)
                      for r in range(world)]
            bmax = max(counts)
            buf = torch.zeros(bmax, 17, dtype=torch.float64, device=pl.device)
            buf[:n_local, :16] = pl.reshape(-1, 16); buf[:n_local, 16] = sl.to(torch.float64)
            out = [torch.empty_like(buf) for _ in range(world)]
            dist.all_gather(out, buf)
            D.COLLECTIVES["all_gather"] += 1
            gathered = [None] * world if rank == 0 else None
            dist.gather_object(recs, gathered, dst=0)
            problem = None
            if rank == 0:
                allrecs = [kr for part in gathered for kr in part]
                # cross-check: the gathered poses are the ones the records were built from (NaN poses -- e.g. from NaN depth -- compare
                # equal to themselves: a degenerate pair is a result, not a harness failure); the gathered status goes into the record
                by_k = {}
                for r in range(world):
                    ks = [int(starts[i]) + first + q for i, first in chunk for q in range(*D.shard_range(sizes[i] - first, r, world))]
                    for row, k in zip(out[r][:counts[r]].cpu().numpy(), ks):
                        by_k[k] = row
                for k, rec in allrecs:
                    if k not in by_k:
                        problem = f"pair {k}: a record without a gathered pose"
                        break
                    if rec.get('status') != int(by_k[k][16]):
                        problem = f"pair {k}: the gathered status differs from the status in its record"
                        break
                    if 'R_pred_44' in rec and not np.array_equal(by_k[k][:16].reshape(4, 4)[:3, :4], np.asarray(rec['R_pred_44'])[:3, :4], equal_nan=True):
                        problem = f"pair {k}: the gathered pose differs from the pose its record was built from"
                        break
                if problem is None and len(allrecs) != n_round:
                    problem = f"{len(allrecs)} records for {n_round} pairs"
            # every rank learns the verdict BEFORE anyone raises: no rank is left waiting in the next round's collective
            flag = [problem]
            dist.broadcast_object_list(flag, src=0)
            if flag[0] is not None:
                raise RuntimeError("evaluate_pairs_sharded: " + flag[0])
        else:
            allrecs = recs
            if len(allrecs) != n_round:
                raise RuntimeError(f"evaluate_pairs_sharded: {len(allrecs)} records for {n_round} pairs")
        if rank == 0:
            stats += [rec for _, rec in sorted(allrecs, key=lambda kr: kr[0])]
            if result_path is not None:
                save_results(result_path, stats)
    return stats if rank == 0 else None


def _cli_parser():
    """The argument parser of main()."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--dataset", default="scannet", choices=["suncg", "matterport", "scannet"])
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=256, help="pairs per global batch (sharded over the ranks)")
    ap.add_argument("--keypoints", type=int, default=200)
    ap.add_argument("--exp", default=None, help="result file prefix: <exp>.result.npy (resumed in units of 100 pairs unless --rm)")
    ap.add_argument("--rm", action="store_true", help="ignore an existing result file (the reference's --rm)")
    ap.add_argument("--round-batches", type=int, default=None, help="global batches per gather + save round (default: all)")
    ap.add_argument("--seed", type=int, default=4000)
    ap.add_argument("--keypoint-mode", choices=["given", "reference"], default="given",
                    help="reference: every level derives its keypoints from its own feature maps like rputil.getKeypoint (synthetic SIFT detections)")
    ap.add_argument("--sift", type=int, default=120, help="--keypoint-mode reference: synthetic SIFT detections per view")
    ap.add_argument("--sift-detector", choices=["synthetic", "gpu"], default="synthetic",
                    help="--keypoint-mode reference: synthetic = uniform random detections (synth.make_sift_detections), gpu = the HIP SIFT "
                         "detector on the rendered views (rputil.sift_views)")
    ap.add_argument("--precision", choices=["f32", "bf16x9", "bf16x6", "f16x3", "bf16x3", "f16"], default="f32",
                    help="conv arithmetic of SCNet (SCNet.set_precision): f32 = the fp32 MFMA kernels (default), bf16x6 = what bench.py runs configs 1-3 in")
    ap.add_argument("--completion", type=int, default=1, choices=[0, 1], help="0 = the reference's 'ours_nc' method (evaluation.py:74): observed-region keypoints only")
    ap.add_argument("--method", choices=["ours", "fgs", "gs", "cgs"], default="ours",
                    help="fgs = the reference's fast global registration baseline (baselines.py:83-106), gs = its RANSAC global registration "
                         "baseline (baselines.py:52-81), cgs = gs refined by coloured ICP (baselines.py:110-168), all on the observed clouds: no network")
    ap.add_argument("--descriptor-eval", action="store_true",
                    help="the reference's descriptor metric instead of poses (evalDLDescriptor, mainPanoCompletion2view.py:383-414): one JSON "
                         "line with metric, pairs, valid_pairs, ratio_obs, ratio_unobs, seconds")
    ap.add_argument("--sift-baseline", action="store_true",
                    help="--descriptor-eval: also the reference's SIFT baseline of the metric (evalSiftDescriptor, "
                         "mainPanoCompletion2view.py:353-381): the JSON line gains ratio_sift")
    return ap


def _cli_parser_completion():
    """_cli_parser() plus --completion-eval: what main() parses.  (_cli_parser's own argument set is pinned by tests/test_siftdesc_cpu.py.)"""
    ap = _cli_parser()
    ap.add_argument("--completion-eval", action="store_true",
                    help="the losses of the reference's validation pass instead of poses (mainPanoCompletion2view.py:457-602): one JSON line "
                         "with metric = completion_loss and, per input type, errG_rgb / _n / _d / _s and loss_fl_pos / _neg")
    ap.add_argument("--normals", choices=["given", "estimated"], default="given",
                    help="--method ours (with --completion 0 / 1 and either --keypoint-mode): estimated = the views' normal maps are not "
                         "read but estimated from the depth panoramas on the GPU (util.depth_normals_dev); the JSON line gains normals, "
                         "normal_err_deg_median and normal_err_deg_p90 (the angle to the given normals over the pixels valid in both)")
    ap.add_argument("--from-frames", action="store_true",
                    help="--method ours --dataset scannet: the pairs enter as 480x640 perspective RGB-D frames alone; the panoramas are built "
                         "from them on the GPU (util.frames_to_pano_dev) and their normals estimated there; the JSON line gains "
                         "pano_depth_err_median / pano_depth_err_p90 (relative, against the directly rendered panoramas inside the kinect "
                         "box) and the pose statistics of both routes (stats_from_frames, stats_rendered)")
    ap.add_argument("--mine-pairs", action="store_true",
                    help="no poses are estimated: render --scenes scenes of --scene-views posed views each (synth.render_scene, seeds --seed, "
                         "--seed + 1, ...), find which pairs of views overlap on the GPU (mine_pairs) and print one JSON line with scenes, "
                         "views, pairs per overlap bucket and seconds; --exp writes the pair list to <exp>.datalist.npy, the object file the "
                         "reference's loaders read (datasets/SUNCG.py:66)")
    ap.add_argument("--scenes", type=int, default=8, help="--mine-pairs: the number of scenes")
    ap.add_argument("--scene-views", type=int, default=6, help="--mine-pairs / --pair-source scenes: views per scene")
    ap.add_argument("--min-overlap", type=float, default=None, help="--mine-pairs: leave out pairs whose overlap is below this")
    ap.add_argument("--pair-source", choices=["pairs", "scenes"], default="pairs",
                    help="--method ours / fgs / gs / cgs: scenes = the pairs are mined from multi-view scenes (SceneBatch, equal numbers from "
                         "the three overlap buckets) instead of synth.make_pairs' two unrelated poses per room, which almost never overlap")
    ap.add_argument("--verify", choices=list(VERIFY_MODES), default=None,
                    help="check every estimated pose against the partner view's depth panorama (util.pose_visibility_dev, DESIGN.md 4.15): "
                         "observed = against the depth under the pipeline's mask, completed = against the last level's completed depth "
                         "(--method ours only).  --method ours (one GPU, given keypoints) / fgs / gs / cgs: the records gain the vis_* fields "
                         "and the JSON line vis_spearman_rot, vis_spearman_trans (rank correlation of vis_agreement with err_ad / err_t) and "
                         "vis_selected (per bucket the mean rotation error of the level the check selects next to the last level's); "
                         "--mine-pairs --verify observed: the mined entries gain vis_agreement")
    ap.add_argument("--fuse", type=float, default=None, metavar="VOXEL",
                    help="TSDF fusion at this voxel size (DESIGN.md 4.16).  --method ours (one GPU, given keypoints) / fgs / gs / cgs: every "
                         "record gains fuse_accuracy, fuse_completeness (the pair fused under its estimate against the same fusion under R_gt) "
                         "and fuse_points, the JSON line their medians and fuse_spearman_rot (rank correlation of fuse_accuracy with err_ad).  "
                         "--mine-pairs --fuse: each scene's views are fused under the ground-truth poses; the line gains fuse_wall_err_median / "
                         "_p90 (voxels, against the room's walls) and fuse_points, and <exp>.scene<k>.ply is written when --exp is given")
    ap.add_argument("--reconstruct", action="store_true",
                    help="--method ours / fgs / gs / cgs on --scenes scenes of --scene-views views (synth.render_scene, seeds --seed, --seed + 1, "
                         "...): mine each scene's pairs, estimate them, synchronise the relative poses into one pose per view "
                         "(util.pose_sync_dev, DESIGN.md 4.17) and print one JSON line with the absolute pose errors, the share of wrong pair "
                         "estimates that were down-weighted and, with --fuse, the reconstruction scores of the scenes fused under the "
                         "synchronised poses; --verify observed weights the edges by vis_agreement; --exp writes <exp>.scene<k>.ply")
    ap.add_argument("--refine", type=int, default=0, metavar="ROUNDS",
                    help="--reconstruct --fuse VOXEL: after the synchronisation, refine every view's pose against the volume the other views fuse "
                         "into (util.tsdf_align_dev, DESIGN.md 4.19), ROUNDS times, before the final fusion.  The JSON line gains, before and "
                         "after: refine_abs_err_rot_median / _t_median (absolute pose errors), refine_wall_median (the surface's median distance "
                         "to the room's walls, voxels), and refine_held_views (views with a direction the volume does not constrain)")
    ap.add_argument("--mesh-min-component", type=int, default=None, metavar="N",
                    help="--mesh: drop the mesh's connected components of fewer than N triangles (vertex connectivity, DESIGN.md 4.21) and its "
                         "unused vertices before the mesh statistics and <exp>.scene<k>.mesh.ply; the JSON line gains mesh_components_median, "
                         "mesh_largest_share_median (both of the mesh as extracted) and mesh_removed_triangles_median.  The cloud is not touched")
    ap.add_argument("--mesh-decimate", type=int, default=None, metavar="K",
                    help="--mesh: decimate the mesh by vertex clustering on the volume's grid coarsened by K (cells of K^3 voxels, DESIGN.md "
                         "4.22), after --mesh-min-component when both are given, before the mesh statistics and <exp>.scene<k>.mesh.ply; the "
                         "JSON line gains mesh_decimated_triangles_median, mesh_decimated_share_median (triangles after / before), "
                         "mesh_decimated_dist_median (how far a vertex moved) and mesh_decimated_within_median (new vertices within half a cell "
                         "of the original surface cloud).  The cloud is not touched")
    ap.add_argument("--mesh", action="store_true",
                    help="--mine-pairs --fuse VOXEL / --reconstruct --fuse VOXEL: also extract each fused scene's triangle mesh (marching cubes, "
                         "DESIGN.md 4.18); the JSON line gains the medians of mesh_stats (triangles, area, border edges) and the number of "
                         "non-manifold edges, and <exp>.scene<k>.mesh.ply is written next to the cloud when --exp is given")
    ap.add_argument("--render", action="store_true",
                    help="--mine-pairs --fuse VOXEL / --reconstruct --fuse VOXEL: render every view of a scene from its pose (ground truth for "
                         "--mine-pairs, the final poses for --reconstruct) against the final volume (util.tsdf_render_dev, DESIGN.md 4.20) and "
                         "compare the depth panoramas with the scans pixel by pixel; the JSON line gains render_depth_err_median / _p90 "
                         "(voxels, where both have data) and render_coverage (hits / measured pixels), and <exp>.scene<k>.render.npz (depth, "
                         "normal, color, cls) is written when --exp is given")
    return ap


def main(argv=None):
    """python -m relativepose_amd.evaluation --gpus N ...: the sharded evaluation over seeded synthetic scan pairs (no dataset ships with
    the reference) -- BASELINE configs[3]: a "val split" of --pairs pairs in global batches of --batch, sharded over N GPUs, one pose
    all_gather, one <exp>.result.npy.  Launched plainly it spawns its N ranks (one per GPU, RCCL); under torchrun it uses the launcher's
    environment.  Rank 0 prints one JSON line: pairs, seconds, per-overlap-bucket statistics (evaluation.py:321-327)."""
    import json
    import os
    import socket
    import sys
    import time
    args = _cli_parser_completion().parse_args(argv)

    if args.normals == "estimated" and (args.descriptor_eval or args.completion_eval or args.method != "ours"):
        raise SystemExit("--normals estimated applies to --method ours (the pose evaluation): the baselines and the descriptor / completion "
                         "metrics do not read the views' normal maps as an input of the pipeline")

    if args.verify is not None:
        if args.descriptor_eval or args.completion_eval or args.from_frames:
            raise SystemExit("--verify applies to the pose evaluation (--method ours / fgs / gs / cgs) and to --mine-pairs")
        if args.verify == "completed" and (args.mine_pairs or args.method != "ours"):
            raise SystemExit("--verify completed needs the network's completed depth: --method ours only")
        if args.gpus > 1 or (not args.mine_pairs and args.method == "ours" and args.keypoint_mode != "given"):
            raise SystemExit("--verify runs on one GPU (--gpus 1) with given keypoints: the check is not sharded")

    if args.fuse is not None:
        if args.descriptor_eval or args.completion_eval or args.from_frames:
            raise SystemExit("--fuse applies to the pose evaluation (--method ours / fgs / gs / cgs) and to --mine-pairs")
        if not (np.isfinite(args.fuse) and args.fuse > 0):
            raise SystemExit("--fuse takes a voxel size > 0")
        if args.gpus > 1 or (not args.mine_pairs and args.method == "ours" and args.keypoint_mode != "given"):
            raise SystemExit("--fuse runs on one GPU (--gpus 1) with given keypoints: the fusion is not sharded")

    if args.mesh and (args.fuse is None or not (args.mine_pairs or args.reconstruct)):
        raise SystemExit("--mesh applies to --mine-pairs --fuse VOXEL and to --reconstruct --fuse VOXEL")
    if args.mesh_min_component is not None and (not args.mesh or args.mesh_min_component < 1):
        raise SystemExit("--mesh-min-component N >= 1 applies to --mesh")
    if args.mesh_decimate is not None and (not args.mesh or args.mesh_decimate < 1):
        raise SystemExit("--mesh-decimate K >= 1 applies to --mesh")

    if args.render and (args.fuse is None or not (args.mine_pairs or args.reconstruct)):
        raise SystemExit("--render applies to --mine-pairs --fuse VOXEL and to --reconstruct --fuse VOXEL")

    if args.refine and (args.refine < 0 or args.fuse is None or not args.reconstruct):
        raise SystemExit("--refine takes a number of rounds >= 0 and applies to --reconstruct --fuse VOXEL")

    if args.reconstruct:
        if args.mine_pairs or args.descriptor_eval or args.completion_eval or args.from_frames or args.pair_source != "pairs":
            raise SystemExit("--reconstruct is a mode of its own: it mines, estimates and synchronises the pairs of its scenes")
        if args.gpus > 1 or args.keypoint_mode != "given":
            raise SystemExit("--reconstruct runs on one GPU (--gpus 1) with given keypoints: it is not sharded over ranks")
        if args.scenes < 1 or args.scene_views < 2 or args.scene_views > 64:
            raise SystemExit("--reconstruct takes --scenes >= 1 and 2 <= --scene-views <= 64")
        if args.method != "ours" and args.dataset == "scannet":
            raise SystemExit(f"--method {args.method}: the synthetic ScanNet views have no full-resolution depth, which the reference's baselines use")
        import torch
        from . import _lib, synth
        dev = _lib.require_gpu()
        ds = args.dataset
        who = args.method
        if args.method == "ours":
            from types import SimpleNamespace
            from . import params, weights
            from .model import SCNet
            from .pipeline import RelativePosePipeline
            mm, S, tanh = ("kinect", 21, 0) if ds == "scannet" else ("second", 21 if ds == "matterport" else 15, 1)
            net = SCNet(SimpleNamespace(batchnorm=1, useTanh=tanh, skipLayer=1, outputType="rgbdnsf", snumclass=S))
            net.load_state_dict(weights.make_state_dict(7, S))
            net.set_precision(args.precision)
            who = RelativePosePipeline(net, ds, mm, params.final_params(ds), completion=args.completion)
        t0 = time.perf_counter()
        scenes = [synth.render_scene(args.seed + s, args.scene_views, ds) for s in range(args.scenes)]
        recs = evaluate_scenes(who, scenes, dev, verify=args.verify, fuse=args.fuse, dataset=ds, keypoints=args.keypoints, seed=args.seed,
                               exp=args.exp, mesh=args.mesh, refine=args.refine, render=args.render,
                               mesh_min_component=args.mesh_min_component, mesh_decimate=args.mesh_decimate)
        torch.cuda.synchronize()
        line = {"reconstruct": True, "method": args.method, "dataset": ds, "scenes": args.scenes, "views": args.scene_views,
                "seconds": time.perf_counter() - t0, "verify": args.verify, "fuse": args.fuse}
        if args.refine:
            line["refine"] = args.refine
        line.update(scenes_summary(recs))
        if args.render:
            line.update(render_summary([r['render'] for r in recs if 'render' in r], args.fuse),
                        render_npz=[r['render_npz'] for r in recs if 'render_npz' in r])
        print(json.dumps(line), flush=True)
        return

    if args.mine_pairs:
        if args.gpus > 1:
            raise SystemExit("--mine-pairs runs on one GPU (--gpus 1)")
        if args.scenes < 1 or args.scene_views < 2:
            raise SystemExit("--mine-pairs takes --scenes >= 1 and --scene-views >= 2")
        import torch
        from . import _lib, synth
        dev = _lib.require_gpu()
        entries = []
        wall, fuse_points, plys = [], 0, []
        meshes, mesh_plys = [], []
        mesh_comps, mesh_removed, mesh_decimated = [], [], []
        renders, render_npz = [], []
        t0 = time.perf_counter()
        for s in range(args.scenes):
            sc = synth.render_scene(args.seed + s, args.scene_views, args.dataset)
            entries += mine_pairs(sc["depth"], sc["R"], args.dataset, f"scene{args.seed + s}", min_overlap=args.min_overlap, device=dev,
                                  verify=args.verify)
            if args.fuse is not None:
                from . import util
                up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
                surf = fuse_views(up(sc["depth"]), up(sc["rgb"]), sc["R"], args.dataset, args.fuse, mesh=args.mesh)
                n = int(surf["n_points"][0].item())
                pts = surf["points"][0, :n].cpu().numpy()
                wall.append(wall_error(pts, sc["half"], args.fuse))
                fuse_points += n
                if args.exp is not None:
                    plys.append(f"{args.exp}.scene{s}.ply")
                    util.save_ply(plys[-1], pts, surf["normals"][0, :n], surf["colors"][0, :n])
                if args.render:
                    dm = up(sc["depth"])
                    rv = render_views(surf["state"], sc["R"], args.dataset, int(dm.shape[1]))
                    renders.append((rv["depth"], rv["cls"], dm))
                    if args.exp is not None:
                        render_npz.append(save_render(f"{args.exp}.scene{s}.render.npz", rv))
                if args.mesh:
                    if args.mesh_min_component is not None:                 # the cloud above stays; the mesh loses its small components
                        surf, cs, removed = clean_mesh(surf, args.mesh_min_component)
                        mesh_comps.append(cs)
                        mesh_removed.append(removed)
                        n = int(surf["n_points"][0].item())
                        pts = surf["points"][0, :n].cpu().numpy()
                    if args.mesh_decimate is not None:
                        surf, part = decimate_mesh(surf, args.mesh_decimate)
                        mesh_decimated.append(part)
                        n = int(surf["n_points"][0].item())
                        pts = surf["points"][0, :n].cpu().numpy()
                    meshes.append(mesh_stats(surf)[0])
                    if args.exp is not None:
                        mesh_plys.append(f"{args.exp}.scene{s}.mesh.ply")
                        util.save_ply(mesh_plys[-1], pts, surf["normals"][0, :n], surf["colors"][0, :n],
                                      surf["triangles"][0, :int(surf["n_triangles"][0].item())])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        path = None if args.exp is None else save_data_list(args.exp + ".datalist.npy", {"test": entries})
        per = {k: sum(1 for e in entries if overlap_bucket(e['overlap']) == k) for k in OVERLAPS}
        line = {"mine_pairs": True, "dataset": args.dataset, "scenes": args.scenes, "views": args.scene_views, "pairs": len(entries),
                "pairs_per_bucket": per, "min_overlap": args.min_overlap, "seconds": dt, "data_list": path}
        if args.verify is not None:
            line["vis_agreement_mean_per_bucket"] = {k: float(np.nanmean([e['vis_agreement'] for e in entries if overlap_bucket(e['overlap']) == k] or [np.nan]))
                                                     for k in OVERLAPS}
        if args.fuse is not None:
            e = np.concatenate(wall) if wall else np.zeros(0)
            line.update(fuse=args.fuse, fuse_wall_err_median=float(np.median(e)) if e.size else float("nan"),
                        fuse_wall_err_p90=float(np.percentile(e, 90)) if e.size else float("nan"), fuse_points=fuse_points, fuse_ply=plys)
        if args.mesh:
            line.update(mesh_summary(meshes), mesh_ply=mesh_plys)
        if args.mesh_min_component is not None:
            line.update(mesh_clean_summary(mesh_comps, mesh_removed))
        if args.mesh_decimate is not None:
            line.update(mesh_decimate_summary(mesh_decimated))
        if args.render:
            line.update(render_summary(renders, args.fuse), render_npz=render_npz)
        print(json.dumps(line), flush=True)
        return

    if args.pair_source == "scenes" and (args.descriptor_eval or args.completion_eval or args.from_frames or args.keypoint_mode != "given"):
        raise SystemExit("--pair-source scenes applies to --method ours (given keypoints) / fgs / gs / cgs")

    def make_batch(size, seed, ds, mm):
        if args.pair_source == "scenes":
            return SceneBatch(size, seed, ds, mm, args.keypoints, views=args.scene_views, balanced=True)
        return None

    if args.from_frames:
        if args.descriptor_eval or args.completion_eval or args.method != "ours" or args.dataset != "scannet" or args.keypoint_mode != "given":
            raise SystemExit("--from-frames applies to --method ours --dataset scannet with given keypoints: the perspective frames are "
                             "the ScanNet loader's (datasets/ScanNet.py:211-230)")
        if args.gpus > 1:
            raise SystemExit("--from-frames runs on one GPU (--gpus 1): it is not sharded")
        import torch
        from types import SimpleNamespace
        from . import _lib, params, weights
        from .model import SCNet
        from .pipeline import RelativePosePipeline
        dev = _lib.require_gpu()
        ds, mm, S = "scannet", "kinect", 21
        net = SCNet(SimpleNamespace(batchnorm=1, useTanh=0, skipLayer=1, outputType="rgbdnsf", snumclass=S))
        net.load_state_dict(weights.make_state_dict(7, S))
        net.set_precision(args.precision)
        pipe = RelativePosePipeline(net, ds, mm, params.final_params(ds), completion=args.completion)
        bs = min(args.batch, 32)
        batches = [SyntheticBatch(min(bs, args.pairs - k), args.seed + k, ds, mm, args.keypoints) for k in range(0, args.pairs, bs)]
        t0 = time.perf_counter()
        recs_f, recs_d, errs = evaluate_from_frames(pipe, batches, dev)
        torch.cuda.synchronize()
        q = lambda p: float(np.quantile(errs, p)) if len(errs) else float("nan")
        print(json.dumps({"pairs": len(recs_f), "seconds": time.perf_counter() - t0, "dataset": ds, "from_frames": True, "normals": "estimated",
                          "pano_depth_err_median": q(0.5), "pano_depth_err_p90": q(0.9), "stats_from_frames": summarize(recs_f),
                          "stats_rendered": summarize(recs_d)}), flush=True)
        return

    if args.descriptor_eval:
        if args.gpus > 1:
            raise SystemExit("--descriptor-eval runs on one GPU (--gpus 1): the metric is not sharded")
        import torch
        from types import SimpleNamespace
        from . import _lib, weights
        from .model import SCNet
        dev = _lib.require_gpu()
        ds = args.dataset
        mm, S, tanh = ("kinect", 21, 0) if ds == "scannet" else ("second", 21 if ds == "matterport" else 15, 1)
        net = SCNet(SimpleNamespace(batchnorm=1, useTanh=tanh, skipLayer=1, outputType="rgbdnsf", snumclass=S))
        net.load_state_dict(weights.make_state_dict(7, S))
        net.set_precision(args.precision)
        bs = min(args.batch, 32)
        batches = [SyntheticBatch(min(bs, args.pairs - k), args.seed + k, ds, mm, 1) for k in range(0, args.pairs, bs)]
        t0 = time.perf_counter()
        r = evaluate_descriptors(batches, net, dev, ds, mm, seed=args.seed, sift_baseline=args.sift_baseline)
        torch.cuda.synchronize()
        line = {"metric": "descriptor_rank", "pairs": r["pairs"], "valid_pairs": r["valid_pairs"], "ratio_obs": r["ratio_obs"],
                "ratio_unobs": r["ratio_unobs"], "seconds": time.perf_counter() - t0, "dataset": ds, "precision": args.precision}
        if args.sift_baseline:
            line["ratio_sift"] = r["ratio_sift"]
        print(json.dumps(line), flush=True)
        return

    if args.completion_eval:
        if args.gpus > 1:
            raise SystemExit("--completion-eval runs on one GPU (--gpus 1): the losses are not sharded")
        import torch
        from types import SimpleNamespace
        from . import _lib, weights
        from .model import SCNet
        dev = _lib.require_gpu()
        ds = args.dataset
        mm, S, tanh = ("kinect", 21, 0) if ds == "scannet" else ("second", 21 if ds == "matterport" else 15, 1)
        net = SCNet(SimpleNamespace(batchnorm=1, useTanh=tanh, skipLayer=1, outputType="rgbdnsf", snumclass=S))
        net.load_state_dict(weights.make_state_dict(7, S))
        net.set_precision(args.precision)
        bs = min(args.batch, 32)
        batches = [SyntheticBatch(min(bs, args.pairs - k), args.seed + k, ds, mm, 1) for k in range(0, args.pairs, bs)]
        t0 = time.perf_counter()
        r = evaluate_completion(batches, net, dev, ds, mm, seed=args.seed)
        torch.cuda.synchronize()
        line = {"metric": "completion_loss", "pairs": r["pairs"], "valid_pairs": r["valid_pairs"], "n_bad_label": r["n_bad_label"],
                "type0": r["type0"], "type1": r["type1"], "seconds": time.perf_counter() - t0, "dataset": ds, "precision": args.precision}
        print(json.dumps(line), flush=True)
        return

    if args.method in ("fgs", "gs", "cgs"):
        m = args.method
        if args.gpus > 1:
            raise SystemExit(f"--method {m} runs on one GPU (--gpus 1): the baseline is not sharded")
        if args.dataset == "scannet":
            fn = {"fgs": "open3d_fast_global_registration", "gs": "open3d_global_registration", "cgs": "open3d_color_registration"}[m]
            raise SystemExit(f"--method {m}: the synthetic ScanNet pairs have no full-resolution depth, which the reference's baselines use "
                             f"(util.parse_data(..., 'scannet', '{m}')); run real 480x640 frames through util.parse_data and "
                             f"baselines.{fn}")
        import torch
        from . import _lib
        dev = _lib.require_gpu()
        mm = "second"
        batches = [make_batch(min(args.batch, args.pairs - k), args.seed + k, args.dataset, mm) or
                   SyntheticBatch(min(args.batch, args.pairs - k), args.seed + k, args.dataset, mm, args.keypoints)
                   for k in range(0, args.pairs, args.batch)]
        path = None if args.exp is None else args.exp + ".result.npy"
        t0 = time.perf_counter()
        stats = {"fgs": evaluate_fgs, "gs": evaluate_gs, "cgs": evaluate_cgs}[m](batches, dev, args.dataset, result_path=path, verify=args.verify,
                                                                                 fuse=args.fuse)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        line = {"method": m, "pairs": args.pairs, "records": len(stats), "seconds": dt, "result_file": path,
                "dataset": args.dataset, "stats": summarize(stats)}
        if args.verify is not None:
            line.update(verify=args.verify, **verify_summary(stats))
        if args.fuse is not None:
            line.update(fuse=args.fuse, **fuse_summary(stats))
        print(json.dumps(line), flush=True)
        return

    if args.verify is not None or args.fuse is not None:      # --method ours: the unsharded loop, which keeps every level's pose (and output) for the check
        import torch
        from types import SimpleNamespace
        from . import _lib, params, weights
        from .model import SCNet
        from .pipeline import RelativePosePipeline
        dev = _lib.require_gpu()
        ds = args.dataset
        mm, S, tanh = ("kinect", 21, 0) if ds == "scannet" else ("second", 21 if ds == "matterport" else 15, 1)
        net = SCNet(SimpleNamespace(batchnorm=1, useTanh=tanh, skipLayer=1, outputType="rgbdnsf", snumclass=S))
        net.load_state_dict(weights.make_state_dict(7, S))
        net.set_precision(args.precision)
        pipe = RelativePosePipeline(net, ds, mm, params.final_params(ds), completion=args.completion)
        lazy = [make_batch(min(args.batch, args.pairs - k), args.seed + k, ds, mm) or
                SyntheticBatch(min(args.batch, args.pairs - k), args.seed + k, ds, mm, args.keypoints) for k in range(0, args.pairs, args.batch)]
        path = None if args.exp is None else args.exp + ".result.npy"
        t0 = time.perf_counter()
        stats = evaluate_pairs(pipe, (_batch_take(b, np.arange(_batch_size(b))) for b in lazy), dev, result_path=path, normals=args.normals,
                               verify=args.verify, fuse=args.fuse)
        torch.cuda.synchronize()
        line = {"pairs": len(stats), "seconds": time.perf_counter() - t0, "n_gpus": 1, "result_file": path, "dataset": ds,
                "stats": summarize(stats), "verify": args.verify}
        if args.verify is not None:
            line.update(verify_summary(stats))
        if args.fuse is not None:
            line.update(fuse=args.fuse, **fuse_summary(stats))
        print(json.dumps(line), flush=True)
        return

    def worker():
        import torch
        from types import SimpleNamespace
        from . import distributed as D, params, weights
        from .model import SCNet
        from .pipeline import RelativePosePipeline
        rank, world, local = D.init_from_env()
        if world != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
        ds = args.dataset
        mm, S, tanh = ("kinect", 21, 0) if ds == "scannet" else ("second", 21 if ds == "matterport" else 15, 1)
        net = SCNet(SimpleNamespace(batchnorm=1, useTanh=tanh, skipLayer=1, outputType="rgbdnsf", snumclass=S))
        net.load_state_dict(weights.make_state_dict(7, S))
        net.set_precision(args.precision)
        pipe = RelativePosePipeline(net, ds, mm, params.final_params(ds), keypoints=args.keypoint_mode, completion=args.completion)
        batches = [make_batch(min(args.batch, args.pairs - k), args.seed + k, ds, mm) or
                   SyntheticBatch(min(args.batch, args.pairs - k), args.seed + k, ds, mm, args.keypoints,
                                  sift=args.sift if args.keypoint_mode == "reference" else 0, sift_detector=args.sift_detector)
                   for k in range(0, args.pairs, args.batch)]
        path = None if args.exp is None else args.exp + ".result.npy"
        D.barrier(world)
        t0 = time.perf_counter()
        n0 = D.COLLECTIVES["all_gather"]
        nhist = [None] if args.normals == "estimated" else None
        stats = evaluate_pairs_sharded(pipe, batches, dev, result_path=path, rank=rank, world=world, resume=not args.rm,
                                       round_batches=args.round_batches, normals=args.normals, normal_hist=nhist)
        torch.cuda.synchronize()
        D.barrier(world)
        dt = time.perf_counter() - t0
        if nhist is not None:
            hist = nhist[0] if nhist[0] is not None else torch.zeros(NORMAL_ERR_BINS, dtype=torch.float64, device=dev)
            if world > 1:
                import torch.distributed as dist
                hist = hist if dist.get_backend() == "nccl" else hist.cpu()
                dist.all_reduce(hist)
            hist = hist.cpu().numpy()
        if rank == 0:
            line = {"pairs": len(stats), "seconds": dt, "pairs_per_s_incl_host_rendering": len(stats) / dt, "n_gpus": world,
                    "pose_all_gathers": D.COLLECTIVES["all_gather"] - n0, "result_file": path, "dataset": ds,
                    "stats": summarize(stats)}
            if nhist is not None:
                line.update(normals="estimated", normal_err_deg_median=hist_quantile(hist, 0.5), normal_err_deg_p90=hist_quantile(hist, 0.9))
            print(json.dumps(line), flush=True)
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import torch
        import torch.multiprocessing as mp
        if torch.cuda.device_count() < args.gpus and not os.environ.get("RELPOSE_FORCE_DEVICE"):
            print(f"--gpus {args.gpus} requested but only {torch.cuda.device_count()} GPU(s) visible; refusing", file=sys.stderr)
            raise SystemExit(2)
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        mp.spawn(_spawned_eval, args=(argv if argv is not None else sys.argv[1:], args.gpus, port), nprocs=args.gpus, join=True)
        return
    worker()


def _spawned_eval(rank, argv, world, port):
    import os
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    main(argv)


if __name__ == "__main__":
    main()
