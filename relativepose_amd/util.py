"""Host-side mirror of the reference's panorama geometry (util.py), backed by
the HIP library.  The *_dev functions take/return CUDA tensors (batched, no host
round trip); the reference-named wrappers keep the reference's numpy signatures.

  apply_mask       util.py:209      warping          util.py:94
  Pano2PointCloud  util.py:751      build_view       evaluation.py:217-230
  sample_primitives  evaluation.py:246-253 + rpmodule.getMatchingPrimitive :526-532
"""
import numpy as np

from . import _lib

DATASETS = {"suncg": 0, "matterport": 1, "scannet": 2}
MASKS = {"second": 0, "kinect": 1}


def dataset_id(name):
    for k, v in DATASETS.items():
        if k in name:
            return v
    raise ValueError(f"unknown dataset {name}")


def build_view_dev(rgb, norm, depth, mask_method):
    """rgb/norm [n,3,h,4h], depth [n,h,4h] f32 CUDA -> view [n,8,h,4h]."""
    import torch
    _lib.require_gpu()
    n, _, h, w = rgb.shape
    assert w == 4 * h
    view = torch.empty(n, 8, h, w, dtype=torch.float32, device=rgb.device)
    rc = _lib.lib().relpose_build_view(_lib.ptr(rgb.contiguous()), _lib.ptr(norm.contiguous()), _lib.ptr(depth.contiguous()),
                                       _lib.ptr(view), n, h, MASKS[mask_method], _lib.stream_ptr())
    _lib.check(rc, "relpose_build_view")
    return view


def apply_mask_dev(x, mask_method):
    import torch
    _lib.require_gpu()
    n, c, h, w = x.shape
    assert w == 4 * h and x.is_contiguous() and x.dtype == torch.float32
    mask = torch.empty(n, 1, h, w, dtype=torch.float32, device=x.device)
    rc = _lib.lib().relpose_apply_mask(_lib.ptr(x), _lib.ptr(mask), n, c, h, MASKS[mask_method], _lib.stream_ptr())
    _lib.check(rc, "relpose_apply_mask")
    return x, mask


_warp_ws = {}


def warping_dev(view, pose, dataset, out=None):
    """view [n,8,h,4h] f32, pose [n,4,4] f64 (CUDA) -> warped view [n,8,h,4h] f32."""
    import torch
    _lib.require_gpu()
    n, c, h, w = view.shape
    assert c == 8 and w == 4 * h and view.is_contiguous() and pose.is_contiguous() and pose.dtype == torch.float64
    L = _lib.lib()
    nbytes = L.relpose_warp_workspace_bytes(n, h)
    key = (view.device.index, torch.cuda.current_stream().cuda_stream)
    ws = _warp_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=view.device)       # (zeros: every warp call leaves its keys reset, see warp_pairs_dev)
        _warp_ws[key] = ws
    if out is None:
        out = torch.empty_like(view)
    rc = L.relpose_warp(_lib.ptr(view), _lib.ptr(pose), _lib.ptr(out), _lib.ptr(ws), n, h, dataset_id(dataset), _lib.stream_ptr())
    _lib.check(rc, "relpose_warp")
    return out


def warp_pairs_dev(x, pose, dataset):
    """In place on the network input x [n,16,h,4h]: x[i, 8:16] = warping(x[i^1, 0:8], pose[i]) (relpose_warp_pairs)."""
    import torch
    _lib.require_gpu()
    n, c, h, w = x.shape
    assert c == 16 and w == 4 * h and n % 2 == 0 and x.is_contiguous() and pose.is_contiguous() and pose.dtype == torch.float64
    L = _lib.lib()
    nbytes = L.relpose_warp_workspace_bytes(n, h)
    key = (x.device.index, torch.cuda.current_stream().cuda_stream)
    ws = _warp_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=x.device)
        _warp_ws[key] = ws
    # the workspace was zero-initialised and every call resets the keys it consumed: no memset in front of the scatter pass
    rc = L.relpose_warp_pairs2(_lib.ptr(x), _lib.ptr(pose), _lib.ptr(ws), n, h, dataset_id(dataset), 1, _lib.stream_ptr())
    _lib.check(rc, "relpose_warp_pairs2")
    return x


def pose_inverse_dev(pose):
    import torch
    out = torch.empty_like(pose)
    rc = _lib.lib().relpose_pose_inverse(_lib.ptr(pose), _lib.ptr(out), pose.shape[0], _lib.stream_ptr())
    _lib.check(rc, "relpose_pose_inverse")
    return out


def pano2pc_dev(depth, dataset):
    """depth [n,h,4h] f32 -> (pc [n,3,4hh] f64, valid [n,4hh] uint8)."""
    import torch
    _lib.require_gpu()
    n, h, w = depth.shape
    pc = torch.empty(n, 3, h * w, dtype=torch.float64, device=depth.device)
    valid = torch.empty(n, h * w, dtype=torch.uint8, device=depth.device)
    rc = _lib.lib().relpose_pano2pc(_lib.ptr(depth.contiguous()), _lib.ptr(pc), _lib.ptr(valid), n, h, dataset_id(dataset),
                                    _lib.stream_ptr())
    _lib.check(rc, "relpose_pano2pc")
    return pc, valid


def depth_normals_dev(depth, dataset, radius=3, gate_scale=3.0, min_neighbors=6, stages=False, out=None):
    """depth [n,h,4h] f32 CUDA (0 = no data) -> (normal [n,3,h,4h] f32, valid [n,h,4h] uint8): one normal per panorama pixel from the
    covariance of the unprojected points of its (2 radius + 1)^2 window (relpose_depth_normals; the contract is DESIGN.md §4.12).
    stages=True: also (count [n,h,4h] i32, moments [n,9,h,4h] f32).  out: an existing [n,3,h,4h] f32 tensor to write the normals into.
    Only enqueues on the current stream."""
    import ctypes as C
    import torch
    _lib.require_gpu()
    n, h, w = depth.shape
    assert w == 4 * h and depth.dtype == torch.float32 and depth.is_cuda
    depth = depth.contiguous()
    dev = depth.device
    if out is None:
        out = torch.empty(n, 3, h, w, dtype=torch.float32, device=dev)
    assert out.shape == (n, 3, h, w) and out.dtype == torch.float32 and out.is_contiguous() and out.device == dev
    valid = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
    count = torch.empty(n, h, w, dtype=torch.int32, device=dev) if stages else None
    moments = torch.empty(n, 9, h, w, dtype=torch.float32, device=dev) if stages else None
    a = _lib.DepthNormalsArgs()
    a.struct_size = C.sizeof(a)
    a.n_views, a.h, a.dataset, a.radius, a.min_neighbors, a.gate_scale = n, h, dataset_id(dataset), int(radius), int(min_neighbors), float(gate_scale)
    a.depth, a.normal, a.valid, a.count, a.moments = _lib.ptr(depth), _lib.ptr(out), _lib.ptr(valid), _lib.ptr(count), _lib.ptr(moments)
    a.stream = _lib.stream_ptr()
    _lib.check(_lib.lib().relpose_depth_normals(C.byref(a)), "relpose_depth_normals")
    return (out, valid, count, moments) if stages else (out, valid)


# (sx, sy) of util.depth2pc's 480x640 branch (reference util.py:499-507): x = xn z / sx, y = yn z / sy
SCANNET_FRAME_SCALE = (0.8921875 * 2, 1.1895 * 2)


def frame_scale(fx, fy, Wf, Hf):
    """(sx, sy) of a pinhole camera with focal lengths fx, fy in pixels and its principal point at the centre of a Wf x Hf frame."""
    return 2.0 * fx / Wf, 2.0 * fy / Hf


def _pano_box(box, h):
    if box is None:
        return (-1, -1, -1, -1)
    if isinstance(box, str):
        from . import synth
        return tuple(int(b) for b in synth.observed_box(box, h))
    y0, y1, x0, x1 = (int(b) for b in box)
    return y0, y1, x0, x1


_pano_ws = {}


def frames_to_pano_dev(depth, rgb, scale, pose=None, dataset="scannet", h=160, box="kinect", gate=0.05, normals=False, stages=False, out=None):
    """Posed perspective RGB-D frames -> four-face skybox panoramas (relpose_frames_to_pano; the contract is DESIGN.md §4.13).
    depth [n,F,Hf,Wf] f32 CUDA (<= 0 or non-finite = no data), rgb [n,F,Hf,Wf,3] uint8, scale [n,F,2] f64 (sx, sy) or one (sx, sy) pair for
    every frame, pose [n,F,4,4] f64 frame -> panorama (None = identity).  box: a mask method name (synth.observed_box), (y0,y1,x0,x1) in
    panorama pixels, or None.  Returns (rgb [n,3,h,4h] f32, depth [n,h,4h] f32, valid [n,h,4h] uint8); normals=True appends the normals of
    depth_normals_dev on the built depth, stages=True appends (zmin [n,h,4h] i32: the bits of the f32 minimum, count [n,h,4h] i32, sum_z
    [n,h,4h] i64, sum_rgb [n,3,h,4h] i32).  out: existing (rgb, depth, valid) tensors to write into.  Only enqueues on the current stream."""
    import ctypes as C
    import torch
    _lib.require_gpu()
    assert depth.dim() == 4 and depth.dtype == torch.float32 and depth.is_cuda
    n, F, Hf, Wf = depth.shape
    assert rgb.shape == (n, F, Hf, Wf, 3) and rgb.dtype == torch.uint8 and rgb.device == depth.device
    dev = depth.device
    depth, rgb = depth.contiguous(), rgb.contiguous()
    if not torch.is_tensor(scale):
        scale = torch.tensor(np.broadcast_to(np.asarray(scale, np.float64), (n, F, 2)).copy(), device=dev)
    assert scale.shape == (n, F, 2) and scale.dtype == torch.float64 and scale.device == dev
    scale = scale.contiguous()
    if pose is not None:
        assert pose.shape == (n, F, 4, 4) and pose.dtype == torch.float64 and pose.device == dev
        pose = pose.contiguous()
    w = 4 * h
    if out is None:
        out = (torch.empty(n, 3, h, w, dtype=torch.float32, device=dev), torch.empty(n, h, w, dtype=torch.float32, device=dev),
               torch.empty(n, h, w, dtype=torch.uint8, device=dev))
    o_rgb, o_depth, o_valid = out
    assert o_rgb.shape == (n, 3, h, w) and o_rgb.dtype == torch.float32 and o_rgb.is_contiguous() and o_rgb.device == dev
    assert o_depth.shape == (n, h, w) and o_depth.dtype == torch.float32 and o_depth.is_contiguous() and o_depth.device == dev
    assert o_valid.shape == (n, h, w) and o_valid.dtype == torch.uint8 and o_valid.is_contiguous() and o_valid.device == dev
    st = None
    if stages:
        st = (torch.empty(n, h, w, dtype=torch.int32, device=dev), torch.empty(n, h, w, dtype=torch.int32, device=dev),
              torch.empty(n, h, w, dtype=torch.int64, device=dev), torch.empty(n, 3, h, w, dtype=torch.int32, device=dev))
    L = _lib.lib()
    nbytes = L.relpose_frames_to_pano_workspace_bytes(n, h)
    if nbytes == 0:
        raise ValueError(f"frames_to_pano: {n} views at h = {h} (h must be even, 2..8192)")
    key = (dev.index, torch.cuda.current_stream().cuda_stream)
    ws = _pano_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _pano_ws[key] = ws
    a = _lib.FramesToPanoArgs()
    a.struct_size = C.sizeof(a)
    a.n_views, a.n_frames, a.frame_h, a.frame_w, a.h, a.dataset, a.gate = n, F, Hf, Wf, h, dataset_id(dataset), float(gate)
    a.box[:] = _pano_box(box, h)
    a.depth, a.rgb, a.scale, a.pose = _lib.ptr(depth), _lib.ptr(rgb), _lib.ptr(scale), _lib.ptr(pose)
    a.out_depth, a.out_rgb, a.out_valid = _lib.ptr(o_depth), _lib.ptr(o_rgb), _lib.ptr(o_valid)
    if stages:
        a.zmin, a.count, a.sum_z, a.sum_rgb = (_lib.ptr(t) for t in st)
    a.workspace, a.workspace_bytes, a.stream = _lib.ptr(ws), ws.numel(), _lib.stream_ptr()
    _lib.check(L.relpose_frames_to_pano(C.byref(a)), "relpose_frames_to_pano")
    res = (o_rgb, o_depth, o_valid)
    if normals:
        res += (depth_normals_dev(o_depth, dataset)[0],)
    if stages:
        res += (st,)
    return res


def sample_primitives_dev(f, feat_off, obs_norm, obs_depth, pts, npts, mask_method, dataset, compose=0):
    """f [n,cf,h,4h] net output, obs_norm [n,3,h,4h], obs_depth [n,h,4h] f32, pts [n,N,2] f64, npts [n] i32
    -> pc [n,N,3] f64, normal [n,N,3] f64, feat [n,N,32] f32.  compose: 0 = evaluation.py:250-251, 1 = rpmodule.py:633-634."""
    import torch
    _lib.require_gpu()
    n, cf, h, w = f.shape
    N = pts.shape[1]
    dev = f.device
    pc = torch.zeros(n, N, 3, dtype=torch.float64, device=dev)
    nn = torch.zeros(n, N, 3, dtype=torch.float64, device=dev)
    ft = torch.zeros(n, N, 32, dtype=torch.float32, device=dev)
    for t in (f, obs_norm, obs_depth, pts, npts):
        assert t.is_contiguous() and t.is_cuda
    rc = _lib.lib().relpose_sample_primitives(_lib.ptr(f), cf, feat_off, _lib.ptr(obs_norm), _lib.ptr(obs_depth), _lib.ptr(pts),
                                              _lib.ptr(npts), N, _lib.ptr(pc), _lib.ptr(nn), _lib.ptr(ft), n, h,
                                              MASKS[mask_method], int(compose), dataset_id(dataset), _lib.stream_ptr())
    _lib.check(rc, "relpose_sample_primitives")
    return pc, nn, ft


# ---- reference-named numpy wrappers -------------------------------------------------------------

def apply_mask(x, maskMethod, *arg):
    """util.py:209: x torch tensor [n,c,h,w] -> (x*mask, mask, geow).  geow (a training-only
    geometric weight) is not computed on the inference path and is returned as None."""
    import torch
    dev = _lib.require_gpu()
    xd = x.to(dev, torch.float32).contiguous().clone()
    xd, m = apply_mask_dev(xd, maskMethod)
    return xd, m, None


def warping(view, R, dataList):
    """util.py:94: view numpy [1,8,h,4h], R [4,4] -> numpy [1,8,h,4h] (float32 values; zeros for identity)."""
    import torch
    dev = _lib.require_gpu()
    v = torch.from_numpy(np.ascontiguousarray(view, dtype=np.float32)).to(dev)
    T = torch.from_numpy(np.ascontiguousarray(R, dtype=np.float64)[None]).to(dev)
    return warping_dev(v, T, dataList).cpu().numpy()


def Pano2PointCloud(depth, dataList):
    """util.py:751: depth numpy [h,4h] -> [3,n] float64 (scannet: zero-depth points dropped)."""
    import torch
    dev = _lib.require_gpu()
    d = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)[None]).to(dev)
    pc, valid = pano2pc_dev(d, dataList)
    pc, valid = pc[0].cpu().numpy(), valid[0].cpu().numpy().astype(bool)
    return pc[:, valid]


def depth_normals(depth, dataList, radius=3, gate_scale=3.0, min_neighbors=6):
    """Normal maps for depth panoramas that come without one (the reference's loaders read them from a normal/ folder,
    datasets/SUNCG.py:300-313): depth numpy [h,4h] -> [3,h,4h], or [B,2,h,4h] -> [B,2,3,h,4h], float32, the dataset dict's `norm` layout;
    (0,0,0) where no normal could be estimated."""
    import torch
    dev = _lib.require_gpu()
    d = np.ascontiguousarray(depth, dtype=np.float32)
    if d.ndim not in (2, 4):
        raise ValueError("depth_normals takes depth [h,4h] or [B,2,h,4h]")
    h, w = d.shape[-2:]
    nrm, _ = depth_normals_dev(torch.from_numpy(d.reshape(-1, h, w)).to(dev), dataList, radius, gate_scale, min_neighbors)
    nrm = nrm.cpu().numpy()
    return nrm[0] if d.ndim == 2 else nrm.reshape(d.shape[0], 2, 3, h, w)


def frames_uint8(rgb_full):
    """Frames in the loader layout [..., 3, Hf, Wf] (float in 0..1, quantised like the reference's (x * 255).astype(uint8), or uint8)
    -> uint8 [..., Hf, Wf, 3]."""
    x = np.asarray(rgb_full)
    if x.dtype != np.uint8:
        x = (x * 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(x, -3, -1))


def frames_to_pano(depth_full, rgb_full, dataList, scale=SCANNET_FRAME_SCALE, pose=None, h=160, box="kinect", gate=0.05):
    """The panorama version of perspective frames in the loader layout (the reference's ScanNet loader reads both from disk,
    datasets/ScanNet.py:211-230): depth_full numpy [B,2,Hf,Wf], rgb_full [B,2,3,Hf,Wf] (float in 0..1 or uint8), one frame per view
    -> (rgb [B,2,3,h,4h], depth [B,2,h,4h], norm [B,2,3,h,4h]) float32, the dataset dict's entries; the normals are depth_normals_dev's
    on the built depth.  pose: [B,2,4,4] frame -> panorama, or None."""
    import torch
    dev = _lib.require_gpu()
    d = np.ascontiguousarray(depth_full, dtype=np.float32)
    if d.ndim != 4 or d.shape[1] != 2:
        raise ValueError("frames_to_pano takes depth_full [B,2,Hf,Wf]")
    B, _, Hf, Wf = d.shape
    c = frames_uint8(rgb_full)
    if c.shape != (B, 2, Hf, Wf, 3):
        raise ValueError("frames_to_pano takes rgb_full [B,2,3,Hf,Wf]")
    p = None if pose is None else torch.from_numpy(np.ascontiguousarray(pose, dtype=np.float64).reshape(2 * B, 1, 4, 4)).to(dev)
    rgb, dep, _, nrm = frames_to_pano_dev(torch.from_numpy(d.reshape(2 * B, 1, Hf, Wf)).to(dev), torch.from_numpy(c.reshape(2 * B, 1, Hf, Wf, 3)).to(dev),
                                          scale, p, dataList, h, box, gate, normals=True)
    w = 4 * h
    return rgb.cpu().numpy().reshape(B, 2, 3, h, w), dep.cpu().numpy().reshape(B, 2, h, w), nrm.cpu().numpy().reshape(B, 2, 3, h, w)


# ---- evaluation-side statistics ---------------------------------------------------------------

def depth2pc_dev(depth, dataset):
    """depth [n,h,4h] f32 CUDA -> (pc [n,P,3] f64, valid [n,P] uint8) of the observed block (util.depth2pc)."""
    import torch
    _lib.require_gpu()
    n, h, w = depth.shape
    L = _lib.lib()
    P = L.relpose_observed_points(h, dataset_id(dataset))
    pc = torch.empty(n, P, 3, dtype=torch.float64, device=depth.device)
    valid = torch.empty(n, P, dtype=torch.uint8, device=depth.device)
    _lib.check(L.relpose_depth2pc(_lib.ptr(depth.contiguous()), _lib.ptr(pc), _lib.ptr(valid), n, h, dataset_id(dataset), _lib.stream_ptr()),
               "relpose_depth2pc")
    return pc, valid


def nn_dist_dev(query, ref, pose=None, query_valid=None, ref_valid=None):
    """min distance of every (pose-moved) query point [nq,3] to the reference set [nr,3] (f64 CUDA tensors)."""
    import torch
    out = torch.empty(query.shape[0], dtype=torch.float64, device=query.device)
    rc = _lib.lib().relpose_nn_dist(_lib.ptr(query.contiguous()), _lib.ptr(query_valid), query.shape[0], _lib.ptr(ref.contiguous()),
                                    _lib.ptr(ref_valid), ref.shape[0], _lib.ptr(pose), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "relpose_nn_dist")
    return out


def point_cloud_overlap(pc_src, pc_tgt, R_gt_44):
    """util.py:21-40 with the two KDTree queries replaced by brute-force GPU nearest neighbours.
    numpy in, (overlap_val, cam_dist, pc_dist, pc_nn) out."""
    import torch
    dev = _lib.require_gpu()
    ps = torch.from_numpy(np.ascontiguousarray(pc_src, dtype=np.float64)).to(dev)
    pt = torch.from_numpy(np.ascontiguousarray(pc_tgt, dtype=np.float64)).to(dev)
    R = np.ascontiguousarray(R_gt_44, dtype=np.float64)
    d_s2t = nn_dist_dev(ps, pt, torch.from_numpy(R).to(dev)).cpu().numpy()
    d_t2s = nn_dist_dev(pt, ps, torch.from_numpy(np.ascontiguousarray(np.linalg.inv(R))).to(dev)).cpu().numpy()
    ov = max((d_s2t < 0.08).sum() / pc_src.shape[0], (d_t2s < 0.08).sum() / pc_tgt.shape[0])
    src_trans = np.matmul(R[:3, :3], pc_src.T) + R[:3, 3:4]
    return ov, np.linalg.norm(R[:3, 3]), np.linalg.norm(src_trans.mean(1) - pc_tgt.T.mean(1)), (d_s2t.min() + d_t2s.min()) / 2


def overlap_dev(pc, valid, query_cloud, ref_cloud, pose, max_dist=0.08, want_hit=False):
    """relpose_overlap (include/relpose.h): pc [n,P,3] f64 and valid [n,P] u8 (or None: all valid) CUDA tensors in
    depth2pc_dev's layout; query_cloud, ref_cloud: n_queries cloud indices (any integer sequence, array or tensor; they are read on the
    host); pose [n_queries,4,4] f64 CUDA, query cloud -> the reference cloud's frame.
    -> (hits [n_queries] i32, nn_min [n_queries] f64, n_valid [n] i32), and hit [n_queries,P] u8 with want_hit.  One grid per cloud per
    call, shared by every query that names the cloud; the call waits for the stream once, at its end."""
    import torch
    _lib.require_gpu()
    as_host = lambda v: np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v, dtype=np.int32).reshape(-1)
    qc, rc = as_host(query_cloud), as_host(ref_cloud)
    if pc.dim() != 3 or pc.shape[2] != 3 or pc.dtype != torch.float64:
        raise ValueError("overlap_dev takes pc [n,P,3] float64")
    n, P = int(pc.shape[0]), int(pc.shape[1])
    nq = len(qc)
    if len(rc) != nq or tuple(pose.shape) != (nq, 4, 4) or pose.dtype != torch.float64:
        raise ValueError("overlap_dev takes one reference cloud and one float64 4x4 pose per query")
    if valid is not None and (tuple(valid.shape) != (n, P) or valid.dtype != torch.uint8):
        raise ValueError("overlap_dev takes valid [n,P] uint8")
    dev = pc.device
    hits = torch.empty(nq, dtype=torch.int32, device=dev)
    nn_min = torch.empty(nq, dtype=torch.float64, device=dev)
    n_valid = torch.empty(n, dtype=torch.int32, device=dev)
    hit = torch.empty(nq, P, dtype=torch.uint8, device=dev) if want_hit else None
    if nq == 0 or n == 0 or P == 0:
        if n and not P:
            n_valid.zero_()
        return (hits, nn_min, n_valid, hit) if want_hit else (hits, nn_min, n_valid)
    L = _lib.lib()
    nbytes = L.relpose_overlap_workspace_bytes(n, P, nq)
    if nbytes == 0:
        raise ValueError("overlap_dev: sizes outside relpose_overlap's limits")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pcc, vc, posec = pc.contiguous(), (None if valid is None else valid.contiguous()), pose.contiguous()
    a = _lib.OverlapArgs()
    a.struct_size = _lib.C.sizeof(_lib.OverlapArgs)
    a.n_clouds, a.n_points, a.n_queries = n, P, nq
    a.pc, a.valid, a.pose = pcc.data_ptr(), (0 if vc is None else vc.data_ptr()), posec.data_ptr()
    a.query_cloud_host, a.ref_cloud_host = qc.ctypes.data, rc.ctypes.data
    a.max_dist = float(max_dist)
    a.hits, a.nn_min, a.n_valid, a.hit = hits.data_ptr(), nn_min.data_ptr(), n_valid.data_ptr(), (hit.data_ptr() if want_hit else 0)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.stream = _lib.stream_ptr()
    rc_ = L.relpose_overlap(_lib.C.byref(a))
    if rc_ == _lib.OVERLAP_EXTENT:
        raise RuntimeError("relpose_overlap: a cloud's finite points span more than 2^20 grid cells along an axis at this max_dist")
    _lib.check(rc_, "relpose_overlap")
    return (hits, nn_min, n_valid, hit) if want_hit else (hits, nn_min, n_valid)


def point_cloud_overlap_dev(pc, valid, R_gt, max_dist=0.08):
    """point_cloud_overlap for a batch of pairs without leaving the device: pc [2B,P,3] f64, valid [2B,P] u8 CUDA tensors in the paired
    layout (cloud 2b = the source of pair b, 2b + 1 its target, as depth2pc_dev writes them), R_gt [B,4,4] host float64 (source -> target)
    -> (overlap, cam_dist, pc_dist, pc_nn) float64 CUDA tensors [B].  One relpose_overlap call with 2B directed queries; the inverse poses
    are np.linalg.inv on the host, as point_cloud_overlap computes them.  overlap = max(hits_s2t / n_src, hits_t2s / n_tgt) and
    pc_nn = (nn_s2t + nn_t2s) / 2 are bitwise point_cloud_overlap's on the pair's valid points.  pc_dist, the distance between the moved
    source's mean and the target's mean, is computed with float64 torch reductions on the device: it is NOT bitwise numpy's pairwise
    mean (it agrees to about 1e-15 relative; the evaluation drivers keep the host expression for their records).  A pair with an empty
    cloud gets overlap 0, pc_nn = +inf and pc_dist NaN."""
    import torch
    R = np.ascontiguousarray(R_gt, dtype=np.float64).reshape(-1, 4, 4)
    B = R.shape[0]
    if pc.shape[0] != 2 * B:
        raise ValueError("point_cloud_overlap_dev takes two clouds per pose")
    dev = pc.device
    poses = np.empty((2 * B, 4, 4))
    for b in range(B):
        poses[2 * b] = R[b]
        poses[2 * b + 1] = np.linalg.inv(R[b])
    src, tgt = np.arange(0, 2 * B, 2), np.arange(1, 2 * B, 2)
    qc = np.stack((src, tgt), 1).reshape(-1)
    rc = np.stack((tgt, src), 1).reshape(-1)
    Rd = torch.from_numpy(R).to(dev)
    hits, nn_min, n_valid = overlap_dev(pc, valid, qc, rc, torch.from_numpy(poses).to(dev), max_dist)
    n = n_valid.to(torch.float64).reshape(B, 2)
    frac = hits.to(torch.float64).reshape(B, 2) / n
    frac = torch.where(n > 0, frac, torch.zeros_like(frac))
    overlap = torch.maximum(frac[:, 0], frac[:, 1])
    overlap = torch.where((n > 0).all(1), overlap, torch.zeros_like(overlap))
    nn = nn_min.reshape(B, 2)
    pc_nn = (nn[:, 0] + nn[:, 1]) / 2
    m = (torch.ones(pc.shape[:2], dtype=torch.bool, device=dev) if valid is None else valid != 0).unsqueeze(-1)
    mean = torch.where(m, pc, torch.zeros_like(pc)).sum(1) / n.reshape(2 * B, 1)                     # [2B,3]
    ms, mt = mean[0::2], mean[1::2]
    moved = torch.einsum("bij,bj->bi", Rd[:, :3, :3], ms) + Rd[:, :3, 3]
    pc_dist = (moved - mt).norm(dim=1)
    cam_dist = Rd[:, :3, 3].norm(dim=1)
    return overlap, cam_dist, pc_dist, pc_nn


def overlap_matrix_dev(pc, valid, R, max_dist=0.08):
    """Which of M posed clouds overlap, and by how much: pc [M,P,3] f64, valid [M,P] u8 CUDA tensors, R [M,4,4] host float64 world -> camera
    poses (the loaders' convention).  T_ij = R_j inv(R_i) moves cloud i into cloud j's frame: the product evaluate_pairs forms for R_gt.
    -> (frac [M,M] f64, nn_min [M,M] f64, n_valid [M] i32) CUDA tensors from ONE relpose_overlap call with M (M - 1) directed queries:
    frac[i,j] = the share of cloud i's valid points with a point of cloud j within max_dist (0 for an empty cloud i), nn_min[i,j] their
    closest-pair distance.  The diagonal is frac 1 (0 for an empty cloud) and nn_min 0 (+inf for an empty cloud) without being computed."""
    import torch
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(-1, 4, 4)
    M = R.shape[0]
    if pc.shape[0] != M:
        raise ValueError("overlap_matrix_dev takes one pose per cloud")
    dev = pc.device
    inv = [np.linalg.inv(R[i]) for i in range(M)]
    ij = [(i, j) for i in range(M) for j in range(M) if i != j]
    frac = torch.zeros(M, M, dtype=torch.float64, device=dev)
    nn = torch.full((M, M), float("inf"), dtype=torch.float64, device=dev)
    if not ij:
        n_valid = (torch.full((M,), pc.shape[1], dtype=torch.int32, device=dev) if valid is None else (valid != 0).sum(1).to(torch.int32))
    else:
        poses = np.stack([np.matmul(R[j], inv[i]) for i, j in ij])
        qi = torch.tensor([i for i, _ in ij], device=dev)
        qj = torch.tensor([j for _, j in ij], device=dev)
        hits, nn_min, n_valid = overlap_dev(pc, valid, [i for i, _ in ij], [j for _, j in ij], torch.from_numpy(poses).to(dev), max_dist)
        nq = n_valid.to(torch.float64)[qi]
        f = hits.to(torch.float64) / nq
        frac[qi, qj] = torch.where(nq > 0, f, torch.zeros_like(f))
        nn[qi, qj] = nn_min
    d = torch.arange(M, device=dev)
    some = n_valid > 0
    frac[d, d] = some.to(torch.float64)
    nn[d, d] = torch.where(some, torch.zeros(M, dtype=torch.float64, device=dev), torch.full((M,), float("inf"), dtype=torch.float64, device=dev))
    return frac, nn, n_valid


VIS_CLASSES = ("invalid", "outside", "unobserved", "consistent", "violation", "occluded")      # relpose_visibility's classes 0..5


def visibility_dev(pc, valid, depth, query_cloud, ref_view, pose, dataset, tol_abs=0.05, tol_rel=0.02, radius=1, want_class=False):
    """relpose_visibility (include/relpose.h): pc [n,P,3] f64 and valid [n,P] u8 (or None: all valid) CUDA tensors in
    depth2pc_dev's layout; depth [V,h,4h] f32 CUDA reference panoramas (not finite or <= 0 = no data); query_cloud, ref_view: n_queries
    cloud / view indices (any integer sequence, array or tensor; they are read on the host); pose [n_queries,4,4] f64 CUDA, query cloud ->
    the reference view's frame.  Every moved point is projected into the reference panorama and compared with the (2 radius + 1)^2 window
    of depths around its pixel: VIS_CLASSES names the six classes.
    -> (counts [n_queries,6] i32, margin_sum [n_queries] i64: the violations' depth margins in 1/65536), and cls [n_queries,P] u8 with
    want_class.  The defaults are parameters of the library, not claims about real sensors.  The call waits for the stream once, at its end."""
    import torch
    _lib.require_gpu()
    as_host = lambda v: np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v, dtype=np.int32).reshape(-1)
    qc, rv = as_host(query_cloud), as_host(ref_view)
    if pc.dim() != 3 or pc.shape[2] != 3 or pc.dtype != torch.float64:
        raise ValueError("visibility_dev takes pc [n,P,3] float64")
    if depth.dim() != 3 or depth.shape[2] != 4 * depth.shape[1] or depth.dtype != torch.float32 or depth.device != pc.device:
        raise ValueError("visibility_dev takes depth [V,h,4h] float32 on pc's device")
    n, P = int(pc.shape[0]), int(pc.shape[1])
    V, h = int(depth.shape[0]), int(depth.shape[1])
    nq = len(qc)
    if len(rv) != nq or tuple(pose.shape) != (nq, 4, 4) or pose.dtype != torch.float64:
        raise ValueError("visibility_dev takes one reference view and one float64 4x4 pose per query")
    if valid is not None and (tuple(valid.shape) != (n, P) or valid.dtype != torch.uint8):
        raise ValueError("visibility_dev takes valid [n,P] uint8")
    if int(radius) not in (0, 1, 2) or not (np.isfinite(tol_abs) and tol_abs >= 0 and np.isfinite(tol_rel) and tol_rel >= 0):
        raise ValueError("visibility_dev takes radius 0, 1 or 2 and finite tolerances >= 0")
    dev = pc.device
    counts = torch.zeros(nq, 6, dtype=torch.int32, device=dev)
    margin = torch.zeros(nq, dtype=torch.int64, device=dev)
    cls = torch.zeros(nq, P, dtype=torch.uint8, device=dev) if want_class else None
    if nq == 0 or n == 0 or P == 0:
        return (counts, margin, cls) if want_class else (counts, margin)
    L = _lib.lib()
    nbytes = L.relpose_visibility_workspace_bytes(V, h, nq)
    if nbytes == 0:
        raise ValueError("visibility_dev: sizes outside relpose_visibility's limits")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pcc, vc, dc, posec = pc.contiguous(), (None if valid is None else valid.contiguous()), depth.contiguous(), pose.contiguous()
    a = _lib.VisibilityArgs()
    a.struct_size = _lib.C.sizeof(_lib.VisibilityArgs)
    a.n_clouds, a.n_points, a.n_views, a.h, a.n_queries = n, P, V, h, nq
    a.dataset, a.radius = dataset_id(dataset), int(radius)
    a.pc, a.valid, a.depth, a.pose = pcc.data_ptr(), (0 if vc is None else vc.data_ptr()), dc.data_ptr(), posec.data_ptr()
    a.query_cloud_host, a.ref_view_host = qc.ctypes.data, rv.ctypes.data
    a.tol_abs, a.tol_rel = float(tol_abs), float(tol_rel)
    a.counts, a.margin_sum, a.cls = counts.data_ptr(), margin.data_ptr(), (cls.data_ptr() if want_class else 0)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.stream = _lib.stream_ptr()
    rc_ = L.relpose_visibility(_lib.C.byref(a))
    if rc_ == -1:
        raise ValueError("relpose_visibility: invalid arguments (an index out of range, h odd or < 2 radius + 1, or sizes outside the limits)")
    _lib.check(rc_, "relpose_visibility")
    return (counts, margin, cls) if want_class else (counts, margin)


def visibility_scores(counts, margin_sum):
    """The ratios behind a visibility verdict: counts [...,6], margin_sum [...] (visibility_dev's, or sums of them) -> a dict of float64
    tensors [...]: with c, v, o = the consistent, violation and occluded counts, agreement = c / (c + v + o), violation_rate = v / (c + v + o),
    observed = (c + v + o) / (n_points - invalid), mean_violation = margin_sum / 65536 / v (the mean depth by which a violating point stands
    in front of the measured surface).  An entry is NaN where its denominator is 0."""
    import torch
    cn = counts.to(torch.float64)
    c, v, o = cn[..., 3], cn[..., 4], cn[..., 5]
    seen = (c + v) + o
    n = cn.sum(-1) - cn[..., 0]
    nan = torch.full_like(seen, float("nan"))
    div = lambda a, b: torch.where(b > 0, a / torch.where(b > 0, b, torch.ones_like(b)), nan)
    return {"agreement": div(c, seen), "violation_rate": div(v, seen), "observed": div(seen, n),
            "mean_violation": div(margin_sum.to(torch.float64) / 65536.0, v)}


def pose_visibility_dev(pc, valid, depth, T, dataset, tol_abs=0.05, tol_rel=0.02, radius=1):
    """Visibility scores of K candidate poses per pair without leaving the device: pc [2B,P,3] f64, valid [2B,P] u8, depth [2B,h,4h] f32
    CUDA tensors in point_cloud_overlap_dev's paired layout (cloud and view 2b = the source of pair b, 2b + 1 its target), T [B,K,4,4] host
    float64 candidates, source -> target.  ONE relpose_visibility call with the 2 B K directed queries (source cloud into the target view
    under T, target cloud into the source view under np.linalg.inv(T) from the host).
    -> (counts [B,K,2,6] i32, margin_sum [B,K,2] i64 per direction, scores: visibility_scores of both directions' sums, [B,K] each)."""
    import torch
    T = np.ascontiguousarray(T, dtype=np.float64)
    if T.ndim != 4 or T.shape[2:] != (4, 4) or pc.shape[0] != 2 * T.shape[0] or depth.shape[0] != pc.shape[0]:
        raise ValueError("pose_visibility_dev takes T [B,K,4,4] and two clouds and two views per pair")
    B, K = T.shape[:2]
    poses = np.empty((B, K, 2, 4, 4))
    qc = np.empty((B, K, 2), np.int32)
    rv = np.empty((B, K, 2), np.int32)
    for b in range(B):
        for k in range(K):
            poses[b, k, 0] = T[b, k]
            poses[b, k, 1] = np.linalg.inv(T[b, k])
        qc[b, :, 0], rv[b, :, 0] = 2 * b, 2 * b + 1
        qc[b, :, 1], rv[b, :, 1] = 2 * b + 1, 2 * b
    counts, margin = visibility_dev(pc, valid, depth, qc, rv, torch.from_numpy(poses.reshape(-1, 4, 4)).to(pc.device), dataset,
                                    tol_abs, tol_rel, radius)
    counts, margin = counts.reshape(B, K, 2, 6), margin.reshape(B, K, 2)
    return counts, margin, visibility_scores(counts.sum(2), margin.sum(2))


def visibility_matrix_dev(pc, valid, depth, R, dataset, tol_abs=0.05, tol_rel=0.02, radius=1):
    """Visibility of every directed pair of M posed views: pc [M,P,3] f64, valid [M,P] u8, depth [M,h,4h] f32 CUDA tensors, R [M,4,4] host
    float64 world -> camera poses (overlap_matrix_dev's convention; T_ij = R_j inv(R_i) moves cloud i into view j's frame).
    -> (counts [M,M,6] i32, margin_sum [M,M] i64, scores: visibility_scores per directed pair, [M,M] each) from ONE relpose_visibility call
    with M (M - 1) queries.  The diagonal is not computed: its counts are 0 and its scores NaN."""
    import torch
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(-1, 4, 4)
    M = R.shape[0]
    if pc.shape[0] != M or depth.shape[0] != M:
        raise ValueError("visibility_matrix_dev takes one pose and one panorama per cloud")
    dev = pc.device
    inv = [np.linalg.inv(R[i]) for i in range(M)]
    ij = [(i, j) for i in range(M) for j in range(M) if i != j]
    counts = torch.zeros(M, M, 6, dtype=torch.int32, device=dev)
    margin = torch.zeros(M, M, dtype=torch.int64, device=dev)
    if ij:
        poses = np.stack([np.matmul(R[j], inv[i]) for i, j in ij])
        qi = torch.tensor([i for i, _ in ij], device=dev)
        qj = torch.tensor([j for _, j in ij], device=dev)
        cn, mg = visibility_dev(pc, valid, depth, [i for i, _ in ij], [j for _, j in ij], torch.from_numpy(poses).to(dev), dataset,
                                tol_abs, tol_rel, radius)
        counts[qi, qj] = cn
        margin[qi, qj] = mg
    return counts, margin, visibility_scores(counts, margin)


def _tsdf_host_geometry(origin, dims, S):
    origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1, 3)
    if origin.shape[0] != S or len(dims) != 3:
        raise ValueError("one origin (x, y, z) per scene and dims = (nx, ny, nz)")
    return origin, tuple(int(v) for v in dims)


def tsdf_fuse_dev(depth, rgb, R, view_begin, origin, dims, voxel, dataset, trunc=None, state=None):
    """relpose_tsdf_fuse (include/relpose.h): integrate posed depth panoramas into one TSDF volume per scene.  depth
    [V,h,4h] f32 and rgb [V,3,h,4h] f32 (or None) CUDA tensors; R [V,4,4] float64 world -> camera poses (host array or CUDA tensor: the
    loaders' R); view_begin: S + 1 ascending view offsets (read on the host; scene s owns the views view_begin[s] .. view_begin[s+1]-1, at
    most 4096 per call); origin [S,3] and dims = (nx, ny, nz) on the host: the corner of voxel (0, 0, 0) and the voxel counts, shared by all
    scenes, like voxel and trunc (default 4 voxel).
    -> the state {"tsdf_sum" i32 [S,nz,ny,nx], "weight" i32, "color_sum" i32 [S,3,nz,ny,nx] or None, "origin", "dims", "voxel", "trunc",
    "dataset"}.  state=None allocates and stores; a given state (of the same geometry) is added to -- the volume does not depend on how the
    views are split over calls, nor on their order.  The caller keeps a voxel's weight <= 65535.  The call waits for the stream once."""
    import torch
    _lib.require_gpu()
    if depth.dim() != 3 or depth.shape[2] != 4 * depth.shape[1] or depth.dtype != torch.float32:
        raise ValueError("tsdf_fuse_dev takes depth [V,h,4h] float32")
    V, h = int(depth.shape[0]), int(depth.shape[1])
    dev = depth.device
    if rgb is not None and (tuple(rgb.shape) != (V, 3, h, 4 * h) or rgb.dtype != torch.float32 or rgb.device != dev):
        raise ValueError("tsdf_fuse_dev takes rgb [V,3,h,4h] float32 on depth's device")
    vb = np.ascontiguousarray(view_begin.cpu().numpy() if hasattr(view_begin, "cpu") else view_begin, dtype=np.int32).reshape(-1)
    S = len(vb) - 1
    if S < 1:
        raise ValueError("tsdf_fuse_dev takes view_begin [S + 1] with S >= 1")
    origin, dims = _tsdf_host_geometry(origin, dims, S)
    voxel = float(voxel)
    trunc = 4.0 * voxel if trunc is None else float(trunc)
    pose = R if hasattr(R, "data_ptr") else torch.from_numpy(np.ascontiguousarray(R, dtype=np.float64).reshape(-1, 4, 4)).to(dev)
    if tuple(pose.shape) != (V, 4, 4) or pose.dtype != torch.float64 or pose.device != dev:
        raise ValueError("tsdf_fuse_dev takes one float64 4x4 pose per view")
    nx, ny, nz = dims
    if state is None:
        state = {"tsdf_sum": torch.empty(S, nz, ny, nx, dtype=torch.int32, device=dev), "weight": torch.empty(S, nz, ny, nx, dtype=torch.int32, device=dev),
                 "color_sum": None if rgb is None else torch.empty(S, 3, nz, ny, nx, dtype=torch.int32, device=dev),
                 "origin": origin.copy(), "dims": dims, "voxel": voxel, "trunc": trunc, "dataset": dataset}
        accumulate = 0
    else:
        if (tuple(state["tsdf_sum"].shape) != (S, nz, ny, nx) or state["dims"] != dims or state["voxel"] != voxel or state["trunc"] != trunc
                or not np.array_equal(state["origin"], origin) or (state["color_sum"] is None) != (rgb is None)
                or dataset_id(state["dataset"]) != dataset_id(dataset)):
            raise ValueError("tsdf_fuse_dev: the state was built with another geometry, truncation, dataset or without / with colours")
        accumulate = 1
    if V == 0:
        if not accumulate:
            for k in ("tsdf_sum", "weight", "color_sum"):
                if state[k] is not None:
                    state[k].zero_()
        return state
    L = _lib.lib()
    nbytes = L.relpose_tsdf_fuse_workspace_bytes(S, V, h, nx, ny, nz)
    if nbytes == 0:
        raise ValueError("tsdf_fuse_dev: sizes outside relpose_tsdf_fuse's limits")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dc, rc, pc_ = depth.contiguous(), (None if rgb is None else rgb.contiguous()), pose.contiguous()
    a = _lib.TsdfFuseArgs()
    a.struct_size = _lib.C.sizeof(_lib.TsdfFuseArgs)
    a.n_scenes, a.n_views, a.h, a.dataset = S, V, h, dataset_id(dataset)
    a.nx, a.ny, a.nz, a.accumulate = nx, ny, nz, accumulate
    a.depth, a.rgb, a.pose = dc.data_ptr(), (0 if rc is None else rc.data_ptr()), pc_.data_ptr()
    a.view_begin_host, a.origin_host = vb.ctypes.data, origin.ctypes.data
    a.voxel, a.trunc = voxel, trunc
    a.tsdf_sum, a.weight = state["tsdf_sum"].data_ptr(), state["weight"].data_ptr()
    a.color_sum = 0 if rgb is None else state["color_sum"].data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.stream = _lib.stream_ptr()
    rc_ = L.relpose_tsdf_fuse(_lib.C.byref(a))
    if rc_ == -1:
        raise ValueError("relpose_tsdf_fuse: invalid arguments (view_begin not ascending from 0 to V, more than 4096 views in a scene, h odd, "
                         "a non-finite origin, voxel or trunc not > 0, or sizes outside the limits)")
    _lib.check(rc_, "relpose_tsdf_fuse")
    return state


def tsdf_surface_dev(state, min_weight=1, max_points=None):
    """relpose_tsdf_surface: the zero crossings of tsdf_fuse_dev's state as an oriented, coloured point cloud per scene.
    -> (points [S,cap,3] f64, normals [S,cap,3] f64, colors [S,cap,3] f32 or None, valid [S,cap] u8, n_points [S] i32) CUDA tensors in
    overlap_dev's pc / valid layout; cap = max_points.  n_points counts every crossing and may exceed cap: only the first cap, in ascending
    voxel order, are written; rows at and beyond n_points are zero with valid 0.  max_points=None sizes cap to the largest scene with a
    counting call first (cap at least 1).  The normals point towards the space the sensors saw through."""
    import torch
    _lib.require_gpu()
    ts, wt, cs = state["tsdf_sum"], state["weight"], state["color_sum"]
    S, nz, ny, nx = (int(v) for v in ts.shape)
    dev = ts.device
    origin = np.ascontiguousarray(state["origin"], dtype=np.float64).reshape(S, 3)
    L = _lib.lib()
    nbytes = L.relpose_tsdf_surface_workspace_bytes(S, nx, ny, nz)
    if nbytes == 0 or int(min_weight) < 1:
        raise ValueError("tsdf_surface_dev: sizes outside relpose_tsdf_surface's limits, or min_weight < 1")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tsc, wtc, csc = ts.contiguous(), wt.contiguous(), (None if cs is None else cs.contiguous())

    def call(cap, colours):
        points = torch.zeros(S, cap, 3, dtype=torch.float64, device=dev)
        normals = torch.zeros(S, cap, 3, dtype=torch.float64, device=dev)
        colors = torch.zeros(S, cap, 3, dtype=torch.float32, device=dev) if colours else None
        valid = torch.empty(S, cap, dtype=torch.uint8, device=dev)
        n_points = torch.empty(S, dtype=torch.int32, device=dev)
        a = _lib.TsdfSurfaceArgs()
        a.struct_size = _lib.C.sizeof(_lib.TsdfSurfaceArgs)
        a.n_scenes, a.nx, a.ny, a.nz, a.min_weight, a.cap = S, nx, ny, nz, int(min_weight), cap
        a.tsdf_sum, a.weight, a.color_sum = tsc.data_ptr(), wtc.data_ptr(), (0 if csc is None else csc.data_ptr())
        a.origin_host, a.voxel = origin.ctypes.data, float(state["voxel"])
        a.points, a.normals, a.colors = points.data_ptr(), normals.data_ptr(), (colors.data_ptr() if colours else 0)
        a.valid, a.n_points = valid.data_ptr(), n_points.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        a.stream = _lib.stream_ptr()
        rc_ = L.relpose_tsdf_surface(_lib.C.byref(a))
        if rc_ == -1:
            raise ValueError("relpose_tsdf_surface: invalid arguments (max_points < 1 or S max_points >= 2^29, or sizes outside the limits)")
        _lib.check(rc_, "relpose_tsdf_surface")
        return points, normals, colors, valid, n_points

    if max_points is None:
        max_points = max(1, int(call(1, False)[4].max().item()))
    return call(int(max_points), cs is not None)


def tsdf_mesh_dev(state, min_weight=1, max_points=None, max_triangles=None):
    """relpose_tsdf_mesh: tsdf_fuse_dev's state as one indexed triangle mesh per scene, marching cubes.
    -> {"points", "normals", "colors", "valid", "n_points": tsdf_surface_dev's five tensors, bit for bit, with cap = max_points,
    "triangles" [S,cap_tri,3] i32: indices into the scene's rows of points, "n_triangles" [S] i32} with cap_tri = max_triangles.  n_triangles
    counts every triangle and may exceed cap_tri: only the first cap_tri, in ascending cell order, are written; the rows beyond are zero.  A
    None cap is sized to the largest scene by a counting call first (at least 1).  A triangle may name any vertex of its scene, so a given
    max_points below a scene's n_points raises ValueError.  The winding faces the space the sensors saw through, as the normals do."""
    import torch
    _lib.require_gpu()
    ts, wt, cs = state["tsdf_sum"], state["weight"], state["color_sum"]
    S, nz, ny, nx = (int(v) for v in ts.shape)
    dev = ts.device
    origin = np.ascontiguousarray(state["origin"], dtype=np.float64).reshape(S, 3)
    L = _lib.lib()
    nbytes = L.relpose_tsdf_mesh_workspace_bytes(S, nx, ny, nz)
    if nbytes == 0 or int(min_weight) < 1:
        raise ValueError("tsdf_mesh_dev: sizes outside relpose_tsdf_mesh's limits, or min_weight < 1")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tsc, wtc, csc = ts.contiguous(), wt.contiguous(), (None if cs is None else cs.contiguous())

    def call(cap, cap_tri, colours):
        out = {"points": torch.zeros(S, cap, 3, dtype=torch.float64, device=dev), "normals": torch.zeros(S, cap, 3, dtype=torch.float64, device=dev),
               "colors": torch.zeros(S, cap, 3, dtype=torch.float32, device=dev) if colours else None,
               "valid": torch.empty(S, cap, dtype=torch.uint8, device=dev), "n_points": torch.empty(S, dtype=torch.int32, device=dev),
               "triangles": torch.zeros(S, cap_tri, 3, dtype=torch.int32, device=dev), "n_triangles": torch.empty(S, dtype=torch.int32, device=dev)}
        a = _lib.TsdfMeshArgs()
        a.struct_size = _lib.C.sizeof(_lib.TsdfMeshArgs)
        a.n_scenes, a.nx, a.ny, a.nz, a.min_weight, a.cap, a.cap_tri = S, nx, ny, nz, int(min_weight), cap, cap_tri
        a.tsdf_sum, a.weight, a.color_sum = tsc.data_ptr(), wtc.data_ptr(), (0 if csc is None else csc.data_ptr())
        a.origin_host, a.voxel = origin.ctypes.data, float(state["voxel"])
        a.points, a.normals, a.colors = out["points"].data_ptr(), out["normals"].data_ptr(), (out["colors"].data_ptr() if colours else 0)
        a.valid, a.n_points = out["valid"].data_ptr(), out["n_points"].data_ptr()
        a.triangles, a.n_triangles = out["triangles"].data_ptr(), out["n_triangles"].data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        a.stream = _lib.stream_ptr()
        rc_ = L.relpose_tsdf_mesh(_lib.C.byref(a))
        if rc_ == -1:
            raise ValueError("relpose_tsdf_mesh: invalid arguments (a cap < 1 or S cap >= 2^29, or sizes outside the limits)")
        _lib.check(rc_, "relpose_tsdf_mesh")
        return out

    if max_points is None or max_triangles is None:
        n = call(1, 1, False)
        max_points = max(1, int(n["n_points"].max().item())) if max_points is None else max_points
        max_triangles = max(1, int(n["n_triangles"].max().item())) if max_triangles is None else max_triangles
    out = call(int(max_points), int(max_triangles), cs is not None)
    if int(out["n_points"].max().item()) > int(max_points):
        raise ValueError(f"tsdf_mesh_dev: max_points = {int(max_points)} truncates a scene of {int(out['n_points'].max().item())} vertices; "
                         "its triangles would name vertices that were not written")
    return out


def _mesh_caps(mesh, what, truncated):
    """(S, cap, cap_tri) of a mesh dict; ValueError where a count exceeds its cap unless truncated"""
    import torch
    pts, tri = mesh["points"], mesh["triangles"]
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.dtype != torch.float64 or tri.dim() != 3 or tri.shape[2] != 3 or tri.dtype != torch.int32 or \
            tri.shape[0] != pts.shape[0]:
        raise ValueError(f"{what} takes points [S,cap,3] float64 and triangles [S,cap_tri,3] int32")
    S, cap, cap_tri = int(pts.shape[0]), int(pts.shape[1]), int(tri.shape[1])
    if not truncated and S and (int(mesh["n_points"].max().item()) > cap or int(mesh["n_triangles"].max().item()) > cap_tri):
        raise ValueError(f"{what}: a scene's n_points or n_triangles exceeds its capacity (a truncated mesh): pass truncated=True to label what was written")
    return S, cap, cap_tri


COMPONENT_KEYS = ("vertex_label", "tri_label", "n_components", "bad_triangles", "comp_root", "comp_vertices", "comp_triangles", "comp_area")


def mesh_components_dev(mesh, area_scale=None, max_components=None, max_rounds=1024, truncated=False):
    """relpose_mesh_components (include/relpose.h): the connected components of tsdf_mesh_dev's meshes (any dict with "points"
    [S,cap,3] f64, "n_points" [S] i32, "triangles" [S,cap_tri,3] i32, "n_triangles" [S] i32 on the GPU).  VERTEX connectivity: triangles that
    share a vertex index are one component; a component's id is its rank by smallest vertex index.
    -> {"vertex_label" [S,cap] i32 (-1: unused), "tri_label" [S,cap_tri] i32 (-1: bad or beyond the count), "n_components" [S] i32 (the true
    count), "bad_triangles" [S] i32, "comp_root", "comp_vertices", "comp_triangles" [S,cap_comp] i32, "comp_area" [S,cap_comp] i64, "rounds" int,
    "area_scale" float}.  cap_comp = max_components; None sizes it to the largest scene by a counting call first (at least 1).  comp_area is in
    units of 1 / area_scale; None = 2^20 / voxel^2 with the mesh's "voxel" (1.0 if it has none).  More than max_rounds propagation rounds
    raises RuntimeError.  A count above its capacity raises ValueError unless truncated=True."""
    import torch
    _lib.require_gpu()
    S, cap, cap_tri = _mesh_caps(mesh, "mesh_components_dev", truncated)
    if area_scale is None:
        area_scale = float(2 ** 20) / float(mesh.get("voxel", 1.0)) ** 2
    L = _lib.lib()
    nbytes = L.relpose_mesh_components_workspace_bytes(S, cap, cap_tri)
    if nbytes == 0:
        raise ValueError("mesh_components_dev: sizes outside relpose_mesh_components' limits")
    dev = mesh["points"].device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pts, tri = mesh["points"].contiguous(), mesh["triangles"].contiguous()
    npts, ntri = mesh["n_points"].contiguous(), mesh["n_triangles"].contiguous()

    def call(cap_comp):
        z = lambda n, dt: torch.zeros(S, n, dtype=dt, device=dev)
        out = {"vertex_label": z(cap, torch.int32), "tri_label": z(cap_tri, torch.int32),
               "n_components": torch.zeros(S, dtype=torch.int32, device=dev), "bad_triangles": torch.zeros(S, dtype=torch.int32, device=dev),
               "comp_root": z(cap_comp, torch.int32), "comp_vertices": z(cap_comp, torch.int32), "comp_triangles": z(cap_comp, torch.int32),
               "comp_area": z(cap_comp, torch.int64)}
        rounds = _lib.C.c_int(0)
        a = _lib.MeshComponentsArgs()
        a.struct_size = _lib.C.sizeof(_lib.MeshComponentsArgs)
        a.n_scenes, a.cap, a.cap_tri, a.cap_comp, a.max_rounds = S, cap, cap_tri, cap_comp, int(max_rounds)
        a.triangles, a.n_triangles, a.n_points, a.points = tri.data_ptr(), ntri.data_ptr(), npts.data_ptr(), pts.data_ptr()
        a.area_scale = float(area_scale)
        for k in COMPONENT_KEYS:
            setattr(a, k, out[k].data_ptr() if out[k].numel() else 0)
        a.rounds_host = _lib.C.addressof(rounds)
        a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
        rc_ = L.relpose_mesh_components(_lib.C.byref(a))
        if rc_ == -1:
            raise ValueError("relpose_mesh_components: invalid arguments (sizes outside the limits, area_scale not finite and > 0, or max_rounds < 1)")
        if rc_ == _lib.MESH_EROUNDS:
            raise RuntimeError(f"relpose_mesh_components: labels still moved after max_rounds = {int(max_rounds)} rounds")
        _lib.check(rc_, "relpose_mesh_components")
        out["rounds"] = int(rounds.value)
        out["area_scale"] = float(area_scale)
        return out

    if max_components is None:
        max_components = max(1, int(call(0)["n_components"].max().item()))
    return call(int(max_components))


def mesh_filter_dev(mesh, comps, keep, drop_unused=True, truncated=False):
    """relpose_mesh_filter (include/relpose.h): the mesh without the components whose keep [S,cap_comp] (bool or uint8, on the
    GPU) is 0, compacted in order; comps is mesh_components_dev's dict.  Unused vertices go too unless drop_unused=False.
    -> a mesh dict of tsdf_mesh_dev's keys with the same capacities (rows beyond the new counts are zero) plus "vertex_map" [S,cap] i32, old
    index -> new index or -1."""
    import torch
    _lib.require_gpu()
    S, cap, cap_tri = _mesh_caps(mesh, "mesh_filter_dev", truncated)
    dev = mesh["points"].device
    keep = keep.to(device=dev, dtype=torch.uint8).contiguous()
    if keep.dim() != 2 or keep.shape[0] != S:
        raise ValueError("mesh_filter_dev takes keep [S,cap_comp]")
    cap_comp = int(keep.shape[1])
    vl, tl = comps["vertex_label"].contiguous(), comps["tri_label"].contiguous()
    if tuple(vl.shape) != (S, cap) or tuple(tl.shape) != (S, cap_tri) or vl.dtype != torch.int32 or tl.dtype != torch.int32:
        raise ValueError("mesh_filter_dev: the labels are not this mesh's")
    L = _lib.lib()
    nbytes = L.relpose_mesh_filter_workspace_bytes(S, cap, cap_tri)
    if nbytes == 0:
        raise ValueError("mesh_filter_dev: sizes outside relpose_mesh_filter's limits")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    col = mesh.get("colors")
    src = {k: (None if mesh.get(k) is None else mesh[k].contiguous()) for k in ("points", "normals", "colors", "n_points", "triangles", "n_triangles")}
    out = {"points": torch.zeros(S, cap, 3, dtype=torch.float64, device=dev), "normals": torch.zeros(S, cap, 3, dtype=torch.float64, device=dev),
           "colors": None if col is None else torch.zeros(S, cap, 3, dtype=torch.float32, device=dev),
           "valid": torch.empty(S, cap, dtype=torch.uint8, device=dev), "n_points": torch.empty(S, dtype=torch.int32, device=dev),
           "triangles": torch.zeros(S, cap_tri, 3, dtype=torch.int32, device=dev), "n_triangles": torch.empty(S, dtype=torch.int32, device=dev),
           "vertex_map": torch.empty(S, cap, dtype=torch.int32, device=dev)}
    a = _lib.MeshFilterArgs()
    a.struct_size = _lib.C.sizeof(_lib.MeshFilterArgs)
    a.n_scenes, a.cap, a.cap_tri, a.cap_comp, a.drop_unused = S, cap, cap_tri, cap_comp, int(bool(drop_unused))
    for k, v in src.items():
        setattr(a, k, 0 if v is None else v.data_ptr())
    a.vertex_label, a.tri_label, a.keep = vl.data_ptr(), tl.data_ptr(), (keep.data_ptr() if cap_comp else 0)
    a.out_points, a.out_normals, a.out_colors = out["points"].data_ptr(), out["normals"].data_ptr(), (0 if col is None else out["colors"].data_ptr())
    a.out_valid, a.out_n_points = out["valid"].data_ptr(), out["n_points"].data_ptr()
    a.out_triangles, a.out_n_triangles, a.vertex_map = out["triangles"].data_ptr(), out["n_triangles"].data_ptr(), out["vertex_map"].data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    rc_ = L.relpose_mesh_filter(_lib.C.byref(a))
    if rc_ == -1:
        raise ValueError("relpose_mesh_filter: invalid arguments (sizes outside the limits)")
    _lib.check(rc_, "relpose_mesh_filter")
    return out                                                 # (the workspace is freed in stream order: the launches are only enqueued)


def mesh_keep_mask(comps, min_triangles=None, min_area=None, largest=None):
    """mesh_clean_dev's selection with torch operators on the device: keep [S,cap_comp] bool, the criteria ANDed over the components that
    exist.  min_triangles: comp_triangles >= it; min_area (in the mesh's length unit squared): comp_area >= min_area area_scale; largest = k:
    the k components with the most triangles, ties to the lower id."""
    import torch
    ct = comps["comp_triangles"]
    S, cap_comp = int(ct.shape[0]), int(ct.shape[1])
    ids = torch.arange(cap_comp, device=ct.device)[None]
    keep = ids < comps["n_components"][:, None]
    if min_triangles is not None:
        keep &= ct >= int(min_triangles)
    if min_area is not None:
        keep &= comps["comp_area"].to(torch.float64) >= float(min_area) * comps["area_scale"]
    if largest is not None:
        key = torch.where(keep, ct.to(torch.int64), torch.full_like(ct, -1, dtype=torch.int64))
        order = torch.argsort(key, dim=1, descending=True, stable=True)          # stable: ties stay in ascending id
        top = torch.zeros_like(keep)
        k = max(0, min(int(largest), cap_comp))
        top.scatter_(1, order[:, :k], True)
        keep &= top
    return keep


def mesh_clean_dev(mesh, min_triangles=None, min_area=None, largest=None, drop_unused=True, truncated=False, area_scale=None):
    """Drop a mesh's small connected components: mesh_components_dev, mesh_keep_mask, mesh_filter_dev.
    -> (clean_mesh, comps); comps describes the mesh as it came in and has "keep" [S,cap_comp] bool."""
    comps = mesh_components_dev(mesh, area_scale, truncated=truncated)
    comps["keep"] = mesh_keep_mask(comps, min_triangles, min_area, largest)
    return mesh_filter_dev(mesh, comps, comps["keep"], drop_unused, truncated), comps


DECIMATE_COUNTERS = ("bad_triangles", "outside_triangles", "degenerate_triangles", "duplicate_triangles")
DECIMATE_KEYS = ("points", "normals", "colors", "valid", "n_points", "count", "triangles", "n_triangles", "vertex_map", "tri_map") + DECIMATE_COUNTERS


def mesh_decimate_grid(mesh, cell):
    """mesh_decimate_dev's default grid, with torch operators on the device: -> (origin [S,3] float64 host array: the per-axis minimum of each
    scene's finite vertices (0 for a scene without one), dims (gx, gy, gz): the smallest grid of `cell` that covers the finite vertices of every
    scene).  It is the vertices' own box, NOT the volume's: see mesh_decimate_volume_dev for the grid aligned with the TSDF."""
    import torch
    pts = mesh["points"]
    S, cap = int(pts.shape[0]), int(pts.shape[1])
    live = torch.arange(cap, device=pts.device)[None] < mesh["n_points"].clamp(0, cap)[:, None]
    live = (live & torch.isfinite(pts).all(2))[:, :, None]
    lo = torch.where(live, pts, torch.full_like(pts, float("inf"))).amin(1)
    hi = torch.where(live, pts, torch.full_like(pts, float("-inf"))).amax(1)
    none = ~torch.isfinite(lo)
    lo, hi = torch.where(none, torch.zeros_like(lo), lo), torch.where(none, torch.zeros_like(hi), hi)
    dims = (torch.floor((hi - lo) / float(cell)).amax(0) + 1).clamp(max=float(2 ** 30))      # (max - origin) / cell rounds as the kernel's u
    return lo.cpu().numpy().astype(np.float64), tuple(int(v) for v in dims.tolist())


def mesh_decimate_dev(mesh, cell, origin=None, dims=None, dedupe=True, truncated=False):
    """relpose_mesh_decimate (include/relpose.h): tsdf_mesh_dev's / mesh_filter_dev's meshes (any dict with "points", "normals"
    [S,cap,3] f64, "colors" [S,cap,3] f32 or None, "n_points" [S] i32, "triangles" [S,cap_tri,3] i32, "n_triangles" [S] i32 on the GPU)
    decimated by vertex clustering: the vertices inside one cell of the grid (origin [S,3] host float64, dims (gx, gy, gz), edge `cell`) become
    one vertex with their mean position, normalised mean normal and mean colour; vertices outside the grid are dropped; triangles are
    remapped, the degenerate ones dropped and, with dedupe, of equal ones (up to rotation, not orientation) the lowest row kept.
    origin / dims None: mesh_decimate_grid's, the smallest grid over the finite vertices with the origin at their per-axis minimum -- these are
    NOT the volume's origin and dimensions, so the clusters are not aligned with the TSDF's voxels (mesh_decimate_volume_dev's are).
    -> a mesh dict of tsdf_mesh_dev's keys with the same capacities (rows beyond the new counts are zero) plus "vertex_map" [S,cap] i32 (old
    index -> new index or -1), "tri_map" [S,cap_tri] i32 (old row -> new row, or -1 bad, -2 outside, -3 degenerate, -4 duplicate, -5 beyond the
    count), "count" [S,cap] i32 (vertices per new vertex), the four counters "bad_triangles", "outside_triangles", "degenerate_triangles",
    "duplicate_triangles" [S] i32, and "decimate_origin", "decimate_dims", "decimate_cell".  Only enqueued on the current stream."""
    import torch
    _lib.require_gpu()
    S, cap, cap_tri = _mesh_caps(mesh, "mesh_decimate_dev", truncated)
    if not (np.isfinite(float(cell)) and float(cell) > 0.0):
        raise ValueError("mesh_decimate_dev: cell must be finite and > 0")
    if origin is None or dims is None:
        o, d = mesh_decimate_grid(mesh, cell)
        origin, dims = (o if origin is None else origin), (d if dims is None else dims)
    origin = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, dtype=np.float64).reshape(-1, 3), (S, 3)))
    gx, gy, gz = (int(v) for v in dims)
    L = _lib.lib()
    nbytes = L.relpose_mesh_decimate_workspace_bytes(S, cap, cap_tri, gx, gy, gz)
    if nbytes == 0:
        raise ValueError(f"mesh_decimate_dev: sizes outside relpose_mesh_decimate's limits (dims {gx} x {gy} x {gz}: each 1 .. 1024, "
                         "S gx gy gz < 2^27)")
    dev = mesh["points"].device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    col = mesh.get("colors")
    src = {k: (None if mesh.get(k) is None else mesh[k].contiguous()) for k in ("points", "normals", "colors", "n_points", "triangles", "n_triangles")}
    z = lambda dt, *shape: torch.zeros(*shape, dtype=dt, device=dev)
    out = {"points": z(torch.float64, S, cap, 3), "normals": z(torch.float64, S, cap, 3), "colors": None if col is None else z(torch.float32, S, cap, 3),
           "valid": z(torch.uint8, S, cap), "n_points": z(torch.int32, S), "count": z(torch.int32, S, cap), "triangles": z(torch.int32, S, cap_tri, 3),
           "n_triangles": z(torch.int32, S), "vertex_map": z(torch.int32, S, cap), "tri_map": z(torch.int32, S, cap_tri)}
    out.update({k: z(torch.int32, S) for k in DECIMATE_COUNTERS})
    a = _lib.MeshDecimateArgs()
    a.struct_size = _lib.C.sizeof(_lib.MeshDecimateArgs)
    a.n_scenes, a.cap, a.cap_tri, a.gx, a.gy, a.gz, a.dedupe = S, cap, cap_tri, gx, gy, gz, int(bool(dedupe))
    for k, v in src.items():
        setattr(a, k, 0 if v is None else v.data_ptr())
    a.origin_host, a.cell = origin.ctypes.data, float(cell)
    for k in ("points", "normals", "colors", "valid", "n_points", "count", "triangles", "n_triangles"):
        setattr(a, "out_" + k, 0 if out[k] is None else out[k].data_ptr())
    for k in ("vertex_map", "tri_map") + DECIMATE_COUNTERS:
        setattr(a, k, out[k].data_ptr())
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    rc_ = L.relpose_mesh_decimate(_lib.C.byref(a))
    if rc_ == -1:
        raise ValueError("relpose_mesh_decimate: invalid arguments (sizes outside the limits, or an origin that is not finite)")
    _lib.check(rc_, "relpose_mesh_decimate")
    out.update(decimate_origin=origin, decimate_dims=(gx, gy, gz), decimate_cell=float(cell))
    return out                                                 # (the workspace is freed in stream order: the launches are only enqueued)


def mesh_decimate_volume_dev(mesh, state, factor, dedupe=True, truncated=False):
    """mesh_decimate_dev on the grid of tsdf_fuse_dev's `state` coarsened by the integer `factor` >= 1: cell = factor * voxel, the volume's
    origin, dims = ceil(n / factor) per axis.  The cells are unions of factor^3 voxels of the TSDF, so a cluster never straddles a coarse
    voxel and meshes of volumes that share an origin decimate alike."""
    factor = int(factor)
    if factor < 1:
        raise ValueError("mesh_decimate_volume_dev takes an integer factor >= 1")
    _, nz, ny, nx = (int(v) for v in state["tsdf_sum"].shape)
    dims = tuple(-(-n // factor) for n in (nx, ny, nz))
    return mesh_decimate_dev(mesh, factor * float(state["voxel"]), state["origin"], dims, dedupe, truncated)


def tsdf_align_dev(state, depth, R, scene_of_view=None, iters=12, eig_min=None, stride=1, trace=False, min_weight=1):
    """relpose_tsdf_align (include/relpose.h): refine the world -> camera poses R [V,4,4] (float64 host array or CUDA tensor)
    of the depth panoramas depth [V,h,4h] f32 against tsdf_fuse_dev's state, so that each view's measured points lie on the zero level of the
    volume scene_of_view[v] names (None: every view against scene 0; read on the host).  iters Gauss-Newton steps (0 scores the poses as
    given); directions whose eigenvalue of JtJ / n_used is not above eig_min (None: _lib.TSDF_ALIGN_EIG_MIN) are held still; stride samples
    every stride-th pixel.
    -> {"pose" [V,4,4] f64, "eig" [V,6] f64 ascending, "held" [V] i32, "sums" [V,32] i64 (the last 4: outside, unknown, saturated, used),
    "rms" [V,2] f64 (first and last evaluation, in units of trunc)} CUDA tensors, and with trace=True "trace_pose" [V,iters+1,4,4] and
    "trace_sums" [V,iters+1,32].  The integer sums make the result bitwise independent of the batch.  The call waits for the stream once."""
    import torch
    _lib.require_gpu()
    if depth.dim() != 3 or depth.shape[2] != 4 * depth.shape[1] or depth.dtype != torch.float32:
        raise ValueError("tsdf_align_dev takes depth [V,h,4h] float32")
    V, h = int(depth.shape[0]), int(depth.shape[1])
    dev = depth.device
    ts, wt = state["tsdf_sum"], state["weight"]
    if ts.dim() != 4 or ts.shape != wt.shape or ts.dtype != torch.int32 or wt.dtype != torch.int32 or ts.device != dev or wt.device != dev:
        raise ValueError("tsdf_align_dev takes tsdf_fuse_dev's state on depth's device")
    S, nz, ny, nx = (int(v) for v in ts.shape)
    origin = np.ascontiguousarray(state["origin"], dtype=np.float64).reshape(S, 3)
    sov = np.zeros(V, np.int32) if scene_of_view is None else np.ascontiguousarray(
        scene_of_view.cpu().numpy() if hasattr(scene_of_view, "cpu") else scene_of_view, dtype=np.int32).reshape(-1)
    pose = R if hasattr(R, "data_ptr") else torch.from_numpy(np.ascontiguousarray(R, dtype=np.float64).reshape(-1, 4, 4)).to(dev)
    if tuple(pose.shape) != (V, 4, 4) or pose.dtype != torch.float64 or pose.device != dev or len(sov) != V:
        raise ValueError("tsdf_align_dev takes one float64 4x4 pose and one scene index per view")
    iters, stride = int(iters), int(stride)
    eig_min = _lib.TSDF_ALIGN_EIG_MIN if eig_min is None else float(eig_min)
    L = _lib.lib()
    nbytes = L.relpose_tsdf_align_workspace_bytes(S, V, h, nx, ny, nz, stride)
    if nbytes == 0 or not 0 <= iters <= 64:
        raise ValueError("tsdf_align_dev: sizes outside relpose_tsdf_align's limits (a dimension above 2048, more than 2^22 sampled pixels, "
                         "stride < 1, or iters outside 0..64)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = {"pose": torch.empty(V, 4, 4, dtype=torch.float64, device=dev), "eig": torch.empty(V, 6, dtype=torch.float64, device=dev),
           "held": torch.empty(V, dtype=torch.int32, device=dev), "sums": torch.empty(V, _lib.TSDF_ALIGN_SUMS, dtype=torch.int64, device=dev),
           "rms": torch.empty(V, 2, dtype=torch.float64, device=dev)}
    if trace:
        out["trace_pose"] = torch.empty(V, iters + 1, 4, 4, dtype=torch.float64, device=dev)
        out["trace_sums"] = torch.empty(V, iters + 1, _lib.TSDF_ALIGN_SUMS, dtype=torch.int64, device=dev)
    tsc, wtc, dc, pc_ = ts.contiguous(), wt.contiguous(), depth.contiguous(), pose.contiguous()
    a = _lib.TsdfAlignArgs()
    a.struct_size = _lib.C.sizeof(_lib.TsdfAlignArgs)
    a.n_scenes, a.n_views, a.h, a.dataset = S, V, h, dataset_id(state["dataset"])
    a.nx, a.ny, a.nz, a.min_weight, a.iters, a.stride = nx, ny, nz, int(min_weight), iters, stride
    a.tsdf_sum, a.weight, a.depth, a.pose = tsc.data_ptr(), wtc.data_ptr(), dc.data_ptr(), pc_.data_ptr()
    a.origin_host, a.scene_of_view_host = origin.ctypes.data, sov.ctypes.data
    a.voxel, a.eig_min = float(state["voxel"]), eig_min
    a.pose_out, a.eig, a.held, a.sums, a.rms = (out[k].data_ptr() for k in ("pose", "eig", "held", "sums", "rms"))
    a.trace_pose, a.trace_sums = (out["trace_pose"].data_ptr(), out["trace_sums"].data_ptr()) if trace else (0, 0)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.stream = _lib.stream_ptr()
    rc_ = L.relpose_tsdf_align(_lib.C.byref(a))
    if rc_ == -1:
        raise ValueError("relpose_tsdf_align: invalid arguments (a scene index outside 0..S-1, min_weight < 1, eig_min negative or not finite, "
                         "a non-finite origin, voxel not > 0, or sizes outside the limits)")
    _lib.check(rc_, "relpose_tsdf_align")
    return out


def tsdf_render_steps(dims, voxel, d_min=0.0, d_max=None, step=None):
    """tsdf_render_dev's host rule -> (step, n_steps): step defaults to half a voxel, d_max to the box diagonal; the samples d_min + k step
    reach up to d_max, at least one and at most _lib.TSDF_RENDER_MAX_STEPS."""
    voxel = float(voxel)
    step = 0.5 * voxel if step is None else float(step)
    if d_max is None:
        d_max = float(np.sqrt(sum((float(n) * voxel) ** 2 for n in dims)))
    if not (np.isfinite(step) and step > 0 and np.isfinite(d_max) and np.isfinite(d_min)):
        raise ValueError("tsdf_render_dev: d_min, d_max and step must be finite and step > 0")
    return step, int(min(max(np.floor((float(d_max) - float(d_min)) / step) + 1, 1), _lib.TSDF_RENDER_MAX_STEPS))


def tsdf_render_dev(state, R, dataset, h, scene_of_view=None, d_min=0.0, d_max=None, step=None, min_weight=1, skip=True, stages=False,
                    normal=True, color=True):
    """relpose_tsdf_render (include/relpose.h): what tsdf_fuse_dev's state looks like from the world -> camera poses R [V,4,4]
    (float64 host array or CUDA tensor): one [h,4h] panorama per view, marched through the volume scene_of_view[v] names (None: every view
    against scene 0; read on the host).  The samples lie at face depth d_min + k step, k < n_steps, up to d_max (tsdf_render_steps: step
    defaults to half a voxel, d_max to the box diagonal).  skip=True skips empty space brick by brick; it changes no output bit.
    -> (depth [V,h,4h] f32 with 0 = no data, normal [V,3,h,4h] f32 in the camera frame or None, color [V,3,h,4h] f32 or None (a state without
    colours, or color=False), cls [V,h,4h] u8: 0 miss, 1 hit, 2 back face) CUDA tensors, and with stages=True also n_evaluated [V,h,4h] i32,
    the samples each ray evaluated.  A view's image does not depend on the batch.  The call waits for the stream once."""
    import torch
    _lib.require_gpu()
    ts, wt, cs = state["tsdf_sum"], state["weight"], state.get("color_sum")
    dev = ts.device
    if ts.dim() != 4 or ts.shape != wt.shape or ts.dtype != torch.int32 or wt.dtype != torch.int32 or wt.device != dev:
        raise ValueError("tsdf_render_dev takes tsdf_fuse_dev's state")
    S, nz, ny, nx = (int(v) for v in ts.shape)
    if cs is not None and (tuple(cs.shape) != (S, 3, nz, ny, nx) or cs.dtype != torch.int32 or cs.device != dev):
        raise ValueError("tsdf_render_dev takes color_sum [S,3,nz,ny,nx] int32 on the state's device")
    origin = np.ascontiguousarray(state["origin"], dtype=np.float64).reshape(S, 3)
    pose = R if hasattr(R, "data_ptr") else torch.from_numpy(np.ascontiguousarray(R, dtype=np.float64).reshape(-1, 4, 4)).to(dev)
    V, h = int(pose.shape[0]), int(h)
    sov = np.zeros(V, np.int32) if scene_of_view is None else np.ascontiguousarray(
        scene_of_view.cpu().numpy() if hasattr(scene_of_view, "cpu") else scene_of_view, dtype=np.int32).reshape(-1)
    if pose.dim() != 3 or tuple(pose.shape[1:]) != (4, 4) or pose.dtype != torch.float64 or pose.device != dev or len(sov) != V:
        raise ValueError("tsdf_render_dev takes one float64 4x4 pose and one scene index per view")
    step, n_steps = tsdf_render_steps((nx, ny, nz), state["voxel"], d_min, d_max, step)
    L = _lib.lib()
    nbytes = L.relpose_tsdf_render_workspace_bytes(S, V, h, nx, ny, nz)
    if nbytes == 0:
        raise ValueError("tsdf_render_dev: sizes outside relpose_tsdf_render's limits (no view, h odd or above 8192, 2^31 pixels or voxels)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    colours = color and cs is not None
    depth = torch.empty(V, h, 4 * h, dtype=torch.float32, device=dev)
    cls = torch.empty(V, h, 4 * h, dtype=torch.uint8, device=dev)
    nrm = torch.empty(V, 3, h, 4 * h, dtype=torch.float32, device=dev) if normal else None
    col = torch.empty(V, 3, h, 4 * h, dtype=torch.float32, device=dev) if colours else None
    nev = torch.empty(V, h, 4 * h, dtype=torch.int32, device=dev) if stages else None
    tsc, wtc, csc, pc_ = ts.contiguous(), wt.contiguous(), (None if cs is None else cs.contiguous()), pose.contiguous()
    a = _lib.TsdfRenderArgs()
    a.struct_size = _lib.C.sizeof(_lib.TsdfRenderArgs)
    a.n_scenes, a.n_views, a.h, a.dataset = S, V, h, dataset_id(dataset)
    a.nx, a.ny, a.nz, a.min_weight, a.n_steps, a.skip = nx, ny, nz, int(min_weight), n_steps, int(bool(skip))
    a.tsdf_sum, a.weight, a.color_sum, a.pose = tsc.data_ptr(), wtc.data_ptr(), (0 if csc is None else csc.data_ptr()), pc_.data_ptr()
    a.origin_host, a.scene_of_view_host = origin.ctypes.data, sov.ctypes.data
    a.voxel, a.d_min, a.step = float(state["voxel"]), float(d_min), step
    a.depth, a.cls = depth.data_ptr(), cls.data_ptr()
    a.normal, a.color, a.n_evaluated = (0 if t is None else t.data_ptr() for t in (nrm, col, nev))
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.stream = _lib.stream_ptr()
    rc_ = L.relpose_tsdf_render(_lib.C.byref(a))
    if rc_ == -1:
        raise ValueError("relpose_tsdf_render: invalid arguments (a scene index outside 0..S-1, min_weight < 1, d_min negative, a non-finite "
                         "origin, voxel not > 0, or sizes outside the limits)")
    _lib.check(rc_, "relpose_tsdf_render")
    return (depth, nrm, col, cls, nev) if stages else (depth, nrm, col, cls)


def tsdf_bounds_dev(depth, R, dataset, voxel, pad=3, view_begin=None):
    """The box tsdf_fuse_dev should be given: per scene, around every pixel with data of its views unprojected (pano2pc_dev) and moved into the
    world frame by the inverse of its pose R [V,4,4] (host float64, world -> camera), widened by `pad` voxels on every side.
    view_begin=None: one scene of all views.  -> (origin [S,3] host float64, dims (nx, ny, nz): the maximum over the batch, so every scene
    gets the same volume shape).  A scene without a valid pixel gets the origin -pad voxel and one voxel plus the padding."""
    import torch
    V = int(depth.shape[0])
    vb = np.array([0, V]) if view_begin is None else np.asarray(view_begin.cpu().numpy() if hasattr(view_begin, "cpu") else view_begin).reshape(-1)
    S = len(vb) - 1
    voxel = float(voxel)
    origin = np.full((S, 3), -pad * voxel)
    dims = np.full(3, 1 + 2 * pad, np.int64)
    if V:
        # the skybox's own unprojection: the scannet branch of relpose_pano2pc scales x and y by the kinect intrinsics, which the projection
        # of relpose_tsdf_fuse (csrc/skybox.h) does not; matterport has scannet's face order.  pano2pc marks every suncg pixel valid, so
        # the validity is the fuse rule's: finite and > 0.
        pc, _ = pano2pc_dev(depth, "suncg" if dataset_id(dataset) == DATASETS["suncg"] else "matterport")      # [V,3,P] camera frame, face-major
        h = int(depth.shape[1])
        faces = depth.reshape(V, h, 4, h).permute(0, 2, 1, 3).reshape(V, 4 * h * h)
        valid = torch.isfinite(faces) & (faces > 0)
        Rh = np.ascontiguousarray(R.cpu().numpy() if hasattr(R, "cpu") else R, dtype=np.float64).reshape(V, 4, 4)
        inv = torch.from_numpy(np.stack([np.linalg.inv(Rh[v]) for v in range(V)])).to(depth.device)
        pw = torch.matmul(inv[:, :3, :3], pc) + inv[:, :3, 3:4]
        ok = valid.unsqueeze(1)
        big = torch.full_like(pw, float("inf"))
        lo = torch.where(ok, pw, big).amin(2).cpu().numpy()                                           # [V,3]
        hi = torch.where(ok, pw, -big).amax(2).cpu().numpy()
        for s in range(S):
            if vb[s + 1] > vb[s]:
                l, u = lo[vb[s]:vb[s + 1]].min(0), hi[vb[s]:vb[s + 1]].max(0)
                if np.isfinite(l).all() and np.isfinite(u).all():
                    origin[s] = l - pad * voxel
                    dims = np.maximum(dims, np.ceil((u - l) / voxel).astype(np.int64) + 2 * pad + 1)
    return origin, tuple(int(v) for v in dims)


def pose_sync_dev(T, src, dst, w0, view_begin, edge_begin, sigma_r=0.1, sigma_t=0.1, mu0=64.0, div=1.4, n_final=10, robust=True, device=None):
    """relpose_pose_sync (include/relpose.h): the relative poses of S scenes' view pairs -> one absolute pose per view and one
    confidence per relative pose.  T [E,4,4] f64 (T ~ R_dst inv(R_src) for world -> camera R: what the pair drivers produce), src / dst [E]
    view indices local to the scene, w0 [E] f64 prior weights: host arrays or CUDA tensors; view_begin / edge_begin: S + 1 ascending offsets
    (read on the host; at most 64 views and 4096 edges per scene).
    -> {"pose" [V,4,4] f64 in each component's gauge (its smallest view = identity), "component" [V] i32 (local), "tree", "edge_state" [E]
    i32, "confidence", "res_rot", "res_trans" [E] f64, "n_components" [S] i32, "cost", "last_step" [S] f64} CUDA tensors.  One launch; the
    call waits for the stream once."""
    import torch
    dev = device if device is not None else next((t.device for t in (T, src, dst, w0) if hasattr(t, "data_ptr") and t.is_cuda), None)
    dev = torch.device(dev) if dev is not None else _lib.require_gpu()
    _lib.require_gpu()

    def put(v, dt, npdt, tail):
        t = v if hasattr(v, "data_ptr") else torch.from_numpy(np.ascontiguousarray(v, dtype=npdt))
        return t.to(device=dev, dtype=dt).reshape((t.numel() // int(np.prod(tail, dtype=np.int64)),) + tail).contiguous()

    Td = put(T, torch.float64, np.float64, (4, 4))
    E = int(Td.shape[0])
    sd, dd, wd = put(src, torch.int32, np.int32, ()), put(dst, torch.int32, np.int32, ()), put(w0, torch.float64, np.float64, ())
    host = lambda v: np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v, dtype=np.int32).reshape(-1)
    vb, eb = host(view_begin), host(edge_begin)
    S = len(vb) - 1
    if S < 1 or len(eb) != S + 1 or sd.numel() != E or dd.numel() != E or wd.numel() != E:
        raise ValueError("pose_sync_dev takes view_begin and edge_begin [S + 1] with S >= 1 and one src, dst, T and w0 per edge")
    V = int(vb[-1])
    L = _lib.lib()
    nbytes = L.relpose_pose_sync_workspace(S, V, E)
    if nbytes == 0 or int(eb[-1]) != E:
        raise ValueError("pose_sync_dev: sizes outside relpose_pose_sync's limits (64 views and 4096 edges per scene), or edge_begin does not end at E")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    out = {"pose": f64(V, 4, 4), "component": i32(V), "tree": i32(E), "edge_state": i32(E), "confidence": f64(E), "res_rot": f64(E),
           "res_trans": f64(E), "n_components": i32(S), "cost": f64(S), "last_step": f64(S)}
    pad = f64(16)                                                  # an empty tensor has no address: the entry is never read or written
    addr = lambda t: t.data_ptr() if t.numel() else pad.data_ptr()
    a = _lib.PoseSyncArgs()
    a.struct_size = _lib.C.sizeof(_lib.PoseSyncArgs)
    a.n_scenes, a.n_views, a.n_edges, a.n_final, a.robust = S, V, E, int(n_final), int(bool(robust))
    a.view_begin_host, a.edge_begin_host = vb.ctypes.data, eb.ctypes.data
    a.src, a.dst, a.T, a.w0 = addr(sd), addr(dd), addr(Td), addr(wd)
    a.sigma_r, a.sigma_t, a.mu0, a.div = float(sigma_r), float(sigma_t), float(mu0), float(div)
    for k, t in out.items():
        setattr(a, k, addr(t))
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    with torch.cuda.device(dev):
        a.stream = _lib.stream_ptr()
        rc_ = L.relpose_pose_sync(_lib.C.byref(a))
    if rc_ == -1:
        raise ValueError("relpose_pose_sync: invalid arguments (offsets not ascending from 0, more than 64 views or 4096 edges in a scene, "
                         "sigma not > 0, div not > 1, mu0 < 1, n_final < 0, or more than 100000 iterations)")
    _lib.check(rc_, "relpose_pose_sync")
    return out


def pose_graph(pairs, poses, weights=None):
    """The edge arrays of ONE scene for pose_sync_dev (host code).  pairs: [(src, dst)] view indices, one per estimated pair -- or a list of
    records (dicts with "src", "dst", "pose" or "poses", and optionally "vis_agreement"), in which case `poses` is None.  poses: per pair one
    4x4 pose T ~ R_dst inv(R_src) or several [K,4,4] (the levels of a recurrence, or several methods' estimates): every pose becomes an edge
    of its own, so competing hypotheses for a pair meet in the graph.  weights: per pair a scalar or one value per pose; default the
    record's "vis_agreement" where present and finite and > 0, otherwise 1.
    -> (src [E] i32, dst [E] i32, T [E,4,4] f64, w0 [E] f64, pair [E] i32: the index of the edge's pair)."""
    if poses is None:
        recs = list(pairs)
        pairs = [(int(r["src"]), int(r["dst"])) for r in recs]
        poses = [r["poses"] if "poses" in r else r["pose"] for r in recs]
        if weights is None:
            weights = [r.get("vis_agreement", 1.0) for r in recs]
    if len(poses) != len(pairs) or (weights is not None and len(weights) != len(pairs)):
        raise ValueError("pose_graph takes one pose (or stack of poses) and one weight per pair")
    src, dst, T, w0, pair = [], [], [], [], []
    for k, (i, j) in enumerate(pairs):
        P = np.asarray(poses[k], dtype=np.float64).reshape(-1, 4, 4)
        w = np.ones(len(P)) if weights is None or weights[k] is None else np.broadcast_to(np.asarray(weights[k], dtype=np.float64), (len(P),))
        for n in range(len(P)):
            src.append(int(i)); dst.append(int(j)); T.append(P[n]); pair.append(k)
            w0.append(float(w[n]) if np.isfinite(w[n]) and w[n] > 0 else 1.0)
    return (np.array(src, np.int32).reshape(-1), np.array(dst, np.int32).reshape(-1), np.array(T, np.float64).reshape(-1, 4, 4),
            np.array(w0, np.float64).reshape(-1), np.array(pair, np.int32).reshape(-1))


def save_ply(path, points, normals=None, colors=None, faces=None):
    """Write a binary little-endian PLY point cloud: points [N,3] (float32 x y z in the file), normals [N,3] (nx ny nz) and colors [N,3] in
    [0, 1] (uchar red green blue) if given; arrays or tensors.  faces [F,3] (integer indices into points): a mesh, `element face` with
    `property list uchar int vertex_indices`.  Returns N."""
    host = lambda v: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    p = host(points).reshape(-1, 3)
    N = p.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {N}", "property float x", "property float y", "property float z"]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.zeros(N, dtype=np.dtype(fields))
    for a, k in enumerate("xyz"):
        rec[k] = p[:, a]
    if normals is not None:
        n = host(normals).reshape(-1, 3)
        if n.shape[0] != N:
            raise ValueError("save_ply: one normal per point")
        for a, k in enumerate(("nx", "ny", "nz")):
            rec[k] = n[:, a]
    if colors is not None:
        c = host(colors).reshape(-1, 3)
        if c.shape[0] != N:
            raise ValueError("save_ply: one colour per point")
        q = np.rint(np.clip(np.nan_to_num(c.astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        for a, k in enumerate(("red", "green", "blue")):
            rec[k] = q[:, a]
    tail = b""
    if faces is not None:
        t = host(faces).reshape(-1, 3)
        if t.size and (t.min() < 0 or t.max() >= N):
            raise ValueError("save_ply: a face names a vertex that is not there")
        header += [f"element face {t.shape[0]}", "property list uchar int vertex_indices"]
        frec = np.zeros(t.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        frec["n"], frec["v"] = 3, t
        tail = frec.tobytes()
    with open(path, "wb") as f:
        f.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        f.write(tail)
    return N


def depth2pc(depth, dataList):
    """util.py:468: depth numpy = one h x h face (suncg / matterport) or the 66x88 kinect crop (scannet)
    -> (pc [k,3] of the non-zero depths, mask)."""
    import torch
    dev = _lib.require_gpu()
    ds = dataset_id(dataList)
    hh, ww = depth.shape
    if ds == 2 and (hh, ww) == (480, 640):                # the full-resolution kinect image (util.py:497-507: the baselines' clouds)
        dd = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)[None]).to(dev)
        pc = torch.empty(1, hh * ww, 3, dtype=torch.float64, device=dev)
        valid = torch.empty(1, hh * ww, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().relpose_depth2pc_full(_lib.ptr(dd), _lib.ptr(pc), _lib.ptr(valid), 1, hh, ww, _lib.stream_ptr()), "relpose_depth2pc_full")
        m = valid[0].cpu().numpy().astype(bool)
        return pc[0].cpu().numpy()[m], m
    h = 160 if ds == 2 else hh
    pano = np.zeros((1, h, 4 * h), np.float32)
    if ds == 2:
        assert (hh, ww) == (66, 88), "scannet: the 66x88 crop or the 480x640 image (the reference defines no other shape, util.py:498,508)"
        pano[0, 47:113, 196:284] = depth
    else:
        pano[0, :, h:2 * h] = depth
    pc, valid = depth2pc_dev(torch.from_numpy(pano).to(dev), dataList)
    m = valid[0].cpu().numpy().astype(bool)
    return pc[0].cpu().numpy()[m], m


def parse_data(depth, rgb, norm, dataList, method):
    """util.py:42-92, same signature and 8-tuple: both scans as point clouds (+ colours, normals).  suncg / matterport: the observed face
    [160,320) of depth [1,2,160,640], rgb uint8 [1,2,3,160,640], norm [1,2,3,160,640].  scannet with an 'ours' method: the 66x88 kinect crop
    of the same panoramas, normals renormalised (:56-76); scannet with a baseline method (:78-90): depth [1,2,480,640], rgb [1,2,3,480,640] are
    the full-resolution kinect IMAGES, back-projected whole, and there are no normals (None, None)."""
    full = False
    if 'suncg' in dataList or 'matterport' in dataList:
        ys, xs = slice(None), slice(160, 320)
    elif 'scannet' in dataList:
        if 'ours' in method:
            ys, xs = slice(80 - 33, 80 + 33), slice(160 + 80 - 44, 160 + 80 + 44)
        else:
            ys, xs, full = slice(None), slice(None), True
    else:
        raise ValueError(f"unknown dataset {dataList}")
    out = {}
    for v, tag in ((0, "src"), (1, "tgt")):
        d = depth[0, v, ys, xs]
        col = rgb[0, v, :, ys, xs].transpose(1, 2, 0)
        pc, mask = depth2pc(d, dataList)
        col = col.reshape(-1, 3)[mask] / 255.
        nrm = None
        if not full:
            nrm = norm[0, v, :, ys, xs].copy().transpose(1, 2, 0).reshape(-1, 3)[mask]
            if 'scannet' in dataList:
                with np.errstate(divide="ignore", invalid="ignore"):
                    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
                nrm[np.isnan(nrm.sum(1))] = 0
        out[tag] = (d, nrm, col, pc)
    s, t = out["src"], out["tgt"]
    return s[0], t[0], s[1], t[1], s[2], t[2], s[3], t[3]


def angular_distance_np(R_hat, R):
    """util.py:176-187 (lives in relativepose_amd.evaluation; re-exported under the reference's module name)."""
    from .evaluation import angular_distance_np as f
    return f(R_hat, R)
