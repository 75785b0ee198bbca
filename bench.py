#!/usr/bin/env python
"""Benchmark of the relative-pose hot path on MI355X.

Metric (BASELINE.json): scan-pairs/sec end-to-end (completion + feat +
spectral-match), 160x640 RGB-D.  One "step" = one pass of the whole hot path
(3 recurrent levels of {warp, SCNet, compose+sample, match}) over one batch of
synthetic scan pairs already resident in HBM.  Default workload = BASELINE.json
configs[1] per GPU: SUNCG conventions, 160x640, 200 keypoints per view, 32 pairs
per GPU, fp32.  ``--config 2|3|4`` select the other single-GPU-runnable BASELINE
configurations (Matterport N=400; ScanNet/kinect 32 pairs per GPU = 256 over 8;
SUNCG 320x1280 with the fp16-MFMA conv path).  Pairs shard across ranks with no
data-path collective and one RCCL all_gather of the 4x4 poses per step
(``--scaling weak``: pairs per GPU fixed; ``--scaling strong``: ``--total-pairs``
fixed).  Three steps are in flight (--inflight 3) over 6 rotating prepared batches:
the launch-bound matcher phase of step k runs under the SCNet forwards of steps k+1, k+2
(round 5: a third slot is free on configs[1] / [3] and worth +2 % / +7 % on configs[2] / [4],
whose tail -> matcher -> warp -> head chain is longer than one forward).

    python bench.py                                   # 1 GPU, configs[1]
    python bench.py --gpus 8                          # spawns 8 ranks itself (one per GPU, RCCL)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W
    python bench.py --steps K --dump-outputs DIR      # + the last timed step's poses / status as DIR/*.npy (seeded inputs: comparable across builds)

Rank 0 prints ONE JSON line (contract in the task statement) with extra objects:
"roofline" (dominant kernel = the MFMA implicit-GEMM conv, live HIP-event timing),
"roofline_affinity" (the N x N affinity build against HBM peak), "roofline_geometry"
(unprojection / warp / keypoint sampling against HBM peak), "pcie_inclusive"
(the same loop with every step's inputs uploaded from pinned host memory) and
"cpu_baseline" (the numpy/torch oracle on the host cores, bounded sample, N=1 only).
"""
import argparse
import json
import os
import socket
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GFLOP_PER_IMAGE = 36.14            # SCNet conv+convT MACs x2 per 224x224 sample
PEAK_F32_MFMA_TFLOPS = 157.3       # MI355X dense fp32 matrix peak (MI355X_MICROARCH.md)
PEAK_F16_MFMA_TFLOPS = 2500.0      # dense fp16 / bf16
MFMA_TERMS = {"bf16x3": 3, "f16x3": 3, "bf16x9": 9, "bf16x6": 6}      # 16-bit MFMA products issued per fp32 product
DTYPE_EXACT = {
    "bf16x9": "f32 (fp32 products emulated on the bf16 matrix pipe: every operand cut into 3 bf16 pieces = its full 24 significand bits, all 9 partial products "
              "issued as v_mfma_f32_32x32x16_bf16, each exact in the fp32 accumulator; fp32 accumulation / activations / BatchNorm statistics / conv1 / heads)",
    "bf16x6": "f32 (fp32 products emulated on the bf16 matrix pipe: every operand cut into 3 bf16 pieces = its full 24 significand bits, the 6 partial products "
              ">= 2^-16 |ab| issued as v_mfma_f32_32x32x16_bf16, the 3 smallest dropped: a product error <= 2^-23 |ab| worst case, rms 2^-27.4 -- an fp32 multiply's own "
              "rounding is <= 2^-24 |ab|, rms 2^-25.2; fp32 accumulation / activations / BatchNorm statistics / conv1 / heads; --precision f32 = the fp32 MFMA kernels)",
}
PEAK_HBM_GBS = 8000.0

# BASELINE.json configs[i] -> concrete single-GPU workload
CONFIGS = {
    # conv arithmetic of configs 1-3 (round 6): "bf16x6" -- fp32 products emulated on the bf16 matrix pipe with every operand at its full 24 bits
    # (DTYPE_EXACT; each product within one fp32 rounding of exact -- rms a quarter of an fp32 multiply's own rounding --, fp32 accumulation); --precision f32 runs the fp32 MFMA
    # kernels of rounds 1-5, --precision bf16x9 the all-nine-terms form (exact products).  Parity of all three: tests/test_gpu_scnet.py, test_gpu_e2e.py.
    # configs[0]: the reference's own CPU-runnable plumbing case -- `evaluation.py --method=ours` on 4 SUNCG pairs (160x640, rgbdnsf); here the 4 pairs
    # and N = 80 keypoints of the e2e fixtures (tests/golden/e2e.npz pins exactly this workload to the reference).  A latency-shaped line (one
    # 4-pair batch per step does not fill the chip); the headline is configs[1].
    0: dict(dataset="suncg", mask="second", h=160, N=80, S=15, tanh=1, pairs=4, precision="bf16x6", cpu_pairs=4,
            label="evaluation.py --method=ours on 4 SUNCG pairs, 160x640 rgbdnsf, N=80 keypoints, alterStep=3 (BASELINE configs[0]: the reference's CPU-runnable case)",
            parity_note="tests/golden/e2e.npz: these 4 pairs x 3 levels captured from the reference (tests/test_gpu_e2e.py, test_gpu_pipeline.py)"),
    1: dict(dataset="suncg", mask="second", h=160, N=200, S=15, tanh=1, pairs=32, precision="bf16x6", cpu_pairs=9,
            label="SUNCG 160x640, N=200 keypoints, batch=32 pairs per GPU, alterStep=3 (BASELINE configs[1])"),
    2: dict(dataset="matterport", mask="second", h=160, N=400, S=21, tanh=1, pairs=32, precision="bf16x6", cpu_pairs=3,
            label="Matterport 160x640, N=400 keypoints (160k-entry affinity), batch=32 pairs per GPU, alterStep=3 (BASELINE configs[2])"),
    3: dict(dataset="scannet", mask="kinect", h=160, N=200, S=21, tanh=1, pairs=32, precision="bf16x6", cpu_pairs=6,
            label="ScanNet (kinect crop) 160x640, N=200 keypoints, 32 pairs per GPU (= batch 256 over 8 GPUs), alterStep=3 (BASELINE configs[3])"),
    4: dict(dataset="suncg", mask="second", h=320, N=200, S=15, tanh=1, pairs=32, precision="f16x3", cpu_pairs=3,
            label="SUNCG 320x1280 high-res pano, fp16 MFMA conv path (f16x3), N=200 keypoints, 32 pairs per GPU, alterStep=3 (BASELINE configs[4])",
            parity_note="h=320 is checked against the parameterised oracle only (tests/test_gpu_pipeline.py): the reference asserts 160x640 panoramas, so no "
                        "reference golden exists at this size -- parity unpinned for this configuration"),
}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)     # (a hand-run times > 2 s; the driver passes its own)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", type=int, default=1, choices=sorted(CONFIGS), help="BASELINE.json configs[] index")
    ap.add_argument("--pairs", type=int, default=None, help="scan pairs per GPU (default: the config's)")
    ap.add_argument("--keypoints", type=int, default=None)
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--total-pairs", type=int, default=256, help="--scaling strong: pairs per step over all GPUs (configs[3]: 256)")
    ap.add_argument("--gather", choices=["run", "step"], default="run",
                    help="multi-GPU: one all_gather of every step's poses at the end of the run (default) or one per step")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-h2d", action="store_true", help="skip the PCIe-inclusive measurement")
    ap.add_argument("--h2d-mode", choices=["auto", "slot", "lookahead"], default="auto",
                    help="PCIe-inclusive run: uploads on the batch's slot stream, or on a copy stream one in-flight depth ahead (auto: lookahead whenever >= 2 x inflight batches rotate)")
    ap.add_argument("--no-aux", action="store_true", help="skip the roofline / affinity side measurements (profiling runs)")
    ap.add_argument("--precision", choices=["f32", "bf16x3", "f16x3", "f16", "bf16x9", "bf16x6"], default=None,
                    help="conv arithmetic (default: the config's -- bf16x6 for configs 1-3, f16x3 for configs[4]; f32 = the fp32 MFMA kernels, bf16x9 = all nine partial products)")
    ap.add_argument("--pose-outputs", action="store_true",
                    help="opt-in: SCNet computes only the heads the pose loop reads (normal, depth, features; RELPOSE_FWD_POSE_OUTPUTS) -- "
                         "same poses, no completed rgb / semantic maps; NOT the BASELINE metric (the default computes every output)")
    ap.add_argument("--no-self-cache", action="store_true",
                    help="levels 1-2 recompute the self-view encoder streams (A/B switch; the default reuses level 0's, bitwise the same poses)")
    ap.add_argument("--no-tail-overlap", action="store_true", help="A/B: the whole SCNet forward on the SCNet stream (no head / tail on the slot streams)")
    ap.add_argument("--net-priority", type=int, default=None, help="A/B: HIP stream priority of the SCNet stream (default: -1 = high when the tail overlaps)")
    ap.add_argument("--fit-cluster", type=int, default=1, help="A/B: workgroups per scan pair in the fit inside the loop (default 1: no helper workgroups)")
    ap.add_argument("--inflight", type=int, default=3,
                    help="batches (steps) in flight per GPU: the matcher phase of step k overlaps the SCNet forward of step k+1")
    ap.add_argument("--batches", type=int, default=6, help="distinct prepared batches rotated through the in-flight slots")
    ap.add_argument("--h2d-inflight", type=int, default=2,
                    help="batches in flight during the PCIe-inclusive run (0 = --inflight): with the copy stream beside them two in flight measured better than "
                         "three (configs[4]: 937 vs 769-876 pairs/s PCIe-inclusive), while three are better with resident inputs")
    ap.add_argument("--hw-queues", type=int, default=0,
                    help="A/B: GPU_MAX_HW_QUEUES for this process (the HIP runtime multiplexes streams onto 4 hardware queues by default); 0 = leave the environment alone")
    ap.add_argument("--keypoint-mode", choices=["given", "reference"], default="given",
                    help="given (default, the BASELINE workload: one injected keypoint set per view for all levels, SURVEY 8d) | reference: every "
                         "level derives its keypoints from its own feature maps like rputil.getKeypoint (synthetic SIFT detections given once; "
                         "descriptor gather + fused distance-map / NMS + random fill on the device INSIDE the timed region) -- reported beside the headline")
    ap.add_argument("--sift", type=int, default=120, help="--keypoint-mode reference: synthetic SIFT detections per view (+ <= 60 / <= 90 derived ones)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (pose.npy [pairs,4,4] float64, status.npy [pairs] float64; "
                         "all pairs of the job, rank 0) to DIR.  The inputs are seeded, so two builds run with the same arguments can be compared "
                         "output for output; the last step runs prepared batch (steps - 1) %% batches, so the dump depends on --steps")
    return ap.parse_args(argv)


def dump_outputs(path, poses, status):
    """The arrays the timed path hands its caller for the last timed step, as float64 .npy files (136 bytes per pair)."""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "pose.npy"), poses.detach().cpu().numpy().astype(np.float64))
    np.save(os.path.join(path, "status.npy"), status.detach().cpu().numpy().astype(np.float64))


def cpu_baseline(cfg, N, data, pts, ptw, sigmas):
    """The oracle (CPU restatement of the reference loop) on the first pairs of the same workload (checker timed beside
    the GPU path; never the product)."""
    import torch
    from oracle import pipeline_oracle as P
    from oracle.scnet_oracle import SCNetOracle
    from relativepose_amd import weights
    S = cfg["S"]
    net = SCNetOracle(weights.make_state_dict(7, S), S, cfg["tanh"])
    # bounded sample: 3 repetitions of npair / 3 DIFFERENT pairs each (~30-40 s of host time in all at configs[1]); value = the median
    # repetition
    tm, npair = {}, min(cfg["cpu_pairs"], len(pts))
    reps = 3 if npair >= 3 else 1
    per = npair // reps
    npair = per * reps
    rates, t_all = [], time.time()
    for r in range(reps):
        t0 = time.time()
        for i in range(r * per, (r + 1) * per):
            tmi = {}
            P.run_pair(net, data["rgb"][i], data["norm"][i], data["depth"][i], pts[i], ptw[i], np.array(sigmas), cfg["dataset"], cfg["mask"], S,
                       timing=tmi)
            for k, v in tmi.items():
                tm[k] = tm.get(k, 0.0) + v / npair
        rates.append(per / (time.time() - t0))
    dt = time.time() - t_all
    return {"value": float(np.median(rates)), "unit": "pairs/s", "cores": int(torch.get_num_threads()), "kind": "port",
            "sample": f"{npair} scan pairs x 3 recurrent levels of the same workload (N={N} keypoints) as {reps} repetitions of {per} different "
                      f"pairs, value = median repetition; oracle = numpy/scipy matcher + torch-CPU fp32 SCNet; {dt:.1f}s in all",
            "repetitions_pairs_per_s": [round(x, 4) for x in rates],
            "seconds_per_stage": {k: round(v, 3) for k, v in tm.items()}}


def _traffic(tag):
    """HBM bytes per forward of the conv stack from a KEPT rocprofv3 PMC profile of this configuration
    (profiles/traffic.json: {tag: {"bytes": ..., "profile": "profiles/<file>"}}), else None."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            return json.load(f).get(tag)
    except OSError:
        return None


def affinity_roofline(N, B, dev, sigmas, want_wij=True):
    """N x N affinity build (materialised fp32 wij), the kernel the HBM target is stated on: HIP-event time of `reps`
    back-to-back launches (no host gaps) at batch B.  want_wij=False: the fused variant the matcher itself runs (top-K straight from the
    exponents, no N x N copy: algorithmic bytes = descriptors in + K correspondences out)."""
    import torch
    from relativepose_amd import rpmodule, synth
    base = [synth.make_match_case(N, 5000 + b)[:2] for b in range(min(B, 32))]
    kp = rpmodule.pack_keypoints([base[b % len(base)] for b in range(B)], dev)
    para = rpmodule.opts(*sigmas[0])
    f_s, w_s, f_t, w_t, ns_, nt_ = kp[2], kp[3], kp[6], kp[7], kp[8], kp[9]
    for _ in range(3):
        rpmodule.affinity_topk(f_s, w_s, f_t, w_t, ns_, nt_, para, want_wij=want_wij)
    reps = 20
    outs = rpmodule.affinity_topk_buffers(B, N, N, para.topK, dev, want_wij=want_wij)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        rpmodule.affinity_topk(f_s, w_s, f_t, w_t, ns_, nt_, para, want_wij=want_wij, out=outs)
    e1.record()
    e1.synchronize()
    a_ms = e0.elapsed_time(e1) / reps
    abytes = ((N + N) * 33 * 4 + (N * N * 4 if want_wij else N * para.topK * 12)) * B
    gbs = abytes / (a_ms * 1e-3) / 1e9
    return {"batch_pairs": B, "keypoints": N, "achieved": gbs, "frac": gbs / PEAK_HBM_GBS, "ms_per_launch": a_ms,
            "algorithmic_bytes_per_launch": abytes}


def geometry_roofline(cfg, n_img, N, dev, net_out_channels, feat_off):
    """The HBM-bound geometry stage at the bench batch (n_img = 2 x pairs panoramas): HIP-event time of back-to-back launches of
    relpose_pano2pc, relpose_warp_pairs (scatter + gather kernels) and relpose_sample_primitives against SURVEY 8(d)'s
    algorithmic bytes (pano2pc: read H*W*4 + write 3*H*W*4; warp: read h*h*7*4 of the observed face + write 8*H*W*4) and the bytes
    the kernels really move (pano2pc writes float64 like the reference + a validity byte; the warp keeps a 4-byte key per pixel)."""
    import torch
    from relativepose_amd import synth, util
    h, ds, mm = cfg["h"], cfg["dataset"], cfg["mask"]
    W = 4 * h
    d = synth.make_pairs(n_img // 2, 777, ds, h=h)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rgb, nrm, dep = t(d["rgb"].reshape(n_img, 3, h, W)), t(d["norm"].reshape(n_img, 3, h, W)), t(d["depth"].reshape(n_img, h, W))
    x = torch.zeros(n_img, 16, h, W, dtype=torch.float32, device=dev)
    x[:, :8].copy_(util.build_view_dev(rgb, nrm, dep, mm))
    rs = np.random.RandomState(5)
    poses = torch.from_numpy(np.stack([synth.random_rigid(rs, 0.5, 0.5) for _ in range(n_img)])).to(dev)
    pts, _ = synth.make_keypoints(n_img // 2, N, 777, mm, h=h)
    pts = t(pts.reshape(n_img, N, 2))
    npts = torch.full((n_img,), N, dtype=torch.int32, device=dev)
    f = torch.randn(n_img, net_out_channels, h, W, device=dev)

    def timed(fn, reps=20):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    out = {"bound": "hbm", "unit": "GB/s", "peak": PEAK_HBM_GBS, "images": n_img, "pano": f"{h}x{W}", "keypoints": N}
    for name, fn, alg, moved in (
            ("pano2pc", lambda: util.pano2pc_dev(dep, ds), h * W * 4 + 3 * h * W * 4, h * W * 4 + 3 * h * W * 8 + h * W),
            ("warp_pairs (scatter + gather)", lambda: util.warp_pairs_dev(x, poses, ds), h * h * 7 * 4 + 8 * h * W * 4,
             h * h * 7 * 4 + 8 * h * W * 4 + 2 * h * W * 4),
            ("sample_primitives", lambda: util.sample_primitives_dev(f, feat_off, nrm, dep, pts, npts, mm, ds, 0),
             N * (4 * 8 * 4 + 4 * 32 * 4 + 48 + 128), N * (4 * 8 * 4 + 4 * 32 * 4 + 48 + 128))):
        ms = timed(fn)
        out[name] = {"ms_per_launch": ms, "algorithmic_bytes_per_launch": alg * n_img, "achieved": alg * n_img / (ms * 1e-3) / 1e9,
                     "frac": alg * n_img / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS, "bytes_moved_per_launch": moved * n_img,
                     "moved_GBps": moved * n_img / (ms * 1e-3) / 1e9}
    return out


def _shared_state_dict(seed, S, rank, world):
    """The random-init weights, generated ONCE per node and shared between the ranks (48.5 M floats: 2.3 s of numpy per rank otherwise, on
    a host whose cores the 8 ranks also need for their input panoramas): rank 0 writes them to a file in shared memory, the others wait for it
    behind the launcher's barrier.  A single rank (or any failure of the shared path) just generates them."""
    from relativepose_amd import weights
    if world == 1:
        return weights.make_state_dict(seed, S)
    import tempfile
    import torch.distributed as dist
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    path = os.path.join(base, f"relpose_bench_weights_{os.environ.get('MASTER_PORT', '0')}_{seed}_{S}.npz")
    sd = None
    if rank == 0:
        sd = weights.make_state_dict(seed, S)
        try:
            np.savez(path + ".tmp.npz", **sd)
            os.replace(path + ".tmp.npz", path)
        except OSError:
            path = None
    dist.barrier()
    if rank != 0:
        try:
            with np.load(path) as z:
                sd = {k: z[k] for k in z.files}
        except Exception:       # noqa: BLE001 (rank 0 could not write it: every rank generates its own)
            sd = weights.make_state_dict(seed, S)
    dist.barrier()
    if rank == 0 and path:
        try:
            os.remove(path)
        except OSError:
            pass
    return sd


def worker(args):
    if args.hw_queues > 0:
        os.environ["GPU_MAX_HW_QUEUES"] = str(args.hw_queues)      # (read by the HIP runtime when it initialises: before the first torch.cuda call)
    import torch
    from relativepose_amd import distributed as D
    from relativepose_amd import params, synth, weights
    from relativepose_amd.model import SCNet
    from relativepose_amd.pipeline import RelativePosePipeline

    rank, world, local = D.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher provides WORLD_SIZE={world}")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        # one line per rank BEFORE any GPU work: which device this rank sits on, what it can reach over xGMI, which RCCL it runs -- so that a
        # multi-GPU run that dies or hangs later still says where every rank was (the JSON line carries rank 0's view only)
        import torch.distributed as dist
        pa = D.peer_access_summary()
        ri = D.rccl_info()
        try:
            prop = torch.cuda.get_device_properties(local)
            devname = f"{prop.name}, {prop.total_memory / 2**30:.0f} GiB, {prop.multi_processor_count} CUs"
        except Exception as e:      # noqa: BLE001
            devname = f"unknown ({type(e).__name__})"
        print(f"[bench rank {rank}/{world}] cuda:{local} ({devname}); visible GPUs {pa.get('gpus')}, peer-accessible pairs {pa.get('peer_accessible')}/{pa.get('peer_pairs')}; "
              f"backend {dist.get_backend()} (RCCL {ri['rccl_version']}); MASTER {os.environ.get('MASTER_ADDR')}:{os.environ.get('MASTER_PORT')}, "
              f"HSA_ENABLE_IPC_MODE_LEGACY={os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')}", file=sys.stderr, flush=True)
    cfg = dict(CONFIGS[args.config])
    prec = args.precision or cfg["precision"]
    ds, mm, h, S = cfg["dataset"], cfg["mask"], cfg["h"], cfg["S"]
    N = args.keypoints or cfg["N"]
    if args.keypoint_mode == "reference":
        N = args.sift + 120                 # capacity: detections + <= 60 cross-view picks + <= 60 picks / 30 random points per view ('second')
        if mm == "kinect":
            N = 300 + 60 + 200              # 300 sampled detections + 60 picks + <= 200 picks / 100 random points (rputil.py:240-353)
    if args.scaling == "strong":
        total = args.total_pairs
    else:
        total = (args.pairs or cfg["pairs"]) * world
    lo, hi = D.shard_range(total, rank, world)
    nloc = hi - lo
    sigmas = params.final_params(ds)
    depth = max(1, args.inflight)
    nbatch = max(depth, args.batches)

    # synthetic inputs + random-init weights (no dataset / checkpoint ships with the reference)
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=cfg["tanh"], skipLayer=1, outputType="rgbdnsf", snumclass=S))
    net.load_state_dict(_shared_state_dict(7, S, rank, world))
    net.set_precision(prec)
    Cc = N * 5
    pipe = RelativePosePipeline(net, ds, mm, sigmas, max_edges=min(Cc * (Cc - 1), (1 << 20) * max(1, (N // 200) ** 2)),
                                outputs="pose" if args.pose_outputs else "all", self_stream_cache=not args.no_self_cache,
                                tail_overlap=not args.no_tail_overlap, net_priority=args.net_priority, loop_fit_cluster=args.fit_cluster,
                                keypoints=args.keypoint_mode)
    ref_kp = args.keypoint_mode == "reference"
    if ref_kp:
        from relativepose_amd import rputil
    batches, first = [], None
    for j in range(nbatch):
        seed = 1000 * (args.config + 1) + lo + 100000 * j      # seed = 1000*config + pair index; slot j>0: other pairs
        dj = synth.make_pairs(nloc, seed, ds, h=h)
        pj, wj = synth.make_keypoints(nloc, N, seed, mm, h=h)
        if j == 0:
            first = (dj, pj, wj)
        if ref_kp:
            sift = [(rputil.map_detections(a, mm, h), rputil.map_detections(c, mm, h)) for a, c in synth.make_sift_detections(nloc, args.sift, seed, mm, h)]
            batches.append(pipe.prepare(dj["rgb"], dj["norm"], dj["depth"], None, None, dev, keep_host=not args.no_h2d, sift=sift,
                                        kp_seeds=[[seed + 31 * b + lvl for lvl in range(3)] for b in range(nloc)]))
        else:
            batches.append(pipe.prepare(dj["rgb"], dj["norm"], dj["depth"], pj, wj, dev, keep_host=not args.no_h2d))

    # PCIe-inclusive mode, where the uploads go (--h2d-mode):
    #   slot       on the batch's own slot stream, right before its first warp (idle then; no fifth stream to share a hardware queue): fine while a
    #              step's upload is short (184 MB = 3.4 ms at 160x640: -1 %)
    #   lookahead  on a copy stream, issued `depth` steps AHEAD (when batch i starts, the inputs of batch i + depth go up; its buffers were last
    #              used `batches - depth` steps ago -- the copy waits for that batch's done event only), so a 734 MB upload (13 ms at 320x1280)
    #              runs under the other batches' convolutions instead of in front of its own batch (round 4: -21 % at configs[4])
    per_step_h2d = 0 if args.no_h2d else sum(t.numel() * t.element_size() for t in batches[0]["host"].values())
    # (measured, round 5: configs[4] 764 -> 925 pairs/s PCIe-inclusive = -4 % instead of -22 %; configs[1] 660 -> 663: look-ahead whenever the rotation allows it)
    depth_h2d = max(1, min(args.h2d_inflight, depth)) if args.h2d_inflight > 0 else depth      # batches in flight while the inputs stream in
    h2d_mode = args.h2d_mode if args.h2d_mode != "auto" else ("lookahead" if nbatch >= 2 * depth_h2d else "slot")
    if h2d_mode == "lookahead" and nbatch < 2 * depth_h2d:
        h2d_mode = "slot"
    copy_stream = torch.cuda.Stream() if (h2d_mode == "lookahead" and not args.no_h2d) else None

    def issue_upload(st):
        if "done_ev" in st:
            copy_stream.wait_event(st["done_ev"])
        with torch.cuda.stream(copy_stream):
            for kk, src in st["host"].items():
                st[kk].copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(copy_stream)
        st["upload_ev"] = ev

    def run_steps(k, h2d=False):
        """k steps = k batches of nloc pairs on this GPU, each followed by the pose gather; returns the last result."""
        dp = depth_h2d if h2d else depth
        if h2d and h2d_mode == "lookahead":
            for st in batches:
                st.pop("upload_ev", None)

            def before(i, st):          # (called under batch i's slot stream, right before the batch is started)
                if "upload_ev" not in st:
                    issue_upload(st)                                   # the first `depth` batches of a run: nothing was sent ahead
                torch.cuda.current_stream().wait_event(st.pop("upload_ev"))
                j = i + dp
                if j < k and "upload_ev" not in batches[j % nbatch]:
                    issue_upload(batches[j % nbatch])
        else:
            before = (lambda i, st: pipe.upload_inputs(st, None)) if h2d else None
        if world == 1 or args.gather == "step" or total % world:        # (ragged shards: the per-step gather pads every block)
            return pipe.run_pipelined(batches, k, lambda i, pose, status: D.gather_poses(pose, status, total, world), depth=dp,
                                      before_batch=before)[-1]
        # --gather run (default): ONE collective for the whole run (north_star: "a single RCCL gather of the poses") -- the k steps'
        # poses of this rank are stacked and gathered once, inside the timed region; no RCCL kernel shares a hardware queue with
        # the SCNet / slot streams in steady state
        res = pipe.run_pipelined(batches, k, None, depth=dp, before_batch=before)
        pose = torch.stack([r[0] for r in res], 1).reshape(nloc * k, 4, 4)          # [pair, step] order: a rank's block stays contiguous
        status = torch.stack([r[1] for r in res], 1).reshape(nloc * k)
        gp, gs = D.gather_poses(pose, status, total * k, world)
        return gp.reshape(total, k, 4, 4)[:, -1], gs.reshape(total, k)[:, -1]

    def timed(k, h2d=False):
        torch.cuda.synchronize()
        D.barrier(world)
        t0 = time.perf_counter()
        out = run_steps(k, h2d)
        torch.cuda.synchronize()
        D.barrier(world)
        return D.max_over_ranks(time.perf_counter() - t0, world, dev), out

    # set-up, not a warm-up step: the first use of an in-flight slot allocates its SCNet workspace (a multi-GB hipMalloc), builds its launch plan and
    # creates its streams -- one pass per slot, so that the timed region is the steady-state loop for any --warmup the caller picks (the default
    # --warmup 2 covers both slots by itself)
    if args.warmup < depth:
        run_steps(depth)                    # (through the gather as well: the first collective creates the RCCL communicator)
    if args.warmup:
        run_steps(args.warmup)
    ncoll0 = D.COLLECTIVES["all_gather"]
    dt, (poses, status) = timed(args.steps)
    ncoll = D.COLLECTIVES["all_gather"] - ncoll0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, poses, status)
    dt_h2d = None
    if not args.no_h2d:
        run_steps(1, True)
        dt_h2d, _ = timed(args.steps, True)

    if world > 1:
        # per-rank rate on stderr (the JSON line carries the whole-job value only): a slow GPU / a bad link shows up here
        print(f"[bench rank {rank}/{world} cuda:{local}] {nloc * args.steps / dt:.1f} pairs/s on this rank's {nloc} pairs per step "
              f"({dt / args.steps * 1e3:.2f} ms/step, max over ranks)", file=sys.stderr, flush=True)
    if rank == 0:
        import torch.distributed as dist
        ms = dt / args.steps * 1e3
        f32 = prec == "f32"
        # BASELINE.json's metric is quoted at 160x640; configs[4] is the same pipeline on 320x1280 panoramas and its lines say so
        res = {"metric": "scan-pairs/sec end-to-end (completion+feat+spectral-match), 160x640 RGB-D" if h == 160 else
                         f"scan-pairs/sec end-to-end (completion+feat+spectral-match), {h}x{4 * h} RGB-D (BASELINE configs[{args.config}]; the headline metric is quoted at 160x640)",
               "value": total * args.steps / dt, "unit": "pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": ms, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
               "dtype": "f32" if f32 else DTYPE_EXACT[prec] if prec in DTYPE_EXACT else ("f16 (plain fp16 MFMA conv products, fp32 accumulate and fp32 BatchNorm statistics; NOT a parity configuration: on the reference-pinned "
                                          "fixtures the free-running rotation is within 1e-5 of the reference after level 0 but only within 4e-3 after level 2 -- "
                                          "it breaks the 1e-4 bar, tests/test_gpu_e2e.py; f16x3 meets it with 1e-7)"
                                          if prec == "f16" else
                                          f"f32 (conv products as 3 x {prec[:-2]} MFMA terms, fp32 accumulate: the configs[4] 'fp16 MFMA conv path'; "
                                          "not the fp32 parity configuration)"),
               "data": "synthetic (seeded box-room RGB-D panoramas, injected keypoints, random-init weights)",
               "config": {"workload": cfg["label"], "baseline_config_index": args.config, "dataset": ds, "mask": mm, "pano": f"{h}x{4 * h}",
                          "parity": cfg.get("parity_note", "reference goldens at this size (tests/golden/*.npz, SURVEY 8c)"),
                          "pairs_per_step_total": total, "pairs_per_gpu": nloc, "keypoints": N, "semantic_classes": S,
                          "keypoint_mode": ("reference: re-derived at every level from the level's feature maps (rputil.getKeypoint behind the SIFT detector, "
                                            f"{args.sift} synthetic detections per view; up to {batches[0]['N']} keypoints per view); NOT the BASELINE workload") if ref_kp
                                           else "given (one injected set per view for all levels: the BASELINE workload, SURVEY 8d)",
                          "recurrent_levels": 3, "conv_precision": prec, "parallelism": f"pairs sharded x{world}",
                          "batches_in_flight": depth, "hw_queues_env": os.environ.get("GPU_MAX_HW_QUEUES"), "prepared_batches_rotated": nbatch, "setup_passes_before_warmup": depth if args.warmup < depth else 0,
                          "scnet_outputs": "pose path only (normal, depth, features): opt-in, NOT the BASELINE metric" if args.pose_outputs else "all (like the reference)",
                          "level0_zero_warp_plan": True,
                          # levels 1-2 take the self-view encoder streams (conv1-3 self members, conv4 self K slices) from level 0 of the same
                          # pass (relpose_scnet_forward4; bitwise the same output); "roofline" below is still measured on FULL forwards
                          "self_stream_cache": not args.no_self_cache,
                          "shard_sizes": [D.shard_range(total, r, world)[1] - D.shard_range(total, r, world)[0] for r in range(world)],
                          "pose_all_gathers_in_timed_region": ncoll,
                          "dist_backend": dist.get_backend() if world > 1 else None,
                          "dist_world_size": dist.get_world_size() if world > 1 else 1,
                          "peer_access": D.peer_access_summary() if world > 1 else None,      # hipDeviceCanAccessPeer (xGMI inside one node)
                          "collective": ("one all_gather of [steps*pairs,17] f64 (pose + status) per run" if (args.gather == "run" and total % world == 0)
                                         else "one all_gather of [pairs,17] f64 (pose + status) per step") if world > 1 else None},
               "status_ok_fraction": float((status == 0).double().mean().item())}
        if dt_h2d is not None:
            res["pcie_inclusive"] = {"value": total * args.steps / dt_h2d, "unit": "pairs/s", "ms_per_step": dt_h2d / args.steps * 1e3,
                                     "h2d_bytes_per_step_per_gpu": per_step_h2d, "mode": h2d_mode, "batches_in_flight": depth_h2d,
                                     "note": ("every step's panoramas + keypoints uploaded from pinned host memory on the batch's own stream (under the other "
                                              "in-flight batch's forward)" if h2d_mode == "slot" else
                                              f"every step's panoramas + keypoints uploaded from pinned host memory on a copy stream {depth_h2d} steps ahead of their batch "
                                              "(under the in-flight batches' convolutions)") + "; never the headline value"}
        if not args.no_aux:
            # --- roofline of the dominant kernel: implicit-GEMM conv, HIP events on the launch stream
            x = torch.randn(2 * nloc, 16, h, 4 * h, device=dev)
            net.profile(x, 1)
            g_ms, o_ms, n_gemm = net.profile(x, 3)
            del x
            flops = GFLOP_PER_IMAGE * 1e9 * 2 * nloc
            ach = flops / (g_ms * 1e-3) / 1e12
            # split-16-bit modes: every fp32 product costs three dense 16-bit MFMA products -> algorithmic peak = 2500 / 3
            # bf16x9 / bf16x6 (exact-product emulation): nine / six dense bf16 MFMA products per fp32 product -> 2500 / 9, 2500 / 6
            peak = PEAK_F32_MFMA_TFLOPS if f32 else (PEAK_F16_MFMA_TFLOPS if prec == "f16" else PEAK_F16_MFMA_TFLOPS / MFMA_TERMS[prec])
            tr = _traffic(f"config{args.config}_{prec}_pairs{nloc}")
            stack16 = ("SCNet conv stack: conv_s2_tile_kernel + conv_s2_strip_kernel + deconv_tile_kernel (SPLIT instantiations) + conv_igemm_kernel (conv6-9, deconv4-9) "
                       "+ conv1_mfma_kernel + heads_kernel (fp32)" if prec != "bf16x3" else "SCNet conv stack: conv_igemm_kernel (every layer) + conv1_mfma_kernel + heads_kernel (fp32)")
            # plan-aware in-loop fraction: what the three forwards of a step really execute (level 0 = the zero-warp plan, levels 1-2 = the
            # self-stream cache) over the step time -- the number that sets the headline; "frac" above it is kernel efficiency on FULL forwards
            FW = SCNet.FLAG_ZERO_WARP | (SCNet.FLAG_POSE_OUTPUTS if args.pose_outputs else 0)
            m_full = net.plan_macs(2 * nloc)
            f_lvl0 = net.plan_macs(2 * nloc, FW) / m_full
            f_next = (net.plan_macs(2 * nloc, FW & ~SCNet.FLAG_ZERO_WARP, self_cached=True) if not args.no_self_cache
                      else net.plan_macs(2 * nloc, FW & ~SCNet.FLAG_ZERO_WARP)) / m_full
            exec_gflop = flops / 1e9 * (f_lvl0 + 2 * f_next)
            # the same three forwards ALONE on the GPU (level-0 plan, then two self-cached ones; nothing on any other stream): what the SCNet part
            # of a step costs without the other batch's matcher / geometry / head / tail beside it
            xa = torch.randn(2 * nloc, 16, h, 4 * h, device=dev)
            xa[:, 8:] = 0
            xb = xa.clone()
            xb[:, 8:] = torch.randn(2 * nloc, 8, h, 4 * h, device=dev)
            fo = torch.empty(2 * nloc, net.out_channels, h, 4 * h, device=dev)
            outs_kw = "pose" if args.pose_outputs else "all"

            def alone_step():
                tag = net.new_self_tag() if not args.no_self_cache else 0
                net.forward(xa, out=fo, zero_warp=True, outputs=outs_kw, self_tag=tag)
                net.forward(xb, out=fo, outputs=outs_kw, self_tag=tag)
                net.forward(xb, out=fo, outputs=outs_kw, self_tag=tag)
            for _ in range(2):
                alone_step()
            ea0, ea1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ea0.record()
            for _ in range(6):
                alone_step()
            ea1.record(); ea1.synchronize()
            alone_ms = ea0.elapsed_time(ea1) / 6
            del xa, xb, fo
            res["roofline"] = {"kernel": "SCNet conv stack: conv_igemm_kernel + conv_s2_tile_kernel + conv_s2_strip_kernel + deconv_tile_kernel + conv1_mfma_kernel + heads_kernel (fp32 MFMA 32x32x2)"
                                         if f32 else (stack16 + " -- fp16 MFMA 32x32x16" if prec == "f16" else stack16 + f" -- {MFMA_TERMS[prec]} x {prec[:-2]} MFMA 32x32x16 per fp32 product"),
                               "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
                               "traffic": tr["bytes"] if tr else None, "traffic_unit": "HBM bytes per forward (all conv launches; rocprofv3 PMC)",
                               "traffic_profile": tr["profile"] if tr else None,
                               "launches_per_forward": int(n_gemm), "ms_per_forward_gemm": g_ms, "ms_per_forward_other": o_ms,
                               "algorithmic_gflop_per_forward": flops / 1e9,
                               "in_loop": {"executed_gflop_per_step": exec_gflop, "achieved": exec_gflop / ms, "frac": exec_gflop / ms / peak,
                                           "executed_fraction_of_full_forward": {"level0_zero_warp_plan": f_lvl0, "levels_1_2": f_next},
                                           "forwards_alone": {"ms_per_step": alone_ms, "achieved": exec_gflop / alone_ms, "frac": exec_gflop / alone_ms / peak,
                                                              "pairs_per_s_if_nothing_else_ran": nloc * 1e3 / alone_ms,
                                                              "note": "the step's three forwards with no other stream active (HIP events): in_loop.frac / this = what overlapping "
                                                                      "the other batch's matcher, geometry, head and tail costs the convolutions"},
                                           "note": "plan-aware: multiply-accumulates the three forwards of a step really launch (relpose_scnet_plan_macs) "
                                                   "x 2 / ms_per_step / peak; the reference's algorithmic work per step is 3 x algorithmic_gflop_per_forward"}}
            # --- N x N affinity build at the bench batch and at a batch where the bytes are meaningful
            a_small = affinity_roofline(N, nloc, dev, sigmas)
            a_big = affinity_roofline(N, 1024, dev, sigmas)
            tra = _traffic(f"affinity_b1024_n{N}")
            ins = _traffic(f"affinity_b1024_n{N}_insts")
            valu = None
            if ins:
                # the bound this kernel actually runs against: VALU issue.  Every VALU wave-instruction takes one 4-cycle issue slot
                # of its SIMD, so wave_insts x 4 / (1024 SIMDs x 2.4 GHz) is the time the kernel cannot beat without issuing fewer instructions
                floor_us = ins["valu"] * 4.0 / (1024 * 2.4e9) * 1e6
                valu = {"wave_insts": ins["valu"], "salu_wave_insts": ins["salu"], "floor_us": floor_us, "measured_us": a_big["ms_per_launch"] * 1e3,
                        "frac": floor_us / (a_big["ms_per_launch"] * 1e3), "lane_ops_per_entry": (ins["valu"] + ins["salu"]) * 64 / ins["entries"],
                        "mfma_screened_entries_over_real": ins["mfma_screened_entries"] / ins["entries"],
                        "hbm_frac_at_the_valu_floor": a_big["algorithmic_bytes_per_launch"] / (floor_us * 1e-6) / 1e9 / PEAK_HBM_GBS,
                        "profile": ins["profile"],
                        "note": "frac = floor_us / measured_us: the share of the launch the VALU issue slots alone account for; at the floor the kernel would reach "
                                "hbm_frac_at_the_valu_floor of HBM peak -- the >= 0.60 HBM target needs fewer instructions, not more bandwidth"}
            res["roofline_affinity"] = {"kernel": "affinity_tile_kernel + fix-up scan (batch 1024) / affinity_rows_kernel (bench batch), materialised fp32 wij", "bound": "hbm", "unit": "GB/s",
                                        "peak": PEAK_HBM_GBS, "achieved": a_big["achieved"], "frac": a_big["frac"],
                                        "traffic": tra["bytes"] if tra else None, "traffic_unit": "HBM bytes per launch at batch 1024 (rocprofv3 PMC: FETCH_SIZE x2 + WRITE_SIZE, profiles/traffic.json)",
                                        "traffic_profile": tra["profile"] if tra else None,
                                        "valu": valu,
                                        "at_batch_1024": a_big, "at_bench_batch": a_small,
                                        "fused_at_batch_1024": affinity_roofline(N, 1024, dev, sigmas, want_wij=False),
                                        "note": "headline = batch 1024 (one launch at the bench batch moves only "
                                                f"{a_small['algorithmic_bytes_per_launch'] / 1e6:.1f} MB, i.e. less than 1 us of HBM time)"}
            res["roofline_geometry"] = geometry_roofline(cfg, 2 * nloc, N, dev, net.out_channels, pipe.feat_off)
            if ref_kp:
                # the per-level keypoint stage alone (descriptors + fused distance / NMS + assembly): HIP events, back-to-back launches on a batch's
                # tables; algorithmic bytes = every view's 32-channel feature map read once + the keypoint lists written
                st0 = batches[0]
                ftest = torch.randn(2 * nloc, net.out_channels, h, 4 * h, device=dev)
                for _ in range(2):
                    rputil.keypoints_reference_dev(ftest, pipe.feat_off, st0["kp"][0], mm, L=st0["N"], workspace=st0["kp_ws"])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    rputil.keypoints_reference_dev(ftest, pipe.feat_off, st0["kp"][0], mm, L=st0["N"], workspace=st0["kp_ws"])
                e1.record(); e1.synchronize()
                k_ms = e0.elapsed_time(e1) / 10
                kb = 2 * nloc * (32 * h * 4 * h * 4 + st0["N"] * 24)
                nq = int(st0["kp"][0]["nq"])
                res["roofline_keypoints"] = {"kernel": "kp_desc_kernel + kp_tile_best_kernel + kp_pick_kernel + kp_assemble_kernel (csrc/keypoints.hip)", "bound": "hbm (by bytes) / valu (in practice: 96 rounded fp32 operations per pixel and query)",
                                             "ms_per_level": k_ms, "queries": nq, "algorithmic_bytes_per_level": kb, "achieved": kb / (k_ms * 1e-3) / 1e9, "unit": "GB/s",
                                             "peak": PEAK_HBM_GBS, "frac": kb / (k_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                                             "valu_gflops": nq * h * 4 * h * 96 / (k_ms * 1e-3) / 1e9}
                del ftest
        if world == 1 and not args.no_cpu_baseline and not ref_kp:      # (the oracle loop takes injected keypoints: the BASELINE workload only)
            res["cpu_baseline"] = cpu_baseline(cfg, N, first[0], first[1], first[2], sigmas)
        print(json.dumps(res), flush=True)
    if world > 1:
        import torch.distributed as dist
        D.barrier(world)                 # rank 0 is still taking its roofline side measurements: leave the group together
        dist.destroy_process_group()


def _spawned(rank, args, port):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    worker(args)


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launched plainly (python bench.py --gpus N): spawn the N ranks here, one per GPU, RCCL over xGMI
        # (counting the devices initialises HIP in this process; under the one-device test hook the parent leaves the GPU to its ranks)
        if not os.environ.get("RELPOSE_FORCE_DEVICE"):
            import torch
            have = torch.cuda.device_count()
            if have < args.gpus:
                print(f"bench.py: --gpus {args.gpus} requested but only {have} GPU(s) visible; refusing to fall back", file=sys.stderr)
                raise SystemExit(2)
        import torch.multiprocessing as mp
        for attempt in range(3):             # a free port can be taken between the probe and the rendezvous: retry with another one
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            try:
                mp.spawn(_spawned, args=(args, port), nprocs=args.gpus, join=True)
                return
            except Exception as e:
                if attempt == 2 or not any(t in str(e) for t in ("Address already in use", "EADDRINUSE", "address already in use")):
                    raise
                print(f"bench.py: port {port} was taken ({e.__class__.__name__}); retrying with another one", file=sys.stderr)
        return
    worker(args)


if __name__ == "__main__":
    main()
