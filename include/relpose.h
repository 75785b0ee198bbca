/*
 * relpose.h -- C ABI of librelpose_hip.so, the MI355X (gfx950) implementation of
 * the relative-pose inference hot path of zhenpeiyang/RelativePose.
 *
 * The reference has no FFI: its boundary is a set of Python call sites.  Each
 * entry point below names the reference function it replaces (file:line in the
 * upstream tree).  INTEGRATION.md shows the ctypes stubs a maintainer would add
 * to the reference to route those call sites here.
 *
 * Conventions
 *  - every pointer argument is DEVICE memory unless its name ends in _host;
 *  - the caller owns all buffers; the library never frees caller memory.  Its own
 *    device allocations belong to a RelposeSCNet handle and are freed by
 *    relpose_scnet_destroy: the packed weights (relpose_scnet_finalize) and one
 *    launch-descriptor table per (workspace, n_images) pair, built by the FIRST
 *    relpose_scnet_forward on that workspace (that first call hipMallocs + copies
 *    synchronously; later calls only enqueue).  Scratch comes from caller-provided
 *    workspaces whose size is returned by the *_workspace_bytes functions;
 *  - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *    default stream); apart from the first-forward plan build and
 *    relpose_scnet_finalize / relpose_scnet_profile / relpose_sift_detect (its overflow flag) / relpose_fgr / relpose_ransac (their statuses) no entry point synchronises;
 *  - return value: 0 = enqueued, <0 = invalid argument (RELPOSE_EINVAL) or HIP
 *    error (-(1000+hipError_t)).  Per-pair degenerate inputs are NOT errors: the
 *    reference returns identity for them (rpmodule.py:346-348,377-379,406-408,
 *    440-443,469-472) and so do we, with the reason in status[b];
 *  - panoramas are four-face skyboxes, h rows x 4h columns (the reference
 *    hard-codes h = 160); images are NCHW float32 like the reference tensors.
 */
#ifndef RELPOSE_H
#define RELPOSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RELPOSE_EINVAL (-1)
#define RELPOSE_ENOMEM (-2)
#define RELPOSE_EROUNDS (-3) /* relpose_mesh_components: labels still moved in round max_rounds; the outputs hold nothing to rely on */

/* status[b] of relpose_match_pairs */
enum {
    RELPOSE_OK = 0,
    RELPOSE_FEW_KEYPOINTS = 1, /* <3 keypoints or <3 correspondences      rpmodule.py:346,377 */
    RELPOSE_DIST_FILTER = 2,   /* <3 pairs pass the distance test          rpmodule.py:406 */
    RELPOSE_ANGLE_FILTER = 3,  /* <3 pairs pass the angle test             rpmodule.py:440 */
    RELPOSE_ZERO_WEIGHT = 4,   /* every pair weight is 0                   rpmodule.py:469 */
    RELPOSE_EDGE_OVERFLOW = 5, /* more surviving pairs than the workspace was sized for */
    RELPOSE_NOT_CONVERGED = 6  /* a leading-eigenvector solve (rpmodule.py:273, ARPACK there) did not reach its residual
                                  tolerance within the restart budget; the pose is computed from the last iterate */
};

enum { RELPOSE_SUNCG = 0, RELPOSE_MATTERPORT = 1, RELPOSE_SCANNET = 2 };   /* dataset conventions */
enum { RELPOSE_MASK_SECOND = 0, RELPOSE_MASK_KINECT = 1 };                   /* util.apply_mask methods */
enum { RELPOSE_COMPOSE_EVAL = 0, RELPOSE_COMPOSE_LIB = 1 };                       /* output composition variants */
enum { RELPOSE_FIT_IRLS_SM = 0, RELPOSE_FIT_HORN87 = 1, RELPOSE_FIT_IRLS = 2, RELPOSE_FIT_SPECTRAL = 3 };

/* Hyper-parameters of the pose module: class opts, RPModule/rputil.py:11-22. */
typedef struct RelposeParams {
    double distThre;    /* 0.08 */
    double distSepThre; /* 1.5*0.08 */
    double angleThre;   /* pi/4 */
    double sigmaAngle1, sigmaAngle2, sigmaDist, sigmaFeat;
    double mu;          /* 0.3 */
    int32_t topK;       /* 5 (<= 8) */
    int32_t method;     /* RELPOSE_FIT_* ; 'irls+sm' by default */
} RelposeParams;

void relpose_default_params(RelposeParams* p_host);

/* Process-wide kernel-selection knobs.  Every setting produces the same results (the parity tests force each variant
 * through the same checks); they exist for those tests and for tuning, NOT for the data path: nothing in the product path sets them
 * (round 6: the one per-call choice the serving loop makes, the fit's workgroups per pair, is an argument of relpose_match_pairs_ex).
 * Returns the previous value, RELPOSE_EINVAL for an unknown key.  Not synchronised with calls in flight on other threads.
 *   RELPOSE_TUNE_AFFINITY_KERNEL    0 = by batch size (default), 1 = row kernel (targets in registers), 2 = tile kernel
 *                                   (fp16-MFMA candidates + exact arithmetic on them), 3 = LDS kernel (the nt_max > 512 path),
 *                                   4 = pool variant (round 5: the tile kernel's stages as separate dense launches; auto-selected for the
 *                                   fused form beyond 256 targets at large batches, where it measured faster; it keeps one grow-only scratch
 *                                   block per (device, stream) it was called on for the life of the process: ~0.3 KB per source row)
 *   RELPOSE_TUNE_FIT_MAX_PRODUCTS   0 = default budget (192) of matrix-vector products per eigen-solve; a tiny budget
 *                                   forces RELPOSE_NOT_CONVERGED
 *   RELPOSE_TUNE_FIT_CLUSTER        0 = by problem size (default), n = workgroups per scan pair in the fit (1, 2, 4, 8)
 *   RELPOSE_TUNE_FIT_GLOBAL_VECTORS 0 = by problem size, 1 = keep the fit's per-correspondence vectors in global memory
 *                                   (the > 4500-correspondence layout) whatever the size
 *   RELPOSE_TUNE_FIT_FIXED_CHECKS   0 = the eigen-solve places its convergence tests where the residual estimate is predicted to
 *                                   reach the tolerance (default), 1 = a test every 8 products (the earlier rule; A/B switch).  The
 *                                   one knob whose settings agree to round-off only (both converge to 1e-13; the number of Lanczos
 *                                   steps differs)
 *   RELPOSE_TUNE_HEADS_KERNEL       0 = SCNet's heads on the streamed kernel (default), 1 = on the lane-per-pixel kernel (same bits)
 *   RELPOSE_TUNE_DECONV_STRIP       0 = SCNet's deconv4 / deconv5 on the phase strip kernel (default): the split-K launches, and deconv4's
 *                                   unsplit launch of the three-piece bf16 modes (direct stores, fused BatchNorm records), 1 = on the
 *                                   implicit-GEMM kernel (same K split, same order of every sum, same bits); read when a forward looks
 *                                   up its plan: each value has plans of its own
 *   RELPOSE_TUNE_ZERO_TILES         0 = SCNet's conv2 / conv3 tile kernels run only the patches whose receptive field holds a non-zero
 *                                   input pixel plus one representative per edge class, the others are copies (default), 1 = every
 *                                   patch is computed (same bits); read when a forward looks up its plan, like RELPOSE_TUNE_DECONV_STRIP
 *   RELPOSE_TUNE_CONV1_ZERO         0 = SCNet's input resize writes the occupancy words of the zero-tile lists itself, and conv1 neither
 *                                   computes nor stores an (image, stream, 8 x 32 tile) block of A1 whose inputs are all +-0 and whose
 *                                   zeros an earlier forward on the workspace left there (it stores +0.0 once otherwise) (default),
 *                                   1 = a separate occupancy pass, every launched block computed and stored (same bits); read by every
 *                                   forward (the plans are the same); without the zero-tile lists (RELPOSE_TUNE_ZERO_TILES = 1) 1 is what runs
 *   RELPOSE_TUNE_CONV4_ROWS         0 = SCNet's conv4 computes, per K slice (= encoder stream), only the rows whose 3 x 3 occupancy blocks hold a
 *                                   non-zero input value plus one representative per BatchNorm group and edge class, on a row-list launch, where
 *                                   that list is sparse enough to pay; the split-K reduce reads the other rows through a map (default),
 *                                   1 = every row on the strip kernel and no extra launches, 2 = the row-list launch for every slice whatever
 *                                   its density (same bits all three; a slice whose stream holds a non-finite input value always
 *                                   stays on the strip kernel); 0 / 2 need the occupancy words (RELPOSE_TUNE_ZERO_TILES = 0); read
 *                                   when a forward looks up its plan (0 and 2 share one) */
enum { RELPOSE_TUNE_AFFINITY_KERNEL = 0, RELPOSE_TUNE_FIT_MAX_PRODUCTS = 1, RELPOSE_TUNE_FIT_CLUSTER = 2,
       RELPOSE_TUNE_FIT_GLOBAL_VECTORS = 3, RELPOSE_TUNE_FIT_FIXED_CHECKS = 4, RELPOSE_TUNE_HEADS_KERNEL = 5, RELPOSE_TUNE_DECONV_STRIP = 6,
       RELPOSE_TUNE_ZERO_TILES = 7, RELPOSE_TUNE_CONV1_ZERO = 8, RELPOSE_TUNE_CONV4_ROWS = 9, RELPOSE_TUNE_COUNT = 10 };
int relpose_set_tuning(int32_t key, int32_t value);
const char* relpose_version(void);
/* ------------------------------------------------------------------ matcher
 * Keypoint sets of B scan pairs, padded to ns_max / nt_max rows.
 * Mirrors the dict the reference helper takes (rpmodule.py:317-326):
 * 'pc'[k,3] f64, 'normal'[k,3] f64, 'feat'[k,32] f32, 'weight'[k] f64. */
typedef struct RelposeKeypoints {
    int32_t B, ns_max, nt_max;
    const int32_t* ns;      /* [B] valid source keypoints per pair */
    const int32_t* nt;      /* [B] */
    const double* pc_s;     /* [B, ns_max, 3] */
    const double* normal_s; /* [B, ns_max, 3] */
    const float* feat_s;    /* [B, ns_max, 32] (unscaled; /100 happens inside, rpmodule.py:342) */
    const double* weight_s; /* [B, ns_max] */
    const double* pc_t;     /* [B, nt_max, 3] */
    const double* normal_t;
    const float* feat_t;
    const double* weight_t;
} RelposeKeypoints;

/* Optional intermediate outputs of the matcher (any pointer may be NULL). */
typedef struct RelposeMatchDebug {
    float* wij;          /* [B, ns_max, nt_max] row-normalised affinity (rpmodule.py:354-363), f32 */
    int32_t* corres_j;   /* [B, ns_max, topK]   target index of each top-K correspondence (:367-374) */
    double* corres_w;    /* [B, ns_max, topK]   wij at those entries, f64 */
    int32_t* counts;     /* [B, 4]  {#pairs passing distance test, #surviving pairs M, #nonzero weights, K_eff} */
    double* trace;       /* [B, 6, 16] pose after the initial IRLS and after each of the 5 spectral rounds */
    int32_t* eig_iters;  /* [B, 5]  power iterations used per spectral round */
} RelposeMatchDebug;

/* max_edges = capacity, per pair, of the symmetric pair-compatibility graph
 * (2 x surviving pairs); 0 = worst case ns_max*topK*(ns_max*topK-1).
 * LIMITS (the reference has none; its largest shipped configuration uses 400 keypoints per view): ns_max * topK <=
 * RELPOSE_MAX_CORRESPONDENCES (the pair-consistency kernels keep a row's correspondence list in LDS) and nt_max <= RELPOSE_MAX_TARGETS
 * (beyond 512 targets the affinity kernel keeps all target descriptors of a pair in LDS).  Outside them
 * relpose_match_workspace_bytes returns 0 and relpose_match_pairs / relpose_affinity_topk RELPOSE_EINVAL. */
#define RELPOSE_MAX_CORRESPONDENCES 8192
#define RELPOSE_MAX_TARGETS 1152
size_t relpose_match_workspace_bytes(int32_t B, int32_t ns_max, int32_t nt_max, int32_t topK, int64_t max_edges);

/* Replaces RelativePoseEstimation_helper (RPModule/rpmodule.py:317-508) for a
 * batch of pairs: affinity + top-K + pairwise consistency + fit.  pose [B,16]
 * row-major 4x4 float64, status [B]. */
int relpose_match_pairs(const RelposeParams* params_host, const RelposeKeypoints* kp_host,
                        void* workspace, size_t workspace_bytes, int64_t max_edges,
                        double* pose, int32_t* status, const RelposeMatchDebug* debug_host, void* stream);

/* relpose_match_pairs with its per-call choices IN the call (round 6; the reference call carries its own `para`, rpmodule.py:317-326): a
 * struct_size-versioned argument block like RelposeForwardArgs -- fields beyond the caller's struct_size take their defaults (0).
 *   params_host .. stream  as relpose_match_pairs
 *   fit_cluster            workgroups per scan pair in the robust fit (rpmodule.py:212-315): 0 = by problem size (small batches of large pairs
 *                          get helper workgroups: a latency tool), 1 = none (what a serving loop with several batches in flight wants: helpers
 *                          take compute units from the other batches' convolutions), 2 / 4 / 8.  Every setting gives bitwise the same poses.
 *                          This is the per-call form of RELPOSE_TUNE_FIT_CLUSTER; a non-zero value here wins over the process-wide test knob,
 *                          so concurrent callers with different choices do not interfere (pipeline.run_pipelined uses it).
 *   affinity_kernel        0 = by batch size, 1..4 as RELPOSE_TUNE_AFFINITY_KERNEL (same results); a non-zero value wins over the test knob. */
typedef struct RelposeMatchArgs {
    uint32_t struct_size;
    int32_t fit_cluster;
    const RelposeParams* params_host;
    const RelposeKeypoints* kp_host;
    void* workspace;
    size_t workspace_bytes;
    int64_t max_edges;
    double* pose;
    int32_t* status;
    const RelposeMatchDebug* debug_host;
    void* stream;
    int32_t affinity_kernel;
    int32_t reserved0;
} RelposeMatchArgs;
int relpose_match_pairs_ex(const RelposeMatchArgs* args);

/* Stage A+B alone (rpmodule.py:342-379): N x N affinity build and row top-K.
 * wij may be NULL (fused variant: the matrix is never materialised). */
int relpose_affinity_topk(const RelposeParams* params_host, const RelposeKeypoints* kp_host,
                          float* wij, int32_t* corres_j, double* corres_w, int32_t* k_eff, void* stream);

/* ----------------------------------------------------------------- geometry */

/* util.apply_mask (util.py:209-232): x [n,c,h,4h] -> x*mask in place, mask [n,1,h,4h] (may be NULL). */
int relpose_apply_mask(float* x, float* mask, int32_t n, int32_t c, int32_t h, int32_t method, void* stream);

/* evaluation.py:217-230: view [n,8,h,4h] = mask*(rgb,norm,depth) ++ (masked depth != 0). */
int relpose_build_view(const float* rgb, const float* norm, const float* depth, float* view,
                       int32_t n, int32_t h, int32_t method, void* stream);

/* util.Pano2PointCloud (util.py:751-811): depth [n,h,4h] f32 -> pc [n,3,4*h*h] f64 in face-major point
 * order; valid [n,4*h*h] u8 marks the points the reference keeps (scannet drops depth==0). */
int relpose_pano2pc(const float* depth, double* pc, uint8_t* valid, int32_t n, int32_t h, int32_t dataset, void* stream);

/* util.warping (util.py:94-172) incl. depth2pc (:468-523) and reproj_helper (:537-749):
 * view [n,8,h,4h] f32, pose [n,16] f64 -> out [n,8,h,4h] f32 (the f64 result cast like torch_op.v);
 * identity pose gives zeros.  workspace: relpose_warp_workspace_bytes(n,h). */
size_t relpose_warp_workspace_bytes(int32_t n, int32_t h);
int relpose_warp(const float* view, const double* pose, float* out, void* workspace,
                 int32_t n, int32_t h, int32_t dataset, void* stream);

/* The warp of evaluation.py:221-222,235-236 for a batch of pairs, in place on the network input
 * x [n,16,h,4h] (n even; images 2b, 2b+1 are a pair): channels 0:8 of every image hold its own view
 * (caller-filled, only read here); channels 8:16 of image i receive the view of its partner (image i^1)
 * warped by pose[i] -- i.e. torch.cat((view, warping(other, pose)), 1) without materialising `other`
 * or the concatenation.  Same workspace as relpose_warp. */
int relpose_warp_pairs(float* x, const double* pose, void* workspace, int32_t n, int32_t h, int32_t dataset, void* stream);
/* The same with flags.  RELPOSE_WARP_KEYS_CLEAN: the first 4 n h 4h bytes of the workspace (the per-pixel winner keys of the scatter
 * pass) are all zeros -- true for a workspace that was zero-initialised once and has only been used by relpose_warp / relpose_warp_pairs*
 * since: every call resets the keys it consumed.  The 26 MB memset in front of the scatter pass (64 panoramas) is then skipped. */
enum { RELPOSE_WARP_KEYS_CLEAN = 1 };
int relpose_warp_pairs2(float* x, const double* pose, void* workspace, int32_t n, int32_t h, int32_t dataset, int32_t flags, void* stream);

/* np.linalg.inv of n 4x4 poses (evaluation.py:235). */
int relpose_pose_inverse(const double* pose, double* inv, int32_t n, void* stream);

/* evaluation.py:246-253 + getMatchingPrimitive after keypoint detection (rpmodule.py:526-532):
 * compose completed normal/depth, bilinear-sample them at the keypoints (rputil.getPixel :88-119),
 * unproject, and gather 32-d descriptors (rputil.interpolate :43-58).
 *   f        [n, cf, h, 4h]  network output; normal = ch 3:6, depth = ch 6, feat = ch feat_off:feat_off+32
 *   obs_norm [n,3,h,4h], obs_depth [n,h,4h]  the complete input scan (evaluation.py:248-253)
 *   pts      [n, npts_max, 2] f64 pixel coords (x,y), x<=4h-2, y<=h-2 ; npts [n]
 *   compose  RELPOSE_COMPOSE_EVAL: normal / (|obs normal| + 1e-6)   evaluation.py:250-251
 *            RELPOSE_COMPOSE_LIB : normal / (|normal| + 1e-12)      rpmodule.py:633-634 (RelativePoseEstimationViaCompletion)
 *   outputs  pc [n,npts_max,3] f64, normal [n,npts_max,3] f64, feat [n,npts_max,32] f32 */
int relpose_sample_primitives(const float* f, int32_t cf, int32_t feat_off,
                              const float* obs_norm, const float* obs_depth,
                              const double* pts, const int32_t* npts, int32_t npts_max,
                              double* pc, double* normal, float* feat,
                              int32_t n, int32_t h, int32_t mask_method, int32_t compose, int32_t dataset, void* stream);

/* The same two samplers on caller-composed maps, for the reference-named host shims:
 * rputil.getPixel (rputil.py:88-119, incl. getPixel_helper :61-86): depth [h,4h] f64, normal [h,4h,3] f64 (HWC),
 * pts [k,2] f64 pixel coords -> pc [k,3] f64 (the reference returns the transpose), nn [k,3] f64 (renormalised, not rotated). */
int relpose_get_pixel(const double* depth, const double* normal, const double* pts, int32_t k, int32_t h, int32_t dataset,
                      double* pc, double* nn, void* stream);
/* rputil.interpolate (rputil.py:43-58): feat [c,h,w] f32, pt [k,2] f32 normalised to [0,1] -> out [c,k] f32. */
int relpose_interpolate(const float* feat, const float* pt, float* out, int32_t c, int32_t h, int32_t w, int32_t k, void* stream);

/* ------------------------------------------------- evaluation-side statistics
 * util.depth2pc (util.py:468-523) of the observed block of each panorama (the face / kinect crop that
 * util.parse_data :42-92 feeds it): pc [n, P, 3] f64 in pixel order, valid [n, P] = depth != 0, with
 * P = relpose_observed_points(h, dataset) (25600 or 66*88 at h = 160). */
int32_t relpose_observed_points(int32_t h, int32_t dataset);
int relpose_depth2pc(const float* depth, double* pc, uint8_t* valid, int32_t n, int32_t h, int32_t dataset, void* stream);
/* util.depth2pc's full-resolution kinect branch (util.py:497-507, reached from util.parse_data :79-90 for the baseline methods on
 * ScanNet): depth [n, 480, 640] f32 IMAGES (no panorama around them) -> pc [n, 480*640, 3] f64 in pixel order, valid = depth != 0.
 * The reference defines the branch for this one shape; any other returns RELPOSE_EINVAL (round 6). */
int relpose_depth2pc_full(const float* depth, double* pc, uint8_t* valid, int32_t n, int32_t hh, int32_t ww, void* stream);

/* Nearest-neighbour distances behind util.point_cloud_overlap (util.py:21-40, sklearn KDTree there):
 * dist[i] = min_j || pose*query_i - ref_j || over valid ref points (pose [12+] row-major 3x4/4x4, or NULL);
 * invalid query points get -1.  query [nq,3], ref [nr,3] f64. */
int relpose_nn_dist(const double* query, const uint8_t* query_valid, int32_t nq, const double* ref, const uint8_t* ref_valid,
                    int32_t nr, const double* pose, double* dist, void* stream);

/* ------------------------------------ feature-guided keypoint augmentation
 * rputil.getKeypoint :182-190: dist [nsel,H,W] f32 = sum_c (query[s][c] - feat[c][y][x])^2
 * (query [nsel,32] = descriptors of the selected keypoints, feat [32,H,W] the other view's feature map). */
int relpose_feature_distance_map(const float* query, const float* feat, float* dist, int32_t nsel, int32_t H, int32_t W, void* stream);
/* rputil.Sampling :355-371 on exp(-dist/2): K x {argmax, suppress a +-window box}; pts [nmaps,K,2] f64 (x,y). */
int relpose_nms_sampling(const float* dist, double* pts, int32_t nmaps, int32_t H, int32_t W, int32_t K, int32_t window, void* stream);

/* The per-level keypoint derivation of the reference behind its SIFT detector, batched over the views of a batch of scan pairs
 * (rputil.getKeypoint :141-237 / getKeypoint_kinect :240-353, called at every recurrent level through getMatchingPrimitive,
 * rpmodule.py:511-533, evaluation.py:278): descriptors at the query points (interpolate :43-58), for every query the `topk`
 * non-maximum-suppressed minima of its squared descriptor distance over the OTHER view's 32-channel feature map (:182-190, :212-214,
 * Sampling :355-371) -- the [n,H,W] distance maps are never materialised --, the validity filter (:192-196), concatenation and the
 * weights 1 / 0.99 (:226-235).  The np.random draws of getKeypoint do not depend on the features: the host pre-draws them in the
 * reference's call order (relativepose_amd.rputil.keypoint_plan) and passes
 *   f [n_views, ., H, W] the network output (features = channels feat_off .. feat_off+32 of every image; image_stride floats per image)
 *   q_src_view [nq] image whose features a query samples, q_pt [nq,2] its normalised (x/W, y/H) float32 point,
 *   q_map_view [nq] the view whose map it searches, queries grouped by that view: q_off [n_views+1]; nq_view_max = max group size
 *   slot_kind [n_views,L]: the keypoint slots of every view in the reference's concatenation order: -1 empty, -2 a host coordinate
 *   (slot_xy [n_views,L,2]: SIFT detections, random points), >= 0 the pick with linear index query * topk + k
 * Outputs: pts [n_views,L,2] f64 pixel coordinates (x,y) compacted in slot order, weight [n_views,L] f64, npts [n_views].
 * flags: RELPOSE_KP_OBSERVED_ONLY = getMatchingPrimitive(..., doCompletion = 0), rpmodule.py:534-537 (the 'ours_nc' method, evaluation.py:74): only
 * the keypoints of weight 1 (inside the observed region) are kept -- the reference filters the sampled primitives by ptsW == 1, which is the same
 * selection in the same order.  nq = 0 is legal (round 6): a batch whose views have no SIFT detections has no queries; a view whose slots are
 * all empty gets npts = 0 and its pair the matcher's "return identity" status, like the reference (rputil.py:156-166, rpmodule.py:522-523,
 * evaluation.py:280-282).  nq_view_max <= RELPOSE_KP_MAX_QUERIES_PER_VIEW (the per-view query descriptors and running bests live in LDS). */
enum { RELPOSE_KP_OBSERVED_ONLY = 1 };
#define RELPOSE_KP_MAX_QUERIES_PER_VIEW 1000
size_t relpose_keypoints_reference_workspace_bytes(int32_t nq, int32_t H, int32_t W, int32_t topk);
int relpose_keypoints_reference(const float* f, int64_t image_stride, int32_t feat_off, int32_t n_views, int32_t H, int32_t W,
                                const int32_t* q_src_view, const float* q_pt, const int32_t* q_map_view, const int32_t* q_off, int32_t nq,
                                int32_t nq_view_max, int32_t topk, int32_t window, const int32_t* slot_kind, const double* slot_xy, int32_t L,
                                int32_t mask_method, int32_t flags, double* pts, double* weight, int32_t* npts, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ------------------------------------------------------------------ SIFT detector
 * The keypoint detector every recurrent level of the reference starts from: cv2.xfeatures2d.SIFT_create(contrastThreshold=0.02)
 * .detectAndCompute on the observed face (SUNCG / Matterport, rputil.py:152-172) or on the 640x480 frame (ScanNet, :253-265); only the
 * positions kp.pt are used.  Lowe's scale space with the reference's parameters (3 layers per octave, contrast 0.02, edge 10, sigma 1.6,
 * image doubled first), batched over views; the detection contract (blur, refinement, orientations, output order) is DESIGN.md's
 * "SIFT detector" section.  Descriptors are not computed (the reference discards them).
 *   images       uint8, channels == 3: [n_views, img_h, img_w, 3] in cv2's BGR order (channel 0 weighted as B, cv2.COLOR_BGR2GRAY's
 *                14-bit fixed-point weights, rputil.bgr2gray); channels == 1: gray [n_views, img_h, img_w]
 *   crop_*       the rectangle the detector sees (like grays[:, H:2H]); coordinates come back in that rectangle's frame, like kp.pt;
 *                16 <= crop_w, crop_h <= RELPOSE_SIFT_MAX_SIDE
 *   xy           [n_views, max_kp, 2] f32 positions, per view sorted by (x, y, size desc, angle, response desc), exact
 *                (x, y, size, angle) duplicates removed; a position repeats once per dominant orientation, like cv2
 *   size, angle  optional (NULL) [n_views, max_kp] f32: the keypoint diameter and orientation in degrees [0, 360)
 *   gray         optional (NULL) [n_views, crop_h, crop_w] uint8: the crop converted to gray (what the detector sees)
 *   count        [n_views] i32: keypoints found per view
 * Overflow: when a view has more than max_kp keypoints, count holds the true total, nothing is written past max_kp and the call returns
 * RELPOSE_SIFT_OVERFLOW.  The per-view intermediate lists hold relpose_sift_stage_capacity(max_kp) entries; if one of them fills up, the
 * call also returns RELPOSE_SIFT_OVERFLOW and count is then a lower bound.
 * This entry point SYNCHRONISES `stream` once at its end (to read the overflow flag).  The number of kernel launches does not depend on
 * n_views.  workspace: relpose_sift_workspace_bytes(n_views, crop_h, crop_w, max_kp) (0 for invalid sizes). */
#define RELPOSE_SIFT_OVERFLOW (-3)
#define RELPOSE_SIFT_MAX_SIDE 2048
typedef struct RelposeSiftArgs {
    uint32_t struct_size;       /* sizeof(RelposeSiftArgs) as the caller compiled it */
    int32_t n_views;
    const uint8_t* images;
    int32_t img_h, img_w, channels;
    int32_t crop_x, crop_y, crop_w, crop_h;
    int32_t max_kp;
    float* xy;
    float* size;
    float* angle;
    uint8_t* gray;
    int32_t* count;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeSiftArgs;
size_t relpose_sift_workspace_bytes(int32_t n_views, int32_t h, int32_t w, int32_t max_kp);
int32_t relpose_sift_stage_capacity(int32_t max_kp);
int relpose_sift_detect(const RelposeSiftArgs* args);

/* ------------------------------------------------------------------ FPFH + fast global registration
 * The reference's `--method fgs` baseline, open3d_fast_global_registration (baselines.py:83-106, preprocess_point_cloud :36-50): voxel
 * 0.05 downsample, normals (r 0.10, max_nn 30), FPFH (r 0.25, max_nn 100), mutual fp32 feature matches, the tuple test (0.95, <= 1000
 * tuples) and 64 Gauss-Newton steps of FGR (division factor 1.4, max correspondence distance 0.075), batched over pairs.  The contract
 * (orders, bins, tie rules, the tuple draws) is DESIGN.md §4.6; it is this project's own and not checked against Open3D.
 *   pc, valid    [2 n_pairs, n_points, 3] f64 and [2 n_pairs, n_points] u8 (relpose_depth2pc's layout): cloud 2b = the source of pair b,
 *                2b + 1 its target; the sensor sits at the origin of each cloud's frame (normals are turned toward it)
 *   max_points   voxels kept per cloud, 1 .. RELPOSE_FGR_MAX_POINTS_LIMIT (RELPOSE_FGR_MAX_POINTS is the default the wrappers use)
 *   seed         the tuple draws: splitmix64(seed * 0x9E3779B97F4A7C15 + 3 t + k) mod (mutual matches), the same for every pair
 *   pose         [n_pairs, 4, 4] f64, T p_src ~ p_tgt (the convention of R_gt_44); identity unless status == 0
 *   status       [n_pairs] i32 RELPOSE_FGR_STATUS_*
 * Optional per-stage outputs (NULL = kept in the workspace), rows past a cloud's count are left unwritten:
 *   down_points [2 n_pairs, max_points, 3] f64 and down_count [2 n_pairs] i32 (the TRUE voxel count, also above max_points),
 *   nbr_index [2 n_pairs, max_points, 100] i32 and nbr_count [2 n_pairs, max_points] i32 (the r 0.25 lists, (d2, index) order),
 *   normals [2 n_pairs, max_points, 3] f64, fpfh [2 n_pairs, max_points, 33] f64,
 *   corr [n_pairs, max_points, 2] i32 and n_corr [n_pairs] (mutual matches, ascending source index),
 *   tuple_corr [n_pairs, 3 * 1000, 2] i32 and n_tuples [n_pairs] (the accepted tuples, 3 matches each: what FGR optimises over).
 * Overflow: a cloud with more than max_points voxels gets its pair status RELPOSE_FGR_STATUS_OVERFLOW, nothing is written past max_points
 * and the call returns RELPOSE_FGR_OVERFLOW (the other pairs are complete).  This entry point SYNCHRONISES `stream` once at its end.  The
 * number of kernel launches does not depend on n_pairs.  workspace: relpose_fgr_workspace_bytes(n_pairs, n_points, max_points). */
#define RELPOSE_FGR_OVERFLOW (-4)
#define RELPOSE_FGR_MAX_POINTS 32768
#define RELPOSE_FGR_MAX_POINTS_LIMIT 65536
enum { RELPOSE_FGR_STATUS_OK = 0, RELPOSE_FGR_STATUS_FEW_POINTS = 1, RELPOSE_FGR_STATUS_FEW_CORR = 2, RELPOSE_FGR_STATUS_OVERFLOW = 3 };
typedef struct RelposeFgrArgs {
    uint32_t struct_size;       /* sizeof(RelposeFgrArgs) as the caller compiled it */
    int32_t n_pairs;
    int32_t n_points;
    int32_t max_points;
    const double* pc;
    const uint8_t* valid;
    uint64_t seed;
    double* pose;
    int32_t* status;
    double* down_points;
    int32_t* down_count;
    int32_t* nbr_index;
    int32_t* nbr_count;
    double* normals;
    double* fpfh;
    int32_t* corr;
    int32_t* n_corr;
    int32_t* tuple_corr;
    int32_t* n_tuples;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeFgrArgs;
size_t relpose_fgr_workspace_bytes(int32_t n_pairs, int32_t n_points, int32_t max_points);
int relpose_fgr(const RelposeFgrArgs* args);

/* ------------------------------------------------------------------ RANSAC feature registration
 * The reference's `--method gs` baseline, open3d_global_registration (baselines.py:52-81): the front end of relpose_fgr (voxel 0.05,
 * normals, FPFH; the exact fp32 feature nearest neighbour from source to target, one correspondence per source voxel), then RANSAC over
 * those correspondences as registration_ransac_based_on_feature_matching(..., 0.075, point-to-point, 4, [EdgeLength(0.9), Distance(0.075)],
 * RANSACConvergenceCriteria(4000000, 500)) reads: 4-point hypotheses, the first max_validations that pass both checkers validated in
 * iteration order, the best by (inlier count, then smaller rmse).  The contract (draws, orders, reductions) is DESIGN.md §4.7; it is this
 * project's own and not checked against Open3D.
 *   pc, valid        as relpose_fgr (cloud 2b = the source of pair b, 2b + 1 its target)
 *   max_points       voxels kept per cloud, 1 .. RELPOSE_FGR_MAX_POINTS_LIMIT
 *   seed             draw k of iteration t: splitmix64(seed * 0x9E3779B97F4A7C15 + 4 t + k) mod (source voxels)
 *   max_iterations   0 = 4000000; at most RELPOSE_RANSAC_MAX_ITERATIONS_LIMIT
 *   max_validations  0 = 500; at most RELPOSE_RANSAC_MAX_VALIDATIONS_LIMIT
 *   pose             [n_pairs, 4, 4] f64, T p_src ~ p_tgt (the convention of R_gt_44); identity unless status == 0
 *   status           [n_pairs] i32 RELPOSE_RANSAC_STATUS_*
 * Optional per-pair outputs (NULL = not written): fitness [n_pairs] f64 (inliers / source voxels), inlier_rmse [n_pairs] f64,
 *   n_iterations, n_validations, best_index [n_pairs] i32 (best_index: the slot of the chosen hypothesis in the validated set, -1 if none).
 * Optional stage outputs (NULL = kept in the workspace), rows past a count are left unwritten:
 *   down_points [2 n_pairs, max_points, 3] f64 and down_count [2 n_pairs] i32 (the true voxel count), fpfh [2 n_pairs, max_points, 33] f64,
 *   nn [n_pairs, max_points] i32 (the source voxels' nearest target feature), val_iter, val_inliers [n_pairs, max_validations] i32 and
 *   val_err [n_pairs, max_validations] f64 (the validated iterations in order, their inlier counts and inlier rmse).
 * Overflow: as relpose_fgr (status RELPOSE_RANSAC_STATUS_OVERFLOW, the call returns RELPOSE_RANSAC_OVERFLOW, other pairs complete).  This
 * entry point SYNCHRONISES `stream` once at its end.  The number of kernel launches depends on max_iterations only.
 * workspace: relpose_ransac_workspace_bytes(n_pairs, n_points, max_points, max_iterations, max_validations) (0 = the defaults). */
#define RELPOSE_RANSAC_OVERFLOW (-5)
#define RELPOSE_RANSAC_MAX_ITERATIONS 4000000
#define RELPOSE_RANSAC_MAX_VALIDATIONS 500
#define RELPOSE_RANSAC_MAX_ITERATIONS_LIMIT 16777216
#define RELPOSE_RANSAC_MAX_VALIDATIONS_LIMIT 4096
enum { RELPOSE_RANSAC_STATUS_OK = 0, RELPOSE_RANSAC_STATUS_FEW_POINTS = 1, RELPOSE_RANSAC_STATUS_OVERFLOW = 3, RELPOSE_RANSAC_STATUS_NO_HYPOTHESIS = 4 };
typedef struct RelposeRansacArgs {
    uint32_t struct_size;       /* sizeof(RelposeRansacArgs) as the caller compiled it */
    int32_t n_pairs;
    int32_t n_points;
    int32_t max_points;
    const double* pc;
    const uint8_t* valid;
    uint64_t seed;
    int32_t max_iterations;
    int32_t max_validations;
    double* pose;
    int32_t* status;
    double* fitness;
    double* inlier_rmse;
    int32_t* n_iterations;
    int32_t* n_validations;
    int32_t* best_index;
    double* down_points;
    int32_t* down_count;
    double* fpfh;
    int32_t* nn;
    int32_t* val_iter;
    int32_t* val_inliers;
    double* val_err;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeRansacArgs;
size_t relpose_ransac_workspace_bytes(int32_t n_pairs, int32_t n_points, int32_t max_points, int32_t max_iterations, int32_t max_validations);
int relpose_ransac(const RelposeRansacArgs* args);

/* -------------------------------------------------------------------- coloured ICP (the `cgs` baseline's refinement)
 * Replaces the three registration_colored_icp levels of open3d_color_registration (baselines.py:110-168; Park, Zhou, Koltun, "Colored
 * Point Cloud Registration Revisited", ICCV 2017) for a batch of pairs: per level (radius 0.04, 0.02, 0.01 with at most 50, 30, 14
 * iterations) a coloured voxel grid of both clouds, normals and colour gradients of the target, then Gauss-Newton on the joint
 * geometric + photometric objective from the previous level's pose, with ICPConvergenceCriteria(1e-6, 1e-6, max_iteration)'s stopping
 * rule evaluated on the device.  The reference starts it from its RANSAC result (relpose_ransac); any initial pose may be passed.
 * The contract is DESIGN.md 4.8 (the project's own; Open3D is not a dependency).
 *   pc, valid        as relpose_fgr (cloud 2b = the source of pair b, 2b + 1 its target)
 *   color            [2 n_pairs, n_points, 3] f64, the colour of every point (rows with valid == 0 are ignored)
 *   init             [n_pairs, 4, 4] f64 starting transform (T p_src ~ p_tgt), NULL = the identity
 *   lambda_geometric weight of the geometric term, 0 .. 1, taken as given (RELPOSE_CICP_LAMBDA_GEOMETRIC = Open3D's default 0.968)
 *   max_points       voxels kept per cloud and level, 1 .. RELPOSE_FGR_MAX_POINTS_LIMIT
 *   pose             [n_pairs, 4, 4] f64, T p_src ~ p_tgt; the identity unless status == 0
 *   status           [n_pairs] i32 RELPOSE_CICP_STATUS_* (too few points: a cloud with fewer than 3 voxels at some level)
 * Optional per-level outputs (NULL = not written): fitness, inlier_rmse [n_pairs, 3] f64 and n_iterations [n_pairs, 3] i32 (the last
 *   evaluation of the level and the number of evaluations it made), level_pose [n_pairs, 3, 4, 4] f64 (the pose the level ended with).
 * Optional stage outputs (NULL = kept in the workspace or not kept), rows past a count and trace slots that were not evaluated are left
 * unwritten: down_points, down_colors [2 n_pairs, 3, max_points, 3] f64 and down_count [2 n_pairs, 3] i32 (the true voxel count);
 *   normals, gradient [n_pairs, 3, max_points, 3] f64 (the target's); and the trace over the RELPOSE_CICP_TRACE_SLOTS = 50 + 30 + 14
 *   iteration slots (level l, iteration k -> slot {0, 50, 80}[l] + k): iter_pose [n_pairs, 94, 4, 4] f64 (the transform the evaluation
 *   used), iter_ncorr [n_pairs, 94] i32, iter_rmse [n_pairs, 94] f64, iter_corr [n_pairs, 94, max_points] i32 (the target voxel of every
 *   source voxel, -1 = none) and iter_x [n_pairs, 94, 6] f64 (the step; unwritten where the level ended without one).
 * Overflow: as relpose_fgr, at any level (status RELPOSE_CICP_STATUS_OVERFLOW, the call returns RELPOSE_CICP_OVERFLOW, other pairs
 * complete).  This entry point SYNCHRONISES `stream` once at its end; nothing inside the iteration loop waits for the device.  The number
 * of kernel launches is fixed (4 + 2 x 94).  workspace: relpose_cicp_workspace_bytes(n_pairs, n_points, max_points). */
#define RELPOSE_CICP_OVERFLOW (-6)
#define RELPOSE_CICP_LEVELS 3
#define RELPOSE_CICP_TRACE_SLOTS 94
#define RELPOSE_CICP_LAMBDA_GEOMETRIC 0.968
enum { RELPOSE_CICP_STATUS_OK = 0, RELPOSE_CICP_STATUS_FEW_POINTS = 1, RELPOSE_CICP_STATUS_OVERFLOW = 3 };
typedef struct RelposeCicpArgs {
    uint32_t struct_size;       /* sizeof(RelposeCicpArgs) as the caller compiled it */
    int32_t n_pairs;
    int32_t n_points;
    int32_t max_points;
    const double* pc;
    const uint8_t* valid;
    const double* color;
    const double* init;
    double lambda_geometric;
    double* pose;
    int32_t* status;
    double* fitness;
    double* inlier_rmse;
    int32_t* n_iterations;
    double* level_pose;
    double* down_points;
    double* down_colors;
    int32_t* down_count;
    double* normals;
    double* gradient;
    double* iter_pose;
    int32_t* iter_ncorr;
    double* iter_rmse;
    int32_t* iter_corr;
    double* iter_x;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeCicpArgs;
size_t relpose_cicp_workspace_bytes(int32_t n_pairs, int32_t n_points, int32_t max_points);
int relpose_cicp(const RelposeCicpArgs* args);

/* -------------------------------------------------------------------- descriptor evaluation
 * The reference's feature-quality metric for a batch of panorama pairs: dense ground-truth correspondences between the two clouds
 * (datasets/SUNCG.py:315-341), their observed / unobserved class (mainPanoCompletion2view.py:535-542) and, per correspondence, the
 * number of target pixels whose descriptor lies closer to the source descriptor than the true match does (evalDLDescriptor,
 * mainPanoCompletion2view.py:383-414).  The contract is DESIGN.md 4.9; both entry points only enqueue on `stream`.
 *
 * relpose_dense_nn: the batched nearest neighbour with index behind the KDTree query of datasets/SUNCG.py:323-332.
 *   pc, valid        [2 n_pairs, 3, n_points] f64 and [2 n_pairs, n_points] u8 as relpose_pano2pc writes them (cloud 2b = the source of
 *                    pair b, 2b + 1 its target); n_points = 4 h h
 *   to_world         [2 n_pairs, 4, 4] f64, applied to every cloud: w_a = ((M_a0 x + M_a1 y) + M_a2 z) + M_a3
 *   query            [n_pairs, n_query] i32 point indices into the source cloud, -1 = an unused slot
 *   max_dist         0 = 0.08 (datasets/SUNCG.py:328)
 *   nn_index         [n_pairs, n_query] i32: the valid target point with the smallest d2 = (dx dx + dy dy) + dz dz, d = target - query;
 *                    ties go to the lowest index
 *   nn_dist          [n_pairs, n_query] f64 = sqrt(d2);  hit [n_pairs, n_query] u8 = nn_dist < max_dist
 *   idx_src, idx_tgt [n_pairs, n_query, 2] i32: the (x, y) panorama pixel of the query and of its neighbour (PanoIdx,
 *                    datasets/SUNCG.py:164-174)
 * An unused slot, a query whose source point is invalid and a pair whose target has no valid point (none with a d2 below +inf) give
 * nn_index -1, nn_dist -1, hit 0 and pixels 0. */
typedef struct RelposeDenseNnArgs {
    uint32_t struct_size;       /* sizeof(RelposeDenseNnArgs) as the caller compiled it */
    int32_t n_pairs;
    int32_t n_points;
    int32_t n_query;
    int32_t h;
    int32_t reserved0;
    const double* pc;
    const uint8_t* valid;
    const double* to_world;
    const int32_t* query;
    double max_dist;
    int32_t* nn_index;
    double* nn_dist;
    uint8_t* hit;
    int32_t* idx_src;
    int32_t* idx_tgt;
    void* stream;
} RelposeDenseNnArgs;
int relpose_dense_nn(const RelposeDenseNnArgs* args);

/* relpose_descriptor_rank: the counts behind evalDLDescriptor's ratio (mainPanoCompletion2view.py:401-405).
 *   f                [2 n_pairs, total_channels, h, 4h] f32, the network output, read in place (8-byte aligned); the descriptor is
 *                    channels feat_off .. feat_off + n_channels - 1, 1 <= n_channels <= RELPOSE_DESC_MAX_CHANNELS
 *   idx_src, idx_tgt [n_pairs, n_corres, 2] i32 (x, y) pixels in image 2b and 2b + 1
 *   sel              [n_pairs, n_slots] i32 indices into n_corres, -1 = unused; NULL = every correspondence (n_slots is ignored and
 *                    the outputs have n_corres slots)
 *   pair_valid       [n_pairs] u8 or NULL (all valid)
 *   mask             [2 n_pairs, h, 4h] f32 or NULL, nonzero = observed (what relpose_apply_mask returns)
 *   thr              [n_pairs, n_slots] f32 = sum_c (f[2b, off + c, y_s, x_s] - f[2b + 1, off + c, y_t, x_t])^2, accumulated in fp32 from 0
 *                    with c ascending as acc = acc + d * d (no fused multiply-add)
 *   count            [n_pairs, n_slots] i32 = #{target pixels p : d_p < thr}, d_p the same expression at pixel p of image 2b + 1 (the
 *                    true match has d_p == thr bit for bit and is never counted); -1 for an unused slot, a slot whose pixels lie
 *                    outside the map and every slot of a pair with pair_valid 0
 *   type             [n_pairs, n_slots] i32 = (mask at the source pixel != 0) + (mask at the target pixel != 0); -1 without a mask or
 *                    where count is -1 */
#define RELPOSE_DESC_MAX_CHANNELS 64
typedef struct RelposeDescRankArgs {
    uint32_t struct_size;       /* sizeof(RelposeDescRankArgs) as the caller compiled it */
    int32_t n_pairs;
    int32_t h;
    int32_t total_channels;
    int32_t feat_off;
    int32_t n_channels;
    int32_t n_corres;
    int32_t n_slots;
    const float* f;
    const int32_t* idx_src;
    const int32_t* idx_tgt;
    const int32_t* sel;
    const uint8_t* pair_valid;
    const float* mask;
    int32_t* count;
    float* thr;
    int32_t* type;
    void* stream;
} RelposeDescRankArgs;
int relpose_descriptor_rank(const RelposeDescRankArgs* args);

/* -------------------------------------------------------------------- SIFT descriptors and the SIFT baseline of the descriptor metric
 * evalSiftDescriptor (mainPanoCompletion2view.py:353-381, the 'sift' curve of evalPlot, :342): SIFT descriptors of the sampled
 * correspondences in both panoramas and of a step-5 grid of the target (cv2.xfeatures2d.SIFT_create().compute(gray, keypoints) with
 * cv2.KeyPoint(x, y, 5), :365-377), then the share of grid descriptors that lie closer to the source descriptor than the true match does
 * (:373, :378-379).  The descriptor contract is DESIGN.md 4.10.  It is the project's own, written from Lowe (IJCV 60(2), 2004) with the
 * parameters of that call; cv2 is not a dependency and agreement with cv2's descriptors is UNTESTED.  Keypoints are on octave 0, layer 0
 * (what cv2.KeyPoint(x, y, size) gives); descriptors for relpose_sift_detect's own keypoints (other octaves) are out of scope.
 * Both entry points only enqueue on `stream`; invalid arguments return RELPOSE_EINVAL before anything is enqueued.
 *
 * relpose_sift_describe: 128-byte descriptors of given keypoints in n_views images (mainPanoCompletion2view.py:361-371, :375-377).
 *   images, img_h, img_w, channels, crop_*   as relpose_sift_detect (uint8 BGR or gray, cv2's 14-bit gray weights); 1 <= crop side <=
 *                    RELPOSE_SIFT_MAX_SIDE
 *   kp               [n_views, n_kp, 4] f32 (x, y, size, angle in degrees; cv2.KeyPoint's default angle is -1) in the crop's frame
 *   kp_count         [n_views] i32 or NULL (all n_kp): slots at or past a view's count are unused
 *   grid_step        > 0: dense grid mode -- kp and kp_count must be NULL and n_kp = ceil(crop_w / step) * ceil(crop_h / step); keypoint
 *                    k is x = (k mod nx) step, y = (k / nx) step, size = step, angle = -1, generated on the device (:375-376)
 *   desc             [n_views, n_kp, 128] u8, bin order (row * 4 + col) * 8 + orientation; may be NULL when n_kp = 0
 *   desc_f32         [n_views, n_kp, 128] f32 or NULL: the values before rounding (desc = clamp(round_half_even(desc_f32), 0, 255))
 *   base             [n_views, crop_h, crop_w] f32 or NULL: the blurred gray image the gradients are taken on
 *   workspace        relpose_sift_describe_workspace_bytes(n_views, crop_h, crop_w); not needed (may be NULL) when `base` is given
 * An unused slot (past the count, a non-finite coordinate, size or angle, size <= 0) reads zeros.  Two launches, whatever n_views is.
 * The sum into every bin runs in an order fixed by the keypoint alone: results do not depend on the batch, the slot or the run. */
typedef struct RelposeSiftDescArgs {
    uint32_t struct_size;       /* sizeof(RelposeSiftDescArgs) as the caller compiled it */
    int32_t n_views;
    const uint8_t* images;
    int32_t img_h, img_w, channels;
    int32_t crop_x, crop_y, crop_w, crop_h;
    int32_t n_kp;
    int32_t grid_step;
    int32_t reserved0;
    const float* kp;
    const int32_t* kp_count;
    uint8_t* desc;
    float* desc_f32;
    float* base;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeSiftDescArgs;
size_t relpose_sift_describe_workspace_bytes(int32_t n_views, int32_t h, int32_t w);
int relpose_sift_describe(const RelposeSiftDescArgs* args);

/* relpose_sift_rank: the counts behind evalSiftDescriptor's ratio (mainPanoCompletion2view.py:373, :378-379), in integers.
 *   src, tgt         [n_pairs, n_slots, 128] u8 (16-byte aligned): the descriptors of the correspondences in the source and the target
 *   dense            [n_pairs, n_points, 128] u8 (16-byte aligned): the target's grid descriptors
 *   pair_valid       [n_pairs] u8 or NULL (all valid)
 *   thr              [n_pairs, n_slots] i32 = sum_k (src - tgt)^2
 *   count            [n_pairs, n_slots] i32 = #{p : sum_k (src[b, e] - dense[b, p])^2 < thr[b, e]} (a tie is not counted)
 * thr and count are -1 for every slot of a pair with pair_valid 0.  All arithmetic is integer (the products on the int8 matrix pipe), so
 * the counts are exact; the reference's float32 expression is exact on these values too (128 * 255^2 < 2^24). */
typedef struct RelposeSiftRankArgs {
    uint32_t struct_size;       /* sizeof(RelposeSiftRankArgs) as the caller compiled it */
    int32_t n_pairs;
    int32_t n_slots;
    int32_t n_points;
    const uint8_t* src;
    const uint8_t* tgt;
    const uint8_t* dense;
    const uint8_t* pair_valid;
    int32_t* thr;
    int32_t* count;
    void* stream;
} RelposeSiftRankArgs;
int relpose_sift_rank(const RelposeSiftRankArgs* args);

/* -------------------------------------------------------------------- completion quality: the losses of the reference's validation pass
 * learner.step(mode='val') (mainPanoCompletion2view.py:457-602) measures the completion with dataMask-weighted L1 on rgb / normal / depth
 * (:553-561), cross-entropy x 0.1 on the semantic head (:565-567) and the contrastive descriptor loss (contrast_loss, :429-455).  Forward
 * only.  The contract is DESIGN.md 4.11; both entry points only enqueue on `stream`, and invalid arguments return RELPOSE_EINVAL before
 * anything is enqueued.  All sums are float64 in a fixed order without floating-point atomics: repeatable bit for bit.
 *
 * relpose_completion_loss: one pass over the network output (mainPanoCompletion2view.py:549-567).
 *   f                [n_images, total_channels, H, W] f32, the network output in the 'rgbdnsf' layout (rgb 0:3, normal 3:6, depth 6,
 *                    semantic logits 7 : 7 + n_classes), read in place; channels >= 7 + n_classes are never read.  H W must be a
 *                    multiple of 4 and f, complete, mask, weight 16-byte aligned (label: 4-byte)
 *   complete         [n_images, 7, H, W] f32: rgb 0:3, normal 3:6, depth 6 (:484-485, :513)
 *   label            [n_images, H, W] u8 or NULL (no cross-entropy: its rows, ce_mag, ce_cross and n_bad_label are 0)
 *   mask             [n_images, H, W] f32, what relpose_apply_mask returns: region 1 = mask != 0 (observed), region 0 = unobserved
 *   weight           [n_images, H, W] f32 or NULL (= 1): the caller's geometric / dynamic weighting (:549-552)
 *   w(i, p)          = (complete[i, 6, p] != 0 ? 1 : 0) * weight[i, p] in fp32 -- the loaders' dataMask is depth != 0
 *   L1 term          fabsf((f - complete) * w) in fp32: subtract, multiply, abs, never fused
 *   CE(i, p)         in float64 from the fp32 logits z: m = max_c z_c, lse = m + log(sum_c exp(z_c - m)) with c ascending,
 *                    CE = lse - z_label; class weights are all ones (:265).  A label >= n_classes has CE = 0 and is counted
 *   sums             [n_images, 5, 2] f64: rows rgb, n, d (the L1 terms summed over the row's channels), ce (sum CE w), w (sum w), each
 *                    split by region.  Row i depends on image i alone: it does not change with the batch around it
 *   ce_mag           [n_images] f64 = sum w (|lse| + |z_label|), the un-cancelled magnitude tolerances on the ce row are stated against
 *   ce_cross         [1] f64 or NULL = sum_p (sum_i CE_i(p)) (sum_j w_j(p)), i and j ascending: the reference multiplies a [N, H, W] loss
 *                    by a [N, 1, H, W] weight, which broadcasts to [N, N, H, W] (:566); errG_s = 0.1 ce_cross / (N N H W)
 *   n_bad_label      [n_images] i32 = #{p : label >= n_classes}
 *   workspace        relpose_completion_loss_workspace_bytes(n_images, H, W, ce_cross != NULL) bytes, 256-byte aligned */
typedef struct RelposeCompletionLossArgs {
    uint32_t struct_size;       /* sizeof(RelposeCompletionLossArgs) as the caller compiled it */
    int32_t n_images;
    int32_t H;
    int32_t W;
    int32_t total_channels;
    int32_t n_classes;
    const float* f;
    const float* complete;
    const uint8_t* label;
    const float* mask;
    const float* weight;
    double* sums;
    double* ce_mag;
    double* ce_cross;
    int32_t* n_bad_label;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeCompletionLossArgs;
size_t relpose_completion_loss_workspace_bytes(int32_t n_images, int32_t H, int32_t W, int32_t with_cross);
int relpose_completion_loss(const RelposeCompletionLossArgs* args);

/* relpose_contrast_loss: the sums behind contrast_loss (mainPanoCompletion2view.py:429-455), per pair.
 *   f, total_channels, feat_off, n_channels, h     as relpose_descriptor_rank (image 2b = the source of pair b, 2b + 1 its target)
 *   idx_src, idx_tgt [n_pairs, n_corres, 2] i32 (x, y) pixels, the layout relpose_dense_nn writes
 *   pair_valid       [n_pairs] u8 or NULL (all valid); a pair with pair_valid 0 yields zeros in all four outputs
 *   neg              [n_pairs, n_corres, n_neg, 2] i32 (x, y) pixels of the TARGET map (:449-453)
 *   margin           the reference's args.D (0.5), fp32
 *   d(a, b)          relpose_descriptor_rank's expression: fp32, from 0, c ascending, acc = acc + d * d, never fused
 *   pos_sum          [n_pairs] f64 = sum_k d(src_k, tgt_k) (:444)
 *   neg_sum          [n_pairs] f64 = sum_{k, m} fmaxf(margin - d(src_k, neg_km), 0), the hinge in fp32 (:453)
 *   n_active         [n_pairs] i32 = #{(k, m) : d(src_k, neg_km) < margin}, exact
 *   n_skipped        [n_pairs] i32: the positive slots k with a source or target pixel outside the map plus the negative slots (k, m)
 *                    with a source or negative pixel outside it; a skipped slot contributes nothing
 *   workspace        relpose_contrast_loss_workspace_bytes(n_pairs, n_corres) bytes, 256-byte aligned */
typedef struct RelposeContrastLossArgs {
    uint32_t struct_size;       /* sizeof(RelposeContrastLossArgs) as the caller compiled it */
    int32_t n_pairs;
    int32_t h;
    int32_t total_channels;
    int32_t feat_off;
    int32_t n_channels;
    int32_t n_corres;
    int32_t n_neg;
    float margin;
    int32_t reserved0;
    const float* f;
    const int32_t* idx_src;
    const int32_t* idx_tgt;
    const uint8_t* pair_valid;
    const int32_t* neg;
    double* pos_sum;
    double* neg_sum;
    int32_t* n_active;
    int32_t* n_skipped;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeContrastLossArgs;
size_t relpose_contrast_loss_workspace_bytes(int32_t n_pairs, int32_t n_corres);
int relpose_contrast_loss(const RelposeContrastLossArgs* args);

/* -------------------------------------------------------------------- normal maps from depth panoramas
 * The reference reads every view's normal map from disk (datasets/SUNCG.py:300-313); the tool that made those files was never published.
 * relpose_depth_normals estimates the map from the depth panorama alone, so that RGB-D panoramas enter the pair pipeline without one.
 * The contract is the project's own (tests/normals_model.py restates it in numpy).  One kernel launch, enqueued on
 * `stream`; no workspace; invalid arguments return RELPOSE_EINVAL before anything is enqueued.  All arithmetic is fp32, every operation
 * rounded on its own (no fused multiply-add), in the order written here, so count and moments are repeatable bit for bit and a view's
 * result does not depend on the batch around it.
 *
 *   depth            [n_views, h, 4h] f32, 0 = no data
 *   dataset          RELPOSE_SUNCG / _MATTERPORT / _SCANNET: which face rotation a column block has
 *   radius           r in 1..4: the window is (2r+1)^2 pixels; h >= 2r+1
 *   gate_scale       finite, > 0 (3.0 is the library's default)
 *   min_neighbors    3 .. (2r+1)^2 - 1 (6 is the library's default)
 *   P(x, y)          the point of pixel (x, y), x in 0..4h-1: slot = x / h, xf = x - slot h, z = depth,
 *                    xn = ((float)xf / (float)h - 0.5f) * 2.0f, yn = (0.5f - (float)y / (float)h) * 2.0f, face point (xn z, yn z, -z),
 *                    rotated by the face rotation Rs[slot] (suncg) / Rs[(slot - 1) % 4] (matterport, scannet): a signed permutation,
 *                    exact.  The frame is relpose_pano2pc's (without its scannet focal scaling) and the one relpose_warp rotates normals in
 *   window           columns wrap around the ring of four faces (column 4h-1 is next to column 0, windows cross the face seams: consecutive
 *                    slots are consecutive quarter turns about the vertical axis and share the ray of their common edge); rows do not
 *                    wrap, rows outside 0..h-1 contribute nothing
 *   acceptance       neighbour q of centre p is used when depth_q != 0, depth_p != 0 and d2 <= g2, with d = P_q - P_p componentwise,
 *                    d2 = d.x d.x + d.y d.y + d.z d.z left to right, g = gate_scale * (float)r * (2.0f / (float)h) * depth_p left to right,
 *                    g2 = g g: the gate keeps a window from mixing a foreground surface with what lies behind it
 *   count            [n_views, h, 4h] i32 or NULL: the number of accepted neighbours
 *   moments          [n_views, 9, h, 4h] f32 or NULL: sums over the accepted neighbours, visited dy ascending (outer), dx ascending (inner),
 *                    centre skipped, of d.x, d.y, d.z, d.x d.x, d.x d.y, d.x d.z, d.y d.y, d.y d.z, d.z d.z
 *   C                C_ab = S_ab - s_a s_b / m with m = (float)(count + 1) (the + 1 is the centre, whose d is 0), evaluated (s_a s_b) / m
 *   normal           [n_views, 3, h, 4h] f32: the eigenvector of C's smallest eigenvalue (six cyclic Jacobi sweeps in fp32), scaled to unit
 *                    length, negated when n . P_p > 0 so that it faces the sensor; (0, 0, 0) where valid is 0
 *   valid            [n_views, h, 4h] u8 or NULL: depth_p != 0 && count >= min_neighbors && l1 > 1e-6f l2 (l0 <= l1 <= l2 the eigenvalues:
 *                    the accepted neighbours are not collinear) */
typedef struct RelposeDepthNormalsArgs {
    uint32_t struct_size;       /* sizeof(RelposeDepthNormalsArgs) as the caller compiled it */
    int32_t n_views;
    int32_t h;
    int32_t dataset;
    int32_t radius;
    int32_t min_neighbors;
    float gate_scale;
    int32_t reserved0;
    const float* depth;
    float* normal;
    uint8_t* valid;
    int32_t* count;
    float* moments;
    void* stream;
} RelposeDepthNormalsArgs;
int relpose_depth_normals(const RelposeDepthNormalsArgs* args);

/* -------------------------------------------------------------------- skybox panoramas from posed perspective RGB-D frames
 * The reference's ScanNet loader reads every frame twice (datasets/ScanNet.py:211-230): the 480x640 frames (obs_depth/, obs_rgb/) and a
 * 160x640 panorama whose kinect window holds the same data; the tool that made the second from the first was never published, the geometry
 * that ties them together was (util.depth2pc :499-521, reproj_helper :537-749).  relpose_frames_to_pano splats one or several posed frames
 * per view into the four-face panorama, with occlusion handled.  The contract is the project's own (tests/panorama_model.py
 * restates it in numpy).  Three launches behind the workspace clear, enqueued on `stream`; invalid arguments return RELPOSE_EINVAL before
 * anything is enqueued.  The geometry is float64, every operation rounded on its own; every accumulator is an integer, so the result does
 * not depend on the order in which points arrive: it is repeatable bit for bit, and a view's result does not depend on the batch around it.
 *
 *   depth            [n_views, n_frames, frame_h, frame_w] f32; a value <= 0 or a non-finite one means no data
 *   rgb              [n_views, n_frames, frame_h, frame_w, 3] u8
 *   scale            [n_views, n_frames, 2] f64: (sx, sy) = (2 fx / frame_w, 2 fy / frame_h); ScanNet's are (0.8921875 * 2, 1.1895 * 2).  The
 *                    principal point is the frame centre: an off-centre principal point and lens distortion are not modelled
 *   pose             [n_views, n_frames, 4, 4] f64 row-major, frame -> panorama; NULL = identity
 *   unprojection     pixel (row r, column c), depth z (as f64): x = ((c / frame_w - 0.5) * 2 * z) / sx, y = ((0.5 - r / frame_h) * 2 * z) / sy,
 *                    p = (x, y, -z), then q_a = ((T_a0 x + T_a1 y) + T_a2 (-z)) + T_a3 when there is a pose
 *   projection       reproj_helper's rule: for slot = 0..3, (X, Y, Z) = Rs[k]^T q with k = slot (suncg) / (slot - 1) % 4 (matterport,
 *                    scannet); xn = X / (|Z| + 1e-32), yn = Y / (|Z| + 1e-32); the slot is taken when Z < 0, |xn| < 1, |yn| < 1 (the first
 *                    such slot; the strict tests make the faces disjoint); column = slot h + clip(rint((xn + 1) * 0.5 * h), 0, h - 1),
 *                    row = clip(rint((1 - yn) * 0.5 * h), 0, h - 1), rint rounding half to even; face depth d = (float)(-Z)
 *   dropped          points on no face, points outside box, points with d >= 32768
 *   box              y0, y1, x0, x1 in panorama pixels (half open), or all -1 for none; 0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= 4h
 *   pass 1           zmin = min d over all points of all frames of the view on the pixel
 *   pass 2           a point is accepted when d <= zmin + zmin * gate (f32, two roundings); it adds 1 to count, llrint((double)d * 65536.0)
 *                    to sum_z and its three bytes to sum_rgb
 *   pass 3           out_depth = (float)((double)sum_z / (double)count / 65536.0); per channel q = (2 sum + count) / (2 count) in integers,
 *                    out_rgb = (float)q / 255.0f; out_valid = count > 0; a pixel without accepted points is 0 everywhere
 *   out_depth        [n_views, h, 4h] f32;  out_rgb [n_views, 3, h, 4h] f32;  out_valid [n_views, h, 4h] u8
 *   zmin, count,     optional copies of the accumulators: zmin [n_views, h, 4h] u32 (the bits of the f32 minimum, 0 on an empty pixel),
 *   sum_z, sum_rgb   count [n_views, h, 4h] u32, sum_z [n_views, h, 4h] u64, sum_rgb [n_views, 3, h, 4h] u32
 *   limits           h even, 2..8192; n_frames >= 1; n_views * n_frames <= 65535; n_frames * frame_h * frame_w <= 2^24 (sum_rgb is u32);
 *                    gate finite, >= 0 (0.05 is the library's default); frame_h * frame_w = 0 is legal and gives an empty panorama;
 *                    a launch holds fewer than 2^32 threads: n_views * n_frames * 256 * ceil(frame_h / 16) * ceil(frame_w / 16) < 2^32 and
 *                    n_views * h * 4h + 255 < 2^32
 *   workspace        relpose_frames_to_pano_workspace_bytes(n_views, h) bytes (0 for invalid sizes), 8-byte aligned (sum_z lies at its base) */
typedef struct RelposeFramesToPanoArgs {
    uint32_t struct_size;       /* sizeof(RelposeFramesToPanoArgs) as the caller compiled it */
    int32_t n_views;
    int32_t n_frames;
    int32_t frame_h;
    int32_t frame_w;
    int32_t h;
    int32_t dataset;
    float gate;
    int32_t box[4];
    const float* depth;
    const uint8_t* rgb;
    const double* scale;
    const double* pose;
    float* out_depth;
    float* out_rgb;
    uint8_t* out_valid;
    uint32_t* zmin;
    uint32_t* count;
    uint64_t* sum_z;
    uint32_t* sum_rgb;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeFramesToPanoArgs;
size_t relpose_frames_to_pano_workspace_bytes(int32_t n, int32_t h);
int relpose_frames_to_pano(const RelposeFramesToPanoArgs* args);

/* -------------------------------------------------------------------- grid-based overlap statistics
 * The nearest-neighbour statistics of util.point_cloud_overlap (util.py:21-40) for a batch of directed (query cloud, reference cloud, pose)
 * triples: how many points of the moved query cloud have a reference point within max_dist, and the clouds' closest-pair distance.  The
 * values are those relpose_nn_dist gives (the same expressions, every operation rounded on its own); the work is not: every cloud gets one
 * uniform grid (cell edge max_dist (1 + 2^-10)) that all queries naming it share, a query point looks at the 27 cells around it, and a
 * query without a hit finds its closest pair in a pass over bounding boxes of 256-point tiles that prunes against a running bound.  The
 * contract is DESIGN.md 4.14; tests/overlap_model.py restates it in numpy.  Four launches behind a 4-byte clear and the upload of the two index arrays, whatever n_queries is.
 * Only integer atomics (add, min on the bit pattern of a non-negative double): results are repeatable bit for bit, and a query's outputs
 * do not depend on the batch around it.
 *
 *   pc, valid        [n_clouds, n_points, 3] f64 and [n_clouds, n_points] u8 as relpose_depth2pc writes them; valid NULL = all valid
 *   query_cloud_host, ref_cloud_host   [n_queries] i32 in HOST memory (they are validated before anything touches the device)
 *   pose             [n_queries, 4, 4] f64 row-major, query cloud -> the reference cloud's frame: q_a = ((T_a0 x + T_a1 y) + T_a2 z) + T_a3
 *   max_dist         finite, > 0 (the reference uses 0.08)
 *   d2               (dx dx + dy dy) + dz dz with d = q - r; a pair with a non-finite d2 is never a neighbour
 *   hits             [n_queries] i32 = #{valid query points : sqrt(min d2 over the valid reference points) < max_dist}
 *   nn_min           [n_queries] f64 = the minimum of that square root over the valid query points: the closest-pair distance, exact
 *                    whether or not a point hits; +inf when either cloud has no valid point (or none with finite coordinates)
 *   n_valid          [n_clouds] i32 = #{valid points}; points with a non-finite coordinate count
 *   hit              [n_queries, n_points] u8 or NULL: the per-point flag behind hits (0 for an invalid point)
 *   workspace        relpose_overlap_workspace_bytes(n_clouds, n_points, n_queries) bytes (0 for invalid sizes), 256-byte aligned
 *   limits           1 <= n_clouds, n_queries; 1 <= n_points <= 2^24; n_queries * ceil(n_points / 256) < 2^31
 * Returns RELPOSE_EINVAL before the device is touched for a NULL required pointer, a max_dist that is not finite or <= 0, a cloud index
 * outside 0..n_clouds-1 or sizes outside the limits.  Returns RELPOSE_OVERLAP_EXTENT, with none of the four outputs written, when the
 * finite points of some cloud span more than 2^20 cells along an axis (the grid keys would not fit).  The call waits for `stream` once, at
 * its end, to read that flag. */
#define RELPOSE_OVERLAP_EXTENT (-7)
typedef struct RelposeOverlapArgs {
    uint32_t struct_size;       /* sizeof(RelposeOverlapArgs) as the caller compiled it */
    int32_t n_clouds;
    int32_t n_points;
    int32_t n_queries;
    const double* pc;
    const uint8_t* valid;
    const int32_t* query_cloud_host;
    const int32_t* ref_cloud_host;
    const double* pose;
    double max_dist;
    int32_t* hits;
    double* nn_min;
    int32_t* n_valid;
    uint8_t* hit;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeOverlapArgs;
size_t relpose_overlap_workspace_bytes(int32_t n_clouds, int32_t n_points, int32_t n_queries);
int relpose_overlap(const RelposeOverlapArgs* args);

/* -------------------------------------------------------------------- visibility consistency of relative poses
 * relpose_overlap is blind where two scans share no surface: no point has a neighbour under the right pose or under a wrong one.  A depth
 * panorama still says which space its sensor saw through.  relpose_visibility scores a batch of directed (query cloud, reference view, pose)
 * triples: every moved query point is projected into the reference view's depth panorama and compared with the depths measured around its
 * pixel.  In front of them the point contradicts the view (violation), behind them it is hidden (occluded), on them it agrees.  The
 * contract is the project's own (tests/visibility_model.py restates it in numpy).  Two launches, whatever n_queries is; the
 * first also clears the counters.  Invalid arguments return RELPOSE_EINVAL before anything is enqueued or any output is touched.  The
 * geometry is float64, every operation rounded on its own; only integer atomics are used, one per class per workgroup: results are
 * repeatable bit for bit, and a query's row does not depend on the batch around it.
 *
 *   pc, valid        [n_clouds, n_points, 3] f64 and [n_clouds, n_points] u8 as relpose_depth2pc writes them; valid NULL = all valid
 *   depth            [n_views, h, 4h] f32 reference panoramas; a value that is not finite or is <= 0 means no data
 *   query_cloud_host, ref_view_host   [n_queries] i32 in HOST memory (they are validated before anything touches the device)
 *   pose             [n_queries, 4, 4] f64 row-major, query cloud -> the reference view's frame: q_a = ((T_a0 x + T_a1 y) + T_a2 z) + T_a3
 *   dataset          RELPOSE_SUNCG / RELPOSE_MATTERPORT / RELPOSE_SCANNET: the face order of the reference panoramas
 *   radius           r in {0, 1, 2}, h >= 2r + 1;  tol_abs, tol_rel: finite, >= 0 (the library's defaults are r = 1, 0.05 and 0.02)
 *   pass 1           once per view however many queries name it: for every pixel (dmin, dmax) as f32 = the minimum and maximum of the valid
 *                    depths in the (2r+1)^2 window around it.  The window is clipped to the pixel's own face: columns do not cross a face
 *                    seam (neighbouring faces see one wall at different face depths), rows are clipped to 0..h-1; invalid neighbours are
 *                    skipped; a pixel whose own depth is invalid is unobserved whatever its neighbours hold
 *   pass 2           relpose_frames_to_pano's projection: for slot = 0..3, (X, Y, Z) = Rs[k]^T q with k = slot (suncg) / (slot - 1) % 4
 *                    (matterport, scannet); xn = X / (|Z| + 1e-32), yn = Y / (|Z| + 1e-32); the first slot with Z < 0, |xn| < 1, |yn| < 1 is
 *                    taken; column = slot h + clip(rint((xn + 1) * 0.5 * h), 0, h - 1), row = clip(rint((1 - yn) * 0.5 * h), 0, h - 1), rint
 *                    rounding half to even; d = -Z, kept in f64
 *   class            0 invalid point; 1 outside: no face, a non-finite moved coordinate, or d >= 32768; 2 unobserved: the pixel has no data;
 *                    4 violation: d < dmin - (tol_abs + tol_rel * dmin); 5 occluded: d > dmax + (tol_abs + tol_rel * dmax); 3 consistent
 *                    otherwise.  dmin, dmax widened to f64; each of the two multiplications, two additions and the subtraction is its own
 *                    f64 operation; the inequalities are strict: a point exactly on a bound is consistent
 *   counts           [n_queries, 6] i32: the number of points in each class 0..5; a row sums to n_points
 *   margin_sum       [n_queries] u64: over the violations, the sum of llrint(min(m, 32768) * 65536.0), m = (dmin - (tol_abs + tol_rel * dmin)) - d
 *                    (the panorama accumulators' fixed point; a term is at most 2^31 -- the minimum only acts where a reference depth
 *                    exceeds 32768 -- so the sum cannot overflow for n_points <= 2^24)
 *   cls              [n_queries, n_points] u8 or NULL: the class of every point
 *   workspace        relpose_visibility_workspace_bytes(n_views, h, n_queries) bytes (0 for invalid sizes), 256-byte aligned: the window
 *                    images (8 bytes per pixel, the pair interleaved so that pass 2 needs one gather per point) and the two index arrays
 *   limits           h even, 2..8192; 1 <= n_views, n_clouds, n_queries; n_views * h * 4h < 2^31; 1 <= n_points <= 2^24;
 *                    n_queries * ceil(n_points / 256) < 2^31; cloud and view indices in range
 * The call waits for `stream` once, at its end: the two host index arrays are the caller's again when it returns. */
typedef struct RelposeVisibilityArgs {
    uint32_t struct_size;       /* sizeof(RelposeVisibilityArgs) as the caller compiled it */
    int32_t n_clouds;
    int32_t n_points;
    int32_t n_views;
    int32_t h;
    int32_t n_queries;
    int32_t dataset;
    int32_t radius;
    const double* pc;
    const uint8_t* valid;
    const float* depth;
    const int32_t* query_cloud_host;
    const int32_t* ref_view_host;
    const double* pose;
    double tol_abs;
    double tol_rel;
    int32_t* counts;
    uint64_t* margin_sum;
    uint8_t* cls;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeVisibilityArgs;
size_t relpose_visibility_workspace_bytes(int32_t n_views, int32_t h, int32_t n_queries);
int relpose_visibility(const RelposeVisibilityArgs* args);

/* -------------------------------------------------------------------- TSDF fusion of posed depth panoramas
 * What a user does with poses is merge the scans.  relpose_tsdf_fuse integrates the views of n_scenes scenes into n_scenes volumes of
 * nx * ny * nz voxels (a truncated signed distance function in the style of Curless-Levoy / KinectFusion: positive in the space a sensor
 * saw through, negative behind the surface it measured), relpose_tsdf_surface extracts the zero crossings as an oriented, coloured point
 * cloud in relpose_overlap's layout.  The contract is the project's own (tests/tsdf_model.py restates it in numpy).  Every
 * accumulated value is an integer: the volume does not depend on the order of the views, nor on whether they come in one call or several.
 * The geometry is float64, every operation rounded on its own.  No atomics.  Invalid arguments return RELPOSE_EINVAL before anything is
 * enqueued or any output is touched.
 *
 *   depth            [n_views, h, 4h] f32 panoramas; a value is data iff z > 0 && z <= FLT_MAX (relpose_visibility's rule)
 *   rgb              [n_views, 3, h, 4h] f32 or NULL
 *   pose             [n_views, 4, 4] f64 row-major on the DEVICE, world -> camera (the loaders' R)
 *   view_begin_host  [n_scenes + 1] i32 in HOST memory, ascending from 0 to n_views: scene s owns the views view_begin[s] .. view_begin[s+1]-1
 *                    (a scene may have none; at most 4096 per scene per call)
 *   origin_host      [n_scenes, 3] f64 in HOST memory, finite: the corner of voxel (0, 0, 0);  voxel, trunc: finite, > 0, shared
 *   tsdf_sum, weight [n_scenes, nz, ny, nx] i32, x fastest;  color_sum [n_scenes, 3, nz, ny, nx] u32, required with rgb and NULL without
 *   accumulate       0: the sums of this call are stored (no clear is needed); 1: they are added to what is there
 *   rule             for voxel (i, j, k) and each view v of its scene: c_a = origin_a + ((double)idx_a + 0.5) * voxel;
 *                    q_a = ((T_a0 cx + T_a1 cy) + T_a2 cz) + T_a3; relpose_visibility's projection of q gives the pixel and d = -Z; the view
 *                    is skipped if q is not finite, no face takes it, or d >= 32768; D = (double)depth[v, pixel], skipped if no data;
 *                    sdf = D - d, skipped if sdf < -trunc; t = fmin(sdf / trunc, 1.0); tsdf_sum += llrint(t * 32768.0); weight += 1; with rgb,
 *                    per channel, color_sum += (uint32)rintf(fminf(fmaxf(c, 0.f), 1.f) * 255.f) of the same pixel (a NaN colour counts 0).
 *                    The lookup is nearest-pixel.
 *   limits           h even, 2..8192; n_views * h * 4h < 2^31; 1 <= n_scenes; n_scenes * nx * ny * nz < 2^31; dataset as relpose_visibility.
 *                    Across accumulating calls the CALLER keeps every voxel's weight <= 65535: |tsdf_sum| <= 65535 * 32768 and
 *                    color_sum <= 65535 * 255 then stay below 2^31.
 *   workspace        relpose_tsdf_fuse_workspace_bytes(n_scenes, n_views, h, nx, ny, nz) bytes (0 for sizes outside the limits), 256-byte
 *                    aligned: the device copies of view_begin and origin
 * The call waits for `stream` once, at its end: the host arrays are the caller's again when it returns. */
typedef struct RelposeTsdfFuseArgs {
    uint32_t struct_size;       /* sizeof(RelposeTsdfFuseArgs) as the caller compiled it */
    int32_t n_scenes;
    int32_t n_views;
    int32_t h;
    int32_t dataset;
    int32_t nx, ny, nz;
    int32_t accumulate;
    int32_t reserved0;
    const float* depth;
    const float* rgb;
    const double* pose;
    const int32_t* view_begin_host;
    const double* origin_host;
    double voxel;
    double trunc;
    int32_t* tsdf_sum;
    int32_t* weight;
    uint32_t* color_sum;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeTsdfFuseArgs;
size_t relpose_tsdf_fuse_workspace_bytes(int32_t n_scenes, int32_t n_views, int32_t h, int32_t nx, int32_t ny, int32_t nz);
int relpose_tsdf_fuse(const RelposeTsdfFuseArgs* args);

/* The surface of relpose_tsdf_fuse's state, per scene.  A voxel is known iff weight >= min_weight (>= 1); its value is
 * t = (double)tsdf_sum / (32768.0 * (double)weight).  For every known voxel a, in ascending linear index, and each positive-axis neighbour
 * b = a + e_axis (x, then y, then z) inside the volume that is known: if (ta >= 0 && tb < 0) || (ta < 0 && tb >= 0) one point is emitted at
 * s = ta / (ta - tb) along the edge: its coordinate on that axis is origin + (((double)idx + 0.5) + s) * voxel, the other two are the
 * centre's, origin + ((double)idx + 0.5) * voxel.
 *   normal           g(a) + s * (g(b) - g(a)) per component, divided by sqrt((gx gx + gy gy) + gz gz); a zero vector stays zero.  Component
 *                    c of g(v) is (t(v + e_c) - t(v - e_c)) * 0.5 when both neighbours are known (inside the volume and weight >=
 *                    min_weight), t(v + e_c) - t(v) or t(v) - t(v - e_c) when one is, 0 when neither is.  t grows towards the space the
 *                    sensors saw through: the normal points there, in the world frame.
 *   colour           with color_sum and colors: (float)(ca + s * (cb - ca)) per channel, c = (double)color_sum / (255.0 * (double)weight)
 *   points, normals  [n_scenes, cap, 3] f64;  colors [n_scenes, cap, 3] f32 or NULL (needs color_sum);  valid [n_scenes, cap] u8:
 *                    relpose_overlap's pc / valid.  n_points [n_scenes] i32: the number of crossings, which may exceed cap; only the
 *                    first cap are written; valid is 1 for rows < min(n, cap) and 0 beyond; the other rows beyond are not touched.
 *   limits           1 <= n_scenes; n_scenes * nx * ny * nz < 2^31; 3 * nx * ny * nz < 2^31; 1 <= cap; n_scenes * cap < 2^29;
 *                    min_weight >= 1; voxel finite > 0; origin finite
 *   workspace        relpose_tsdf_surface_workspace_bytes(n_scenes, nx, ny, nz) bytes (0 for sizes outside the limits), 256-byte aligned: the
 *                    crossings per workgroup, their scan, and the device copy of origin
 * Three launches: count per workgroup, scan per scene, write.  The call waits for `stream` once, at its end. */
typedef struct RelposeTsdfSurfaceArgs {
    uint32_t struct_size;       /* sizeof(RelposeTsdfSurfaceArgs) as the caller compiled it */
    int32_t n_scenes;
    int32_t nx, ny, nz;
    int32_t min_weight;
    int32_t cap;
    int32_t reserved0;
    const int32_t* tsdf_sum;
    const int32_t* weight;
    const uint32_t* color_sum;
    const double* origin_host;
    double voxel;
    double* points;
    double* normals;
    float* colors;
    uint8_t* valid;
    int32_t* n_points;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeTsdfSurfaceArgs;
size_t relpose_tsdf_surface_workspace_bytes(int32_t n_scenes, int32_t nx, int32_t ny, int32_t nz);
int relpose_tsdf_surface(const RelposeTsdfSurfaceArgs* args);

/* One indexed triangle mesh per scene from relpose_tsdf_fuse's state: marching cubes (tests/mesh_model.py restates the
 * contract in numpy).  The crossings relpose_tsdf_surface emits are exactly the vertices of such a mesh; this call adds the triangles.
 *   vertices         points, normals, colors, valid, n_points with capacity cap: in content and order exactly what relpose_tsdf_surface
 *                    writes for the same state, min_weight, origin, voxel and cap.  A vertex that no triangle uses is kept (its edge
 *                    touches no complete cell).
 *   cells            cell (i, j, k), i < nx-1, j < ny-1, k < nz-1, contributes iff all eight corner voxels are known.  Corner c (0..7) sits
 *                    at offset (c & 1, c >> 1 & 1, c >> 2 & 1); case = the mask with bit c set iff t(corner c) < 0.  Edge 4a + u + 2v runs
 *                    along axis a from the corner whose offsets on the other two axes, ascending, are (u, v); its vertex is the crossing
 *                    that corner's voxel owns on axis a, and that vertex's index is the index of the voxel's first crossing plus the
 *                    number of lower axes on which the voxel has one.
 *   table            per case a list of at most 5 triangles of edge ids, generated by tools/gen_mc_table.py into csrc/mc_table.h from a
 *                    face rule: on each cube face, corners counter-clockwise seen from outside, every maximal run of negative corners
 *                    gives one directed segment from the crossing edge that enters the run to the one that leaves it; the segments
 *                    close into loops (ordered by smallest edge id); each loop is a fan from the vertex with the fewest in-face fan
 *                    diagonals (ties: smallest edge id).  Two cells sharing a face draw the same segments on it: the mesh has no holes
 *                    between cells, and (p1 - p0) x (p2 - p0) points where t grows, as the normals do.
 *   triangles        [n_scenes, cap_tri, 3] i32 indices into the scene's vertex list; cells in ascending linear index (x fastest), within a
 *                    cell in the table's order.  n_triangles [n_scenes] i32 may exceed cap_tri: only the first cap_tri are written, rows
 *                    beyond are not touched.  The indices are the true vertex indices even where they are >= cap: the CALLER checks
 *                    n_points <= cap before using the mesh.  Where t == 0 at a corner several vertices coincide and a triangle has zero
 *                    area; it is kept, and its three indices are still distinct.
 *   limits           relpose_tsdf_surface's, and 5 (nx-1) (ny-1) (nz-1) < 2^31; 1 <= cap_tri; n_scenes * cap_tri < 2^29.  A volume with a
 *                    dimension of 1 has no cells and no triangles.
 *   workspace        relpose_tsdf_mesh_workspace_bytes(n_scenes, nx, ny, nz) bytes (0 for sizes outside the limits), 256-byte aligned: both
 *                    counts per workgroup, the device copy of origin, and per voxel the index of its first vertex and one flag byte
 * No atomics: a scene's result is bitwise repeatable and independent of the batch around it.  Invalid arguments return RELPOSE_EINVAL
 * before anything is enqueued or any output is touched.  Four launches: count, scan, vertices, triangles.  The call waits for `stream`
 * once, at its end. */
typedef struct RelposeTsdfMeshArgs {
    uint32_t struct_size;       /* sizeof(RelposeTsdfMeshArgs) as the caller compiled it */
    int32_t n_scenes;
    int32_t nx, ny, nz;
    int32_t min_weight;
    int32_t cap;
    int32_t cap_tri;
    const int32_t* tsdf_sum;
    const int32_t* weight;
    const uint32_t* color_sum;
    const double* origin_host;
    double voxel;
    double* points;
    double* normals;
    float* colors;
    uint8_t* valid;
    int32_t* n_points;
    int32_t* triangles;
    int32_t* n_triangles;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeTsdfMeshArgs;
size_t relpose_tsdf_mesh_workspace_bytes(int32_t n_scenes, int32_t nx, int32_t ny, int32_t nz);
int relpose_tsdf_mesh(const RelposeTsdfMeshArgs* args);

/* -------------------------------------------------------------------- connected components of triangle meshes, and their removal
 * relpose_mesh_components labels the connected components of n_scenes indexed triangle meshes in relpose_tsdf_mesh's layout and sums a few
 * integers per component; relpose_mesh_filter keeps the components a caller selects and compacts the mesh.  The contract is the project's own
 * (tests/components_model.py restates it in numpy).  Every input and output is device memory unless it says host.
 *   scene            nv = min(max(n_points, 0), cap) vertices and nt = min(max(n_triangles, 0), cap_tri) triangle rows (relpose_tsdf_mesh's
 *                    counts may exceed its caps; only what was written is read).
 *   bad rows         a row < nt with an index outside [0, nv) is bad: it joins nothing, gets label -1 and is counted in bad_triangles [S].
 *   rule             VERTEX connectivity: two vertices are connected iff a chain of good triangles links them through shared vertex
 *                    indices.  Two triangles that meet in ONE vertex are one component -- unlike Open3D's cluster_connected_triangles, which
 *                    joins triangles across shared edges only.  It is what union-find over vertices gives, and it keeps the zero-area
 *                    triangles marching cubes leaves where t == 0 with the surface they belong to.  Vertices are joined by index, never by
 *                    position.  A vertex no good triangle names belongs to no component.
 *   numbering        components are numbered 0, 1, ... in ascending order of their smallest vertex index: the result is unique.
 *   vertex_label     [S, cap] i32: the component, -1 for unused vertices and rows >= nv.      tri_label [S, cap_tri] i32: -1 for bad rows and
 *                    rows >= nt.      n_components [S] i32: the true count, which may exceed cap_comp.      bad_triangles [S] i32.
 *   statistics       for components c < cap_comp, each [S, cap_comp]: comp_root i32 (the smallest vertex index), comp_vertices i32,
 *                    comp_triangles i32, comp_area i64; entries at and beyond n_components hold -1, 0, 0, 0.  The four pointers may be NULL
 *                    with cap_comp = 0 (the counting call).  comp_area = the sum over the component's triangles of
 *                    llrint(min(A area_scale, 2147483648.0)) with A = sqrt((cx cx + cy cy) + cz cz) 0.5 and c = (p1 - p0) x (p2 - p0), every
 *                    operation its own f64 rounding; a product A area_scale that is not finite counts 0.  points NULL: comp_area is 0.
 *   method           monotone lowering: L[v] starts at v; a round lowers, with device-scope atomic minima only, every good triangle's three
 *                    entries and the entries they point to to the triangle's smallest label, then shortcuts L[v] <- L[L[v]].  Every write is
 *                    the minimum with a label of the same component, so a stale read costs a round and never an answer; the fixpoint is the
 *                    component's smallest index.  The host reads one flag word per group of 4 rounds and stops at the first round that
 *                    lowered nothing; *rounds_host (host, may be NULL) receives the number of rounds counted, that last one included.  If
 *                    round max_rounds still lowered a label the call returns RELPOSE_EROUNDS and promises nothing about the outputs:
 *                    max_rounds is a guard, not a tuning knob.
 *   limits           n_scenes >= 1; 1 <= cap, 1 <= cap_tri; n_scenes * cap, n_scenes * cap_tri and n_scenes * cap_comp < 2^29; cap_comp >= 0;
 *                    area_scale finite and > 0; max_rounds >= 1.
 *   workspace        relpose_mesh_components_workspace_bytes(n_scenes, cap, cap_tri) bytes (0 outside the limits), 256-byte aligned.
 * The sums are integer atomic adds: every output is bitwise repeatable and a scene does not depend on its batch.  Invalid arguments return
 * RELPOSE_EINVAL before anything is enqueued or any output is touched.  The call waits for `stream` once per group of rounds; the ranking
 * and statistics launches behind the last wait are only enqueued. */
typedef struct RelposeMeshComponentsArgs {
    uint32_t struct_size;       /* sizeof(RelposeMeshComponentsArgs) as the caller compiled it */
    int32_t n_scenes;
    int32_t cap;
    int32_t cap_tri;
    int32_t cap_comp;
    int32_t max_rounds;
    const int32_t* triangles;   /* [n_scenes, cap_tri, 3] */
    const int32_t* n_triangles; /* [n_scenes] */
    const int32_t* n_points;    /* [n_scenes] */
    const double* points;       /* [n_scenes, cap, 3], or NULL for no areas */
    double area_scale;
    int32_t* vertex_label;
    int32_t* tri_label;
    int32_t* n_components;
    int32_t* bad_triangles;
    int32_t* comp_root;
    int32_t* comp_vertices;
    int32_t* comp_triangles;
    int64_t* comp_area;
    int32_t* rounds_host;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeMeshComponentsArgs;
size_t relpose_mesh_components_workspace_bytes(int32_t n_scenes, int32_t cap, int32_t cap_tri);
int relpose_mesh_components(const RelposeMeshComponentsArgs* args);

/* Keep the selected components of relpose_mesh_components' meshes and compact them.
 *   survivors        a triangle row < nt survives iff its tri_label is in [0, cap_comp) and keep [S, cap_comp] u8 is not 0 for it.  A vertex
 *                    < nv survives iff its vertex_label is kept in the same sense; a vertex with label < 0 survives iff drop_unused is 0.
 *   order            survivors keep their order: a vertex's new index is the number of surviving vertices below it, and the triangles' indices
 *                    are renumbered (an index whose vertex did not survive, which labels of relpose_mesh_components never produce, becomes -1).
 *   outputs          out_points, out_normals f64 [S, cap, 3], out_colors f32 [S, cap, 3] (NULL iff colors is), out_triangles i32 [S, cap_tri, 3]:
 *                    only rows below the new counts out_n_points, out_n_triangles [S] i32 are written, each a bitwise copy of its source
 *                    row; out_valid u8 [S, cap] is written whole, 1 below the new count.  vertex_map [S, cap] i32 (may be NULL): old index
 *                    -> new index, -1 for dropped vertices and rows >= nv.  Every output is a buffer of its own, none an input.
 *   limits           relpose_mesh_components'; drop_unused 0 or 1; keep may be NULL only with cap_comp = 0 (nothing labelled survives).
 *   workspace        relpose_mesh_filter_workspace_bytes(n_scenes, cap, cap_tri) bytes (0 outside the limits), 256-byte aligned.
 * Flag, scan per scene, scatter: four launches, no atomics, only enqueued on `stream`.  Invalid arguments return RELPOSE_EINVAL before
 * anything is enqueued or any output is touched. */
typedef struct RelposeMeshFilterArgs {
    uint32_t struct_size;       /* sizeof(RelposeMeshFilterArgs) as the caller compiled it */
    int32_t n_scenes;
    int32_t cap;
    int32_t cap_tri;
    int32_t cap_comp;
    int32_t drop_unused;
    const double* points;
    const double* normals;
    const float* colors;
    const int32_t* n_points;
    const int32_t* triangles;
    const int32_t* n_triangles;
    const int32_t* vertex_label;
    const int32_t* tri_label;
    const uint8_t* keep;
    double* out_points;
    double* out_normals;
    float* out_colors;
    uint8_t* out_valid;
    int32_t* out_n_points;
    int32_t* out_triangles;
    int32_t* out_n_triangles;
    int32_t* vertex_map;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeMeshFilterArgs;
size_t relpose_mesh_filter_workspace_bytes(int32_t n_scenes, int32_t cap, int32_t cap_tri);
int relpose_mesh_filter(const RelposeMeshFilterArgs* args);

/* -------------------------------------------------------------------- decimation of triangle meshes by vertex clustering
 * relpose_mesh_decimate merges the vertices of n_scenes indexed triangle meshes in relpose_tsdf_mesh's layout that fall into one cell of a
 * regular grid, and rewrites the triangles.  The contract is the project's own (tests/decimate_model.py restates it in numpy,
 * on whole arrays and as plain loops).  Every input and output is device memory unless it says host.
 *   scene            relpose_mesh_components' rule: nv = min(max(n_points, 0), cap) vertices and nt = min(max(n_triangles, 0), cap_tri) rows.
 *                    A row < nt with an index outside [0, nv) is bad: it is dropped and counted in bad_triangles.
 *   cells            origin_host [S, 3] f64 (HOST), cell f64, gx, gy, gz.  For vertex v and axis a: u_a = (p_a - origin_a) / cell, each
 *                    operation its own f64 rounding.  v is INSIDE iff all three u_a are finite and 0 <= floor(u_a) < g_a; its cell is
 *                    (floor(u_x), floor(u_y), floor(u_z)).  A vertex that is not inside is dropped (vertex_map = -1), and every good triangle
 *                    that names a dropped vertex is dropped too and counted in outside_triangles.
 *   clusters         all inside vertices of one cell form one cluster, whether a triangle uses them or not: the clusters do not depend on
 *                    the triangle list.  A cluster's representative is its smallest vertex index; clusters are numbered 0, 1, ... in
 *                    ascending order of their representative.  vertex_map [S, cap] i32: old index -> cluster, -1 for dropped vertices and
 *                    rows >= nv; written whole.  out_n_points [S] i32: the true cluster count (<= cap).
 *   attributes       integer sums over the n vertices of a cluster, so the order of the additions does not matter:
 *                    position  q_a = llrint(u_a * 65536.0) summed as int64; out_p_a = origin_a + ((double)sum_a / (65536.0 * (double)n)) * cell,
 *                              each operation rounded on its own;
 *                    normal    llrint(n_a * 32768.0) per component summed as int64; a component that is not finite counts 0 (and so does one
 *                              of magnitude above 65536.0, which no normal has: the conversion stays defined and the sum inside int64);
 *                              with s the sums as doubles, len = sqrt((s_x s_x + s_y s_y) + s_z s_z) and the output is s / len, or
 *                              (0, 0, 0) when len == 0;
 *                    colour    (colors not NULL) llrint(min(max((double)c, 0.0), 1.0) * 65535.0) summed as int64, NaN counts 0; the output
 *                              is (float)((double)sum / (65535.0 * (double)n));
 *                    count     out_count [S, cap] i32 = n.
 *                    Only rows below out_n_points of out_points, out_normals f64 [S, cap, 3], out_colors f32 [S, cap, 3] (NULL iff colors is)
 *                    and out_count are written; out_valid [S, cap] u8 is written whole, 1 below out_n_points.
 *   triangles        a good row (i, j, k) whose vertices are all inside becomes (m(i), m(j), m(k)), m = vertex_map.  It is DEGENERATE iff
 *                    two of the three are equal: dropped and counted in degenerate_triangles.  With dedupe = 1 two surviving rows are
 *                    DUPLICATES iff they are equal after rotating each so that its smallest index comes first; the rotation keeps the
 *                    orientation, so (a, b, c) and (a, c, b) are not duplicates.  Of a set of duplicates the lowest row survives, the
 *                    others are counted in duplicate_triangles.  Survivors keep their order and are written as remapped, UNROTATED indices
 *                    to out_triangles [S, cap_tri, 3] i32 (only rows below out_n_triangles [S] i32, the true count, are written).
 *                    tri_map [S, cap_tri] i32 (may be NULL; written whole): old row -> new row, or -1 bad, -2 outside, -3 degenerate,
 *                    -4 duplicate, -5 row >= nt.  The four counters are i32 [S]; bad + outside + degenerate + duplicate + survivors = nt.
 *   limits           n_scenes >= 1; 1 <= cap, 1 <= cap_tri; n_scenes * cap and n_scenes * cap_tri < 2^29; 1 <= gx, gy, gz <= 1024;
 *                    n_scenes * gx * gy * gz < 2^27; cell finite and > 0; origin finite; dedupe 0 or 1.  Every output is a buffer of its own,
 *                    none an input.
 *   workspace        relpose_mesh_decimate_workspace_bytes(n_scenes, cap, cap_tri, gx, gy, gz) bytes (0 outside the limits), 256-byte
 *                    aligned.
 *   method           a dense table of gx gy gz entries per scene takes the atomic minimum of the vertex indices of each cell; the
 *                    representatives are flagged, scanned per scene and numbered; one pass adds each vertex's ten integers to its cluster's
 *                    row, runs of equal clusters summed inside the wave first, then int64 atomic adds.  Duplicates need no sort: one
 *                    open-addressing table keyed by the packed pair (a, b) of the rotated row gives the pair a slot, a second keyed by
 *                    (slot, c) takes the atomic minimum of the row index; every probe loop is bounded by the table size (a power of two
 *                    >= 2 cap_tri) and nothing waits on another thread.  Slot numbers depend on the order of insertion, the surviving row
 *                    does not.
 * Every output is bitwise repeatable and a scene does not depend on its batch.  Invalid arguments return RELPOSE_EINVAL before anything is
 * enqueued or any output is touched.  The origins travel as kernel arguments: origin_host is the caller's again when the call returns, and
 * the launches are only enqueued on `stream`. */
typedef struct RelposeMeshDecimateArgs {
    uint32_t struct_size;       /* sizeof(RelposeMeshDecimateArgs) as the caller compiled it */
    int32_t n_scenes;
    int32_t cap;
    int32_t cap_tri;
    int32_t gx;
    int32_t gy;
    int32_t gz;
    int32_t dedupe;
    const double* points;       /* [n_scenes, cap, 3] */
    const double* normals;      /* [n_scenes, cap, 3] */
    const float* colors;        /* [n_scenes, cap, 3] or NULL */
    const int32_t* n_points;    /* [n_scenes] */
    const int32_t* triangles;   /* [n_scenes, cap_tri, 3] */
    const int32_t* n_triangles; /* [n_scenes] */
    const double* origin_host;  /* HOST [n_scenes, 3] */
    double cell;
    double* out_points;
    double* out_normals;
    float* out_colors;
    uint8_t* out_valid;
    int32_t* out_n_points;
    int32_t* out_count;
    int32_t* out_triangles;
    int32_t* out_n_triangles;
    int32_t* vertex_map;
    int32_t* tri_map;
    int32_t* bad_triangles;
    int32_t* outside_triangles;
    int32_t* degenerate_triangles;
    int32_t* duplicate_triangles;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeMeshDecimateArgs;
size_t relpose_mesh_decimate_workspace_bytes(int32_t n_scenes, int32_t cap, int32_t cap_tri, int32_t gx, int32_t gy, int32_t gz);
int relpose_mesh_decimate(const RelposeMeshDecimateArgs* args);

/* Frame-to-model alignment: refine the poses of n_views depth panoramas against relpose_tsdf_fuse's volumes, so that each view's measured
 * points come to lie on the zero level of the volume it names (the KinectFusion tracking step, sampled at the measured points: no ray is
 * marched).  The contract is the project's own (tests/align_model.py restates it in numpy, the per-point rule on whole arrays
 * and as plain loops).  The geometry is float64, every operation rounded on its own; whatever is summed across points is an integer, so the
 * result does not depend on the order of the points, on the decomposition into workgroups or on the batch around a view.  No atomics.
 *
 *   tsdf_sum, weight [n_scenes, nz, ny, nx] i32, origin_host [n_scenes, 3] f64 (HOST), voxel, min_weight (>= 1): relpose_tsdf_fuse's state
 *   depth            [n_views, h, 4h] f32; pose [n_views, 4, 4] f64 row-major on the DEVICE, world -> camera (the last row is copied through)
 *   scene_of_view_host [n_views] i32 in HOST memory, each in 0 .. n_scenes-1: several views may name one volume, a volume may have none
 *   points           pixel p = row * 4h + column takes part iff p % stride == 0 and its depth is data (z > 0 && z <= FLT_MAX).  With
 *                    slot = column / h, px = column % h, D = (double)z: xn = (2.0 * px) / h - 1.0, yn = 1.0 - (2.0 * row) / h -- the centre
 *                    that relpose_visibility's projection rounds to, so a point of column px >= 1 and row >= 1 projects onto its own pixel
 *                    (xn = -1 or yn = 1 lie on the face's open edge) -- and the camera point is Rs[face(dataset, slot)] (xn D, yn D, -D).
 *   evaluation       W = the rigid inverse of the current pose T: W_ab = T_ba, W_a3 = -((T_0a T_03 + T_1a T_13) + T_2a T_23);
 *                    q_a = ((W_a0 x + W_a1 y) + W_a2 z) + W_a3;  u_a = (q_a - origin_a) / voxel - 0.5, i0_a = floor(u_a), f_a = u_a - i0_a.
 *                    The point is, in this order: OUTSIDE unless q is finite and 0 <= i0_a <= n_a - 2 on every axis (nothing is read for
 *                    it); UNKNOWN if any of the 8 corners (i0 + (c & 1, c >> 1 & 1, c >> 2 & 1)) has weight < min_weight; SATURATED if any
 *                    corner has |t| >= 1, t = (double)tsdf_sum / (32768.0 * (double)weight); USED otherwise.  For a used point, with t_c:
 *                      d00 = t1 - t0, d10 = t3 - t2, d01 = t5 - t4, d11 = t7 - t6;  a00 = t0 + fx d00, a10 = t2 + fx d10, a01 = t4 + fx d01,
 *                      a11 = t6 + fx d11;  c0 = a10 - a00, c1 = a11 - a01;  b0 = a00 + fy c0, b1 = a01 + fy c1;
 *                      gz = b1 - b0;  r = b0 + fz gz;  gy = c0 + fz (c1 - c0);  e0 = d00 + fy (d10 - d00), e1 = d01 + fy (d11 - d01);
 *                      gx = e0 + fz (e1 - e0)          (r: the trilinear value in units of trunc; g: its gradient per voxel)
 *                      l_a = (q_a - c_a) / voxel, c_a = origin_a + (n_a * 0.5) * voxel;  J = (l x g, g) = (ly gz - lz gy, lz gx - lx gz,
 *                      lx gy - ly gx, gx, gy, gz);  Jq_i = llrint(J_i * 2^8) for i < 3, llrint(J_i * 2^16) for i >= 3, rq = llrint(r * 2^16).
 *   sums             [32] i64 per view and evaluation: the 21 products Jq_i Jq_j (i <= j, row-major), the 6 products Jq_i rq, rq rq, and
 *                    the counts of OUTSIDE, UNKNOWN, SATURATED and USED points, each summed over the view's points.  No overflow: a used
 *                    point lies inside the volume and n_a <= 2048, so |l_a| <= 1024; |t| < 1 at every corner, so |g_a| <= 2 and |r| < 1;
 *                    |Jq_i| <= 4096 * 2^8 = 2^20 (i < 3) and 2^17 (i >= 3), |rq| <= 2^16; at most 2^22 points per view:
 *                    every sum stays below 2^40 * 2^22 = 2^62.
 *   step             A_ij = (double)sum / (s_i s_j), b_i = (double)sum / (s_i 2^16) with s = 2^8 (i < 3) or 2^16: one rounding from int64
 *                    (exact below 2^53), the scales are exact.  A = V diag(lambda) V^T by cyclic Jacobi: 8 sweeps over (p, q), p < q,
 *                    row-major; a pair with A_pq == 0 is skipped; theta = (A_qq - A_pp) / (2 A_pq), t = +-1 / (|theta| + sqrt(theta theta + 1))
 *                    with theta's sign (+ for 0), c = 1 / sqrt(t t + 1), s = t c; A_pp -= t A_pq, A_qq += t A_pq, A_pq = 0, and for the
 *                    other k: A_kp' = c A_kp - s A_kq, A_kq' = s A_kp + c A_kq (mirrored); V likewise for every row.
 *                    Column k is taken iff n_used >= 6 and lambda_k > eig_min * n_used: coef_k = -((sum_i V_ik b_i) / lambda_k), summed from
 *                    0 in ascending i; every other column is HELD (coef_k = 0).  delta_i = sum_k V_ik coef_k, from 0 in ascending k.
 *   update           skipped (the pose is copied bit for bit) when n_used < 6.  Otherwise a = delta_0..2 * 0.5, aa = (a0 a0 + a1 a1) + a2 a2,
 *                    the Cayley rotation Rd = ((1 - aa) I + 2 a a^T + 2 [a]x) / (1 + aa), entry by entry ((1 - aa) + 2.0 * (a_i a_i)) / (1 + aa)
 *                    and (2.0 * (a_i a_j -+ a_k)) / (1 + aa);  d_i = (c_i - ((Rd_i0 c0 + Rd_i1 c1) + Rd_i2 c2)) + voxel * delta_{3+i}: the
 *                    points move by x -> c + Rd (x - c) + voxel tau in the world frame, about the volume's centre.  The new pose is
 *                    T' = T D^-1: R'_ij = (T_i0 Rd_j0 + T_i1 Rd_j1) + T_i2 Rd_j2, t'_i = T_i3 - ((R'_i0 d0 + R'_i1 d1) + R'_i2 d2).
 *                    Only + - * / sqrt: the numpy model follows every bit.
 *   iterations       iters + 1 evaluations (iters in 0..64); each but the last is followed by a step.  iters = 0 scores the poses as given.
 *   outputs          pose_out [n_views, 4, 4] f64 (may be `pose` itself); of the LAST evaluation, at the returned pose: eig [n_views, 6] f64 =
 *                    lambda / n_used ascending (0 without a used point), held [n_views] i32, sums [n_views, 32] i64;
 *                    rms [n_views, 2] f64 = sqrt((double)sum(rq rq) / n_used) / 2^16 (0 without a used point) at the first and the last
 *                    evaluation.  Optional, both or neither: trace_pose [n_views, iters + 1, 4, 4] f64 and trace_sums [n_views, iters + 1, 32]
 *                    i64, the pose and the sums of every evaluation.
 *   eig_min          finite, >= 0.  A direction the points do not constrain (a view that sees no wall across one axis) has a small
 *                    lambda / n_used, and a Gauss-Newton step along it follows gradient noise; 0.0043 separates the two ranges measured on the
 *                    synthetic rooms and is the default of the Python layers.
 *   limits           relpose_tsdf_fuse's for h, n_views and the volume; nx, ny, nz <= 2048; stride >= 1; ceil(4 h h / stride) <= 2^22
 *   workspace        relpose_tsdf_align_workspace_bytes(n_scenes, n_views, h, nx, ny, nz, stride) bytes (0 for sizes outside the limits),
 *                    256-byte aligned: the device copies of origin and scene_of_view, and 32 i64 per workgroup of 1024 sampled pixels
 * Invalid arguments return RELPOSE_EINVAL before anything is enqueued or any output is touched.  Two launches per evaluation whatever
 * n_views is.  The call waits for `stream` once, at its end. */
typedef struct RelposeTsdfAlignArgs {
    uint32_t struct_size;       /* sizeof(RelposeTsdfAlignArgs) as the caller compiled it */
    int32_t n_scenes;
    int32_t n_views;
    int32_t h;
    int32_t dataset;
    int32_t nx, ny, nz;
    int32_t min_weight;
    int32_t iters;
    int32_t stride;
    int32_t reserved0;
    const int32_t* tsdf_sum;
    const int32_t* weight;
    const float* depth;
    const double* pose;
    const double* origin_host;
    const int32_t* scene_of_view_host;
    double voxel;
    double eig_min;
    double* pose_out;
    double* eig;
    int32_t* held;
    int64_t* sums;
    double* rms;
    double* trace_pose;
    int64_t* trace_sums;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeTsdfAlignArgs;
size_t relpose_tsdf_align_workspace_bytes(int32_t n_scenes, int32_t n_views, int32_t h, int32_t nx, int32_t ny, int32_t nz, int32_t stride);
int relpose_tsdf_align(const RelposeTsdfAlignArgs* args);

/* What the fused model looks like from a pose: depth, normal and colour panoramas of n_views views, each marched through the volume of
 * relpose_tsdf_fuse's state it names.  The contract is the project's own (tests/render_model.py restates it in numpy, on
 * whole arrays and as a plain loop per ray).  One plain march defines every output bit; the one optimisation, skipping empty space, cannot
 * change a bit (the proof is in DESIGN.md 4.20).  The geometry is float64, every operation rounded on its own, + - * / sqrt floor only.
 * A pixel depends on its own ray and the volume alone: no atomics, bitwise repeatable, independent of the batch around a view and of skip.
 *
 *   tsdf_sum, weight [n_scenes, nz, ny, nx] i32, color_sum [n_scenes, 3, nz, ny, nx] u32 or NULL, origin_host [n_scenes, 3] f64 (HOST), voxel,
 *                    min_weight (>= 1): relpose_tsdf_fuse's state
 *   pose             [n_views, 4, 4] f64 row-major on the DEVICE, world -> camera (the last row is not read)
 *   scene_of_view_host [n_views] i32 in HOST memory, each in 0 .. n_scenes-1: several views may name one volume, a volume may have none
 *   ray              pixel (row, col) of the [h, 4h] panorama: slot = col / h, px = col - slot h, xn = (2.0 * px) / h - 1.0,
 *                    yn = 1.0 - (2.0 * row) / h, dir = Rs[face(dataset, slot)] (xn, yn, -1) (a signed permutation: exact): the ray
 *                    relpose_tsdf_align unprojects.  Column 0 of a slot and row 0 lie on the face's open edge (xn = -1, yn = 1); they are
 *                    rendered like any other pixel, as alignment uses them.  W = the rigid inverse of the pose as relpose_tsdf_align
 *                    writes it out.  Sample k (0 <= k < n_steps) lies at face depth d_k = d_min + (double)k * step: the camera point
 *                    (x, y, z) = (d_k dir_0, d_k dir_1, d_k dir_2), the world point q_a = ((W_a0 x + W_a1 y) + W_a2 z) + W_a3.
 *   sample           u_a = (q_a - origin_a) / voxel - 0.5, i0_a = floor(u_a), f_a = u_a - i0_a.  The sample is IN RANGE iff q is finite and
 *                    0 <= i0_a <= n_a - 2 on every axis; it is VALID iff it is in range, it is evaluated (below) and each of the 8 corners
 *                    i0 + (c & 1, c >> 1 & 1, c >> 2 & 1) has weight >= min_weight.  Its value t is the trilinear interpolation of
 *                    t_c = (double)tsdf_sum / (32768.0 * (double)weight) and its gradient g = (gx, gy, gz), in relpose_tsdf_align's order:
 *                      d00 = t1 - t0, d10 = t3 - t2, d01 = t5 - t4, d11 = t7 - t6;  a00 = t0 + fx d00, a10 = t2 + fx d10, a01 = t4 + fx d01,
 *                      a11 = t6 + fx d11;  c0 = a10 - a00, c1 = a11 - a01;  b0 = a00 + fy c0, b1 = a01 + fy c1;
 *                      gz = b1 - b0;  t = b0 + fz gz;  gy = c0 + fz (c1 - c0);  e0 = d00 + fy (d10 - d00), e1 = d01 + fy (d11 - d01);
 *                      gx = e0 + fz (e1 - e0).      A corner with |t_c| >= 1 (saturated) is an ordinary value here.
 *                    The colour of a sample is the same rule for t on c_c = (double)color_sum / (255.0 * (double)weight), per channel.
 *   march            for k = 1, 2, .. n_steps-1 the FIRST pair (k-1, k) of valid samples with t_{k-1} >= 0 && t_k < 0 or
 *                    t_{k-1} < 0 && t_k >= 0 ends the ray.  The first: a HIT, cls = 1, s = t_{k-1} / (t_{k-1} - t_k),
 *                    depth = (float)(d_{k-1} + s * step); the normal is n = g_{k-1} + s * (g_k - g_{k-1}) per component, divided by
 *                    sqrt((nx nx + ny ny) + nz nz) unless that is 0, then rotated into the camera frame by the pose's rotation
 *                    R_ij = W_ji, (float)((R_i0 nx + R_i1 ny) + R_i2 nz): the frame relpose_depth_normals writes; it points where t grows,
 *                    towards the space the sensors saw through.  colour = (float)(c_{k-1} + s * (c_k - c_{k-1})) per channel.
 *                    The second: a BACK FACE, cls = 2: the ray left a solid, no data.  No such pair: a MISS, cls = 0.  A pair with a
 *                    sample that is not valid never ends a ray: no surface is invented across unknown space.  Without a hit depth,
 *                    normal and colour are 0: depth 0 is "no data", the rule of every consumer of a depth panorama.
 *   skip             0: every in-range sample is evaluated (its sixteen loads are made).  1: a first launch sets one flag byte per brick
 *                    of 8 x 8 x 8 cells (cell i0 lies in brick i0 / 8 per axis) iff one of the brick's cells has a corner voxel with
 *                    weight >= min_weight and tsdf_sum < 0; an in-range sample k is evaluated iff the cell of sample k-1, k or k+1 (those
 *                    of them that exist, 0 .. n_steps-1, and are in range) lies in a flagged brick.  Every output but n_evaluated is bit for
 *                    bit what skip = 0 gives.
 *   outputs          depth [n_views, h, 4h] f32; cls [n_views, h, 4h] u8; optional (NULL: not written) normal [n_views, 3, h, 4h] f32,
 *                    color [n_views, 3, h, 4h] f32 (needs color_sum), n_evaluated [n_views, h, 4h] i32: the number of samples evaluated
 *                    up to and including the one that ended the ray, under the mode in force.
 *   limits           relpose_tsdf_fuse's for h, n_views and the volume; 3 nx ny nz < 2^31; d_min >= 0 and step > 0, both finite;
 *                    1 <= n_steps <= 65536; skip 0 or 1; min_weight >= 1; voxel finite > 0; origin finite.  A volume with a dimension of 1
 *                    has no cells: every pixel is a miss.  A pose with a NaN or an inf makes every world point non-finite: all misses.
 *   workspace        relpose_tsdf_render_workspace_bytes(n_scenes, n_views, h, nx, ny, nz) bytes (0 for sizes outside the limits), 256-byte
 *                    aligned: the device copies of origin and scene_of_view, and the brick flags
 * The kernels restrict each march to a conservative clip of the ray against the box; samples outside it are out of range, so the plain
 * loop above stays the definition.  Invalid arguments return RELPOSE_EINVAL before anything is enqueued or any output is touched.  One
 * launch, two with skip, whatever n_views is.  The call waits for `stream` once, at its end. */
typedef struct RelposeTsdfRenderArgs {
    uint32_t struct_size;       /* sizeof(RelposeTsdfRenderArgs) as the caller compiled it */
    int32_t n_scenes;
    int32_t n_views;
    int32_t h;
    int32_t dataset;
    int32_t nx, ny, nz;
    int32_t min_weight;
    int32_t n_steps;
    int32_t skip;
    int32_t reserved0;
    const int32_t* tsdf_sum;
    const int32_t* weight;
    const uint32_t* color_sum;
    const double* pose;
    const double* origin_host;
    const int32_t* scene_of_view_host;
    double voxel;
    double d_min;
    double step;
    float* depth;
    uint8_t* cls;
    float* normal;
    float* color;
    int32_t* n_evaluated;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposeTsdfRenderArgs;
size_t relpose_tsdf_render_workspace_bytes(int32_t n_scenes, int32_t n_views, int32_t h, int32_t nx, int32_t ny, int32_t nz);
int relpose_tsdf_render(const RelposeTsdfRenderArgs* args);

/* -------------------------------------------------------------------- robust synchronisation of pose graphs
 * The pair drivers give a relative pose per pair of views; some are grossly wrong.  relpose_pose_sync turns the relative poses of n_scenes
 * scenes into one absolute pose per view and one confidence per relative pose: graduated Geman-McClure re-weighting around a linearised
 * rotation and translation averaging, initialised on a maximum-weight spanning tree.  The contract is the project's own (DESIGN.md 4.17;
 * tests/sync_model.py restates it in numpy, on whole arrays and as plain loops).  The geometry is float64, every operation rounded on its
 * own; no atomics, no eigen-solver, no stopping rule: the number of iterations is known at launch.  One workgroup per scene, one launch.
 * Invalid arguments return RELPOSE_EINVAL before anything is enqueued or any output is touched.
 *
 *   layout           scene s owns the views view_begin[s] .. view_begin[s+1]-1 and the edges edge_begin[s] .. edge_begin[s+1]-1; both
 *                    [n_scenes + 1] i32 in HOST memory, ascending from 0 to n_views / n_edges.  At most 64 views and 4096 edges per scene;
 *                    a scene may have no views or no edges.  1 <= n_scenes < 2^24.
 *   edges            src, dst [n_edges] i32, view indices LOCAL to the scene; T [n_edges, 4, 4] f64 row-major, T ~ X_dst inv(X_src) for world ->
 *                    camera poses X (what the pair drivers produce: R_gt = R_t inv(R_s), evaluation.py:227; the bottom row is not read);
 *                    w0 [n_edges] f64, the prior weight.  Several edges may join the same two views.
 *   edge_state       [n_edges] i32: 0 = used, else the edge is ignored and the code is the FIRST of: RELPOSE_SYNC_BAD_INDEX (src or dst outside
 *                    0 .. M-1), RELPOSE_SYNC_SELF_EDGE (src == dst), RELPOSE_SYNC_BAD_WEIGHT (w0 not finite or <= 0), RELPOSE_SYNC_BAD_POSE (an
 *                    entry of T's top three rows not finite).  The other outputs are what they are without the ignored edges.
 *   components       M steps of Prim: each adds the used edge of largest w0 (ties: the smaller index) that joins a visited and an unvisited
 *                    view and marks it in tree [n_edges] i32; where none does, the smallest unvisited view starts a component and is its
 *                    gauge (pose = identity).  component [n_views] i32: the smallest view index (local) connected to the view by used
 *                    edges.  n_components [n_scenes] i32.
 *   state            per view R (3x3) and u = R^T t; every 3x3 product entry is (a0 b0 + a1 b1) + a2 b2.  Along a tree edge from a visited
 *                    src i: R_j = R_ij R_i, u_j = u_i + R_j^T t_ij; from a visited dst j: R_i = R_ij^T R_j, u_i = u_j - R_j^T t_ij.
 *   schedule         mu = mu0; after every iteration mu = fmax(mu / div, 1.0).  The iterations with mu > 1 run, then n_final more at
 *                    mu = 1 (defaults 64, 1.4, 10: 13 + 10).  More than RELPOSE_SYNC_MAX_ITERATIONS in total is RELPOSE_EINVAL.
 *   iteration        1. per used edge: omega = log(R_j^T (R_ij R_i)), rho = R_j^T t_ij - (u_j - u_i).
 *                    2. conf = 1 / (q q), q = 1 + (|omega|^2 / sigma_r^2 + |rho|^2 / sigma_t^2) / mu^2 (robust = 0: conf = 1); w = w0 conf.
 *                    3. L = the graph Laplacian of w, the rows and columns of the gauge views replaced by the identity (which leaves the
 *                       other entries what they are with those rows removed); row v is summed along v's adjacency list, its used edges
 *                       in ascending index: L_vv = sum w, L_vo = 0 - w - w .., b_v = sum of +w omega where v is the edge's dst, -w omega
 *                       where it is its src (0 for a gauge).  Right-looking Cholesky of the lower triangle (column k: d_k = sqrt(L_kk),
 *                       l_ik = L_ik / d_k, L_ij -= l_ik l_jk for k < j <= i), then both substitutions column by column
 *                       (x_k = y_k / d_k, y_i -= l_ik x_k): L d = b.  R_v = R_v exp(d_v) for every non-gauge view.
 *                    4. with the new rotations, the same factor solves L u = b' with b' summed like b from R_j^T t_ij.
 *   log              v = (E21 - E12, E02 - E20, E10 - E01), n = |v|, c = ((E00 + E11 + E22) - 1) / 2, th = atan2(n / 2, c), omega = v (th / n).
 *                    n < 1e-6 and c > 0: omega = v / 2.  n < 1e-6 and c <= 0 (near pi): the axis from the symmetric part, at the first
 *                    largest diagonal entry k a_k = sqrt(max((E_kk - c) / (1 - c), 0)), a_m = (E_km + E_mk) / ((2 (1 - c)) a_k), negated if
 *                    a . v < 0; omega = th a.
 *   exp              th^2 = |d|^2; A = sin(th) / th, B = (2 sin(th / 2)^2) / th^2; th^2 < 1e-8: A = 1 - th^2 / 6, B = 0.5 - th^2 / 24;
 *                    X = I + A [d]x + B [d]x^2 entry by entry: X00 = 1 - B (d1 d1 + d2 d2), X01 = B (d0 d1) - A d2, X02 = B (d0 d2) + A d1, ..
 *   outputs          pose [n_views, 4, 4] f64 world -> camera in its component's gauge: [R | R u; 0 0 0 1].  confidence [n_edges] f64: conf
 *                    of the last iteration (1 if none ran), 0 for ignored edges.  res_rot, res_trans [n_edges] f64: |omega|, |rho| under
 *                    the final poses, NaN for ignored edges.  cost [n_scenes] f64: sum of w0 r^2 / (1 + r^2) under the final poses with
 *                    mu = 1 (robust = 0: w0 r^2), per view over the edges it is the dst of in ascending index, then over the views in
 *                    ascending order.  last_step [n_scenes] f64: the largest |component of d| of the last iteration (0 if none ran).
 *   determinism      a scene's result is bitwise repeatable and does not depend on the batch around it or its place in it.
 *   degenerate       weights that underflow to 0 around a view make L singular there: the poses of that component are then NaN.
 *   workspace        relpose_pose_sync_workspace(n_scenes, n_views, n_edges) bytes (0 outside the limits), 256-byte aligned: the device
 *                    copies of the offsets, the weights and residuals per edge and the adjacency lists.
 * The call waits for `stream` once, at its end: the host arrays are the caller's again when it returns. */
enum { RELPOSE_SYNC_MAX_VIEWS = 64, RELPOSE_SYNC_MAX_EDGES = 4096, RELPOSE_SYNC_MAX_ITERATIONS = 100000 };
enum { RELPOSE_SYNC_USED = 0, RELPOSE_SYNC_BAD_INDEX = 1, RELPOSE_SYNC_SELF_EDGE = 2, RELPOSE_SYNC_BAD_WEIGHT = 3, RELPOSE_SYNC_BAD_POSE = 4 };
typedef struct RelposePoseSyncArgs {
    uint32_t struct_size;       /* sizeof(RelposePoseSyncArgs) as the caller compiled it */
    int32_t n_scenes;
    int32_t n_views;            /* over all scenes */
    int32_t n_edges;            /* over all scenes */
    int32_t n_final;
    int32_t robust;             /* 1: Geman-McClure, 0: plain least squares */
    int32_t reserved0, reserved1;
    const int32_t* view_begin_host;
    const int32_t* edge_begin_host;
    const int32_t* src;
    const int32_t* dst;
    const double* T;
    const double* w0;
    double sigma_r, sigma_t;    /* radians, metres: finite, > 0 */
    double mu0, div;            /* mu0 >= 1, div > 1 */
    double* pose;
    int32_t* component;
    int32_t* tree;
    int32_t* edge_state;
    double* confidence;
    double* res_rot;
    double* res_trans;
    int32_t* n_components;
    double* cost;
    double* last_step;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} RelposePoseSyncArgs;
size_t relpose_pose_sync_workspace(int32_t n_scenes, int32_t n_views, int32_t n_edges);
int relpose_pose_sync(const RelposePoseSyncArgs* args);

/* -------------------------------------------------------------------- SCNet
 * Replaces SCNet (model/mymodel.py:141-380).  relpose_scnet_create builds the configuration evaluation.py runs
 * (skipLayer=1, batchnorm=1, outputType 'rgbdnsf'); relpose_scnet_create_ex (round 6) the other constructor variants. */
typedef struct RelposeSCNet RelposeSCNet;

RelposeSCNet* relpose_scnet_create(int32_t snumclass, int32_t use_tanh);
void relpose_scnet_destroy(RelposeSCNet* net);

/* The reference constructor's switches (model/mymodel.py:145-149, 189-243: args.batchnorm, args.skipLayer, args.outputType).
 *   batchnorm   1: conv -> BatchNorm(batch statistics) -> LeakyReLU (mymodel.py:16-21); 0: conv + bias -> LeakyReLU (:22-25;
 *               state-dict keys "<block>.0.bias" instead of "<block>.1.weight|bias").
 *   skip_layer  1: every decoder block also reads the encoder activation of its resolution (:302-307); 0: the plain chain (:335-340).
 *   output_mask which heads exist, RELPOSE_OUT_* bits in the reference's concatenation order rgb, n, d, s, f (:309-376).  A head that
 *               was not constructed has no parameters and its decoder branch does not run.
 * NULL for what the reference cannot run either: skip_layer = 0 with any of rgb / n / d (their 1x1 output convs always take 64
 * input channels, 32 of them the skip: the reference fails inside torch, mymodel.py:192 vs :347) and the 'k' head (reads an
 * undefined `xsift`, :328).
 * The forward's `out` keeps the layout [n, 7 + snumclass + 32, H, W] for every variant: the channels of a head that does not
 * exist are 0 (the reference concatenates only the existing heads; relativepose_amd.model.SCNet gathers them).  Variants run the
 * same kernels under the plain launch plan on ONE stream: RELPOSE_FWD_ZERO_WARP / _POSE_OUTPUTS, `self_tag` and `tail_stream`
 * are accepted and ignored (each is "bitwise the plain forward" by contract). */
enum { RELPOSE_OUT_RGB = 1, RELPOSE_OUT_N = 2, RELPOSE_OUT_D = 4, RELPOSE_OUT_S = 8, RELPOSE_OUT_F = 16, RELPOSE_OUT_ALL = 31 };
typedef struct RelposeSCNetConfig {
    uint32_t struct_size;       /* sizeof(RelposeSCNetConfig) as the caller compiled it */
    int32_t snumclass, use_tanh;
    int32_t batchnorm, skip_layer, output_mask;
} RelposeSCNetConfig;
RelposeSCNet* relpose_scnet_create_ex(const RelposeSCNetConfig* cfg);

/* One state_dict entry (key names = the reference module tree, e.g. "conv4.0.weight",
 * "deconv3rgb.1.bias", "deconv1f.weight"); data_host float32 in torch layout. */
int relpose_scnet_set_param(RelposeSCNet* net, const char* key, const float* data_host, size_t numel);
/* Pack + upload once all keys are set; returns <0 and lists nothing if a key is missing. */
int relpose_scnet_finalize(RelposeSCNet* net);
int64_t relpose_scnet_num_params(const RelposeSCNet* net);

/* Arithmetic of the implicit-GEMM convolutions.  RELPOSE_PREC_F32 (default): exact fp32 products on
 * v_mfma_f32_32x32x2_f32 -- the parity configuration.  RELPOSE_PREC_BF16X3 (opt-in): both operands are split
 * into bfloat16 hi + lo and a*b ~= hi*hi + hi*lo + lo*hi runs on v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation (products exact to ~2^-16 instead of 2^-24; activations, BatchNorm statistics, conv1 and the heads
 * stay fp32).  RELPOSE_PREC_F16X3 (opt-in): the same with float16 halves (11 + 11 mantissa bits: products exact to
 * ~2^-21 for O(1) operands; float16 range, so inputs must stay below 65504).  RELPOSE_PREC_F16 (opt-in): plain float16 products
 * (the hi halves only, one v_mfma_f32_32x32x16_f16 per product, fp32 accumulation and fp32 BatchNorm statistics: SURVEY 8d
 * config 5's "fp16 MFMA convs"; products exact to 2^-11).
 * RELPOSE_PREC_BF16X9 (round 6): EXACT fp32 products on the bf16 matrix pipe -- every fp32 operand is cut into three bfloat16
 * pieces (8 + 8 + 8 = 24 significand bits: a = a1 + a2 + a3 exactly, fp32 exponent range), all nine partial products
 * ai * bj (each exact in the fp32 accumulator) are issued as v_mfma_f32_32x32x16_bf16, smallest first, fp32 accumulation:
 * the arithmetic of the fp32 MFMA path (exact products, fp32 sums in another order) at 9/16 of its matrix-pipe cycles.
 * RELPOSE_PREC_BF16X6: the same without the three smallest partial products a2 b3, a3 b2, a3 b3: what is dropped is at most 2^-23 |a b| (two terms of
 * <= 2^-24 |a b|), observed maximum 2^-24.3 and rms 2^-27.4 over 2e6 random float32 pairs -- a correctly rounded fp32 multiply errs by up to 2^-24 |a b| with an rms
 * of 2^-25.2 (tests/test_split_arithmetic_cpu.py): the size of one fp32 rounding per product, where the fp32 accumulation that follows rounds once per product anyway.
 * May be switched at any time after finalize. */
enum { RELPOSE_PREC_F32 = 0, RELPOSE_PREC_BF16X3 = 1, RELPOSE_PREC_F16X3 = 2, RELPOSE_PREC_F16 = 3, RELPOSE_PREC_BF16X9 = 4, RELPOSE_PREC_BF16X6 = 5 };
int relpose_scnet_set_precision(RelposeSCNet* net, int32_t mode);

size_t relpose_scnet_workspace_bytes(const RelposeSCNet* net, int32_t n_images, int32_t H, int32_t W);

/* forward: x [n,16,H,W] -> out [n,7+S+32,H,W]; n even, BatchNorm statistics over each
 * consecutive group of 2 images (the reference always feeds batch 2, evaluation.py:242).
 * Replaces the reference call `f = net(x)` (evaluation.py:242, rpmodule.py:623; SCNet.forward, model/mymodel.py:259-380). */
int relpose_scnet_forward(RelposeSCNet* net, const float* x, float* out, int32_t n_images, int32_t H, int32_t W,
                          void* workspace, size_t workspace_bytes, void* stream);

/* The same forward with every option of the serving loop, in ONE struct_size-versioned argument block (round 5; round 6 removed the
 * accreted relpose_scnet_forward2 / 3 / 4 exports, which were thin wrappers filling this block).
 *   struct_size           sizeof(RelposeForwardArgs) as the CALLER compiled it: fields beyond it take their defaults (0), so the block can grow
 *   x, out, n_images, H, W, workspace, workspace_bytes, stream   as relpose_scnet_forward
 *   tail_stream           NULL = `stream`.  Otherwise the HBM-bound ends of the forward -- the head (input resize mymodel.py:261 + conv1*
 *                         :266-286) and the tail (the five 1x1 heads deconv1* :312-376 + the final resize :379) -- are enqueued on `tail_stream` and
 *                         the MFMA-bound middle on `stream`, ordered by events: `stream` is busy with this forward only between conv2 and deconv2,
 *                         so the next forward -- of ANOTHER workspace -- overlaps its convolutions with this head / tail
 *                         (pipeline.run_pipelined).  x is read and `out` written on tail_stream only.
 *   flags                 RELPOSE_FWD_ZERO_WARP: the caller guarantees that channels 8:16 of EVERY image are zero -- level 0 of the recurrence,
 *                         where the pose estimate is the identity and util.warping returns zeros (util.py:95-96, evaluation.py:232-236).  The
 *                         three warped-view encoder streams (conv1*..conv3* on rgb_t2s / norm_t2s / depth_t2s, mymodel.py:278-288) then produce
 *                         the same activations for every image, so they run for the first BatchNorm group only: results are bitwise those of
 *                         the flag-less forward.  With the flag set and a non-zero warped view the output is undefined.
 *                         RELPOSE_FWD_POSE_OUTPUTS: compute only the outputs the pose path consumes -- normal (channels 3:6), depth (6) and the
 *                         32 feature channels (7+S:), evaluation.py:246-253 / rpmodule.py:629-636 -- and skip the decoder branches that feed
 *                         nothing else (deconv3/2/1 of the rgb and semantic heads, mymodel.py:312-316,364-368); channels 0:3 and 7:7+S of `out`
 *                         are written as zeros, the others are bitwise those of the full forward.  Opt-in; never the default.
 *                         RELPOSE_FWD_NEW_WORKSPACE: the caller (re)allocated the workspace since its last forward -- possibly at the same
 *                         address --: whatever self-stream cache the library associates with the pointer is dropped before this forward.
 *   self_tag              the self-stream cache.  Inside one scan pair's recurrence (evaluation.py:217-242) the masked own views -- channels 0:8
 *                         of every image -- never change between the levels, only the warped partner view (channels 8:16) does, and the
 *                         reference runs the self-view encoder streams as module calls of their own with their own batch statistics
 *                         (conv1/2/3{rgb,n,d} on x[:,0:8], mymodel.py:266-276; the warped-view calls are :278-288).  `self_tag` names the
 *                         content of channels 0:8: when it is non-zero and equal to the tag (and n, H, W) of the PREVIOUS forward on this
 *                         workspace, the self-view blocks of conv1 / conv2 / conv3, their BatchNorm scale / shift, conv4's three self K slices
 *                         and the skip-connection halves of the decoder are taken from the workspace instead of being recomputed -- bitwise the
 *                         values the full forward would produce.  Any other tag (or 0) runs the full forward and leaves the cache filled.
 *                         Contract: two forwards on one workspace that carry the same non-zero tag have identical channels 0:8 (the caller
 *                         draws a fresh tag whenever it rewrites them); set_param / finalize / set_precision drop the cache.
 *                         RELPOSE_FWD_ZERO_WARP forwards always compute (and cache) the self streams.
 *                         The flags of the forward that filled the cache do not matter.  Everything head-independent (the self members of
 *                         conv1-3, their scale / shift, conv4's self slices and row maps) is taken from the workspace whichever outputs the
 *                         filling forward computed; the skip-connection halves are kept per skip head (rgb, n, d), each in a slot of its own,
 *                         and the record says which heads the filling forward stored.  A forward WITHOUT RELPOSE_FWD_POSE_OUTPUTS behind a
 *                         fill WITH it (the last level of a step whose earlier levels asked for the pose outputs only) is therefore cached
 *                         too: it takes the n and d halves from the workspace and computes the rgb head's halves (deconv3rgb, deconv2rgb, the
 *                         rgb lines of the 1x1 heads) in the full forward's order, storing nothing.  Cached forwards never change the record,
 *                         and a pose-outputs forward never writes an rgb slot: full, pose, full under one tag -> the third forward still
 *                         starts from the first one's rgb halves.  Every such forward is bitwise the tag-less full forward of its input.
 *   workspace_generation  the caller's name for THIS ALLOCATION of `workspace` (e.g. a counter bumped whenever the buffer is re-allocated),
 *                         sent with every call: the self-stream cache is used only when the previous forward on the pointer carried the
 *                         same generation -- a workspace re-created at a recycled address is never mistaken for the old one, whichever call
 *                         touches it first (RELPOSE_FWD_NEW_WORKSPACE needs the first call to carry the flag).  0 = not tracked.
 *   reserved1             must be NULL (a non-NULL value, like an unknown flag bit, returns RELPOSE_EINVAL before anything is enqueued).
 * Error behaviour: a call that returns != 0 leaves no self-stream record on the workspace (the next forward recomputes everything); a
 * self-cached plan that cannot be built falls back to the full forward (same output) instead of failing.
 *
 * RELPOSE_FWD_SAMPLED_OUTPUTS (with sample_pts, sample_npts, sample_npts_max): the pose-outputs forward for a caller that only SAMPLES its
 * output at keypoints (relpose_sample_primitives with the same pts / npts / npts_max; W must be 4 H).  The plan is the pose-outputs plan up
 * to and including deconv2 and its BatchNorm statistics (dense); in place of the dense 1x1 heads and the output resize one kernel writes,
 * for every image and every keypoint k < sample_npts[img], exactly the elements of `out` that relpose_sample_primitives loads:
 *   channels 3:7 at (ty .. ty + 1, tx .. tx + 1) and channels 7+S : 7+S+32 at (yi .. yi + 1, xi .. xi + 1)
 * (tx, ty, xi, yi as csrc/sample_pixels.h derives them from the keypoint), each bit for bit the value of the RELPOSE_FWD_POSE_OUTPUTS
 * forward -- also where the keypoint lies inside the observed box (the sampler multiplies the network value by 0 there, which keeps a NaN).
 * EVERY OTHER ELEMENT OF `out` IS UNSPECIFIED after such a forward (it keeps whatever it held).  sample_pts (double [n, npts_max, 2], pixel
 * coordinates) and sample_npts (int32 [n]) are device arrays read by that kernel on every call, on tail_stream when there is one; entries
 * k >= sample_npts[img] are never read; a block pixel outside the map is not written.  A constructor variant ignores the flag like
 * RELPOSE_FWD_POSE_OUTPUTS (the plain dense forward).  Self-stream cache: a sampled forward stores no accumulator snapshot of the 1x1
 * heads and, when it fills the cache, records none -- a snapshot an earlier tag left in the workspace is never picked up: a later forward
 * of its tag that runs the dense heads computes the skip lines of rgb, n and d from A1 (whose self blocks stay in the workspace), bitwise the
 * same output; the deconv3 / deconv2 snapshots are stored and used as by a pose-outputs forward.  relpose_scnet_last_tail tells which tail ran. */
enum { RELPOSE_FWD_ZERO_WARP = 1, RELPOSE_FWD_POSE_OUTPUTS = 2, RELPOSE_FWD_NEW_WORKSPACE = 4, RELPOSE_FWD_SAMPLED_OUTPUTS = 32 };   /* (8 and 16 named a removed form and stay invalid) */
typedef struct RelposeForwardArgs {
    uint32_t struct_size;
    int32_t flags;
    const float* x;
    float* out;
    int32_t n_images, H, W, reserved0;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
    void* tail_stream;
    uint64_t self_tag;
    uint64_t workspace_generation;
    void* reserved1;
    const double* sample_pts;        /* RELPOSE_FWD_SAMPLED_OUTPUTS: device, [n_images, sample_npts_max, 2] */
    const int32_t* sample_npts;      /* device, [n_images] */
    int32_t sample_npts_max, reserved2;
} RelposeForwardArgs;
int relpose_scnet_forward_ex(RelposeSCNet* net, const RelposeForwardArgs* args);

/* Which tail the last forward of `net` ran: 0 = the dense 1x1 heads and output resize, 1 = the sampled tail (RELPOSE_FWD_SAMPLED_OUTPUTS),
 * -1 = no forward yet.  Host-only.  For tests and profiles. */
int relpose_scnet_last_tail(RelposeSCNet* net);

/* Multiply-accumulates one forward of a plan family executes (host-only, no device access): flags as above, self_cached != 0 = the plan
 * a forward takes when it finds its self_tag on the workspace: 1 = behind a fill that stored every skip head's halves, 2 = behind a
 * pose-outputs fill (no rgb halves in the workspace: a forward without RELPOSE_FWD_POSE_OUTPUTS computes them, and they are counted; with
 * the flag 2 counts what 1 does), 3 = behind a sampled-outputs fill (no snapshot of the 1x1 heads either: their skip lines are counted).
 * RELPOSE_FWD_SAMPLED_OUTPUTS counts the pose-outputs plan without the 1x1 heads (the sampled tail's few multiply-adds depend on the
 * keypoint count and are left out).  The full forward (flags 0, self_cached 0) counts every member of
 * model/mymodel.py:259-380; the level-0 plan and the self-stream cache count what they really launch.  bench.py divides the two for
 * its plan-aware in-loop roofline ("roofline.in_loop").  It is the STATIC plan that is counted: the patches and rows that the zero-tile lists
 * and conv4's row lists drop depend on the input and stay counted (relpose_scnet_zero_tiles / relpose_scnet_conv4_rows report them). */
int relpose_scnet_plan_macs(RelposeSCNet* net, int32_t n_images, int32_t flags, int32_t self_cached, double* macs_host);

/* Which kernel the plain plan of n_images runs `layer` ("deconv4", ...) on under the current precision and tuning knobs (host-only, a dry-run
 * plan build): 1 = the phase strip kernel (deconv_strip_kernel) as a split-K launch, 2 = that kernel unsplit (direct stores and fused
 * BatchNorm records), 0 = another kernel, <0 = invalid argument or unknown layer.  For tests that
 * compare the two arms of RELPOSE_TUNE_DECONV_STRIP. */
int relpose_scnet_layer_kernel(RelposeSCNet* net, const char* layer, int32_t n_images);

/* Workgroups the conv2 / conv3 tile kernels of the last forward computed and dropped (RELPOSE_TUNE_ZERO_TILES): counts_host[4] =
 * {conv2 computed, conv2 dropped, conv3 computed, conv3 dropped}, in workgroups (conv2: one 16 x 16 patch, conv3: a pair of 8 x 8
 * patches), summed over the launch members of that forward's plan.  Synchronises `stream` (the forward's).  For tests and profiles. */
int relpose_scnet_zero_tiles(RelposeSCNet* net, void* workspace, void* stream, int64_t* counts_host);

/* conv1's zero units in the last forward (RELPOSE_TUNE_CONV1_ZERO): counts_host[3] = {launched, skipped without a store, stored as zeros},
 * in (image, stream, 8 x 32 tile) blocks of A1; the last two are 0 when conv1 computed every block (the knob set, no zero-tile lists, or a
 * non-finite conv1 weight).  occ_host, if not NULL, receives that forward's occupancy words [n_images][6][28] (RELPOSE_EINVAL if it ran
 * without the zero-tile lists).  Synchronises `stream` (the forward's).  For tests and profiles. */
int relpose_scnet_conv1_zero(RelposeSCNet* net, void* workspace, void* stream, int64_t* counts_host, uint32_t* occ_host);

/* conv4's rows in the last forward (RELPOSE_TUNE_CONV4_ROWS): counts_host[18] = per K slice ks = encoder stream ks {rows computed, rows
 * dropped (read from their representative by the split-K reduce), 1 if the slice ran on the row-list launch else 0}.  A slice on the strip
 * kernel computes all its rows (a shared slice of the level-0 plan has 2 x 784); a slice the self-stream cache did not compute reports
 * {0, 0, 0}.  counts_host[0] = -1 (the rest 0) if the forward ran without row lists.  Synchronises `stream`.  For tests and profiles. */
int relpose_scnet_conv4_rows(RelposeSCNet* net, void* workspace, void* stream, int64_t* counts_host);

/* Debug: copy a raw (pre-BatchNorm) layer output of the last forward, NHWC float32, to out (device).
 * Returns the number of floats written (or needed if out is NULL), <0 if unknown. */
int64_t relpose_scnet_read_tap(RelposeSCNet* net, const char* layer, float* out, void* workspace, void* stream);

/* Per-kernel timing of the conv stack for the bench roofline (HIP events on `stream`):
 * runs `iters` forwards and returns mean ms of the implicit-GEMM kernels and of everything else. */
int relpose_scnet_profile(RelposeSCNet* net, const float* x, float* out, int32_t n_images, int32_t H, int32_t W,
                          void* workspace, size_t workspace_bytes, int32_t iters,
                          double* ms_gemm_host, double* ms_other_host, int64_t* n_gemm_launches_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_H */
