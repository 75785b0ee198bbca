"""Generate tests/golden/completion.npz from the reference (needs the reference checkout, see ref_loader.py; CPU only):

    python tests/golden/make_completion_golden.py

  contrast_<s>_*   learner.contrast_loss (mainPanoCompletion2view.py:429-455) called unbound on seeded feature maps and correspondences,
                   under np.random.seed(1000 + s); the negatives it drew (the same two np.random.choice calls under the same seed) and the
                   share of active negatives
  pose_*           the loaders' perturbed poses (datasets/SUNCG.py:358-364, :405-410) with the reference's util.randomRotation under a
                   seeded np.random
  loss_*           errG_rgb / _n / _d / _s: the L1 / CE lines sit inline in learner.step (:553-567) and cannot be called, so the same
                   torch fp32 expressions are written out here, including the [N,N,H,W] broadcast of the CE term; with and without the
                   reference's geow (apply_mask, :53-78)
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_loader  # noqa: E402

N_PAIRS, C, H, K, S = 2, 32, 8, 16, 15


def main():
    import torch
    ref = ref_loader.load()
    import mainPanoCompletion2view as main_ref
    out = {}

    # ---- contrast_loss
    valid_of = {0: [1, 1], 1: [1, 1], 2: [0, 1]}
    for s in range(3):
        rs = np.random.RandomState(s)
        fs = (0.15 * np.tanh(rs.randn(N_PAIRS, C, H, 4 * H))).astype(np.float32)
        ft = (0.15 * np.tanh(rs.randn(N_PAIRS, C, H, 4 * H))).astype(np.float32)
        idx = lambda: np.stack([rs.randint(0, 4 * H, (N_PAIRS, K)), rs.randint(0, H, (N_PAIRS, K))], -1).astype(np.float64)
        isrc, itgt = idx(), idx()
        valid = np.array(valid_of[s])
        dc = {"idxSrc": torch.from_numpy(isrc), "idxTgt": torch.from_numpy(itgt), "valid": torch.from_numpy(valid)}
        np.random.seed(1000 + s)
        fl, fl_pos, fl_neg = main_ref.learner.contrast_loss(SimpleNamespace(args=SimpleNamespace(D=0.5)), torch.from_numpy(fs), torch.from_numpy(ft), dc)
        nv = int(valid.sum())
        np.random.seed(1000 + s)
        ny = np.random.choice(range(H), K * 100 * nv)
        nx = np.random.choice(range(4 * H), K * 100 * nv)
        # the share of active negatives among the ones it drew (flat index j K 100 + k 100 + m for the j-th valid pair), in float32 numpy
        hits = total = 0
        for j, b in enumerate(np.nonzero(valid)[0]):
            src = fs[b][:, isrc[b, :, 1].astype(int), isrc[b, :, 0].astype(int)]                       # [C, K]
            sl = slice(j * K * 100, (j + 1) * K * 100)
            ngf = ft[b][:, ny[sl], nx[sl]].reshape(C, K, 100)
            d = ((src[:, :, None] - ngf) ** 2).sum(0)
            hits += int((d < np.float32(0.5)).sum())
            total += d.size
        active = hits / total
        assert 0.10 <= active <= 0.90, active
        print(f"contrast seed {s}: loss_fl_pos {float(fl_pos):.6f} loss_fl_neg {float(fl_neg):.6f} active {active:.3f}")
        out.update({f"contrast_{s}_fs": fs, f"contrast_{s}_ft": ft, f"contrast_{s}_idx_src": isrc.astype(np.int16), f"contrast_{s}_idx_tgt": itgt.astype(np.int16),
                    f"contrast_{s}_valid": valid, f"contrast_{s}_ny": ny.astype(np.int16), f"contrast_{s}_nx": nx.astype(np.int16),
                    f"contrast_{s}_loss": np.array([float(fl), float(fl_pos), float(fl_neg)], np.float32), f"contrast_{s}_active": np.float64(active)})

    # ---- perturbed poses
    from relativepose_amd import synth
    rs = np.random.RandomState(7)
    R = np.stack([np.stack([synth.random_rigid(rs), synth.random_rigid(rs)]) for _ in range(3)])       # [B,2,4,4]
    np.random.seed(77)
    Rp = np.zeros((3, 2, 4, 4))
    for b in range(3):
        for v, R_this in enumerate((np.matmul(R[b, 0], np.linalg.inv(R[b, 1])), np.matmul(R[b, 1], np.linalg.inv(R[b, 0])))):
            R_this_p = R_this.copy()
            dR = ref["util"].randomRotation(epsilon=0.1)
            R_this_p[:3, :3] = np.matmul(dR, R_this_p[:3, :3])
            R_this_p[:3, 3] += np.random.randn(3) * 0.1
            Rp[b, v] = R_this_p
    out.update(pose_R=R, pose_seed=np.int64(77), pose_perturbed=Rp)

    # ---- L1 / CE scalars (the expressions of :549-567 written out in torch fp32)
    rs = np.random.RandomState(11)
    n4 = 4
    fake = rs.randn(n4, 7 + S, H, 4 * H).astype(np.float32)
    fake[:, 7:] *= 4
    complete = rs.randn(n4, 7, H, 4 * H).astype(np.float32)
    complete[:, 6][rs.rand(n4, H, 4 * H) < 0.05] = 0
    segm = rs.randint(0, S, (n4, 1, H, 4 * H)).astype(np.uint8)
    _, tp, geow = main_ref.apply_mask(torch.from_numpy(complete).clone(), "second")
    tfake, tcomp = torch.from_numpy(fake), torch.from_numpy(complete)
    dataMask = (tcomp[:, 6:7] != 0).float()
    CEcriterion = torch.nn.CrossEntropyLoss(weight=torch.ones(S), reduce=False)
    for tag, total_weight in (("", 1 * dataMask), ("_geow", geow[:, 0:1, :, :].float() * 1 * dataMask)):
        errG_rgb = ((tfake[:, 0:3] - tcomp[:, 0:3]) * total_weight).abs().mean()
        errG_n = ((tfake[:, 3:6] - tcomp[:, 3:6]) * total_weight).abs().mean()
        errG_d = ((tfake[:, 6:7] - tcomp[:, 6:7]) * total_weight).abs().mean()
        ce = CEcriterion(tfake[:, 7:7 + S], torch.from_numpy(segm).squeeze(1).long()) * total_weight
        assert tuple(ce.shape) == (n4, n4, H, 4 * H)                   # the broadcast of :566
        errG_s = ce.mean() * 0.1
        out["loss_err" + tag] = np.array([float(errG_rgb), float(errG_n), float(errG_d), float(errG_s)], np.float32)
        print("errG" + tag, out["loss_err" + tag])
    out.update(loss_f=fake, loss_complete=complete, loss_label=segm[:, 0], loss_mask=tp.numpy().astype(np.float32)[:, 0],
               loss_geow=geow.numpy().astype(np.float32)[0, 0])
    path = os.path.join(HERE, "completion.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
