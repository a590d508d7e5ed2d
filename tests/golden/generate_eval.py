#!/usr/bin/env python3
"""Generate tests/golden/depth_eval.pt and tests/golden/eval_io/ by running the REFERENCE's evaluation code on CPU.

Run in the build container only (`python tests/golden/generate_eval.py`); the GPU box has no reference tree and only reads the
committed files. What is imported from the reference, unmodified: dust3r.depth_eval.depth_evaluation (use_gpu=False),
dust3r.utils.vo_eval.sintel_cam_read / load_sintel_traj and lvdm.data.eval_dataset_geo4d.depth_read_sintel / depth_read_bonn /
depth_read_kitti, with the packages they import but never call on these paths (cv2, evo, ...) mocked by generate.py's
_mock_absent_packages.

depth_eval.pt: one synthetic sequence (T = 4 at 48 x 64: invalid pixels at 0 and below, far pixels beyond 70 / 80, a prediction that is
an affine map of the truth plus noise, partial align / custom masks) and the reference's (results, s, t, error map) for four
cases: Sintel / Bonn style (lad2, max_depth 70, post_clip_max 70, lr 1e-2, 5000 iterations, align_mask), KITTI style (lad2,
max_depth None, defaults), the default median scaling, and median scaling with pre / post clips and a custom_mask.
eval_io/: a tiny .dpt, Bonn and KITTI 16-bit PNGs and a two-frame Sintel .cam sequence, with the readers' outputs in depth_eval.pt.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate  # noqa: E402  (puts the repository and the reference on sys.path)

IO_DIR = os.path.join(HERE, "eval_io")
T, H, W = 4, 48, 64

CASES = {
    "sintel": dict(max_depth=70, align_with_lad2=True, post_clip_max=70, lr=1e-2, max_iters=5000, masks=("align_mask",), flat=True),
    "kitti": dict(max_depth=None, align_with_lad2=True, masks=(), flat=True),
    "median": dict(masks=(), flat=False),
    "median_clip": dict(max_depth=60, pre_clip_min=0.2, pre_clip_max=30.0, post_clip_min=0.5, post_clip_max=50.0,
                        masks=("custom_mask", "align_mask"), flat=False),
}


def sequence():
    g = torch.Generator().manual_seed(2024)
    gt = 0.5 + 89.5 * torch.rand((T, H, W), generator=g) ** 2                       # 0.5 .. 90: some beyond 70 and 80
    gt[torch.rand((T, H, W), generator=g) < 0.08] = 0.0                               # missing depth
    gt[torch.rand((T, H, W), generator=g) < 0.02] = -1.0                              # the readers' "missing" value
    pred = (gt.clamp(min=0.5) - 0.7) / 3.1 + 0.3 * torch.randn((T, H, W), generator=g)
    pred = pred.abs() + 1e-3
    align_mask = torch.rand((T, H, W), generator=g) < 0.8
    custom_mask = torch.rand((T, H, W), generator=g) < 0.9
    return dict(pred=pred, gt=gt, align_mask=align_mask, custom_mask=custom_mask)


def median_scale(pred, gt, kw, align_mask):
    """The reference's median-scaling factor (depth_eval.py:243 / :266), same torch ops: returned as its (s, t = 0)."""
    md = kw.get("max_depth", 80)
    m = (gt > 0) if md is None else (gt > 0) & (gt < md)
    p, t = pred[m], gt[m]
    if kw.get("pre_clip_min") is not None:
        p = torch.clamp(p, min=kw["pre_clip_min"])
    if kw.get("pre_clip_max") is not None:
        p = torch.clamp(p, max=kw["pre_clip_max"])
    if align_mask is not None:
        am = align_mask[m]
        p, t = p[am], t[am]
    return float(torch.median(t) / torch.median(p)), 0.0


def depth_cases(de, seq):
    out = {}
    for name, spec in CASES.items():
        kw = {k: v for k, v in spec.items() if k not in ("masks", "flat")}
        pred, gt = seq["pred"].clone(), seq["gt"].clone()
        masks = {k: seq[k].clone() for k in spec["masks"]}
        if spec["flat"]:                                                              # as infer_geo4d.py passes them
            pred, gt = pred.reshape(-1), gt.reshape(-1)
            masks = {k: v.reshape(-1) for k, v in masks.items()}
        elif "align_mask" in masks:                                                   # the reference reshapes only custom_mask (:177-183)
            masks["align_mask"] = masks["align_mask"].reshape(-1, W)
        lad = kw.get("align_with_lad2", False)
        res, err, _, _ = de.depth_evaluation(pred, gt, use_gpu=False, return_st=lad, **kw, **masks)
        if lad:
            s, t = res.pop("s"), res.pop("t")
        else:
            am = masks.get("align_mask")
            s, t = median_scale(pred.reshape(-1), gt.reshape(-1), kw, None if am is None else am.reshape(-1))
        out[name] = dict(kwargs=kw, masks=list(spec["masks"]), flat=spec["flat"], results=res, s=s, t=t, error_map=err.clone())
        print(name, {k: (round(v, 6) if isinstance(v, float) else v) for k, v in res.items()}, "s, t =", s, t)
    return out


def write_io_files():
    from PIL import Image
    os.makedirs(os.path.join(IO_DIR, "cams"), exist_ok=True)
    rng = np.random.default_rng(7)
    d = (0.5 + 20 * rng.random((5, 7))).astype(np.float32)
    with open(os.path.join(IO_DIR, "depth.dpt"), "wb") as f:
        np.array([202021.25], np.float32).tofile(f)
        np.array([7, 5], np.int32).tofile(f)
        d.tofile(f)
    for name, scale in (("bonn.png", 5000.0), ("kitti.png", 256.0)):
        v = np.round(rng.uniform(0.3, 8.0, (6, 5)) * scale).astype(np.uint16)
        v[0, 0], v[3, 2] = 0, 0
        Image.fromarray(v).save(os.path.join(IO_DIR, name))
    from scipy.spatial.transform import Rotation
    for i in range(2):
        K = np.array([[300.0 + i, 0, 160], [0, 301.0, 120], [0, 0, 1]])
        w2c = np.concatenate([Rotation.from_rotvec(rng.normal(size=3) * 0.3).as_matrix(), rng.normal(size=(3, 1))], 1)
        with open(os.path.join(IO_DIR, "cams", f"frame_{i + 1:04d}.cam"), "wb") as f:
            np.array([202021.25], np.float32).tofile(f)
            K.astype(np.float64).tofile(f)
            w2c.astype(np.float64).tofile(f)


def io_outputs():
    import lvdm.data.eval_dataset_geo4d as ed
    import dust3r.utils.vo_eval as vo
    M, N = vo.sintel_cam_read(os.path.join(IO_DIR, "cams", "frame_0001.cam"))
    poses, stamps = vo.load_sintel_traj(os.path.join(IO_DIR, "cams"))
    return dict(sintel=torch.from_numpy(ed.depth_read_sintel(os.path.join(IO_DIR, "depth.dpt")).copy()),
                bonn=torch.from_numpy(ed.depth_read_bonn(os.path.join(IO_DIR, "bonn.png"))),
                kitti=torch.from_numpy(ed.depth_read_kitti(os.path.join(IO_DIR, "kitti.png"))),
                cam_M=torch.from_numpy(M), cam_N=torch.from_numpy(N), traj_poses=torch.from_numpy(poses), traj_stamps=torch.from_numpy(stamps))


def main():
    generate._mock_absent_packages()
    import dust3r.depth_eval as de
    torch.manual_seed(0)
    seq = sequence()
    cases = depth_cases(de, seq)
    write_io_files()
    torch.save(dict(shape=(T, H, W), **seq, cases=cases, io=io_outputs()), os.path.join(HERE, "depth_eval.pt"))
    for f in ["depth_eval.pt"] + [os.path.join("eval_io", x) for x in sorted(os.listdir(IO_DIR))]:
        p = os.path.join(HERE, f)
        if os.path.isfile(p):
            print(f, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
