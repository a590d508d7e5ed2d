#!/usr/bin/env python3
"""Generate tests/golden/scene_export.pt by running the REFERENCE's scene-export code on CPU.

Run in the build container only (`python tests/golden/generate_scene.py`); the GPU box has no reference tree and only reads the
committed file. What is imported from the reference, unmodified: dust3r.cloud_opt.base_opt_group.clean_pointcloud and
dust3r.viz.pts3d_to_trimesh / cat_meshes, with the packages they import but never call on these paths (cv2, trimesh, ...) mocked by
generate.py's _mock_absent_packages.

scene_export.pt holds
  occl: a synthetic 6-image scene (24 x 32) whose cameras orbit a wavy back wall with a box in front that moves from frame to frame,
        so that many pixels lie in front of another view's depth; per-pixel confidences in [1, 6]; the reference's cleaned
        confidences for tol = 0.001 and tol = 0.05 (bad_conf 0) and for tol = 0.01 with bad_conf 0.5.
  order: a 4-image 8 x 8 scene of exactly representable values (identity rotations, dyadic depths, translations and focal) on which the
        reference's sequential answer differs from a one-pass "every pair against the original confidences" answer; both are stored.
  faces: three 5 x 6 images and two validity masks (random, and a structured one) with cat_meshes([pts3d_to_trimesh(...)])'s faces.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate  # noqa: E402  (puts the repository and the reference on sys.path)


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float32)


def _points(depth, c2w, f, H, W):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grid = torch.stack([xs, ys], -1).float()
    pp = torch.tensor([W / 2, H / 2])
    cam = torch.cat([depth[..., None] * (grid - pp) / f, depth[..., None]], -1)
    return cam @ c2w[:3, :3].T + c2w[:3, 3]


def _intrinsics(n, f, H, W):
    K = torch.zeros(n, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W / 2, H / 2, 1
    return K


def occluded_scene():
    """Cameras on a small arc looking at a wall at z ~ 6 with a box at z ~ 3.5 that slides right from frame to frame."""
    g = torch.Generator().manual_seed(31)
    n, H, W, f = 6, 24, 32, 28.0
    ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    c2w, depth, pts = [], [], []
    for i in range(n):
        M = torch.eye(4)
        M[:3, :3] = _rot_y(0.05 * (i - 2.5))
        M[:3, 3] = torch.tensor([0.15 * (i - 2.5), 0.03 * i, 0.05 * i])
        d = 6.0 + 0.4 * torch.sin(xs / 4.0 + 0.5 * i) + 0.3 * torch.cos(ys / 5.0)
        box = (xs >= 6 + 3 * i) & (xs < 16 + 3 * i) & (ys >= 5) & (ys < 17)
        d = torch.where(box, 3.5 + 0.05 * torch.randn((H, W), generator=g), d)
        c2w.append(M), depth.append(d), pts.append(_points(d, M, f, H, W))
    c2w = torch.stack(c2w)
    conf = 1.0 + 5.0 * torch.rand((n, H, W), generator=g)
    return dict(conf=conf, K=_intrinsics(n, f, H, W), cams=torch.linalg.inv(c2w), depth=torch.stack(depth), pts3d=torch.stack(pts))


def exact_scene(seed):
    """Identity rotations, translations in quarters, depths in {2, 3, 4, 6}, focal 8: every product and sum of the projection is exact."""
    g = torch.Generator().manual_seed(seed)
    n, H, W, f = 4, 8, 8, 8.0
    levels = torch.tensor([2.0, 3.0, 4.0, 6.0])
    c2w, depth, pts = [], [], []
    for i in range(n):
        M = torch.eye(4)
        M[:3, 3] = torch.randint(-4, 5, (3,), generator=g).float() / 4
        d = levels[torch.randint(0, 4, (H, W), generator=g)]
        c2w.append(M), depth.append(d), pts.append(_points(d, M, f, H, W))
    c2w = torch.stack(c2w)
    conf = torch.randint(1, 9, (n, H, W), generator=g).float()
    return dict(conf=conf, K=_intrinsics(n, f, H, W), cams=torch.linalg.inv(c2w), depth=torch.stack(depth), pts3d=torch.stack(pts))


def run_clean(clean, s, **kw):
    return torch.stack(clean(list(s["conf"].clone()), s["K"], s["cams"], list(s["depth"]), list(s["pts3d"]), **kw))


def one_pass(clean, s, **kw):
    """Every pair against the ORIGINAL confidences: the reference function applied per source image with the other rows untouched."""
    return torch.stack([_one_row(clean, s, i, **kw) for i in range(len(s["conf"]))])


def _one_row(clean, s, i, **kw):
    # reorder so that image i comes first: then every comparison of row i reads rows that were not cleaned yet
    order = [i] + [j for j in range(len(s["conf"])) if j != i]
    r = {k: v[order] for k, v in s.items()}
    return run_clean(clean, r, **kw)[0]


def order_case(clean):
    for seed in range(1000):
        s = exact_scene(seed)
        seq, flat = run_clean(clean, s), one_pass(clean, s)
        if not torch.equal(seq, flat) and int((seq != s["conf"]).sum()) >= 8:
            print(f"order case: seed {seed}, {int((seq != s['conf']).sum())} cleaned, {int((seq != flat).sum())} differ from one pass")
            return dict(s, seed=seed, cleaned=seq, one_pass=flat)
    raise RuntimeError("no order-dependent case found")


def face_cases(viz):
    g = torch.Generator().manual_seed(5)
    n, H, W = 3, 5, 6
    imgs = torch.rand((n, H, W, 3), generator=g).numpy()
    pts = torch.randn((n, H, W, 3), generator=g).numpy()
    structured = np.zeros((n, H, W), bool)
    structured[0, 1:4, 1:5] = True
    structured[1] = True
    structured[1, 2, 3] = False
    structured[2, :, ::2] = True
    out = {}
    for name, m in (("random", (torch.rand((n, H, W), generator=g) < 0.7).numpy()), ("structured", structured)):
        meshes = [viz.pts3d_to_trimesh(imgs[i], pts[i], m[i]) for i in range(n)]
        faces = viz.cat_meshes(meshes)["faces"]
        out[name] = dict(mask=torch.from_numpy(m.copy()), faces=torch.from_numpy(np.asarray(faces, np.int64)))
        print(f"faces[{name}]: {len(faces)}")
    return dict(shape=(n, H, W), cases=out)


def main():
    generate._mock_absent_packages()
    from dust3r.cloud_opt.base_opt_group import clean_pointcloud
    import dust3r.viz as viz
    torch.manual_seed(0)
    s = occluded_scene()
    cleaned = {}
    for tol, bad in ((0.001, 0.0), (0.05, 0.0), (0.01, 0.5)):
        cleaned[(tol, bad)] = run_clean(clean_pointcloud, s, tol=tol, bad_conf=bad)
        print(f"occl tol={tol} bad_conf={bad}: {int((cleaned[(tol, bad)] != s['conf']).sum())} of {s['conf'].numel()} cleaned")
    out = dict(occl=dict(s, cleaned=cleaned), order=order_case(clean_pointcloud), faces=face_cases(viz))
    path = os.path.join(HERE, "scene_export.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
