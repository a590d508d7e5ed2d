#!/usr/bin/env python3
"""Wall time of the scene export (geo4d_amd/scene_export.py) at 64 and 128 frames of 320 x 512.

clean_pointcloud: the HIP form (csrc/scene_export.hip, one launch per source image) against `torch_clean`, a plain-torch restatement of
the reference's double loop (dust3r/cloud_opt/base_opt_group.py:630-665: per ordered pair geotrf, round, visibility mask, boolean
gathers and the clip), both on the same GPU and the same seeded scene. The torch loop over every pair of a 128-frame clip takes long,
so at sizes above --torch-full it times the first --torch-rows source images and scales by n / rows (reported as such). The two results
are compared where the torch loop ran in full. Export: get_3D_model_from_scene(as_pointcloud=True) on a GroupAligner holding the
scene (masks, device compaction, host copy, glb write) and the mesh-face compaction alone. Prints one JSON line.
usage: scene_export_bench.py [--frames 64 128] [--torch-rows 16] [--torch-full 64]"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geo4d_amd import ops, scene_export  # noqa: E402
from geo4d_amd.align import GroupAligner  # noqa: E402


@torch.no_grad()
def torch_clean(conf, K, cams, depth, pts3d, tol=0.001, bad_conf=0, rows=None):
    """The reference's clean_pointcloud loop restated in torch ([n, ...] tensors on any device): geotrf(cams[j], pts) as a matmul + the
    translation, geotrf(K[j], ., norm=1, ncol=2), round, the visibility mask, boolean gathers, clip. `rows`: only these source images."""
    res = conf.clone()
    n, H, W = conf.shape
    for i in (range(n) if rows is None else rows):
        pts = pts3d[i]
        for j in range(n):
            if i == j:
                continue
            T = cams[j].swapaxes(-1, -2)
            proj = (pts @ T[:-1, :] + T[-1:, :])[..., :3]
            proj_depth = proj[:, :, 2]
            kp = proj @ K[j].swapaxes(-1, -2)
            kp = kp / kp[..., -1:]
            u, v = kp[..., :2].round().long().unbind(-1)
            msk_i = (proj_depth > 0) & (0 <= u) & (u < W) & (0 <= v) & (v < H)
            msk_j = v[msk_i], u[msk_i]
            bad = (proj_depth[msk_i] < (1 - tol) * depth[j][msk_j]) & (res[i][msk_i] < res[j][msk_j])
            bad_i = msk_i.clone()
            bad_i[msk_i] = bad
            res[i][bad_i] = res[i][bad_i].clip_(max=bad_conf)
    return res


def synthetic_scene(n, H, W, dev, seed=0):
    """Cameras on an arc round a wavy wall with a sliding box in front (the shape of tests/golden/generate_scene.py's occluded scene)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    f = 0.9 * max(H, W)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    i = torch.arange(n, dtype=torch.float32).view(n, 1, 1)
    depth = 6.0 + 0.4 * torch.sin(xs / 40.0 + 0.1 * i) + 0.3 * torch.cos(ys / 50.0)
    x0 = (0.2 * W + 0.4 * W * i / n)
    box = (xs >= x0) & (xs < x0 + 0.3 * W) & (ys >= 0.25 * H) & (ys < 0.7 * H)
    depth = torch.where(box, torch.full_like(depth, 3.5), depth)
    a = 0.3 * (i.view(n) / n - 0.5)
    c2w = torch.eye(4).repeat(n, 1, 1)
    c2w[:, 0, 0], c2w[:, 0, 2], c2w[:, 2, 0], c2w[:, 2, 2] = a.cos(), a.sin(), -a.sin(), a.cos()
    c2w[:, 0, 3], c2w[:, 2, 3] = 1.5 * (i.view(n) / n - 0.5), 0.2 * i.view(n) / n
    grid = torch.stack([xs - W / 2, ys - H / 2], -1)
    cam = torch.cat([depth[..., None] * grid / f, depth[..., None]], -1)
    pts = torch.einsum("nij,nhwj->nhwi", c2w[:, :3, :3], cam) + c2w[:, None, None, :3, 3]
    K = torch.zeros(n, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W / 2, H / 2, 1
    conf = 1.0 + 5.0 * torch.rand((n, H, W), generator=g)
    to = lambda t: t.to(dev).contiguous()
    return dict(conf=to(conf), K=to(K), c2w=to(c2w), cams=torch.linalg.inv(to(c2w)), depth=to(depth), pts3d=to(pts), f=f)


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = math.inf
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def aligner_for(s, dev, S=16, stride=4):
    """A GroupAligner whose parameters reproduce the scene (windows of S frames, stride 4): what get_3D_model_from_scene reads."""
    n, H, W = s["conf"].shape
    groups = [list(range(a, a + S)) for a in range(0, n - S + 1, stride)]
    pred = torch.zeros((len(groups), S, H, W, 3), device=dev)
    conf = torch.stack([s["conf"][g] for g in groups])
    a = GroupAligner(groups, pred, conf)
    a.P["im_depthmaps"].copy_(s["depth"].reshape(n, -1).log())
    from geo4d_amd.align import rotmat_to_quat, signed_log1p, FOCAL_BREAK
    for k in range(n):
        a.P["im_poses"][k, :4] = rotmat_to_quat(s["c2w"][k, :3, :3].cpu()).to(dev)
        a.P["im_poses"][k, 4:7] = signed_log1p(s["c2w"][k, :3, 3])
    a.P["im_focals"][:] = FOCAL_BREAK * math.log(s["f"])
    a.imgs = torch.rand((n, H, W, 3), device=dev)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--torch-rows", type=int, default=16)
    ap.add_argument("--torch-full", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = 320, 512
    out = {"H": H, "W": W}
    for n in args.frames:
        s = synthetic_scene(n, H, W, dev)
        args_c = (s["conf"], s["K"], s["cams"], s["depth"], s["pts3d"])
        hip_res = scene_export.clean_pointcloud(*args_c)
        t_hip = timed(lambda: scene_export.clean_pointcloud(*args_c))
        r = {"pairs": n * (n - 1), "projections_G": n * (n - 1) * H * W / 1e9, "clean_hip_ms": 1e3 * t_hip,
             "cleaned_frac": float((hip_res != s["conf"]).float().mean())}
        if n <= args.torch_full:
            tr = torch_clean(*args_c)
            t_torch = timed(lambda: torch_clean(*args_c), reps=1)
            r["clean_torch_ms"] = 1e3 * t_torch
            r["differ"] = int((tr != hip_res).sum())
        else:
            rows = list(range(args.torch_rows))
            t_rows = timed(lambda: torch_clean(*args_c, rows=rows), reps=1)
            r["clean_torch_ms_extrapolated"] = 1e3 * t_rows * n / len(rows)
            r["torch_rows_timed"] = len(rows)
        a = aligner_for(s, dev)
        a.min_conf_thr = 3.5
        with tempfile.TemporaryDirectory() as d:
            t_pc = timed(lambda: scene_export.get_3D_model_from_scene(d, True, a, min_conf_thr=3.5, as_pointcloud=True,
                                                                       thr_for_init_conf=True), reps=2)
            r["glb_points_MB"] = os.path.getsize(os.path.join(d, "scene.glb")) / 2 ** 20
        r["export_pointcloud_ms"] = 1e3 * t_pc
        m = a.get_masks()
        r["mesh_faces_ms"] = 1e3 * timed(lambda: ops.scene_mesh_faces(m, n, H, W, dev))
        out[f"n{n}"] = r
        print(f"[n={n}] {r}", file=sys.stderr, flush=True)
        del a, s
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
