#!/usr/bin/env python3
"""Generate tests/golden/prefix_init.pt by running the REFERENCE's shift / focal recovery and its shipped group initialisation on CPU.

Run in the build container only (`python tests/golden/generate_prefix_init.py`); the GPU box has no reference tree and only reads the
committed file. What is imported from the reference, unmodified: utils.geometry (point_map_to_depth, image_plane_uv,
intrinsics_from_fov_xy), dust3r.cloud_opt.optimizer_group.LightPointCloudGroupOptimizer and dust3r.cloud_opt.init_im_poses
(init_from_group -> align_group_prefix -> fast_pnp -> init_from_pts3d_group), with absent packages mocked by generate.py's
_mock_absent_packages and cv2.solvePnPRansac / cv2.Rodrigues stubbed over geo4d_amd.pnp.solve_pnp_ransac, as generate.py pnp_init does.

prefix_init.pt holds
  uv / intrinsics: image_plane_uv and intrinsics_from_fov_xy values for the CPU test.
  focal:  two sets of 3 synthetic point maps (24 x 32, true shift 0; 40 x 64, z offset by +4): smooth non-planar depth, Gaussian noise, a
          random 90 % mask. Per set the reference's point_map_to_depth at downsample_size = (H, W) and (16, 16), the fp64 exact minimiser
          of the same objective on the same pixels (scipy minimize_scalar, tol 1e-14, bracket from 0) and
          ref_gap = max |focal_ref / focal_exact - 1| over everything in `focal`.
  shapes: the small shapes of the GPU test (3 x 5 with one masked pixel; 24 x 32 with 65 selected; 72 x 64 with 4097 selected - 24 x 32
          holds only 768 pixels; five 24 x 32 maps with a different mask count each), with the same reference / exact outputs and their
          own ref_gap.
  prefix: the 10-image / 4-window scene of generate.py pnp_init without ray maps, through LightPointCloudGroupOptimizer(...,
          opt_raydir=False) and init_from_group(scene, niter_PnP=50): parameters after the initialisation, the loss, focal_group
          before and after align_group_prefix's outlier filter, and focal_group_gap = the relative distance of the reference's window
          focals (scipy least_squares stops at ftol = 1e-3) to the exact minimiser's.
  outlier: the same scene with window 2's reference frame scaled by 3 in x and y, so that its focal trips the filter (asserted).
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate  # noqa: E402  (puts the repository and the reference on sys.path)


def cv2_stub():
    from unittest.mock import MagicMock
    from geo4d_amd import pnp as gpnp
    cv2 = MagicMock()
    cv2.__name__, cv2.__path__, cv2.SOLVEPNP_SQPNP = "cv2", [], 8

    def solvePnPRansac(obj, img, K, dist, iterationsCount=100, reprojectionError=8.0, flags=0):
        ok, R, t, inl = gpnp.solve_pnp_ransac(obj, img, K, iterations=iterationsCount, reproj=reprojectionError, seed=0)
        if not ok:
            return False, None, None, None
        ang = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2)))
        axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        rvec = (axis / (2 * math.sin(ang)) * ang if ang > 1e-12 else np.zeros(3)).reshape(3, 1)
        return True, rvec, t.reshape(3, 1), inl.reshape(-1, 1)

    def Rodrigues(rvec):
        r = np.asarray(rvec, np.float64).reshape(3)
        th = np.linalg.norm(r)
        if th < 1e-12:
            return np.eye(3), None
        k = r / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx, None
    cv2.solvePnPRansac, cv2.Rodrigues = solvePnPRansac, Rodrigues
    return cv2


# ---- focal / shapes ---------------------------------------------------------------------------------------------------------------
def synthetic_maps(geo, B, H, W, z_offset, gen, keep=0.9, noise=0.004):
    uv = geo.image_plane_uv(W, H, dtype=torch.float32)
    u, v = uv[..., 0], uv[..., 1]
    pts, masks, truth = [], [], []
    for b in range(B):
        f = 0.7 + 0.45 * b
        depth = 3.0 + 0.7 * torch.sin(5.0 * u + 0.6 * b) + 0.5 * torch.cos(6.0 * v - 0.3 * b) + 0.8 * u * v
        xy = uv * depth[..., None] / f + noise * torch.randn((H, W, 2), generator=gen)
        z = depth + z_offset + noise * torch.randn((H, W), generator=gen)
        pts.append(torch.cat([xy, z[..., None]], -1))
        masks.append(torch.rand((H, W), generator=gen) < keep)
        truth.append(f)
    return torch.stack(pts), torch.stack(masks), torch.tensor(truth)


def mask_with_count(H, W, count, gen):
    m = torch.zeros(H * W, dtype=torch.bool)
    m[torch.randperm(H * W, generator=gen)[:count]] = True
    return m.reshape(H, W)


def exact_minimiser(geo, pts, mask, size):
    """fp64 minimiser of the objective solve_optimal_shift_focal states, on the pixels point_map_to_depth hands it for `size`."""
    import torch.nn.functional as F
    from scipy.optimize import minimize_scalar
    H, W = pts.shape[-3], pts.shape[-2]
    uv = geo.image_plane_uv(W, H, dtype=torch.float32)
    nearest = lambda t: F.interpolate(t.permute(2, 0, 1)[None], size, mode="nearest")[0].permute(1, 2, 0)
    out = []
    for b in range(pts.shape[0]):
        sel = nearest(mask[b].float()[..., None])[..., 0] > 0
        p, q = nearest(pts[b])[sel].double().numpy(), nearest(uv)[sel].double().numpy()

        def parts(s):
            proj = p[:, :2] / (p[:, 2] + s)[:, None]
            return (proj * q).sum(), (proj * proj).sum()

        def energy(s):
            a, bb = parts(s)
            return (q * q).sum() - a * a / bb
        res = minimize_scalar(energy, bracket=(0.0, 0.05), tol=1e-14)
        a, bb = parts(res.x)
        out.append((res.x, a / bb, energy(res.x)))
    return torch.tensor(out, dtype=torch.float64)


def solver_case(geo, pts, mask, sizes, keep_depth=True):
    H, W = pts.shape[-3], pts.shape[-2]
    case, gap = dict(points=pts, mask=mask, ref={}, exact={}), 0.0
    for size in sizes:
        depth, fov_x, fov_y, shift = geo.point_map_to_depth(pts, mask, downsample_size=size)
        focal = (W / math.hypot(H, W)) / torch.tan(fov_x.double() / 2)                 # optim_focal back from fov_x = 2 atan(W / diag / focal)
        ex = exact_minimiser(geo, pts, mask, size)
        case["ref"][size] = dict(fov_x=fov_x, fov_y=fov_y, shift=shift, focal=focal.float(), **(dict(depth=depth) if keep_depth else {}))
        case["exact"][size] = dict(shift=ex[:, 0], focal=ex[:, 1], energy=ex[:, 2])
        g = float((focal / ex[:, 1] - 1).abs().max())
        print(f"  {tuple(pts.shape)} at {size}: shift {shift.tolist()}, focal {focal.tolist()}, gap to the exact minimiser {g:.2e}")
        gap = max(gap, g)
    return case, gap


def focal_fixtures(geo):
    gen = torch.Generator().manual_seed(23)
    focal, shapes, gap_f, gap_s = {}, {}, 0.0, 0.0
    for name, (H, W, off) in (("24x32", (24, 32, 0.0)), ("40x64_offset", (40, 64, 4.0))):
        pts, mask, truth = synthetic_maps(geo, 3, H, W, off, gen)
        focal[name], g = solver_case(geo, pts, mask, ((H, W), (16, 16)))
        focal[name].update(truth_focal=truth, z_offset=off)
        gap_f = max(gap_f, g)
    pts, mask, _ = synthetic_maps(geo, 1, 3, 5, 0.0, gen, keep=2.0)
    mask[0, 1, 3] = False
    shapes["3x5_one_masked"], g = solver_case(geo, pts, mask, ((3, 5),), keep_depth=False); gap_s = max(gap_s, g)
    pts, _, _ = synthetic_maps(geo, 1, 24, 32, 0.0, gen)
    shapes["24x32_65"], g = solver_case(geo, pts, mask_with_count(24, 32, 65, gen)[None], ((24, 32),), keep_depth=False); gap_s = max(gap_s, g)
    pts, _, _ = synthetic_maps(geo, 1, 72, 64, 0.0, gen)
    shapes["72x64_4097"], g = solver_case(geo, pts, mask_with_count(72, 64, 4097, gen)[None], ((72, 64),), keep_depth=False); gap_s = max(gap_s, g)
    pts, _, _ = synthetic_maps(geo, 5, 24, 32, 2.0, gen)
    counts = [700, 64, 129, 512, 33]
    shapes["5_maps_counts"], g = solver_case(geo, pts, torch.stack([mask_with_count(24, 32, c, gen) for c in counts]), ((24, 32),), keep_depth=False); gap_s = max(gap_s, g)
    shapes["5_maps_counts"]["counts"] = counts
    print(f"ref_gap: focal {gap_f:.2e}, shapes {gap_s:.2e}")
    return dict(cases=focal, ref_gap=gap_f), dict(cases=shapes, ref_gap=gap_s)


# ---- prefix / outlier -------------------------------------------------------------------------------------------------------------
def window_scene():
    """generate.py pnp_init_fixtures' 10-image / 4-window scene (same seeds, same arithmetic), without ray maps."""
    g = torch.Generator().manual_seed(11)
    n, S, stride, H, W, f = 10, 4, 2, 24, 32, 30.0
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grid, pp = torch.stack([xs, ys], -1).float(), torch.tensor([W / 2, H / 2])
    c2w, pts = [], []
    for i in range(n):
        depth = 3.0 + 0.6 * torch.sin(xs / 5.0 + 0.3 * i) + 0.4 * torch.cos(ys / 4.0)
        cam = torch.cat([depth[..., None] * (grid - pp) / f, depth[..., None]], -1)
        a = torch.tensor(0.04 * i)
        R = torch.tensor([[torch.cos(a), 0, torch.sin(a)], [0, 1, 0], [-torch.sin(a), 0, torch.cos(a)]])
        M = torch.eye(4); M[:3, :3] = R; M[:3, 3] = torch.tensor([0.1 * i, 0.0, 0.02 * i])
        c2w.append(M); pts.append(cam @ R.T + M[:3, 3])
    groups = [list(range(s0, s0 + S)) for s0 in range(0, n - S + 1, stride)]
    preds, confs = [], []
    for gi, grp in enumerate(groups):
        w2c = torch.inverse(c2w[grp[0]])
        sc = 0.8 + 0.15 * gi
        preds.append(torch.stack([(pts[i] @ w2c[:3, :3].T + w2c[:3, 3]) * sc for i in grp]) + 0.002 * torch.randn((S, H, W, 3), generator=g))
        confs.append(1.0 + 3.0 * torch.rand((S, H, W, 1), generator=g))
    return groups, torch.stack(preds), torch.stack(confs), f, torch.stack(c2w)


def reference_prefix_init(groups, pred, conf, niter_PnP=50):
    from dust3r.cloud_opt.optimizer_group import LightPointCloudGroupOptimizer
    import dust3r.cloud_opt.init_im_poses as init_fun
    torch.manual_seed(0)
    views = [[{"idx": [i]} for i in grp] for grp in groups]
    pred_list = [{"pts3d": p.clone(), "conf": c.clone()} for p, c in zip(pred, conf)]
    scene = LightPointCloudGroupOptimizer(views, pred_list, conf="id", conf_optimize=True, verbose=False, shared_focal=True,
                                          temporal_smoothing_weight=0.015, translation_weight=1.0, opt_raydir=False)
    seen = {}
    orig_p2d, orig_pnp = init_fun.point_map_to_depth, init_fun.fast_pnp

    def spy_p2d(points, mask, downsample_size):
        out = orig_p2d(points, mask, downsample_size=downsample_size)
        H, W = points.shape[-3], points.shape[-2]
        K = init_fun.intrinsics_from_fov_xy(out[1], out[2])
        seen["before"] = ((K[:, 0, 0] * W) + (K[:, 1, 1] * H)) / 2
        seen["size"] = tuple(downsample_size)
        import utils.geometry as geo
        diag = math.hypot(H, W)
        focal_ref = (W / diag) / torch.tan(out[1].double() / 2)
        seen["gap"] = float((focal_ref / exact_minimiser(geo, points, mask, tuple(downsample_size))[:, 1] - 1).abs().max())
        return out

    def spy_pnp(pts3d, focal, **kw):
        seen.setdefault("pnp_focals", []).append(focal)
        return orig_pnp(pts3d, focal, **kw)
    init_fun.point_map_to_depth, init_fun.fast_pnp = spy_p2d, spy_pnp
    try:
        with torch.no_grad():
            init_fun.init_from_group(scene, niter_PnP=niter_PnP)
    finally:
        init_fun.point_map_to_depth, init_fun.fast_pnp = orig_p2d, orig_pnp
    S = len(groups[0])
    after = torch.tensor([seen["pnp_focals"][g * S] for g in range(len(groups))])        # temp_focal of every window's slot 0 = its filtered focal
    assert seen["size"] == tuple(pred.shape[2:4]) and len(seen["pnp_focals"]) == len(groups) * S
    out = {k: getattr(scene, k).detach().clone() for k in ("im_depthmaps", "im_poses", "im_focals", "pw_poses")}
    loss = float(scene(epoch=0))
    print(f"prefix init: focal_group {seen['before'].tolist()} -> {after.tolist()}; shared focal {float(scene.get_focals()[0]):.4f}; loss {loss:.6f}")
    print(f"  gap of the reference's window focals to the exact minimiser {seen['gap']:.2e}")
    return dict(after_init=out, loss=loss, focal_group_before=seen["before"].clone(), focal_group_after=after, focal_group_gap=seen["gap"])


def main():
    generate._mock_absent_packages(cv2_stub())
    import utils.geometry as geo
    out = {}
    out["uv"] = {(W, H, ar): geo.image_plane_uv(W, H, aspect_ratio=ar, dtype=torch.float32) for W, H, ar in ((32, 24, None), (5, 3, None), (64, 40, 2.0))}
    fov = torch.tensor([[0.6, 0.45], [1.2, 0.9], [1.9, 1.5]])
    out["intrinsics"] = dict(fov_x=fov[:, 0], fov_y=fov[:, 1], K=geo.intrinsics_from_fov_xy(fov[:, 0], fov[:, 1]))
    out["focal"], out["shapes"] = focal_fixtures(geo)
    groups, pred, conf, f, c2w = window_scene()
    out["prefix"] = dict(groups=groups, pred=pred, conf=conf, niter_PnP=50, truth_focal=f, c2w=c2w, **reference_prefix_init(groups, pred, conf))
    bad_window = 2
    frame = pred[bad_window, 0].clone()
    frame[..., :2] *= 3.0
    pred_o = pred.clone()
    pred_o[bad_window, 0] = frame
    res = reference_prefix_init(groups, pred_o, conf)
    before, after = res["focal_group_before"], res["focal_group_after"]
    assert float(after[bad_window]) != float(before[bad_window]) and all(float(after[g]) == float(before[g]) for g in range(len(groups)) if g != bad_window), \
        "the distorted window must trip the 0.6 outlier filter, the others must not"
    out["outlier"] = dict(window=bad_window, frame=frame, focal_group_before=before, focal_group_after=after, focal_group_gap=res["focal_group_gap"],
                          im_focals=res["after_init"]["im_focals"])
    path = os.path.join(HERE, "prefix_init.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
