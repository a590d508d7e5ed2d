#!/usr/bin/env python3
"""Time of the mesh renderer (geo4d_amd/render.py render_mesh, csrc/render_mesh.hip) on the TSDF surface of tools/tsdf_mesh_bench.py's
field: the static part of a 64-image 320 x 512 synthetic scene at the default voxel, as one indexed mesh with vertex colours.

1. The mesh drawn into --views of the scene's own cameras: ms per view of the raster (with its clear) and of the resolve (shade 0.5),
   next to the one-pixel point splat and resolve of the same scene's points into the same views, in the same process.
2. Close-up views, the middle camera moved forward until the wall's nearest point is --close units away, so that triangles span tens
   to hundreds of pixels: the raster for every --large-area threshold, 0 (every triangle through the list) and "off" (every triangle
   in its own thread) among them, with the number of clipped bounding boxes above each threshold and a check that the images are equal.
3. The wall time of the numpy restatement (tests/render_mesh_restatement.py) for --numpy-views of the views of 1, compared with the
   device's images.
Device time by HIP events round --inner back-to-back warm calls, median and best of --reps such windows. Prints one JSON line.
usage: render_mesh_bench.py [--frames 64] [--views 64] [--numpy-views 1] [--reps 7] [--inner 5] [--close 3.0 1.5 0.6 0.2]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_mesh_restatement as rm  # noqa: E402
from geo4d_amd import fusion, motion, ops  # noqa: E402
from geo4d_amd.scene_view import source_lists, views_of  # noqa: E402
from tools.motion_bench import device_ms  # noqa: E402
from tools.scene_export_bench import synthetic_scene  # noqa: E402

OFF = (1 << 31) - 1


def box_areas(vertices, faces, view, size):
    """Pixels in every triangle's clipped bounding box (float32 torch, close to the kernel's rule; dropped triangles count 0)."""
    H, W = size
    M = view
    x, y, z = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    xc, yc, zc = [((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] for r in range(3)]
    ok = torch.isfinite(xc) & torch.isfinite(yc) & torch.isfinite(zc) & (zc > 1e-3)
    u, v = M[12] * (xc / zc) + M[14], M[13] * (yc / zc) + M[15]
    ok &= (u.abs() < 65536) & (v.abs() < 65536)
    f = faces.long()
    u, v, ok = u[f], v[f], ok[f].all(1)
    nx = (torch.floor(u.max(1).values).clamp(max=W - 1) - torch.ceil(u.min(1).values).clamp(min=0) + 1).clamp(min=0)
    ny = (torch.floor(v.max(1).values).clamp(max=H - 1) - torch.ceil(v.min(1).values).clamp(min=0) + 1).clamp(min=0)
    return torch.where(ok, nx * ny, torch.zeros_like(nx))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--numpy-views", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--close", type=float, nargs="*", default=[3.0, 1.5, 0.6, 0.2])
    ap.add_argument("--large-area", type=int, nargs="*", default=[0, 8, 16, 32, 64, 256, 1024])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H, W, V = args.frames, 320, 512, args.views
    s = synthetic_scene(n, H, W, dev)
    pts3d, depth = s["pts3d"].contiguous(), s["depth"].contiguous()
    every = torch.ones((n, H, W), dtype=torch.bool, device=dev)
    c2w, Kcam = s["c2w"].double().cpu(), s["K"].double().cpu()
    static = (~motion.dynamic_mask(motion.motion_votes(pts3d, depth, every, c2w, Kcam))).contiguous()
    all_views, centres = views_of(c2w, Kcam).to(dev), c2w[:, :3, 3].float().contiguous().to(dev)
    rgba = torch.randint(0, 256, (n, H, W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    voxel = torch.tensor(fusion.default_voxel(depth, torch.full((n,), s["f"], device=dev), static), dtype=torch.float32).item()
    Kk, f, wt, col, M, dropped = ops.tsdf_field(pts3d, depth, static, all_views, centres, rgba, None, voxel=voxel, trunc=4, near=1e-3)
    vert, vcol, _, faces = ops.tsdf_mesh_extract(Kk, f, wt, col, voxel=voxel, min_weight=4.0)
    del Kk, f, wt, col, rgba, every, static
    Nv, T = len(vert), len(faces)
    out = {"frames": n, "H": H, "W": W, "views": V, "voxel": voxel, "vertices": Nv, "triangles": T, "reps": args.reps,
           "calls_per_window": args.inner, "device": torch.cuda.get_device_name(0), "default_large_area": ops.RASTER_LARGE_AREA}

    # 1. the scene's own cameras, next to the point splat
    pick = [round(i * (n - 1) / max(V - 1, 1)) for i in range(V)]
    views = all_views[pick].contiguous()
    ws = ops.render_workspace(V, H, W, n * V, dev)
    raster = lambda **kw: ops.render_raster(vert, faces, views, (H, W), ws, **kw)
    resolve = lambda: ops.render_resolve_mesh(ws, None, vert, faces, views, (H, W), vertex_colors=vcol, shade=0.5)
    r = {}
    r["raster_ms_per_view"], r["raster_ms_per_view_best"] = (t / V for t in device_ms(raster, args.reps, args.inner))
    r["raster_in_thread_ms_per_view"] = device_ms(lambda: raster(large_area=OFF), args.reps, args.inner)[0] / V
    raster()
    r["resolve_ms_per_view"], r["resolve_ms_per_view_best"] = (t / V for t in device_ms(resolve, args.reps, args.inner))
    rgb, zc, _, face = resolve()
    r["covered_frac"] = float((face >= 0).float().mean())
    r["box_pixels_per_view_M"] = float(sum(box_areas(vert, faces, v, (H, W)).sum() for v in views)) / V / 1e6
    pts, pcol = pts3d.reshape(-1, 3).contiguous(), torch.rand((n * H * W, 3), device=dev)
    ptr, idx = source_lists(None, V, n)
    splat = lambda: ops.render_splat(pts, views, ptr, idx, (H, W), ws, pts_per_image=H * W)
    r["point_splat_ms_per_view"], r["point_splat_ms_per_view_best"] = (t / V for t in device_ms(splat, args.reps, args.inner))
    r["point_resolve_ms_per_view"] = device_ms(lambda: ops.render_resolve(ws, pcol, V, (H, W)), args.reps, args.inner)[0] / V
    r["points_per_view_M"] = n * H * W / 1e6
    out["cameras"] = r
    print(f"[cameras] {r}", file=sys.stderr, flush=True)

    # 3. the restatement, for scale (before the close-ups reuse the names)
    nv = min(args.numpy_views, V)
    if nv:
        v_np, f_np, c_np = vert.cpu().numpy(), faces.cpu().numpy(), vcol.cpu().numpy()
        t0 = time.perf_counter()
        ref = rm.render(v_np, f_np, c2w[pick[:nv]].numpy(), Kcam[pick[:nv]].numpy(), (H, W), colors=c_np, shade=0.5)
        out["numpy_s_per_view"] = (time.perf_counter() - t0) / nv
        out["numpy_pixels_differ"] = {k: int((ref[k] != t[:nv].cpu().numpy()).sum()) for k, t in (("rgb", rgb), ("depth", zc), ("face", face))}
        print(f"[numpy] {out['numpy_s_per_view']:.1f} s per view, differing {out['numpy_pixels_differ']}", file=sys.stderr, flush=True)

    # 2. close-ups: one view, the list path at every threshold
    mid = n // 2
    wall = float(depth[mid][depth[mid] > 4.0].min())                              # the wall's nearest point (the sliding box is at 3.5)
    ws1 = ops.render_workspace(1, H, W, 0, dev)
    out["close_ups"] = []
    for dist in args.close:
        pose = c2w[mid].clone()
        pose[:3, 3] += pose[:3, 2] * (wall - dist)                                # forward along the camera's own z
        view = views_of(pose[None], Kcam[mid:mid + 1]).to(dev)
        areas = box_areas(vert, faces, view[0], (H, W))
        c = {"wall_distance": dist, "triangles_with_a_box": int((areas > 0).sum()), "box_pixels_M": float(areas.sum()) / 1e6,
             "largest_box": int(areas.max()), "ms": {}, "boxes_over": {}}
        images = []
        for la in args.large_area + [OFF]:
            name = "off" if la == OFF else str(la)
            fn = lambda: ops.render_raster(vert, faces, view, (H, W), ws1, large_area=la)
            c["ms"][name] = device_ms(fn, args.reps, args.inner)[0]
            c["boxes_over"][name] = int((areas > la).sum())
            fn()
            images.append(ws1[:H * W].clone())
        c["images_equal"] = all(torch.equal(images[0], k) for k in images[1:])
        c["resolve_ms"] = device_ms(lambda: ops.render_resolve_mesh(ws1, None, vert, faces, view, (H, W), vertex_colors=vcol, shade=0.5),
                                    args.reps, args.inner)[0]
        c["covered_frac"] = float((images[0] != -1).float().mean())
        out["close_ups"].append(c)
        print(f"[close-up {dist}] {c}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
