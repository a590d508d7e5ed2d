#!/usr/bin/env python3
"""Time of the renderer (geo4d_amd/render.py, csrc/render.hip) on a 64-image 320 x 512 synthetic scene (tools/scene_export_bench.py's):
every image drawn into --views of its own cameras, one pixel per point and with the adaptive radius of render_scene(point_size=2).

Per configuration: ms per view of splat, fill (one pass) and resolve (device time by events round --inner back-to-back calls, best and
median of --reps such windows), the atomics issued per view (counted from the restatement's footprint rule evaluated with torch on the device) and the atomic bytes per second that makes of
the splat, and the wall time of the numpy restatement (tests/render_restatement.py) on the same input for --numpy-views views, with the
two images compared. Prints one JSON line.
usage: render_bench.py [--frames 64] [--views 64] [--numpy-views 1] [--reps 7] [--inner 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_restatement as rr  # noqa: E402
from geo4d_amd import ops  # noqa: E402
from geo4d_amd.scene_view import source_lists, views_of  # noqa: E402
from tools.scene_export_bench import synthetic_scene  # noqa: E402


def device_ms(fn, reps, inner):
    """(best, median) ms per call over `reps` event-timed windows of `inner` back-to-back calls, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return min(ms), sorted(ms)[len(ms) // 2]


def atomics_issued(pts, views, radius, size, near, max_size):
    """Covered pixels summed over every (view, point): the number of atomicMin the splat issues (float32 torch, the kernel's rule)."""
    H, W = size
    total = 0
    for M in views:
        cam = [((M[4 * r] * pts[:, 0] + M[4 * r + 1] * pts[:, 1]) + M[4 * r + 2] * pts[:, 2]) + M[4 * r + 3] for r in range(3)]
        xc, yc, zc = cam
        keep = torch.isfinite(xc) & torch.isfinite(yc) & torch.isfinite(zc) & ~(zc <= near)
        u, v = M[12] * (xc / zc) + M[14], M[13] * (yc / zc) + M[15]
        s = torch.ones_like(zc)
        if radius is not None:
            s = torch.ceil(2 * radius * M[12] / zc).clamp(1, max_size)
        x0, y0 = torch.floor(u - 0.5 * (s - 1) + 0.5), torch.floor(v - 0.5 * (s - 1) + 0.5)
        nx = (torch.minimum(x0 + s, torch.full_like(s, W)) - x0.clamp(min=0)).clamp(min=0)
        ny = (torch.minimum(y0 + s, torch.full_like(s, H)) - y0.clamp(min=0)).clamp(min=0)
        total += int((nx * ny)[keep].sum().item())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--numpy-views", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H, W, V = args.frames, 320, 512, args.views
    s = synthetic_scene(n, H, W, dev)
    pts = s["pts3d"].reshape(-1, 3).contiguous()
    col = torch.rand((n * H * W, 3), device=dev)
    pick = [round(i * (n - 1) / max(V - 1, 1)) for i in range(V)]
    c2w, K = s["c2w"][pick].double().cpu(), s["K"][pick].double().cpu()
    views = views_of(c2w, K).to(dev)
    ptr, idx = source_lists(None, V, n)
    ws = ops.render_workspace(V, H, W, len(idx), dev)
    out = {"frames": n, "H": H, "W": W, "views": V, "points_M": n * H * W / 1e6, "reps": args.reps, "calls_per_window": args.inner}
    for name, radius, max_size in (("size1", None, 9), ("adaptive", (0.5 * 2.0 * s["depth"] / s["f"]).reshape(-1).contiguous(), 9)):
        splat = lambda: ops.render_splat(pts, views, ptr, idx, (H, W), ws, radius=radius, pts_per_image=H * W, max_size=max_size)
        t_splat, med_splat = device_ms(splat, args.reps, args.inner)
        t_fill, med_fill = device_ms(lambda: ops.render_fill(ws, V, (H, W), 1), args.reps, args.inner)
        splat()
        t_res, med_res = device_ms(lambda: ops.render_resolve(ws, col, V, (H, W)), args.reps, args.inner)
        rgb, depth, index = ops.render_resolve(ws, col, V, (H, W))
        atomics = atomics_issued(pts, views, radius, (H, W), 1e-3, max_size)
        r = {"splat_ms_per_view": t_splat / V, "fill_ms_per_view": t_fill / V, "resolve_ms_per_view": t_res / V,
             "median_ms_per_view": {"splat": med_splat / V, "fill": med_fill / V, "resolve": med_res / V},
             "atomics_per_view_M": atomics / V / 1e6, "atomic_MB_per_view": 8 * atomics / V / 1e6,
             "atomic_GB_per_s": 8 * atomics / (t_splat * 1e-3) / 1e9, "covered_frac": float((index >= 0).float().mean())}
        nv = min(args.numpy_views, V)
        if nv:
            p_np, c_np = pts.cpu().numpy(), col.cpu().numpy()
            r_np = None if radius is None else radius.cpu().numpy()
            t0 = time.perf_counter()
            ref = rr.render(p_np.reshape(n, H * W, 3), c_np, c2w[:nv].numpy(), K[:nv].numpy(), (H, W), radius=r_np, max_size=max_size)
            r["numpy_s_per_view"] = (time.perf_counter() - t0) / nv
            r["numpy_pixels_differ"] = int((ref["index"] != index[:nv].cpu().numpy()).sum())
        out[name] = r
        print(f"[{name}] {r}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
