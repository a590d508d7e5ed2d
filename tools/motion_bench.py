#!/usr/bin/env python3
"""Time of the motion votes (geo4d_amd/motion.py, csrc/motion.hip) on a 64-image 320 x 512 synthetic scene (tools/scene_export_bench.py's:
a wavy wall with a box sliding in front), radius 8.

Device time by HIP events round --inner back-to-back warm calls each of the range pass, the vote pass and both (so the host's
per-call time hides behind the device's), median and best of --reps such windows; the votes
cast (the sum of the output) and votes per second of the vote pass; the wall time of the numpy restatement
(tests/motion_restatement.py) for --numpy-images images of the same input, with the two results compared; the share of dynamic pixels
under the default thresholds. Prints one JSON line.
usage: motion_bench.py [--frames 64] [--radius 8] [--reps 20] [--inner 10] [--numpy-images 1]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import motion_restatement as mr  # noqa: E402
from geo4d_amd import motion, ops  # noqa: E402
from geo4d_amd.scene_view import views_of  # noqa: E402
from tools.scene_export_bench import synthetic_scene  # noqa: E402


def device_ms(fn, reps, inner):
    """(median, best) ms per call over `reps` event-timed windows of `inner` back-to-back calls, after two warm-up calls."""
    fn(), fn()
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
    return sorted(ms)[len(ms) // 2], min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--numpy-images", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H, W, radius = args.frames, 320, 512, args.radius
    s = synthetic_scene(n, H, W, dev)
    pts3d, depth = s["pts3d"].contiguous(), s["depth"].contiguous()
    valid = torch.ones((n, H, W), dtype=torch.bool, device=dev)
    c2w, K = s["c2w"].double().cpu(), s["K"].double().cpu()
    views = views_of(c2w, K).to(dev)
    ws = ops.motion_range(depth, valid)
    votes = ops.motion_votes(pts3d, depth, valid, views, radius=radius, ws=ws)
    cast = int(votes.sum(dtype=torch.int64).item())
    out = {"frames": n, "H": H, "W": W, "radius": radius, "pixels_M": n * H * W / 1e6, "reps": args.reps, "calls_per_window": args.inner, "device": torch.cuda.get_device_name(0)}
    out["range_ms"], out["range_ms_best"] = device_ms(lambda: ops.motion_range(depth, valid), args.reps, args.inner)
    out["votes_ms"], out["votes_ms_best"] = device_ms(lambda: ops.motion_votes(pts3d, depth, valid, views, radius=radius, ws=ws), args.reps, args.inner)
    out["both_ms"], out["both_ms_best"] = device_ms(lambda: ops.motion_votes(pts3d, depth, valid, views, radius=radius), args.reps, args.inner)
    out["votes_cast_M"] = cast / 1e6
    pairs = sum(min(n - 1, i + radius) - max(0, i - radius) for i in range(n)) * H * W
    out["projections_M"] = pairs / 1e6
    out["votes_G_per_s"] = cast / (out["votes_ms"] * 1e-3) / 1e9
    out["projections_G_per_s"] = pairs / (out["votes_ms"] * 1e-3) / 1e9
    out["dynamic_frac"] = float(motion.dynamic_mask(votes).float().mean())
    k = min(args.numpy_images, n)
    if k:
        images = [n // 2 + d for d in range(k)]                                   # middle images: the full 2 radius voters
        p_np, d_np, v_np = pts3d.cpu().numpy(), depth.cpu().numpy(), valid.cpu().numpy()
        views_np = mr.views_of(c2w.numpy(), K.numpy())
        t0 = time.perf_counter()
        ref = mr.votes(p_np, d_np, v_np, views_np, radius=radius, images=images)
        out["numpy_s_per_image"] = (time.perf_counter() - t0) / k                  # includes the depth ranges of all n images
        out["numpy_pixels_differ"] = int((ref[images] != votes[images].cpu().numpy()).any(-1).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
