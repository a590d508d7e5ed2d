#!/usr/bin/env python3
"""Wall time of the per-window shift / focal recovery of pose_init="prefix" (geo4d_amd.geometry.recover_focal_pixels -> ops.focal_shift,
csrc/focal_shift.hip) on the reference frames of a 128-frame clip - 30 maps at 320 x 512, every pixel, a confidence mask - against a
numpy / scipy restatement of the reference's path (utils/geometry.py:162-270: device -> host copy of the maps, then
scipy.optimize.least_squares(method="lm", x0 = 0, ftol = 1e-3) per map on the masked pixels) on the same seeded inputs. Also reports the
solver's enqueue alone by device events and the bytes per second its pixel passes move if every one of the `iters` passes ran (a lower
bound: converged maps skip theirs). Prints one JSON line; writes nothing.
usage: focal_shift_bench.py [--maps 30] [--height 320] [--width 512] [--iters 40] [--host-maps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geo4d_amd import geometry, ops  # noqa: E402


def host_reference_path(points, conf, z_offset):
    """What align_group_prefix does per call: the maps leave the device, one least_squares per map."""
    from scipy.optimize import least_squares
    B, H, W, _ = points.shape
    pts = points.cpu().numpy().copy()
    pts[..., 2] += z_offset
    mask = (conf > 0.5).cpu().numpy()
    uv = geometry.image_plane_uv(W, H, dtype=torch.float32).numpy()
    out = []
    for b in range(B):
        xyz, q = pts[b][mask[b]], uv[mask[b]]
        xy, z = xyz[:, :2], xyz[:, 2]

        def residual(shift):
            proj = xy / (z + shift)[:, None]
            f = (proj * q).sum() / np.square(proj).sum()
            return (f * proj - q).ravel()
        s = np.float32(least_squares(residual, x0=0, ftol=1e-3, method="lm")["x"].squeeze())
        proj = xy / (z + s)[:, None]
        out.append((float(s), float((proj * q).sum() / (proj * proj).sum())))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=30)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--host-maps", type=int, default=3, help="maps timed through the host path (its time is scaled to --maps)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W = args.maps, args.height, args.width
    g = torch.Generator(device=dev).manual_seed(0)
    uv = geometry.image_plane_uv(W, H, dtype=torch.float32, device=dev)
    u, v = uv[..., 0], uv[..., 1]
    k = torch.arange(B, device=dev).float()[:, None, None]
    depth = 3.0 + 0.7 * torch.sin(5.0 * u + 0.3 * k) + 0.5 * torch.cos(6.0 * v - 0.2 * k) + 0.8 * u * v
    focal = (0.8 + 0.02 * k)
    xy = uv * depth[..., None] / focal[..., None] + 0.004 * torch.randn((B, H, W, 2), generator=g, device=dev)
    z = depth * (0.8 + 0.05 * k) + 0.004 * torch.randn((B, H, W), generator=g, device=dev)
    points = torch.cat([xy * (0.8 + 0.05 * k)[..., None], z[..., None]], -1).contiguous()
    conf = 0.2 + 3.0 * torch.rand((B, H, W), generator=g, device=dev)             # ~ 10 % below the 0.5 threshold

    def device_path():
        z_offset = (1.0 - points[..., 2].min()).reshape(1)
        px, status = geometry.recover_focal_pixels(points, conf, (H, W), z_offset=z_offset, return_status=True)
        return torch.stack([px, status.float()]).cpu()                            # the one small copy the initialisation makes

    device_path()                                                                 # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = device_path()
    hip_ms = (time.perf_counter() - t0) * 1e3

    z_offset = (1.0 - points[..., 2].min()).reshape(1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    shift, fnorm, status = ops.focal_shift(points, conf, 0.5, (H, W), z_offset, iters=args.iters)
    e1.record()
    torch.cuda.synchronize()
    solver_ms = e0.elapsed_time(e1)

    nh = max(1, min(args.host_maps, B))
    t0 = time.perf_counter()
    host = host_reference_path(points[:nh], conf[:nh], float(z_offset))
    host_ms = (time.perf_counter() - t0) * 1e3 * B / nh
    rel = float(np.abs(fnorm[:nh].cpu().numpy() / host[:, 1] - 1).max())
    out = dict(tool="focal_shift_bench", maps=B, H=H, W=W, iters=args.iters, status_ok=bool((status == 0).all()),
               hip_ms=round(hip_ms, 3), solver_ms=round(solver_ms, 3), host_ms=round(host_ms, 1), host_maps_timed=nh,
               speedup=round(host_ms / hip_ms, 1), all_pass_GBps=round(16.0 * B * H * W * args.iters / (solver_ms * 1e-3) / 1e9, 1),
               focal_px_mean=float(got[0].mean()), focal_rel_diff_vs_host=rel)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
