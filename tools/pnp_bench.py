#!/usr/bin/env python3
"""Wall time of GroupAligner.init_from_group(pose_init="prefix") with the host RANSAC-PnP (geo4d_amd/pnp.py, numpy, one call per image of
every window) against the device backend (ops.pnp_ransac, csrc/pnp.hip), in one process on one GPU, on a synthetic clip: 64 frames at
320 x 512 cut into 16-frame windows at stride 4, every window in its own frame and scale, point noise, 15 % gross outliers and 20 % of
the confidences below the threshold, so RANSAC runs many iterations and the refit runs long. The window reference frames carry noise
but no outliers: their focal comes from a least-squares fit without outlier rejection, which is not what is timed here.
Reports both times, the time per solved image, and the largest absolute parameter difference between the two initialisations.
The device backend draws one sampler table per distinct masked-pixel count on the host (pnp.sample_tables, cached); a fresh clip has about
one count per slot, so the quoted device time is COLD: the cache is emptied after the warm-up. The warm time (tables cached, as when a
clip is initialised again) and the time of drawing the tables alone are reported next to it. Prints one JSON line; writes nothing.
usage: pnp_bench.py [--frames 64] [--height 320] [--width 512] [--windows N (first N windows only)] [--niter 100] [--skip-host]"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geo4d_amd import pnp  # noqa: E402
from geo4d_amd.align import GroupAligner  # noqa: E402


def clip(n, S, stride, H, W, f, dev, windows=None):
    gen = torch.Generator(device=dev).manual_seed(4)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    grid, pp = torch.stack([xs, ys], -1).float(), torch.tensor([W / 2, H / 2], device=dev)
    c2w, pts = [], []
    for i in range(n):
        depth = 3.0 + 0.6 * torch.sin(xs / 70.0 + 0.2 * i) + 0.4 * torch.cos(ys / 50.0)
        cam = torch.cat([depth[..., None] * (grid - pp) / f, depth[..., None]], -1)
        a = 0.02 * i
        R = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], device=dev)
        M = torch.eye(4, device=dev)
        M[:3, :3], M[:3, 3] = R, torch.tensor([0.05 * i, 0.0, 0.01 * i], device=dev)
        c2w.append(M)
        pts.append(cam @ R.T + M[:3, 3])
    groups = [list(range(s0, s0 + S)) for s0 in range(0, n - S + 1, stride)][:windows]
    pred = torch.empty((len(groups), S, H, W, 3), device=dev)
    for g, grp in enumerate(groups):
        w2c = torch.inverse(c2w[grp[0]])
        pred[g] = torch.stack([(pts[i] @ w2c[:3, :3].T + w2c[:3, 3]) * (0.8 + 0.1 * g) for i in grp])
    pred += 0.006 * torch.randn(pred.shape, generator=gen, device=dev)
    bad = torch.rand(pred.shape[:-1], generator=gen, device=dev) < 0.15
    bad[:, 0] = False
    pred[bad] += (torch.rand((int(bad.sum()), 3), generator=gen, device=dev) - 0.5) * 4.0
    conf = torch.where(torch.rand(pred.shape[:-1], generator=gen, device=dev) < 0.2, 0.1, 1.5)
    return groups, pred, conf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--windows", type=int, default=None, help="time the first N windows only (the host leg takes about a second per image)")
    ap.add_argument("--niter", type=int, default=100)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    S, stride, f = 16, 4, 440.0
    groups, pred, conf = clip(args.frames, S, stride, args.height, args.width, f, dev, args.windows)

    def run(backend):
        a = GroupAligner(groups, pred, conf, shared_focal=True, temporal_smoothing_weight=0.015, translation_weight=1.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.init_from_group(None, pose_init="prefix", niter_PnP=args.niter, pnp_backend=backend)
        torch.cuda.synchronize()
        return a, time.perf_counter() - t0

    run("device")                                                   # warm-up: code objects, allocator
    pnp._TABLES.clear()                                             # ... but not the sampler's tables: a fresh clip draws every one
    d, dev_s = run("device")
    _, warm_s = run("device")
    counts = (conf.reshape(len(groups) * S, -1) > 0.5).sum(-1).cpu().tolist()
    pnp._TABLES.clear()
    t0 = time.perf_counter()
    for n in counts:
        pnp.sample_tables(n, args.niter, 0)
    tables_s = time.perf_counter() - t0
    print(f"device backend: {dev_s:.3f} s cold, {warm_s:.3f} s with cached tables, {tables_s:.3f} s drawing {len(set(counts))} tables", file=sys.stderr, flush=True)
    slots = len(groups) * S
    out = dict(tool="pnp_bench", frames=args.frames, H=args.height, W=args.width, windows=len(groups), images_solved=slots, niter_PnP=args.niter,
               device_s=round(dev_s, 3), device_ms_per_image=round(1e3 * dev_s / slots, 3), device_failed=int((d.pnp_status > 0).sum()),
               device_cached_tables_s=round(warm_s, 3), tables_s=round(tables_s, 3), distinct_tables=len(set(counts)),
               focal_px=round(float(d.init_focals.mean()), 2), true_focal_px=f)
    if not args.skip_host:
        h, host_s = run("host")
        print(f"host backend: {host_s:.3f} s", file=sys.stderr, flush=True)
        diff = max(float((d.P[k].double() - h.P[k].double()).abs().max()) for k in d.P)
        out.update(host_s=round(host_s, 2), host_ms_per_image=round(1e3 * host_s / slots, 1), speedup=round(host_s / dev_s, 1),
                   statuses_equal=bool(torch.equal(d.pnp_status == 0, h.pnp_status == 0)), max_param_abs_diff=diff)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
