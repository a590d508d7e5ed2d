#!/usr/bin/env python3
"""Time of the nearest-neighbour search (geo4d_amd/nearest.py, csrc/nearest.hip) on the fused static cloud of a 64-image 320 x 512
synthetic scene (tools/fusion_bench.py's, at the default voxel), queried by a jittered copy of itself at radius = 4 voxel.

Device time by HIP events round --inner back-to-back warm calls each of the grid build (ops.nn_grid: keys, sort, unique, cumsum, gather,
one read-back), the whole query (ops.nn_query: keys, sort, the query kernel, one read-back), the query kernel alone on sorted queries,
one evaluation.cloud_metrics call and one nearest.radius_outliers call at 2 voxel; median and best of --reps such windows. `candidates`
is the number of (query, reference) pairs the query kernel looks at: the points in the 27 cells round every query. The baseline, for
time only, is brute force on the same device in the same process: chunked torch.cdist + min over a subset of the queries against the
whole reference, scaled to all queries; its indices are compared with the kernel's on that subset. Prints one JSON line.
usage: nearest_bench.py [--frames 64] [--reps 20] [--inner 5] [--brute 8192]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geo4d_amd import _lib, evaluation, fusion, motion, nearest, ops  # noqa: E402
from tools.motion_bench import device_ms  # noqa: E402
from tools.scene_export_bench import synthetic_scene  # noqa: E402

LIMIT = 1 << 20


def candidates(grid, query):
    """The number of points in the 27 cells round every query (the scene is well inside the grid: no range check)."""
    c = torch.floor(query / torch.tensor(grid.radius, dtype=torch.float32, device=query.device)).long()
    per_cell = (grid.cell_start[1:] - grid.cell_start[:-1]).long()
    total = 0
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                key = ((c[:, 0] + dx + LIMIT) << 42) | ((c[:, 1] + dy + LIMIT) << 21) | (c[:, 2] + dz + LIMIT)
                at = torch.searchsorted(grid.cell_keys, key).clamp(max=len(grid.cell_keys) - 1)
                total += int(per_cell[at][grid.cell_keys[at] == key].sum())
    return total


def brute(query, reference, radius, chunk=1024):
    """(index, dist2) of the nearest reference within radius by torch.cdist + min, `chunk` queries at a time."""
    idx, d2 = [], []
    for s in range(0, len(query), chunk):
        d, i = torch.cdist(query[s:s + chunk], reference).min(1)
        idx.append(torch.where(d <= radius, i, torch.full_like(i, -1)))
        d2.append(d * d)
    return torch.cat(idx), torch.cat(d2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--brute", type=int, default=8192)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H, W = args.frames, 320, 512
    s = synthetic_scene(n, H, W, dev)
    pts3d, depth = s["pts3d"].contiguous(), s["depth"].contiguous()
    valid = torch.ones((n, H, W), dtype=torch.bool, device=dev)
    dyn = motion.dynamic_mask(motion.motion_votes(pts3d, depth, valid, s["c2w"].double().cpu(), s["K"].double().cpu()))
    voxel = fusion.check_fuse_args(fusion.default_voxel(depth, torch.full((n,), s["f"], device=dev), ~dyn), "mean", 1)
    ref = fusion.fuse_points(pts3d.reshape(-1, 3), None, s["conf"].reshape(-1).contiguous(), (~dyn).reshape(-1), voxel=voxel)["points"].contiguous()
    jitter = (torch.rand(ref.shape, generator=torch.Generator().manual_seed(0)) - 0.5).to(dev) * voxel
    query = (ref + jitter).contiguous()
    r = nearest.check_radius(4 * voxel)
    N = len(ref)

    grid = ops.nn_grid(ref, radius=r)
    index, dist2, count, _ = ops.nn_query(grid, query)
    order, taking, _, _ = ops._nn_sorted_rows(query, None, r)
    lib = _lib.load()

    def kernel():
        _lib.check(lib.geo4d_nn_query(query.data_ptr(), order.data_ptr(), taking, N, grid.cell_keys.data_ptr(), grid.cell_start.data_ptr(),
                                      len(grid.cell_keys), grid.ref_sorted.data_ptr(), grid.ref_row.data_ptr(), grid.n_taking, grid.n_reference,
                                      r, 0, index.data_ptr(), dist2.data_ptr(), count.data_ptr(), ops._stream()), "geo4d_nn_query")

    visited = candidates(grid, query)
    out = {"frames": n, "H": H, "W": W, "voxel": voxel, "radius": r, "points": N, "cells": len(grid.cell_keys),
           "points_per_cell": N / len(grid.cell_keys), "candidates_M": visited / 1e6, "candidates_per_query": visited / N,
           "within_per_query": float(count.float().mean()), "matched": int((index >= 0).sum()), "reps": args.reps,
           "calls_per_window": args.inner, "device": torch.cuda.get_device_name(0)}
    for name, fn in (("grid", lambda: ops.nn_grid(ref, radius=r)), ("query", lambda: ops.nn_query(grid, query)), ("query_kernel", kernel),
                     ("cloud_metrics", lambda: evaluation.cloud_metrics(query, ref, max_dist=r, thresholds=(voxel, 2 * voxel, r))),
                     ("radius_outliers", lambda: nearest.radius_outliers(ref, radius=2 * voxel, min_neighbours=4))):
        out[name + "_ms"], out[name + "_ms_best"] = device_ms(fn, args.reps, args.inner)
    out["candidates_G_per_s"] = visited / (out["query_kernel_ms"] * 1e-3) / 1e9
    sub = query[torch.randperm(N, generator=torch.Generator().manual_seed(1))[:args.brute].to(dev)].contiguous()
    got = ops.nn_query(grid, sub)
    b_idx, _ = brute(sub, ref, r)
    out["brute_queries"] = len(sub)
    out["brute_index_agrees"] = float((b_idx == got[0]).float().mean())            # cdist rounds differently: ties and the shell may differ
    ms, best = device_ms(lambda: brute(sub, ref, r), max(args.reps // 4, 3), 1)
    out["brute_ms_scaled"], out["brute_ms_scaled_best"] = ms * N / len(sub), best * N / len(sub)
    out["speedup_vs_brute"] = out["brute_ms_scaled"] / out["query_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
