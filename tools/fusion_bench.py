#!/usr/bin/env python3
"""Time of the point fusion (geo4d_amd/fusion.py, csrc/fuse.hip) on the static part of a 64-image 320 x 512 synthetic scene
(tools/scene_export_bench.py's: a wavy wall with a box sliding in front; the static part by geo4d_amd.motion's default rule), at the
default voxel 2 * median(depth / focal), with colours and the confidence as weight.

Device time by HIP events round --inner back-to-back warm calls each of insert (the table reset included), compact, the torch.sort of
the (key, slot) pairs with its gather, finalize, and the whole ops.fuse_points (which also reads the two counts back); median and best of
--reps such windows. `reset_ms` is an insert whose mask is all false: the memsets and an empty pass over the mask. The baseline is the
same rule written with torch.unique(return_inverse=True) + index_add_ on int64 sums, on the same device in the same process, and its
result is compared with the kernels'. Prints one JSON line.
usage: fusion_bench.py [--frames 64] [--reduce mean] [--reps 20] [--inner 5]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geo4d_amd import fusion, motion, ops  # noqa: E402
from tools.motion_bench import device_ms  # noqa: E402
from tools.scene_export_bench import synthetic_scene  # noqa: E402

LIMIT = 1 << 20


def torch_fuse(points, rgba, weight, mask, voxel):
    """reduce="mean" of the rule in include/geo4d_hip.h with torch.unique + index_add_ (no range check: the scene is inside)."""
    v = torch.tensor(voxel, dtype=torch.float32, device=points.device)
    ok = mask & torch.isfinite(points).all(1) & torch.isfinite(weight) & (weight > 0)
    P, C, w = points[ok], rgba[ok], weight[ok]
    c = torch.floor(P / v)
    q = torch.floor((P - c * v) / v * 65536.0 + 0.5).clamp(0.0, 65535.0).long()
    wq = torch.floor(w * 128.0 + 0.5).clamp(1.0, 32767.0).long()
    ci = c.long() + LIMIT
    key = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
    ukey, inv = torch.unique(key, return_inverse=True)
    sums = torch.zeros((len(ukey), 8), dtype=torch.int64, device=points.device)
    rows = torch.cat([wq[:, None], wq[:, None] * q, wq[:, None] * C[:, :3].long(), torch.ones_like(wq)[:, None]], 1)
    sums.index_add_(0, inv, rows)
    sw, n = sums[:, 0], sums[:, 7]
    uc = torch.stack([(ukey >> 42) - LIMIT, ((ukey >> 21) & 0x1fffff) - LIMIT, (ukey & 0x1fffff) - LIMIT], 1)
    pos = ((uc.double() + sums[:, 1:4].double() / (sw.double() * 65536.0)[:, None]) * v.double()).float()
    col = torch.cat([((sums[:, 4:7] + (sw // 2)[:, None]) // sw[:, None]).to(torch.uint8), torch.full_like(sw, 255, dtype=torch.uint8)[:, None]], 1)
    return pos, col, (sw.double() / (128.0 * n.double())).float(), n.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reduce", default="mean", choices=["mean", "best"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H, W = args.frames, 320, 512
    s = synthetic_scene(n, H, W, dev)
    pts3d, depth = s["pts3d"].contiguous(), s["depth"].contiguous()
    valid = torch.ones((n, H, W), dtype=torch.bool, device=dev)
    dyn = motion.dynamic_mask(motion.motion_votes(pts3d, depth, valid, s["c2w"].double().cpu(), s["K"].double().cpu()))
    mask = (~dyn).reshape(-1).contiguous()
    points, weight = pts3d.reshape(-1, 3), s["conf"].reshape(-1).contiguous()
    rgba = torch.randint(0, 256, (n * H * W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    voxel = fusion.check_fuse_args(fusion.default_voxel(depth, torch.full((n,), s["f"], device=dev), ~dyn), args.reduce, 1)
    kw = dict(voxel=voxel, reduce=args.reduce)
    N, taking = points.shape[0], int(mask.sum())

    table = ops.fuse_insert(points, rgba, weight, mask, **kw)
    keys, slots, count = ops.fuse_compact(table)
    M = int(count)
    sort = lambda: slots[:M][torch.sort(keys[:M]).indices].contiguous()
    order = sort()
    got = ops.fuse_finalize(table, order)
    out = {"frames": n, "H": H, "W": W, "reduce": args.reduce, "points_M": N / 1e6, "taking_part_M": taking / 1e6, "voxel": voxel,
           "voxels": M, "fusion_ratio": taking / M, "capacity": table.capacity, "workspace_GB": table.need / 1e9, "reps": args.reps,
           "calls_per_window": args.inner, "device": torch.cuda.get_device_name(0)}
    none = torch.zeros_like(mask)
    for name, fn in (("reset", lambda: ops.fuse_insert(points, rgba, weight, none, **kw)),
                     ("insert", lambda: ops.fuse_insert(points, rgba, weight, mask, **kw)),
                     ("compact", lambda: ops.fuse_compact(table)), ("sort", sort), ("finalize", lambda: ops.fuse_finalize(table, order)),
                     ("fuse_points", lambda: ops.fuse_points(points, rgba, weight, mask, **kw))):
        out[name + "_ms"], out[name + "_ms_best"] = device_ms(fn, args.reps, args.inner)
    adds = taking * (8 if args.reduce == "mean" else 2)
    out["atomic_adds_M"] = adds / 1e6                                              # the accumulator atomics; the CAS that claims a slot not counted
    out["atomic_adds_G_per_s"] = adds / ((out["insert_ms"] - out["reset_ms"]) * 1e-3) / 1e9
    out["atomic_bytes_TB_per_s"] = 8 * adds / ((out["insert_ms"] - out["reset_ms"]) * 1e-3) / 1e12
    if args.reduce == "mean":
        ref = torch_fuse(points, rgba, weight, mask, voxel)
        out["torch_equal"] = all(torch.equal(a, b) for a, b in zip(got, ref))
        out["torch_ms"], out["torch_ms_best"] = device_ms(lambda: torch_fuse(points, rgba, weight, mask, voxel), max(args.reps // 4, 3), 1)
        out["speedup_vs_torch"] = out["torch_ms"] / out["fuse_points_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
