#!/usr/bin/env python3
"""Time of the surface nets (ops.tsdf_mesh_extract, csrc/tsdf_mesh.hip) on the TSDF field of tools/tsdf_bench.py's scene: the static
part of a 64-image 320 x 512 synthetic scene at the default voxel, truncation 4 voxels, with colours and unit weights.

Device time by HIP events round --inner back-to-back warm calls each of the four launches (cells, count with the reset of `used`,
vertices, faces), the two torch.cumsum, and the whole ops.tsdf_mesh_extract (which also allocates and reads Q and V back); median and
best of --reps such windows. The baseline is the same rule written with torch ops (torch.searchsorted for every neighbour, gathers,
cumsum) on the same device in the same process, and its result is compared with the kernels'. Prints one JSON line.
usage: tsdf_mesh_bench.py [--frames 64] [--trunc 4] [--reps 20] [--inner 5]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geo4d_amd import _lib, fusion, motion, ops  # noqa: E402
from geo4d_amd.scene_view import views_of  # noqa: E402
from tools.motion_bench import device_ms  # noqa: E402
from tools.scene_export_bench import synthetic_scene  # noqa: E402

LIMIT = 1 << 20
STEP = (1 << 42, 1 << 21, 1)
CORNERS = [(ox, oy, oz) for ox in (0, 1) for oy in (0, 1) for oz in (0, 1)]


def edges():
    """(axis, corner p, corner q) of a cell's twelve edges in the rule's order."""
    out = []
    for a in range(3):
        lo, hi = [k for k in range(3) if k != a]
        for e in range(4):
            o = [0, 0, 0]
            o[lo], o[hi] = e & 1, e >> 1
            p = 4 * o[0] + 2 * o[1] + o[2]
            out.append((a, p, p + (4, 2, 1)[a]))
    return out


def torch_mesh(K, f, wt, col, voxel, min_weight):
    """The rule of include/geo4d_hip.h with torch ops (the scene is far from the grid's ends: int64 key arithmetic does not wrap)."""
    dev, M = K.device, K.shape[0]
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)
    v = f32(voxel)
    live = (wt >= f32(min_weight)) & (f.abs() < 1)
    s = f >= 0

    def find(target):
        at = torch.searchsorted(K, target).clamp(max=M - 1)
        return torch.where(K[at] == target, at, torch.full_like(at, -1))

    corner = torch.stack([find(K + (ox * STEP[0] + oy * STEP[1] + oz * STEP[2])) for ox, oy, oz in CORNERS], 1)
    complete = (corner >= 0).all(1) & live[corner.clamp(min=0)].all(1)
    rows = torch.arange(M, device=dev)
    ok, rings = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        m2 = corner[:, (4, 2, 1)[a]].clamp(min=0)
        ring = torch.stack([rows, find(K - STEP[b]), find(K - STEP[b] - STEP[c]), find(K - STEP[c])], 1)
        ok.append(complete & (s != s[m2]) & (ring >= 0).all(1) & complete[ring.clamp(min=0)].all(1))
        rings.append(ring)
    m, a = torch.stack(ok, 1).nonzero().unbind(1)                                    # row-major: (m, a) order
    ring = torch.stack(rings, 1)[m, a]
    ring = torch.where((f[m] < 0)[:, None], ring, ring[:, [0, 3, 2, 1]])
    used = torch.zeros(M, dtype=torch.bool, device=dev)
    used[ring.reshape(-1)] = True
    vid = torch.cumsum(used, 0) - 1
    faces = vid[ring][:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3).int()
    cell = used.nonzero()[:, 0]
    cr = corner[cell]
    fc, sc = f[cr], s[cr]
    S = torch.zeros((len(cell), 3), device=dev)
    cnt = torch.zeros(len(cell), device=dev)
    for a, p, q in edges():
        cross = sc[:, p] != sc[:, q]
        o = f32([float(x) for x in CORNERS[p]]).repeat(len(cell), 1)
        o[:, a] = fc[:, p] / (fc[:, p] - fc[:, q])
        S = torch.where(cross[:, None], S + o, S)
        cnt = cnt + cross
    Kc = K[cell]
    cells = torch.stack([(Kc >> 42) - LIMIT, ((Kc >> 21) & 0x1fffff) - LIMIT, (Kc & 0x1fffff) - LIMIT], 1)
    vertices = (cells.float() + 0.5) * v + (S / cnt[:, None]) * v
    pick = cr.gather(1, fc.abs().argmin(1, keepdim=True))[:, 0]
    return vertices, col[pick], wt[cr].min(1).values, faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--trunc", type=int, default=4)
    ap.add_argument("--min-weight", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H, W, T, near, mw = args.frames, 320, 512, args.trunc, 1e-3, args.min_weight
    s = synthetic_scene(n, H, W, dev)
    pts3d, depth = s["pts3d"].contiguous(), s["depth"].contiguous()
    every = torch.ones((n, H, W), dtype=torch.bool, device=dev)
    c2w, Kcam = s["c2w"].double().cpu(), s["K"].double().cpu()
    static = (~motion.dynamic_mask(motion.motion_votes(pts3d, depth, every, c2w, Kcam))).contiguous()
    views, centres = views_of(c2w, Kcam).to(dev), c2w[:, :3, 3].float().contiguous().to(dev)
    rgba = torch.randint(0, 256, (n, H, W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    voxel = torch.tensor(fusion.default_voxel(depth, torch.full((n,), s["f"], device=dev), static), dtype=torch.float32).item()
    K, f, wt, col, M, dropped = ops.tsdf_field(pts3d, depth, static, views, centres, rgba, None, voxel=voxel, trunc=T, near=near)
    assert dropped == 0 and M > 0
    del pts3d, depth, rgba, every, static

    lib, stream = _lib.load(), ops._stream
    complete, used = (torch.empty(M, device=dev, dtype=torch.uint8) for _ in range(2))
    counts = torch.empty(M, device=dev, dtype=torch.int32)
    cells = lambda: _lib.check(lib.geo4d_tsdf_mesh_cells(K.data_ptr(), M, f.data_ptr(), wt.data_ptr(), mw, complete.data_ptr(), stream()), "cells")
    count = lambda: _lib.check(lib.geo4d_tsdf_mesh_count(K.data_ptr(), M, complete.data_ptr(), counts.data_ptr(), used.data_ptr(), stream()), "count")
    cells(), count()
    scans = lambda: (torch.cumsum(counts, 0, dtype=torch.int64), torch.cumsum(used, 0, dtype=torch.int64))
    last_quad, last_vertex = scans()
    Q, V = int(last_quad[-1]), int(last_vertex[-1])
    first_quad, first_vertex = (last_quad - counts).contiguous(), (last_vertex - used).contiguous()
    vert, vcol, vw = torch.empty((V, 3), device=dev), torch.empty((V, 4), device=dev, dtype=torch.uint8), torch.empty(V, device=dev)
    faces = torch.empty((2 * Q, 3), device=dev, dtype=torch.int32)
    vertices = lambda: _lib.check(lib.geo4d_tsdf_mesh_vertices(K.data_ptr(), M, f.data_ptr(), wt.data_ptr(), col.data_ptr(), used.data_ptr(),
                                                               first_vertex.data_ptr(), V, voxel, vert.data_ptr(), vcol.data_ptr(), vw.data_ptr(),
                                                               stream()), "vertices")
    triangles = lambda: _lib.check(lib.geo4d_tsdf_mesh_faces(K.data_ptr(), M, f.data_ptr(), complete.data_ptr(), counts.data_ptr(),
                                                             first_quad.data_ptr(), first_vertex.data_ptr(), Q, V, faces.data_ptr(), stream()), "faces")
    vertices(), triangles()
    whole = lambda: ops.tsdf_mesh_extract(K, f, wt, col, voxel=voxel, min_weight=mw)
    got = whole()
    out = {"frames": n, "H": H, "W": W, "trunc": T, "min_weight": mw, "voxel": voxel, "voxels": M, "vertices_V": V, "triangles_T": 2 * Q,
           "complete_cells": int((complete != 0).sum()), "points_P": len(ops.tsdf_extract(K, f, wt, col, voxel=voxel, min_weight=mw)[0]),
           "reps": args.reps, "calls_per_window": args.inner, "device": torch.cuda.get_device_name(0),
           "stages_equal_whole": all(torch.equal(a, b) for a, b in zip((vert, vcol, vw, faces), got))}
    for name, fn in (("cells", cells), ("count", count), ("cumsums", scans), ("vertices", vertices), ("faces", triangles),
                     ("tsdf_mesh_extract", whole),
                     ("tsdf_extract", lambda: ops.tsdf_extract(K, f, wt, col, voxel=voxel, min_weight=mw))):
        out[name + "_ms"], out[name + "_ms_best"] = device_ms(fn, args.reps, args.inner)
    if not args.no_torch:
        ref = torch_mesh(K, f, wt, col, voxel, mw)
        out["torch_equal"] = all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(got, ref))
        out["torch_ms"], out["torch_ms_best"] = device_ms(lambda: torch_mesh(K, f, wt, col, voxel, mw), 3, 1)
        out["speedup_vs_torch"] = out["torch_ms"] / out["tsdf_mesh_extract_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
