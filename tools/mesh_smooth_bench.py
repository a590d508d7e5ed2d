#!/usr/bin/env python3
"""Time of the corner table and its consumers (ops.mesh_adjacency, ops.mesh_smooth_step, ops.mesh_vertex_normals,
csrc/mesh_smooth.hip) on the surface-nets mesh of a 64-image 320 x 512 synthetic scene's static TSDF at the default voxel
(tools/tsdf_mesh_bench.py's field; vertices in voxel-key order).

Device time by HIP events round --inner back-to-back warm calls of each launch sequence: the table (count, cumsum, fill, sort and
boundary, which also allocates and reads E back), its launches one by one, one smoothing step, mesh.smooth_mesh with 10 iterations (20
launches) on a given table, the normals, and all of it together; median and best of --reps such windows. Then the same table at a
sweep of `long_row` (the row length above which a wave instead of a thread sorts a row and looks for its boundary neighbours), on the
mesh itself and on the mesh with a 4000-face fan added, which has one long row. The yardstick is the same rule written with torch ops on
the same device in the same process: index_add_ sums, which are not bit-equal (the order of their additions is not fixed), so it is a
baseline for time only; the largest difference is printed. Bytes moved per step are the compulsory ones: every table entry, the faces
the entries point into, and the positions read and written once. Prints one JSON line.
usage: mesh_smooth_bench.py [--frames 64] [--reps 20] [--inner 5] [--no-torch]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geo4d_amd import _lib, fusion, mesh, motion, ops  # noqa: E402
from geo4d_amd.scene_view import views_of  # noqa: E402
from tools.motion_bench import device_ms  # noqa: E402
from tools.scene_export_bench import synthetic_scene  # noqa: E402

SWEEP = (0, 4, 8, 16, 32, 64, 128, 1 << 30)


def torch_table(faces, Nv):
    """(flat vertex of every corner, its two neighbours) of the valid faces: what the torch statement gathers from."""
    valid = ((faces >= 0) & (faces < Nv)).all(1)
    f = faces[valid].long()
    own = f.reshape(-1)
    a, b = f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
    return f, own, a, b


def torch_boundary(own, a, b, Nv):
    v, w = torch.cat([own, own]), torch.cat([a, b])
    keep = v != w
    pair, count = torch.unique(v[keep] * Nv + w[keep], return_counts=True)
    out = torch.zeros(Nv, dtype=torch.bool, device=own.device)
    out[pair[count == 1] // Nv] = True
    return out


def torch_step(p, own, a, b, s, pinned):
    S, m = torch.zeros_like(p), torch.zeros(p.shape[0], device=p.device)
    for w in (a, b):
        keep = (w != own).float()
        S.index_add_(0, own, p[w] * keep[:, None])
        m.index_add_(0, own, keep)
    moved = (m > 0) & ~pinned
    return torch.where(moved[:, None], p + s * (S / m.clamp(min=1)[:, None] - p), p)


def torch_smooth(p, own, a, b, pinned, iterations=10, lam=0.5, mu=-0.53):
    for _ in range(iterations):
        p = torch_step(torch_step(p, own, a, b, lam, pinned), own, a, b, mu, pinned)
    return p


def torch_normals(p, f):
    n = torch.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]], dim=1)
    N = torch.zeros_like(p).index_add_(0, f.reshape(-1), n.repeat_interleave(3, 0))
    length = N.norm(dim=1, keepdim=True)
    return torch.where(length > 0, N / length.clamp(min=1e-30), torch.zeros_like(N))


def with_a_fan(vertices, faces, n=4000):
    """The mesh with a fan of n triangles round one new vertex added: one row of n entries beside the mesh's short ones."""
    Nv, dev = vertices.shape[0], faces.device
    rim = torch.arange(Nv + 1, Nv + n + 2, device=dev, dtype=torch.int32)
    fan = torch.stack([torch.full((n,), Nv, device=dev, dtype=torch.int32), rim[:-1], rim[1:]], 1)
    more = torch.rand((n + 2, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(0)) + 0.5
    return torch.cat([vertices, more]).contiguous(), torch.cat([faces, fan]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H, W = args.frames, 320, 512
    s = synthetic_scene(n, H, W, dev)
    pts3d, depth = s["pts3d"].contiguous(), s["depth"].contiguous()
    every = torch.ones((n, H, W), dtype=torch.bool, device=dev)
    c2w, Kcam = s["c2w"].double().cpu(), s["K"].double().cpu()
    static = (~motion.dynamic_mask(motion.motion_votes(pts3d, depth, every, c2w, Kcam))).contiguous()
    views, centres = views_of(c2w, Kcam).to(dev), c2w[:, :3, 3].float().contiguous().to(dev)
    voxel = torch.tensor(fusion.default_voxel(depth, torch.full((n,), s["f"], device=dev), static), dtype=torch.float32).item()
    K, f, wt, col, M, dropped = ops.tsdf_field(pts3d, depth, static, views, centres, None, None, voxel=voxel, trunc=4, near=1e-3)
    assert dropped == 0 and M > 0
    vertices, _, _, faces = ops.tsdf_mesh_extract(K, f, wt, col, voxel=voxel, min_weight=4.0)
    del K, f, wt, col, pts3d, depth
    Nv, T = vertices.shape[0], faces.shape[0]
    lib, stream = _lib.load(), ops._stream

    table = mesh.mesh_adjacency(faces, Nv)
    offsets, corners, E = table["offsets"], table["corners"], table["entries"]
    pinned = table["boundary"].view(torch.uint8)
    degree, cursor = torch.zeros(Nv, device=dev, dtype=torch.int32), torch.zeros(Nv, device=dev, dtype=torch.int32)
    unsorted, resorted = torch.empty(E, device=dev, dtype=torch.int32), torch.empty(E, device=dev, dtype=torch.int32)
    again, spare = torch.empty(Nv, device=dev, dtype=torch.uint8), torch.empty_like(vertices)
    fp, op, cp = faces.data_ptr(), offsets.data_ptr(), corners.data_ptr()
    long_row = ops.MESH_LONG_ROW
    stages = {
        "count": lambda: (degree.zero_(), _lib.check(lib.geo4d_mesh_adjacency_count(fp, T, Nv, 0, degree.data_ptr(), stream()), "count")),
        "cumsum": lambda: torch.cumsum(degree, 0, dtype=torch.int32),
        "fill": lambda: (cursor.zero_(), _lib.check(lib.geo4d_mesh_adjacency_fill(fp, T, Nv, 0, op, E, cursor.data_ptr(), unsorted.data_ptr(),
                                                                                  stream()), "fill")),
        "sort": lambda: _lib.check(lib.geo4d_mesh_adjacency_sort(op, T, Nv, E, unsorted.data_ptr(), resorted.data_ptr(), long_row, stream()), "sort"),
        "boundary": lambda: _lib.check(lib.geo4d_mesh_boundary(fp, T, Nv, op, cp, E, long_row, again.data_ptr(), stream()), "boundary"),
        "table": lambda: ops.mesh_adjacency(faces, Nv),
        "step": lambda: ops.mesh_smooth_step(vertices, faces, offsets, corners, 0.5, pinned, out=spare),
        "smooth_10": lambda: mesh.smooth_mesh(vertices, faces, iterations=10, adjacency=table),
        "normals": lambda: ops.mesh_vertex_normals(vertices, faces, offsets, corners),
        "all": lambda: mesh.vertex_normals(mesh.smooth_mesh(vertices, faces, iterations=10), faces),
    }
    for fn in stages.values():
        fn()
    torch.cuda.synchronize()
    rows = torch.diff(offsets)
    step_bytes = 4 * E + 12 * T + 2 * 12 * Nv + 4 * Nv + Nv                          # entries, faces, positions in and out, offsets, pins
    out = {"vertices_Nv": Nv, "triangles_T": T, "entries_E": E, "longest_row": int(rows.max()), "mean_row": float(rows.float().mean()),
           "boundary_vertices": int(table["boundary"].sum()), "long_row": long_row, "reps": args.reps, "calls_per_window": args.inner,
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "stages_equal_whole": torch.equal(resorted, corners) and torch.equal(again, pinned), "step_bytes": step_bytes,
           "mesh_bytes": 12 * Nv + 12 * T}
    for stage, fn in stages.items():
        out[stage + "_ms"], out[stage + "_ms_best"] = device_ms(fn, args.reps, args.inner)
    out["step_GB_per_s"] = step_bytes / out["step_ms"] / 1e6
    out["smooth_10_ms_per_launch"] = out["smooth_10_ms"] / 20
    fan_vertices, fan_faces = with_a_fan(vertices, faces)
    base = ops.mesh_adjacency(fan_faces, fan_vertices.shape[0])
    out["sweep_long_row"], out["sweep_mesh_table_ms"], out["sweep_fan_table_ms"], equal = list(SWEEP), [], [], True
    for lr in SWEEP:
        equal = equal and all(torch.equal(a, b) for a, b in zip(ops.mesh_adjacency(fan_faces, fan_vertices.shape[0], long_row=lr), base))
        out["sweep_mesh_table_ms"].append(device_ms(lambda: ops.mesh_adjacency(faces, Nv, long_row=lr), args.reps, args.inner)[0])
        out["sweep_fan_table_ms"].append(device_ms(lambda: ops.mesh_adjacency(fan_faces, fan_vertices.shape[0], long_row=lr), args.reps,
                                                   args.inner)[0])
    out["sweep_tables_equal"] = equal
    out["fan_step_ms"], _ = device_ms(lambda: ops.mesh_smooth_step(fan_vertices, fan_faces, base[0], base[1], 0.5), args.reps, args.inner)
    if not args.no_torch:
        f64, own, a, b = torch_table(faces, Nv)
        tb = torch_boundary(own, a, b, Nv)
        out["torch_boundary_equal"] = torch.equal(tb, table["boundary"])
        ours = mesh.smooth_mesh(vertices, faces, iterations=10, adjacency=table)
        out["torch_smooth_max_diff"] = float((torch_smooth(vertices, own, a, b, tb) - ours).abs().max())
        out["torch_normals_max_diff"] = float((torch_normals(ours, f64) - ops.mesh_vertex_normals(ours, faces, offsets, corners)).abs().max())
        out["torch_table_ms"], _ = device_ms(lambda: torch_boundary(*torch_table(faces, Nv)[1:], Nv), 5, 1)
        out["torch_step_ms"], _ = device_ms(lambda: torch_step(vertices, own, a, b, 0.5, tb), 5, 1)
        out["torch_smooth_10_ms"], _ = device_ms(lambda: torch_smooth(vertices, own, a, b, tb), 5, 1)
        out["torch_normals_ms"], _ = device_ms(lambda: torch_normals(vertices, f64), 5, 1)
        out["speedup_vs_torch_all"] = (out["torch_table_ms"] + out["torch_smooth_10_ms"] + out["torch_normals_ms"]) / out["all_ms"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
