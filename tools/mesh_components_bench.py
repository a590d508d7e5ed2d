#!/usr/bin/env python3
"""Time of the mesh components (ops.mesh_components, ops.mesh_select, csrc/mesh_components.hip) on two meshes of a 64-image 320 x 512
synthetic scene (tools/tsdf_mesh_bench.py's): (a) the surface-nets mesh of its static part's TSDF at the default voxel, whose vertices
are in voxel-key order, and (b) the per-image sheet mesh of the same static mask (ops.scene_mesh_faces), n H W vertices in raster order.

Device time by HIP events round --inner back-to-back warm calls of each launch sequence (hook with the resets of `touched` and `parent`,
flatten, count with the reset of the counters), and of the whole ops.mesh_components followed by ops.mesh_select of the components
holding at least 5 % of the largest one's faces (which also allocate and read C and (V', T') back); median and best of --reps such
windows. The yardstick is the same rule written with torch ops on the same device in the same process: the minimum label of each valid
face scattered to its vertices (scatter_reduce_ amin), then pointer jumping, repeated to a fixed point; its result is compared with the
kernels'. Prints one JSON line per mesh.
usage: mesh_components_bench.py [--frames 64] [--reps 20] [--inner 5] [--mesh tsdf|sheets|both] [--no-torch]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geo4d_amd import _lib, fusion, motion, ops  # noqa: E402
from geo4d_amd.mesh import keep_rule  # noqa: E402
from geo4d_amd.scene_view import views_of  # noqa: E402
from tools.motion_bench import device_ms  # noqa: E402
from tools.scene_export_bench import synthetic_scene  # noqa: E402


def torch_components(faces, Nv):
    """The rule of include/geo4d_hip.h with torch ops; also returns how many scatter rounds it took."""
    dev = faces.device
    valid = ((faces >= 0) & (faces < Nv)).all(1)
    f = faces[valid].long()
    flat = f.reshape(-1)
    ids = torch.arange(Nv, device=dev)
    touched = torch.zeros(Nv, dtype=torch.bool, device=dev)
    touched[flat] = True
    label, rounds = ids, 0
    while True:
        rounds += 1
        new = label.clone().scatter_reduce_(0, flat, label[f].min(1).values.repeat_interleave(3), "amin")
        while True:                                                                  # pointer jumping: label[v] <= v, so this ends at roots
            jumped = new[new]
            if torch.equal(jumped, new):
                break
            new = jumped
        if torch.equal(new, label):
            break
        label = new
    is_root = touched & (label == ids)
    dense = torch.cumsum(is_root, 0) - is_root.long()
    C = int(is_root.sum())
    vertex_component = torch.where(touched, dense[label], torch.full_like(dense, -1)).int()
    face_component = torch.full((faces.shape[0],), -1, dtype=torch.int32, device=dev)
    face_component[valid] = vertex_component[f[:, 0]]
    return (vertex_component, face_component, torch.bincount(vertex_component[touched].long(), minlength=C).int(),
            torch.bincount(face_component[valid].long(), minlength=C).int()), rounds


def torch_select(vertices, faces, keep_face, rgba):
    Nv = vertices.shape[0]
    kept = keep_face & ((faces >= 0) & (faces < Nv)).all(1)
    f = faces[kept].long()
    keep_vertex = torch.zeros(Nv, dtype=torch.bool, device=faces.device)
    keep_vertex[f.reshape(-1)] = True
    new_row = torch.cumsum(keep_vertex, 0) - 1
    return vertices[keep_vertex], rgba[keep_vertex], None, new_row[f].int(), keep_vertex.nonzero()[:, 0].int()


def time_mesh(name, vertices, rgba, faces, args):
    dev, Nv, T = faces.device, vertices.shape[0], faces.shape[0]
    lib, stream = _lib.load(), ops._stream
    parent, root = (torch.empty(Nv, device=dev, dtype=torch.int32) for _ in range(2))
    touched, is_root = (torch.empty(Nv, device=dev, dtype=torch.uint8) for _ in range(2))
    hook = lambda: _lib.check(lib.geo4d_mesh_components_hook(faces.data_ptr(), T, Nv, 0, parent.data_ptr(), touched.data_ptr(), stream()), "hook")
    flatten = lambda: _lib.check(lib.geo4d_mesh_components_flatten(parent.data_ptr(), touched.data_ptr(), Nv, root.data_ptr(), is_root.data_ptr(),
                                                                   stream()), "flatten")
    hook(), flatten()
    scan = lambda: torch.cumsum(is_root, 0, dtype=torch.int64)
    last = scan()
    C = int(last[-1])
    first = (last - is_root).contiguous()
    vc, fc = torch.empty(Nv, device=dev, dtype=torch.int32), torch.empty(T, device=dev, dtype=torch.int32)
    cv, cf = (torch.empty(C, device=dev, dtype=torch.int32) for _ in range(2))
    count = lambda: _lib.check(lib.geo4d_mesh_components_count(faces.data_ptr(), T, Nv, 0, root.data_ptr(), first.data_ptr(), C, vc.data_ptr(),
                                                               fc.data_ptr(), cv.data_ptr(), cf.data_ptr(), stream()), "count")
    count()

    def whole():
        labels = ops.mesh_components(faces, Nv)
        keep = torch.tensor(keep_rule(labels[3], min_fraction=0.05) + [False], device=dev)
        return labels, ops.mesh_select(vertices, faces, keep[labels[1].long()], rgba)

    labels, selected = whole()
    sizes = torch.sort(cf, descending=True).values
    out = {"mesh": name, "vertices_Nv": Nv, "triangles_T": T, "components_C": C, "largest_faces": int(sizes[0]), "second_faces": int(sizes[1]) if C > 1 else 0,
           "untouched_vertices": int((vc < 0).sum()), "kept_vertices": len(selected[0]), "kept_triangles": len(selected[3]),
           "reps": args.reps, "calls_per_window": args.inner, "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "stages_equal_whole": all(torch.equal(a, b) for a, b in zip((vc, fc, cv, cf), labels))}
    for stage, fn in (("hook", hook), ("flatten", flatten), ("cumsum", scan), ("count", count),     # flatten only reads what hook left
                      ("components", lambda: ops.mesh_components(faces, Nv)), ("components_select", whole)):
        out[stage + "_ms"], out[stage + "_ms_best"] = device_ms(fn, args.reps, args.inner)
    if not args.no_torch:
        ref, rounds = torch_components(faces, Nv)
        out["torch_rounds"] = rounds
        out["torch_equal"] = all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(labels, ref))
        keep = torch.tensor(keep_rule(ref[3], min_fraction=0.05) + [False], device=dev)
        picked = torch_select(vertices, faces, keep[ref[1].long()], rgba)
        out["torch_select_equal"] = all(b is None or (a.shape == b.shape and torch.equal(a, b)) for a, b in zip(selected, picked))
        out["torch_components_ms"], out["torch_components_ms_best"] = device_ms(lambda: torch_components(faces, Nv), 3, 1)
        out["torch_select_ms"], _ = device_ms(lambda: torch_select(vertices, faces, keep[ref[1].long()], rgba), 3, 1)
        out["speedup_vs_torch"] = (out["torch_components_ms"] + out["torch_select_ms"]) / out["components_select_ms"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--mesh", choices=("tsdf", "sheets", "both"), default="both")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H, W = args.frames, 320, 512
    s = synthetic_scene(n, H, W, dev)
    pts3d, depth = s["pts3d"].contiguous(), s["depth"].contiguous()
    every = torch.ones((n, H, W), dtype=torch.bool, device=dev)
    c2w, Kcam = s["c2w"].double().cpu(), s["K"].double().cpu()
    static = (~motion.dynamic_mask(motion.motion_votes(pts3d, depth, every, c2w, Kcam))).contiguous()
    rgba = torch.randint(0, 256, (n, H, W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    if args.mesh in ("tsdf", "both"):
        views, centres = views_of(c2w, Kcam).to(dev), c2w[:, :3, 3].float().contiguous().to(dev)
        voxel = torch.tensor(fusion.default_voxel(depth, torch.full((n,), s["f"], device=dev), static), dtype=torch.float32).item()
        K, f, wt, col, M, dropped = ops.tsdf_field(pts3d, depth, static, views, centres, rgba, None, voxel=voxel, trunc=4, near=1e-3)
        assert dropped == 0 and M > 0
        vertices, vcol, _, faces = ops.tsdf_mesh_extract(K, f, wt, col, voxel=voxel, min_weight=4.0)
        del K, f, wt, col
        time_mesh("tsdf", vertices, vcol, faces, args)
        del vertices, vcol, faces
    if args.mesh in ("sheets", "both"):
        faces, count = ops.scene_mesh_faces(static, n, H, W, dev)
        faces = faces[:int(count)].contiguous()
        time_mesh("sheets", pts3d.reshape(-1, 3), rgba.reshape(-1, 4), faces, args)


if __name__ == "__main__":
    main()
