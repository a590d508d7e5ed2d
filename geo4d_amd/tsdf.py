"""The static scene denoised: a truncated signed distance function (TSDF) fused from every image, and the surface points where it
crosses zero, on the HIP device (csrc/tsdf.hip).

``fusion.fuse_points`` removes duplicates, not noise: it bins points by their noisy positions. Here every voxel within ``trunc`` voxels
of an observed point (along that pixel's ray) averages, over all images that see it, the signed gap between the image's depth and the
voxel's own depth in that camera, cut off at +-``trunc`` voxels; the surface is where that average crosses zero between two
neighbouring voxels, and independent per-frame depth errors average out there. ``tsdf_points`` does that for arrays, ``tsdf_scene`` for
a ``GroupAligner`` with the masks of the export (``get_3D_model_from_scene``) and leaves the result in ``scene.tsdf``;
``get_3D_model_from_scene(tsdf_voxel=...)`` and ``save_scene(tsdf_static=...)`` write it as a glb. The reference has no such step and
nothing is ported. The rule is stated in include/geo4d_hip.h and restated in numpy in tests/tsdf_restatement.py; each voxel sums its
images in the order 0 .. n-1 in one thread, so the result is bitwise reproducible and does not depend on the table's capacity. Rows come
out ordered by voxel (cx, cy, cz), then axis.

The defaults (voxel = ``fusion.default_voxel``, truncation 4 voxels, at least 4 observations) were chosen on the synthetic scene of
tests/motion_restatement.py: at 2 % depth noise the surface points lie 0.025 RMS from the wall against 0.079 for the raw points, and with
fewer than 4 observations a handful of points survive from the sphere pixels ``segment_motion`` leaves in the static part. Nobody has
tried them on real predictions.

``tsdf_mesh`` (and ``tsdf_scene(mesh=True)``) turns the same field into one indexed triangle mesh by naive surface nets
(csrc/tsdf_mesh.hip, restated in tests/tsdf_mesh_restatement.py): one vertex per cell of eight live voxels the surface passes through,
at the mean of the cell's edge crossings, and two triangles per sign change between two neighbouring voxels, front faces toward the
cameras; ``get_3D_model_from_scene(tsdf_mesh=...)`` and ``save_scene(tsdf_mesh_static=...)`` write it as a glb. On the synthetic scene
at 2 % depth noise its vertices lie 0.017 RMS from the wall (the points: 0.025). ``min_component_faces`` / ``min_component_fraction``
drop the mesh's small detached pieces, the debris a TSDF of noisy depth leaves in front of and behind the surface (geo4d_amd/mesh.py).
``smooth_iterations`` runs that many iterations of Taubin smoothing on the mesh (mesh.smooth_mesh; 10 of them bring the noisy wall's
vertices from 0.0171 to 0.0142 RMS) and ``normals=True`` adds area-weighted unit vertex normals (mesh.vertex_normals), which the glb
then carries as NORMAL.

Limits: normals and smoothing only on request; the mesh is not simplified, and where a grid face has four sign changes a mesh edge is shared by
four triangles (a property of surface nets); one resolution; cell indices must stay below 2^20 in magnitude (samples beyond are refused,
not clipped); a surface seen by fewer than ``min_weight`` images (in weight) gives no point, and a cell with such a voxel no vertex; the
moving part has no TSDF (``motion="dynamic"`` is refused); the voxel table must hold every marked voxel, and a table that is too small
is refused with the capacity to pass, never grown silently.
"""
import math

import torch

from . import _lib, ops
from .fusion import default_voxel
from .mesh import mesh_adjacency, remove_small_components, smooth_mesh, vertex_normals
from .motion import segment_motion
from .scene_view import MeshOptions, rgba_of, scene_view, views_of

MOTION = (None, "static")
MAX_TRUNC = 8


def check_tsdf_args(voxel, trunc=4, min_weight=4.0, near=1e-3, capacity=None):
    """The fp32 voxel; ValueError for a voxel that is not finite and > 0 in fp32, a truncation that is no integer in 1..8, a min_weight
    that is not > 0, a negative near or a capacity that is no power of two."""
    try:
        v = torch.tensor(float(voxel), dtype=torch.float32).item()
    except (TypeError, ValueError):
        v = math.nan
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"tsdf_points: voxel must be finite and > 0 in fp32, got {voxel!r}")
    if isinstance(trunc, bool) or not isinstance(trunc, (int, float)) or int(trunc) != trunc or not 1 <= trunc <= MAX_TRUNC:
        raise ValueError(f"tsdf_points: trunc must be an integer number of voxels in 1..{MAX_TRUNC}, got {trunc!r}")
    if not (isinstance(min_weight, (int, float)) and min_weight > 0):
        raise ValueError(f"tsdf_points: min_weight must be > 0, got {min_weight!r}")
    if not (isinstance(near, (int, float)) and near >= 0):
        raise ValueError(f"tsdf_points: near must be >= 0, got {near!r}")
    if capacity is not None and (int(capacity) != capacity or not 1 <= capacity <= 1 << 32 or int(capacity) & (int(capacity) - 1)):
        raise ValueError(f"tsdf_points: capacity must be a power of two in 1 .. 2^32, got {capacity!r}")
    return v


@torch.no_grad()
def tsdf_points(pts3d, depth, valid, cams2world, K, rgb=None, weight=None, *, voxel, trunc=4, min_weight=4.0, near=1e-3, capacity=None):
    """dict(points fp32 [P, 3], rgba uint8 [P, 4] or None, weight fp32 [P], voxels, dropped, overflow, voxel): the surface points of
    the TSDF, on the device, ordered by voxel (cx, cy, cz) and axis.

    pts3d [n, H, W, 3] fp32 world points, depth [n, H, W] fp32 (camera z) and valid [n, H, W] bool (None: every pixel) on the HIP
    device; cams2world [n, 4, 4] camera-to-world (OpenCV axes) and K [n, 3, 3]; rgb float [n, H, W, 3] in [0, 1] or uint8 rgba
    [n, H, W, 4] (None: no colours, `rgba` None); weight [n, H, W] fp32 (None: every image counts 1; a pixel whose weight is not finite
    and > 0 is not an observation). `voxel`: the voxel's side; `trunc`: the truncation in voxels, 1..8; a surface point needs two
    neighbouring voxels of weight >= `min_weight` each (with unit weights: seen by that many images); pixels and voxels not beyond
    `near` in front of a camera are ignored there. `weight` of a point is the smaller of its two voxels' weights; `voxels` is the number
    of voxels marked and integrated. `capacity` overrides the voxel table's size (a power of two; default: >= 4 x the taking-part
    pixels); a table that is too small raises ops.TsdfTableFull naming the capacity to pass. Raises ValueError when a sample's cell
    index floor(x / voxel) reaches 2^20 in magnitude."""
    return _tsdf(pts3d, depth, valid, cams2world, K, rgb, weight, voxel, trunc, min_weight, near, capacity, MeshOptions(), points=True,
                 mesh=False)


@torch.no_grad()
def tsdf_mesh(pts3d, depth, valid, cams2world, K, rgb=None, weight=None, *, voxel, trunc=4, min_weight=4.0, near=1e-3, capacity=None,
              min_component_faces=None, min_component_fraction=None, smooth_iterations=None, smooth_pin_boundary=True, normals=False):
    """dict(vertices fp32 [V, 3], rgba uint8 [V, 4] or None, weight fp32 [V], faces int32 [T, 3], voxels, dropped, overflow, voxel): the
    surface of the TSDF as one indexed triangle mesh, on the device: naive surface nets (ops.tsdf_mesh_extract), about one vertex per
    cell the surface passes through, ordered by cell (cx, cy, cz); two triangles per sign change between two neighbouring voxels whose
    four surrounding cells are complete, ordered by voxel and axis, front faces toward the cameras. Inputs, checks and errors are
    tsdf_points'. `weight` of a vertex is the smallest weight of its cell's eight voxels, its colour that of the voxel nearest the
    surface.

    `min_component_faces` / `min_component_fraction` (None: no filter, the dict is what it was): the detached pieces of the extracted mesh
    with fewer faces than that, or than that fraction of the largest piece's, are removed (mesh.remove_small_components); vertices, faces,
    colours and weights are the filtered ones, still in their order, and the dict gains `components`, `kept_components` and
    `removed_faces`.

    `smooth_iterations` (None: no smoothing): that many iterations of Taubin smoothing at mesh.smooth_mesh's lam and mu move the
    vertices of the (filtered) mesh, the boundary vertices staying where they are unless `smooth_pin_boundary` is False; faces, colours
    and weights are untouched. `normals=True`: the dict gains `normals` fp32 [V, 3], the area-weighted unit vertex normals of the mesh as
    returned (mesh.vertex_normals). The order is extraction, component filter, smoothing, normals."""
    opts = MeshOptions(min_component_faces, min_component_fraction, smooth_iterations, smooth_pin_boundary, normals)
    return _tsdf(pts3d, depth, valid, cams2world, K, rgb, weight, voxel, trunc, min_weight, near, capacity, opts, points=False, mesh=True)


def _tsdf(pts3d, depth, valid, cams2world, K, rgb, weight, voxel, trunc, min_weight, near, capacity, opts, *, points, mesh):
    """The checks of tsdf_points, one field (ops.tsdf_field), and what is asked for of its surface: the points (`points`, rgba,
    weight), the mesh, or both (then the mesh's colours and weights are `vertex_rgba`, `vertex_weight`). As `opts` (a MeshOptions)
    says, the mesh goes through mesh.remove_small_components when either component argument is given, then through mesh.smooth_mesh
    when `smooth_iterations` is given, and mesh.vertex_normals adds `normals` (`vertex_normals` beside points), all on one corner table."""
    v = check_tsdf_args(voxel, trunc, min_weight, near, capacity)
    opts.check("tsdf_mesh")
    for t, what in ((pts3d, "pts3d"), (depth, "depth")):
        if not t.is_cuda:
            raise _lib.Geo4DNativeError(f"tsdf_points: `{what}` lives on {t.device}; the TSDF runs only on a HIP device (there is no CPU "
                                        "fallback)")
    if pts3d.dim() != 4 or pts3d.shape[-1] != 3 or tuple(depth.shape) != tuple(pts3d.shape[:3]):
        raise ValueError(f"tsdf_points: need pts3d [n, H, W, 3] and depth [n, H, W], got {tuple(pts3d.shape)} and {tuple(depth.shape)}")
    shape, dev = tuple(depth.shape), pts3d.device
    for t, what in ((valid, "valid"), (weight, "weight")):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"tsdf_points: {what} must be [n, H, W] = {shape}, got {tuple(t.shape)}")
    views = views_of(cams2world, K)
    if len(views) != shape[0]:
        raise ValueError(f"tsdf_points: {len(views)} cameras for {shape[0]} images")
    centres = torch.as_tensor(cams2world).detach().double().cpu().reshape(-1, 4, 4)[:, :3, 3].float().contiguous()
    rgba = rgba_of(rgb, shape, dev, "tsdf_points", "rgb", "the TSDF")
    Kv, f, wt, col, voxels, dropped = ops.tsdf_field(pts3d.detach().float().contiguous(), depth.detach().float().contiguous(),
                                                     None if valid is None else valid.to(dev), views.to(dev), centres.to(dev), rgba,
                                                     None if weight is None else weight.detach().float().contiguous(), voxel=v,
                                                     trunc=int(trunc), near=float(near), capacity=None if capacity is None else int(capacity))
    if dropped:
        raise ValueError(f"tsdf_points: {dropped} sample(s) lie outside the voxel grid: a cell index floor(x / voxel) must stay below 2^20 "
                         f"in magnitude, which at voxel = {v:g} means |x| < {(1 << 20) * v:g} on every axis; use a larger voxel or mask "
                         "the outliers")
    if voxels == 0:                                                 # no voxel: the empty field gives the empty outputs
        Kv, f, wt = torch.empty(0, device=dev, dtype=torch.int64), torch.empty(0, device=dev), torch.empty(0, device=dev)
        col = None if rgba is None else torch.empty((0, 4), device=dev, dtype=torch.uint8)
    out = {}
    if points:
        out["points"], out["rgba"], out["weight"] = ops.tsdf_extract(Kv, f, wt, col, voxel=v, min_weight=float(min_weight))
    out.update(voxels=voxels, dropped=0, overflow=0, voxel=v)
    if mesh:
        vertices, vcol, vw, faces = ops.tsdf_mesh_extract(Kv, f, wt, col, voxel=v, min_weight=float(min_weight))
        if opts.filtering:
            kept = remove_small_components(vertices, faces, min_faces=opts.min_component_faces, min_fraction=opts.min_component_fraction,
                                           rgba=vcol, weight=vw)
            vertices, vcol, vw, faces = kept["vertices"], kept["rgba"], kept["weight"], kept["faces"]
            out.update(components=kept["components"], kept_components=kept["kept_components"], removed_faces=kept["removed_faces"])
        if opts.smooth_iterations is not None or opts.normals:
            table = mesh_adjacency(faces, vertices.shape[0])       # one table for both: a smoothing step moves no vertex between faces
            if opts.smooth_iterations is not None:
                vertices = smooth_mesh(vertices, faces, adjacency=table, iterations=opts.smooth_iterations,
                                       pin_boundary=bool(opts.smooth_pin_boundary))
            if opts.normals:
                out["vertex_normals" if points else "normals"] = vertex_normals(vertices, faces, adjacency=table)
        out.update(vertices=vertices, faces=faces, **(dict(vertex_rgba=vcol, vertex_weight=vw) if points else dict(rgba=vcol, weight=vw)))
    return out


@torch.no_grad()
def tsdf_scene(scene, voxel=None, motion="static", *, min_conf_thr=3, thr_for_init_conf=True, is_msk=True, use_conf=False, trunc=4,
               min_weight=4.0, near=1e-3, capacity=None, mesh=False, min_component_faces=None, min_component_fraction=None,
               smooth_iterations=None, smooth_pin_boundary=True, normals=False):
    """tsdf_points on a GroupAligner; the result (see tsdf_points) is also stored as scene.tsdf. `mesh=True`: the dict additionally holds
    the surface as a triangle mesh (see tsdf_mesh) from the same field: `vertices`, `faces`, `vertex_rgba`, `vertex_weight`, without its
    small detached pieces when `min_component_faces` / `min_component_fraction` say so (see tsdf_mesh; with `mesh=False` either raises).
    `smooth_iterations` / `smooth_pin_boundary` smooth that mesh and `normals=True` adds `vertex_normals` fp32 [V, 3], as tsdf_mesh does
    (with `mesh=False` any of the three raises); the points are left as they are.

    Points, depth, colours and masks are taken as fusion.fuse_scene and get_3D_model_from_scene take them, through scene_view: scene.imgs
    (None: no colours), the masks of `min_conf_thr` / `thr_for_init_conf` (`is_msk=False`: every pixel) restricted by `motion` (None, or
    "static": not scene.dynamic_masks, which segment_motion makes with these thresholds when the scene has none; a TSDF of moving
    things is meaningless, so "dynamic" is refused). Every image counts 1; `use_conf=True` weights by scene.get_conf(). `voxel=None`
    means fusion.default_voxel, 2 * median(depth / focal) over the exported pixels. The defaults were chosen on the synthetic scene of
    tests/motion_restatement.py; nobody has tried them on real predictions."""
    if motion not in MOTION:
        raise ValueError(f"tsdf_scene: motion must be one of {MOTION}, got {motion!r} (the moving part has no TSDF)")
    check_tsdf_args(1.0 if voxel is None else voxel, trunc, min_weight, near, capacity)
    opts = MeshOptions(min_component_faces, min_component_fraction, smooth_iterations, smooth_pin_boundary, normals)
    if opts.filtering and not mesh:
        raise ValueError("tsdf_scene: min_component_faces / min_component_fraction filter the mesh; pass mesh=True")
    if opts.shaping and not mesh:
        raise ValueError("tsdf_scene: smooth_iterations / smooth_pin_boundary / normals work on the mesh; pass mesh=True")
    opts.check("tsdf_scene")
    view = scene_view(scene, "tsdf_scene", min_conf_thr=min_conf_thr, thr_for_init_conf=thr_for_init_conf, is_msk=is_msk, motion=motion,
                      segment=segment_motion)
    msk = view.mask()
    if voxel is None:
        voxel = default_voxel(view.depth, view.focals, msk, empty=1.0)   # no pixel: any voxel gives the empty cloud
    scene.tsdf = _tsdf(view.pts3d, view.depth, msk, *view.cameras, view.rgb, view.conf if use_conf else None, voxel, trunc, min_weight, near,
                       capacity, opts, points=True, mesh=bool(mesh))
    return scene.tsdf
