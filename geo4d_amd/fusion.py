"""The aligned scene's points fused into one cloud: one point per occupied voxel, on the HIP device (csrc/fuse.hip).

The export, the renderer and the static / moving split all treat the aligned scene as n separate images, so a wall seen in 64 frames is
exported 64 times. ``fuse_points`` bins points into voxels of side ``voxel`` and reduces every voxel to one point: the weighted mean of
its points' positions and colours (``reduce="mean"``) or its point of highest weight (``reduce="best"``). ``fuse_scene`` does that for a
``GroupAligner`` with the masks of the export (``get_3D_model_from_scene``), weighted by the scene's confidence, and leaves the result in
``scene.fused``; ``get_3D_model_from_scene(fuse_voxel=...)`` and ``save_scene(fuse_static=...)`` write it as a glb. The reference has no
such step and nothing is ported. The rule is stated in include/geo4d_hip.h and restated in numpy in tests/fusion_restatement.py; the
per-voxel sums are integers, so the result does not depend on the order of the points and is bitwise reproducible, and the rows come
out sorted by voxel (cx, cy, cz).

This removes duplicates, not noise: points are binned by their noisy positions, so every voxel keeps its bias (at 2 % depth noise the
fused points of the synthetic scene are no closer to the wall than the raw ones). The one kind of noise it can name is the isolated
point: ``min_neighbours`` leaves out fused points with too few other fused points near them (csrc/nearest.hip). Limits: cell indices
must stay below 2^20 in magnitude on every axis (points beyond are refused, not clipped); offsets inside a voxel are kept to 1 / 65536
of its side and weights to 1 / 128 within [1 / 128, 256); a surface that crosses a voxel obliquely still leaves one point per voxel it
touches.
"""
import math

import torch

from . import _lib, ops
from .motion import segment_motion
from .scene_view import MOTION, rgba_of, scene_view

REDUCE = tuple(ops.FUSE_REDUCE)
CELL_LIMIT = 1 << 20


def check_neighbour_args(who, min_neighbours, neighbour_radius):
    """ValueError for a min_neighbours that is not an integer >= 0 or a neighbour_radius (None: the default) that is not finite and
    > 0 in fp32."""
    ops.check_min_neighbours(min_neighbours, who)
    if neighbour_radius is not None:
        ops.check_nn_radius(neighbour_radius, who, "neighbour_radius")


def check_fuse_args(voxel, reduce, min_count):
    """The fp32 voxel; ValueError for a voxel that is not finite and > 0 in fp32, an unknown reduce or a min_count below 1."""
    try:
        v = torch.tensor(float(voxel), dtype=torch.float32).item()
    except (TypeError, ValueError):
        v = math.nan
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"fuse_points: voxel must be finite and > 0 in fp32, got {voxel!r}")
    if reduce not in REDUCE:
        raise ValueError(f"fuse_points: reduce must be one of {REDUCE}, got {reduce!r}")
    if int(min_count) != min_count or min_count < 1:
        raise ValueError(f"fuse_points: min_count must be an integer >= 1, got {min_count!r}")
    return v


@torch.no_grad()
def fuse_points(points, colors=None, weight=None, mask=None, *, voxel, reduce="mean", min_count=1, capacity=None, min_neighbours=0,
                neighbour_radius=None):
    """dict(points fp32 [M, 3], rgba uint8 [M, 4] or None, weight fp32 [M], count int32 [M], voxel): one row per occupied voxel, in
    (cx, cy, cz) order, on the device.

    points [N, 3] fp32; colors float [N, 3] in [0, 1] or uint8 rgba [N, 4] (None: no colours, `rgba` None); weight [N] fp32 (None:
    every weight is 1); mask [N] bool (None: all), all on the HIP device. A point takes part when its mask is set, its coordinates are
    finite and its weight is finite and > 0. reduce "mean": the weighted mean position and colour and the mean weight of the voxel's
    points; "best": the voxel's point of highest weight (the lowest row on ties), copied bit for bit. `count` is the number of points
    in the voxel; voxels with fewer than `min_count` are left out. `capacity` overrides the hash table's size (a power of two >= N).
    `min_neighbours` > 0: after the reduction and `min_count`, fused points with fewer than that many OTHER fused points within
    `neighbour_radius` are left out as well (geo4d_amd.nearest.radius_outliers: what removes an isolated floating point);
    `neighbour_radius=None` means 2 * voxel, a default nobody has tried on real predictions. `min_neighbours=0` launches nothing new.
    Raises ValueError when a point's cell index floor(x / voxel) reaches 2^20 in magnitude."""
    v = check_fuse_args(voxel, reduce, min_count)
    check_neighbour_args("fuse_points", min_neighbours, neighbour_radius)
    if not points.is_cuda:
        raise _lib.Geo4DNativeError(f"fuse_points: `points` lives on {points.device}; the fusion runs only on a HIP device (there is no "
                                    "CPU fallback)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"fuse_points: need points [N, 3], got {tuple(points.shape)}")
    N, dev = points.shape[0], points.device
    for t, what in ((weight, "weight"), (mask, "mask")):
        if t is not None and tuple(t.shape) != (N,):
            raise ValueError(f"fuse_points: {what} must be [N] = {(N,)}, got {tuple(t.shape)}")
    rgba = rgba_of(colors, (N,), dev, "fuse_points", "colors", "the fusion", "[N, {}] = ")
    pts, rgba, w, count, dropped = ops.fuse_points(points.detach().float().contiguous(), rgba,
                                                   None if weight is None else weight.detach().float().contiguous(),
                                                   None if mask is None else mask.to(dev), voxel=v, reduce=reduce, capacity=capacity)
    if dropped:
        raise ValueError(f"fuse_points: {dropped} point(s) lie outside the voxel grid: a cell index floor(x / voxel) must stay below 2^20 "
                         f"in magnitude, which at voxel = {v:g} means |x| < {CELL_LIMIT * v:g} on every axis; use a larger voxel or mask "
                         "the outliers")
    if min_count > 1:
        keep = count >= int(min_count)
        pts, w, count, rgba = pts[keep], w[keep], count[keep], None if rgba is None else rgba[keep]
    if min_neighbours > 0:
        r = ops.check_nn_radius(2 * v if neighbour_radius is None else neighbour_radius, "fuse_points", "neighbour_radius")
        grid = ops.nn_grid(pts, radius=r)                           # geo4d_amd.nearest.radius_outliers, from below it in the scene layer
        if grid.dropped:
            raise ValueError(f"fuse_points: {grid.dropped} fused point(s) lie outside the neighbour search's cell grid: at neighbour_radius "
                             f"= {r:g} it needs |x| < {CELL_LIMIT * r:g} on every axis; use a larger neighbour_radius")
        keep = ops.nn_query(grid, pts, exclude_same_row=True)[2] >= min_neighbours
        pts, w, count, rgba = pts[keep], w[keep], count[keep], None if rgba is None else rgba[keep]
    return dict(points=pts, rgba=rgba, weight=w, count=count, voxel=v)


def default_voxel(depth, focals, mask=None, empty=None):
    """2 * median(depth / focal) over the pixels of `mask` (None: all), i.e. twice the median pixel footprint, on the device: depth
    [n, H, W], focals [n] or [n, 1]; fp32, the lower median (torch.median). `empty` (None) when the mask keeps no pixel."""
    r = depth.float() / focals.float().reshape(-1, 1, 1)
    r = r.reshape(-1) if mask is None else r[mask]
    return 2.0 * float(torch.median(r)) if r.numel() else empty


@torch.no_grad()
def fuse_scene(scene, *, voxel=None, motion="static", min_conf_thr=3, thr_for_init_conf=True, is_msk=True, reduce="mean", min_count=1,
               min_neighbours=0, neighbour_radius=None):
    """fuse_points on a GroupAligner; the result (see fuse_points) is also stored as scene.fused.

    Points, colours and masks are taken as get_3D_model_from_scene takes them, through scene_view: scene.imgs (None: no colours), the
    masks of `min_conf_thr` / `thr_for_init_conf` (`is_msk=False`: every pixel) restricted by `motion` (None, "static", "dynamic") to
    scene.dynamic_masks, which segment_motion makes with these thresholds when the scene has none. The weight is the scene's
    confidence, scene.get_conf(), so a pixel whose confidence is not > 0 takes no part. `voxel=None` means default_voxel: 2 *
    median(depth / focal) over the exported pixels, twice the median pixel footprint. That default gave 22.6 times fewer points on the
    synthetic scene of tests/motion_restatement.py; nobody has tried it on real predictions. `min_neighbours` / `neighbour_radius`
    are fuse_points': isolated fused points are left out."""
    if motion not in MOTION:
        raise ValueError(f"fuse_scene: motion must be one of {MOTION}, got {motion!r}")
    check_fuse_args(1.0 if voxel is None else voxel, reduce, min_count)
    check_neighbour_args("fuse_scene", min_neighbours, neighbour_radius)
    view = scene_view(scene, "fuse_scene", min_conf_thr=min_conf_thr, thr_for_init_conf=thr_for_init_conf, is_msk=is_msk, motion=motion,
                      segment=segment_motion)
    msk = view.mask()
    if voxel is None:
        voxel = default_voxel(view.depth, view.focals, msk, empty=1.0)   # nothing to fuse: any voxel gives the empty cloud
    scene.fused = fuse_points(view.pts3d.reshape(-1, 3), None if view.rgb is None else view.rgb.reshape(-1, 3), view.conf.reshape(-1),
                              None if msk is None else msk.reshape(-1), voxel=voxel, reduce=reduce, min_count=min_count,
                              min_neighbours=min_neighbours, neighbour_radius=neighbour_radius)
    return scene.fused
