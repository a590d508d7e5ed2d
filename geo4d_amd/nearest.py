"""Nearest neighbours within a radius on a cell grid, on the HIP device (csrc/nearest.hip): for every query point the nearest reference
point within ``radius`` and the number of reference points within it.

``build_grid`` bins a reference cloud into cells of side ``radius`` once; ``nearest_points`` queries a grid (or builds one) for any
number of query clouds; ``radius_outliers`` marks the points of a cloud that have fewer than ``min_neighbours`` other points within
``radius``. ``geo4d_amd.evaluation.cloud_metrics`` (accuracy, completeness, Chamfer distance, precision / recall / F-score) and
``geo4d_amd.fusion.fuse_points(min_neighbours=...)`` stand on them. The reference has no such step and nothing is ported. The rule is
stated in include/geo4d_hip.h and restated in numpy in tests/nearest_restatement.py; every output is a minimum or an integer count
over a set, so the results do not depend on the order of anything and are bitwise reproducible.

Limits: time grows with the number of points per cell, so raw unfused clouds (the same wall 64 times over) and large radii are slow:
fuse first (``geo4d_amd.fusion.fuse_points``), or pass ``voxel=`` to ``cloud_metrics``. Only the single nearest neighbour is found:
there is no k-NN, no statistical (mean-distance) outlier removal, no normals for point clouds, no ICP. Cell indices must stay below
2^20 in magnitude on every axis (points beyond are refused, not clipped); indices are int32.
"""
import torch

from . import _lib, ops

CELL_LIMIT = 1 << 20


check_radius, check_min_neighbours = ops.check_nn_radius, ops.check_min_neighbours


def check_cloud(points, mask, who, what):
    """ValueError unless points is a tensor [N, 3] and mask (None: none) a tensor [N]."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: need {what} [N, 3], got {tuple(points.shape) if torch.is_tensor(points) else type(points).__name__}")
    if mask is not None and tuple(mask.shape) != (points.shape[0],):
        raise ValueError(f"{who}: {what}_mask must be [N] = {(points.shape[0],)}, got {tuple(mask.shape)}")


def _cloud(points, mask, who, what):
    """points as fp32 [N, 3] contiguous on the HIP device and its mask; ValueError for a wrong shape, Geo4DNativeError for a CPU tensor."""
    check_cloud(points, mask, who, what)
    if not points.is_cuda:
        raise _lib.Geo4DNativeError(f"{who}: `{what}` lives on {points.device}; the search runs only on a HIP device (there is no CPU "
                                    "fallback)")
    return points.detach().float().contiguous(), None if mask is None else mask.to(points.device)


def _refuse_dropped(dropped, r, who, what):
    """fuse_points' refusal of points outside the grid, for a cell side r."""
    if dropped:
        raise ValueError(f"{who}: {dropped} {what} point(s) lie outside the cell grid: a cell index floor(x / radius) must stay below 2^20 "
                         f"in magnitude, which at radius = {r:g} means |x| < {CELL_LIMIT * r:g} on every axis; use a larger radius or "
                         "mask the outliers")


@torch.no_grad()
def build_grid(reference, *, radius, mask=None):
    """The ops.NNGrid of reference [Nr, 3] (mask [Nr] bool or None: all) for `radius`, on the HIP device; reusable for any number of
    nearest_points calls with that radius. Raises ValueError when a reference point's cell index floor(x / radius) reaches 2^20 in
    magnitude."""
    r = check_radius(radius, "build_grid")
    ref, mask = _cloud(reference, mask, "build_grid", "reference")
    grid = ops.nn_grid(ref, radius=r, mask=mask)
    _refuse_dropped(grid.dropped, r, "build_grid", "reference")
    return grid


@torch.no_grad()
def nearest_points(query, reference=None, *, radius, grid=None, query_mask=None, reference_mask=None, exclude_self=False):
    """dict(index int32 [Nq], dist2 fp32 [Nq], count int32 [Nq], grid): per query point the row of the nearest reference point within
    `radius` (-1: none; the lowest row on ties), its squared distance (+inf) and the number of reference points within `radius`.

    query [Nq, 3] and either reference [Nr, 3] (a grid is built, and returned for the next call) or `grid` (build_grid's, whose radius
    must be this one), on the HIP device; the masks [N] bool (None: all). A point takes part when its mask is set and its coordinates
    are finite; a query that takes no part gets (-1, +inf, 0). `exclude_self`: the query is the reference cloud itself, and row i is no
    neighbour of row i. Raises ValueError when a point's cell index floor(x / radius) reaches 2^20 in magnitude."""
    who = "nearest_points"
    r = check_radius(radius, who)
    if (reference is None) == (grid is None):
        raise ValueError(f"{who}: give either `reference` or `grid`, not {'both' if grid is not None else 'neither'}")
    q, query_mask = _cloud(query, query_mask, who, "query")
    if grid is None:
        grid = build_grid(reference, radius=r, mask=reference_mask)
    else:
        if not isinstance(grid, ops.NNGrid):
            raise ValueError(f"{who}: grid must be build_grid's result, got {type(grid).__name__}")
        if reference_mask is not None:
            raise ValueError(f"{who}: reference_mask belongs to the reference: a grid already has its own")
        if grid.radius != r:
            raise ValueError(f"{who}: the grid was built for radius {grid.radius:g}, not {r:g}")
    index, dist2, count, dropped = ops.nn_query(grid, q, mask=query_mask, exclude_same_row=bool(exclude_self))
    _refuse_dropped(dropped, r, who, "query")
    return dict(index=index, dist2=dist2, count=count, grid=grid)


@torch.no_grad()
def radius_outliers(points, *, radius, min_neighbours, mask=None):
    """keep bool [N]: True where at least `min_neighbours` OTHER taking-part points of the cloud lie within `radius` (the cloud is its own
    reference, row i no neighbour of row i). points [N, 3] on the HIP device, mask [N] bool (None: all); a point that takes no part
    (masked out, or not finite) has no neighbours, so it is kept only when min_neighbours is 0."""
    who = "radius_outliers"
    r = check_radius(radius, who)
    k = check_min_neighbours(min_neighbours, who)
    pts, mask = _cloud(points, mask, who, "points")
    grid = ops.nn_grid(pts, radius=r, mask=mask)
    _refuse_dropped(grid.dropped, r, who, "cloud")
    return ops.nn_query(grid, pts, mask=mask, exclude_same_row=True)[2] >= k
