"""Depth, field of view and focal from a point map alone: utils/geometry.py's point_map_to_depth family on the device.

The reference's shipped command line initialises the global alignment from these (scripts/evaluation/test_geo4d.py:368 hard-codes
use_raymap = False -> init_im_poses.align_group_prefix :244-271): the reference frame of every window goes through
``point_map_to_depth`` - nearest down-sampling, a device->host copy, one scipy least_squares per map - and the focal in pixels is read
off the recovered field of view. Here the solve is ``ops.focal_shift`` (csrc/focal_shift.hip): every map in one enqueue, no copy of
the maps, and the small closed-form conversions below run as tensor ops on the solver's device outputs. Names and signatures are the
reference's.
"""
import math

import torch

from . import ops


def image_plane_uv(width, height, aspect_ratio=None, dtype=None, device=None):
    """[height, width, 2] of (u, v): pixel centres of an image plane whose corners are (-width, -height) / diagonal and
    (+width, +height) / diagonal (utils/geometry.py:217-229; `aspect_ratio` overrides width / height for the spans only)."""
    ar = width / height if aspect_ratio is None else aspect_ratio
    norm = math.sqrt(1.0 + ar * ar)
    half_u, half_v = (ar / norm) * (width - 1) / width, (1.0 / norm) * (height - 1) / height
    u = torch.linspace(-half_u, half_u, width, dtype=dtype, device=device)
    v = torch.linspace(-half_v, half_v, height, dtype=dtype, device=device)
    return torch.stack([u[None, :].expand(height, width), v[:, None].expand(height, width)], -1)


def intrinsics_from_fov_xy(fov_x, fov_y):
    """[..., 3, 3] normalised OpenCV intrinsics (image = unit square, principal point at its centre) of the two fields of view, radians
    (utils/geometry.py:146-160)."""
    fov_x, fov_y = torch.as_tensor(fov_x), torch.as_tensor(fov_y)
    fx, fy = 0.5 / torch.tan(fov_x / 2), 0.5 / torch.tan(fov_y / 2)
    K = torch.zeros(fx.shape + (3, 3), dtype=fx.dtype, device=fx.device)
    K[..., 0, 0], K[..., 1, 1] = fx, fy
    K[..., 0, 2] = K[..., 1, 2] = 0.5
    K[..., 2, 2] = 1.0
    return K


def _solve(points, mask, downsample_size, z_offset=None):
    """ops.focal_shift on [..., H, W, 3] points with an optional [..., H, W] selection; returns (shift, focal, status), each [N]."""
    H, W = points.shape[-3], points.shape[-2]
    flat = points.reshape(-1, H, W, 3)
    weight = None if mask is None else mask.reshape(-1, H, W).to(torch.float32)
    return ops.focal_shift(flat, weight, 0.5, downsample_size, z_offset)


def point_map_to_depth(points, mask=None, downsample_size=(64, 64)):
    """points [..., H, W, 3] on the device, mask [..., H, W] bool or None -> (depth [..., H, W] = z + shift, fov_x [...], fov_y [...],
    shift [...]) as utils/geometry.py:162-215 returns them, without leaving the device. A map the solver could not fit (fewer than 3
    selected pixels, non-finite values) comes back with shift 0 and the solver's placeholder focal 1; `ops.focal_shift` exposes the status."""
    H, W = points.shape[-3], points.shape[-2]
    lead = points.shape[:-3]
    shift, focal, _ = _solve(points, mask, downsample_size)
    diagonal = math.sqrt(H * H + W * W)
    fov_x = 2 * torch.atan(W / diagonal / focal)
    fov_y = 2 * torch.atan(H / diagonal / focal)
    depth = (points.reshape(-1, H, W, 3)[..., 2] + shift[:, None, None]).reshape(points.shape[:-1])
    return depth, fov_x.reshape(lead), fov_y.reshape(lead), shift.reshape(lead)


def focal_pixels_from_fov(fov_x, fov_y, H, W):
    """The focal in pixels align_group_prefix reads off the fields of view (init_im_poses.py:262-263): mean of K00 * W and K11 * H."""
    K = intrinsics_from_fov_xy(fov_x, fov_y)
    return (K[..., 0, 0] * W + K[..., 1, 1] * H) / 2


def recover_focal_pixels(points, mask=None, downsample_size=None, z_offset=None, return_status=False):
    """Focal in pixels of every map of `points` [..., H, W, 3] = ((K00 * W) + (K11 * H)) / 2 of the recovered intrinsics, as
    init_im_poses.align_group_prefix :261-263 computes it (downsample_size None = (H, W), its choice). `mask`: bool, or any per-pixel
    value selected where > 0.5 after conversion to float. `z_offset`: device fp32 scalar added to z (the caller's z normalisation)."""
    H, W = points.shape[-3], points.shape[-2]
    _, focal, status = _solve(points, mask, (H, W) if downsample_size is None else downsample_size, z_offset)
    diagonal = math.sqrt(H * H + W * W)
    out = focal_pixels_from_fov(2 * torch.atan(W / diagonal / focal), 2 * torch.atan(H / diagonal / focal), H, W).reshape(points.shape[:-3])
    return (out, status.reshape(points.shape[:-3])) if return_status else out
