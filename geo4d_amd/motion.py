"""Static and moving points of an aligned scene, decided from geometry alone on the HIP device (csrc/motion.hip).

The reference's results folder has a slot for this, ``dynamic_mask_{i}.png`` (dust3r/utils/misc.py:176-180), which Geo4D fills from
optical flow and SAM2 or not at all; neither is part of this engine and nothing is ported. The rule here is the project's own, stated
in include/geo4d_hip.h and restated in numpy in tests/motion_restatement.py: every pixel's world point is projected into the images up
to ``radius`` frames away and each of those votes *free* (that camera sees past the place where the point was: it has moved),
*occluded* (something is in front: no evidence) or *consistent*. A pixel is dynamic when enough of its evidence says free.

``motion_votes`` counts the votes, ``dynamic_mask`` thresholds them, ``segment_motion`` does both for a ``GroupAligner`` and leaves the
result in ``scene.dynamic_masks`` for the export (``get_3D_model_from_scene(motion=...)``, ``save_scene(dynamic_masks=True)``) and the
renderer (``render_scene(persist_static=True)``).

The defaults (radius 8, tol 0.05, min_votes 2, ratio 0.25) were chosen on the synthetic scene of tests/motion_restatement.py. Nobody
has tried them on real predictions. Limits: motion shows only where another frame looks through the vacated space, so an object that
moves along a viewing ray, or in front of nothing, stays static; depth errors beyond ``tol`` on static surfaces read as motion; there
is no spatial clean-up; clips of fewer than three images give empty masks (min_votes = 2 needs two voters).
"""
import torch

from . import _lib, ops
from .scene_view import scene_view, views_of


@torch.no_grad()
def motion_votes(pts3d, depth, valid, cams2world, K, *, radius=8, tol=0.05, near=1e-3):
    """uint8 [n, H, W, 3] = (consistent, free, occluded) votes per pixel, on the device.

    pts3d [n, H, W, 3] fp32 world points, depth [n, H, W] fp32 and valid [n, H, W] bool (None: every pixel) on the HIP device;
    cams2world [n, 4, 4] camera-to-world (OpenCV axes) and K [n, 3, 3]. Image i's pixels are voted on by the images j with
    0 < |j - i| <= radius (1..127); `tol` in (0, 1) is the relative depth tolerance, points not beyond `near` in front of a voter do
    not vote there. Invalid pixels and pixels whose point is not finite get (0, 0, 0)."""
    for t, what in ((pts3d, "pts3d"), (depth, "depth")):
        if not t.is_cuda:
            raise _lib.Geo4DNativeError(f"motion_votes: `{what}` lives on {t.device}; the votes run only on a HIP device (there is no "
                                        "CPU fallback)")
    if pts3d.dim() != 4 or pts3d.shape[-1] != 3 or tuple(depth.shape) != tuple(pts3d.shape[:3]):
        raise ValueError(f"motion_votes: need pts3d [n, H, W, 3] and depth [n, H, W], got {tuple(pts3d.shape)} and {tuple(depth.shape)}")
    if not (1 <= int(radius) <= 127) or not (0 < tol < 1):
        raise ValueError(f"motion_votes: need 1 <= radius <= 127 and 0 < tol < 1, got radius={radius}, tol={tol}")
    views = views_of(cams2world, K)
    if len(views) != pts3d.shape[0]:
        raise ValueError(f"motion_votes: {len(views)} cameras for {pts3d.shape[0]} images")
    if valid is not None:
        valid = valid.to(pts3d.device)
    return ops.motion_votes(pts3d.detach().float().contiguous(), depth.detach().float().contiguous(), valid, views.to(pts3d.device),
                            radius=radius, tol=tol, near=near)


def dynamic_mask(votes, min_votes=2, ratio=0.25):
    """bool [n, H, W] of votes [n, H, W, 3]: free >= min_votes and free >= ratio (consistent + free), compared in fp32. Occluded votes
    are no evidence and do not count. ratio is 0.25 and not 0.5 because a moving object keeps collecting consistent votes from the
    frames in which it still overlaps its old silhouette, while static points collect next to no free votes."""
    c, f = votes[..., 0].float(), votes[..., 1].float()
    return (f >= float(min_votes)) & (f >= torch.tensor(float(ratio), dtype=torch.float32, device=votes.device) * (c + f))


@torch.no_grad()
def segment_motion(scene, *, min_conf_thr=3, thr_for_init_conf=True, is_msk=True, radius=8, tol=0.05, min_votes=2, ratio=0.25, near=1e-3):
    """bool [n, H, W]: the dynamic pixels of a GroupAligner, also stored as scene.dynamic_masks.

    Valid pixels are those get_3D_model_from_scene exports (scene.get_masks() with `min_conf_thr` / `thr_for_init_conf`, set on the
    scene as the export sets them); `is_msk=False` lets every pixel vote and be voted on. The rest is the rule of motion_votes and
    dynamic_mask."""
    view = scene_view(scene, "segment_motion", min_conf_thr=min_conf_thr, thr_for_init_conf=thr_for_init_conf, is_msk=is_msk)
    votes = motion_votes(view.pts3d, view.depth, view.msk, *view.cameras, radius=radius, tol=tol, near=near)
    scene.dynamic_masks = dynamic_mask(votes, min_votes, ratio)
    return scene.dynamic_masks
