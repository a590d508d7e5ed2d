"""One view of the aligned scene for everything that consumes it: the Python counterpart of csrc/scene_view.h.

The export, the motion split, the voxel fusion, the TSDF and the renderer all take a ``GroupAligner`` apart in the same way;
``scene_view`` is the one place that does it, so "points, colours and masks as get_3D_model_from_scene takes them" holds by
construction. Beside it live what those modules share: the kernels' camera rows, colour quantisation and source lists, the ``motion``
values, the voxel arguments' convention (``voxel_option``) and the record of the mesh options (``MeshOptions``). This is the base of
the scene layer: scene_view <- motion <- {fusion, tsdf} <- render <- scene_export, with mesh beside.
"""
from dataclasses import dataclass
from functools import cached_property

import numpy as np
import torch

from . import _lib
from .mesh import check_keep_args, check_smooth_args

MOTION = (None, "static", "dynamic")


def views_of(cams2world, K):
    """[V, 16] fp32 on the host: rows 0..2 of inv(cams2world) (4x4 algebra in fp64), then fx, fy, cx, cy of K [V, 3, 3]."""
    c2w = torch.as_tensor(cams2world).detach().double().cpu().numpy().reshape(-1, 4, 4)
    K = torch.as_tensor(K).detach().double().cpu().numpy().reshape(-1, 3, 3)
    if len(c2w) != len(K):
        raise ValueError(f"render: {len(c2w)} camera poses but {len(K)} intrinsics")
    w2c = np.linalg.inv(c2w)
    v = np.concatenate([w2c[:, :3, :].reshape(-1, 12), K[:, 0, 0:1], K[:, 1, 1:2], K[:, 0, 2:3], K[:, 1, 2:3]], 1)
    return torch.from_numpy(v.astype(np.float32))


def rgba_of(colors, lead, device, who, arg, step, named=""):
    """u8 [*lead, 4] of `colors`: a u8 rgba as it is, or float [*lead, 3] in [0, 1] quantised as ops.scene_points does (clip(c * 255 +
    0.5, 0, 255) truncated, in fp32) with alpha 255. The messages speak as `who` of its argument `arg` and of `step`, the thing that
    runs; `named` puts a name in front of the shapes they quote ("[N, {}] = ")."""
    if colors is None:
        return None
    if not colors.is_cuda:
        raise _lib.Geo4DNativeError(f"{who}: `{arg}` lives on {colors.device}; {step} runs only on a HIP device")
    if colors.dtype == torch.uint8:
        if tuple(colors.shape) != (*lead, 4):
            raise ValueError(f"{who}: uint8 colours must be rgba {named.format(4)}{(*lead, 4)}, got {tuple(colors.shape)}")
        return colors.contiguous()
    if tuple(colors.shape) != (*lead, 3):
        raise ValueError(f"{who}: float colours must be {named.format(3)}{(*lead, 3)}, got {tuple(colors.shape)}")
    rgb = ((colors.float() * 255.0) + 0.5).clamp(0.0, 255.0).to(torch.uint8)
    return torch.cat([rgb, torch.full((*lead, 1), 255, dtype=torch.uint8, device=device)], -1).contiguous()


def scene_cameras(scene):
    """(cams2world [n, 4, 4], K [n, 3, 3]) fp64 on the host from a GroupAligner's poses, focals and principal points."""
    n = scene.n
    K = torch.zeros((n, 3, 3), dtype=torch.float64)
    K[:, 0, 0] = K[:, 1, 1] = scene.get_focals().detach().reshape(n).double().cpu()
    K[:, :2, 2] = scene.get_principal_points().detach().double().cpu()
    K[:, 2, 2] = 1
    return scene.get_im_poses_matrix().detach().double().cpu(), K


def source_lists(sources, V, n_img):
    """Host CSR (ptr, idx) of the source images per view; None = every image for every view."""
    if sources is None:
        sources = [range(n_img)] * V
    if len(sources) != V:
        raise ValueError(f"render: {len(sources)} source lists for {V} views")
    ptr, idx = [0], []
    for s in sources:
        idx.extend(int(i) for i in s)
        ptr.append(len(idx))
    return ptr, idx


def voxel_option(x):
    """(on, voxel) of an argument that is a voxel size, True for the callee's default (then voxel is None), or None / False for off."""
    on = x is not None and x is not False
    return on, x if on and x is not True else None


@dataclass(frozen=True)
class MeshOptions:
    """The five keywords for the TSDF surface mesh (see tsdf.tsdf_mesh), built once per call; `**vars(options)` passes them on."""
    min_component_faces: object = None
    min_component_fraction: object = None
    smooth_iterations: object = None
    smooth_pin_boundary: object = True
    normals: object = False

    filtering = property(lambda self: self.min_component_faces is not None or self.min_component_fraction is not None)
    shaping = property(lambda self: self.smooth_iterations is not None or self.smooth_pin_boundary is not True or bool(self.normals))

    def check(self, who):
        """mesh.check_keep_args and mesh.check_smooth_args on what is given, speaking as `who`."""
        check_keep_args(self.min_component_faces, self.min_component_fraction, who=who)
        if self.smooth_iterations is not None:
            check_smooth_args(self.smooth_iterations, who=who)


class SceneView:
    """A GroupAligner as `who` takes it. Making one checks scene.require_all_depthmaps(who), sets `min_conf_thr` / `thr_for_init_conf`
    on the scene as the demo does and takes `msk`, scene.get_masks() [n, H, W] or None for every pixel (`is_msk=False`), in that order.
    The rest is read when first asked for and then kept, detached: `pts3d` [n, H, W, 3] and `depth` [n, H, W] (contiguous), `focals`
    [n, 1], `conf`, `poses` (cams2world on the device), `cameras` (scene_cameras), `rgb` (scene.imgs as floats on the device, or None)
    and `imgs` (`rgb`, or a ValueError in `who`'s name). `thresholds`: the three keywords, for a callee that takes the scene again.
    `segment`: motion.segment_motion, which is built on this view, so those who may need dynamic() on a scene without masks hand it in."""

    def __init__(self, scene, who, *, min_conf_thr, thr_for_init_conf, is_msk, motion=None, segment=None):
        scene.require_all_depthmaps(who)
        scene.min_conf_thr, scene.thr_for_init_conf = min_conf_thr, thr_for_init_conf
        self.msk = scene.get_masks() if is_msk else None
        self.scene, self.who, self.motion, self.segment = scene, who, motion, segment
        self.thresholds = dict(min_conf_thr=min_conf_thr, thr_for_init_conf=thr_for_init_conf, is_msk=is_msk)
        self.n, self.H, self.W, self.dev = scene.n, scene.H, scene.W, scene.dev

    pts3d = cached_property(lambda self: self.scene.get_pts3d().detach().contiguous())
    depth = cached_property(lambda self: self.scene.get_depthmaps().detach().contiguous())
    focals = cached_property(lambda self: self.scene.get_focals().detach())
    conf = cached_property(lambda self: self.scene.get_conf().detach())
    poses = cached_property(lambda self: self.scene.get_im_poses_matrix().detach())
    cameras = cached_property(lambda self: scene_cameras(self.scene))
    rgb = cached_property(lambda self: None if self.scene.imgs is None else self.scene.imgs.to(self.dev).float().contiguous())

    @property
    def imgs(self):
        if self.rgb is None:
            raise ValueError(f"{self.who}: the scene has no RGB frames; pass imgs= to post_optimization or set scene.imgs [n, H, W, 3] "
                             "in [0, 1]")
        return self.rgb

    def dynamic(self):
        """bool [n, H, W]: scene.dynamic_masks; `segment` makes them with this view's thresholds when the scene has none."""
        dyn = getattr(self.scene, "dynamic_masks", None)
        return self.segment(self.scene, **self.thresholds) if dyn is None else dyn

    def mask(self, motion=None):
        """`msk` restricted to the "static" or "dynamic" pixels of dynamic(); `motion` None means the view's own (None: `msk` itself)."""
        motion = motion or self.motion
        if motion is None:
            return self.msk
        part = self.dynamic() if motion == "dynamic" else ~self.dynamic()
        return part if self.msk is None else self.msk & part


scene_view = SceneView
