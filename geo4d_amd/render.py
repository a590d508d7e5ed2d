"""Frames of an aligned scene, rendered where it was computed: z-buffered point splats on the HIP device (csrc/render.hip).

The reference's user opens the results folder in a browser viewer; a GPU server has neither browser nor display, so this module draws
the scene's points into images instead. Nothing is ported: the projection, the footprint rule and the depth test are stated in
include/geo4d_hip.h and restated in numpy in tests/render_restatement.py. ``render_points`` draws any point set from any cameras,
``render_scene`` a ``GroupAligner`` in three modes (its own cameras, 4-D playback, a turntable), ``save_render`` writes PNG frames and
a GIF. Pixel convention as everywhere in the project: pixel i sits at coordinate i, the principal point defaults to (W/2, H/2).
Images are identical from run to run, bit for bit: the depth test is an integer minimum, which no arrival order changes.
``render_mesh`` draws a triangle mesh, alone or under points, into the same buffer (csrc/render_mesh.hip: exact integer coverage,
restated in tests/render_mesh_restatement.py), and ``render_scene(static_mesh=True)`` the static background as its TSDF surface.
"""
import math
import os

import numpy as np
import torch

from . import _lib, ops
from .motion import segment_motion
from .scene_view import MeshOptions, rgba_of, scene_view, source_lists, views_of, voxel_option
from .tsdf import tsdf_scene

MODES = ("cameras", "playback", "turntable")


@torch.no_grad()
def render_points(points, colors, cams2world, K, size, *, mask=None, radius=None, sources=None, near=1e-3, max_size=9, fill=0,
                  background=(1, 1, 1)):
    """Draw points into V views; returns dict(rgb uint8 [V, H, W, 3], depth fp32 [V, H, W], index int32 [V, H, W]) on the device.

    points [n_img, ..., 3] or [N, 3] fp32 world points on the HIP device (the leading axis of a >2-D tensor is the image axis that
    `sources` indexes; [N, 3] is one image), colors the same shape in [0, 1]; cams2world [V, 4, 4] camera-to-world (OpenCV axes), K
    [V, 3, 3]; size = (H, W) of the frames. mask (points' shape without the 3, bool) drops points; radius (same shape, world units)
    gives every point a square footprint of ceil(2 radius fx / z) pixels, at most max_size, instead of one pixel; sources = per view the
    list of images drawn into it (None: all). Points not beyond `near` in front of the camera are dropped. `fill` hole-filling passes
    let an empty pixel take the nearest of its 3 x 3 neighbours. Per pixel the nearest point wins, at equal depth the lower index;
    `index` is that point's row in points.reshape(-1, 3), -1 where nothing landed (rgb = background, depth = 0)."""
    for t, what in ((points, "points"), (colors, "colors")):
        if not t.is_cuda:
            raise _lib.Geo4DNativeError(f"render_points: `{what}` lives on {t.device}; rendering runs only on a HIP device (there is no "
                                        "CPU fallback)")
    if points.shape[-1] != 3 or colors.shape != points.shape:
        raise ValueError(f"render_points: points and colors must both be [..., 3], got {tuple(points.shape)} and {tuple(colors.shape)}")
    H, W = int(size[0]), int(size[1])
    n_img = points.shape[0] if points.dim() > 2 else 1
    pts = points.reshape(-1, 3).float().contiguous()
    col = colors.reshape(-1, 3).float().contiguous()
    N = pts.shape[0]
    views = views_of(cams2world, K)
    V = len(views)
    ptr, idx = source_lists(sources, V, n_img)
    flat = lambda t, dt: None if t is None else t.to(pts.device).reshape(-1).to(dt).contiguous()
    mask, radius = flat(mask, torch.bool), flat(radius, torch.float32)
    ws = ops.render_workspace(V, H, W, len(idx), pts.device)
    ops.render_splat(pts, views.to(pts.device), ptr, idx, (H, W), ws, mask=mask, radius=radius, pts_per_image=N // n_img, near=near,
                     max_size=max_size)
    if fill:
        ops.render_fill(ws, V, (H, W), fill)
    rgb, depth, index = ops.render_resolve(ws, col, V, (H, W), background)
    return dict(rgb=rgb, depth=depth, index=index)


@torch.no_grad()
def render_mesh(vertices, faces, cams2world, K, size, *, colors=None, mesh_color=(0.7, 0.7, 0.7), shade=0.0, cull_back=False,
                face_mask=None, points=None, point_colors=None, mask=None, radius=None, sources=None, max_size=9, fill=0, near=1e-3,
                background=(1, 1, 1)):
    """Draw a triangle mesh, alone or under points, into V views; returns dict(rgb, depth, index as render_points gives them, face int32
    [V, H, W]) on the device.

    vertices [Nv, 3] fp32 world coordinates and faces [T, 3] integer on the HIP device; colors uint8 rgba [Nv, 4] (as tsdf_mesh returns
    them, alpha ignored) or float [Nv, 3] in [0, 1], interpolated perspective-correctly, None: the uniform `mesh_color`. `shade` in
    [0, 1] mixes in flat headlight shading (colour * ((1 - shade) + shade |n_z| / |n|), n the face normal in camera space).
    `cull_back=True` drops the faces seen from behind (a front face is counter-clockwise as seen); face_mask [T] bool drops faces.
    Every view draws the whole mesh. A triangle with a vertex not beyond `near` is dropped whole (no clipping), as is one that
    projects more than 65536 pixels off; H and W may be at most 16384. Coverage is exact: a pixel belongs to a triangle iff its centre,
    on a 1/256-pixel grid, is inside or on an edge; there is no anti-aliasing. points / point_colors / mask / radius / sources /
    max_size / fill: points drawn into the same frames exactly as render_points draws them (hole filling acts on the points only);
    per pixel the nearest of everything wins, at equal depth a point beats a triangle and a lower face a higher one. `index` is the
    winning point's row or -1, `face` the winning triangle's row or -1. T = 0 or Nv = 0 gives what the points alone give."""
    who = "render_mesh"
    for t, what in ((vertices, "vertices"), (faces, "faces"), (points, "points"), (point_colors, "point_colors"), (face_mask, "face_mask")):
        if t is not None and not t.is_cuda:
            raise _lib.Geo4DNativeError(f"{who}: `{what}` lives on {t.device}; rendering runs only on a HIP device (there is no CPU "
                                        "fallback)")
    if vertices.dim() != 2 or vertices.shape[-1] != 3 or faces.dim() != 2 or faces.shape[-1] != 3 or faces.is_floating_point():
        raise ValueError(f"{who}: need vertices [Nv, 3] and integer faces [T, 3], got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    if (points is None) != (point_colors is None):
        raise ValueError(f"{who}: points and point_colors go together")
    if not 0.0 <= float(shade) <= 1.0:
        raise ValueError(f"{who}: shade must lie in [0, 1], got {shade}")
    dev = vertices.device
    H, W = int(size[0]), int(size[1])
    if H > 16384 or W > 16384:
        raise ValueError(f"{who}: frames may be at most 16384 x 16384, got {(H, W)}")
    vert = vertices.detach().float().contiguous()
    tri = faces.to(torch.int32).contiguous()
    Nv, T = vert.shape[0], tri.shape[0]
    vcol = None
    if colors is not None:
        vcol = rgba_of(colors, (Nv,), dev, who, "colors", "rendering", "[Nv, {}] = ") if colors.dtype == torch.uint8 else None
        if vcol is None:
            if not colors.is_cuda:
                raise _lib.Geo4DNativeError(f"{who}: `colors` lives on {colors.device}; rendering runs only on a HIP device")
            if tuple(colors.shape) != (Nv, 3):
                raise ValueError(f"{who}: float colours must be [Nv, 3] = {(Nv, 3)}, got {tuple(colors.shape)}")
            vcol = colors.detach().float().contiguous()
    if face_mask is not None and tuple(face_mask.shape) != (T,):
        raise ValueError(f"{who}: face_mask must be [T] = {(T,)}, got {tuple(face_mask.shape)}")
    views = views_of(cams2world, K)
    V = len(views)
    dviews = views.to(dev)
    N, col = 0, None
    if points is not None:
        if points.shape[-1] != 3 or point_colors.shape != points.shape:
            raise ValueError(f"{who}: points and point_colors must both be [..., 3], got {tuple(points.shape)} and "
                             f"{tuple(point_colors.shape)}")
        n_img = points.shape[0] if points.dim() > 2 else 1
        pts = points.reshape(-1, 3).float().contiguous()
        col = point_colors.reshape(-1, 3).float().contiguous()
        N = pts.shape[0]
    if N:
        ptr, idx = source_lists(sources, V, n_img)
        flat = lambda t, dt: None if t is None else t.to(dev).reshape(-1).to(dt).contiguous()
        ws = ops.render_workspace(V, H, W, len(idx), dev)
        ops.render_splat(pts, dviews, ptr, idx, (H, W), ws, mask=flat(mask, torch.bool), radius=flat(radius, torch.float32),
                         pts_per_image=N // n_img, near=near, max_size=max_size)
        if fill:
            ops.render_fill(ws, V, (H, W), fill)                 # before the raster: a copied triangle key would have no barycentrics
    else:
        ws, col = ops.render_workspace(V, H, W, 0, dev), None
    ops.render_raster(vert, tri, dviews, (H, W), ws, face_mask=face_mask, near=near, cull_back=cull_back, id_base=N, clear=not N)
    rgb, depth, index, face = ops.render_resolve_mesh(ws, col, vert, tri, dviews, (H, W), vertex_colors=vcol, mesh_color=mesh_color,
                                                      shade=shade, near=near, background=background)
    return dict(rgb=rgb, depth=depth, index=index, face=face)


def orbit_cameras(center, radius, n, elevation=0.0, up=(0.0, -1.0, 0.0)):
    """[n, 4, 4] fp64 camera-to-world poses on a circle of `radius` round `center`, raised by `elevation` radians above the plane
    normal to `up`, each looking at `center`. OpenCV convention: x right, y down, z forward, so the image's top points along `up`
    (the default is the -y of a world laid out like the first camera)."""
    c = np.asarray(center, dtype=np.float64).reshape(3)
    up = np.asarray(up, dtype=np.float64).reshape(3)
    up = up / np.linalg.norm(up)
    a = np.eye(3)[np.argmin(np.abs(up))]                      # any direction that is not parallel to `up`
    e0 = np.cross(up, a)
    e0 /= np.linalg.norm(e0)
    e1 = np.cross(up, e0)
    poses = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        th = 2 * math.pi * k / n
        pos = c + radius * (math.cos(elevation) * (math.cos(th) * e0 + math.sin(th) * e1) + math.sin(elevation) * up)
        z = c - pos
        z /= np.linalg.norm(z)
        x = np.cross(z, up)                                     # right = forward x up (y down = -up once orthogonalised)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        poses[k, :3, 0], poses[k, :3, 1], poses[k, :3, 2], poses[k, :3, 3] = x, y, z, pos
    return poses


@torch.no_grad()
def render_scene(scene, mode="cameras", *, size=None, min_conf_thr=3, is_msk=True, thr_for_init_conf=True, point_size=0, trail=0,
                 path=None, sources=None, n_views=24, elevation=0.3, orbit_radius=None, near=1e-3, max_size=9, fill=0,
                 background=(1, 1, 1), persist_static=False, static_mesh=None, shade=0.0, cull_back=False, min_component_faces=None,
                 min_component_fraction=None, smooth_iterations=None, smooth_pin_boundary=True):
    """Frames of a GroupAligner: dict(rgb, depth, index) as render_points returns them, one view per frame.

    Points, colours and masks are those get_3D_model_from_scene exports (get_pts3d, scene.imgs, get_masks with `min_conf_thr` /
    `thr_for_init_conf`; `is_msk=False` keeps every pixel). mode "cameras": view i is image i's camera and draws every image;
    "playback": view t is image t's camera - or pose t of `path` [n, 4, 4] - and draws images t - trail .. t, the clip as it unfolds;
    "turntable": `n_views` cameras of orbit_cameras round the masked points' median, `orbit_radius` away (None: twice the median
    distance of the points from it), `elevation` radians up, drawing every image. `sources` overrides the mode's lists. `point_size`
    > 0 draws point p of image i with the world radius 0.5 point_size depth / focal, i.e. point_size pixels wide in its own camera and
    accordingly larger from nearer by; 0 draws single pixels. `size` (H, W) other than the scene's rescales the intrinsics.
    `persist_static=True`: every view draws the static points of ALL images and the dynamic points (scene.dynamic_masks, made by
    geo4d_amd.motion.segment_motion with this call's thresholds when the scene has none) only of the images in its source list, so
    playback shows the current frame's movers over a background that is complete from the first frame and cameras / turntable
    show the movers of no frame unless `sources` names some; `index` still counts rows of the scene's pts3d.reshape(-1, 3).
    `static_mesh=True`, or a voxel size: the static background is drawn as the TSDF surface mesh instead (render_mesh; from
    geo4d_amd.tsdf.tsdf_scene(scene, voxel, motion="static", mesh=True) with this call's thresholds, True meaning its default voxel;
    scene.tsdf is reused when it already holds `vertices` - for True whatever its voxel, else for that voxel), with `shade` and
    `cull_back` as render_mesh takes them. No static point is drawn, the moving points are chosen as persist_static chooses them, and
    the dict also holds `face`, the winning triangle's row in scene.tsdf["faces"] or -1. Not together with persist_static.
    `min_component_faces` / `min_component_fraction` go to tsdf_scene when this call builds the mesh (its small detached pieces are then
    not drawn, see geo4d_amd.tsdf.tsdf_mesh); a mesh reused from scene.tsdf is drawn as found, filtered or not. They need static_mesh.
    `smooth_iterations` / `smooth_pin_boundary` go to tsdf_scene likewise (Taubin smoothing of the mesh's vertices; scene.tsdf then holds
    the smoothed mesh) and need static_mesh; the shading stays flat, per triangle."""
    if mode not in MODES:
        raise ValueError(f"render_scene: mode must be one of {MODES}, got {mode!r}")
    options = MeshOptions(min_component_faces, min_component_fraction, smooth_iterations, smooth_pin_boundary)
    as_mesh, voxel = voxel_option(static_mesh)
    if as_mesh and persist_static:
        raise ValueError("render_scene: static_mesh draws the static part as a mesh and persist_static as points; choose one")
    if options.filtering and not as_mesh:
        raise ValueError("render_scene: min_component_faces / min_component_fraction filter the static mesh; pass static_mesh")
    if options.shaping and not as_mesh:
        raise ValueError("render_scene: smooth_iterations / smooth_pin_boundary smooth the static mesh; pass static_mesh")
    view = scene_view(scene, "render_scene", min_conf_thr=min_conf_thr, thr_for_init_conf=thr_for_init_conf, is_msk=is_msk,
                      segment=segment_motion)
    n, H, W, imgs, pts3d, msk, (c2w, K) = view.n, view.H, view.W, view.imgs, view.pts3d, view.msk, view.cameras
    radius = 0.5 * float(point_size) * view.depth / view.focals.reshape(n, 1, 1) if point_size else None
    everything = list(range(n))
    if mode == "cameras":
        poses, Kv, src = c2w, K, [everything] * n
    elif mode == "playback":
        poses = c2w if path is None else torch.as_tensor(path).double().reshape(-1, 4, 4)
        if len(poses) != n:
            raise ValueError(f"render_scene: playback needs one pose per image ({n}), got {len(poses)}")
        Kv, src = K, [list(range(max(0, t - int(trail)), t + 1)) for t in range(n)]
    else:
        sel = pts3d[msk] if msk is not None else pts3d.reshape(-1, 3)
        sel = sel[torch.isfinite(sel).all(-1)]
        if len(sel) == 0:
            raise ValueError("render_scene: no valid point to orbit round (lower min_conf_thr or pass is_msk=False)")
        center = sel.median(0).values
        if orbit_radius is None:
            orbit_radius = 2 * float((sel - center).norm(dim=-1).median())
        up = -c2w[0, :3, 1].numpy()                              # the first camera's "up"
        poses = torch.from_numpy(orbit_cameras(center.double().cpu().numpy(), orbit_radius, n_views, elevation, up))
        Kv, src = K[:1].expand(n_views, 3, 3).clone(), [everything] * n_views
    if sources is not None:
        src = sources
    oh, ow = (H, W) if size is None else (int(size[0]), int(size[1]))
    if (oh, ow) != (H, W):
        Kv = Kv.clone()
        Kv[:, 0] *= ow / W
        Kv[:, 1] *= oh / H
    if not (as_mesh or persist_static):
        return render_points(pts3d, imgs, poses, Kv, (oh, ow), mask=msk, radius=radius, sources=src, near=near, max_size=max_size,
                             fill=fill, background=background)
    movers = src if sources is not None or mode == "playback" else [[]] * len(src)  # "every image" would smear the movers again
    if as_mesh:
        # the static part as its TSDF surface, the moving points of each view's source images over it
        voxel = voxel if voxel is None else float(np.float32(voxel))               # as scene.tsdf["voxel"] holds it
        tsdf = getattr(scene, "tsdf", None)
        if tsdf is None or "vertices" not in tsdf or (voxel is not None and tsdf["voxel"] != voxel):
            tsdf = tsdf_scene(scene, voxel, motion="static", mesh=True, near=near, **view.thresholds, **vars(options))
        return render_mesh(tsdf["vertices"], tsdf["faces"], poses, Kv, (oh, ow), colors=tsdf.get("vertex_rgba", tsdf.get("rgba")),
                           shade=shade, cull_back=cull_back, points=pts3d, point_colors=imgs, mask=view.mask("dynamic"), radius=radius,
                           sources=movers, max_size=max_size, fill=fill, near=near, background=background)
    # the images twice, n static-masked copies then n dynamic-masked ones: every view draws all of the former and its own sources of the latter
    twice = lambda t: None if t is None else torch.cat([t, t])
    out = render_points(twice(pts3d), twice(imgs), poses, Kv, (oh, ow), mask=torch.cat([view.mask("static"), view.mask("dynamic")]),
                        radius=twice(radius), sources=[everything + [n + int(i) for i in s] for s in movers], near=near, max_size=max_size,
                        fill=fill, background=background)
    idx = out["index"]
    out["index"] = torch.where(idx >= n * H * W, idx - n * H * W, idx)            # rows of the original pts3d.reshape(-1, 3)
    return out


def save_render(path, rgb, fps=10):
    """frame_%04d.png per view of rgb uint8 [V, H, W, 3] (tensor or array) and render.gif at `fps`, in directory `path`."""
    from PIL import Image
    frames = rgb.detach().cpu().numpy() if torch.is_tensor(rgb) else np.asarray(rgb)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[-1] != 3:
        raise ValueError(f"save_render: rgb must be uint8 [V, H, W, 3], got {frames.dtype} {frames.shape}")
    os.makedirs(path, exist_ok=True)
    images = []
    for i, f in enumerate(frames):
        p = os.path.join(path, f"frame_{i:04d}.png")
        Image.fromarray(np.ascontiguousarray(f)).save(p)
        images.append(Image.open(p))
    if images:
        images[0].save(os.path.join(path, "render.gif"), save_all=True, append_images=images[1:], duration=max(1, round(1000 / fps)), loop=0)
    return path
