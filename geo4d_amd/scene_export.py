"""Scene export: from an aligned ``GroupAligner`` to what a user opens (the end of scripts/evaluation/test_geo4d.py:513-534).

``get_3D_model_from_scene`` is ``dust3r/demo.py:56-86`` on a ``GroupAligner``: optional ``clean_depth`` (``clean_pointcloud``, the
n (n - 1) H W projections of csrc/scene_export.hip, one launch per source image), the confidence masks, and the glb of
``convert_scene_output_to_glb`` (dust3r/utils/viz_demo.py:13-58): the point cloud (``as_pointcloud``) or the mesh of
``pts3d_to_trimesh`` + ``cat_meshes`` (dust3r/viz.py:40-90), plus the camera glyphs. Masking and compaction run on the device; only the
kept points / faces go to the host. ``save_scene`` writes the script's whole results folder.
"""
import os

import torch

from . import _lib, io, ops
from .fusion import check_neighbour_args, fuse_scene
from .mesh import remove_small_components
from .motion import segment_motion
from .render import render_scene, save_render
from .scene_view import MOTION, MeshOptions, scene_view, voxel_option
from .tsdf import tsdf_scene


def check_tol(tol):
    """clean_pointcloud's `assert 0 <= tol < 1`, as an error."""
    if not (0 <= tol < 1):
        raise ValueError(f"clean_pointcloud: tol must satisfy 0 <= tol < 1, got {tol}")


def _stack(x):
    return torch.stack(list(x)) if isinstance(x, (list, tuple)) else x


@torch.no_grad()
def clean_pointcloud(im_confs, K, cams, depthmaps, all_pts3d, tol=0.001, bad_conf=0):
    """base_opt_group.py:630-665 with the same arguments (tensors [n, ...] or lists of per-image tensors, on the HIP device): for every
    ordered pair (i, j) in the reference's loop order, pixels of i that project in front of j's depth and are less confident than j's
    pixel there get min(conf, bad_conf). cams = world-to-camera 4x4, K = 3x3 intrinsics. Returns the cleaned confidences [n, H, W]
    (a new tensor; the inputs are left as they are)."""
    check_tol(tol)
    conf = _stack(im_confs)
    n, H, W = conf.shape
    cams, K = _stack(cams), _stack(K)
    if not (conf.is_cuda and cams.is_cuda and K.is_cuda):
        raise _lib.Geo4DNativeError("clean_pointcloud runs only on a HIP device (there is no CPU fallback)")
    assert len(cams) == len(K) == n, (cams.shape, K.shape, conf.shape)
    mats = torch.cat([cams[:, :3, :].reshape(n, 12), K.reshape(n, 9)], 1).float().contiguous()
    out = conf.float().clone().contiguous()
    ops.scene_clean(out, _stack(all_pts3d).reshape(n, H, W, 3).float().contiguous(), _stack(depthmaps).reshape(n, H, W).float().contiguous(),
                    mats, tol=tol, bad_conf=bad_conf)
    return out


def camera_colors(n):
    """The demo's camera edge colours: viridis(i / n) scaled to 0-255 (demo.py:80-81)."""
    import matplotlib
    cmap = matplotlib.colormaps["viridis"]
    return [tuple(255 * c for c in cmap(i / n)[:3]) for i in range(n)]


def get_3D_model_from_scene(outdir, silent, scene, min_conf_thr=3, as_pointcloud=False, mask_sky=False, clean_depth=False,
                            transparent_cams=False, cam_size=0.05, show_cam=True, save_name=None, thr_for_init_conf=True, is_msk=True,
                            motion=None, fuse_voxel=None, tsdf_voxel=None, tsdf_mesh=None, min_component_faces=None,
                            min_component_fraction=None, smooth_iterations=None, smooth_pin_boundary=True, normals=False,
                            fuse_min_neighbours=0, fuse_neighbour_radius=None):
    """dust3r/demo.py:56-86 on a GroupAligner; returns the path of <outdir>/<save_name or 'scene'>.glb (None when scene is None).

    Sets scene.min_conf_thr / thr_for_init_conf as the demo does; `is_msk=False` keeps every pixel. The point cloud is byte-identical
    to geo4d_amd.io.save_glb on the same points, colours and masks; the mesh is one indexed TRIANGLES primitive with per-vertex colours
    (io.mesh_geometry says why it is not trimesh's per-face layout). `mask_sky=True` raises NotImplementedError: segment_sky needs
    OpenCV, which this engine does not use. `transparent_cams` is accepted and changes nothing: the camera glyphs here are untextured
    wireframes, there is no image on them to make transparent. `motion`: None exports everything, "static" only the points and mesh
    faces that are not dynamic, "dynamic" only the dynamic ones; the masks are scene.dynamic_masks, made by
    geo4d_amd.motion.segment_motion with this call's thresholds and its default rule when the scene has none yet. `fuse_voxel`: None
    (or False) exports every pixel's point; a voxel size, or True for geo4d_amd.fusion.fuse_scene's default, exports the voxel-merged
    cloud of fuse_scene (same masks, thresholds and `motion`; also left in scene.fused) and needs as_pointcloud=True. `tsdf_voxel`:
    None (or False) likewise; a voxel size, or True for geo4d_amd.tsdf.tsdf_scene's default, exports the surface points of tsdf_scene
    (same masks and thresholds, `motion` None or "static"; also left in scene.tsdf); it needs as_pointcloud=True and excludes
    `fuse_voxel`. `tsdf_mesh`: None (or False) likewise; a voxel size, or True for tsdf_scene's default, exports the surface of
    tsdf_scene(mesh=True) as one indexed TRIANGLES primitive (one clean surface in place of the n overlapping per-image sheets; same
    masks and thresholds, `motion` None or "static"; also left in scene.tsdf); it needs as_pointcloud=False and excludes `fuse_voxel`
    and `tsdf_voxel`. `min_component_faces` / `min_component_fraction`: None (both: the mesh as it is); else the detached pieces of
    the mesh that is written, the TSDF surface (then tsdf_scene filters it, and scene.tsdf holds the filtered mesh) or the per-image
    sheets, with fewer faces than that, or than that fraction of the largest piece's, are left out
    (geo4d_amd.mesh.remove_small_components) and the glb holds only the vertices its faces name; it needs a mesh: as_pointcloud=False
    and neither `fuse_voxel` nor `tsdf_voxel`. `smooth_iterations` / `smooth_pin_boundary` / `normals`: for the TSDF surface alone
    (`tsdf_mesh`): tsdf_scene smooths its mesh by that many Taubin iterations (scene.tsdf then holds the smoothed vertices) and, with
    `normals=True`, the primitive carries the area-weighted unit vertex normals as NORMAL, so that a viewer shades it smoothly. Without
    `tsdf_mesh` they raise: points have no faces, and the per-image sheets keep unreferenced vertices, whose normal would be zero.
    `fuse_min_neighbours` / `fuse_neighbour_radius`: fuse_scene's `min_neighbours` / `neighbour_radius` for the fused cloud alone
    (fused points with fewer other fused points within the radius are left out); without `fuse_voxel` they raise."""
    if motion not in MOTION:
        raise ValueError(f"get_3D_model_from_scene: motion must be one of {MOTION}, got {motion!r}")
    check_neighbour_args("get_3D_model_from_scene", fuse_min_neighbours, fuse_neighbour_radius)
    options = MeshOptions(min_component_faces, min_component_fraction, smooth_iterations, smooth_pin_boundary, normals)
    (fuse, fuse_voxel), (tsdf, tsdf_voxel), (surface, tsdf_mesh) = voxel_option(fuse_voxel), voxel_option(tsdf_voxel), voxel_option(tsdf_mesh)
    if (fuse_min_neighbours or fuse_neighbour_radius is not None) and not fuse:
        raise ValueError("get_3D_model_from_scene: fuse_min_neighbours / fuse_neighbour_radius thin out the fused cloud alone: they need "
                         "fuse_voxel")
    if fuse and not as_pointcloud:
        raise ValueError("get_3D_model_from_scene: fuse_voxel merges points and has no faces to give: it needs as_pointcloud=True")
    if tsdf and fuse:
        raise ValueError("get_3D_model_from_scene: fuse_voxel and tsdf_voxel are two different clouds of the same points: give one of them")
    if tsdf and not as_pointcloud:
        raise ValueError("get_3D_model_from_scene: tsdf_voxel gives surface points and has no faces to give: it needs as_pointcloud=True")
    if tsdf and motion == "dynamic":
        raise ValueError("get_3D_model_from_scene: tsdf_voxel with motion='dynamic': the moving part has no TSDF")
    if surface and (fuse or tsdf):
        raise ValueError("get_3D_model_from_scene: tsdf_mesh writes triangles, fuse_voxel and tsdf_voxel write points: give one of them")
    if surface and as_pointcloud:
        raise ValueError("get_3D_model_from_scene: tsdf_mesh writes triangles: it needs as_pointcloud=False (tsdf_voxel gives the points)")
    if surface and motion == "dynamic":
        raise ValueError("get_3D_model_from_scene: tsdf_mesh with motion='dynamic': the moving part has no TSDF")
    if options.filtering and (as_pointcloud or fuse or tsdf):
        raise ValueError("get_3D_model_from_scene: min_component_faces / min_component_fraction remove pieces of a mesh and points have "
                         "no faces to connect them: they need as_pointcloud=False and neither fuse_voxel nor tsdf_voxel")
    if options.shaping and not surface:
        raise ValueError("get_3D_model_from_scene: smooth_iterations / smooth_pin_boundary / normals are for the TSDF surface mesh alone: "
                         "they need tsdf_mesh (points have no faces, and the per-image sheets keep vertices that no face names)")
    options.check("get_3D_model_from_scene")
    if scene is None:
        return None
    if mask_sky:
        raise NotImplementedError("get_3D_model_from_scene(mask_sky=True): segment_sky needs OpenCV (cv2), which is not available")
    if clean_depth:
        scene = scene.clean_pointcloud()
    with torch.no_grad():
        view = scene_view(scene, "get_3D_model_from_scene", min_conf_thr=min_conf_thr, thr_for_init_conf=thr_for_init_conf, is_msk=is_msk,
                          motion=motion, segment=segment_motion)
        imgs, n, H, W = view.imgs, view.n, view.H, view.W
        part = dict(view.thresholds, motion=motion)                 # fuse_scene and tsdf_scene take the scene again, the same way
        cloud = lambda d: [dict(mode=0, positions=d["points"].cpu().numpy(), colors=d["rgba"].cpu().numpy())] if len(d["points"]) else []
        if fuse:
            geometry = cloud(fuse_scene(scene, voxel=fuse_voxel, min_neighbours=fuse_min_neighbours, neighbour_radius=fuse_neighbour_radius,
                                        **part))
        elif tsdf:
            geometry = cloud(tsdf_scene(scene, voxel=tsdf_voxel, **part))
        elif surface:
            surf = tsdf_scene(scene, voxel=tsdf_mesh, mesh=True, **part, **vars(options))
            geometry = [io.mesh_geometry(surf["vertices"].cpu().numpy(), surf["vertex_rgba"].cpu().numpy(), surf["faces"].cpu().numpy(),
                                         surf["vertex_normals"].cpu().numpy() if normals else None)] if len(surf["faces"]) else []
        elif as_pointcloud:
            pts, rgba, count = ops.scene_points(view.pts3d, imgs, view.mask())
            c = int(count.item())
            geometry = [dict(mode=0, positions=pts[:c].cpu().numpy(), colors=rgba[:c].cpu().numpy())] if c else []   # e.g. no mover
        else:
            pts, rgba, _ = ops.scene_points(view.pts3d, imgs, None)     # every vertex, as cat_meshes keeps them
            faces, count = ops.scene_mesh_faces(view.mask(), n, H, W, view.dev)
            c = int(count.item())
            faces = faces[:c]
            if options.filtering and c:
                kept = remove_small_components(pts, faces, min_faces=min_component_faces, min_fraction=min_component_fraction, rgba=rgba)
                pts, rgba, faces, c = kept["vertices"], kept["rgba"], kept["faces"], len(kept["faces"])
            geometry = [io.mesh_geometry(pts.cpu().numpy(), rgba.cpu().numpy(), faces.cpu().numpy())] if c else []
    outfile = os.path.join(outdir, (save_name or "scene") + ".glb")
    if not silent:
        print("(exporting 3D scene to", outfile, ")")
    return io.write_scene_glb(outfile, geometry, view.focals, view.poses, (W, H), cam_size=cam_size, show_cam=show_cam,
                              cam_color=camera_colors(n))


def save_scene(scene, outdir, seq, imgs=None, min_conf_thr=2, render=None, dynamic_masks=False, fuse_static=None, tsdf_static=None,
               tsdf_mesh_static=None, render_kw=None, **glb_kw):
    """test_geo4d.py:513-534: writes <outdir>/<seq>/ with <seq>.glb (called as the script calls it: as_pointcloud=True, is_msk=False,
    cam_size=0.01; `glb_kw` overrides), pred_traj.txt, pred_focal.txt, pred_intrinsics.txt, the depth maps (frame_%04d.npy + colour
    previews), conf_{i}.npy, init_conf_{i}.npy and frame_{i:04d}.png. `imgs` (a clip, see align.rgb_frames) replaces scene.imgs.
    `render`: None, or a mode of geo4d_amd.render.render_scene ("cameras", "playback", "turntable"): also writes <seq>/render/
    (frame_%04d.png, render.gif) with the glb's threshold and masking; `render_kw`: a dict of further arguments for render_scene, for
    example dict(static_mesh=True, shade=0.5) (None: none). `dynamic_masks=True` also writes dynamic_mask_{i}.png
    (scene.dynamic_masks, made by geo4d_amd.motion.segment_motion with the glb's threshold and masking when the scene has none) and
    <seq>_static.glb, the glb without the moving points. `fuse_static`: a voxel size, or True for fuse_scene's default, also writes
    <seq>_static_fused.glb, the static points merged into one cloud (get_3D_model_from_scene(motion="static", fuse_voxel=...), always a
    point cloud); it segments motion first when the scene has no masks, and writes no other file: the dynamic_mask PNGs and
    <seq>_static.glb stay with `dynamic_masks`. `tsdf_static`: a voxel size, or True for tsdf_scene's default, likewise also writes
    <seq>_static_tsdf.glb, the surface points of the static part's TSDF (get_3D_model_from_scene(motion="static", tsdf_voxel=...)), and
    nothing else. `tsdf_mesh_static`: a voxel size, or True for tsdf_scene's default, likewise also writes <seq>_static_tsdf_mesh.glb,
    the static part's TSDF surface as a triangle mesh (get_3D_model_from_scene(motion="static", as_pointcloud=False, tsdf_mesh=...)),
    and nothing else; `min_component_faces` / `min_component_fraction` among `glb_kw` filter that mesh alone (see
    get_3D_model_from_scene): the other files are point clouds unless `glb_kw` says otherwise, and are written as without them;
    `smooth_iterations` / `smooth_pin_boundary` / `normals` among `glb_kw` likewise reach that mesh alone; `fuse_min_neighbours` /
    `fuse_neighbour_radius` among `glb_kw` reach <seq>_static_fused.glb alone and raise without `fuse_static`. Returns the directory."""
    from .align import rgb_frames
    d = os.path.join(outdir, seq)
    os.makedirs(d, exist_ok=True)
    if imgs is not None:
        scene.imgs = rgb_frames(imgs, scene.n, scene.H, scene.W).to(scene.dev)
    kw = dict(silent=True, as_pointcloud=True, mask_sky=False, clean_depth=False, transparent_cams=False, cam_size=0.01, is_msk=False)
    kw.update(glb_kw)
    pieces = {k: kw.pop(k) for k in ("min_component_faces", "min_component_fraction") if k in kw}   # of the meshes only
    if not kw["as_pointcloud"]:
        kw.update(pieces)
    pieces.update({k: kw.pop(k) for k in ("smooth_iterations", "smooth_pin_boundary", "normals") if k in kw})   # of the TSDF mesh only
    near = {k: kw.pop(k) for k in ("fuse_min_neighbours", "fuse_neighbour_radius") if k in kw}   # of the fused static cloud only
    check_neighbour_args("save_scene", near.get("fuse_min_neighbours", 0), near.get("fuse_neighbour_radius"))
    if (near.get("fuse_min_neighbours") or near.get("fuse_neighbour_radius") is not None) and not voxel_option(fuse_static)[0]:
        raise ValueError("save_scene: fuse_min_neighbours / fuse_neighbour_radius thin out the fused static cloud alone: they need fuse_static")
    is_msk, thr_init = kw["is_msk"], kw.get("thr_for_init_conf", True)
    silent = kw.pop("silent")
    get_3D_model_from_scene(d, silent, scene, min_conf_thr=min_conf_thr, save_name=seq, **kw)
    if dynamic_masks:
        if getattr(scene, "dynamic_masks", None) is None:
            segment_motion(scene, min_conf_thr=min_conf_thr, thr_for_init_conf=thr_init, is_msk=is_msk)
        io.save_dynamic_masks(d, scene.dynamic_masks)
        get_3D_model_from_scene(d, silent, scene, min_conf_thr=min_conf_thr, save_name=seq + "_static", **dict(kw, motion="static"))
    for name, arg, voxel, cloud in (("fused", "fuse_voxel", fuse_static, True), ("tsdf", "tsdf_voxel", tsdf_static, True),
                                    ("tsdf_mesh", "tsdf_mesh", tsdf_mesh_static, False)):
        if voxel_option(voxel)[0]:                                  # the static part again, as another cloud or as the TSDF mesh
            get_3D_model_from_scene(d, silent, scene, min_conf_thr=min_conf_thr, save_name=f"{seq}_static_{name}",
                                    **dict(kw, motion="static", as_pointcloud=cloud, **{arg: voxel}, **({} if cloud else pieces),
                                           **(near if name == "fused" else {})))
    with torch.no_grad():
        io.save_tum_poses(os.path.join(d, "pred_traj.txt"), scene.get_im_poses_matrix().detach())
        io.save_focals(os.path.join(d, "pred_focal.txt"), scene.get_focals().detach())
        io.save_intrinsics(os.path.join(d, "pred_intrinsics.txt"), scene.get_intrinsics())
        io.save_depth_maps(d, scene.get_depthmaps())
        io.save_conf_maps(d, scene.get_conf(), "conf")
        io.save_conf_maps(d, scene.get_init_conf(), "init_conf")
        io.save_rgb_imgs(d, scene.imgs.detach().cpu().numpy())
    if render is not None:
        frames = render_scene(scene, render, min_conf_thr=min_conf_thr, is_msk=is_msk, thr_for_init_conf=thr_init, **(render_kw or {}))
        save_render(os.path.join(d, "render"), frames["rgb"])
    return d
