"""The motion rule on the HIP path (geo4d_amd/motion.py + csrc/motion.hip) against its numpy restatement (tests/motion_restatement.py):
exact votes on the synthetic scene (clean, noisy, with an invalid band; radius 8 and 1), image borders and the ends of the voter loop,
determinism, and what is built on the masks: segment_motion on an aligned scene, the export's static / dynamic parts, the renderer's
persist_static and save_scene's PNGs."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import motion_restatement as mr
from scene_cases import tiny_aligner as _aligner, truth_aligner as _synthetic_aligner

pytestmark = pytest.mark.gpu
SCENES = {"clean": dict(), "noisy": dict(noise=0.02), "banded": dict(band=True)}


def _scene_arrays(a):
    """What segment_motion reads from a GroupAligner, as numpy: pts3d, depth, cams2world, K."""
    K = np.zeros((a.n, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = a.get_focals().detach().reshape(a.n).double().cpu().numpy()
    K[:, :2, 2] = a.get_principal_points().detach().double().cpu().numpy()
    K[:, 2, 2] = 1
    return (a.get_pts3d().detach().cpu().numpy(), a.get_depthmaps().detach().cpu().numpy(),
            a.get_im_poses_matrix().detach().double().cpu().numpy(), K)


def _gpu_votes(dev, s, **kw):
    from geo4d_amd import motion
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = motion.motion_votes(t(s["pts3d"]), t(s["depth"]), t(s["valid"]), torch.from_numpy(s["cams2world"]), torch.from_numpy(s["K"]), **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and out.device.type == "cuda"
    return out.cpu().numpy()


def _points(path):
    """Vertices of the POINTS primitives of a glb (0 when it holds none)."""
    data = open(path, "rb").read()
    jlen = struct.unpack("<I", data[12:16])[0]
    doc = json.loads(data[20:20 + jlen])
    return sum(doc["accessors"][p["attributes"]["POSITION"]]["count"] for m in doc["meshes"] for p in m["primitives"] if p["mode"] == 0)


@pytest.fixture(scope="module")
def scenes():
    """The synthetic scenes and the restatement's votes at radius 8 and 1, computed once."""
    out = {}
    for name, kw in SCENES.items():
        s = mr.synthetic_scene(**kw)
        s["views"] = mr.views_of(s["cams2world"], s["K"])
        s["ref"] = {r: mr.votes(s["pts3d"], s["depth"], s["valid"], s["views"], radius=r) for r in (8, 1)}
        out[name] = s
    return out


@pytest.mark.parametrize("radius", [8, 1])
@pytest.mark.parametrize("name", list(SCENES))
def test_votes_match_the_restatement(dev, scenes, name, radius):
    """Exact equality of the uint8 votes. A differing pixel is excusable only when one of its voters projects it within 1e-4 px of a
    rounding boundary or sees zc within 4 ulp of dmin lo / dmax hi, and at most 0.05 % of the valid pixels may be excused."""
    s = scenes[name]
    ref = s["ref"][radius]
    got = _gpu_votes(dev, s, radius=radius)
    assert got.shape == ref.shape == (12, 48, 64, 3)
    where = np.nonzero((got != ref).any(-1))
    ok = mr.excusable(s["pts3d"], s["depth"], s["valid"], s["views"], where, radius=radius)
    valid = int(s["valid"].sum())
    print(f"[motion {name} r={radius}] {valid} valid pixels, {int(ref.astype(np.int64).sum())} votes, {len(ok)} pixels differ / excused "
          f"(0 expected)")
    assert all(ok), (name, radius, [tuple(int(w[k]) for w in where) for k in range(len(ok)) if not ok[k]][:10])
    assert len(ok) <= 5e-4 * valid
    assert (got[~s["valid"]] == 0).all()
    if radius == 8 and name != "banded":
        m = mr.dynamic_mask(got)
        assert mr.iou(m, s["truth"]) >= 0.9


def test_image_borders_and_loop_ends(dev):
    """5 x 7 images, n = 3, a third of the pixels invalid: every 3 x 3 range touches a border, every image is an end of the voter loop."""
    s = mr.synthetic_scene(n=3, H=5, W=7)
    s["valid"] = np.random.default_rng(3).uniform(size=(3, 5, 7)) < 0.67
    s["depth"] = np.where(s["valid"], s["depth"], np.float32(np.nan))
    s["views"] = mr.views_of(s["cams2world"], s["K"])
    for radius in (1, 8, 127):
        ref = mr.votes(s["pts3d"], s["depth"], s["valid"], s["views"], radius=radius)
        assert ref.any() and (ref[~s["valid"]] == 0).all()
        assert np.array_equal(_gpu_votes(dev, s, radius=radius), ref), radius
    one = {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in mr.synthetic_scene().items()}
    lone = _gpu_votes(dev, one)
    assert lone.shape == (1, 48, 64, 3) and not lone.any()                             # a 1-image scene: nobody votes


def test_two_runs_are_equal_and_valid_none_is_all(dev, scenes):
    from geo4d_amd import motion
    s = scenes["noisy"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    args = (t(s["pts3d"]), t(s["depth"]))
    cams = (torch.from_numpy(s["cams2world"]), torch.from_numpy(s["K"]))
    a, b = motion.motion_votes(*args, t(s["valid"]), *cams), motion.motion_votes(*args, t(s["valid"]), *cams)
    assert torch.equal(a, b)
    assert torch.equal(a, motion.motion_votes(*args, None, *cams))                     # the scene's valid is all true
    with pytest.raises(ValueError):
        motion.motion_votes(*args, None, *cams, radius=128)
    with pytest.raises(ValueError):
        motion.motion_votes(*args, None, *cams, tol=1.0)


def test_segment_motion_on_the_aligned_scene(dev, tmp_path):
    from geo4d_amd import motion, scene_export
    a = _aligner(dev)
    assert a.dynamic_masks is None
    thr = float(a.im_conf.median())
    pts3d, depth, c2w, K = _scene_arrays(a)
    for is_msk in (True, False):
        got = motion.segment_motion(a, min_conf_thr=thr, is_msk=is_msk)
        assert got.dtype == torch.bool and tuple(got.shape) == (a.n, a.H, a.W) and got is a.dynamic_masks
        valid = a.get_masks().cpu().numpy() if is_msk else np.ones((a.n, a.H, a.W), dtype=bool)
        want = mr.segment(pts3d, depth, valid, c2w, K)
        assert np.array_equal(got.cpu().numpy(), want), is_msk
        assert not (got.cpu().numpy() & ~valid).any()
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    a.dynamic_masks = None                                                             # the export segments with its own thresholds
    kw = dict(min_conf_thr=thr, as_pointcloud=True)
    plain = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="plain", **kw)
    none = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="none", motion=None, **kw)
    assert a.dynamic_masks is None and open(plain, "rb").read() == open(none, "rb").read()
    static = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="static", motion="static", **kw)
    dyn = a.dynamic_masks
    assert dyn is not None and np.array_equal(dyn.cpu().numpy(), mr.segment(pts3d, depth, a.get_masks().cpu().numpy(), c2w, K))
    moving = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="moving", motion="dynamic", **kw)
    msk = a.get_masks()
    assert _points(plain) == int(msk.sum()) and _points(moving) == int((msk & dyn).sum()) and _points(static) == int((msk & ~dyn).sum())
    assert _points(static) + _points(moving) == _points(plain)
    mesh_kw = dict(min_conf_thr=thr, as_pointcloud=False)                              # the mesh path takes the same masks
    m_plain = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="m_plain", **mesh_kw)
    m_none = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="m_none", motion=None, **mesh_kw)
    assert open(m_plain, "rb").read() == open(m_none, "rb").read()
    m_static = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="m_static", motion="static", **mesh_kw)
    assert os.path.getsize(m_static) <= os.path.getsize(m_plain)
    a.dynamic_masks = torch.zeros_like(dyn)                                            # a scene without movers: the dynamic part is empty
    empty = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="empty", motion="dynamic", **kw)
    assert _points(empty) == 0 and _points(scene_export.get_3D_model_from_scene(str(tmp_path), True, a, motion="static", **kw)) == int(msk.sum())


def test_persist_static_off_is_todays_render(dev):
    from geo4d_amd import render
    a = _aligner(dev)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(2)).to(dev)
    thr = float(a.im_conf.median())
    for mode in ("cameras", "playback"):
        base = render.render_scene(a, mode, min_conf_thr=thr, trail=1, point_size=2)
        off = render.render_scene(a, mode, min_conf_thr=thr, trail=1, point_size=2, persist_static=False)
        for k in ("rgb", "depth", "index"):
            assert torch.equal(base[k], off[k]), (mode, k)
    assert a.dynamic_masks is None


def test_persist_static_playback_on_the_synthetic_scene(dev, scenes):
    """Truth cameras, arbitrary colours: with persist_static every view shows all images' static points and only its own movers."""
    from geo4d_amd import motion, render
    s = scenes["clean"]
    a = _synthetic_aligner(dev, s)
    n, HW = a.n, a.H * a.W
    a.imgs = torch.rand((n, a.H, a.W, 3), generator=torch.Generator().manual_seed(9)).to(dev)
    dyn = motion.segment_motion(a, is_msk=False)
    assert mr.iou(dyn.cpu().numpy(), s["truth"]) >= 0.9                                # the aligner reproduces the scene
    out = render.render_scene(a, "playback", is_msk=False, persist_static=True)
    flat = dyn.reshape(-1)
    for t in (0, 5, n - 1):
        ids = out["index"][t][out["index"][t] >= 0].long()
        assert int(ids.min()) >= 0 and int(ids.max()) < n * HW                         # rows of the original pts3d
        img = ids // HW
        assert not bool((flat[ids] & (img != t)).any())                               # no mover of another frame
        assert bool((flat[ids] & (img == t)).any()) and bool((~flat[ids] & (img != t)).any())
    plain = render.render_scene(a, "playback", is_msk=False)
    assert bool((plain["index"][0] < HW).all())                                       # without it, view 0 knows image 0 alone
    smeared = render.render_scene(a, "cameras", is_msk=False)
    ids = smeared["index"][0][smeared["index"][0] >= 0].long()
    assert bool((flat[ids] & (ids // HW != 0)).any())                                 # without it, other frames' movers do show
    cams = render.render_scene(a, "cameras", is_msk=False, persist_static=True)
    ids = cams["index"][0][cams["index"][0] >= 0].long()
    assert len(ids) and not bool(flat[ids].any())                                     # cameras: the movers of no frame
    named = render.render_scene(a, "cameras", is_msk=False, persist_static=True, sources=[[3]] * n)
    ids = named["index"][0][named["index"][0] >= 0].long()
    assert bool(flat[ids].any()) and bool((ids[flat[ids]] // HW == 3).all())           # ... unless `sources` names some


def test_save_scene_writes_the_masks_and_the_static_glb(dev, tmp_path):
    from PIL import Image
    from geo4d_amd import scene_export
    a = _aligner(dev)
    video = torch.rand((1, 3, a.n, a.H, a.W), generator=torch.Generator().manual_seed(6)) * 2 - 1
    plain = scene_export.save_scene(a, str(tmp_path / "plain"), "seq", imgs=video)
    assert a.dynamic_masks is None
    full = scene_export.save_scene(a, str(tmp_path / "full"), "seq", imgs=video, dynamic_masks=True)
    names = sorted(os.listdir(plain))
    extra = [f"dynamic_mask_{i}.png" for i in range(a.n)] + ["seq_static.glb"]
    assert sorted(os.listdir(full)) == sorted(names + extra)
    for f in names:
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(full, f), "rb").read(), f
    dyn = a.dynamic_masks.cpu().numpy()
    for i in range(a.n):
        png = np.asarray(Image.open(os.path.join(full, f"dynamic_mask_{i}.png")))
        assert png.dtype == np.uint8 and np.array_equal(png, dyn[i].astype(np.uint8) * 255)
    assert _points(os.path.join(full, "seq_static.glb")) == a.n * a.H * a.W - int(dyn.sum())     # save_scene exports with is_msk=False
