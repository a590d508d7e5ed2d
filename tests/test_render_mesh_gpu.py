"""The mesh renderer on the HIP path (geo4d_amd/render.py render_mesh + csrc/render_mesh.hip) against its numpy restatement
(tests/render_mesh_restatement.py), bit for bit on rgb, depth, index and face: the hand-made cases, a random mesh alone and over
points, the in-thread / list / overflow paths of the raster, determinism, the TSDF mesh in its own cameras, render_scene(static_mesh=)
and save_scene(render_kw=)."""
import os

import numpy as np
import pytest
import torch

import motion_restatement as mr
import render_mesh_restatement as rm
import render_restatement as rr
import tsdf_restatement as tr
from scene_cases import truth_aligner as _synthetic_aligner
from test_render_cpu import random_case
from test_render_mesh_cpu import check_hand_cases

pytestmark = pytest.mark.gpu
KEYS = ("rgb", "depth", "index", "face")
F = np.float32


def _t(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _gpu(dev, vertices, faces, cams2world, K, size, **kw):
    """render_mesh on numpy inputs, numpy outputs."""
    from geo4d_amd import render
    for k in ("colors", "face_mask", "points", "point_colors", "mask", "radius"):
        if k in kw:
            kw[k] = _t(dev, kw[k])
    out = render.render_mesh(_t(dev, vertices), _t(dev, faces), torch.from_numpy(np.asarray(cams2world)), torch.from_numpy(np.asarray(K)),
                             size, **kw)
    torch.cuda.synchronize()
    assert out["rgb"].dtype == torch.uint8 and out["depth"].dtype == torch.float32 and out["index"].dtype == out["face"].dtype == torch.int32
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, ref, tag=""):
    for k in KEYS:
        bad = int((got[k] != ref[k]).sum())
        assert np.array_equal(got[k], ref[k]), (tag, k, bad)


def test_hand_made_cases_on_the_device(dev):
    check_hand_cases(lambda *a, **kw: _gpu(dev, *a, **kw))


# ---- the random case -------------------------------------------------------------------------------------------------------------------------
def random_mesh(seed=5, T=400):
    """T triangles round random_case()'s three cameras, depths from a continuous distribution: most a few pixels wide, some partly off
    frame or behind a camera, NaN vertices, sub-pixel ones, and face 7 fills the frame. Colours uint8 rgba and float."""
    g = np.random.default_rng(seed)
    centre = np.stack([g.uniform(-3.0, 3.0, T), g.uniform(-2.5, 2.5, T), g.uniform(-1.0, 6.0, T)], 1)
    v = centre[:, None, :] + g.normal(0, 0.35, (T, 3, 3))
    tiny = np.arange(T) % 10 == 3
    v[tiny] = centre[tiny, None, :] + g.normal(0, 0.004, (int(tiny.sum()), 3, 3))
    v[7] = [[-12 + g.uniform(), -8, 6.0], [12, -8 + g.uniform(), 6.2], [0, 16, 5.8 + g.uniform(0, 0.1)]]
    v = v.astype(F)
    v[g.choice(T, 12, replace=False), g.integers(0, 3, 12)] = np.nan
    v[11, 1, 2] = np.inf
    faces = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    faces[21] = [3, 4, 3 * T]                                                       # out of bounds
    faces[22] = [-1, 4, 5]
    return dict(vertices=v.reshape(-1, 3), faces=faces, rgba=g.integers(0, 256, (3 * T, 4), dtype=np.uint8),
                rgbf=g.uniform(-0.05, 1.05, (3 * T, 3)).astype(F), face_mask=g.uniform(size=T) < 0.95)


@pytest.fixture(scope="module")
def case():
    c = random_case()
    c["mesh"] = random_mesh()
    c["mesh"]["face_mask"][7] = True
    return c


def _points_kw(c, how):
    if how == "alone":
        return {}
    kw = dict(points=c["points"], point_colors=c["colors"], mask=c["mask"], sources=c["sources"])
    return dict(kw, radius=c["radius"], max_size=5) if how == "adaptive" else kw


COMBOS = [("alone", 0, "u8", 0.0, False), ("alone", 0, "float", 0.6, True), ("alone", 0, None, 0.6, False), ("s1", 0, "u8", 0.6, False),
          ("s1", 2, "float", 0.0, True), ("adaptive", 2, "u8", 0.6, True), ("adaptive", 0, None, 0.0, False), ("s1", 2, None, 0.6, False),
          ("adaptive", 2, "float", 0.6, False)]


@pytest.mark.parametrize("how,fill,colours,shade,cull", COMBOS)
def test_random_case_matches_the_restatement(dev, case, how, fill, colours, shade, cull):
    m = case["mesh"]
    kw = dict(_points_kw(case, how), fill=fill, shade=shade, cull_back=cull, face_mask=m["face_mask"], background=(0.2, 0.4, 1.0),
              colors={"u8": m["rgba"], "float": m["rgbf"], None: None}[colours], mesh_color=(0.9, 0.5, 0.1))
    ref = rm.render(m["vertices"], m["faces"], case["cams2world"], case["K"], case["size"], **kw)
    got = _gpu(dev, m["vertices"], m["faces"], case["cams2world"], case["K"], case["size"], **kw)
    faces_seen = len(np.unique(ref["face"][ref["face"] >= 0]))
    print(f"[render_mesh {how} fill {fill}] {int((ref['face'] >= 0).sum())} triangle pixels of {faces_seen} faces, "
          f"{int((ref['index'] >= 0).sum())} point pixels; differing: " + ", ".join(f"{k} {int((got[k] != ref[k]).sum())}" for k in KEYS))
    assert faces_seen > (20 if fill or cull else 100) and (how == "alone" or (ref["index"] >= 0).sum() > 500)
    if how == "alone" and not cull:
        assert (ref["face"][1] >= 0).all() and (ref["face"][1] == 7).sum() > 200        # face 7 fills the frame behind the others
    _same(got, ref, how)


def _views(dev, c):
    from geo4d_amd.scene_view import views_of
    return views_of(c["cams2world"], c["K"]).to(dev)


def _raster(dev, case, **kw):
    """ops.render_raster + ops.render_resolve_mesh on the random mesh alone; (keys, rgb, depth, index, face)."""
    from geo4d_amd import ops
    m, (H, W) = case["mesh"], case["size"]
    views = _views(dev, case)
    v, f = _t(dev, m["vertices"]), _t(dev, m["faces"])
    ws = ops.render_workspace(len(views), H, W, 0, dev)
    ops.render_raster(v, f, views, (H, W), ws, **kw)
    out = ops.render_resolve_mesh(ws, None, v, f, views, (H, W), vertex_colors=_t(dev, m["rgba"]), shade=0.6)
    return (ws[:len(views) * H * W].clone(),) + tuple(out)


def test_in_thread_list_and_overflow_paths_agree(dev, case):
    """Every triangle drawn by its own thread, every triangle through the list, and a list of one entry that overflows at once."""
    m = case["mesh"]
    runs = [_raster(dev, case, large_area=(1 << 31) - 1), _raster(dev, case, large_area=0, capacity=4096),
            _raster(dev, case, large_area=0, capacity=1), _raster(dev, case, large_area=0, capacity=0), _raster(dev, case)]
    torch.cuda.synchronize()
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    ref = rm.render(m["vertices"], m["faces"], case["cams2world"], case["K"], case["size"], colors=m["rgba"], shade=0.6)
    assert np.array_equal(runs[0][0].cpu().numpy().view(np.uint64).reshape(ref["keys"].shape), ref["keys"])
    _same(dict(zip(KEYS, [t.cpu().numpy() for t in runs[0][1:]])), ref)


def test_deterministic_order_free_and_view_by_view(dev, case):
    m = case["mesh"]
    args = (case["cams2world"], case["K"], case["size"])
    kw = dict(colors=m["rgbf"], shade=0.3, **_points_kw(case, "adaptive"))
    a, b = _gpu(dev, m["vertices"], m["faces"], *args, **kw), _gpu(dev, m["vertices"], m["faces"], *args, **kw)
    _same(a, b)
    perm = np.random.default_rng(1).permutation(len(m["faces"]))                    # new face t is old face perm[t]
    p = _gpu(dev, m["vertices"], m["faces"][perm], *args, **kw)
    assert np.array_equal(p["rgb"], a["rgb"]) and np.array_equal(p["depth"], a["depth"]) and np.array_equal(p["index"], a["index"])
    assert np.array_equal(np.where(p["face"] >= 0, perm[p["face"]], -1), a["face"]) and (a["face"] >= 0).sum() > 1000
    for v in range(3):
        single = _gpu(dev, m["vertices"], m["faces"], case["cams2world"][v:v + 1], case["K"][v:v + 1], case["size"],
                      **dict(kw, sources=[case["sources"][v]]))
        for k in KEYS:
            assert np.array_equal(single[k][0], a[k][v]), (k, v)


def test_raster_leaves_nearer_points_alone_and_render_points_is_unchanged(dev, case):
    from geo4d_amd import ops, render, scene_view
    m, (H, W) = case["mesh"], case["size"]
    views = _views(dev, case)
    pts, col = _t(dev, case["points"]), _t(dev, case["colors"])
    c2w, K = torch.from_numpy(case["cams2world"]), torch.from_numpy(case["K"])
    kw = dict(mask=_t(dev, case["mask"]), sources=case["sources"], fill=1)
    before = render.render_points(pts, col, c2w, K, (H, W), **kw)
    N, n = pts.reshape(-1, 3).shape[0], len(views) * H * W
    ptr, idx = scene_view.source_lists(case["sources"], len(views), 3)
    ws = ops.render_workspace(len(views), H, W, len(idx), dev)
    ops.render_splat(pts.reshape(-1, 3).contiguous(), views, ptr, idx, (H, W), ws, mask=kw["mask"].reshape(-1), pts_per_image=N // 3)
    k0 = ws[:n].clone()
    ops.render_raster(_t(dev, m["vertices"]), _t(dev, m["faces"]), views, (H, W), ws, id_base=N, clear=False)
    k1 = ws[:n].clone()
    point_wins = (k1 & 0xFFFFFFFF) < N                                              # int64 views of the keys: the low word is the id
    assert torch.equal(k1[point_wins], k0[point_wins]) and int(point_wins.sum()) > 500
    changed = k1 != k0
    assert int(changed.sum()) > 1000 and bool(((k1[changed] & 0xFFFFFFFF) >= N).all())
    lt = lambda a, b: torch.where((a < 0) == (b < 0), a < b, b < 0)                 # unsigned order of int64 views
    assert bool(lt(k1[changed], k0[changed]).all())
    mesh = render.render_mesh(_t(dev, m["vertices"]), _t(dev, m["faces"]), c2w, K, (H, W), points=pts, point_colors=col, **kw)
    none = render.render_mesh(_t(dev, m["vertices"]), _t(dev, m["faces"])[:0], c2w, K, (H, W), points=pts, point_colors=col, **kw)
    after = render.render_points(pts, col, c2w, K, (H, W), **kw)
    for k in ("rgb", "depth", "index"):
        assert torch.equal(before[k], after[k]) and torch.equal(before[k], none[k]), k
    assert bool((none["face"] == -1).all()) and bool((mesh["face"] >= 0).any())
    seen = mesh["index"] >= 0
    assert torch.equal(mesh["index"][seen], before["index"][seen]) and torch.equal(mesh["depth"][seen], before["depth"][seen])
    bare = render.render_mesh(_t(dev, m["vertices"])[:0], _t(dev, m["faces"]), c2w, K, (H, W))
    assert bool((bare["face"] == -1).all()) and bool((bare["index"] == -1).all()) and bool((bare["rgb"] == 255).all())


@pytest.mark.parametrize("T", [1, 255, 256, 257])
def test_face_counts_round_a_block(dev, case, T):
    m = case["mesh"]
    f = m["faces"][7:7 + T]                                                         # the frame-filling face first
    ref = rm.render(m["vertices"], f, case["cams2world"], case["K"], case["size"], colors=m["rgba"])
    _same(_gpu(dev, m["vertices"], f, case["cams2world"], case["K"], case["size"], colors=m["rgba"]), ref, T)
    assert (ref["face"] == 0).sum() > 1000 and (T == 1 or ref["face"].max() > T - 40)


# ---- the TSDF mesh ---------------------------------------------------------------------------------------------------------------------------
def test_tsdf_mesh_in_the_scenes_own_cameras(dev):
    from geo4d_amd import tsdf
    s = tr.static_scene(0.0)
    mesh = tsdf.tsdf_mesh(_t(dev, s["pts3d"]), _t(dev, s["depth"]), _t(dev, s["static"]), s["cams2world"], s["K"], _t(dev, s["rgba"]),
                          voxel=s["voxel"])
    v, f, rgba = mesh["vertices"].cpu().numpy(), mesh["faces"].cpu().numpy(), mesh["rgba"].cpu().numpy()
    sel = [0, 4, 8, 11]
    c2w, K, size = s["cams2world"][sel], s["K"][sel], (s["H"], s["W"])
    assert len(f) > 1800
    ref = rm.render(v, f, c2w, K, size, colors=rgba, shade=0.5)
    got = _gpu(dev, v, f, c2w, K, size, colors=rgba, shade=0.5)
    _same(got, ref)
    culled = _gpu(dev, v, f, c2w, K, size, colors=rgba, shade=0.5, cull_back=True)
    bits = lambda a: a.view(np.int32).astype(np.int64)
    for vi, view in enumerate(rr.views_of(c2w, K)):
        st = rm.setup(v, f, view, size)
        hit = got["face"][vi] >= 0
        t = got["face"][vi][hit]
        z = st["cam"][t][:, :, 2]
        d = got["depth"][vi][hit]
        assert hit.sum() > 1500
        assert (bits(d) >= bits(z.min(1)) - 1).all() and (bits(d) <= bits(z.max(1)) + 1).all()
        front = np.zeros(hit.shape, dtype=bool)
        front[hit] = st["neg"][t]
        assert front.sum() > 1500
        for k in KEYS:
            assert np.array_equal(culled[k][vi][front], got[k][vi][front]), k


# ---- the scene level -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aligner(dev):
    s = mr.synthetic_scene(noise=0.0)
    a = _synthetic_aligner(dev, s)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(9)).to(dev)
    return a, s


def test_render_scene_draws_the_movers_over_the_static_mesh(dev, aligner):
    from geo4d_amd import render
    a, s = aligner
    n, HW = a.n, a.H * a.W
    play = render.render_scene(a, "playback", is_msk=False, static_mesh=True, shade=0.4)
    assert sorted(play) == ["depth", "face", "index", "rgb"] and a.tsdf is not None and "vertices" in a.tsdf
    dyn = a.dynamic_masks.reshape(-1)
    T = len(a.tsdf["faces"])
    assert T > 1000 and int(play["face"].max()) < T
    assert bool(((play["face"] >= 0) != (play["index"] >= 0))[(play["face"] >= 0) | (play["index"] >= 0)].all())
    for t in range(n):
        ids = play["index"][t][play["index"][t] >= 0].long()
        assert len(ids) and bool(dyn[ids].all()) and bool((ids // HW == t).all())     # view t: the movers of image t alone
        assert int((play["face"][t] >= 0).sum()) > HW // 4
    cams = render.render_scene(a, "cameras", is_msk=False, static_mesh=True, shade=0.4)
    assert bool((cams["index"] == -1).all()) and torch.equal(cams["face"] >= 0, cams["depth"] > 0)
    # same poses in both modes: a playback pixel differs from the cameras' only where a mover covers it
    differs = (play["rgb"] != cams["rgb"]).any(-1) | (play["depth"] != cams["depth"]) | (play["face"] != cams["face"])
    assert bool(differs.any()) and bool((play["index"] >= 0)[differs].all())
    again = render.render_scene(a, "playback", is_msk=False, static_mesh=a.tsdf["voxel"], shade=0.4)        # reuses scene.tsdf
    for k in KEYS:
        assert torch.equal(again[k], play[k]), k
    named = render.render_scene(a, "cameras", is_msk=False, static_mesh=True, sources=[[3]] * n)
    ids = named["index"][0][named["index"][0] >= 0].long()
    assert len(ids) and bool(dyn[ids].all()) and bool((ids // HW == 3).all())
    with pytest.raises(ValueError, match="static_mesh"):
        render.render_scene(a, "playback", static_mesh=True, persist_static=True)
    first, coarse = a.tsdf, 1.3 * a.tsdf["voxel"]                                   # another voxel: a new mesh, then that one reused
    wide = render.render_scene(a, "cameras", is_msk=False, static_mesh=coarse)
    assert a.tsdf is not first and a.tsdf["voxel"] == float(np.float32(coarse)) and len(a.tsdf["faces"]) < T
    made = a.tsdf
    assert torch.equal(render.render_scene(a, "cameras", is_msk=False, static_mesh=coarse)["face"], wide["face"]) and a.tsdf is made


def test_render_scene_without_the_new_arguments_is_the_parents(dev, aligner):
    """static_mesh=None runs the code of before, whatever shade and cull_back say: the same dict, key for key (tests/test_render_gpu.py
    and tests/test_motion_gpu.py, unchanged, pin what that code gives)."""
    from geo4d_amd import render
    a, s = aligner
    for persist in (False, True):
        base = render.render_scene(a, "playback", is_msk=False, persist_static=persist, trail=1)
        off = render.render_scene(a, "playback", is_msk=False, persist_static=persist, trail=1, static_mesh=None, shade=0.7, cull_back=True)
        assert sorted(base) == sorted(off) == ["depth", "index", "rgb"]
        for k in base:
            assert torch.equal(base[k], off[k]), (persist, k)


def test_save_scene_passes_render_kw_on(dev, tmp_path):
    from PIL import Image
    from geo4d_amd import scene_export
    a = _synthetic_aligner(dev, mr.synthetic_scene(noise=0.0))
    video = torch.rand((1, 3, a.n, a.H, a.W), generator=torch.Generator().manual_seed(6)) * 2 - 1
    plain = scene_export.save_scene(a, str(tmp_path / "plain"), "seq", imgs=video, render="playback")
    none = scene_export.save_scene(a, str(tmp_path / "none"), "seq", imgs=video, render="playback", render_kw=None)
    mesh = scene_export.save_scene(a, str(tmp_path / "mesh"), "seq", imgs=video, render="playback", render_kw=dict(static_mesh=True, shade=0.5))
    names = sorted(os.listdir(plain))
    assert sorted(os.listdir(none)) == names == sorted(os.listdir(mesh)) and "render" in names
    frames = sorted(os.listdir(os.path.join(plain, "render")))
    assert frames == sorted(os.listdir(os.path.join(mesh, "render"))) == [f"frame_{i:04d}.png" for i in range(a.n)] + ["render.gif"]
    read = lambda *p: open(os.path.join(*p), "rb").read()
    for f in names:
        if f != "render":
            assert read(plain, f) == read(none, f) == read(mesh, f), f
    for f in frames:
        assert read(plain, "render", f) == read(none, "render", f), f
    first = lambda d: np.asarray(Image.open(os.path.join(d, "render", "frame_0000.png")))
    assert first(mesh).shape == first(plain).shape and (first(mesh) != first(plain)).any()
