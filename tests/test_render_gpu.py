"""The renderer on the HIP path (geo4d_amd/render.py + csrc/render.hip) against its numpy restatement (tests/render_restatement.py):
exact images on a random case and the hand-made six-point case, a scene re-rendered into its own cameras, determinism, hole filling,
empty views, render_scene's modes and save_scene's render folder."""
import os

import numpy as np
import pytest
import torch

import render_restatement as rr
from scene_cases import tiny_aligner_and_fixture as _aligner
from test_render_cpu import CAM, KMAT, SIZE, check_six_point_case, random_case, six_points

pytestmark = pytest.mark.gpu


def _gpu(dev, points, colors, cams2world, K, size, **kw):
    """render_points on numpy inputs, numpy outputs."""
    from geo4d_amd import render
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = render.render_points(t(points), t(colors), torch.from_numpy(np.asarray(cams2world)), torch.from_numpy(np.asarray(K)), size,
                               mask=t(kw.pop("mask", None)), radius=t(kw.pop("radius", None)), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def case():
    """The random case and the restatement's images of it, computed once: s = 1 and adaptive radius with max_size 5."""
    c = random_case()
    kw = dict(mask=c["mask"], sources=c["sources"])
    c["kw"] = {"s1": kw, "adaptive": dict(kw, radius=c["radius"], max_size=5)}
    c["ref"] = {k: rr.render(c["points"], c["colors"], c["cams2world"], c["K"], c["size"], **v) for k, v in c["kw"].items()}
    return c


def _excusable(c, kw, ref, got):
    """Pixels that differ and may: a candidate of the pixel (the restatement's or the device's winner) projects within 1e-4 px of a
    rounding boundary, or the two winners' depths are less than 1 ulp apart."""
    views = rr.views_of(c["cams2world"], c["K"])
    ok = []
    for v, y, x in zip(*np.nonzero((ref["index"] != got["index"]) | (ref["depth"] != got["depth"]) | (ref["rgb"] != got["rgb"]).any(-1))):
        ids = np.array([i for i in (ref["index"][v, y, x], got["index"][v, y, x]) if i >= 0], dtype=np.int64)
        _, u, w, zc, s = rr.project(c["points"], views[v], ids, None, kw.get("radius"), 1e-3, kw.get("max_size", 9))
        edge = np.concatenate([u - np.float32(0.5) * (s - 1) + np.float32(0.5), w - np.float32(0.5) * (s - 1) + np.float32(0.5)])
        near_edge = (np.abs(edge - np.round(edge)) < 1e-4).any()
        bits = zc.view(np.uint32).astype(np.int64)
        ok.append(bool(near_edge or (len(ids) == 2 and abs(int(bits[0]) - int(bits[1])) < 1)))
    return ok


@pytest.mark.parametrize("which", ["s1", "adaptive"])
def test_matches_the_restatement(dev, case, which):
    ref = case["ref"][which]
    got = _gpu(dev, case["points"], case["colors"], case["cams2world"], case["K"], case["size"], **dict(case["kw"][which]))
    covered = int((ref["index"] >= 0).sum())
    ok = _excusable(case, case["kw"][which], ref, got)
    print(f"[render {which}] covered {covered} of {ref['index'].size} pixels, {len(ok)} differ / excluded (0 expected)")
    assert covered > 1000 and all(ok), ok
    assert len(ok) <= 1e-3 * covered
    assert got["rgb"].dtype == np.uint8 and got["depth"].dtype == np.float32 and got["index"].dtype == np.int32
    if which == "adaptive":                                                       # footprints did grow
        assert covered > 1.5 * int((case["ref"]["s1"]["index"] >= 0).sum())


def test_six_point_case_on_the_device(dev):
    check_six_point_case(lambda *a, **kw: _gpu(dev, *a, **kw))


def test_scene_renders_onto_itself(dev):
    """Every image drawn alone into its own camera at one pixel per point lands every masked point on the pixel it came from."""
    from geo4d_amd import render
    a, _ = _aligner(dev)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(2)).to(dev)
    thr = float(a.im_conf.median())
    out = render.render_scene(a, "cameras", sources=[[i] for i in range(a.n)], min_conf_thr=thr)
    msk = a.get_masks()
    assert 0 < int(msk.sum()) < msk.numel()
    own = torch.arange(a.n * a.H * a.W, device=dev, dtype=torch.int32).reshape(a.n, a.H, a.W)
    assert torch.equal(out["index"], torch.where(msk, own, torch.full_like(own, -1)))
    depth = a.get_depthmaps().detach()
    rel = ((out["depth"] - depth).abs() / depth)[msk].max().item()
    print(f"[self-render] {int(msk.sum())} points, depth rel err max {rel:.2e}")
    assert rel <= 1e-5 and bool((out["depth"][~msk] == 0).all())
    want = torch.from_numpy(rr.quantise(a.imgs.cpu().numpy())).to(dev)
    assert torch.equal(out["rgb"][msk], want[msk]) and bool((out["rgb"][~msk] == 255).all())


def test_deterministic_and_order_free(dev, case):
    from geo4d_amd import render
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    pts, col, mask, rad = t(case["points"]), t(case["colors"]), t(case["mask"]), t(case["radius"])
    c2w, K = torch.from_numpy(case["cams2world"]), torch.from_numpy(case["K"])
    run = lambda src, views=slice(None): render.render_points(pts, col, c2w[views], K[views], case["size"], mask=mask, radius=rad,
                                                              max_size=5, fill=1, sources=src)
    a, b = run(case["sources"]), run(case["sources"])
    permuted = run([s[::-1] for s in case["sources"]])
    for k in ("rgb", "depth", "index"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], permuted[k]), k
    for v in range(3):
        single = run([case["sources"][v]], slice(v, v + 1))
        for k in ("rgb", "depth", "index"):
            assert torch.equal(single[k][0], a[k][v]), (k, v)


@pytest.mark.parametrize("passes", [1, 2, 3])
def test_fill_matches_the_restatement(dev, case, passes):
    kw = case["kw"]["s1"]
    base = case["ref"]["s1"]
    ref = rr.resolve(rr.fill(base["keys"], passes), case["colors"])
    got = _gpu(dev, case["points"], case["colors"], case["cams2world"], case["K"], case["size"], fill=passes, **dict(kw))
    for k, r in zip(("rgb", "depth", "index"), ref):
        assert np.array_equal(got[k], r), k
    hit = base["index"] >= 0
    assert np.array_equal(got["index"][hit], base["index"][hit]) and (got["index"] >= 0).sum() > hit.sum()
    none = _gpu(dev, case["points"], case["colors"], case["cams2world"], case["K"], case["size"], fill=0, **dict(kw))
    for k in ("rgb", "depth", "index"):
        assert np.array_equal(none[k], base[k]), k


def test_view_without_sources_is_background(dev):
    pts, col = six_points()
    out = _gpu(dev, pts, col, np.stack([CAM, CAM]), np.stack([KMAT, KMAT]), SIZE, sources=[[], [0]], background=(0.2, 0.4, 1.0), fill=2)
    assert (out["index"][0] == -1).all() and (out["depth"][0] == 0).all()
    assert (out["rgb"][0] == rr.quantise([0.2, 0.4, 1.0])).all()
    assert (out["index"][1] >= 0).sum() > 3
    empty = _gpu(dev, pts, col, CAM[None], KMAT[None], SIZE, sources=[[]])
    assert (empty["index"] == -1).all() and (empty["rgb"] == 255).all()


def test_render_scene_modes_and_save_scene(dev, tmp_path):
    from geo4d_amd import render, scene_export
    a, _ = _aligner(dev)
    video = torch.rand((1, 3, a.n, a.H, a.W), generator=torch.Generator().manual_seed(6)) * 2 - 1
    plain = scene_export.save_scene(a, str(tmp_path / "plain"), "seq", imgs=video)
    drawn = scene_export.save_scene(a, str(tmp_path / "drawn"), "seq", imgs=video, render="cameras")
    names = sorted(os.listdir(plain))
    assert sorted(os.listdir(drawn)) == sorted(names + ["render"])
    for f in names:
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(drawn, f), "rb").read(), f
    assert sorted(os.listdir(os.path.join(drawn, "render"))) == [f"frame_{i:04d}.png" for i in range(a.n)] + ["render.gif"]
    from PIL import Image
    first = np.asarray(Image.open(os.path.join(drawn, "render", "frame_0000.png")))
    cams = render.render_scene(a, "cameras", min_conf_thr=2, is_msk=False)
    assert first.shape == (a.H, a.W, 3) and np.array_equal(first, cams["rgb"][0].cpu().numpy())

    play = render.render_scene(a, "playback", trail=1, min_conf_thr=2, is_msk=False, point_size=2)
    for k, shape, dt in (("rgb", (a.n, a.H, a.W, 3), torch.uint8), ("depth", (a.n, a.H, a.W), torch.float32), ("index", (a.n, a.H, a.W), torch.int32)):
        assert tuple(play[k].shape) == shape and play[k].dtype == dt and play[k].device.type == "cuda"
    HW = a.H * a.W
    for t in range(a.n):                                                          # view t draws images t - 1 and t only
        ids = play["index"][t][play["index"][t] >= 0]
        assert len(ids) and int(ids.min()) >= max(0, t - 1) * HW and int(ids.max()) < (t + 1) * HW
    size = (a.H // 2 + 3, a.W + 5)
    turn = render.render_scene(a, "turntable", n_views=5, size=size, min_conf_thr=2, is_msk=False, point_size=2, fill=1)
    assert tuple(turn["rgb"].shape) == (5,) + size + (3,) and tuple(turn["depth"].shape) == (5,) + size == tuple(turn["index"].shape)
    assert all(int((turn["index"][v] >= 0).sum()) > 0 for v in range(5))           # the orbit looks at the scene
    with pytest.raises(ValueError):
        render.render_scene(a, "playback", path=torch.eye(4)[None])
