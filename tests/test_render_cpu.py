"""The renderer's host side (geo4d_amd/render.py, the four geo4d_render_* symbols) and its numpy restatement
(tests/render_restatement.py), without a GPU: ABI agreement, host-side argument validation, orbit poses, PNG round trip, and the
restatement's rules on a hand-made six-point case (shared with tests/test_render_gpu.py, which asserts the same on the device)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import render_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geo4d_render_workspace", "geo4d_render_splat", "geo4d_render_fill", "geo4d_render_resolve")


# ---- the hand-made case: one camera at the origin looking down +z, f = 8, 8 x 8 frame, principal point (4, 4) --------------------------
def six_points():
    """points, colours, the expected winner per pixel. u = 8 x / z + 4, v = 8 y / z + 4."""
    nan, inf = float("nan"), float("inf")
    pts = np.array([
        [0.0, 0.0, 4.0],        # 0: far point on pixel (4, 4)
        [0.0, 0.0, 2.0],        # 1: nearer point on the same pixel: wins, whatever the order
        [0.5, 0.0, 2.0],        # 2: pixel (x 6, y 4) ...
        [1.0, 0.0, 4.0],        # 3: ... the same pixel at a larger depth; with equal depth (below) the lower id wins
        [-1.0, -1.0, 2.0],      # 4: pixel (0, 0): a 3 x 3 footprint is clipped to 2 x 2
        [0.0, 0.0, -2.0],       # 5: behind the camera: never writes
    ], dtype=np.float32)
    bad = np.array([[nan, 0, 2], [0, inf, 2], [0, 0, inf], [0.25, 0.25, nan]], dtype=np.float32)
    col = np.linspace(0.05, 0.95, 3 * (len(pts) + len(bad)), dtype=np.float32).reshape(-1, 3)
    return np.concatenate([pts, bad]), col


CAM = np.eye(4)
KMAT = np.array([[8.0, 0, 4], [0, 8.0, 4], [0, 0, 1]])
SIZE = (8, 8)


def check_six_point_case(render):
    """`render(points, colors, cams2world, K, size, **kw)` -> dict of numpy rgb / depth / index [1, 8, 8(, 3)]: the rules of the issue."""
    pts, col = six_points()
    base = render(pts, col, CAM[None], KMAT[None], SIZE)
    idx, depth, rgb = base["index"][0], base["depth"][0], base["rgb"][0]
    assert idx[4, 4] == 1 and depth[4, 4] == np.float32(2.0)                      # the nearer point wins ...
    assert idx[4, 6] == 2 and depth[4, 6] == np.float32(2.0)
    assert idx[0, 0] == 4
    assert (idx >= 0).sum() == 3 and set(idx[idx >= 0]) == {1, 2, 4}              # behind-camera, NaN and Inf points never write
    assert (depth[idx < 0] == 0).all() and (rgb[idx < 0] == 255).all()
    assert (rgb[4, 4] == rr.quantise(col[1])).all()
    perm = np.array([3, 9, 1, 5, 0, 7, 2, 8, 4, 6])                               # ... whatever the order
    shuffled = render(pts[perm], col[perm], CAM[None], KMAT[None], SIZE)
    assert np.array_equal(np.where(shuffled["index"] >= 0, perm[shuffled["index"]], -1), base["index"])
    assert np.array_equal(shuffled["depth"], base["depth"]) and np.array_equal(shuffled["rgb"], base["rgb"])
    tie = pts.copy()
    tie[3] = [0.5, 0.0, 2.0]                                                      # equal depth on pixel (6, 4): the lower id wins
    assert render(tie, col, CAM[None], KMAT[None], SIZE)["index"][0, 4, 6] == 2
    tie[[2, 3]] = tie[[3, 2]]
    assert render(tie, col, CAM[None], KMAT[None], SIZE)["index"][0, 4, 6] == 2
    # footprints: radius 0.375 at z = 2, f = 8 -> ceil(2 * 0.375 * 8 / 2) = 3 pixels; clipped at the border, capped by max_size
    rad = np.full(len(pts), 0.375, dtype=np.float32)
    fat = render(pts, col, CAM[None], KMAT[None], SIZE, radius=rad, max_size=5)["index"][0]
    assert (fat[0:2, 0:2] == 4).all() and (fat == 4).sum() == 4                   # 3 x 3 round (0, 0), clipped to 2 x 2
    assert (fat[3:6, 3:6] == 1).all() and (fat == 1).sum() == 9
    assert (fat[3:6, 6:8] == 2).all() and (fat == 2).sum() == 6                   # columns 5..7, column 5 lost to point 1 at equal depth
    assert (fat == 0).sum() == 0 and (fat == 3).sum() == 0
    capped = render(pts, col, CAM[None], KMAT[None], SIZE, radius=rad, max_size=2)["index"][0]
    assert (capped == 1).sum() == 4 and (capped[4:6, 4:6] == 1).all()             # even side 2: floor(4 - 0.5 + 0.5) = 4 -> pixels 4, 5
    keep = np.ones(len(pts), dtype=bool)
    keep[1] = False
    assert render(pts, col, CAM[None], KMAT[None], SIZE, mask=keep)["index"][0, 4, 4] == 0     # masked out: the far point shows


def test_restatement_on_the_six_point_case():
    check_six_point_case(rr.render)


def test_restatement_fill_and_empty_view():
    pts, col = six_points()
    out = rr.render(pts, col, np.stack([CAM, CAM]), np.stack([KMAT, KMAT]), SIZE, sources=[[0], []])
    assert (out["index"][1] == -1).all() and (out["depth"][1] == 0).all() and (out["rgb"][1] == 255).all()
    k0 = out["keys"]
    k1 = rr.fill(k0, 1)
    hit = k0 != rr.EMPTY
    assert np.array_equal(k1[hit], k0[hit]) and (k1[1] == rr.EMPTY).all()
    assert (k1[0, 3:6, 3:6] == k0[0, 4, 4]).all() and (k1[0] != rr.EMPTY).sum() == 9 + 6 + 4
    assert np.array_equal(rr.fill(k0, 0), k0)
    # between two neighbours the smaller key (the nearer point) fills
    k = np.full((1, 1, 3), rr.EMPTY, dtype=np.uint64)
    k[0, 0, 0], k[0, 0, 2] = (np.uint64(np.float32(3).view(np.uint32)) << np.uint64(32)) | np.uint64(7), \
                             (np.uint64(np.float32(2).view(np.uint32)) << np.uint64(32)) | np.uint64(9)
    assert rr.fill(k, 1)[0, 0, 1] == k[0, 0, 2]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_render_symbols_agree_between_header_binding_and_library():
    from geo4d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geo4d_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.geo4d_abi_version() == _lib.ABI_VERSION == 9 == int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1))
    assert lib.geo4d_render_workspace(3, 40, 48, 9) == 2 * 3 * 40 * 48 * 8 + 9 * 8
    assert lib.geo4d_render_workspace(0, 40, 48, 9) == 0 and lib.geo4d_render_workspace(1 << 11, 1 << 10, 1 << 10, 1) == 0


def test_bad_descriptors_are_refused_on_the_host():
    """Every refusal is -EINVAL with a message and comes before any launch: the pointers below are not device memory."""
    from geo4d_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 8192)()                                   # host memory standing in for "non-null, 8-byte aligned"
    p = ctypes.addressof(buf)
    ptr, src = (ctypes.c_int * 3)(0, 1, 2), (ctypes.c_int * 2)(0, 1)
    V, H, W, N, P = 2, 4, 4, 32, 16
    need = lib.geo4d_render_workspace(V, H, W, 2)

    def splat(points=p, views=p, vptr=ptr, vsrc=src, N=N, P=P, V=V, H=H, W=W, near=1e-3, max_size=9, ws=p, ws_bytes=need):
        return lib.geo4d_render_splat(points, None, None, N, P, views, vptr, vsrc, V, H, W, near, max_size, ws, ws_bytes, None)

    cases = [dict(points=None), dict(views=None), dict(vptr=None), dict(ws=None), dict(V=0), dict(H=0), dict(W=-1),
             dict(V=1, H=1 << 16, W=1 << 15), dict(N=(1 << 32) - 1, P=(1 << 32) - 1), dict(N=0), dict(N=33), dict(max_size=0),
             dict(max_size=65), dict(near=float("nan")), dict(vsrc=(ctypes.c_int * 2)(0, 2)), dict(vsrc=(ctypes.c_int * 2)(-1, 0)),
             dict(vptr=(ctypes.c_int * 3)(0, 2, 1)), dict(vptr=(ctypes.c_int * 3)(1, 1, 2)), dict(ws_bytes=need - 1), dict(ws=p + 4)]
    for kw in cases:
        assert splat(**kw) == -22, kw
        assert b"render_splat" in lib.geo4d_last_error(), kw
    for args in [(0, H, W, 1, p, need), (V, H, W, -1, p, need), (V, H, W, 1, None, need), (V, H, W, 1, p, 2 * V * H * W * 8 - 1),
                 (1, 1 << 16, 1 << 15, 1, p, need)]:
        assert lib.geo4d_render_fill(*args, None) == -22 and b"render_fill" in lib.geo4d_last_error(), args
    bg = (ctypes.c_float * 3)(1, 1, 1)

    def resolve(colors=p, N=N, bg=bg, V=V, H=H, W=W, rgb=p, depth=p, index=p, ws=p, ws_bytes=need):
        return lib.geo4d_render_resolve(colors, N, bg, V, H, W, rgb, depth, index, ws, ws_bytes, None)
    for kw in [dict(colors=None), dict(bg=None), dict(N=0), dict(N=1 << 31), dict(V=0), dict(W=0), dict(ws=None), dict(ws_bytes=V * H * W * 8 - 1),
               dict(rgb=None, depth=None, index=None), dict(V=1, H=1 << 16, W=1 << 15)]:
        assert resolve(**kw) == -22 and b"render_resolve" in lib.geo4d_last_error(), kw


def test_render_points_refuses_cpu_tensors():
    from geo4d_amd import _lib, render
    pts, col = six_points()
    with pytest.raises(_lib.Geo4DNativeError):
        render.render_points(torch.from_numpy(pts), torch.from_numpy(col), torch.eye(4)[None], torch.from_numpy(KMAT)[None], SIZE)


def test_render_scene_refuses_unknown_modes():
    from geo4d_amd import render
    with pytest.raises(ValueError):
        render.render_scene(object(), "fly-through")


# ---- host helpers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", [(0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.3, -0.9, 0.2)])
def test_orbit_cameras_look_at_the_centre(up):
    from geo4d_amd.render import orbit_cameras
    c = np.array([0.5, -1.0, 3.0])
    poses = orbit_cameras(c, 2.5, 7, elevation=0.4, up=up)
    assert poses.shape == (7, 4, 4) and np.array_equal(poses[:, 3], np.tile([0, 0, 0, 1.0], (7, 1)))
    upn = np.asarray(up) / np.linalg.norm(up)
    for T in poses:
        R, t = T[:3, :3], T[:3, 3]
        np.testing.assert_allclose(R.T @ R, np.eye(3), atol=1e-12)                # orthonormal
        assert np.linalg.det(R) > 0.999999                                       # right-handed
        np.testing.assert_allclose(np.linalg.norm(c - t), 2.5, rtol=1e-12)
        np.testing.assert_allclose(np.cross(R[:, 2], c - t), 0, atol=1e-12)       # the +z axis passes through the centre ...
        assert R[:, 2] @ (c - t) > 0                                             # ... forwards
        assert R[:, 1] @ upn < 0 and abs(R[:, 0] @ upn) < 1e-12                   # y down, x level
        np.testing.assert_allclose((t - c) @ upn, 2.5 * np.sin(0.4), rtol=1e-12)
    assert len({tuple(np.round(T[:3, 3], 9)) for T in poses}) == 7
    # the centre projects onto the principal point of every view
    pts = np.float32(c)[None]
    out = rr.render(pts, np.float32([[0, 0, 0]]), poses, np.tile(KMAT, (7, 1, 1)), SIZE)
    assert (out["index"][:, 4, 4] == 0).all() and (out["index"] >= 0).sum() == 7


def test_save_render_round_trips_through_png(tmp_path):
    from PIL import Image
    from geo4d_amd.render import save_render
    rgb = np.random.default_rng(0).integers(0, 256, (3, 5, 7, 3), dtype=np.uint8)
    d = save_render(str(tmp_path / "r"), torch.from_numpy(rgb), fps=5)
    assert sorted(os.listdir(d)) == ["frame_0000.png", "frame_0001.png", "frame_0002.png", "render.gif"]
    for i in range(3):
        assert np.array_equal(np.asarray(Image.open(os.path.join(d, f"frame_{i:04d}.png"))), rgb[i])
    assert Image.open(os.path.join(d, "render.gif")).n_frames == 3
    with pytest.raises(ValueError):
        save_render(str(tmp_path / "bad"), rgb.astype(np.float32))


# ---- the GPU test's random case, checked here first: the seed keeps clear of rounding boundaries --------------------------------------
def random_case(seed=11):
    """3 images of 24 x 32 points round three cameras, 3 views of 40 x 48: some points behind a camera, some outside the frustum, and
    masked-out entries that hold NaN."""
    g = np.random.default_rng(seed)
    n, h, w, H, W = 3, 24, 32, 40, 48
    pts = np.stack([g.uniform(-2.5, 2.5, (n, h, w)), g.uniform(-2.0, 2.0, (n, h, w)), g.uniform(-1.0, 6.0, (n, h, w))], -1).astype(np.float32)
    col = g.uniform(-0.05, 1.05, (n, h, w, 3)).astype(np.float32)
    mask = g.uniform(size=(n, h, w)) < 0.85
    holes = ~mask & (g.uniform(size=(n, h, w)) < 0.5)
    pts[holes] = np.nan
    radius = g.uniform(0.0, 0.12, (n, h, w)).astype(np.float32)
    c2w = np.tile(np.eye(4), (3, 1, 1))
    for k, a in enumerate((-0.35, 0.0, 0.3)):
        c2w[k, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        c2w[k, :3, 3] = [0.8 * k - 0.8, 0.1 * k, -0.5 * k]
    K = np.tile(np.array([[30.0, 0, W / 2], [0, 31.0, H / 2], [0, 0, 1]]), (3, 1, 1))
    K[1, 0, 2] += 1.25
    return dict(points=pts, colors=col, mask=mask, radius=radius, cams2world=c2w, K=K, size=(H, W), sources=[[0, 1, 2], [2, 0], [1]])


def test_random_case_seed_keeps_clear_of_rounding_boundaries():
    """Moving u and v by one float32 step either way changes at most 0.1 % of the covered pixels (the cap on what the GPU test may
    exclude); the case really holds points behind the cameras, outside the frustum and NaN under the mask."""
    c = random_case()
    kw = dict(mask=c["mask"], sources=c["sources"])
    for extra in (dict(), dict(radius=c["radius"], max_size=5)):
        base = rr.render(c["points"], c["colors"], c["cams2world"], c["K"], c["size"], **kw, **extra)
        covered = int((base["index"] >= 0).sum())
        assert covered > 1000
        for du in (-1, 1):
            for dv in (-1, 1):
                moved = rr.render(c["points"], c["colors"], c["cams2world"], c["K"], c["size"], ulp=(du, dv), **kw, **extra)
                assert int((moved["index"] != base["index"]).sum()) <= 1e-3 * covered
    assert np.isnan(c["points"][~c["mask"]]).any() and not np.isnan(c["points"][c["mask"]]).any()
    views = rr.views_of(c["cams2world"], c["K"])
    ids = np.arange(c["points"].size // 3)
    keep, u, v, zc, _ = rr.project(c["points"], views[0], ids, c["mask"])
    assert (zc[np.isfinite(zc)] < 0).sum() > 50
    assert (keep & ((u < -1) | (u > c["size"][1]) | (v < -1) | (v > c["size"][0]))).sum() > 50
