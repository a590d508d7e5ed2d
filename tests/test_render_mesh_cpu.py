"""The mesh renderer's host side (geo4d_amd/render.py render_mesh, the three new geo4d_render_* symbols) and its numpy restatement
(tests/render_mesh_restatement.py), without a GPU: the rule on hand-made triangles (shared with tests/test_render_mesh_gpu.py, which
asserts the same on the device), watertight shared edges, ABI agreement and host-side refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import render_mesh_restatement as rm
import render_restatement as rr
from test_render_cpu import CAM, KMAT, SIZE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geo4d_render_raster_workspace", "geo4d_render_raster", "geo4d_render_resolve_mesh")
F = np.float32


def tri_at(pixels, z, K=KMAT):
    """World vertices (camera at the origin) that project onto `pixels` [(x, y), ...] at depths z (scalar or per vertex)."""
    px = np.asarray(pixels, dtype=np.float64)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (len(px),))
    return np.stack([(px[:, 0] - K[0, 2]) * z / K[0, 0], (px[:, 1] - K[1, 2]) * z / K[1, 1], z], 1).astype(F)


HAND = [(1, 1), (6, 1), (1, 6)]                                                    # A > 0: a back face


def check_hand_cases(render):
    """`render(vertices, faces, cams2world, K, size, **kw)` -> dict of numpy rgb / depth / index / face: the rules of the issue."""
    one = lambda v, f=((0, 1, 2),), **kw: render(np.asarray(v, dtype=F), np.asarray(f, dtype=np.int32).reshape(-1, 3), CAM[None], KMAT[None],
                                                  SIZE, **kw)
    yy, xx = np.mgrid[0:8, 0:8]
    want = (xx >= 1) & (yy >= 1) & (xx + yy <= 7)
    out = one(tri_at(HAND, 2.0))
    assert want.sum() == 21 and np.array_equal(out["face"][0] == 0, want)
    assert (out["depth"][0][want] == F(2)).all() and (out["depth"][0][~want] == 0).all()
    assert (out["index"] == -1).all() and (out["rgb"][0][~want] == 255).all()
    assert (out["rgb"][0][want] == rr.quantise([0.7, 0.7, 0.7])).all()
    out3 = one(tri_at(HAND, 3.0))
    assert np.array_equal(out3["face"][0] == 0, want)
    ulps = np.abs(out3["depth"][0][want].view(np.int32).astype(np.int64) - int(F(3).view(np.int32)))
    assert ulps.max() <= 1, ulps.max()
    # the nearer of two overlapping triangles wins in either face order; at equal depth the lower face
    both = np.concatenate([tri_at(HAND, 3.0), tri_at([(0, 0), (7, 0), (0, 7)], 2.0)])
    far_first = one(both, [(0, 1, 2), (3, 4, 5)])
    assert (far_first["face"][0][want] == 1).all() and (far_first["depth"][0][want] < F(2.001)).all()       # weights of 1 / 49: 2 +- 1 ulp
    near_first = one(both, [(3, 4, 5), (0, 1, 2)])
    assert (near_first["face"][0][want] == 0).all() and np.array_equal(near_first["depth"], far_first["depth"])
    tie = one(np.concatenate([tri_at(HAND, 2.0), tri_at(HAND, 2.0)]), [(3, 4, 5), (0, 1, 2)])
    assert np.array_equal(tie["face"][0] == 0, want) and (tie["face"] != 1).all()
    # a point at the same depth beats the triangle
    pt = tri_at([(2, 2)], 2.0)
    mixed = one(tri_at(HAND, 2.0), points=pt, point_colors=np.array([[0.1, 0.5, 0.9]], dtype=F))
    assert mixed["index"][0, 2, 2] == 0 and mixed["face"][0, 2, 2] == -1 and (mixed["rgb"][0, 2, 2] == rr.quantise([0.1, 0.5, 0.9])).all()
    assert (mixed["face"][0] == 0).sum() == 20 and (mixed["index"] >= 0).sum() == 1
    behind = one(tri_at(HAND, 2.0), points=tri_at([(2, 2)], 2.5), point_colors=np.zeros((1, 3), dtype=F))
    assert (behind["index"] == -1).all() and np.array_equal(behind["face"][0] == 0, want)
    # dropped whole: a vertex behind the camera, NaN, Inf, beyond the guard band, zero area, masked, an index of -1, an index of Nv
    empty = lambda o: (o["face"] == -1).all() and (o["index"] == -1).all() and (o["depth"] == 0).all() and (o["rgb"] == 255).all()
    good = tri_at(HAND, 2.0)
    for k, bad in enumerate(([0.0, 0.0, -2.0], [np.nan, 0, 2], [0, np.inf, 2], [20000.0, 0.0, 2.0])):
        v = good.copy()
        v[k % 3] = bad
        assert empty(one(v)), bad
    assert 8.0 * 20000.0 / 2.0 + 4 > 65536                                         # the last one was the guard band
    assert empty(one(tri_at([(1, 1), (3, 3), (6, 6)], 2.0)))
    assert empty(one(good, face_mask=np.array([False])))
    assert empty(one(good, [(0, 1, -1)])) and empty(one(good, [(0, 3, 2)]))
    # cull_back drops exactly the faces with A > 0
    assert empty(one(good, cull_back=True))
    front = one(good, [(0, 2, 1)], cull_back=True)
    assert np.array_equal(front["face"][0] == 0, want) and np.array_equal(front["depth"], out["depth"])
    # smaller than a pixel and no pixel centre inside: nothing
    assert empty(one(tri_at([(2.2, 2.2), (2.8, 2.3), (2.4, 2.9)], 2.0)))
    assert (one(tri_at([(2.7, 2.7), (3.3, 2.8), (2.9, 3.4)], 2.0))["face"] == 0).sum() == 1


def test_restatement_on_the_hand_made_cases():
    check_hand_cases(rm.render)


K32 = np.array([[16.0, 0, 16], [0, 16.0, 16], [0, 0, 1]])


def _inside(X, Y, x, y):
    """Exact integer test of pixel centres (x, y) against the convex polygon with snapped corners X, Y (either orientation): all edge
    functions >= 0 or all <= 0."""
    sx, sy = x * 256, y * 256
    n = len(X)
    E = [(int(X[(k + 1) % n]) - int(X[k])) * (sy - int(Y[k])) - (int(Y[(k + 1) % n]) - int(Y[k])) * (sx - int(X[k])) for k in range(n)]
    return np.logical_and.reduce([e >= 0 for e in E]) | np.logical_and.reduce([e <= 0 for e in E])


def test_quads_split_along_a_diagonal_leave_no_gap():
    g = np.random.default_rng(0)
    H = W = 32
    verts, faces = [], []
    for q in range(300):
        centre, rad = g.uniform(-2, 34, 2), g.uniform(2, 14)
        ang = np.sort(g.uniform(0, 2 * np.pi / 4 - 0.3, 4) + np.arange(4) * (2 * np.pi / 4))[::(-1 if q & 1 else 1)]
        verts.append(tri_at(centre + rad * np.stack([np.cos(ang), np.sin(ang)], 1), g.uniform(1.0, 4.0, 4), K32))
        faces += [(4 * q, 4 * q + 1, 4 * q + 2), (4 * q, 4 * q + 2, 4 * q + 3)]
    s = rm.setup(np.concatenate(verts), np.array(faces), rr.views_of(CAM[None], K32[None])[0], (H, W))
    assert s["keep"].all()
    yy, xx = np.mgrid[0:H, 0:W]
    covered_any = 0
    for q in range(300):
        got = np.zeros((H, W), dtype=bool)
        for t in (2 * q, 2 * q + 1):
            x, y, _ = rm.candidates(s, t)
            got[y, x] = True
        X = np.append(s["X"][2 * q], s["X"][2 * q + 1][2])
        Y = np.append(s["Y"][2 * q], s["Y"][2 * q + 1][2])
        assert np.array_equal(got, _inside(X, Y, xx, yy)), q
        covered_any += int(got.sum())
    assert covered_any > 300 * 20


def jittered_grid(seed=3, n=7, K=K32):
    """(vertices [n n, 3], faces [2 (n-1)^2, 3]) of an n x n grid over a 32 x 32 frame, jittered in the image and in depth."""
    g = np.random.default_rng(seed)
    gy, gx = np.mgrid[0:n, 0:n]
    px = np.stack([gx, gy], -1).reshape(-1, 2) * (36.0 / (n - 1)) - 2 + g.uniform(-1.5, 1.5, (n * n, 2))
    v = tri_at(px, g.uniform(2.0, 3.0, n * n), K)
    f = []
    for r in range(n - 1):
        for c in range(n - 1):
            a = r * n + c
            f += [(a, a + 1, a + n), (a + 1, a + n + 1, a + n)]
    return v, np.array(f, dtype=np.int32)


def test_jittered_grid_is_watertight_and_the_nearest_candidate_wins():
    v, f = jittered_grid()
    H = W = 32
    assert len(f) == 72
    out = rm.render(v, f, CAM[None], K32[None], (H, W))
    s = rm.setup(v, f, rr.views_of(CAM[None], K32[None])[0], (H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    best = np.full((H, W), np.iinfo(np.int64).max)
    for t in range(72):
        inside = _inside(s["X"][t], s["Y"][t], xx, yy)
        _, _, zc = rm.weights(s, t, xx.reshape(-1), yy.reshape(-1))
        key = (zc.view(np.uint32).astype(np.int64).reshape(H, W) << 32) | t
        best = np.where(inside, np.minimum(best, key), best)
    hit = best != np.iinfo(np.int64).max
    assert hit.sum() > 600 and np.array_equal(out["face"][0] >= 0, hit)
    assert np.array_equal(out["face"][0][hit], (best & 0xFFFFFFFF)[hit])
    assert np.array_equal(out["depth"][0][hit].view(np.uint32), (best >> 32)[hit].astype(np.uint32))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_mesh_symbols_agree_between_header_binding_and_library():
    from geo4d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geo4d_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.geo4d_abi_version() == _lib.ABI_VERSION == 9 == int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1))
    assert lib.geo4d_render_raster_workspace(0) == 8 and lib.geo4d_render_raster_workspace(1000) == 8 + 8 * 1000
    assert lib.geo4d_render_raster_workspace(-1) == 0 and lib.geo4d_render_raster_workspace((1 << 28) + 1) == 0


def test_bad_mesh_arguments_are_refused_on_the_host():
    """Every refusal is -EINVAL with the function's name and comes before any launch: the pointers below are not device memory."""
    from geo4d_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 8192)()
    p = ctypes.addressof(buf)
    V, H, W, Nv, T = 2, 4, 4, 12, 5
    need = lib.geo4d_render_workspace(V, H, W, 0)

    def raster(vertices=p, Nv=Nv, faces=p, T=T, views=p, V=V, H=H, W=W, near=1e-3, id_base=0, large_area=64, ws=p, ws_bytes=need, lst=p,
               lst_bytes=lib.geo4d_render_raster_workspace(4)):
        return lib.geo4d_render_raster(vertices, Nv, faces, T, None, views, V, H, W, near, 0, id_base, 1, large_area, ws, ws_bytes, lst,
                                       lst_bytes, None)

    for kw in [dict(views=None), dict(ws=None), dict(ws=p + 4), dict(lst=None), dict(lst=p + 4), dict(V=0), dict(H=0), dict(W=-1),
               dict(V=1, H=16385, W=4), dict(V=1, H=4, W=16385), dict(V=1 << 11, H=1 << 10, W=1 << 10), dict(vertices=None), dict(faces=None),
               dict(Nv=-1), dict(T=-1), dict(Nv=1 << 31), dict(id_base=-1), dict(id_base=(1 << 32) - 1 - T), dict(near=float("nan")),
               dict(near=-1.0), dict(large_area=-1), dict(ws_bytes=V * H * W * 8 - 1), dict(lst_bytes=7)]:
        assert raster(**kw) == -22, kw
        assert b"render_raster" in lib.geo4d_last_error(), kw
    bg = (ctypes.c_float * 3)(1, 1, 1)

    def resolve(colors=p, N=7, vertices=p, Nv=Nv, faces=p, T=T, rgba=None, rgbf=None, mc=bg, views=p, near=1e-3, shade=0.5, bg=bg, V=V, H=H,
                W=W, rgb=p, depth=p, index=p, face=p, ws=p, ws_bytes=need):
        return lib.geo4d_render_resolve_mesh(colors, N, vertices, Nv, faces, T, rgba, rgbf, mc, views, near, shade, bg, V, H, W, rgb, depth,
                                             index, face, ws, ws_bytes, None)

    for kw in [dict(colors=None), dict(N=-1), dict(N=1 << 31), dict(vertices=None), dict(faces=None), dict(Nv=-1), dict(T=-1), dict(T=1 << 31),
               dict(rgba=p, rgbf=p), dict(mc=None), dict(views=None), dict(bg=None),
               dict(near=float("nan")), dict(shade=-0.1), dict(shade=1.5), dict(shade=float("nan")), dict(V=0), dict(W=0),
               dict(V=1, H=16385, W=4), dict(ws=None), dict(ws=p + 4), dict(ws_bytes=V * H * W * 8 - 1),
               dict(rgb=None, depth=None, index=None, face=None)]:
        assert resolve(**kw) == -22, kw
        assert b"render_resolve_mesh" in lib.geo4d_last_error(), kw


def test_render_mesh_refuses_cpu_tensors():
    from geo4d_amd import _lib, render
    v, f = torch.from_numpy(tri_at(HAND, 2.0)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(_lib.Geo4DNativeError):
        render.render_mesh(v, f, torch.eye(4)[None], torch.from_numpy(KMAT)[None], SIZE)


def test_render_scene_refuses_static_mesh_with_persist_static():
    from geo4d_amd import render
    with pytest.raises(ValueError, match="static_mesh"):
        render.render_scene(object(), "cameras", static_mesh=True, persist_static=True)
