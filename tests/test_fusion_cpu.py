"""The fusion rule without a GPU: its numpy restatement (tests/fusion_restatement.py) on random clouds and on the synthetic scene of
tests/motion_restatement.py, and the host side of the HIP path (geo4d_amd/fusion.py, the four geo4d_fuse_* symbols): ABI agreement,
host-side argument validation and the Python errors. tests/test_fusion_gpu.py asserts the device against the same restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fusion_restatement as fr
import motion_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geo4d_fuse_workspace", "geo4d_fuse_insert", "geo4d_fuse_compact", "geo4d_fuse_finalize")
KEYS = ("points", "rgba", "weight", "count")


@pytest.fixture(scope="module")
def cloud():
    """3 000 points in [-2, 2]^3 with colours, weights in (0, 300), a mask, and some rows that take no part."""
    g = np.random.default_rng(5)
    p = g.uniform(-2, 2, size=(3000, 3)).astype(np.float32)
    w = g.uniform(0.001, 300, size=3000).astype(np.float32)
    p[::97, 1] = np.nan
    p[5::101, 0] = np.inf
    w[3::89] = 0
    w[7::83] = -1
    w[11::79] = np.nan
    return dict(points=p, rgba=g.integers(0, 256, size=(3000, 4), dtype=np.uint8), weight=w, mask=g.uniform(size=3000) < 0.8, voxel=0.25)


def _fuse(c, **kw):
    return fr.fuse(c["points"], c["rgba"], c["weight"], c["mask"], voxel=c["voxel"], **kw)


# ---- properties of the rule --------------------------------------------------------------------------------------------------------------
def test_mean_does_not_depend_on_the_row_order(cloud):
    a = _fuse(cloud)
    perm = np.random.default_rng(1).permutation(3000)
    b = fr.fuse(cloud["points"][perm], cloud["rgba"][perm], cloud["weight"][perm], cloud["mask"][perm], voxel=cloud["voxel"])
    assert len(a["points"]) > 1000
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


def test_count_sums_to_the_points_that_take_part(cloud):
    part, dropped = fr.taking_part(cloud["points"], cloud["weight"], cloud["mask"], cloud["voxel"])
    w = cloud["weight"]
    with np.errstate(invalid="ignore"):
        by_hand = cloud["mask"] & np.isfinite(cloud["points"]).all(1) & np.isfinite(w) & (w > 0)
    assert dropped == 0 and np.array_equal(part, by_hand) and 0 < part.sum() < cloud["mask"].sum()
    for reduce in ("mean", "best"):
        out = _fuse(cloud, reduce=reduce)
        assert int(out["count"].sum()) == int(part.sum()) and out["count"].dtype == np.int32 and out["count"].min() >= 1
    three = _fuse(cloud, min_count=3)
    full = _fuse(cloud)
    assert three["count"].min() >= 3 and np.array_equal(three["points"], full["points"][full["count"] >= 3])


def test_fused_positions_lie_inside_their_voxels_and_in_key_order(cloud):
    out = _fuse(cloud)
    key = out["sums"]["key"]
    assert (np.diff(key) > 0).all() and key.max() < 2 ** 63
    c = np.stack([(key >> 42) - fr.LIMIT, ((key >> 21) & 0x1fffff) - fr.LIMIT, (key & 0x1fffff) - fr.LIMIT], 1)
    assert (c[np.lexsort((c[:, 2], c[:, 1], c[:, 0]))] == c).all()                  # key order is (cx, cy, cz) order
    v = np.float32(cloud["voxel"])
    lo, hi = (c * v).astype(np.float32), ((c + 1) * v).astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(lo), np.abs(hi)))
    assert (out["points"] >= lo - ulp).all() and (out["points"] <= hi + ulp).all()
    assert (out["rgba"][:, 3] == 255).all() and (out["weight"] > 0).all()


def test_best_returns_rows_of_the_input(cloud):
    out = _fuse(cloud, reduce="best")
    part = fr.taking_part(cloud["points"], cloud["weight"], cloud["mask"], cloud["voxel"])[0]
    rows = {cloud["points"][i].tobytes() + cloud["rgba"][i].tobytes() + cloud["weight"][i].tobytes() for i in np.nonzero(part)[0]}
    assert len(out["points"]) == len(_fuse(cloud)["points"])
    for p, c, w in zip(out["points"], out["rgba"], out["weight"]):
        assert p.tobytes() + c.tobytes() + w.tobytes() in rows
    pts = np.full((4, 3), 0.1, np.float32) + np.arange(4, dtype=np.float32)[:, None] * np.float32(0.01)
    tie = fr.fuse(pts, weight=np.array([1, 5, 5, 2], np.float32), voxel=1.0, reduce="best")
    assert np.array_equal(tie["points"], pts[1:2]) and tie["weight"].tolist() == [5.0] and tie["count"].tolist() == [4]   # the lower row of the two 5s


def test_weights_clamp_and_missing_weights_are_ones():
    p = np.array([[0.25, 0.5, 0.75], [0.75, 0.5, 0.25]], np.float32)
    a = fr.fuse(p, voxel=1.0)
    assert a["sums"]["sw"].tolist() == [256] and a["weight"].tolist() == [1.0] and a["points"].tolist() == [[0.5, 0.5, 0.5]]
    b = fr.fuse(p, weight=np.array([1e-4, 1e9], np.float32), voxel=1.0)
    assert b["sums"]["sw"].tolist() == [1 + 32767]
    c, q, wq = fr.quantise(np.array([[-0.25, 0.0, 0.9999999]], np.float32), None, 0.25)
    assert c.tolist() == [[-1, 0, 3]] and q[0, 0] == 0 and q[0, 1] == 0 and q[0, 2] == 65535 and wq.tolist() == [128]


def test_cell_range_and_dropped():
    out = fr.fuse(np.array([[0, 0, 0], [2, 0, 0]], np.float32), voxel=1e-6)
    assert out["dropped"] == 1 and len(out["points"]) == 1                           # cell index 2e6 >= 2^20
    nan = fr.fuse(np.array([[np.nan, 0, 0], [2, 0, 0]], np.float32), voxel=1e-6)
    assert nan["dropped"] == 1 and len(nan["points"]) == 0                           # NaN is skipped silently, not counted
    empty = fr.fuse(np.zeros((0, 3), np.float32), np.zeros((0, 4), np.uint8), voxel=1.0)
    assert empty["points"].shape == (0, 3) and empty["rgba"].shape == (0, 4) and empty["count"].shape == (0,)


def test_static_part_of_the_synthetic_scene():
    """22.6 times fewer points, every one on the wall: the measurement quoted in DESIGN.md. The bound 1e-5 is 8 times the 1.3e-6 measured
    in numpy, for fp32 rounding of points at depth 4."""
    s = mr.synthetic_scene()
    static = ~s["truth"]
    voxel = 2 * np.median(s["depth"][static] / 60)
    out = fr.fuse(s["pts3d"][static], voxel=voxel)
    M = len(out["points"])
    p = out["points"].astype(np.float64)
    off = np.abs(-0.2 * p[:, 0] + p[:, 2] - 4.0).max()
    print(f"[fusion clean] voxel {voxel:.4f}: {int(static.sum())} static points -> {M} fused ({static.sum() / M:.1f} x), {off:.2e} off the plane")
    assert int(static.sum()) == 31050 and 1000 <= M <= 2000 and int(out["count"].sum()) == 31050
    assert off < 1e-5


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_fuse_symbols_agree_between_header_binding_and_library():
    from geo4d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geo4d_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.geo4d_abi_version() == _lib.ABI_VERSION == 9 == int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1))


def test_workspace_query():
    from geo4d_amd import _lib, ops
    lib = _lib.load()
    assert lib.geo4d_fuse_workspace(4096, 0) == 4096 * (8 + 64) and lib.geo4d_fuse_workspace(4096, 1) == 4096 * (8 + 16)
    assert lib.geo4d_fuse_workspace(1, 0) == 72 and lib.geo4d_fuse_workspace(1 << 32, 1) == (1 << 32) * 24
    for cap, reduce in [(0, 0), (-8, 0), (4095, 0), (6, 1), (1 << 33, 0), (4096, 2), (4096, -1)]:
        assert lib.geo4d_fuse_workspace(cap, reduce) == 0, (cap, reduce)
    assert [ops.fuse_capacity(n) for n in (0, 1, 2, 3, 4, 5, 4096, 4097)] == [1, 2, 4, 8, 8, 16, 8192, 16384]


def test_bad_arguments_are_refused_on_the_host():
    """Every refusal is -EINVAL with a message and comes before any device work: the pointers below are not device memory."""
    from geo4d_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    N, cap = 100, 128
    need = lib.geo4d_fuse_workspace(cap, 0)
    nan, inf = float("nan"), float("inf")

    def insert(points=p, N=N, voxel=0.1, reduce=0, cap=cap, dropped=p, ws=p, ws_bytes=need):
        return lib.geo4d_fuse_insert(points, None, None, None, N, voxel, reduce, cap, dropped, ws, ws_bytes, None)

    for kw in [dict(points=None), dict(dropped=None), dict(ws=None), dict(ws=p + 4), dict(N=-1), dict(N=1 << 31), dict(voxel=0.0),
               dict(voxel=-1.0), dict(voxel=nan), dict(voxel=inf), dict(cap=100), dict(cap=64), dict(cap=0), dict(reduce=2), dict(reduce=-1),
               dict(ws_bytes=need - 1)]:
        assert insert(**kw) == -22 and b"fuse_insert" in lib.geo4d_last_error(), kw
    assert insert(cap=64) == -22 and b"capacity must be >= N" in lib.geo4d_last_error()
    assert insert(cap=100) == -22 and b"power of two" in lib.geo4d_last_error()
    assert insert(reduce=2) == -22 and b"unknown reduce" in lib.geo4d_last_error()
    assert insert(ws_bytes=need - 1) == -22 and b"workspace too small" in lib.geo4d_last_error()
    assert insert(voxel=nan) == -22 and b"voxel" in lib.geo4d_last_error()
    assert insert(N=1 << 31) == -22 and b"N < 2^31" in lib.geo4d_last_error()

    def compact(cap=cap, reduce=0, keys=p, slots=p, max_pairs=N, count=p, ws=p, ws_bytes=need):
        return lib.geo4d_fuse_compact(cap, reduce, keys, slots, max_pairs, count, ws, ws_bytes, None)

    for kw in [dict(keys=None), dict(slots=None), dict(count=None), dict(max_pairs=-1), dict(ws=None), dict(ws=p + 4), dict(cap=100),
               dict(cap=0), dict(reduce=2), dict(ws_bytes=need - 1)]:
        assert compact(**kw) == -22 and b"fuse_compact" in lib.geo4d_last_error(), kw

    def finalize(order=p, M=10, points=p, rgba=None, N=N, voxel=0.1, reduce=0, cap=cap, pts=p, rgba_out=None, w=p, cnt=p, ws=p, ws_bytes=need):
        return lib.geo4d_fuse_finalize(order, M, points, rgba, None, N, voxel, reduce, cap, pts, rgba_out, w, cnt, ws, ws_bytes, None)

    for kw in [dict(order=None), dict(points=None), dict(pts=None), dict(w=None), dict(cnt=None), dict(rgba_out=p), dict(M=-1), dict(M=N + 1),
               dict(N=-1), dict(N=1 << 31), dict(voxel=0.0), dict(voxel=nan), dict(voxel=inf), dict(ws=None), dict(ws=p + 4), dict(cap=100),
               dict(cap=64), dict(reduce=2), dict(ws_bytes=need - 1)]:
        assert finalize(**kw) == -22 and b"fuse_finalize" in lib.geo4d_last_error(), kw


# ---- Python errors -----------------------------------------------------------------------------------------------------------------------
def test_fuse_points_refuses_cpu_tensors_and_bad_arguments(cloud, tmp_path):
    from geo4d_amd import _lib, fusion, ops
    from geo4d_amd.scene_export import get_3D_model_from_scene
    p = torch.from_numpy(cloud["points"])
    with pytest.raises(_lib.Geo4DNativeError):
        fusion.fuse_points(p, voxel=0.25)
    with pytest.raises(_lib.Geo4DNativeError):
        ops.fuse_points(p, voxel=0.25)
    for kw in [dict(voxel=0), dict(voxel=-0.1), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(voxel=1e-50), dict(voxel=None),
               dict(voxel=0.25, reduce="median"), dict(voxel=0.25, min_count=0), dict(voxel=0.25, min_count=1.5)]:
        with pytest.raises(ValueError):
            fusion.fuse_points(p, **kw)
    with pytest.raises(ValueError):
        fusion.fuse_scene(object(), motion="bogus")
    with pytest.raises(ValueError, match="as_pointcloud"):
        get_3D_model_from_scene(str(tmp_path), True, object(), as_pointcloud=False, fuse_voxel=0.1)
    with pytest.raises(ValueError, match="as_pointcloud"):
        get_3D_model_from_scene(str(tmp_path), True, object(), fuse_voxel=True)     # the mesh is the default export
