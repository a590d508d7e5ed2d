"""The TSDF rule without a GPU: its numpy restatement (tests/tsdf_restatement.py) on the synthetic scene of tests/motion_restatement.py
(what it denoises, and the properties the rule promises), and the host side of the HIP path (geo4d_amd/tsdf.py, the geo4d_tsdf_*
symbols): ABI agreement, host-side argument validation and the Python errors. tests/test_tsdf_gpu.py asserts the device against the
same restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import motion_restatement as mr
import tsdf_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geo4d_tsdf_workspace", "geo4d_tsdf_mark", "geo4d_tsdf_compact", "geo4d_tsdf_integrate", "geo4d_tsdf_count", "geo4d_tsdf_write")
KEYS = ("points", "rgba", "weight")


@pytest.fixture(scope="module")
def noisy():
    return tr.static_scene(0.02)


@pytest.fixture(scope="module")
def clean():
    return tr.static_scene(0.0)


def off_plane(p):
    """Distance of points [N, 3] to the wall -0.2 x + z = 4."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return np.abs(-0.2 * p[:, 0] + p[:, 2] - 4.0) / np.sqrt(1.04)


def rms_near(p):
    """(RMS distance to the wall over the points within 0.5 of it, how many are farther, how many there are)."""
    d = off_plane(p)
    return float(np.sqrt((d[d < 0.5] ** 2).mean())), int((d >= 0.5).sum()), len(d)


# ---- what it denoises ----------------------------------------------------------------------------------------------------------------------
def test_noisy_wall_is_denoised_to_half_or_better(noisy):
    """The surface points' RMS distance to the wall must be at most half the raw static points' (both over the points within 0.5 of
    it); points farther than 0.5, which come from sphere pixels left in the static part, at most 1 % of the output. Measured here:
    0.0250 against 0.0789 raw (0.32 x), 2 of 1 389 points far."""
    out = noisy["out"]
    got, far, P = rms_near(out["points"])
    raw, raw_far, N = rms_near(noisy["pts3d"][noisy["static"]])
    print(f"[tsdf noisy] voxel {noisy['voxel']:.4f}: {N} static pixels ({raw_far} far) -> {out['voxels']} voxels -> {P} points; RMS {got:.4f} "
          f"against {raw:.4f} raw ({got / raw:.2f} x), {far} far")
    assert N > 30000 and P > 1000 and out["dropped"] == 0
    assert got <= 0.5 * raw
    assert far <= 0.01 * P


def test_clean_wall_has_no_far_point(clean):
    """Without noise no point may lie farther than 0.5 from the wall. Measured: RMS 0.0017, 0 of 1 095 far."""
    got, far, P = rms_near(clean["out"]["points"])
    print(f"[tsdf clean] {clean['out']['voxels']} voxels -> {P} points; RMS {got:.4f}, {far} far")
    assert P > 800 and far == 0 and got < 0.01


# ---- properties of the rule --------------------------------------------------------------------------------------------------------------
def test_every_point_lies_between_its_two_voxel_centres(noisy):
    out, v = noisy["out"], np.float32(noisy["voxel"])
    X = tr.voxel_centres(out["K"], v)
    a, b, p = X[out["m"]], X[out["m2"]], out["points"]
    rows = np.arange(len(p))
    assert len(p) > 1000 and (np.diff(out["K"]) > 0).all()
    assert (tr.cells_of(out["K"][out["m2"]]) - tr.cells_of(out["K"][out["m"]]) == np.eye(3, dtype=np.int64)[out["axis"]]).all()
    other = np.ones_like(p, dtype=bool)
    other[rows, out["axis"]] = False
    assert (p[other] == a[other]).all()                                             # the centre's own coordinates, bit for bit
    ulp = np.spacing(np.abs(b[rows, out["axis"]]))
    assert (p[rows, out["axis"]] >= a[rows, out["axis"]]).all() and (p[rows, out["axis"]] <= b[rows, out["axis"]] + ulp).all()
    order = out["m"] * 3 + out["axis"]
    assert (np.diff(order) > 0).all()                                               # rows in (m, a) order
    live = tr.live_of(out["f"], out["Wt"], 4.0)
    assert live[out["m"]].all() and live[out["m2"]].all() and ((out["f"][out["m"]] >= 0) != (out["f"][out["m2"]] >= 0)).all()
    assert (out["weight"] >= 4).all() and (out["rgba"][:, 3] == 255).all()


def test_output_voxels_are_marked_and_capacity_changes_nothing(noisy):
    s = noisy
    keys, dropped = tr.mark_keys(s["pts3d"], s["depth"], s["static"], s["centres"], s["voxel"], 4, 1e-3)
    assert dropped == 0 and set(s["out"]["K"].tolist()) == set(keys.tolist())
    taking = int(tr.taking_part(s["pts3d"], s["depth"], s["static"], 1e-3).sum())
    assert taking == int(s["static"].sum())
    cap = tr.default_capacity(taking)
    assert cap == 131072 and [tr.default_capacity(k) for k in (0, 1, 2, 64, 65)] == [1, 4, 8, 256, 512]
    kw = dict(voxel=s["voxel"])
    a = tr.tsdf(s["pts3d"], s["depth"], s["static"], s["views"], s["centres"], s["rgba"], capacity=cap, **kw)
    b = tr.tsdf(s["pts3d"], s["depth"], s["static"], s["views"], s["centres"], s["rgba"], capacity=2 * cap, **kw)
    for got in (a, b):
        assert got["overflow"] == 0 and got["voxels"] == s["out"]["voxels"]
        for k in KEYS + ("K", "f", "Wt"):
            assert np.array_equal(got[k], s["out"][k], equal_nan=True), k
    some = keys[np.isin(keys, np.unique(keys)[:300])]                               # 300 voxels into 256 slots: the probe ends, overflow > 0
    full, overflow = tr.table_insert(some, 256)
    assert len(full) == 256 and overflow >= 44 and set(full.tolist()) < set(some.tolist())
    roomy, none = tr.table_insert(some, 512)
    assert none == 0 and np.array_equal(roomy, np.unique(some))


def test_weights_colours_and_min_weight(clean):
    """Unit weights: Wt counts the images; halving every weight halves Wt and leaves f and the points alone; min_weight is inclusive."""
    s, out = clean, clean["out"]
    assert (out["Wt"] == np.round(out["Wt"])).all() and out["Wt"].max() <= s["n"]
    half = tr.tsdf(s["pts3d"], s["depth"], s["static"], s["views"], s["centres"], s["rgba"], np.full(s["depth"].shape, 0.5, np.float32),
                   voxel=s["voxel"], min_weight=2.0)
    assert np.array_equal(half["points"], out["points"]) and np.array_equal(half["rgba"], out["rgba"])
    assert np.array_equal(half["weight"] * 2, out["weight"]) and np.array_equal(half["f"], out["f"], equal_nan=True)
    more = tr.tsdf(s["pts3d"], s["depth"], s["static"], s["views"], s["centres"], voxel=s["voxel"], min_weight=9.0)
    assert more["rgba"] is None and 0 < len(more["points"]) < len(out["points"]) and more["weight"].min() == 9.0
    none = tr.tsdf(s["pts3d"], s["depth"], np.zeros_like(s["static"]), s["views"], s["centres"], s["rgba"], voxel=s["voxel"])
    assert none["voxels"] == 0 and none["points"].shape == (0, 3) and none["weight"].shape == (0,)


def test_out_of_range_samples_are_dropped():
    s = mr.synthetic_scene(n=2, H=4, W=5)
    views, centres = mr.views_of(s["cams2world"], s["K"]), tr.centres_of(s["cams2world"])
    out = tr.tsdf(s["pts3d"], s["depth"], s["valid"], views, centres, voxel=1e-6, trunc=1, min_weight=1.0)
    assert out["dropped"] == 2 * 4 * 5 * 5 and out["voxels"] == 0                  # z / v = 4e6 >= 2^20 for every sample


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_tsdf_symbols_agree_between_header_binding_and_library():
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
    assert lib.geo4d_tsdf_workspace(4096) == 4096 * 8 and lib.geo4d_tsdf_workspace(1) == 8 and lib.geo4d_tsdf_workspace(1 << 32) == 8 << 32
    for cap in (0, -8, 4095, 6, 1 << 33):
        assert lib.geo4d_tsdf_workspace(cap) == 0, cap
    assert [ops.tsdf_capacity(k) for k in (0, 1, 2, 64, 65)] == [tr.default_capacity(k) for k in (0, 1, 2, 64, 65)] == [1, 4, 8, 256, 512]


def test_bad_arguments_are_refused_on_the_host():
    """Every refusal is -EINVAL with a message and comes before any device work: the pointers below are not device memory."""
    from geo4d_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    nan, inf = float("nan"), float("inf")

    def mark(pts=p, depth=p, centres=p, n=2, H=4, W=5, voxel=0.1, T=4, near=1e-3, cap=128, counters=p, ws=p, ws_bytes=1024):
        return lib.geo4d_tsdf_mark(pts, depth, None, centres, n, H, W, voxel, T, near, cap, counters, ws, ws_bytes, None)

    for kw in [dict(pts=None), dict(depth=None), dict(centres=None), dict(counters=None), dict(ws=None), dict(ws=p + 4), dict(n=0), dict(H=0),
               dict(W=-1), dict(n=1 << 11, H=1 << 10, W=1 << 10), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan), dict(voxel=inf), dict(T=0),
               dict(T=9), dict(T=-4), dict(near=-1.0), dict(near=nan), dict(cap=100), dict(cap=0), dict(cap=1 << 33), dict(ws_bytes=1023)]:
        assert mark(**kw) == -22 and b"tsdf_mark" in lib.geo4d_last_error(), kw
    assert mark(T=9) == -22 and b"1 .. 8" in lib.geo4d_last_error()
    assert mark(cap=100) == -22 and b"power of two" in lib.geo4d_last_error()
    assert mark(ws_bytes=1023) == -22 and b"workspace too small" in lib.geo4d_last_error()
    assert mark(voxel=nan) == -22 and b"voxel" in lib.geo4d_last_error()

    def compact(cap=128, keys=p, max_keys=128, count=p, ws=p, ws_bytes=1024):
        return lib.geo4d_tsdf_compact(cap, keys, max_keys, count, ws, ws_bytes, None)

    for kw in [dict(keys=None), dict(count=None), dict(max_keys=-1), dict(ws=None), dict(ws=p + 4), dict(cap=100), dict(cap=0), dict(ws_bytes=1023)]:
        assert compact(**kw) == -22 and b"tsdf_compact" in lib.geo4d_last_error(), kw

    def integrate(keys=p, M=10, depth=p, rgba=None, views=p, n=2, H=4, W=5, voxel=0.1, T=4, near=1e-3, f=p, wt=p, rgba_out=None):
        return lib.geo4d_tsdf_integrate(keys, M, depth, None, None, rgba, views, n, H, W, voxel, T, near, f, wt, rgba_out, None)

    for kw in [dict(keys=None), dict(depth=None), dict(views=None), dict(f=None), dict(wt=None), dict(rgba_out=p), dict(M=-1), dict(M=1 << 31),
               dict(n=0), dict(H=0), dict(W=0), dict(voxel=0.0), dict(voxel=nan), dict(voxel=inf), dict(T=0), dict(T=9), dict(near=-0.5)]:
        assert integrate(**kw) == -22 and b"tsdf_integrate" in lib.geo4d_last_error(), kw

    def count(keys=p, M=10, f=p, wt=p, min_weight=4.0, counts=p):
        return lib.geo4d_tsdf_count(keys, M, f, wt, min_weight, counts, None)

    for kw in [dict(keys=None), dict(f=None), dict(wt=None), dict(counts=None), dict(M=-1), dict(M=1 << 31), dict(min_weight=0.0),
               dict(min_weight=-1.0), dict(min_weight=nan)]:
        assert count(**kw) == -22 and b"tsdf_count" in lib.geo4d_last_error(), kw

    def write(keys=p, M=10, f=p, wt=p, rgba=None, first=p, P=5, voxel=0.1, min_weight=4.0, pts=p, rgba_out=None, w=p):
        return lib.geo4d_tsdf_write(keys, M, f, wt, rgba, first, P, voxel, min_weight, pts, rgba_out, w, None)

    for kw in [dict(keys=None), dict(f=None), dict(wt=None), dict(first=None), dict(pts=None), dict(w=None), dict(rgba_out=p), dict(M=-1),
               dict(P=-1), dict(P=31), dict(voxel=0.0), dict(voxel=nan), dict(min_weight=0.0), dict(min_weight=nan)]:
        assert write(**kw) == -22 and b"tsdf_write" in lib.geo4d_last_error(), kw


# ---- Python errors -----------------------------------------------------------------------------------------------------------------------
def test_tsdf_points_refuses_cpu_tensors_and_bad_arguments(tmp_path):
    from geo4d_amd import _lib, ops, tsdf
    from geo4d_amd.scene_export import get_3D_model_from_scene
    s = mr.synthetic_scene(n=2, H=4, W=5)
    args = [torch.from_numpy(s["pts3d"]), torch.from_numpy(s["depth"]), torch.from_numpy(s["valid"]), s["cams2world"], s["K"]]
    with pytest.raises(_lib.Geo4DNativeError, match="only on a HIP device"):
        tsdf.tsdf_points(*args, voxel=0.1)
    with pytest.raises(_lib.Geo4DNativeError):
        ops.tsdf_points(args[0], args[1], args[2], torch.zeros(2, 16), torch.zeros(2, 3), voxel=0.1)
    for kw, msg in [(dict(voxel=0.1, trunc=0), r"trunc must be an integer number of voxels in 1\.\.8"),
                    (dict(voxel=0.1, trunc=9), r"trunc must be an integer number of voxels in 1\.\.8"),
                    (dict(voxel=0.1, trunc=2.5), r"trunc must be an integer"),
                    (dict(voxel=0.1, min_weight=0), "min_weight must be > 0"), (dict(voxel=0.1, min_weight=-1.0), "min_weight must be > 0"),
                    (dict(voxel=float("nan")), "voxel must be finite and > 0"), (dict(voxel=float("inf")), "voxel must be finite and > 0"),
                    (dict(voxel=0), "voxel must be finite and > 0"), (dict(voxel=1e-50), "voxel must be finite and > 0"),
                    (dict(voxel=None), "voxel must be finite and > 0"), (dict(voxel=0.1, near=-1), "near must be >= 0"),
                    (dict(voxel=0.1, capacity=100), "capacity must be a power of two"), (dict(voxel=0.1, capacity=0), "capacity must be a power of two")]:
        with pytest.raises(ValueError, match=msg):
            tsdf.tsdf_points(*args, **kw)                                           # before the device is asked for
    with pytest.raises(ValueError, match="moving part has no TSDF"):
        tsdf.tsdf_scene(object(), motion="dynamic")
    with pytest.raises(ValueError, match="trunc must be"):
        tsdf.tsdf_scene(object(), trunc=12)
    with pytest.raises(ValueError, match="fuse_voxel and tsdf_voxel"):
        get_3D_model_from_scene(str(tmp_path), True, object(), as_pointcloud=True, fuse_voxel=0.1, tsdf_voxel=0.1)
    with pytest.raises(ValueError, match="tsdf_voxel.*as_pointcloud"):
        get_3D_model_from_scene(str(tmp_path), True, object(), tsdf_voxel=True)      # the mesh is the default export
    with pytest.raises(ValueError, match="moving part has no TSDF"):
        get_3D_model_from_scene(str(tmp_path), True, object(), as_pointcloud=True, motion="dynamic", tsdf_voxel=True)
