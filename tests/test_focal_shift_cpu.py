"""Shift / focal recovery without a GPU (geo4d_amd/geometry.py, ops.focal_shift, csrc/focal_shift.hip): the two C ABI entry points in
the header and the ctypes table, argument errors raised before any device work, the closed-form helpers against the reference's values
stored in tests/golden/prefix_init.pt (generate_prefix_init.py), and the outlier filter of pose_init="prefix" against the reference's."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("geo4d_focal_shift_workspace", "geo4d_focal_shift")


@pytest.fixture(scope="module")
def fix():
    return torch.load(os.path.join(ROOT, "tests", "golden", "prefix_init.pt"), weights_only=False)


def test_header_and_ctypes_table_agree_on_the_new_symbols():
    from geo4d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geo4d_hip.h")).read()
    assert int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 9     # symbols added, no struct changed
    lib = _lib.load()
    for name in NEW:
        m = re.search(r"\b(size_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/geo4d_hip.h"
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(m.group(2).split(",")), (name, m.group(2))
        assert (res is _lib.C.c_size_t) == (m.group(1) == "size_t")
        assert hasattr(lib, name)
    # per map 10 state doubles + 9 sums per 4096-pixel chunk (at most 64 chunks)
    assert lib.geo4d_focal_shift_workspace(1, 3, 5) == (10 + 9) * 8
    assert lib.geo4d_focal_shift_workspace(30, 320, 512) == 30 * (10 + 9 * 40) * 8
    assert lib.geo4d_focal_shift_workspace(2, 4096, 4096) == 2 * (10 + 9 * 64) * 8
    assert lib.geo4d_focal_shift_workspace(0, 8, 8) == 0


def test_argument_errors_come_before_any_device_work():
    from geo4d_amd import _lib, ops
    lib = _lib.load()
    buf = (_lib.C.c_double * 64)()
    p = _lib.C.addressof(buf)
    good = dict(points=p, ms=24, weight=None, ws_=0, thr=0.5, zoff=None, B=1, H=2, W=4, h=2, w=4, iters=8, shift=p, focal=p, status=p, ws=p, nbytes=512)

    def call(**kw):
        a = dict(good, **kw)
        return lib.geo4d_focal_shift(a["points"], a["ms"], a["weight"], a["ws_"], a["thr"], a["zoff"], a["B"], a["H"], a["W"], a["h"], a["w"], a["iters"],
                                     a["shift"], a["focal"], a["status"], a["ws"], a["nbytes"], None)
    for bad in (dict(points=None), dict(shift=None), dict(focal=None), dict(status=None), dict(ws=None), dict(B=0), dict(B=70000), dict(H=0), dict(w=0),
                dict(iters=0), dict(thr=float("nan")), dict(nbytes=(10 + 9) * 8 - 1), dict(ws=p + 4)):
        assert call(**bad) == -22 and b"focal_shift" in lib.geo4d_last_error(), bad
    pts = torch.zeros(2, 4, 6, 3)
    with pytest.raises(_lib.Geo4DNativeError):
        ops.focal_shift(pts)
    from geo4d_amd import geometry
    with pytest.raises(_lib.Geo4DNativeError):
        geometry.point_map_to_depth(pts, torch.ones(2, 4, 6, dtype=torch.bool))
    with pytest.raises(_lib.Geo4DNativeError):
        geometry.recover_focal_pixels(pts, None, (4, 6))


def test_image_plane_uv_and_intrinsics_against_the_reference(fix):
    from geo4d_amd import geometry
    for (W, H, ar), ref in fix["uv"].items():
        got = geometry.image_plane_uv(W, H, aspect_ratio=ar, dtype=torch.float32)
        assert got.shape == ref.shape == (H, W, 2)
        assert float((got - ref).abs().max()) <= 1e-7, (W, H, ar)
    # the solver's in-kernel formula: u_x = (2 x - (W - 1)) / diagonal, v_y = (2 y - (H - 1)) / diagonal
    ref = fix["uv"][(32, 24, None)].double()
    d = (32 ** 2 + 24 ** 2) ** 0.5
    u = (2 * torch.arange(32, dtype=torch.float64) - 31) / d
    v = (2 * torch.arange(24, dtype=torch.float64) - 23) / d
    assert float((ref[..., 0] - u[None, :]).abs().max()) < 2e-7 and float((ref[..., 1] - v[:, None]).abs().max()) < 2e-7
    i = fix["intrinsics"]
    K = geometry.intrinsics_from_fov_xy(i["fov_x"], i["fov_y"])
    assert K.shape == i["K"].shape and float((K - i["K"]).abs().max()) <= 1e-6
    K1 = geometry.intrinsics_from_fov_xy(i["fov_x"][1], i["fov_y"][1])
    assert K1.shape == (3, 3) and torch.equal(K1, K[1])
    got = geometry.focal_pixels_from_fov(i["fov_x"], i["fov_y"], 24, 32)
    assert torch.allclose(got, (i["K"][:, 0, 0] * 32 + i["K"][:, 1, 1] * 24) / 2, rtol=1e-6)


def _filter_numpy(f):
    f = np.asarray(f, np.float32).copy()
    mean = f[f > 30].mean(dtype=np.float32)
    f[np.abs(f - mean) / mean > np.float32(0.6)] = mean
    return f


def test_outlier_filter_against_the_reference(fix):
    from geo4d_amd.align import filter_outlier_focals
    for key in ("prefix", "outlier"):
        before, after = fix[key]["focal_group_before"], fix[key]["focal_group_after"]
        got, _ = filter_outlier_focals(before)
        assert np.allclose(_filter_numpy(before.numpy()), after.numpy(), rtol=1e-6, atol=0), key
        assert torch.allclose(got, after, rtol=1e-6, atol=0), key
        assert torch.equal(before, fix[key]["focal_group_before"])                         # the input is not modified
    o = fix["outlier"]
    assert float(o["focal_group_after"][o["window"]]) != float(o["focal_group_before"][o["window"]])
    assert torch.equal(fix["prefix"]["focal_group_after"], fix["prefix"]["focal_group_before"])
    # the mean is taken over focals above 30 only; with none above, nothing is replaced (NaN compares false), as in the reference
    got, mean = filter_outlier_focals(torch.tensor([10.0, 20.0, 25.0]))
    assert torch.isnan(mean) and torch.equal(got, torch.tensor([10.0, 20.0, 25.0]))
