"""The motion rule without a GPU: its numpy restatement (tests/motion_restatement.py) on the synthetic scene the defaults were chosen
on, and the host side of the HIP path (geo4d_amd/motion.py, the three geo4d_motion_* symbols): ABI agreement, host-side argument
validation, the PNG round trip and the export's `motion` argument. tests/test_motion_gpu.py asserts the device against the same
restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import motion_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geo4d_motion_workspace", "geo4d_motion_range", "geo4d_motion_votes")


@pytest.fixture(scope="module")
def scenes():
    """The synthetic scene clean, with 2 % depth noise and with the invalid band, and the restatement's default votes of each."""
    out = {}
    for name, kw in (("clean", dict()), ("noisy", dict(noise=0.02)), ("banded", dict(band=True))):
        s = mr.synthetic_scene(**kw)
        s["views"] = mr.views_of(s["cams2world"], s["K"])
        s["votes"] = mr.votes(s["pts3d"], s["depth"], s["valid"], s["views"])
        out[name] = s
    return out


# ---- the rule on the synthetic scene -----------------------------------------------------------------------------------------------------
def test_scene_is_the_documented_one(scenes):
    s = scenes["clean"]
    assert s["pts3d"].shape == (12, 48, 64, 3) and s["pts3d"].dtype == np.float32 and s["depth"].dtype == np.float32
    assert int((~s["truth"]).sum()) == 31050 and s["truth"].any(axis=(1, 2)).all()     # the sphere shows in every frame
    # depth is camera z: every point re-projects onto its own pixel at its own depth
    for i in (0, 5, 11):
        _, _, zc, u, v = mr.project(s["pts3d"][i].reshape(-1, 3), s["views"][i])
        ys, xs = np.divmod(np.arange(48 * 64), 64)
        assert np.abs(u - xs).max() < 1e-3 and np.abs(v - ys).max() < 1e-3
        np.testing.assert_allclose(zc, s["depth"][i].reshape(-1), rtol=1e-5)
    wall = s["pts3d"][~s["truth"]].astype(np.float64)
    np.testing.assert_allclose(-0.2 * wall[:, 0] + wall[:, 2], 4.0, atol=1e-5)


def test_defaults_find_the_sphere_without_noise(scenes):
    s = scenes["clean"]
    m = mr.dynamic_mask(s["votes"], mr.DEFAULTS["min_votes"], mr.DEFAULTS["ratio"])
    iou, fp = mr.iou(m, s["truth"]), int((m & ~s["truth"]).sum())
    print(f"[motion clean] IoU {iou:.3f}, {fp} dynamic pixels off the sphere")
    assert iou >= 0.9 and fp == 0
    assert int(s["votes"][~s["truth"]][:, 1].sum()) == 0                              # static points collect no free vote at all


def test_defaults_survive_two_percent_depth_noise(scenes):
    s = scenes["noisy"]
    m = mr.dynamic_mask(s["votes"], mr.DEFAULTS["min_votes"], mr.DEFAULTS["ratio"])
    iou, fp, static = mr.iou(m, s["truth"]), int((m & ~s["truth"]).sum()), int((~s["truth"]).sum())
    print(f"[motion noisy] IoU {iou:.3f}, {fp} false positives of {static} static pixels")
    assert iou >= 0.9 and fp <= 0.002 * static
    half = mr.dynamic_mask(s["votes"], mr.DEFAULTS["min_votes"], 0.5)                 # why ratio is 0.25: the movers keep consistent votes
    assert mr.iou(half, s["truth"]) < iou


def test_invalid_pixels_neither_vote_nor_are_voted_on(scenes):
    s, c = scenes["banded"], scenes["clean"]
    assert not s["valid"][:, :, :5].any() and not s["valid"][:, 40:, :].any() and np.isnan(s["depth"][~s["valid"]]).all()
    assert (s["votes"][~s["valid"]] == 0).all() and s["votes"][s["valid"]].any()
    assert (s["votes"].sum(-1) <= c["votes"].sum(-1)).all()                           # a voter's invalid pixel casts no vote
    assert (s["votes"].sum(-1) < c["votes"].sum(-1)).any()
    dmin, dmax = mr.depth_range(s["depth"], s["valid"])                              # the range skips invalid neighbours
    assert np.isfinite(dmin[s["valid"]]).all() and np.isfinite(dmax[s["valid"]]).all()


def test_votes_count_the_voters_and_radius_limits_them(scenes):
    s = scenes["clean"]
    total = s["votes"].astype(np.int64).sum(-1)
    reach = np.array([min(11, i + 8) - max(0, i - 8) for i in range(12)])
    assert (total <= reach[:, None, None]).all() and (total.reshape(12, -1).max(1) == reach).all()
    one = mr.votes(s["pts3d"], s["depth"], s["valid"], s["views"], radius=1).astype(np.int64).sum(-1)
    assert one.max() == 2 and (one[0] <= 1).all() and (one[11] <= 1).all()
    lone = mr.votes(s["pts3d"][:1], s["depth"][:1], s["valid"][:1], s["views"][:1])
    assert lone.shape == (1, 48, 64, 3) and not lone.any()
    pair = mr.segment(s["pts3d"][:2], s["depth"][:2], s["valid"][:2], s["cams2world"][:2], s["K"][:2])
    assert not pair.any()                                                             # fewer than three images: empty masks


def test_depth_range_borders():
    d = np.arange(15, dtype=np.float32).reshape(1, 3, 5)
    v = np.ones((1, 3, 5), dtype=bool)
    v[0, 1, 1] = False
    lo, hi = mr.depth_range(d, v)
    assert lo[0, 0, 0] == 0 and hi[0, 0, 0] == 5 and hi[0, 2, 4] == 14 and lo[0, 2, 4] == 8     # (1, 1) = 6 is skipped at (0, 0)
    assert lo[0, 1, 2] == 1 and hi[0, 1, 2] == 13
    d[0, 0, 0] = np.nan
    lo, hi = mr.depth_range(d, v)
    assert lo[0, 0, 0] == 1 and hi[0, 0, 0] == 5                                      # a NaN depth never wins


def test_dynamic_mask_thresholds():
    v = np.array([[[[0, 1, 9], [0, 2, 0], [6, 2, 0], [7, 2, 0], [0, 0, 5]]]], dtype=np.uint8)
    assert mr.dynamic_mask(v, 2, 0.25).tolist() == [[[False, True, True, False, False]]]
    from geo4d_amd.motion import dynamic_mask
    assert dynamic_mask(torch.from_numpy(v), 2, 0.25).tolist() == [[[False, True, True, False, False]]]
    assert dynamic_mask(torch.from_numpy(v), 1, 0.5).tolist() == [[[True, True, False, False, False]]]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_motion_symbols_agree_between_header_binding_and_library():
    from geo4d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geo4d_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.geo4d_abi_version() == _lib.ABI_VERSION == 9 == int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1))
    assert lib.geo4d_motion_workspace(3, 40, 48) == 3 * 40 * 48 * 8
    assert lib.geo4d_motion_workspace(0, 40, 48) == 0 and lib.geo4d_motion_workspace(1 << 11, 1 << 10, 1 << 10) == 0


def test_bad_arguments_are_refused_on_the_host():
    """Every refusal is -EINVAL with a message and comes before any launch: the pointers below are not device memory."""
    from geo4d_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 1024)()
    p = ctypes.addressof(buf)
    n, H, W = 3, 4, 5
    need = lib.geo4d_motion_workspace(n, H, W)

    def rng(depth=p, valid=None, n=n, H=H, W=W, ws=p, ws_bytes=need):
        return lib.geo4d_motion_range(depth, valid, n, H, W, ws, ws_bytes, None)

    for kw in [dict(depth=None), dict(ws=None), dict(ws=p + 4), dict(n=0), dict(H=0), dict(W=-1), dict(n=1, H=1 << 16, W=1 << 15),
               dict(ws_bytes=need - 1)]:
        assert rng(**kw) == -22 and b"motion_range" in lib.geo4d_last_error(), kw

    def votes(pts=p, views=p, n=n, H=H, W=W, radius=8, tol=0.05, near=1e-3, out=p, ws=p, ws_bytes=need):
        return lib.geo4d_motion_votes(pts, views, n, H, W, radius, tol, near, out, ws, ws_bytes, None)

    for kw in [dict(pts=None), dict(views=None), dict(out=None), dict(ws=None), dict(ws=p + 4), dict(n=0), dict(H=-2), dict(W=0),
               dict(n=1, H=1 << 16, W=1 << 15), dict(radius=0), dict(radius=128), dict(radius=-1), dict(tol=0.0), dict(tol=1.0),
               dict(tol=-0.1), dict(tol=float("nan")), dict(near=-1.0), dict(near=float("nan")), dict(ws_bytes=need - 1)]:
        assert votes(**kw) == -22 and b"motion_votes" in lib.geo4d_last_error(), kw


def test_motion_votes_refuses_cpu_tensors(scenes):
    from geo4d_amd import _lib, motion
    s = scenes["clean"]
    t = torch.from_numpy
    with pytest.raises(_lib.Geo4DNativeError):
        motion.motion_votes(t(s["pts3d"]), t(s["depth"]), t(s["valid"]), t(s["cams2world"]), t(s["K"]))


# ---- host helpers ------------------------------------------------------------------------------------------------------------------------
def test_save_dynamic_masks_round_trips_through_png(tmp_path):
    from PIL import Image
    from geo4d_amd.io import save_dynamic_masks
    m = np.random.default_rng(0).uniform(size=(3, 5, 7)) < 0.4
    d = save_dynamic_masks(str(tmp_path / "m"), torch.from_numpy(m))
    assert sorted(os.listdir(d)) == ["dynamic_mask_0.png", "dynamic_mask_1.png", "dynamic_mask_2.png"]
    for i in range(3):
        im = Image.open(os.path.join(d, f"dynamic_mask_{i}.png"))
        a = np.asarray(im)
        assert im.mode == "L" and a.dtype == np.uint8 and np.array_equal(a, m[i].astype(np.uint8) * 255)
    with pytest.raises(ValueError):
        save_dynamic_masks(str(tmp_path / "bad"), m[0])


def test_export_refuses_unknown_motion(tmp_path):
    from geo4d_amd.scene_export import get_3D_model_from_scene
    with pytest.raises(ValueError):
        get_3D_model_from_scene(str(tmp_path), True, object(), motion="bogus")
