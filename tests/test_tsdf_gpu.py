"""The TSDF on the HIP path (geo4d_amd/tsdf.py + csrc/tsdf.hip) against its numpy restatement (tests/tsdf_restatement.py): exact
points, colours, weights and voxel counts on the synthetic scenes and on a small random case with every kind of pixel that takes no
part, a full table and one that is too small, determinism, the edges, and what is built on it: tsdf_scene on an aligned scene, the
export's `tsdf_voxel` and save_scene's `tsdf_static`."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import motion_restatement as mr
import tsdf_restatement as tr
from scene_cases import tiny_aligner as _aligner, truth_aligner as _synthetic_aligner

pytestmark = pytest.mark.gpu
KEYS = ("points", "rgba", "weight")


def _points(path):
    """Vertices of the POINTS primitives of a glb (0 when it holds none)."""
    data = open(path, "rb").read()
    jlen = struct.unpack("<I", data[12:16])[0]
    doc = json.loads(data[20:20 + jlen])
    return sum(doc["accessors"][p["attributes"]["POSITION"]]["count"] for m in doc["meshes"] for p in m["primitives"] if p["mode"] == 0)


def _gpu(dev, s, valid, rgba=None, weight=None, raw=False, **kw):
    """tsdf.tsdf_points on the numpy arrays of scene dict `s`; the outputs as numpy (raw: as they are)."""
    from geo4d_amd import tsdf
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = tsdf.tsdf_points(t(s["pts3d"]), t(s["depth"]), t(valid), s["cams2world"], s["K"], t(rgba), t(weight), **kw)
    torch.cuda.synchronize()
    assert out["points"].dtype == torch.float32 and out["weight"].dtype == torch.float32 and out["points"].device.type == "cuda"
    assert out["points"].dim() == 2 and out["points"].shape[1] == 3 and tuple(out["weight"].shape) == (len(out["points"]),)
    assert out["rgba"] is None or (out["rgba"].dtype == torch.uint8 and tuple(out["rgba"].shape) == (len(out["points"]), 4))
    assert out["dropped"] == 0 and out["overflow"] == 0
    if raw:
        return out
    return dict({k: None if out[k] is None else out[k].cpu().numpy() for k in KEYS}, voxels=out["voxels"])


def _ref(s, valid, rgba=None, weight=None, **kw):
    return tr.tsdf(s["pts3d"], s["depth"], valid, mr.views_of(s["cams2world"], s["K"]), tr.centres_of(s["cams2world"]), rgba, weight, **kw)


def _rows(out):
    """One bytes object per output row: position, colour and weight."""
    return [out["points"][m].tobytes() + (b"" if out["rgba"] is None else out["rgba"][m].tobytes()) + out["weight"][m].tobytes()
            for m in range(len(out["points"]))]


def _compare(tag, got, ref, s, valid, weight, **kw):
    """Exact equality of every output. A point may differ only if one of its two voxels (taken here as the cell of the point and its six
    face neighbours, which contain them) is excusable by tests/tsdf_restatement.excusable, and at most 0.05 % of the points may be
    excused; the arithmetic is correctly rounded on both sides, so the allowance should go unused. Returns the number excused."""
    a, b = _rows(got), _rows(ref)
    differ = set(a) ^ set(b)
    print(f"[tsdf {tag}] {ref['voxels']} voxels, {len(b)} points, {len(differ)} differ / excused (0 expected)")
    if not differ:
        assert got["voxels"] == ref["voxels"]
        for k in KEYS:
            assert (got[k] is None and ref[k] is None) or np.array_equal(got[k], ref[k]), (tag, k)    # the same rows in the same order
        return 0
    v = np.float32(kw["voxel"])
    ex = tr.excusable(s["pts3d"], s["depth"], valid, mr.views_of(s["cams2world"], s["K"]), tr.centres_of(s["cams2world"]), weight, ref["K"],
                      voxel=v, trunc=kw.get("trunc", 4), near=kw.get("near", 1e-3))
    cells = {tuple(c) for c in tr.cells_of(ref["K"][ex])}
    for r in differ:
        c = np.floor(np.frombuffer(r[:12], dtype=np.float32).astype(np.float64) / np.float64(v)).astype(np.int64)
        near = [tuple(c)] + [tuple(c + d * np.eye(3, dtype=np.int64)[a]) for a in range(3) for d in (-1, 1)]
        assert any(x in cells for x in near), (tag, c)
    assert len(differ) <= 5e-4 * len(b) and abs(got["voxels"] - ref["voxels"]) <= len(differ)
    return len(differ)


@pytest.fixture(scope="module")
def scenes():
    """The clean, the noisy and the invalid-band synthetic scene (12 x 48 x 64) with their static parts, colours and the restatement's
    result at the defaults, computed once."""
    return dict(clean=tr.static_scene(0.0), noisy=tr.static_scene(0.02), band=tr.static_scene(0.0, band=True))


# ---- 1. device against restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["clean", "noisy", "band"])
def test_synthetic_scenes_match_the_restatement(dev, scenes, which):
    s = scenes[which]
    ref = s["out"]
    assert ref["dropped"] == 0 and ref["voxels"] > 5000 and len(ref["points"]) > 500
    got = _gpu(dev, s, s["static"], s["rgba"], voxel=s["voxel"])
    _compare(which, got, ref, s, s["static"], None, voxel=s["voxel"])


def _random_case():
    """3 images of 5 x 7 on the synthetic cameras: a third of the pixels invalid, NaN / inf depths and points, zero / negative / NaN / inf
    weights, random colours."""
    g = np.random.default_rng(21)
    s = mr.synthetic_scene(noise=0.01, n=3, H=5, W=7)
    valid = g.uniform(size=(3, 5, 7)) > 1 / 3
    depth, pts = s["depth"].copy(), s["pts3d"].copy()
    depth[0, 0, 0], depth[1, 2, 3], depth[2, 4, 6], depth[2, 1, 1] = np.nan, np.inf, -np.inf, -1.0
    pts[0, 1, 2, 0], pts[1, 3, 4, 1], pts[2, 0, 5, 2] = np.nan, np.inf, -np.inf
    valid[0, 0, 0] = valid[1, 2, 3] = valid[2, 4, 6] = valid[2, 1, 1] = valid[0, 1, 2] = valid[1, 3, 4] = valid[2, 0, 5] = True
    w = g.uniform(0.25, 3.0, size=(3, 5, 7)).astype(np.float32)
    w[0, 2, 2], w[1, 1, 5], w[2, 3, 3], w[0, 4, 1], w[1, 0, 6] = 0.0, -1.5, np.nan, np.inf, -0.0
    valid[0, 2, 2] = valid[1, 1, 5] = valid[2, 3, 3] = valid[0, 4, 1] = valid[1, 0, 6] = True
    s.update(depth=depth, pts3d=pts, valid=valid, weight=w, rgba=g.integers(0, 256, size=(3, 5, 7, 4), dtype=np.uint8))
    return s


@pytest.mark.parametrize("colours", [False, True])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("trunc", [1, 8])
def test_random_case_matches_the_restatement(dev, trunc, weights, colours):
    s = _random_case()
    assert 20 < s["valid"].sum() < 85
    rgba, w = s["rgba"] if colours else None, s["weight"] if weights else None
    kw = dict(voxel=0.11, trunc=trunc, min_weight=1.0)
    ref = _ref(s, s["valid"], rgba, w, **kw)
    assert ref["dropped"] == 0 and ref["voxels"] > (50 if trunc == 1 else 300) and len(ref["points"]) > 10 and (ref["rgba"] is None) == (not colours)
    got = _gpu(dev, s, s["valid"], rgba, w, capacity=4096, **kw)                    # at T = 8 more voxels than 4 x the pixels
    _compare(f"random T={trunc} weights={weights} colours={colours}", got, ref, s, s["valid"], w, **kw)


def test_min_weight_is_inclusive(dev, scenes):
    """min_weight = 9 with unit weights: voxels seen by exactly 9 images are live."""
    s = scenes["clean"]
    ref = _ref(s, s["static"], voxel=s["voxel"], min_weight=9.0)
    assert (ref["Wt"] == 9.0).any() and ref["weight"].min() == 9.0 and 0 < len(ref["points"]) < len(s["out"]["points"])
    got = _gpu(dev, s, s["static"], voxel=s["voxel"], min_weight=9.0)
    _compare("min_weight 9", got, ref, s, s["static"], None, voxel=s["voxel"])
    assert got["weight"].min() == 9.0 and got["rgba"] is None


# ---- 2. table edges ----------------------------------------------------------------------------------------------------------------------
def test_exactly_full_table_and_one_too_small(dev):
    """128 marked voxels: capacity 128 is load factor 1 (long probe chains, wrap-around) and gives the default's output; capacity 64
    cannot hold them: every probe ends, the host refuses. Nothing faults: a full table is an ordinary input."""
    from geo4d_amd import ops
    s = mr.synthetic_scene(n=3, H=5, W=7)
    kw = dict(voxel=np.float32(0.0785), trunc=1, min_weight=1.0)
    ref = _ref(s, s["valid"], **kw)
    assert ref["voxels"] == 128 and len(ref["points"]) > 20
    default = _gpu(dev, s, s["valid"], **kw)
    full = _gpu(dev, s, s["valid"], capacity=128, **kw)
    _compare("default capacity", default, ref, s, s["valid"], None, **kw)
    _compare("capacity = voxels", full, ref, s, s["valid"], None, **kw)
    with pytest.raises(ops.TsdfTableFull, match=r"overflow = \d+ > 0.*capacity = 64; pass capacity >= \d+"):
        _gpu(dev, s, s["valid"], capacity=64, **kw)
    again = _gpu(dev, s, s["valid"], capacity=256, **kw)                            # and the next call is unharmed
    _compare("after the refusal", again, ref, s, s["valid"], None, **kw)


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_three_capacities_are_equal(dev, scenes):
    s = scenes["noisy"]
    cap = tr.default_capacity(int(s["static"].sum()))
    runs = [_gpu(dev, s, s["static"], s["rgba"], raw=True, voxel=s["voxel"], capacity=c) for c in (None, None, cap, 2 * cap, 4 * cap)]
    assert len(runs[0]["points"]) > 1000
    for r in runs[1:]:
        assert r["voxels"] == runs[0]["voxels"]
        for k in KEYS:
            assert torch.equal(r[k], runs[0][k]), k


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------------
def test_one_image_thin_images_and_nothing_valid(dev):
    from geo4d_amd import tsdf
    for n, H, W in ((1, 6, 9), (3, 1, 9), (3, 6, 1), (2, 1, 1)):
        s = mr.synthetic_scene(n=n, H=H, W=W)
        rgba = np.random.default_rng(n).integers(0, 256, size=(n, H, W, 4), dtype=np.uint8)
        kw = dict(voxel=0.09, trunc=2, min_weight=1.0)
        ref = _ref(s, s["valid"], rgba, **kw)
        assert ref["voxels"] > 0 and (len(ref["points"]) > 0 or H * W == 1)
        capacity = 16 if H * W == 1 else None                                       # 2 pixels mark 10 voxels: the default table of 8 is refused
        _compare(f"{n} x {H} x {W}", _gpu(dev, s, s["valid"], rgba, capacity=capacity, **kw), ref, s, s["valid"], None, **kw)
    none = np.zeros_like(s["valid"])
    for capacity in (None, 64):                                                     # no table at all / an empty table: no launch with zero blocks
        out = _gpu(dev, s, none, rgba, capacity=capacity, **kw)
        assert out["points"].shape == (0, 3) and out["rgba"].shape == (0, 4) and out["weight"].shape == (0,) and out["voxels"] == 0
    assert _gpu(dev, s, none, **kw)["rgba"] is None
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    assert _ref(s, s["valid"], voxel=1e-6, trunc=1)["dropped"] == 2 * 5                # cell index 4e6 >= 2^20 for every sample
    with pytest.raises(ValueError, match=r"\b10 sample\(s\) lie outside the voxel grid"):
        tsdf.tsdf_points(t(s["pts3d"]), t(s["depth"]), t(s["valid"]), s["cams2world"], s["K"], voxel=1e-6, trunc=1)


# ---- 5. the scene level ------------------------------------------------------------------------------------------------------------------
def _scene_ref(a, msk, voxel, weight=None, **kw):
    """The restatement fed the scene's own arrays."""
    from geo4d_amd.scene_view import scene_cameras
    c2w, K = scene_cameras(a)
    imgs = a.imgs.float().cpu().numpy()
    u8 = np.concatenate([np.clip(imgs * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8), np.full((*imgs.shape[:3], 1), 255, np.uint8)], -1)
    valid = np.ones((a.n, a.H, a.W), bool) if msk is None else msk
    s = dict(pts3d=a.get_pts3d().detach().cpu().numpy(), depth=a.get_depthmaps().detach().cpu().numpy(), cams2world=c2w.numpy(), K=K.numpy())
    return _ref(s, valid, u8, weight, voxel=voxel, **kw), s, valid


def _as_numpy(out):
    return dict({k: None if out[k] is None else out[k].cpu().numpy() for k in KEYS}, voxels=out["voxels"])


def test_tsdf_scene_on_the_tiny_aligned_scene(dev):
    import fusion_restatement as fr
    from geo4d_amd import tsdf
    a = _aligner(dev)
    assert a.tsdf is None
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    thr = float(a.im_conf.median())
    depth, focal = a.get_depthmaps().detach().cpu().numpy(), a.get_focals().detach().cpu().numpy().reshape(-1)
    conf = a.get_conf().detach().cpu().numpy()
    for motion in (None, "static"):
        for use_conf in (False, True):
            got = tsdf.tsdf_scene(a, motion=motion, min_conf_thr=thr, min_weight=1.0, trunc=2, use_conf=use_conf)
            assert got is a.tsdf
            msk = a.get_masks().cpu().numpy()
            if motion is not None:
                msk = msk & ~a.dynamic_masks.cpu().numpy()
            voxel = fr.default_voxel(depth, focal, msk)
            assert got["voxel"] == float(np.float32(voxel))
            ref, s, valid = _scene_ref(a, msk, voxel, conf if use_conf else None, min_weight=1.0, trunc=2)
            assert ref["dropped"] == 0 and ref["voxels"] > 0
            _compare(f"tiny scene motion={motion} use_conf={use_conf}", _as_numpy(got), ref, s, valid, conf if use_conf else None, voxel=voxel, trunc=2)
    with pytest.raises(ValueError, match="moving part has no TSDF"):
        tsdf.tsdf_scene(a, motion="dynamic")


def test_tsdf_scene_denoises_the_synthetic_aligner(dev):
    """The noisy synthetic scene through a GroupAligner: equal to the restatement fed the aligner's own arrays for motion None and
    "static", and for the static part the same bound as tests/test_tsdf_cpu.py: RMS distance to the wall at most half the raw points'."""
    from geo4d_amd import tsdf
    s0 = mr.synthetic_scene(noise=0.02)
    a = _synthetic_aligner(dev, s0)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(5)).to(dev)
    dist = lambda p: np.abs(-0.2 * p[:, 0].astype(np.float64) + p[:, 2] - 4.0) / np.sqrt(1.04)
    for motion in (None, "static"):
        got = tsdf.tsdf_scene(a, motion=motion, is_msk=False)
        msk = None if motion is None else ~a.dynamic_masks.cpu().numpy()
        ref, s, valid = _scene_ref(a, msk, got["voxel"])
        assert len(ref["points"]) > 1000
        _compare(f"synthetic aligner motion={motion}", _as_numpy(got), ref, s, valid, None, voxel=got["voxel"])
    d, raw = dist(got["points"].cpu().numpy()), dist(s["pts3d"][valid])
    rms = lambda x: float(np.sqrt((x[x < 0.5] ** 2).mean()))
    print(f"[tsdf synthetic aligner] RMS {rms(d):.4f} against {rms(raw):.4f} raw, {(d >= 0.5).sum()} of {len(d)} far")
    assert rms(d) <= 0.5 * rms(raw) and (d >= 0.5).sum() <= 0.01 * len(d)


def test_export_and_save_scene_write_the_surface_points(dev, tmp_path):
    """tsdf_voxel=None is today's glb byte for byte; with a voxel the glb holds the P surface points. save_scene(tsdf_static=True) writes
    <seq>_static_tsdf.glb and nothing else, and every other file stays byte-identical."""
    from geo4d_amd import scene_export
    s0 = mr.synthetic_scene(noise=0.02)
    a = _synthetic_aligner(dev, s0)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    kw = dict(as_pointcloud=True)
    plain = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="plain", **kw)
    none = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="none", tsdf_voxel=None, **kw)
    assert a.tsdf is None and open(plain, "rb").read() == open(none, "rb").read()
    for name, tsdf_voxel, motion in (("auto", True, None), ("static", True, "static"), ("fixed", None, None)):
        if name == "fixed":
            tsdf_voxel = 1.5 * a.tsdf["voxel"]
        path = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name=name, tsdf_voxel=tsdf_voxel, motion=motion, **kw)
        P = len(a.tsdf["points"])
        assert 0 < P < _points(plain) and _points(path) == P, name
        assert name != "fixed" or a.tsdf["voxel"] == float(np.float32(tsdf_voxel))
    with pytest.raises(ValueError, match="fuse_voxel and tsdf_voxel"):
        scene_export.get_3D_model_from_scene(str(tmp_path), True, a, fuse_voxel=0.05, tsdf_voxel=0.05, **kw)
    b = _synthetic_aligner(dev, s0)
    video = torch.rand((1, 3, b.n, b.H, b.W), generator=torch.Generator().manual_seed(6)) * 2 - 1
    base = scene_export.save_scene(b, str(tmp_path / "base"), "seq", imgs=video)
    assert b.dynamic_masks is None and b.tsdf is None
    full = scene_export.save_scene(b, str(tmp_path / "full"), "seq", imgs=video, tsdf_static=True)
    names = sorted(os.listdir(base))
    assert sorted(os.listdir(full)) == sorted(names + ["seq_static_tsdf.glb"])
    for f in names:
        assert open(os.path.join(base, f), "rb").read() == open(os.path.join(full, f), "rb").read(), f
    assert b.dynamic_masks is not None                                              # it segmented motion first
    assert 0 < _points(os.path.join(full, "seq_static_tsdf.glb")) == len(b.tsdf["points"])
