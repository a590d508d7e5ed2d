"""The fusion on the HIP path (geo4d_amd/fusion.py + csrc/fuse.hip) against its numpy restatement (tests/fusion_restatement.py): exact
positions, colours, weights and counts on a random cloud with every kind of row that takes no part, a full hash table, one hot voxel,
order independence and determinism, the edges, and what is built on it: fuse_scene on an aligned scene, the export's `fuse_voxel` and
save_scene's `fuse_static`."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import fusion_restatement as fr
import motion_restatement as mr
from scene_cases import tiny_aligner as _aligner, truth_aligner as _synthetic_aligner

pytestmark = pytest.mark.gpu
KEYS = ("points", "rgba", "weight", "count")


def _points(path):
    """Vertices of the POINTS primitives of a glb (0 when it holds none)."""
    data = open(path, "rb").read()
    jlen = struct.unpack("<I", data[12:16])[0]
    doc = json.loads(data[20:20 + jlen])
    return sum(doc["accessors"][p["attributes"]["POSITION"]]["count"] for m in doc["meshes"] for p in m["primitives"] if p["mode"] == 0)


def _gpu(dev, points, rgba=None, weight=None, mask=None, **kw):
    """fusion.fuse_points on numpy inputs; the outputs as numpy."""
    from geo4d_amd import fusion
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = fusion.fuse_points(t(points), t(rgba), t(weight), t(mask), **kw)
    torch.cuda.synchronize()
    assert out["points"].dtype == torch.float32 and out["weight"].dtype == torch.float32 and out["count"].dtype == torch.int32
    assert out["points"].device.type == "cuda" and out["points"].dim() == 2 and out["points"].shape[1] == 3
    assert out["rgba"] is None or (out["rgba"].dtype == torch.uint8 and tuple(out["rgba"].shape) == (len(out["points"]), 4))
    return {k: None if out[k] is None else out[k].cpu().numpy() for k in KEYS}


def _equal(got, ref):
    return all((got[k] is None and ref[k] is None) or np.array_equal(got[k], ref[k]) for k in KEYS)


def _rows(out):
    """One bytes object per output row: position, colour, weight and count."""
    return [out["points"][m].tobytes() + (b"" if out["rgba"] is None else out["rgba"][m].tobytes()) + out["weight"][m].tobytes() +
            out["count"][m].tobytes() for m in range(len(out["points"]))]


@pytest.fixture(scope="module")
def cloud():
    """20 000 points in [-3, 3]^3, v = 0.25: weights in (0, 300) (wq clamps at both ends), colours, a mask, NaN / inf coordinates,
    zero / negative / NaN weights, points exactly on cell boundaries; and the restatement's results, computed once."""
    g = np.random.default_rng(11)
    N = 20000
    p = g.uniform(-3, 3, size=(N, 3)).astype(np.float32)
    w = g.uniform(0.0, 300.0, size=N).astype(np.float32)
    w[w == 0] = 1.0
    w[:400] = g.uniform(1e-5, 0.01, size=400).astype(np.float32)                   # wq = 0 before the clamp -> 1
    p[1000:1600] = g.integers(-12, 13, size=(600, 3)).astype(np.float32) * np.float32(0.25)    # on cell boundaries, negatives too
    p[2000:2300, 0] = g.integers(-12, 13, size=300).astype(np.float32) * np.float32(0.25)      # on a boundary on one axis
    p[3000:3050, 1] = np.nan
    p[3050:3100, 2] = np.inf
    p[3100:3150, 0] = -np.inf
    w[4000:4050] = 0.0
    w[4050:4100] = -2.0
    w[4100:4150] = np.nan
    w[4150:4200] = np.inf
    c = dict(points=p, rgba=g.integers(0, 256, size=(N, 4), dtype=np.uint8), weight=w, mask=g.uniform(size=N) < 0.85, voxel=0.25)
    assert (w[~np.isnan(w)] < 256).sum() > 0 and (w[np.isfinite(w)] > 255.99).sum() > 0
    c["ref"] = {(r, k): fr.fuse(p, c["rgba"], w, c["mask"], voxel=0.25, reduce=r, min_count=k) for r in ("mean", "best") for k in (1, 3)}
    return c


# ---- 1. the random cloud -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("reduce", ["mean", "best"])
def test_random_cloud_matches_the_restatement(dev, cloud, reduce, min_count):
    """Exact equality of every output. A voxel may differ only if it contains, or neighbours the cell of, an input point within 1e-4
    voxel of a cell boundary, and at most 0.05 % of the voxels may be excused; fp32 division is correctly rounded on both sides, so the
    allowance should go unused."""
    ref = cloud["ref"][(reduce, min_count)]
    got = _gpu(dev, cloud["points"], cloud["rgba"], cloud["weight"], cloud["mask"], voxel=cloud["voxel"], reduce=reduce, min_count=min_count)
    assert ref["dropped"] == 0 and len(ref["points"]) > (5000 if min_count == 1 else 100)
    a, b = _rows(got), _rows(ref)
    differ = [r for r in set(a) ^ set(b)]
    print(f"[fusion random {reduce} min_count={min_count}] {len(b)} voxels, {len(differ)} differ / excused (0 expected)")
    if differ:
        part = fr.taking_part(cloud["points"], cloud["weight"], cloud["mask"], cloud["voxel"])[0]
        rows = np.nonzero(part)[0]
        rows = rows[fr.excusable(cloud["points"], cloud["voxel"], rows)]
        near = {tuple(c) for c in fr.cells(cloud["points"][rows], cloud["voxel"]).astype(np.int64)}
        excused = set()
        for r in differ:
            c = np.floor(np.frombuffer(r[:12], dtype=np.float32).astype(np.float64) / np.float64(np.float32(cloud["voxel"]))).astype(np.int64)
            assert any((c[0] + dx, c[1] + dy, c[2] + dz) in near for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)), c
            excused.add(tuple(c))
        assert len(excused) <= 5e-4 * len(b)
    else:
        assert _equal(got, ref)                                                     # the same rows in the same order


# ---- 2. a full table ---------------------------------------------------------------------------------------------------------------------
def test_full_table_equals_a_roomy_one(dev):
    """4 096 points in 4 096 distinct voxels with capacity 4 096: load factor 1, long probe chains, wrap-around past the last slot."""
    g = np.random.default_rng(2)
    cells = np.stack(np.meshgrid(np.arange(-8, 8), np.arange(-8, 8), np.arange(-8, 8), indexing="ij"), -1).reshape(-1, 3)
    p = ((cells[g.permutation(4096)] + g.uniform(0.1, 0.9, size=(4096, 3))) * 0.5).astype(np.float32)
    rgba = g.integers(0, 256, size=(4096, 4), dtype=np.uint8)
    w = g.uniform(0.5, 20, size=4096).astype(np.float32)
    ref = fr.fuse(p, rgba, w, voxel=0.5)
    assert len(ref["points"]) == 4096 and (ref["count"] == 1).all()
    for reduce in ("mean", "best"):
        full = _gpu(dev, p, rgba, w, voxel=0.5, reduce=reduce, capacity=4096)
        roomy = _gpu(dev, p, rgba, w, voxel=0.5, reduce=reduce, capacity=8192)
        assert _equal(full, roomy), reduce
        assert _equal(full, ref if reduce == "mean" else fr.fuse(p, rgba, w, voxel=0.5, reduce="best")), reduce


# ---- 3. one hot voxel --------------------------------------------------------------------------------------------------------------------
def test_one_hot_voxel_loses_no_add(dev):
    """50 000 points in a single cell at weight 255.99 (wq = 32 767): every lane of every wave adds into the same eight words."""
    g = np.random.default_rng(3)
    p = g.uniform(1.0, 2.0, size=(50000, 3)).astype(np.float32)
    p = np.clip(p, np.float32(1.0), np.nextafter(np.float32(2.0), np.float32(0)))
    rgba = g.integers(0, 256, size=(50000, 4), dtype=np.uint8)
    w = np.full(50000, 255.99, np.float32)
    ref = fr.fuse(p, rgba, w, voxel=1.0)
    assert len(ref["points"]) == 1 and ref["sums"]["sw"].tolist() == [50000 * 32767] and ref["count"].tolist() == [50000]
    got = _gpu(dev, p, rgba, w, voxel=1.0)
    assert _equal(got, ref), (got, {k: ref[k] for k in KEYS})
    from geo4d_amd import ops                                                     # the integer sums themselves, straight from the table
    t = lambda x: torch.from_numpy(x).to(dev)
    table = ops.fuse_insert(t(p), t(rgba), t(w), voxel=1.0)
    keys, slots, count = ops.fuse_compact(table)
    assert int(count) == 1 and int(keys[0]) == int(ref["sums"]["key"][0]) and int(table.dropped) == 0
    acc = table.ws[table.capacity:].reshape(table.capacity, 8)[int(slots[0])].tolist()
    s = ref["sums"]
    assert acc == [int(s["sw"][0]), *s["sq"][0].tolist(), *s["sc"][0].tolist(), 50000]
    best = _gpu(dev, p, rgba, w, voxel=1.0, reduce="best")                        # all weights tie: row 0 wins
    assert np.array_equal(best["points"][0], p[0]) and np.array_equal(best["rgba"][0], rgba[0]) and best["count"].tolist() == [50000]


# ---- 4. order and determinism ------------------------------------------------------------------------------------------------------------
def test_two_runs_and_row_permutations_are_equal(dev, cloud):
    from geo4d_amd import fusion
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    w = cloud["weight"].copy()
    ok = np.isfinite(w) & (w > 0)
    w[ok] = (np.random.default_rng(4).permutation(int(ok.sum())) + 1).astype(np.float32) * np.float32(0.01)    # distinct weights
    perm = np.random.default_rng(5).permutation(len(w))
    for reduce in ("mean", "best"):
        args = [cloud["points"], cloud["rgba"], w, cloud["mask"]]
        a = fusion.fuse_points(*[t(x) for x in args], voxel=0.25, reduce=reduce)
        b = fusion.fuse_points(*[t(x) for x in args], voxel=0.25, reduce=reduce)
        c = fusion.fuse_points(*[t(x[perm]) for x in args], voxel=0.25, reduce=reduce)
        assert len(a["points"]) > 5000
        for k in KEYS:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), (reduce, k)
        ref = fr.fuse(*args, voxel=0.25, reduce=reduce)
        assert all(np.array_equal(a[k].cpu().numpy(), ref[k]) for k in KEYS), reduce


# ---- 5. edges ----------------------------------------------------------------------------------------------------------------------------
def test_empty_inputs_dropped_points_and_no_colours(dev):
    from geo4d_amd import fusion
    for reduce in ("mean", "best"):
        none = _gpu(dev, np.zeros((0, 3), np.float32), np.zeros((0, 4), np.uint8), np.zeros(0, np.float32), voxel=0.5, reduce=reduce)
        masked = _gpu(dev, np.ones((70, 3), np.float32), np.zeros((70, 4), np.uint8), None, np.zeros(70, bool), voxel=0.5, reduce=reduce)
        for out in (none, masked):
            assert out["points"].shape == (0, 3) and out["rgba"].shape == (0, 4) and out["weight"].shape == (0,) and out["count"].shape == (0,)
    two = np.array([[0, 0, 0], [2, 0, 0]], np.float32)
    assert fr.fuse(two, voxel=1e-6)["dropped"] == 1                                 # cell index 2e6 >= 2^20
    with pytest.raises(ValueError, match=r"\b1 point"):
        fusion.fuse_points(torch.from_numpy(two).to(dev), voxel=1e-6)
    plain = _gpu(dev, two, voxel=0.5)
    assert plain["rgba"] is None and _equal(plain, fr.fuse(two, voxel=0.5)) and plain["weight"].tolist() == [1.0, 1.0]
    floats = np.random.default_rng(6).uniform(-0.1, 1.1, size=(500, 3)).astype(np.float32)     # float colours: scene_points' rounding
    pts = np.random.default_rng(7).uniform(-1, 1, size=(500, 3)).astype(np.float32)
    u8 = np.concatenate([np.clip(floats * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8), np.full((500, 1), 255, np.uint8)], 1)
    assert _equal(_gpu(dev, pts, floats, voxel=0.3), fr.fuse(pts, u8, voxel=0.3))


# ---- 6. the scene level ------------------------------------------------------------------------------------------------------------------
def _scene_ref(a, msk, voxel, **kw):
    """The restatement fed the scene's own arrays."""
    n, H, W = a.n, a.H, a.W
    imgs = a.imgs.float().cpu().numpy().reshape(-1, 3)
    u8 = np.concatenate([np.clip(imgs * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8), np.full((n * H * W, 1), 255, np.uint8)], 1)
    return fr.fuse(a.get_pts3d().detach().cpu().numpy().reshape(-1, 3), u8, a.get_conf().detach().cpu().numpy().reshape(-1),
                   None if msk is None else msk.reshape(-1), voxel=voxel, **kw)


def test_fuse_scene_matches_the_restatement(dev):
    from geo4d_amd import fusion
    a = _aligner(dev)
    assert a.fused is None
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    thr = float(a.im_conf.median())
    depth, focal = a.get_depthmaps().detach().cpu().numpy(), a.get_focals().detach().cpu().numpy().reshape(-1)
    for motion in (None, "static", "dynamic"):
        for is_msk in (True, False):
            got = fusion.fuse_scene(a, motion=motion, min_conf_thr=thr, is_msk=is_msk)
            assert got is a.fused
            msk = a.get_masks().cpu().numpy() if is_msk else np.ones((a.n, a.H, a.W), bool)
            if motion is not None:
                dyn = a.dynamic_masks.cpu().numpy()
                msk = msk & (dyn if motion == "dynamic" else ~dyn)
            if not msk.any():
                assert len(got["points"]) == 0
                continue
            voxel = fr.default_voxel(depth, focal, msk)
            assert got["voxel"] == float(np.float32(voxel))
            ref = _scene_ref(a, msk, voxel)
            assert ref["dropped"] == 0 and 0 < len(ref["points"]) <= int(msk.sum())
            assert all(np.array_equal(got[k].cpu().numpy(), ref[k]) for k in KEYS), (motion, is_msk)
    msk = a.get_masks().cpu().numpy()
    wide = 1.5 * fr.default_voxel(depth, focal, msk)                                # a voxel of the caller's, the other mode, min_count
    fixed = fusion.fuse_scene(a, voxel=wide, motion=None, min_conf_thr=thr, reduce="best", min_count=2)
    ref = _scene_ref(a, msk, wide, reduce="best", min_count=2)
    assert len(ref["points"]) > 0 and all(np.array_equal(fixed[k].cpu().numpy(), ref[k]) for k in KEYS) and int(fixed["count"].min()) >= 2


def test_export_and_save_scene_write_the_fused_cloud(dev, tmp_path):
    """fuse_voxel=None is today's glb byte for byte; with a voxel the glb holds the M fused points. save_scene(fuse_static=True) writes
    <seq>_static_fused.glb and nothing else: the dynamic_mask PNGs and <seq>_static.glb stay with dynamic_masks=True."""
    from geo4d_amd import scene_export
    a = _aligner(dev)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    thr = float(a.im_conf.median())
    kw = dict(min_conf_thr=thr, as_pointcloud=True)
    plain = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="plain", **kw)
    none = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="none", fuse_voxel=None, **kw)
    assert a.fused is None and open(plain, "rb").read() == open(none, "rb").read()
    for name, fuse_voxel, motion in (("auto", True, None), ("static", True, "static"), ("fixed", None, None)):
        if name == "fixed":
            fuse_voxel = 1.5 * a.fused["voxel"]
        path = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name=name, fuse_voxel=fuse_voxel, motion=motion, **kw)
        M = len(a.fused["points"])
        assert 0 < M < _points(plain) and _points(path) == M, name
        assert name != "fixed" or a.fused["voxel"] == float(np.float32(fuse_voxel))
    with pytest.raises(ValueError):
        scene_export.get_3D_model_from_scene(str(tmp_path), True, a, min_conf_thr=thr, as_pointcloud=False, fuse_voxel=0.05)
    b = _aligner(dev)
    video = torch.rand((1, 3, b.n, b.H, b.W), generator=torch.Generator().manual_seed(6)) * 2 - 1
    base = scene_export.save_scene(b, str(tmp_path / "base"), "seq", imgs=video)
    assert b.dynamic_masks is None and b.fused is None
    full = scene_export.save_scene(b, str(tmp_path / "full"), "seq", imgs=video, fuse_static=True)
    names = sorted(os.listdir(base))
    assert sorted(os.listdir(full)) == sorted(names + ["seq_static_fused.glb"])
    for f in names:
        assert open(os.path.join(base, f), "rb").read() == open(os.path.join(full, f), "rb").read(), f
    assert b.dynamic_masks is not None                                              # it segmented motion first
    static = b.n * b.H * b.W - int(b.dynamic_masks.sum())                           # save_scene exports with is_msk=False
    assert 0 < _points(os.path.join(full, "seq_static_fused.glb")) == len(b.fused["points"]) < static


# ---- 7. the synthetic scene --------------------------------------------------------------------------------------------------------------
def test_static_part_of_the_synthetic_scene_fuses_onto_the_wall(dev):
    """At least 15 times fewer points than static pixels (22.6 in numpy), every fused point within 1e-5 of the wall -0.2 x + z = 4 except
    voxels that hold a pixel segment_motion got wrong against `truth`. The scene's points come from its fp32 depth maps and poses, so
    they differ in the last bits from the truth arrays of the CPU test: hence 1e-5 and not 1.4e-6."""
    from geo4d_amd import fusion
    s = mr.synthetic_scene()
    a = _synthetic_aligner(dev, s)
    out = fusion.fuse_scene(a, motion="static", is_msk=False)
    assert out["rgba"] is None                                                      # the scene has no frames
    dyn = a.dynamic_masks.cpu().numpy()
    static = int((~dyn).sum())
    M = len(out["points"])
    pts3d = a.get_pts3d().detach().cpu().numpy().reshape(-1, 3)
    ref = fr.fuse(pts3d, None, a.get_conf().detach().cpu().numpy().reshape(-1), ~dyn.reshape(-1), voxel=out["voxel"])
    assert all(np.array_equal(out[k].cpu().numpy(), ref[k]) for k in ("points", "weight", "count"))
    wrong = (~dyn & s["truth"]).reshape(-1)                                         # sphere pixels that went into the static part
    key = lambda c: ((c[:, 0] + fr.LIMIT) << 42) | ((c[:, 1] + fr.LIMIT) << 21) | (c[:, 2] + fr.LIMIT)
    clean = ~np.isin(ref["sums"]["key"], key(fr.cells(pts3d[wrong], out["voxel"]).astype(np.int64)))     # voxels that hold none of them
    p = out["points"].cpu().numpy().astype(np.float64)
    off = np.abs(-0.2 * p[:, 0] + p[:, 2] - 4.0)
    print(f"[fusion synthetic] voxel {out['voxel']:.4f}: {static} static pixels -> {M} fused ({static / M:.1f} x), {int(wrong.sum())} sphere "
          f"pixels in the static part, {int((~clean).sum())} voxels excluded, {off[clean].max():.2e} off the plane")
    assert static >= 15 * M and int(out["count"].sum()) == static
    assert clean.sum() >= 0.9 * M and off[clean].max() < 1e-5
