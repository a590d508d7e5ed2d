"""The nearest-neighbour kernels (geo4d_amd/csrc/nearest.hip) and what stands on them against the numpy restatement
(tests/nearest_restatement.py): index, dist2 and count by np.array_equal, nothing excused; the cloud metrics, the radius outlier removal
of the fusion, and the arguments' defaults, which must leave every earlier output as it was."""
import os

import numpy as np
import pytest
import torch

import motion_restatement as mr
import nearest_restatement as nr
from scene_cases import truth_aligner
from test_nearest_cpu import FAR, HAND_CASES, hand_arrays, planar_grid

pytestmark = pytest.mark.gpu
F = np.float32
EDGE = 2.0 ** 20


def t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def gpu_query(dev, ref, query, r, rmask=None, qmask=None, excl=False, grid=None):
    """ops.nn_grid + ops.nn_query on numpy inputs: (dict of numpy outputs and the two dropped counts, the grid)."""
    from geo4d_amd import ops
    if grid is None:
        grid = ops.nn_grid(t(np.asarray(ref, F).reshape(-1, 3), dev), radius=float(F(r)), mask=t(rmask, dev))
    index, dist2, count, dropped = ops.nn_query(grid, t(np.asarray(query, F).reshape(-1, 3), dev), mask=t(qmask, dev), exclude_same_row=excl)
    torch.cuda.synchronize()
    assert index.dtype == torch.int32 and dist2.dtype == torch.float32 and count.dtype == torch.int32
    return dict(index=index.cpu().numpy(), dist2=dist2.cpu().numpy(), count=count.cpu().numpy(), dropped_reference=grid.dropped,
                dropped_query=dropped), grid


def same(got, ref):
    return all(np.array_equal(got[k], ref[k]) for k in ("index", "dist2", "count")) and \
        got["dropped_reference"] == ref["dropped_reference"] and got["dropped_query"] == ref["dropped_query"]


def check(dev, ref, query, r, rmask=None, qmask=None, excl=False):
    want = nr.query(ref, query, r, reference_mask=rmask, query_mask=qmask, exclude_same_row=excl)
    got, _ = gpu_query(dev, ref, query, r, rmask, qmask, excl)
    assert same(got, want), {k: (got[k][:8], want[k][:8]) for k in ("index", "dist2", "count")}
    return want


# ---- hand cases and empty inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_hand_cases(dev, case):
    ref, query, r, rmask, qmask, excl, index, dist2, count = hand_arrays(case)
    got, _ = gpu_query(dev, ref, query, r, rmask, qmask, excl)
    assert got["index"].tolist() == index.tolist() and got["count"].tolist() == count.tolist() and np.array_equal(got["dist2"], dist2)
    assert got["dropped_reference"] == got["dropped_query"] == 0


def test_empty_inputs(dev):
    from geo4d_amd import nearest
    none, some = np.zeros((0, 3), F), np.array([[0, 0, 0], [0.5, 0, 0]], F)
    for ref, query in ((none, some), (some, none), (none, none)):
        got, grid = gpu_query(dev, ref, query, 1.0)
        assert got["index"].tolist() == [-1] * len(query) and got["count"].tolist() == [0] * len(query)
        assert np.array_equal(got["dist2"], np.full(len(query), np.inf, F)) and got["dropped_query"] == 0
        assert grid.n_taking == 0 or len(ref) == 2
        out = nearest.nearest_points(t(query, dev), t(ref, dev), radius=1.0)
        assert out["index"].shape == (len(query),) and out["grid"].n_reference == len(ref)
        assert nearest.radius_outliers(t(query, dev), radius=1.0, min_neighbours=1).tolist() == [True] * len(query)


# ---- clouds --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nq", [255, 256, 257, 4097])
def test_uniform_clouds(dev, Nq):
    g = np.random.default_rng(Nq)
    ref, query = g.uniform(-1, 1, size=(1000, 3)).astype(F), g.uniform(-1, 1, size=(Nq, 3)).astype(F)
    want = check(dev, ref, query, 0.25)
    assert (want["count"] > 0).sum() > 0.9 * Nq and want["count"].max() > 5


@pytest.mark.parametrize("case", [c for c in nr.rule7_inputs() if c[0] != "uniform"], ids=lambda c: f"{c[0]} r={c[3]}")
def test_lattices(dev, case):
    """Points on the lattices 0.1 k and 0.05 k: many on cell boundaries, many ties in d2 (the lowest row wins), many at d2 = r2 up to
    rounding."""
    _, ref, query, r = case
    want = check(dev, ref, query, r)
    assert (want["count"] > 0).sum() > 0.5 * len(query)
    check(dev, ref, ref, r, excl=True)


def test_one_crowded_cell(dev):
    """5 000 references inside one cell, 64 queries in and around it: the long row."""
    g = np.random.default_rng(5)
    ref = g.uniform(0.25, 0.5, size=(5000, 3)).astype(F)
    query = g.uniform(0.0, 0.75, size=(64, 3)).astype(F)
    query[:8] = g.uniform(0.25, 0.5, size=(8, 3)).astype(F)
    assert (nr.cells(ref, 0.25) == 1).all()
    want = check(dev, ref, query, 0.25)
    assert want["count"].max() > 2000 and (want["count"] == 0).any()


def edge_points():
    """Points in the outermost cells +-(2^20 - 1) of every axis at r = 1 with a neighbour one cell inwards, the two corners where all
    three fields of the key are at their ends, and pairs whose keys are neighbours only through a carry between fields."""
    hi, lo = EDGE - 0.5, -EDGE + 1.5                                                # cells 2^20 - 1 and -(2^20 - 1)
    pts = []
    for axis in range(3):
        for edge, inward in ((hi, hi - 0.75), (lo, lo + 0.75)):
            for v in (edge, inward):
                p = [0.25, 0.25, 0.25]
                p[axis] = v
                pts.append(p)
    pts += [[hi, hi, hi], [hi - 0.75, hi, hi], [lo, lo, lo], [lo, lo + 0.75, lo]]
    pts += [[0.5, 0.5, hi], [0.5, 1.5, lo], [0.5, hi, hi], [1.5, lo, lo], [0.5, 0.5, lo], [0.5, -0.5, hi]]   # a carry apart in key space
    return np.asarray(pts, dtype=F)


def test_grid_edges(dev):
    from geo4d_amd import nearest, ops
    pts = edge_points()
    c = nr.cells(pts, 1.0)
    assert c.max() == EDGE - 1 and c.min() == -(EDGE - 1)
    g = np.random.default_rng(9)
    query = (pts[g.integers(0, len(pts), 200)] + g.uniform(-0.4, 0.4, size=(200, 3)).astype(F)).astype(F)
    query = query[(np.abs(nr.cells(query, 1.0)) < EDGE).all(1)]
    assert len(query) > 100
    for q, excl in ((pts, False), (pts, True), (query, False)):
        want = check(dev, pts, q, 1.0, excl=excl)
        assert want["dropped_reference"] == want["dropped_query"] == 0 and (want["count"] > 0).sum() >= 12
    # a point beyond the grid is dropped: the wrapper raises, ops returns the count
    out = np.concatenate([pts, np.array([[EDGE + 0.5, 0, 0], [0, -EDGE - 0.5, 0]], F)])
    want = check(dev, out, out, 1.0)
    assert want["dropped_reference"] == want["dropped_query"] == 2 and want["index"][-2:].tolist() == [-1, -1]
    grid = ops.nn_grid(t(out, dev), radius=1.0)
    assert grid.dropped == 2 and grid.n_taking == len(pts) and ops.nn_query(grid, t(out, dev))[3] == 2
    with pytest.raises(ValueError, match=r"2 reference point\(s\) lie outside the cell grid"):
        nearest.nearest_points(t(pts, dev), t(out, dev), radius=1.0)
    with pytest.raises(ValueError, match=r"2 query point\(s\) lie outside the cell grid"):
        nearest.nearest_points(t(out, dev), t(pts, dev), radius=1.0)
    with pytest.raises(ValueError, match=r"2 cloud point\(s\) lie outside the cell grid"):
        nearest.radius_outliers(t(out, dev), radius=1.0, min_neighbours=1)


def test_masked_and_non_finite_rows(dev):
    g = np.random.default_rng(21)
    ref, query = g.uniform(-1, 1, size=(1500, 3)).astype(F), g.uniform(-1, 1, size=(700, 3)).astype(F)
    for a in (ref, query):
        a[10:20, 0] = np.nan
        a[20:30, 1] = np.inf
        a[30:40, 2] = -np.inf
    rmask, qmask = g.uniform(size=1500) < 0.7, g.uniform(size=700) < 0.7
    want = check(dev, ref, query, 0.25, rmask, qmask)
    assert (want["index"][~qmask] == -1).all() and (want["index"][10:40] == -1).all() and rmask[want["index"][want["index"] >= 0]].all()
    check(dev, ref, ref, 0.25, rmask, rmask, excl=True)
    check(dev, ref, query, 0.25, np.zeros(1500, bool), None)
    check(dev, ref, query, 0.25, None, np.zeros(700, bool))


def test_determinism_reuse_and_permutation(dev):
    from geo4d_amd import nearest
    g = np.random.default_rng(33)
    ref, q1, q2 = (g.uniform(-1, 1, size=(n, 3)).astype(F) for n in (2000, 900, 1100))
    first = nearest.nearest_points(t(q1, dev), t(ref, dev), radius=0.2)
    again = nearest.nearest_points(t(q1, dev), t(ref, dev), radius=0.2)
    reused = nearest.nearest_points(t(q1, dev), grid=first["grid"], radius=0.2)
    for k in ("index", "dist2", "count"):
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], reused[k]), k
    assert reused["grid"] is first["grid"]
    other = nearest.nearest_points(t(q2, dev), grid=first["grid"], radius=0.2)
    want = nr.query(ref, q2, 0.2)
    assert all(np.array_equal(other[k].cpu().numpy(), want[k]) for k in ("index", "dist2", "count"))
    with pytest.raises(ValueError, match="the grid was built for radius"):
        nearest.nearest_points(t(q2, dev), grid=first["grid"], radius=0.25)
    perm = g.permutation(len(ref))
    moved = nearest.nearest_points(t(q1, dev), t(ref[perm], dev), radius=0.2)
    assert torch.equal(moved["dist2"], first["dist2"]) and torch.equal(moved["count"], first["count"])
    hit = (first["index"] >= 0).cpu().numpy()
    assert hit.sum() > 500
    assert np.array_equal(ref[first["index"].cpu().numpy()[hit]], ref[perm][moved["index"].cpu().numpy()[hit]])
    self_ = nearest.nearest_points(t(ref, dev), t(ref, dev), radius=0.2, exclude_self=True)
    want = nr.query(ref, ref, 0.2, exclude_same_row=True)
    assert all(np.array_equal(self_[k].cpu().numpy(), want[k]) for k in ("index", "dist2", "count"))


# ---- metrics -------------------------------------------------------------------------------------------------------------------------------
INTS = ("n_pred", "n_gt", "within_pred", "within_gt", "unmatched_pred", "unmatched_gt", "precision", "recall", "fscore")
MEANS = ("accuracy", "completeness", "chamfer")


def metrics_match(got, want):
    for k in INTS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in MEANS:
        assert got[k] == pytest.approx(want[k], rel=1e-12), (k, got[k], want[k])
    for k in ("pred_dist", "gt_dist"):
        assert got[k].dtype == torch.float32 and np.array_equal(got[k].cpu().numpy(), want[k], equal_nan=True), k


@pytest.fixture(scope="module")
def scene(dev):
    s = mr.synthetic_scene()
    a = truth_aligner(dev, s)
    return a, a.get_pts3d().detach().reshape(-1, 3).float().contiguous()


def test_cloud_metrics_on_planar_grids(dev):
    from geo4d_amd import evaluation
    gt, pred = planar_grid(0.0), np.concatenate([planar_grid(0.03), FAR])
    mask = np.ones(407, bool)
    mask[[5, 403]] = False
    pred[3] = np.nan
    for pm, ts in ((None, (0.05, 0.02)), (mask, None)):
        got = evaluation.cloud_metrics(t(pred, dev), t(gt, dev), max_dist=0.05, thresholds=ts, pred_mask=t(pm, dev))
        metrics_match(got, nr.cloud_metrics(pred, gt, 0.05, thresholds=ts, pred_mask=pm))
    assert got["unmatched_pred"] == 6 and got["unmatched_gt"] == 2 and got["n_pred"] == 404
    far = evaluation.cloud_metrics(t(FAR, dev), t(gt, dev), max_dist=0.05)
    assert far["fscore"] == [0.0] and far["precision"] == [0.0] and far["recall"] == [0.0]
    for p, g, pm in ((pred[3:4], gt, None), (gt, pred[3:4], None), (pred, gt, np.zeros(407, bool)), (np.zeros((0, 3), F), gt, None)):
        with pytest.raises(ValueError, match="no point takes part"):
            evaluation.cloud_metrics(t(p, dev), t(g, dev), max_dist=0.05, pred_mask=t(pm, dev))


def test_cloud_metrics_on_the_synthetic_scene(dev, scene):
    from geo4d_amd import evaluation
    _, pts = scene
    own = evaluation.cloud_metrics(pts, pts, max_dist=0.05, thresholds=(0.01, 0.05))
    assert own["accuracy"] == own["completeness"] == own["chamfer"] == 0.0 and own["precision"] == own["recall"] == own["fscore"] == [1.0, 1.0]
    assert own["n_pred"] == own["n_gt"] == len(pts) and own["unmatched_pred"] == 0 and not own["pred_dist"].any()
    shifted = pts + torch.tensor([0.02, -0.01, 0.03], device=dev)
    got = evaluation.cloud_metrics(shifted, pts, max_dist=0.15, thresholds=(0.05, 0.15), voxel=0.1)
    p, g = got["pred_points"].cpu().numpy(), got["gt_points"].cpu().numpy()
    assert 500 < len(p) < 5000 and 500 < len(g) < 5000
    want = nr.cloud_metrics(p, g, 0.15, thresholds=(0.05, 0.15))
    metrics_match(got, want)
    assert 0 < want["within_pred"][0] < want["within_pred"][1] and 0 < want["accuracy"] < 0.15
    sub, sub_gt = pts[::16].contiguous(), pts[5::16].contiguous() + torch.tensor([0.0, 0.03, 0.0], device=dev)
    qm = torch.arange(len(sub), device=dev) % 7 != 0
    got = evaluation.cloud_metrics(sub, sub_gt, max_dist=0.1, thresholds=(0.04, 0.1), pred_mask=qm)
    metrics_match(got, nr.cloud_metrics(sub.cpu().numpy(), sub_gt.cpu().numpy(), 0.1, thresholds=(0.04, 0.1), pred_mask=qm.cpu().numpy()))


def test_scene_cloud_metrics_moves_the_points_as_documented(dev, tmp_path):
    from scipy.spatial.transform import Rotation
    from geo4d_amd import evaluation, io
    a = truth_aligner(dev, mr.synthetic_scene())                                    # the scene's cameras stand on a line: move them off it
    a.P["im_poses"][:, 4:7] += 0.05 * torch.randn((a.n, 3), generator=torch.Generator().manual_seed(8)).to(dev)
    pts = a.get_pts3d().detach().reshape(-1, 3).float().contiguous()
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = 1.3 * Rotation.from_euler("xyz", [0.2, -0.4, 0.1]).as_matrix(), [0.5, -2.0, 1.0]
    Mt = torch.from_numpy(M).to(dev).float()
    moved = pts @ Mt[:3, :3].T + Mt[:3, 3]
    gt = (moved[3::4] + torch.tensor([0.01, 0.0, -0.02], device=dev)).contiguous()
    kw = dict(max_dist=0.1, thresholds=(0.03, 0.1))
    want = evaluation.cloud_metrics(moved, gt, **kw)
    got = evaluation.scene_cloud_metrics(a, gt, transform=M, out_dir=str(tmp_path), seq="wall", **kw)
    same_dict = lambda x, y: all(x[k] == y[k] for k in INTS + MEANS) and all(torch.equal(x[k], y[k]) for k in ("pred_dist", "gt_dist"))
    assert same_dict(got, want) and np.array_equal(got["transform"], M)
    assert 0 < got["accuracy"] < 0.1 and got["n_pred"] == len(pts)
    text = open(tmp_path / "wall_cloud_metric.txt").read()
    assert "Seq: wall" in text and repr(got["chamfer"]) in text and repr(got["fscore"][1]) in text
    plain = evaluation.scene_cloud_metrics(a, gt.cpu().numpy(), **kw)               # not moved; a numpy ground truth
    assert plain["transform"] is None and same_dict(plain, evaluation.cloud_metrics(pts, gt, **kw))
    # the trajectories' sim(3): the scene's own poses moved by M are the ground-truth trajectory
    c2w = a.get_im_poses_matrix().detach().double().cpu().numpy()
    gt_c2w = c2w.copy()
    gt_c2w[:, :3, :3] = (M[:3, :3] / 1.3) @ c2w[:, :3, :3]
    gt_c2w[:, :3, 3] = c2w[:, :3, 3] @ M[:3, :3].T + M[:3, 3]
    fitted = evaluation.scene_cloud_metrics(a, gt, gt_traj=io.get_tum_poses(torch.from_numpy(gt_c2w)), **kw)
    assert np.allclose(fitted["transform"], M, atol=1e-5)
    assert same_dict(fitted, evaluation.scene_cloud_metrics(a, gt, transform=fitted["transform"], **kw))
    assert sorted(os.listdir(tmp_path)) == ["wall_cloud_metric.txt"]


# ---- outliers in the fusion ----------------------------------------------------------------------------------------------------------------
FUSED = ("points", "rgba", "weight", "count")


def test_fusion_drops_isolated_points(dev, scene):
    from geo4d_amd import fusion, nearest
    a, pts = scene
    isolated = torch.tensor([[10.0 + 2 * k, 10.0, 10.0 - k] for k in range(20)], device=dev)
    cloud = torch.cat([pts, isolated])
    base = fusion.fuse_scene(a, motion=None, is_msk=False)
    v = base["voxel"]
    plain = fusion.fuse_points(cloud, voxel=v)
    M = len(plain["points"])
    assert M == len(base["points"]) + 20
    for k, radius in ((2, None), (5, 3 * v)):
        r = float(F(2 * v if radius is None else radius))
        keep = nr.radius_outliers(plain["points"].cpu().numpy(), r, k)
        got = fusion.fuse_points(cloud, voxel=v, min_neighbours=k, neighbour_radius=radius)
        assert 0.5 * M < keep.sum() <= M - 20 and got["voxel"] == v and got["rgba"] is None
        for name in ("points", "weight", "count"):
            assert np.array_equal(got[name].cpu().numpy(), plain[name].cpu().numpy()[keep]), (k, name)
        assert not bool((got["points"][:, 0] >= 9).any())                           # all 20 are gone
        assert torch.equal(nearest.radius_outliers(plain["points"], radius=r, min_neighbours=k), t(keep, dev))
        thinned = fusion.fuse_scene(a, motion=None, is_msk=False, min_neighbours=k, neighbour_radius=radius)
        assert thinned is a.fused
        keep_scene = nr.radius_outliers(base["points"].cpu().numpy(), r, k)
        assert np.array_equal(thinned["points"].cpu().numpy(), base["points"].cpu().numpy()[keep_scene])
        assert np.array_equal(thinned["count"].cpu().numpy(), base["count"].cpu().numpy()[keep_scene])
    # with colours and min_count, the rows still belong together
    rgb = torch.rand((len(cloud), 3), generator=torch.Generator().manual_seed(1)).to(dev)
    full = fusion.fuse_points(cloud, rgb, voxel=v, min_count=2)
    keep = nr.radius_outliers(full["points"].cpu().numpy(), float(F(2 * v)), 3)
    got = fusion.fuse_points(cloud, rgb, voxel=v, min_count=2, min_neighbours=3)
    assert all(np.array_equal(got[name].cpu().numpy(), full[name].cpu().numpy()[keep]) for name in FUSED)


def test_defaults_leave_the_fusion_and_the_export_as_they_were(dev, scene, tmp_path):
    """min_neighbours=0, or the argument left out, runs what ran before: equal tensors, a byte-identical glb."""
    from geo4d_amd import fusion, scene_export
    from scene_cases import tiny_aligner
    _, pts = scene
    w = torch.rand(len(pts), generator=torch.Generator().manual_seed(2)).to(dev) + 0.1
    for kw in (dict(), dict(reduce="best", min_count=2)):
        old, zero = fusion.fuse_points(pts, None, w, voxel=0.05, **kw), fusion.fuse_points(pts, None, w, voxel=0.05, min_neighbours=0, **kw)
        wide = fusion.fuse_points(pts, None, w, voxel=0.05, min_neighbours=0, neighbour_radius=0.3, **kw)
        assert all(torch.equal(old[k], zero[k]) and torch.equal(old[k], wide[k]) for k in ("points", "weight", "count"))
    a = tiny_aligner(dev)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    thr = float(a.im_conf.median())
    old = dict(fusion.fuse_scene(a, min_conf_thr=thr))
    zero = fusion.fuse_scene(a, min_conf_thr=thr, min_neighbours=0)
    assert all(torch.equal(old[k], zero[k]) for k in FUSED)
    kw = dict(min_conf_thr=thr, as_pointcloud=True, fuse_voxel=True)
    plain = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="plain", **kw)
    full = a.fused
    zero = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="zero", fuse_min_neighbours=0, **kw)
    assert open(plain, "rb").read() == open(zero, "rb").read()
    r = float(F(2 * full["voxel"]))
    k = int(np.median(nr.query(full["points"].cpu().numpy(), full["points"].cpu().numpy(), r, exclude_same_row=True)["count"])) + 1
    keep = nr.radius_outliers(full["points"].cpu().numpy(), r, k)                   # the restatement's median count + 1: about half stay
    thin = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="thin", fuse_min_neighbours=k, **kw)
    assert os.path.exists(thin) and np.array_equal(a.fused["points"].cpu().numpy(), full["points"].cpu().numpy()[keep])
    assert np.array_equal(a.fused["rgba"].cpu().numpy(), full["rgba"].cpu().numpy()[keep])
    print(f"[nearest export] {len(keep)} fused points, {int(keep.sum())} with {k} neighbours within 2 voxels")
    assert 0 < keep.sum() < len(keep)
    d = scene_export.save_scene(a, str(tmp_path / "s"), "seq", min_conf_thr=thr, fuse_static=True, fuse_min_neighbours=k)
    static = dict(a.fused)
    d0 = scene_export.save_scene(a, str(tmp_path / "s0"), "seq", min_conf_thr=thr, fuse_static=True)
    assert sorted(os.listdir(d)) == sorted(os.listdir(d0)) and "seq_static_fused.glb" in os.listdir(d)
    keep = nr.radius_outliers(a.fused["points"].cpu().numpy(), float(F(2 * a.fused["voxel"])), k)
    assert np.array_equal(static["points"].cpu().numpy(), a.fused["points"].cpu().numpy()[keep])
    for f in os.listdir(d0):
        same = open(os.path.join(d, f), "rb").read() == open(os.path.join(d0, f), "rb").read()
        assert same == (f != "seq_static_fused.glb") or keep.all(), f
