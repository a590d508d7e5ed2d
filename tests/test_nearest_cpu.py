"""The nearest-neighbour rule without a GPU: its numpy restatement (tests/nearest_restatement.py) against the cell-free definition on
rule 7's six inputs, hand cases with every output written out, the metrics and the outlier rule on planar grids, and the host side of
the HIP path (the geo4d_nn_keys, geo4d_nn_gather and geo4d_nn_query symbols): ABI agreement, host-side argument validation and the
Python errors. tests/test_nearest_gpu.py asserts the device against the same restatement."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import nearest_restatement as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geo4d_nn_keys", "geo4d_nn_gather", "geo4d_nn_query")
F = np.float32
INF = float("inf")
NAN = float("nan")
TENTH2 = float(F(0.1) * F(0.1))                                                     # 0.1f * 0.1f as the kernel rounds it
BEYOND_4 = float(np.nextafter(F(4), F(5)))
LINE = [[0, 0, 0], [0.5, 0, 0], [3, 0, 0]]
FIVE = [[1, 1, 1]] * 5
# (name, reference, query (None: the reference itself), r, reference mask, query mask, exclude_same_row, index, dist2, count)
HAND_CASES = [
    ("one point", [[0, 0, 0]], [[0.5, 0, 0]], 1.0, None, None, False, [0], [0.25], [1]),
    ("one point out of reach", [[0, 0, 0]], [[1.5, 0, 0]], 1.0, None, None, False, [-1], [INF], [0]),
    ("query set = reference set", LINE, None, 1.0, None, None, False, [0, 1, 2], [0, 0, 0], [2, 2, 1]),
    ("query set = reference set without the own row", LINE, None, 1.0, None, None, True, [1, 0, -1], [0.25, 0.25, INF], [1, 1, 0]),
    ("five identical reference points", FIVE, [[1, 1, 1.5], [1, 1, 1]], 1.0, None, None, False, [0, 0], [0.25, 0], [5, 5]),
    ("five identical points among themselves", FIVE, None, 1.0, None, None, True, [1, 0, 0, 0, 0], [0] * 5, [4] * 5),
    ("five identical points, the first two masked out", FIVE, [[1, 1, 1]], 1.0, [0, 0, 1, 1, 1], None, False, [2], [0], [3]),
    ("d2 == r2 counts", [[3, 4, 0]], [[0, 0, 0]], 5.0, None, None, False, [0], [25], [1]),
    ("one step beyond r does not", [[3, BEYOND_4, 0]], [[0, 0, 0]], 5.0, None, None, False, [-1], [INF], [0]),
    ("on cell boundaries, negative coordinates", [[-0.5, -0.5, -0.5], [0, 0, 0], [-1, 0, 0.5], [-1, 0, 0]], [[-0.5, 0, 0], [0, -0.5, 0]], 0.5,
     None, None, False, [1, 1], [0.25, 0.25], [2, 1]),
    ("a reference mask hiding everything", LINE, [[0, 0, 0]], 1.0, [0, 0, 0], None, False, [-1], [INF], [0]),
    ("a query mask hiding everything", LINE, LINE, 1.0, None, [0, 0, 0], False, [-1] * 3, [INF] * 3, [0] * 3),
    ("NaN and inf coordinates", [[NAN, 0, 0], [0, 0, 0], [INF, 0, 0]], [[0.1, 0, 0], [NAN, 0, 0], [0, -INF, 0]], 1.0, None, None, False,
     [1, -1, -1], [TENTH2, INF, INF], [1, 0, 0]),
]


def planar_grid(z=0.0, n=20, step=0.1):
    """n x n points i * step, j * step (float32 products) at height z."""
    i = np.arange(n, dtype=F) * F(step)
    x, y = np.meshgrid(i, i, indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), np.full(n * n, z, F)], 1).astype(F)


FAR = np.array([[50 + 3 * k, -20, 7] for k in range(7)], dtype=F)                    # 7 points far from the grid and from each other


def hand_arrays(case):
    _, ref, query, r, rmask, qmask, excl, index, dist2, count = case
    ref = np.asarray(ref, dtype=F).reshape(-1, 3)
    query = ref if query is None else np.asarray(query, dtype=F).reshape(-1, 3)
    m = lambda x: None if x is None else np.asarray(x, dtype=bool)
    return ref, query, r, m(rmask), m(qmask), excl, np.asarray(index, np.int32), np.asarray(dist2, F), np.asarray(count, np.int32)


# ---- rule 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nr.rule7_inputs(), ids=lambda c: f"{c[0]} r={c[3]}")
def test_neighbouring_cells_give_what_the_cell_free_definition_gives(case):
    """A query may differ only if some reference point's float64 distance lies within a relative 1e-5 of r, and at most 0.5 % of the
    queries may be excused. Measured: 0 of 3 000 differ in all six runs."""
    name, ref, query, r = case
    a, b = nr.query(ref, query, r), nr.query(ref, query, r, cell_free=True)
    differ = (a["index"] != b["index"]) | (a["dist2"] != b["dist2"]) | (a["count"] != b["count"])
    shell = nr.near_the_shell(ref, query, r)
    print(f"[nearest rule 7] {name} r = {r}: {int(differ.sum())} of {len(query)} queries differ, {int(shell.sum())} in the shell; "
          f"{int((a['count'] > 0).sum())} matched, mean count {a['count'].mean():.2f}")
    assert a["dropped_reference"] == a["dropped_query"] == 0
    assert not (differ & ~shell).any()
    assert differ.sum() <= 0.005 * len(query)
    assert (a["count"] > 0).sum() > 0.5 * len(query)                                # the comparison is about something


# ---- hand cases --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_hand_cases(case):
    ref, query, r, rmask, qmask, excl, index, dist2, count = hand_arrays(case)
    for cell_free in (False, True):
        got = nr.query(ref, query, r, reference_mask=rmask, query_mask=qmask, exclude_same_row=excl, cell_free=cell_free)
        assert got["index"].dtype == np.int32 and got["dist2"].dtype == F and got["count"].dtype == np.int32
        assert got["index"].tolist() == index.tolist() and got["count"].tolist() == count.tolist()
        assert np.array_equal(got["dist2"], dist2)
        assert got["dropped_reference"] == got["dropped_query"] == 0


def test_points_outside_the_grid_are_counted_and_take_no_part():
    edge = F(2 ** 20)
    ref = np.array([[edge + F(0.5), 0, 0], [edge - 1, 0, 0], [-edge, 0, 0], [-edge - 1, 0, 0], [NAN, 0, 0]], dtype=F)   # cells 2^20, 2^20 - 1, -2^20, ..
    got = nr.query(ref, ref, 1.0)
    assert got["dropped_reference"] == got["dropped_query"] == 3
    assert got["index"].tolist() == [-1, 1, -1, -1, -1] and got["count"].tolist() == [0, 1, 0, 0, 0]


def test_a_permuted_reference_leaves_dist2_and_count():
    _, ref, query, r = nr.rule7_inputs()[3]
    a = nr.query(ref, query, r)
    perm = np.random.default_rng(3).permutation(len(ref))
    b = nr.query(ref[perm], query, r)
    assert np.array_equal(a["dist2"], b["dist2"]) and np.array_equal(a["count"], b["count"])
    hit = a["index"] >= 0
    assert np.array_equal(ref[a["index"][hit]], ref[perm][b["index"][hit]])          # tie-free data: the same positions


# ---- metrics -----------------------------------------------------------------------------------------------------------------------------
def test_metrics_of_a_planar_grid_against_its_shifted_copy():
    """Every distance is sqrtf of one value, 0.03f * 0.03f: precision 1 at 0.05, 0 at 0.02."""
    gt, pred = planar_grid(0.0), planar_grid(0.03)
    d = float(np.sqrt(F(0.03) * F(0.03)))
    m = nr.cloud_metrics(pred, gt, 0.05, thresholds=(0.05, 0.02))
    assert m["n_pred"] == m["n_gt"] == 400 and m["unmatched_pred"] == m["unmatched_gt"] == 0
    assert m["within_pred"] == [400, 0] and m["within_gt"] == [400, 0]
    assert m["precision"] == [1.0, 0.0] and m["recall"] == [1.0, 0.0] and m["fscore"] == [1.0, 0.0]
    assert (m["pred_dist"] == F(d)).all() and (m["gt_dist"] == F(d)).all()
    assert m["accuracy"] == pytest.approx(d, rel=1e-12) and m["completeness"] == pytest.approx(d, rel=1e-12)
    assert m["chamfer"] == pytest.approx(d, rel=1e-12)


def test_metrics_with_seven_far_points_and_a_masked_row():
    gt, pred = planar_grid(0.0), np.concatenate([planar_grid(0.03), FAR])
    d, r = float(np.sqrt(F(0.03) * F(0.03))), float(F(0.05))
    m = nr.cloud_metrics(pred, gt, 0.05)
    assert m["n_pred"] == 407 and m["unmatched_pred"] == 7 and m["unmatched_gt"] == 0 and m["within_pred"] == [400]
    assert m["accuracy"] == pytest.approx((400 * d + 7 * r) / 407, rel=1e-12) and m["completeness"] == pytest.approx(d, rel=1e-12)
    assert m["precision"] == [400 / 407] and m["recall"] == [1.0]
    assert m["fscore"][0] == pytest.approx(2 * (400 / 407) / (400 / 407 + 1), rel=1e-15)
    mask = np.ones(407, bool)
    mask[400:] = False
    pred[3] = NAN
    m = nr.cloud_metrics(pred, gt, 0.05, pred_mask=mask)
    assert m["n_pred"] == 399 and m["unmatched_pred"] == 0 and m["unmatched_gt"] == 1 and m["recall"] == [399 / 400]
    assert np.isnan(m["pred_dist"][[3, 400, 406]]).all() and m["gt_dist"][3] == F(0.05)


def test_fscore_is_zero_when_nothing_matches():
    m = nr.cloud_metrics(FAR, planar_grid(), 0.05)
    assert m["precision"] == [0.0] and m["recall"] == [0.0] and m["fscore"] == [0.0]
    assert m["unmatched_pred"] == 7 and m["unmatched_gt"] == 400
    for k in ("accuracy", "completeness", "chamfer"):
        assert m[k] == pytest.approx(float(F(0.05)), rel=1e-12), k


# ---- outliers ----------------------------------------------------------------------------------------------------------------------------
def test_outliers_of_a_planar_grid_with_isolated_points():
    """At radius 0.15 a grid point of spacing 0.1 has its 4 (edge: 3, corner: 2) axis neighbours and the diagonal ones at 0.1414: 8 / 5 / 3."""
    pts = np.concatenate([planar_grid(), FAR])
    count = nr.query(pts, pts, 0.15, exclude_same_row=True)["count"]
    assert sorted(set(count[:400].tolist())) == [3, 5, 8] and (count[400:] == 0).all()
    for k, kept in ((0, 407), (1, 400), (3, 400), (4, 396), (6, 324), (9, 0)):
        keep = nr.radius_outliers(pts, 0.15, k)
        assert keep.dtype == bool and int(keep.sum()) == kept and (k == 0 or not keep[400:].any()), k
    mask = np.ones(407, bool)
    mask[:20] = False                                                               # the first grid row takes no part: the second becomes an edge
    keep = nr.radius_outliers(pts, 0.15, 4, mask)
    assert not keep[:20].any() and int(keep.sum()) == 19 * 20 - 4


# ---- ABI and host ------------------------------------------------------------------------------------------------------------------------
def test_symbols_agree_between_header_binding_and_library():
    from geo4d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geo4d_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.geo4d_abi_version() == _lib.ABI_VERSION == 9 == int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1))


def test_bad_arguments_are_refused_on_the_host():
    """Every refusal is -EINVAL with the function's name in the message and comes before any device work: the pointers below are not
    device memory."""
    from geo4d_amd import _lib
    lib = _lib.load()
    bufs = [(ctypes.c_double * 64)() for _ in range(10)]
    a, b, c, d, e, f, g, h, i, j = (ctypes.addressof(x) for x in bufs)
    big = 1 << 31
    radii = [dict(radius=v) for v in (0.0, -1.0, NAN, INF, 1e39, 1e30)]             # 1e39 is inf in fp32; 1e30 squared is

    def keys(points=a, mask=None, N=10, radius=1.0, out=b, dropped=c):
        return lib.geo4d_nn_keys(points, mask, N, radius, out, dropped, None)

    for kw in [dict(points=None), dict(out=None), dict(dropped=None), dict(dropped=None, N=0), dict(N=-1), dict(N=big), dict(out=a),
               dict(dropped=a), dict(dropped=b), dict(mask=b), dict(mask=c)] + radii:
        assert keys(**kw) == -22 and b"nn_keys" in lib.geo4d_last_error(), kw

    def gather(points=a, order=b, Nt=5, N=10, out=c, rows=d):
        return lib.geo4d_nn_gather(points, order, Nt, N, out, rows, None)

    for kw in [dict(points=None), dict(order=None), dict(out=None), dict(rows=None), dict(Nt=-1), dict(Nt=11), dict(N=-1), dict(N=big),
               dict(out=a), dict(out=b), dict(rows=a), dict(rows=b), dict(rows=c)]:
        assert gather(**kw) == -22 and b"nn_gather" in lib.geo4d_last_error(), kw
    assert gather(Nt=0) == 0 and gather(Nt=0, N=0, points=None, order=None, out=None, rows=None) == 0

    def query(query=a, order=b, taking=5, Nq=10, cell_keys=c, cell_start=d, M=3, ref=e, rows=f, Nt=4, Nr=5, radius=1.0, excl=0, index=g,
              dist2=h, count=i):
        return lib.geo4d_nn_query(query, order, taking, Nq, cell_keys, cell_start, M, ref, rows, Nt, Nr, radius, excl, index, dist2, count, None)

    inputs = (a, b, c, d, e, f)
    for kw in [dict(query=None), dict(order=None), dict(cell_keys=None), dict(cell_start=None), dict(ref=None), dict(rows=None),
               dict(index=None), dict(dist2=None), dict(count=None), dict(taking=-1), dict(taking=11), dict(Nq=-1), dict(Nq=big), dict(M=-1),
               dict(M=5), dict(Nt=6), dict(Nt=-1, M=-1), dict(Nr=big), dict(Nr=-1), dict(excl=2), dict(excl=-1), dict(index=h), dict(index=i),
               dict(dist2=i)] + radii + [{out: p} for out in ("index", "dist2", "count") for p in inputs]:
        assert query(**kw) == -22 and b"nn_query" in lib.geo4d_last_error(), kw
    # nothing to do is no error and no launch
    assert query(Nq=0, taking=0) == 0 and query(Nq=0, taking=0, query=None, order=None, index=None, dist2=None, count=None) == 0


def test_python_refusals_come_before_any_device_work(tmp_path):
    import torch
    from geo4d_amd import _lib, evaluation, fusion, nearest, ops
    from geo4d_amd.scene_export import get_3D_model_from_scene, save_scene
    pts = torch.zeros((4, 3))
    grid = ops.NNGrid(1.0, torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros((0, 3)),
                      torch.zeros(0, dtype=torch.int32), 0, 0, 0, pts.device)
    for call in (lambda: ops.nn_grid(pts, radius=1.0), lambda: ops.nn_query(grid, pts), lambda: nearest.build_grid(pts, radius=1.0),
                 lambda: nearest.nearest_points(pts, pts, radius=1.0), lambda: nearest.nearest_points(pts, grid=grid, radius=1.0),
                 lambda: nearest.radius_outliers(pts, radius=1.0, min_neighbours=1), lambda: evaluation.cloud_metrics(pts, pts, max_dist=1.0),
                 lambda: fusion.fuse_points(pts, voxel=1.0, min_neighbours=2)):
        with pytest.raises(_lib.Geo4DNativeError, match="no CPU fallback"):
            call()
    for r in (0, -1.0, NAN, INF, 1e39, 1e30, None, "wide"):
        for call in (lambda: nearest.build_grid(pts, radius=r), lambda: nearest.nearest_points(pts, pts, radius=r),
                     lambda: nearest.radius_outliers(pts, radius=r, min_neighbours=1)):
            with pytest.raises(ValueError, match="radius must be finite and > 0"):
                call()
        with pytest.raises(ValueError, match="max_dist must be finite and > 0"):
            evaluation.cloud_metrics(pts, pts, max_dist=r)
        if r is not None:
            with pytest.raises(ValueError, match="neighbour_radius must be finite and > 0"):
                fusion.fuse_points(pts, voxel=1.0, min_neighbours=1, neighbour_radius=r)
    for k in (-1, 1.5, True, None, "2"):
        with pytest.raises(ValueError, match="min_neighbours must be an integer >= 0"):
            nearest.radius_outliers(pts, radius=1.0, min_neighbours=k)
        with pytest.raises(ValueError, match="min_neighbours must be an integer >= 0"):
            fusion.fuse_points(pts, voxel=1.0, min_neighbours=k)
        with pytest.raises(ValueError, match="min_neighbours must be an integer >= 0"):
            fusion.fuse_scene(object(), min_neighbours=k)
        with pytest.raises(ValueError, match="min_neighbours must be an integer >= 0"):
            get_3D_model_from_scene(str(tmp_path), True, None, as_pointcloud=True, fuse_voxel=0.1, fuse_min_neighbours=k)
    with pytest.raises(ValueError, match="either `reference` or `grid`, not both"):
        nearest.nearest_points(pts, pts, grid=grid, radius=1.0)
    with pytest.raises(ValueError, match="either `reference` or `grid`, not neither"):
        nearest.nearest_points(pts, radius=1.0)
    for bad in (torch.zeros(4), torch.zeros((4, 2)), torch.zeros((2, 4, 3))):
        with pytest.raises(ValueError, match=r"need query \[N, 3\]"):
            nearest.nearest_points(bad, pts, radius=1.0)
        with pytest.raises(ValueError, match=r"need points \[N, 3\]"):
            nearest.radius_outliers(bad, radius=1.0, min_neighbours=1)
        with pytest.raises(ValueError, match=r"need pred \[N, 3\]"):
            evaluation.cloud_metrics(bad, pts, max_dist=1.0)
        with pytest.raises(ValueError, match=r"need gt \[N, 3\]"):
            evaluation.cloud_metrics(pts, bad, max_dist=1.0)
    with pytest.raises(ValueError, match=r"query_mask must be \[N\]"):
        nearest.nearest_points(pts, pts, radius=1.0, query_mask=torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"pred_mask must be \[N\]"):
        evaluation.cloud_metrics(pts, pts, max_dist=1.0, pred_mask=torch.ones(5, dtype=torch.bool))
    for ts in ((), (0.0,), (-0.1,), (0.5, 1.5), ("a",), (NAN,)):
        with pytest.raises(ValueError, match="thresholds must be"):
            evaluation.cloud_metrics(pts, pts, max_dist=1.0, thresholds=ts)
    with pytest.raises(ValueError, match="motion must be one of"):
        evaluation.scene_cloud_metrics(object(), pts, max_dist=1.0, motion="moving")
    with pytest.raises(ValueError, match="`transform` or `gt_traj`, not both"):
        evaluation.scene_cloud_metrics(object(), pts, max_dist=1.0, transform=np.eye(4), gt_traj=[np.zeros((2, 7)), np.arange(2.0)])
    with pytest.raises(ValueError, match="finite 4 x 4"):
        evaluation.scene_cloud_metrics(object(), pts, max_dist=1.0, transform=np.eye(3))
    # the export's two arguments belong to the fused cloud alone
    for kw in (dict(fuse_min_neighbours=2), dict(fuse_neighbour_radius=0.1)):
        for more in (dict(as_pointcloud=True), dict(as_pointcloud=True, tsdf_voxel=0.1), dict(as_pointcloud=False, tsdf_mesh=0.1)):
            with pytest.raises(ValueError, match="they need fuse_voxel"):
                get_3D_model_from_scene(str(tmp_path), True, None, **kw, **more)
        assert get_3D_model_from_scene(str(tmp_path), True, None, as_pointcloud=True, fuse_voxel=0.1, **kw) is None
        with pytest.raises(ValueError, match="they need fuse_static"):
            save_scene(object(), str(tmp_path / "scene"), "seq", **kw)
    assert os.listdir(tmp_path) == ["scene"] and os.listdir(tmp_path / "scene") == ["seq"] and os.listdir(tmp_path / "scene" / "seq") == []
    for fn, a, b in ((fusion.fuse_points, "min_neighbours", "neighbour_radius"), (fusion.fuse_scene, "min_neighbours", "neighbour_radius"),
                     (get_3D_model_from_scene, "fuse_min_neighbours", "fuse_neighbour_radius")):
        par = inspect.signature(fn).parameters
        assert par[a].default == 0 and par[b].default is None, fn


def test_sim3_helper_leaves_eval_metrics_as_it_was():
    """trajectory_sim3 is the (s, R, T) eval_metrics aligns with: a trajectory moved by a known sim(3) comes back, and the ATE is ~0."""
    from scipy.spatial.transform import Rotation
    from geo4d_amd import evaluation
    g = np.random.default_rng(2)
    n = 9
    pos = g.uniform(-1, 1, size=(n, 3))
    quat = Rotation.random(n, random_state=4).as_quat()                              # x y z w
    gt = np.concatenate([pos, quat[:, [3, 0, 1, 2]]], 1)
    s, R, T = 1.7, Rotation.from_euler("xyz", [0.3, -0.2, 0.5]).as_matrix(), np.array([0.4, -1.0, 2.0])
    est_pos = (pos - T) @ R / s                                                     # gt = s R est + T
    est_rot = Rotation.from_matrix(R.T @ Rotation.from_quat(quat).as_matrix()).as_quat()
    est = np.concatenate([est_pos, est_rot[:, [3, 0, 1, 2]]], 1)
    stamps = np.arange(n, dtype=np.float64)
    M = evaluation.trajectory_sim3([est, stamps], [gt, stamps])
    assert M.shape == (4, 4) and np.allclose(M[:3, :3], s * R, atol=1e-9) and np.allclose(M[:3, 3], T, atol=1e-9) and M[3].tolist() == [0, 0, 0, 1]
    ate, rpe_t, rpe_r = evaluation.eval_metrics([est, stamps], [gt, stamps])
    assert ate < 1e-9 and rpe_t < 1e-9 and rpe_r < 1e-4
    assert math.isclose(np.linalg.det(M[:3, :3]), s ** 3, rel_tol=1e-9)
