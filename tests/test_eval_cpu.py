"""Host side of the ground-truth evaluation (geo4d_amd/evaluation.py, geo4d_amd/io.py readers): the readers against the reference's
own outputs on tiny files (tests/golden/generate_eval.py), eval_metrics (evo's sim(3)-aligned ATE / RPE, restated) on closed-form
cases and against an independent fp64 Umeyama, and the valid-pixel weighting of average_depth_metrics."""
import os

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IO = os.path.join(G, "eval_io")


@pytest.fixture(scope="module")
def fix():
    return torch.load(os.path.join(G, "depth_eval.pt"), weights_only=False)["io"]


def test_depth_readers_match_reference(fix):
    from geo4d_amd import io
    d = io.depth_read_sintel(os.path.join(IO, "depth.dpt"))
    assert d.dtype == np.float32 and np.array_equal(d, fix["sintel"].numpy())
    for name, reader in (("bonn", io.depth_read_bonn), ("kitti", io.depth_read_kitti)):
        d = reader(os.path.join(IO, f"{name}.png"))
        assert d.dtype == np.float64 and np.array_equal(d, fix[name].numpy()), name
        assert (d == -1.0).sum() == 2                     # the two zero pixels of each file: missing -> -1


def test_sintel_cam_and_trajectory_match_reference(fix, tmp_path):
    from geo4d_amd import io
    M, N = io.sintel_cam_read(os.path.join(IO, "cams", "frame_0001.cam"))
    assert np.array_equal(M, fix["cam_M"].numpy()) and np.array_equal(N, fix["cam_N"].numpy())
    poses, stamps = io.load_traj(os.path.join(IO, "cams"), "sintel")
    assert np.allclose(poses, fix["traj_poses"].numpy(), rtol=0, atol=1e-12) and np.array_equal(stamps, fix["traj_stamps"].numpy())
    assert stamps.shape == (2, 1)


def test_tum_text_trajectory(tmp_path):
    from geo4d_amd import io
    p = tmp_path / "gt.txt"
    p.write_text("# timestamp tx ty tz qx qy qz qw\n1.5 1 2 3 0.1 0.2 0.3 0.9\n2.5 4 5 6 0 0 0 1\n")
    poses, stamps = io.load_traj(str(p), "tum")
    assert np.array_equal(stamps, [1.5, 2.5])
    assert np.array_equal(poses[0], [1, 2, 3, 0.9, 0.1, 0.2, 0.3])          # quaternion reordered to w x y z
    assert np.array_equal(io.load_traj(str(p), "tum", skip=1)[0], poses[1:])


# ---- eval_metrics ----------------------------------------------------------------------------------------------------------------
def _traj(n=12, seed=0):
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.normal(size=(n, 3)), 0)
    q = Rotation.random(n, random_state=seed).as_quat()
    return [np.concatenate([pos, q[:, [3, 0, 1, 2]]], 1), np.arange(n).astype(float)]


def _sim3(traj, s, R, t):
    pos = s * traj[0][:, :3] @ R.T + t
    q = (Rotation.from_matrix(R) * Rotation.from_quat(traj[0][:, [4, 5, 6, 3]])).as_quat()
    return [np.concatenate([pos, q[:, [3, 0, 1, 2]]], 1), traj[1].copy()]


def _perturb(traj, seed=3, sigma=0.05):
    rng = np.random.default_rng(seed)
    pos = traj[0][:, :3] + sigma * rng.normal(size=traj[0][:, :3].shape)
    q = (Rotation.from_rotvec(sigma * rng.normal(size=(len(pos), 3))) * Rotation.from_quat(traj[0][:, [4, 5, 6, 3]])).as_quat()
    return [np.concatenate([pos, q[:, [3, 0, 1, 2]]], 1), traj[1].copy()]


def _mats(traj):
    M = np.tile(np.eye(4), (len(traj[0]), 1, 1))
    M[:, :3, :3] = Rotation.from_quat(traj[0][:, [4, 5, 6, 3]]).as_matrix()
    M[:, :3, 3] = traj[0][:, :3]
    return M


def _umeyama(x, y):
    """Umeyama 1991 (evo geometry.umeyama_alignment), fp64: y ~ c R x + t."""
    mx, my = x.mean(0), y.mean(0)
    sx = np.mean(np.sum((x - mx) ** 2, 1))
    cov = (y - my).T @ (x - mx) / len(x)
    u, d, vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0:
        S[2, 2] = -1
    R = u @ S @ vt
    c = np.trace(np.diag(d) @ S) / sx
    return c, R, my - c * R @ mx


def _independent_metrics(est, ref):
    P, Q = _mats(est), _mats(ref)
    c, R, t = _umeyama(P[:, :3, 3], Q[:, :3, 3])
    A = P.copy()
    A[:, :3, :3] = R @ P[:, :3, :3]
    A[:, :3, 3] = c * P[:, :3, 3] @ R.T + t
    ate = np.sqrt(np.mean(np.sum((A[:, :3, 3] - Q[:, :3, 3]) ** 2, 1)))
    tr, rot = [], []
    for k in range(len(A) - 1):
        E = np.linalg.inv(np.linalg.inv(Q[k]) @ Q[k + 1]) @ np.linalg.inv(A[k]) @ A[k + 1]
        tr.append(np.linalg.norm(E[:3, 3]))
        rot.append(np.degrees(Rotation.from_matrix(E[:3, :3]).magnitude()))
    return ate, np.sqrt(np.mean(np.square(tr))), np.sqrt(np.mean(np.square(rot)))


def test_exact_sim3_gives_zero():
    from geo4d_amd.evaluation import eval_metrics
    ref = _traj()
    est = _sim3(ref, 0.37, Rotation.from_rotvec([0.3, -1.1, 0.4]).as_matrix(), np.array([5.0, -2.0, 1.0]))
    extent = np.ptp(ref[0][:, :3], 0).max()
    ate, rpe_t, rpe_r = eval_metrics(est, ref)
    assert ate < 1e-6 * extent and rpe_t < 1e-6 * extent and rpe_r < 1e-5


def test_invariant_under_sim3_of_estimate():
    from geo4d_amd.evaluation import eval_metrics
    ref = _traj(seed=1)
    est = _perturb(ref)
    base = np.array(eval_metrics(est, ref))
    assert base.min() > 0
    for s, rv, t in ((2.5, [0.1, 0.2, 0.3], [1, 2, 3]), (0.01, [-2.0, 0.5, 1.0], [-40, 0, 7])):
        moved = np.array(eval_metrics(_sim3(est, s, Rotation.from_rotvec(rv).as_matrix(), np.array(t, float)), ref))
        np.testing.assert_allclose(moved, base, rtol=1e-7, atol=0)


def test_single_rotated_frame_rpe_rot():
    from geo4d_amd.evaluation import eval_metrics
    ref = _traj(n=9, seed=2)
    est = [ref[0].copy(), ref[1].copy()]
    theta = 7.0
    q = (Rotation.from_rotvec(np.radians(theta) * np.array([0.0, 0.6, 0.8])) * Rotation.from_quat(est[0][4, [4, 5, 6, 3]])).as_quat()
    est[0][4, 3:] = q[[3, 0, 1, 2]]
    ate, rpe_t, rpe_r = eval_metrics(est, ref)
    n = len(ref[0])
    assert ate < 1e-9 and rpe_t > 0                # positions untouched; the pair translations are seen from the turned frame
    assert abs(rpe_r - theta * np.sqrt(2 / (n - 1))) < 1e-6


def test_matches_independent_umeyama(tmp_path):
    from geo4d_amd.evaluation import eval_metrics
    ref = _traj(n=20, seed=4)
    est = _sim3(_perturb(ref, seed=5, sigma=0.2), 1.7, Rotation.from_rotvec([1.0, 0.2, -0.5]).as_matrix(), np.array([0.0, 3.0, -1.0]))
    out = tmp_path / "metric.txt"
    got = eval_metrics(est, ref, seq="s", filename=str(out))
    np.testing.assert_allclose(got, _independent_metrics(est, ref), rtol=1e-9)
    assert out.read_text().startswith("Seq: s")
    # stride: every second pose of both trajectories
    np.testing.assert_allclose(eval_metrics(est, ref, sample_stride=2),
                               _independent_metrics([est[0][::2], est[1][::2]], [ref[0][::2], ref[1][::2]]), rtol=1e-9)


def test_estimate_timestamps_follow_reference_and_degenerate_raises():
    from geo4d_amd.evaluation import eval_metrics
    ref = _traj(n=6, seed=6)
    est = [ref[0].copy(), ref[1] * 10 + 100]                  # same length: the estimate takes the reference's stamps (vo_eval.py:200)
    assert max(eval_metrics(est, ref)) < 1e-5
    still = [np.tile(ref[0][:1], (6, 1)), ref[1]]
    with pytest.raises(ValueError):
        eval_metrics(still, ref)


def test_average_depth_metrics_weighting():
    from geo4d_amd.evaluation import average_depth_metrics
    a = {"Abs Rel": 0.1, "RMSE": 2.0, "valid_pixels": 300}
    b = {"Abs Rel": 0.4, "RMSE": 1.0, "valid_pixels": 100}
    avg = average_depth_metrics([a, b])
    assert set(avg) == {"Abs Rel", "RMSE"}
    assert abs(avg["Abs Rel"] - (0.1 * 300 + 0.4 * 100) / 400) < 1e-15 and abs(avg["RMSE"] - 1.75) < 1e-15


def test_depth_evaluation_refuses_cpu_and_unsupported_modes():
    from geo4d_amd import _lib
    from geo4d_amd.evaluation import depth_evaluation
    x = torch.ones(16)
    with pytest.raises(NotImplementedError):
        depth_evaluation(x, x, align_with_lstsq=True)
    with pytest.raises(NotImplementedError):
        depth_evaluation(x, x, disp_input=True)
    with pytest.raises(_lib.Geo4DNativeError):
        depth_evaluation(x, x, use_gpu=False)
