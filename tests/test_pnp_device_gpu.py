"""Batched RANSAC-PnP on the HIP path (csrc/pnp.hip, ops.pnp_ransac) and the initialisations built on it
(GroupAligner.init_from_group(pose_init="pnp" | "prefix", pnp_backend="device")). The oracle is the host solver geo4d_amd/pnp.py run on the
same sampler tables (pnp.sample_tables), closed-form scenes with known poses, and the two reference fixtures - never the device code.

Exact integers. The device mirrors the host hypothesis for hypothesis, so the success flag, the RANSAC iterations run, the chosen
hypothesis and both inlier counts must be EQUAL. That needs every masked point to sit clear of the threshold under the host's accepted
model; each scene asserts a margin of at least 1e-6 px there (the two solvers differ by rounding only, see below).

Parity bound (PARITY). Device and host differ in reduction order, in Jacobi versus LAPACK for the small SVDs, and in the refit's moment
form. Measured on the first MI355X run over the eight scenes of the parity test: max |R_dev - R_host| = 3.58e-15, max |t_dev - t_host| =
1.25e-14 (MEASURED_R, MEASURED_T below; also in profiles/pnp_device.md). PARITY is ten times the larger one and never looser than 1e-6, i.e. ten times tighter than
the bar against the truth (1e-5 on R, 1e-4 on t, from tests/test_pnp_cpu.py), so the comparison stays meaningful.
Through the integration the poses and focals pass through fp32 parameters, so every entry of a.P is compared with the host backend's
at the absolute bound max(PARITY, 1e-6) (measured: 0, the fp64 results round to the same fp32 values)."""
import math
import os

import numpy as np
import pytest
import torch

from geo4d_amd import pnp

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEASURED_R, MEASURED_T = 3.6e-15, 1.3e-14                      # first MI355X run, see the module docstring
PARITY = min(10 * max(MEASURED_R, MEASURED_T), 1e-6)
P_TOL = max(PARITY, 1e-6)
ITER = 60


def _rot(rng):
    ang = rng.uniform(-0.4, 0.4, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])


def _map(H, W, f, seed, planar=False, outliers=0.3, low_conf=0.2):
    """A point map = depth times the pixel grid under a known pose: (points fp32 [H, W, 3] in the world, conf fp32 [H, W], R, t world ->
    camera). `outliers` of the points are displaced grossly (1 .. 3 units sideways in the camera frame: at least 10 px at these depths and
    focals, so none can pass a 5 px threshold), `low_conf` of the confidences are below 0.5."""
    rng = np.random.default_rng(seed)
    depth = 3.0 + 0.3 * np.arange(W)[None, :] / W + np.zeros((H, 1)) if planar else rng.uniform(2.0, 6.0, (H, W))
    grid = pnp.pixel_grid(H, W).astype(np.float64)
    cam = np.concatenate([(grid - [W / 2, H / 2]) / f * depth[..., None], depth[..., None]], -1)
    bad = rng.uniform(size=(H, W)) < outliers
    cam[bad, :2] += rng.uniform(1.0, 3.0, (int(bad.sum()), 2)) * rng.choice([-1.0, 1.0], (int(bad.sum()), 2))
    R, t = _rot(rng), rng.uniform(-0.5, 0.5, 3)
    pts = (cam - t) @ R                                               # X = R^T (Xc - t)
    conf = np.where(rng.uniform(size=(H, W)) < low_conf, 0.2, 1.5)
    return pts.astype(np.float32), conf.astype(np.float32), R, t


def _host_trace(X, pix, K, iterations, reproj, max_points):
    """pnp.solve_pnp_ransac, instrumented: the same loop on the same tables through the module's own functions, returning what the solver
    does not expose (iterations run, chosen hypothesis, sub-sample inliers); its pose must be the solver's to the bit."""
    n = len(X)
    sub, draws = pnp.sample_tables(n, iterations, 0, 6, max_points)
    ok, R, t, full = pnp.solve_pnp_ransac(X, pix, K, iterations=iterations, reproj=reproj, max_points=max_points, tables=(sub, draws))
    Xs, ps = X[sub], pix[sub]
    bs = np.concatenate([ps, np.ones((len(ps), 1))], 1) @ np.linalg.inv(K).T
    best, it, needed = (0, None, None, None, -1), 0, iterations
    while it < min(iterations, needed):
        it += 1
        Rh, th = pnp.pnp_orthogonal_iteration(Xs[draws[it - 1]], bs[draws[it - 1]], iters=15)
        inl = pnp.reprojection_error(Xs, ps, K, Rh, th) < reproj
        if int(inl.sum()) > best[0]:
            best = (int(inl.sum()), Rh, th, inl, it - 1)
            p_all = (best[0] / len(Xs)) ** 6
            needed = np.inf if p_all < 1e-9 else (0 if p_all >= 1 else np.log(1 - 0.99) / np.log(1 - p_all))
    out = dict(ok=ok, it=it, besti=best[4], n=n, tables=(sub, draws, n))
    if ok:
        Rr, tr, inl = best[1], best[2], best[3]
        for _ in range(2):
            R2, t2 = pnp.pnp_orthogonal_iteration(Xs[inl], bs[inl], R=Rr, t=None, iters=500)
            inl2 = pnp.reprojection_error(Xs, ps, K, R2, t2) < reproj
            if inl2.sum() < inl.sum():
                break
            Rr, tr, inl = R2, t2, inl2
        assert np.array_equal(Rr, R) and np.array_equal(tr, t)
        err = pnp.reprojection_error(X, pix, K, R, t)
        out.update(R=R, t=t, sub_inl=int(inl.sum()), full=len(full), margin=float(np.abs(err[np.isfinite(err)] - reproj).min()))
    return out


def _masked(pts, conf):
    H, W = conf.shape
    msk = conf > 0.5
    return pts[msk].astype(np.float64), pnp.pixel_grid(H, W)[msk].astype(np.float64)


def _device(dev, pts, conf, cands, tables, reproj=5.0, iterations=ITER, out=None):
    from geo4d_amd import ops
    pts, conf = torch.as_tensor(np.asarray(pts)), torch.as_tensor(np.asarray(conf))
    if pts.dim() == 3:
        pts, conf, tables = pts[None], conf[None], [tables]
    cand = torch.as_tensor(np.asarray(cands, np.float64).reshape(pts.shape[0], -1))
    return ops.pnp_ransac(pts.to(dev), conf.to(dev), cand.to(dev), tables, reproj=reproj, iterations=iterations, out=out)


def _w2c(c2w):
    R = c2w[:3, :3].T
    return R, -R @ c2w[:3, 3]


measured = {"R": 0.0, "t": 0.0}


@pytest.mark.parametrize("reproj", [5.0, 1.0])
@pytest.mark.parametrize("max_points", [4096, 1024])
@pytest.mark.parametrize("planar", [False, True])
def test_hypothesis_for_hypothesis_parity_with_the_host(dev, planar, max_points, reproj):
    """C = 1 on a 48 x 64 map, 30 % gross outliers, 20 % of conf below the threshold, n no multiple of 64; the planar map makes the DLT
    refuse (start from the identity). max_points 4096 scores all points, 1024 the sub-sample gather.
    Measured |device - host| on the first MI355X run: R 3.58e-15, t 1.25e-14 at most over the eight cases (MEASURED_R / MEASURED_T)."""
    H, W, f = 48, 64, 60.0
    pts, conf, R, t = _map(H, W, f, 3, planar)
    X, pix = _masked(pts, conf)
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    ref = _host_trace(X, pix, K, ITER, reproj, max_points)
    assert ref["n"] % 64 != 0 and 1024 < ref["n"] <= 4096              # 4096 scores every point, 1024 goes through the sub-sample
    assert ref["ok"] and ref["margin"] >= 1e-6, ref["margin"]          # exact counts are only meaningful clear of the threshold
    focal, c2w, status, info = _device(dev, pts, conf, [f], ref["tables"], reproj)
    info = info.cpu()[0, 0].tolist()
    print(f"[pnp parity planar={planar} max_points={max_points} reproj={reproj}] n {ref['n']} host (it, best, sub, full) "
          f"{(ref['it'], ref['besti'], ref['sub_inl'], ref['full'])} device {info} margin {ref['margin']:.3g} px")
    assert int(status[0]) == 0 and float(focal[0]) == f
    assert info == [ref["it"], ref["besti"], ref["sub_inl"], ref["full"]]
    Rd, td = _w2c(c2w[0].cpu().numpy())
    dR, dt = float(np.abs(Rd - ref["R"]).max()), float(np.abs(td - ref["t"]).max())
    measured["R"], measured["t"] = max(measured["R"], dR), max(measured["t"], dt)
    print(f"    |R - truth| {np.abs(Rd - R).max():.2e} |t - truth| {np.abs(td - t).max():.2e}; device - host: R {dR:.3e} t {dt:.3e} "
          f"(running max R {measured['R']:.3e} t {measured['t']:.3e}; bound {PARITY:.1e})")
    assert np.abs(Rd - R).max() < 1e-5 and np.abs(td - t).max() < 1e-4
    assert dR <= PARITY and dt <= PARITY


def _candidate_scene():
    """The 240 x 320, f = 260 scene of tests/test_pnp_cpu.py::test_fast_pnp_picks_the_focal_candidate_and_returns_cam_to_world."""
    H, W, f = 240, 320, 260.0
    rng = np.random.default_rng(5)
    depth = rng.uniform(2.0, 6.0, (H, W))
    grid = pnp.pixel_grid(H, W).astype(np.float64)
    cam = np.concatenate([(grid - [W / 2, H / 2]) / f * depth[..., None], depth[..., None]], -1)
    rng7 = np.random.default_rng(7)
    rng7.uniform(-1, 1, (4, 3))                                         # _scene(4, 7) draws its points first
    R = _rot(rng7)
    t = rng7.uniform(-0.5, 0.5, 3)
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = R.T, -R.T @ t
    pts = cam @ c2w[:3, :3].T + c2w[:3, 3]
    msk = rng.uniform(size=(H, W)) > 0.2
    return H, W, f, pts, msk, c2w


def test_candidate_choice_against_fast_pnp(dev):
    """Given f - 0.03 S the device returns exactly the +3 % candidate and the true pose; host fast_pnp agrees on the focal, and the host
    solver on each candidate's full inlier count."""
    H, W, f, pts, msk, c2w = _candidate_scene()
    S, n, it = max(H, W), int(msk.sum()), 100
    guess = f - 0.03 * S
    cands = [guess, -0.03 * S + guess, 0.03 * S + guess]
    conf = np.where(msk, 1.0, 0.0).astype(np.float32)
    focal, pose, status, info = _device(dev, pts.astype(np.float32), conf, cands, pnp.sample_tables(n, it) + (n,), iterations=it)
    host = pnp.fast_pnp(pts.astype(np.float32), guess, msk, niter_PnP=it)
    assert int(status[0]) == 0 and float(focal[0]) == cands[2] and host is not None and host[0] == cands[2]
    assert abs(float(focal[0]) - f) < 1e-9
    X, pix = pts.astype(np.float32)[msk].astype(np.float64), pnp.pixel_grid(H, W)[msk].astype(np.float64)
    full = []
    for fc in cands:
        K = np.array([[fc, 0, W / 2], [0, fc, H / 2], [0, 0, 1.0]])
        ok, _, _, inl = pnp.solve_pnp_ransac(X, pix, K, iterations=it)
        full.append(len(inl) if ok else 0)
    print(f"[pnp candidates] full inlier counts host {full} device {info.cpu()[0, :, 3].tolist()}; |pose - truth| {np.abs(pose[0].cpu().numpy() - c2w).max():.2e}")
    assert info.cpu()[0, :, 3].tolist() == full
    assert np.abs(pose[0].cpu().numpy() - c2w).max() < 1e-5 and np.abs(pose[0].cpu().numpy() - host[1]).max() <= P_TOL


def test_ties_go_to_the_first_candidate(dev):
    """24 x 32, exact points: -/+ 3 % of the image size moves no pixel by 5 px, so all three candidates count every masked pixel."""
    H, W, f = 24, 32, 30.0
    pts, conf, R, t = _map(H, W, f, 11, outliers=0.0)
    n = int((conf > 0.5).sum())
    cands = [f, -0.03 * W + f, 0.03 * W + f]
    focal, pose, status, info = _device(dev, pts, conf, cands, pnp.sample_tables(n, ITER) + (n,))
    full = info.cpu()[0, :, 3].tolist()
    assert int(status[0]) == 0 and full == [n, n, n], full
    assert float(focal[0]) == f
    host = pnp.fast_pnp(pts, f, conf > 0.5, niter_PnP=ITER)
    assert host[0] == f and np.abs(pose[0].cpu().numpy() - host[1]).max() <= P_TOL


def test_failure_contract_in_one_launch(dev):
    """B = 4: 3 masked pixels, 5 masked pixels, pure noise, one good image. Failures set their bit and leave the caller's focal and pose
    alone; the good image is what it is alone; nothing is NaN; a NaN candidate sets its own bit."""
    from geo4d_amd import ops
    H, W, f = 24, 32, 30.0
    good, gconf, R, t = _map(H, W, f, 12)
    rng = np.random.default_rng(13)
    pts = np.stack([good, good, rng.normal(size=(H, W, 3)).astype(np.float32), good])
    conf = np.stack([np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), np.ones((H, W), np.float32), gconf])
    conf[0].reshape(-1)[[5, 100, 700]] = 1.0
    conf[1].reshape(-1)[[5, 100, 300, 500, 700]] = 1.0
    ns = [int((c > 0.5).sum()) for c in conf]
    assert ns[:2] == [3, 5]
    tables = [pnp.sample_tables(n, ITER) + (n,) for n in ns]
    cands = np.tile([f, -0.03 * W + f, 0.03 * W + f], (4, 1))
    focal = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    pose = torch.full((4, 4, 4), -7.0, dtype=torch.float64, device=dev)
    _, _, status, info = _device(dev, pts, conf, cands, tables, out=(focal, pose))
    status = status.cpu().tolist()
    print(f"[pnp failure contract] status {status}")
    assert status[0] == ops.PNP_FEW and status[1] == ops.PNP_FEW and status[3] == 0 and status[2] in (0, ops.PNP_NO_CONSENSUS)
    for b in range(4):
        if status[b]:
            assert bool((focal[b] == -7.0).all()) and bool((pose[b] == -7.0).all())
    assert bool(torch.isfinite(focal).all()) and bool(torch.isfinite(pose).all())
    f1, p1, s1, i1 = _device(dev, pts[3], conf[3], cands[3], tables[3])
    assert int(s1[0]) == 0 and torch.equal(f1[0], focal[3]) and torch.equal(p1[0], pose[3]) and torch.equal(i1[0], info[3])
    Rd, td = _w2c(pose[3].cpu().numpy())
    assert np.abs(Rd - R).max() < 1e-5 and np.abs(td - t).max() < 1e-4
    bad = cands.copy()
    bad[2, 1] = float("nan")
    bad[0, 0] = -1.0
    f2, p2, s2, _ = _device(dev, pts, conf, bad, tables)
    s2 = s2.cpu().tolist()
    assert s2[2] & ops.PNP_BAD_FOCAL and s2[0] & ops.PNP_BAD_FOCAL and s2[3] == 0 and torch.equal(f2[3], focal[3]) and torch.equal(p2[3], pose[3])
    assert bool(torch.isnan(f2[2])) and bool(torch.isnan(p2[2]).all())              # fresh outputs: the unset marker, never written
    # tables drawn for another count are refused, not followed out of bounds
    _, _, s3, _ = _device(dev, pts[3], conf[3], cands[3], pnp.sample_tables(ns[3] + 9, ITER) + (ns[3] + 9,))
    assert int(s3[0]) == ops.PNP_BAD_TABLES


def test_two_runs_are_bit_identical(dev):
    H, W, f = 48, 64, 60.0
    a, ca, _, _ = _map(H, W, f, 21)
    b, cb, _, _ = _map(H, W, f, 22, planar=True)
    ns = [int((c > 0.5).sum()) for c in (ca, cb)]
    tables = [pnp.sample_tables(n, ITER, 0, 6, 1024) + (n,) for n in ns]
    cands = np.tile([f, -0.03 * W + f, 0.03 * W + f], (2, 1))
    one = _device(dev, np.stack([a, b]), np.stack([ca, cb]), cands, tables)
    two = _device(dev, np.stack([a, b]), np.stack([ca, cb]), cands, tables)
    assert one[2].cpu().tolist() == [0, 0]
    assert all(torch.equal(x, y) for x, y in zip(one, two))


# ---- through the integration ---------------------------------------------------------------------------------------------------------
def _aligner(groups, pred, conf, dev):
    from geo4d_amd.align import GroupAligner
    return GroupAligner(groups, pred.to(dev), conf.squeeze(-1).to(dev), shared_focal=True, temporal_smoothing_weight=0.015, translation_weight=1.0)


def _vs_reference(a, ref, what):
    got = {k: a.P[k].detach().cpu() for k in ref}
    for k in ("im_poses", "pw_poses"):                      # quaternions are defined up to sign
        sign = torch.sign((got[k][:, :4] * ref[k][:, :4]).sum(1, keepdim=True))
        got[k] = torch.cat([got[k][:, :4] * sign, got[k][:, 4:]], 1)
    errs = {k: float((got[k].reshape(ref[k].shape) - ref[k]).abs().max()) for k in ref}
    print(f"[{what}, device backend vs reference] {errs}")
    assert errs["im_focals"] < 1e-3 and errs["pw_poses"] < 2e-3 and errs["im_poses"] < 5e-3 and errs["im_depthmaps"] < 5e-3, errs


def _vs_host_backend(a, b, what):
    worst = 0.0
    for k in a.P:
        x, y = a.P[k].detach().cpu().double(), b.P[k].detach().cpu().double()
        worst = max(worst, float((x - y).abs().max()))
    print(f"[{what}] device vs host backend: max absolute parameter difference {worst:.3e} (tol {P_TOL:.1e})")
    assert worst <= P_TOL
    assert torch.equal(a.pnp_status == 0, b.pnp_status == 0) and torch.equal(a.pnp_status == -1, b.pnp_status == -1)


def test_pnp_fixture_through_the_device_backend(dev):
    """tests/test_align_gpu.py::test_pnp_initialisation_vs_the_reference_init_from_group with pnp_backend="device", same thresholds."""
    g = torch.load(os.path.join(G, "pnp_init_tiny.pt"), weights_only=False)
    Gn, S, H, W, _ = g["pred"].shape
    rays = g["rays"].expand(Gn, S, H, W, 3).to(dev)
    a = _aligner(g["groups"], g["pred"], g["conf"], dev)
    a.init_from_group(None, raymaps=rays, pose_init="pnp", niter_PnP=g["niter_PnP"], pnp_backend="device")
    _vs_reference(a, g["after_init"], "pnp init")
    loss = float(a.loss_and_grads()[0])
    assert abs(loss - g["loss"]) < 0.05 * g["loss"] + 1e-4
    b = _aligner(g["groups"], g["pred"], g["conf"], dev)
    b.init_from_group(None, raymaps=rays, pose_init="pnp", niter_PnP=g["niter_PnP"])
    _vs_host_backend(a, b, "pnp init")
    assert int((a.pnp_status >= 0).sum()) == 10 and int((a.pnp_status == 0).sum()) == 10      # every image solved once, none failed


@pytest.mark.parametrize("key", ["prefix", "outlier"])
def test_prefix_fixture_through_the_device_backend(dev, key):
    """tests/test_focal_shift_gpu.py::test_prefix_initialisation_vs_the_reference_init_from_group and
    ::test_prefix_initialisation_replaces_an_outlier_window_focal with pnp_backend="device", same thresholds."""
    fix = torch.load(os.path.join(G, "prefix_init.pt"), weights_only=False)
    p, o = fix["prefix"], fix["outlier"]
    pred = p["pred"].clone()
    if key == "outlier":
        pred[o["window"], 0] = o["frame"]
    a = _aligner(p["groups"], pred, p["conf"], dev)
    a.init_from_group(None, pose_init="prefix", niter_PnP=p["niter_PnP"], pnp_backend="device")
    if key == "prefix":
        tol_f = max(10 * p["focal_group_gap"], 2e-5)
        assert float((a.prefix_focals_raw / p["focal_group_before"] - 1).abs().max()) <= tol_f
        _vs_reference(a, p["after_init"], "prefix init")
        loss = float(a.loss_and_grads()[0])
        assert abs(loss - p["loss"]) < 0.05 * p["loss"]
    else:
        tol_f = max(10 * o["focal_group_gap"], 2e-5)
        assert float((a.prefix_focals_raw / o["focal_group_before"] - 1).abs().max()) <= tol_f
        assert float((a.prefix_focals / o["focal_group_after"] - 1).abs().max()) <= tol_f
        assert float(a.prefix_focals[o["window"]]) > 2 * float(a.prefix_focals_raw[o["window"]])
        assert float((a.P["im_focals"].cpu().reshape(o["im_focals"].shape) - o["im_focals"]).abs().max()) < 1e-3
    b = _aligner(p["groups"], pred, p["conf"], dev)
    b.init_from_group(None, pose_init="prefix", niter_PnP=p["niter_PnP"])
    _vs_host_backend(a, b, f"prefix init ({key})")
    assert int((a.pnp_status == 0).sum()) == 16


def test_a_chain_that_actually_chains(dev):
    """The prefix fixture's geometry with noise (0.002 x extent), 15 % outliers, 20 % of conf below the threshold and ONE slot without any
    confidence (outliers on every frame but the windows' reference frames): its PnP fails, its image keeps the pose and focal of the earlier window, and the next image starts from that focal. Host
    and device backends agree on every status, on the per-image focals and on a.P."""
    fix = torch.load(os.path.join(G, "prefix_init.pt"), weights_only=False)
    p = fix["prefix"]
    gen = torch.Generator().manual_seed(31)
    pred, conf = p["pred"].clone(), p["conf"].clone()
    extent = float(pred.reshape(-1, 3).max(0).values.sub(pred.reshape(-1, 3).min(0).values).max())
    pred += 0.002 * extent * torch.randn(pred.shape, generator=gen)
    bad = torch.rand(pred.shape[:-1], generator=gen) < 0.15
    bad[:, 0] = False                 # the window focals come from a least-squares fit of the reference frames (no outlier rejection, not under test)
    pred[bad] += (torch.rand((int(bad.sum()), 3), generator=gen) - 0.5) * extent
    conf[torch.rand(conf.shape, generator=gen) < 0.2] = 0.1
    g_fail, k_fail = 1, 1
    img = p["groups"][g_fail][k_fail]
    assert img in p["groups"][0] and p["groups"][g_fail][k_fail + 1] == img + 1 and all(img not in grp for grp in p["groups"][2:])
    conf[g_fail, k_fail] = 0.0
    runs = {}
    for backend in ("host", "device"):
        a = _aligner(p["groups"], pred, conf, dev)
        a.init_from_group(None, pose_init="prefix", niter_PnP=p["niter_PnP"], pnp_backend=backend)
        runs[backend] = a
    h, d = runs["host"], runs["device"]
    print(f"[pnp chain] status host {h.pnp_status.tolist()} device {d.pnp_status.tolist()}; focals {d.init_focals.tolist()}")
    assert int(d.pnp_status[g_fail, k_fail]) == 1 and int(h.pnp_status[g_fail, k_fail]) == 1       # PNP_FEW on the device, "failed" on the host
    assert int((d.pnp_status == 0).sum()) >= 12                                                   # the rest of the chain ran and mostly solved
    ef = float((d.init_focals / h.init_focals - 1).abs().max())
    print(f"    per-image focals: max relative difference {ef:.3e}")
    assert ef <= P_TOL
    _vs_host_backend(d, h, "noisy prefix chain")
    from geo4d_amd.align import rotmat_to_quat
    ident = rotmat_to_quat(torch.eye(3)).cpu()
    moved = max(float((d.P["im_poses"][img, :4].cpu() - ident).abs().max()), float(d.P["im_poses"][img, 4:7].abs().max()))
    assert moved > 1e-4                                                # the earlier window's pose, not the identity of an unset image


def test_an_unusable_start_focal_falls_back_to_the_host_backend(dev, monkeypatch):
    """pose_init="pnp" without ray maps leaves every image without a base focal, where the host searches 63 candidates. The device backend
    reports the unusable focal and the whole initialisation reruns through the host solver (stubbed here: the search itself is
    tests/test_pnp_cpu.py's subject and takes seconds)."""
    calls = []
    monkeypatch.setattr(pnp, "fast_pnp", lambda pts3d, focal, msk, **kw: calls.append(focal))
    g = torch.load(os.path.join(G, "pnp_init_tiny.pt"), weights_only=False)
    a = _aligner(g["groups"], g["pred"], g["conf"], dev)
    a.init_from_group(None, pose_init="pnp", niter_PnP=5, pnp_backend="device")
    assert len(calls) == 16 and all(f is None for f in calls)                  # every slot, without a focal: the host path ran
    assert int((a.pnp_status == 1).sum()) == 16 and bool(torch.isfinite(a.P["im_poses"]).all())
