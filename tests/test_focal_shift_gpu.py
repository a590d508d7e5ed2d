"""Shift / focal recovery from point maps on the HIP path (csrc/focal_shift.hip, ops.focal_shift, geo4d_amd/geometry.py) and the
initialisation built on it (GroupAligner.init_from_group(pose_init="prefix")) against tests/golden/prefix_init.pt - the REFERENCE's
utils.geometry.point_map_to_depth and its init_from_group -> align_group_prefix (tests/golden/generate_prefix_init.py).

Tolerances of the solver tests. The reference stops its Levenberg-Marquardt at ftol = 1e-3, so it sits a little off the minimiser it
is heading for; the generator measures that distance against an fp64 exact minimiser (ref_gap = max |focal_ref / focal_exact - 1|).
The engine's focal must be within 10 x ref_gap of the reference's, with a floor of 2e-5 (10 x the gap first measured on such scenes).
The shift is an offset on z, so its error is measured against the mean depth z + shift of the selected pixels (d ln focal / d shift is
about 1 / depth: the same relative bound). Independently E(engine) <= E(reference) (1 + 1e-6) with E evaluated here in fp64."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fix():
    return torch.load(os.path.join(G, "prefix_init.pt"), weights_only=False)


def _selected(points, mask, size):
    """(xyz [n, 3], uv [n, 2]) fp64 of the pixels point_map_to_depth hands the solver for ONE map at `size`."""
    from geo4d_amd.geometry import image_plane_uv
    H, W = points.shape[0], points.shape[1]
    near = lambda t: F.interpolate(t.permute(2, 0, 1)[None], size, mode="nearest")[0].permute(1, 2, 0)
    sel = near(mask.float()[..., None])[..., 0] > 0
    return near(points)[sel].double(), near(image_plane_uv(W, H, dtype=torch.float32))[sel].double()


def _energy(xyz, uv, shift):
    p = xyz[:, :2] / (xyz[:, 2:3] + float(shift))
    a, b = (p * uv).sum(), (p * p).sum()
    return float((uv * uv).sum() - a * a / b)


def _check_case(case, size, tol, dev, what, **kw):
    from geo4d_amd import ops
    pts, mask, ref = case["points"], case["mask"], case["ref"][size]
    shift, focal, status = ops.focal_shift(pts.to(dev), mask.float().to(dev), 0.5, size, **kw)
    shift, focal, status = shift.cpu(), focal.cpu(), status.cpu()
    assert status.tolist() == [0] * pts.shape[0], status
    for b in range(pts.shape[0]):
        xyz, uv = _selected(pts[b], mask[b], size)
        depth = float((xyz[:, 2] + float(ref["shift"][b])).mean())
        ef = abs(float(focal[b]) / float(ref["focal"][b]) - 1)
        es = abs(float(shift[b]) - float(ref["shift"][b])) / depth
        e_ours, e_ref = _energy(xyz, uv, shift[b]), _energy(xyz, uv, ref["shift"][b])
        print(f"[focal_shift {what} {size} map {b}] {len(xyz)} pixels: focal {float(focal[b]):.7f} (reference {float(ref['focal'][b]):.7f}, rel {ef:.2e}), "
              f"shift {float(shift[b]):.7f} (reference {float(ref['shift'][b]):.7f}, / depth {es:.2e}), tol {tol:.1e}; E {e_ours:.9e} vs reference {e_ref:.9e}")
        assert ef <= tol and es <= tol, (what, size, b, ef, es, tol)
        assert e_ours <= e_ref * (1 + 1e-6), (what, size, b, e_ours, e_ref)
    return shift, focal


@pytest.mark.parametrize("name", ["24x32", "40x64_offset"])
def test_solver_vs_the_reference(fix, dev, name):
    case = fix["focal"]["cases"][name]
    H, W = case["points"].shape[1:3]
    _check_case(case, (H, W), max(10 * fix["focal"]["ref_gap"], 2e-5), dev, name)


def test_downsampled_solve_vs_the_reference(fix, dev):
    """(16, 16): F.interpolate(mode="nearest")'s source indices, non-integer ratios in both directions (24 / 16, 40 / 16)."""
    for name, case in fix["focal"]["cases"].items():
        _check_case(case, (16, 16), max(10 * fix["focal"]["ref_gap"], 2e-5), dev, name)


@pytest.mark.parametrize("name", ["3x5_one_masked", "24x32_65", "72x64_4097", "5_maps_counts"])
def test_smallest_shapes_that_can_go_wrong(fix, dev, name):
    """Fewer pixels than one wave (14); one more than a wave (65); one more than a block's 4096-pixel chunk (4097 selected of 72 x 64 - a
    24 x 32 map holds only 768 pixels - so two blocks feed one map); five maps with a different number of selected pixels each in one launch."""
    case = fix["shapes"]["cases"][name]
    H, W = case["points"].shape[1:3]
    assert int(case["mask"].sum()) == {"3x5_one_masked": 14, "24x32_65": 65, "72x64_4097": 4097, "5_maps_counts": 700 + 64 + 129 + 512 + 33}[name]
    _check_case(case, (H, W), max(10 * fix["shapes"]["ref_gap"], 2e-5), dev, name)


def test_strided_map_views_are_solved_in_place(fix, dev):
    """`pred[:, 0]` of a [G, S, H, W, 3] tensor and `conf[:, 0]`: a map stride that is not H W 3. Same bits as the contiguous call."""
    from geo4d_amd import ops
    case = fix["focal"]["cases"]["24x32"]
    pts, mask = case["points"].to(dev), case["mask"].float().to(dev)
    big = torch.full((3, 3, 24, 32, 3), float("nan"), device=dev)
    wbig = torch.full((3, 2, 24, 32), float("nan"), device=dev)
    big[:, 1], wbig[:, 1] = pts, mask
    view, wview = big[:, 1], wbig[:, 1]
    assert not view.is_contiguous() and view.stride(0) == 3 * 24 * 32 * 3
    a = ops.focal_shift(pts, mask, 0.5)
    b = ops.focal_shift(view, wview, 0.5)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[2].tolist() == [0, 0, 0]
    # z_offset: a device scalar added to every z moves the shift by exactly that much and leaves the focal alone
    off = torch.tensor([2.5], device=dev)
    c = ops.focal_shift(view, wview, 0.5, z_offset=off)
    assert float((c[0] + 2.5 - a[0]).abs().max()) < 1e-5 and float((c[1] / a[1] - 1).abs().max()) < 1e-6
    # no weight: every pixel
    d = ops.focal_shift(pts)
    e = ops.focal_shift(pts, torch.ones_like(mask), 0.5)
    assert all(torch.equal(x, y) for x, y in zip(d, e))


def test_degenerate_maps_do_not_disturb_their_neighbours(fix, dev):
    """An all-masked map (status != 0) and a constant-z plane facing the camera (the shift is unobservable: any answer, but a finite one)
    in one launch with two ordinary maps, which must come out exactly as they do on their own."""
    from geo4d_amd import ops
    from geo4d_amd.geometry import image_plane_uv
    case = fix["focal"]["cases"]["24x32"]
    H, W = 24, 32
    uv = image_plane_uv(W, H, dtype=torch.float32)
    plane = torch.cat([uv * 2.0 / 1.3, torch.full((H, W, 1), 2.0)], -1)
    pts = torch.stack([case["points"][0], case["points"][1], plane, case["points"][2]]).to(dev)
    mask = torch.stack([case["mask"][0], torch.zeros(H, W, dtype=torch.bool), torch.ones(H, W, dtype=torch.bool), case["mask"][2]]).float().to(dev)
    shift, focal, status = ops.focal_shift(pts, mask, 0.5)
    alone = ops.focal_shift(pts[[0, 3]], mask[[0, 3]], 0.5)
    print("[focal_shift degenerate] shift", shift.tolist(), "focal", focal.tolist(), "status", status.tolist())
    assert int(status[1]) != 0 and status[[0, 3]].tolist() == [0, 0]
    assert torch.isfinite(shift).all() and torch.isfinite(focal).all()
    assert torch.equal(shift[[0, 3]], alone[0]) and torch.equal(focal[[0, 3]], alone[1])
    # two selected pixels are still too few; non-finite coordinates under the mask are reported, not propagated
    mask2 = torch.zeros(1, H, W, device=dev)
    mask2[0, 3, 4] = mask2[0, 10, 20] = 1
    assert int(ops.focal_shift(pts[:1], mask2, 0.5)[2][0]) == 1
    bad = pts[:1].clone()
    bad[0, 5, 5, 0] = float("nan")
    s, f, st = ops.focal_shift(bad, torch.ones(1, H, W, device=dev), 0.5)
    assert int(st[0]) != 0 and torch.isfinite(s).all() and torch.isfinite(f).all()


@pytest.mark.parametrize("name", ["24x32", "40x64_offset"])
def test_point_map_to_depth_vs_the_reference(fix, dev, name):
    """depth, fov_x, fov_y, shift of utils.geometry.point_map_to_depth. fov = 2 atan(c / focal) moves by at most |d ln focal| radians
    (|d fov / d ln focal| = 2 x / (1 + x^2) <= 1), depth by the shift's error (+ one fp32 rounding of z + shift)."""
    from geo4d_amd import geometry
    case = fix["focal"]["cases"][name]
    pts, mask = case["points"], case["mask"]
    H, W = pts.shape[1:3]
    tol = max(10 * fix["focal"]["ref_gap"], 2e-5)
    fp32 = 1e-6                                             # a few ulps of the fp32 outputs (order 1) through atan and z + shift
    for size in ((H, W), (16, 16)):
        ref = case["ref"][size]
        depth, fov_x, fov_y, shift = geometry.point_map_to_depth(pts.to(dev), mask.to(dev), downsample_size=size)
        assert depth.shape == ref["depth"].shape and fov_x.shape == ref["fov_x"].shape and shift.shape == ref["shift"].shape and depth.is_cuda
        mean_depth = float(ref["depth"][mask].mean())
        errs = dict(depth=float((depth.cpu() - ref["depth"]).abs().max()) / mean_depth, fov_x=float((fov_x.cpu() - ref["fov_x"]).abs().max()),
                    fov_y=float((fov_y.cpu() - ref["fov_y"]).abs().max()), shift=float((shift.cpu() - ref["shift"]).abs().max()) / mean_depth)
        print(f"[point_map_to_depth {name} {size}] {errs} tol {tol:.1e}")
        assert max(errs.values()) <= tol + fp32, errs
    # leading dimensions are kept, as in the reference: [2, 1, H, W, 3] -> depth [2, 1, H, W], fov [2, 1]
    depth, fov_x, fov_y, shift = geometry.point_map_to_depth(pts[:2, None].to(dev), mask[:2, None].to(dev), downsample_size=(H, W))
    assert depth.shape == (2, 1, H, W) and fov_x.shape == fov_y.shape == shift.shape == (2, 1)
    px = geometry.recover_focal_pixels(pts.to(dev), mask.to(dev), (H, W))
    want = 0.5 * math.hypot(H, W) * case["ref"][(H, W)]["focal"]             # ((K00 W) + (K11 H)) / 2 with K00 = focal diag / (2 W), K11 alike
    assert float((px.cpu() / want - 1).abs().max()) <= tol + fp32


def _aligner(p, pred, dev):
    from geo4d_amd.align import GroupAligner
    return GroupAligner(p["groups"], pred.to(dev), p["conf"].squeeze(-1).to(dev), shared_focal=True, temporal_smoothing_weight=0.015, translation_weight=1.0)


def test_prefix_initialisation_vs_the_reference_init_from_group(fix, dev):
    """init_from_group(pose_init="prefix") against the REFERENCE's init_from_group with opt_raydir=False (align_group_prefix -> fast_pnp ->
    init_from_pts3d_group) on the 10-image / 4-window scene, cv2.solvePnPRansac stubbed by the seeded restatement this engine calls: window
    focals from the point maps, chaining WITH overwrite, every PnP started at its predecessor's focal, pairwise poses, scale
    normalisation, depth maps and camera poses. Tolerances of test_pnp_initialisation_vs_the_reference_init_from_group."""
    p = fix["prefix"]
    a = _aligner(p, p["pred"], dev)
    a.init_from_group(None, pose_init="prefix", niter_PnP=p["niter_PnP"])
    tol_f = max(10 * p["focal_group_gap"], 2e-5)
    ef = float((a.prefix_focals_raw / p["focal_group_before"] - 1).abs().max())
    print(f"[prefix init] window focals {a.prefix_focals_raw.tolist()} (reference {p['focal_group_before'].tolist()}): rel {ef:.2e}, tol {tol_f:.1e}")
    assert ef <= tol_f
    ref = p["after_init"]
    got = {k: a.P[k].detach().cpu() for k in ref}
    for k in ("im_poses", "pw_poses"):                      # quaternions are defined up to sign
        sign = torch.sign((got[k][:, :4] * ref[k][:, :4]).sum(1, keepdim=True))
        got[k] = torch.cat([got[k][:, :4] * sign, got[k][:, 4:]], 1)
    errs = {k: float((got[k].reshape(ref[k].shape) - ref[k]).abs().max()) for k in ref}
    loss = float(a.loss_and_grads()[0])
    print(f"[prefix init vs reference] max abs parameter differences {errs}; loss {loss:.5f} (reference {p['loss']:.5f})")
    assert errs["im_focals"] < 1e-3 and errs["pw_poses"] < 2e-3 and errs["im_poses"] < 5e-3 and errs["im_depthmaps"] < 5e-3, errs
    assert abs(loss - p["loss"]) < 0.05 * p["loss"]


def test_prefix_initialisation_replaces_an_outlier_window_focal(fix, dev):
    """One window's reference frame stretched by 3 in x and y: its focal drops to a third, trips the 0.6 filter and is replaced by the mean
    over focals above 30 - the reference's focal_group before and after the filter, and the shared focal it ends with."""
    p, o = fix["prefix"], fix["outlier"]
    pred = p["pred"].clone()
    pred[o["window"], 0] = o["frame"]
    a = _aligner(p, pred, dev)
    a.init_from_group(None, pose_init="prefix", niter_PnP=p["niter_PnP"])
    tol_f = max(10 * o["focal_group_gap"], 2e-5)
    print(f"[prefix init, outlier] window focals {a.prefix_focals_raw.tolist()} -> {a.prefix_focals.tolist()} (reference {o['focal_group_before'].tolist()} -> "
          f"{o['focal_group_after'].tolist()})")
    assert float((a.prefix_focals_raw / o["focal_group_before"] - 1).abs().max()) <= tol_f
    assert float((a.prefix_focals / o["focal_group_after"] - 1).abs().max()) <= tol_f
    assert float(a.prefix_focals[o["window"]]) > 2 * float(a.prefix_focals_raw[o["window"]])
    assert float((a.P["im_focals"].cpu().reshape(o["im_focals"].shape) - o["im_focals"]).abs().max()) < 1e-3


def _scene28_maps():
    """The 28-frame / 4-window ground-truth scene of test_align_gpu.py (_scene28: 16-frame windows, stride 4, 40 x 64, focal 55, every
    window in its own frame and scale), encoded as the decoded maps post_optimization consumes: channels 0..2 the point map in
    normalised bbox coordinates (pts3d = x / 2, y / 2, (z + 1) / 2 - pipeline.denormalize_pc_bbox2), 3 the confidence logit."""
    gen = torch.Generator().manual_seed(4)
    n, S, stride, H, W, f = 28, 16, 4, 40, 64, 55.0
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grid, pp = torch.stack([xs, ys], -1).float(), torch.tensor([W / 2, H / 2])
    c2w, pts = [], []
    for i in range(n):
        depth = 3.0 + 0.6 * torch.sin(xs / 9.0 + 0.2 * i) + 0.4 * torch.cos(ys / 7.0)
        cam = torch.cat([depth[..., None] * (grid - pp) / f, depth[..., None]], -1)
        a_ = torch.tensor(0.02 * i)
        R = torch.tensor([[torch.cos(a_), 0, torch.sin(a_)], [0, 1, 0], [-torch.sin(a_), 0, torch.cos(a_)]])
        M = torch.eye(4); M[:3, :3] = R; M[:3, 3] = torch.tensor([0.05 * i, 0.0, 0.01 * i])
        c2w.append(M); pts.append(cam @ R.T + M[:3, 3])
    slices = [slice(s0, s0 + S) for s0 in range(0, n - S + 1, stride)]
    maps = torch.zeros(len(slices), 11, S, H, W)
    for gi, sl in enumerate(slices):
        w2c = torch.inverse(c2w[sl.start])
        sc = 0.8 + 0.1 * gi
        p = torch.stack([(pts[i] @ w2c[:3, :3].T + w2c[:3, 3]) * sc for i in range(sl.start, sl.stop)]) + 0.003 * torch.randn((S, H, W, 3), generator=gen)
        p = 0.1 * p                                             # any global scale: keeps |channel| < 1.99 (far-away mask) and z out of the sky band
        maps[gi, 0], maps[gi, 1], maps[gi, 2] = 2 * p[..., 0], 2 * p[..., 1], 2 * p[..., 2] - 1
    return slices, maps, f, n, H, W            # confidence logit 0: softplus = 0.69, inverse confidence 1.44 > 0.5 everywhere


def test_post_optimization_mirrors_the_script_without_ray_maps(dev):
    """post_optimization(..., use_raymap=False, pose_init="prefix", align=False) - the reference script's hard-coded use_raymap = False -
    recovers the focal of a ground-truth scene from the point maps alone: shared focal within 5 % of the truth."""
    from geo4d_amd.align import post_optimization
    slices, maps, f, n, H, W = _scene28_maps()
    traj = torch.eye(4).repeat(len(slices), 16, 1, 1)
    scene = post_optimization(slices, maps.to(dev), traj.to(dev), None, use_raymap=False, use_inverse_depthmap=False, use_traj=False,
                              pose_init="prefix", align=False)
    focal = float(scene.get_focals()[0])
    print(f"[post_optimization prefix] window focals {scene.prefix_focals.tolist()}, shared focal {focal:.3f} (truth {f})")
    assert abs(focal - f) < 0.05 * f
    assert scene.get_depthmaps().shape == (n, H, W) and torch.isfinite(scene.get_depthmaps()).all()
    assert torch.isfinite(scene.loss_and_grads()[0])


def test_two_solves_back_to_back_on_a_side_stream(fix, dev):
    """Two solver calls enqueued on a side stream with the input buffers overwritten between them by stream-ordered copies, nothing
    synchronised until both are queued: each call must answer for the data it was enqueued on - no hidden host synchronisation, no state
    outside its own workspace."""
    from geo4d_amd import ops
    case = fix["focal"]["cases"]["24x32"]
    tol = max(10 * fix["focal"]["ref_gap"], 2e-5)
    first, mfirst = case["points"].to(dev), case["mask"].float().to(dev)
    second, msecond = first.flip(0).contiguous(), mfirst.flip(0).contiguous()
    buf, mbuf = torch.empty_like(first), torch.empty_like(mfirst)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        buf.copy_(first, non_blocking=True); mbuf.copy_(mfirst, non_blocking=True)
        a = ops.focal_shift(buf, mbuf, 0.5)
        buf.copy_(second, non_blocking=True); mbuf.copy_(msecond, non_blocking=True)
        b = ops.focal_shift(buf, mbuf, 0.5)
    side.synchronize()
    ref = case["ref"][(24, 32)]
    assert a[2].tolist() == [0, 0, 0] and b[2].tolist() == [0, 0, 0]
    assert float((a[1].cpu() / ref["focal"] - 1).abs().max()) <= tol and float((b[1].cpu().flip(0) / ref["focal"] - 1).abs().max()) <= tol
    assert torch.equal(a[0], b[0].flip(0)) and torch.equal(a[1], b[1].flip(0))
    torch.cuda.current_stream().wait_stream(side)
