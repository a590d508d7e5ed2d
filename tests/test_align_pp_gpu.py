"""Principal points in the multi-window global alignment (geo4d_amd/align.py optimize_pp / preset_principal_point, csrc/align.hip's
principal-point form of the fused residual kernel) against tests/golden/align_pp_tiny.pt - the REFERENCE LightPointCloudGroupOptimizer
with optimize_pp=True (tests/golden/generate_align_pp.py) on align_tiny.pt's scene - and against an fp64 autograd restatement."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def fix():
    base = torch.load(os.path.join(G, "align_tiny.pt"), weights_only=False)
    pp = torch.load(os.path.join(G, "align_pp_tiny.pt"), weights_only=False)
    return dict(base=base, pp=pp)


def _aligner(fix, case, dev, **kw):
    """The fixture scene with the reference's start of `case`; `preset` goes through preset_principal_point like the reference did."""
    from geo4d_amd.align import GroupAligner
    g, c = fix["base"], fix["pp"][case]
    a = GroupAligner(g["groups"], g["pred"].to(dev), g["conf"].squeeze(-1).to(dev), shared_focal=case != "per_image", optimize_pp=True,
                     temporal_smoothing_weight=g["kw"]["temporal_smoothing_weight"], translation_weight=g["kw"]["translation_weight"], **kw)
    if case == "preset":
        a.preset_principal_point(fix["pp"]["preset_pixels"])
        assert torch.allclose(a.P["im_pp"].cpu(), c["init"]["im_pp"], atol=1e-7) and "im_pp" in a.frozen
    for k, v in c["init"].items():
        if not (case == "preset" and k == "im_pp"):
            a.P[k] = v.clone().to(dev)
    return a


@pytest.mark.parametrize("chunk", [256, 1024])
@pytest.mark.parametrize("case", ["optimize", "preset", "per_image"])
def test_loss_and_gradients_vs_reference(fix, dev, case, chunk):
    """Bars of test_align_gpu.py::test_loss_and_gradients_vs_reference: loss 1e-5, every gradient (im_pp included) 1e-4 relative L2;
    two calls bit-identical. A frozen im_pp (preset) has no gradient, here as in the reference."""
    c = fix["pp"][case]
    a = _aligner(fix, case, dev, chunk_pixels=chunk)
    loss, grads = a.loss_and_grads()
    loss, grads = loss.clone(), {k: v.clone() for k, v in grads.items()}
    loss2, grads2 = a.loss_and_grads()
    print(f"[align pp {case} chunk {chunk}] loss {float(loss):.6f} vs reference {c['loss0']:.6f}; grad rel errors " +
          " ".join(f"{k}: {rel(grads[k], c['grads'][k]):.2e}" for k in grads))
    assert set(grads) == set(c["grads"]) and ("im_pp" in grads) == (case != "preset")
    assert abs(float(loss) - c["loss0"]) < 1e-5 * abs(c["loss0"])
    for k in grads:
        assert rel(grads[k], c["grads"][k]) < 1e-4, k
        assert torch.equal(grads[k], grads2[k]), "alignment gradients must be run-to-run deterministic"
    assert torch.equal(loss, loss2)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("case", ["optimize", "preset"])
def test_alignment_loop_vs_reference(fix, dev, case, graph, monkeypatch):
    """The reference's own 40-iteration global_alignment_loop with principal points, eager and as the captured iteration. Bar per
    parameter: the larger of test_alignment_loop_vs_reference's 2e-3 and four times the reference's own fp32-to-fp64 distance stored in
    the fixture (im_depthmaps 2.9e-7, im_poses 1.4e-7, im_focals 1.3e-7, pw_poses 1.8e-7, im_pp 7.5e-7: so 2e-3 everywhere).
    Measured on an MI355X, eager and captured alike: optimize - final loss 3.3e-7, im_depthmaps 1.7e-7, im_poses 8.5e-8, im_focals 0,
    pw_poses 1.8e-7, im_pp 5.3e-7; preset - final loss 0, im_depthmaps 1.5e-7, im_poses 1.1e-7, im_focals 0, pw_poses 1.2e-7, im_pp 0."""
    f, c = fix["pp"], fix["pp"][case]
    a = _aligner(fix, case, dev)
    pp_before = a.P["im_pp"].clone()
    replays, replay = [], torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda g: (replays.append(1), replay(g))[1])
    final, hist = a.compute_global_alignment(niter=f["niter"], lr=f["lr"], lr_min=f["lr_min"], schedule=f["schedule"], history=True, use_graph=graph)
    errs = {k: rel(a.P[k], c["after"][k]) for k in c["after"]}
    bars = {k: max(2e-3, 4 * f["fp64"]["rel"][k]) for k in errs}
    loss_err = abs(hist[-1] - c["loss_final"]) / abs(c["loss_final"])
    print(f"[align pp loop {case} graph {graph}] loss {hist[0]:.4f} -> {hist[-1]:.4f} (reference {c['loss_final']:.4f}, rel {loss_err:.2e}); "
          + " ".join(f"{k}: {v:.2e} (bar {bars[k]:.1e})" for k, v in errs.items()))
    assert loss_err < max(2e-3, 4 * f["fp64"]["loss_final_rel"])
    for k, v in errs.items():
        assert v < bars[k], (k, v, bars[k])
    # capturable: one eager iteration, then the captured one replayed for all the others (a failed capture would finish eagerly)
    assert len(replays) == (f["niter"] - 1 if graph else 0)
    if case == "preset":
        assert torch.equal(a.P["im_pp"], pp_before), "a preset principal point is frozen"
    else:
        assert not torch.equal(a.P["im_pp"], pp_before)


def _point_term_fp64(P, pred, conf, e_all, slot_group, H, W, base_scale=0.5, conf_clamp=10.0):
    """Independent restatement of the point term in fp64: X = R (d ((u - ppx) / f, (v - ppy) / f, 1)) + t against sR P + st."""
    def rot(q):
        x, y, z, w = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
        return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                            2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    sexp = lambda v: torch.sign(v) * torch.expm1(v.abs())
    n = P["im_poses"].shape[0]
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    uv = torch.stack([u.reshape(-1), v.reshape(-1)], -1)                                   # [HW, 2]
    d = P["im_depthmaps"].exp()[..., None]                                                 # [n, HW, 1]
    f = (P["im_focals"].expand(n, 1) / 20.0).exp()[:, None]
    cam = torch.cat([d * (uv[None] - P["pp"][:, None]) / f, d], -1)
    X = cam @ rot(P["im_poses"][:, :4]).transpose(1, 2) + sexp(P["im_poses"][:, 4:7])[:, None]
    ls = P["pw_poses"][:, 7]
    s = (ls + math.log(base_scale) - ls.mean()).exp()
    Y = (pred @ rot(P["pw_poses"][:, :4]).transpose(1, 2)[slot_group] + sexp(P["pw_poses"][:, 4:7])[slot_group][:, None]) * s[slot_group][:, None, None]
    return (conf.clamp(max=conf_clamp) * (X[e_all] - Y).norm(dim=-1)).sum() / conf.numel()


@pytest.mark.parametrize("H,W,chunk", [(17, 23, 256), (40, 64, 1024)])
def test_kernel_sums_vs_fp64_autograd(dev, H, W, chunk):
    """The residual kernel's principal-point sums where indexing can go wrong: 5 images in 2 windows of 4 at 17x23 (HW = 391, no multiple
    of 64, a partial second chunk) and at 40x64 with chunk_pixels = 1024 (three chunks, the last one partial), every image with its own
    principal point. dL/dpp of EVERY image within 1e-4 relative of fp64 autograd; the other gradients within their usual 1e-4 (so rows
    cannot be swapped unnoticed)."""
    from geo4d_amd.align import GroupAligner
    gen = torch.Generator().manual_seed(31 + H)
    groups, n, S = [[0, 1, 2, 3], [1, 2, 3, 4]], 5, 4
    Gn, HW = len(groups), H * W
    pred = torch.randn((Gn, S, H, W, 3), generator=gen) * 0.4 + torch.tensor([0.0, 0.0, 2.0])
    conf = 0.5 + 11.5 * torch.rand((Gn, S, H, W), generator=gen)
    a = GroupAligner(groups, pred.to(dev), conf.to(dev), shared_focal=False, optimize_pp=True, chunk_pixels=chunk)
    r = lambda *s: torch.randn(s, generator=gen)
    start = dict(im_depthmaps=r(n, HW) * 0.1 + math.log(2.0), im_poses=torch.cat([r(n, 3) * 0.05, torch.ones(n, 1), r(n, 3) * 0.1], 1),
                 im_focals=20.0 * math.log(0.9 * W) + r(n, 1), pw_poses=torch.cat([r(Gn, 3) * 0.05, torch.ones(Gn, 1), r(Gn, 3) * 0.1, r(Gn, 1) * 0.1], 1),
                 im_pp=torch.stack([0.3 - 0.15 * torch.arange(n).float(), -0.2 + 0.1 * torch.arange(n).float()], 1))
    for k, v in start.items():
        a.P[k] = v.clone().to(dev)
    loss, grads = a.loss_and_grads()
    P = {k: v.double().clone().requires_grad_(True) for k, v in start.items() if k != "im_pp"}
    P["pp"] = (torch.tensor([W / 2, H / 2]).double() + 10 * start["im_pp"].double()).requires_grad_(True)     # pixels
    e_all = torch.tensor([i for grp in groups for i in grp])
    ref = _point_term_fp64(P, pred.reshape(Gn * S, HW, 3).double(), conf.reshape(Gn * S, HW).double(), e_all, torch.arange(Gn * S) // S, H, W)
    ref.backward()
    per_image = [rel(a._pp_sums[i], P["pp"].grad[i]) for i in range(n)]
    errs = {k: rel(grads[k], P[k].grad) for k in grads if k != "im_pp"}
    print(f"[align pp sums {H}x{W} chunk {chunk}] loss {float(loss):.6f} vs fp64 {float(ref.detach()):.6f}; dL/dpp per image " +
          " ".join(f"{e:.1e}" for e in per_image) + "; " + " ".join(f"{k}: {v:.1e}" for k, v in errs.items()))
    assert abs(float(loss) - float(ref.detach())) < 1e-5 * float(ref.detach())
    assert max(per_image) < 1e-4, per_image
    assert torch.equal(grads["im_pp"], 10 * a._pp_sums)
    assert set(errs) == {"im_depthmaps", "im_poses", "im_focals", "pw_poses"} and max(errs.values()) < 1e-4, errs


def _offcentre_scene(dev, preset):
    """5 images / 2 windows of 4 at 12x16 rendered with the principal point (W/2 + 3, H/2 - 2); the aligner sits AT the ground truth."""
    from geo4d_amd.align import GroupAligner, rotmat_to_quat, signed_log1p
    n, S, H, W, f = 5, 4, 12, 16, 14.0
    pp = torch.tensor([W / 2 + 3, H / 2 - 2])
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grid = torch.stack([xs, ys], -1).float()
    c2w, pts, depths = [], [], []
    for i in range(n):
        depth = 2.0 + 0.5 * torch.sin(xs / 3.0 + 0.4 * i) + 0.3 * torch.cos(ys / 2.0)
        cam = torch.cat([depth[..., None] * (grid - pp) / f, depth[..., None]], -1)
        a_ = torch.tensor(0.06 * i)
        R = torch.tensor([[torch.cos(a_), 0, torch.sin(a_)], [0, 1, 0], [-torch.sin(a_), 0, torch.cos(a_)]])
        M = torch.eye(4); M[:3, :3] = R; M[:3, 3] = torch.tensor([0.15 * i, 0.02 * i, -0.03 * i])
        c2w.append(M); depths.append(depth); pts.append(cam @ R.T + M[:3, 3])
    groups = [[0, 1, 2, 3], [1, 2, 3, 4]]
    scales = [0.6, 0.85]
    preds = [torch.stack([(pts[i] @ torch.inverse(c2w[grp[0]])[:3, :3].T + torch.inverse(c2w[grp[0]])[:3, 3]) * sc for i in grp]) for grp, sc in zip(groups, scales)]
    a = GroupAligner(groups, torch.stack(preds).to(dev), torch.full((2, S, H, W), 2.0, device=dev))
    a.window_traj = torch.stack([torch.stack([torch.inverse(c2w[grp[0]]) @ c2w[i] for i in grp]) for grp in groups])     # cameras in the window's frame ...
    for g, sc in enumerate(scales):
        a.window_traj[g, :, :3, 3] *= sc                       # ... and scale
    a.norm_pw_scale = False                                    # the windows' true scales, not their normalised ones
    if preset:
        a.preset_principal_point(pp.expand(n, 2))
    a.P["im_depthmaps"] = torch.stack(depths).reshape(n, H * W).log().to(dev)
    a.P["im_focals"][:] = 20.0 * math.log(f)
    for i in range(n):
        a.P["im_poses"][i, :4], a.P["im_poses"][i, 4:7] = rotmat_to_quat(c2w[i][:3, :3]).to(dev), signed_log1p(c2w[i][:3, 3]).to(dev)
    for g, (grp, sc) in enumerate(zip(groups, scales)):       # world = (1 / sc) (R_0 P + sc t_0): get_pw_poses scales rotation AND translation
        M = c2w[grp[0]]
        a.P["pw_poses"][g, :4], a.P["pw_poses"][g, 4:7], a.P["pw_poses"][g, 7] = rotmat_to_quat(M[:3, :3]).to(dev), signed_log1p(M[:3, 3] * sc).to(dev), math.log(1 / sc)
    return a, torch.stack(pts), pp


def test_geometry_with_a_preset_principal_point(dev, tmp_path):
    """A scene whose true principal point is (W/2 + 3, H/2 - 2): at the ground-truth parameters the preset reproduces the true world
    points and beats the image centre; intrinsics, point-cloud cleaning and the written pred_intrinsics.txt carry it."""
    import numpy as np
    from geo4d_amd import scene_export
    a, truth, pp = _offcentre_scene(dev, True)
    b, _, _ = _offcentre_scene(dev, False)
    assert "im_pp" not in b.P and "im_pp" in a.P and "im_pp" in a.frozen
    e = rel(a.get_pts3d(), truth)
    la, lb = float(a.loss_and_grads()[0]), float(b.loss_and_grads()[0])
    print(f"[align pp geometry] get_pts3d vs truth {e:.2e}; loss preset {la:.3e} vs centre {lb:.3e}")
    assert e < 1e-5 and rel(b.get_pts3d(), truth) > 1e-2
    assert la < lb
    assert "im_pp" not in a.loss_and_grads()[1]
    K = a.get_intrinsics().cpu()
    assert torch.equal(K[:, :2, 2], pp.expand(a.n, 2)) and torch.allclose(K[:, 0, 0], torch.full((a.n,), 14.0), rtol=1e-6)
    assert torch.equal(b.get_intrinsics().cpu()[:, :2, 2], torch.tensor([8.0, 6.0]).expand(b.n, 2))
    a.clean_pointcloud()                                       # reads get_intrinsics() / get_pts3d(): runs with per-image principal points
    assert bool(torch.isfinite(a.im_conf).all())
    a.imgs = torch.rand(a.n, a.H, a.W, 3, device=dev)
    d = scene_export.save_scene(a, str(tmp_path), "seq")
    rows = np.loadtxt(os.path.join(d, "pred_intrinsics.txt")).reshape(a.n, 3, 3)
    assert np.allclose(rows[:, 0, 2], float(pp[0])) and np.allclose(rows[:, 1, 2], float(pp[1])) and np.allclose(rows[:, 0, 0], 14.0, atol=1e-4)


def test_initialisations_read_the_principal_points(dev):
    """init_from_group on the off-centre scene: the focal estimated from window 0's first point map is the true one only with the true
    principal point; the device PnP backend takes one principal point per launch and refuses presets that differ between images."""
    from geo4d_amd.align import GroupAligner
    a, _, pp = _offcentre_scene(dev, True)
    b, _, _ = _offcentre_scene(dev, False)
    traj = a.window_traj.to(dev)
    for sc in (a, b):
        sc.norm_pw_scale = True
        sc.init_from_group(traj)
    fa, fb = float(a.get_focals()[0]), float(b.get_focals()[0])
    print(f"[align pp init] focal from the first point map: {fa:.3f} with the preset, {fb:.3f} with the centre (true 14)")
    assert abs(fa - 14.0) < 0.01 * 14.0 and abs(fb - 14.0) > abs(fa - 14.0)
    assert torch.equal(a.get_principal_points().cpu(), pp.expand(a.n, 2))                 # the initialisation leaves a preset alone
    # the reference's "pnp" recipe with ray maps rendered at the true principal point: ray-map focal and RANSAC-PnP per image with its pp
    ys, xs = torch.meshgrid(torch.arange(a.H), torch.arange(a.W), indexing="ij")
    rays = torch.cat([(torch.stack([xs, ys], -1).float() - pp) / 14.0, torch.ones(a.H, a.W, 1)], -1).expand(a.G, a.S, a.H, a.W, 3).to(dev)
    fresh = lambda: GroupAligner(a.groups, a.pred.reshape(a.G, a.S, a.H, a.W, 3), a.conf.reshape(a.G, a.S, a.H, a.W))
    losses = {}
    for name, preset, backend in (("host", pp.expand(a.n, 2), "host"), ("device", pp.expand(a.n, 2), "device"), ("centre", None, "host")):
        c = fresh()
        if preset is not None:
            c.preset_principal_point(preset)
        c.init_from_group(None, raymaps=rays, pose_init="pnp", niter_PnP=20, pnp_backend=backend)
        losses[name] = (float(c.loss_and_grads()[0]), float(c.get_focals()[0]))
    print("[align pp init] pnp start (loss, focal):", losses)
    assert all(math.isfinite(l) for l, _ in losses.values())
    assert losses["host"][0] < losses["centre"][0] and losses["device"][0] < losses["centre"][0]
    assert abs(losses["host"][1] - 14.0) < 0.05 * 14.0 and abs(losses["device"][1] - 14.0) < 0.05 * 14.0
    c = fresh()
    c.preset_principal_point(pp + torch.arange(a.n).float()[:, None] * 0.5)
    with pytest.raises(ValueError, match="differ between images"):
        c.init_from_group(None, raymaps=rays, pose_init="pnp", niter_PnP=20, pnp_backend="device")
    c.init_from_group(None, raymaps=rays, pose_init="pnp", niter_PnP=20, pnp_backend="host")      # the host backend takes each image's own
    assert math.isfinite(float(c.loss_and_grads()[0]))


@pytest.mark.parametrize("case", ["optimize", "preset", "per_image"])
def test_autograd_chain_stays_a_cross_check(fix, dev, case):
    """`_loss_and_grads_torch` (GEO4D_ALIGN_CHAIN=torch) carries im_pp through autograd: same key set, same numbers as the fused chain."""
    a = _aligner(fix, case, dev)
    loss_t, g_t = a._loss_and_grads_torch()
    g_t = {k: v.clone() for k, v in g_t.items()}
    loss_h, g_h = a.loss_and_grads()
    errs = {k: rel(g_h[k], g_t[k]) for k in g_t}
    print(f"[align pp chain {case}] loss {float(loss_h):.6f} vs autograd {float(loss_t):.6f}; " + " ".join(f"{k}: {v:.1e}" for k, v in errs.items()))
    assert set(g_h) == set(g_t) and ("im_pp" in g_h) == (case != "preset")
    assert abs(float(loss_h) - float(loss_t)) < 2e-6 * abs(float(loss_t))
    for k, e in errs.items():                                  # test_fused_parameter_chain_rule_equals_autograd's bars; im_pp is a plain sum like im_focals
        assert e < (2e-4 if k in ("im_focals", "im_depthmaps", "im_pp") else 2e-5), (k, e)


def test_presets_masks_and_intrinsics(fix, dev):
    """preset_principal_point / preset_focal / preset_intrinsics with the reference's kinds of `msk`; what each freezes; argument errors."""
    from geo4d_amd.align import GroupAligner
    g = fix["base"]
    H, W = g["pred"].shape[2:4]
    centre = torch.tensor([W / 2, H / 2])
    new = lambda **kw: GroupAligner(g["groups"], g["pred"].to(dev), g["conf"].squeeze(-1).to(dev), **kw)
    a = new()
    n = a.n
    assert "im_pp" not in a.P and torch.equal(a.get_principal_points().cpu(), centre.expand(n, 2))
    a.preset_principal_point([[9.0, 5.0], [7.5, 6.5]], msk=[1, 4])                       # a list of pairs, index list; the others stay centred
    want = centre.repeat(n, 1)
    want[1], want[4] = torch.tensor([9.0, 5.0]), torch.tensor([7.5, 6.5])
    assert torch.allclose(a.get_principal_points().cpu(), want, atol=1e-6) and a.frozen == {"im_pp"}
    mask = torch.zeros(n, dtype=torch.bool)
    mask[2] = True
    a.preset_principal_point(torch.tensor([[8.5, 6.25]]), msk=mask)                       # boolean mask
    a.preset_principal_point(torch.tensor([[8.25, 5.75]]), msk=0)                         # a single index
    want[2], want[0] = torch.tensor([8.5, 6.25]), torch.tensor([8.25, 5.75])
    assert torch.allclose(a.get_principal_points().cpu(), want, atol=1e-6)
    for bad, msk in ((torch.zeros(n, 3), None), (torch.zeros(2, 2), None), (torch.zeros(1, 2), [n]), (torch.zeros(1, 2), torch.zeros(n - 1, dtype=torch.bool))):
        with pytest.raises(ValueError):
            a.preset_principal_point(bad, msk=msk)
    K = torch.eye(3).repeat(n, 1, 1)
    K[:, 0, 0], K[:, 1, 1] = 11.0 + torch.arange(n), 13.0 + torch.arange(n)
    K[:, 0, 2], K[:, 1, 2] = W / 2 + 1.0, H / 2 - 0.5 * torch.arange(n)
    b = new(shared_focal=False)
    b.preset_intrinsics(K)                                                                # optimize_pp off: focal only, as the reference
    assert "im_pp" not in b.P and b.frozen == {"im_focals"} and torch.allclose(b.get_focals().cpu().flatten(), 12.0 + torch.arange(n), rtol=1e-6)
    b.preset_intrinsics(K, use_pp=True)
    assert b.frozen == {"im_focals", "im_pp"} and torch.allclose(b.get_intrinsics().cpu()[:, :2, 2], K[:, :2, 2], atol=1e-6)
    c = new(optimize_pp=True)                                                             # optimize_pp on: the reference sets the principal point too
    c.preset_intrinsics(list(K))
    assert c.frozen == {"im_focals", "im_pp"} and torch.allclose(c.get_intrinsics().cpu()[:, :2, 2], K[:, :2, 2], atol=1e-6)
    assert abs(float(c.get_focals()[0]) - float((12.0 + torch.arange(n)).mean())) < 1e-4     # shared focal: the mean
    d = new(shared_focal=False)
    d.preset_focal([20.0], msk=3)                                                         # a subset: set, not frozen
    assert d.frozen == set() and abs(float(d.get_focals()[3]) - 20.0) < 1e-4


def test_sharded_principal_point_gradients_sum_to_the_full_gradient(fix, dev):
    """Two emulated ranks as in test_sharded_residual_kernel_sums_to_the_full_objective: im_pp rides in the one packed all-reduce; the
    two shards' gradients sum to the un-sharded ones within 2e-5."""
    from geo4d_amd.align_dist import AlignShard
    full = _aligner(fix, "optimize", dev)
    loss, grads = full.loss_and_grads()
    parts = []
    for r in range(2):
        sh = AlignShard(fix["base"]["groups"], full.n, rank=r, world=2, exchange="allreduce")
        sh._all_reduce = lambda t: t                         # no process group here: ranks are summed by hand below
        a = _aligner(fix, "optimize", dev, shard=sh)
        l, g = a.loss_and_grads()
        parts.append((float(l), {k: v.clone() for k, v in g.items()}))
    assert set(parts[0][1]) == set(grads) and "im_pp" in grads
    assert abs(parts[0][0] + parts[1][0] - float(loss)) < 1e-5 * abs(float(loss))
    for k in grads:
        tot = parts[0][1][k] + parts[1][1][k]
        print(f"[align pp shards] {k}: {rel(tot, grads[k]):.2e}")
        assert rel(tot, grads[k]) < 2e-5, (k, rel(tot, grads[k]))
    assert float(parts[0][1]["im_pp"].abs().sum()) > 0 and float(parts[1][1]["im_pp"].abs().sum()) > 0


def _tiny_clip(dev):
    """test_align_gpu.py::test_post_optimization_consumes_the_gathered_clip's synthetic clip."""
    from geo4d_amd.pipeline import window_slices
    gen = torch.Generator().manual_seed(3)
    T, H, W, n, f = 4, 16, 24, 7, 30.0
    slices = window_slices(n, 1, T)
    G_ = len(slices)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    ray = torch.stack([(xs - W / 2) / f, (ys - H / 2) / f, torch.ones(H, W)], 0)
    ray = ray / ray.norm(dim=0, keepdim=True)
    maps = torch.zeros(G_, 11, T, H, W)
    depth = 0.5 + 0.2 * torch.rand((G_, T, H, W), generator=gen)
    maps[:, 0:3] = (ray[None, :, None] * depth[:, None] * 1.2).clamp(-0.9, 0.9)
    maps[:, 2] = maps[:, 2] * 2 - 1
    maps[:, 3] = 1.0
    maps[:, 4:7] = ray[None, :, None]
    maps[:, 10] = (1.0 / (1.0 + depth)) * 2 - 1
    traj = torch.eye(4).repeat(G_, T, 1, 1)
    traj[:, :, 0, 3] = torch.arange(T).float() * 0.01
    return slices, maps.to(dev), traj.to(dev), n, H, W


def test_post_optimization_principal_point_arguments(dev):
    from geo4d_amd.align import post_optimization
    slices, maps, traj, n, H, W = _tiny_clip(dev)
    args = dict(n_iter=5, pose_schedule="linear", temporal_smoothing_weight=0.015, translation_weight=1.0)
    # both defaults: today's path, bit for bit, with and without naming the arguments - also when intrinsics are passed
    K = torch.eye(3).repeat(n, 1, 1)
    K[:, 0, 0], K[:, 1, 1] = 41.0, 43.0
    K[:, 0, 2], K[:, 1, 2] = W / 2 + 2.0 + 0.25 * torch.arange(n), H / 2 - 1.5
    for kw in (dict(), dict(intrinsics=K)):
        plain = post_optimization(slices, maps, traj, args, **kw)
        named = post_optimization(slices, maps, traj, args, optimize_pp=False, principal_points=None, **kw)
        assert "im_pp" not in plain.P and "im_pp" not in named.P and set(plain.P) == set(named.P)
        assert all(torch.equal(plain.P[k], named.P[k]) for k in plain.P)
        assert torch.equal(plain.get_intrinsics()[:, :2, 2].cpu(), torch.tensor([W / 2, H / 2]).expand(n, 2))
    # the points of the intrinsics, frozen
    fixed = post_optimization(slices, maps, traj, args, intrinsics=K, principal_points="intrinsics")
    assert "im_pp" in fixed.frozen and "im_focals" in fixed.frozen
    assert torch.allclose(fixed.get_principal_points().cpu(), K[:, :2, 2], atol=1e-5) and torch.allclose(fixed.get_intrinsics()[:, :2, 2].cpu(), K[:, :2, 2], atol=1e-5)
    assert torch.isfinite(fixed.loss_and_grads()[0])
    # optimised from the centre
    scene = post_optimization(slices, maps, traj, args, optimize_pp=True, align=False)
    assert float(scene.P["im_pp"].abs().max()) == 0.0 and "im_pp" not in scene.frozen
    final, hist = scene.compute_global_alignment(niter=5, lr=0.03, schedule="linear", history=True)
    print("[post_optimization optimize_pp] losses", hist, "im_pp", scene.P["im_pp"].flatten().tolist())
    assert len(hist) == 5 and all(math.isfinite(h) for h in hist)
    assert float(scene.P["im_pp"].abs().min()) > 0 and bool(torch.isfinite(scene.P["im_pp"]).all())
    moved = post_optimization(slices, maps, traj, args, optimize_pp=True)
    assert float(moved.P["im_pp"].abs().max()) > 0 and bool(torch.isfinite(moved.get_depthmaps()).all())
