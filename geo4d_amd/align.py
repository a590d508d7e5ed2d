"""Multi-window global alignment — the stage the all-gathered clip feeds.

``GroupAligner`` is the core of ``dust3r.cloud_opt.optimizer_group.LightPointCloudGroupOptimizer`` +
``base_opt_group.global_alignment_loop`` (called by ``post_optimization``, scripts/evaluation/test_geo4d.py:30-51,509): the same
parameters (per-image log-depth maps, camera poses as XYZW quaternion + signed-log1p translation, ``focal_break * log f`` focals —
shared by default —, one sim(3) ``pw_poses`` row per window with the reference's scale normalisation), the same loss (the
confidence-weighted L2-norm residual between re-projected depth points and the windows' aligned point maps, confidences clamped
at 10, + the camera temporal-smoothing term) and the same optimiser (Adam, betas (0.9, 0.9), linear / cosine schedule).

How an iteration runs here: ONE fused HIP kernel (csrc/align.hip) reads every window prediction once and produces the loss, the
gradient of the depth maps and 3x3 / 3-vector gradient sums per image and per (window, frame); the chain rule from those sums to
quaternions, log-translations, log-focal and log-scales is a few hundred flops per image and is taken by autograd over tiny device
tensors (no host synchronisation); the depth maps get a fused HIP Adam step. The reference needs ~40 full-size elementwise kernels
per iteration for the same numbers.

Initialisation follows ``init_im_poses.align_group`` / ``init_from_pts3d_group`` (:82-181, :569-635): windows are chained by
confidence-weighted similarity registration (``roma.rigid_points_registration`` = weighted Umeyama, restated here), ``pw_poses``
come from registering every window to the chained cloud, depths are the z of the cloud in each camera. The reference finds every
camera by OpenCV RANSAC-PnP (cv2.solvePnPRansac, absent here): ``init_from_group(pose_init="pnp")`` follows it with the seeded
restatement in geo4d_amd/pnp.py (same candidate focals, threshold and consensus rule; sampler and minimal solver differ and say so);
the DEFAULT start takes the per-window camera-to-world matrices that the Plücker ray maps already give (geo4d_amd/rays.py, N2) —
cheaper (no host loop over images) and equally close to the optimum on the fixtures. DEVIATION (second call): calling
``compute_global_alignment`` again continues with the late terms ON from its first iteration, whereas the reference restarts its
epoch counter (terms off until iteration 150, ``_set_st_depth`` re-run). The focals start, as in the reference,
from the Weiszfeld estimate on every image's ray map (`estimate_focal_weiszfeld`, pinned on dust3r.post_process; the reference then
lets PnP pick among that value and +-3 % of the image size).

From iteration ``depth_traj_start_iter`` (150) on the reference adds two terms (optimizer_group.py:470-512), built here as well:
  * inverse depth: ``2/A sum |1/(depth + 1e-6) - (s_g q + t_g)|`` over the pixels whose predicted inverse depth q exceeds 0.05, fused
    into the SAME residual kernel (4 more bytes per slot-pixel). Its start-up ``_set_st_depth`` (:333-372) — per window a
    5000-iteration Adam least-absolute-deviation fit of (s, t) started at a median ratio, scored by delta < 1.25, retried at two
    smaller learning rates under 80 %, dropped under 30 % — runs as HIP kernels for all windows at once (csrc/align.hip: radix-select
    medians, one launch per Adam iteration, one scoring pass); the reference runs ~6 torch kernels per iteration per window.
  * trajectory: ``0.005 sum relative_pose_loss(T_g [R_k | e^l_g t_k], pose_i)`` over the windows whose predicted trajectory agrees
    with the current cameras within 4 degrees of relative rotation after ``_set_traj`` (:242-268, evo's align_origin + RPE, restated:
    16 4x4 matrices per window, host side); the term itself is tiny-tensor autograd like the smoothing term.
s_depth / t_depth / traj_align_poses join Adam when their terms start (torch skips parameters without gradients, so their moments
and bias corrections count from the start iteration — reproduced with a second hyper-parameter table).

Principal points (optimizer_group.py:37, 67-68, 137-167, 203-219): the image centre by default, with no trace in the parameters or the
launches; ``optimize_pp=True`` adds ``im_pp`` [n, 2] (principal point = centre + 10 im_pp) to the optimised parameters - the residual
kernel's principal-point form sums dL/dpp per image in the same pass -, ``preset_principal_point`` / ``preset_intrinsics`` set and freeze
them. ``get_principal_points()`` is what the geometry, the intrinsics, the export and the initialisations read.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, ops

FOCAL_BREAK = 20.0
TORCH_CHAIN = __import__("os").environ.get("GEO4D_ALIGN_CHAIN", "hip") == "torch"   # round 2's autograd chain rule instead of align_small.hip


def signed_expm1(x):
    return torch.sign(x) * torch.expm1(torch.abs(x))


def signed_log1p(x):
    return torch.sign(x) * torch.log1p(torch.abs(x))


def quat_to_rotmat(q):
    """XYZW quaternion [..., 4] (normalised here) -> [..., 3, 3] (roma.RigidUnitQuat(...).normalize().to_homogeneous())."""
    x, y, z, w = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).reshape(q.shape[:-1] + (3, 3))


def rotmat_to_quat(R):
    """[3, 3] -> XYZW unit quaternion (branch on the largest diagonal term; w >= 0 convention not enforced, like scipy)."""
    R = R.double()
    m00, m11, m22 = R[0, 0], R[1, 1], R[2, 2]
    tr = m00 + m11 + m22
    if tr > 0:
        s = torch.sqrt(tr + 1.0) * 2
        q = torch.stack([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    elif m00 > m11 and m00 > m22:
        s = torch.sqrt(1.0 + m00 - m11 - m22) * 2
        q = torch.stack([0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s])
    elif m11 > m22:
        s = torch.sqrt(1.0 + m11 - m00 - m22) * 2
        q = torch.stack([(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s])
    else:
        s = torch.sqrt(1.0 + m22 - m00 - m11) * 2
        q = torch.stack([(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s])
    return (q / q.norm()).float()


def rigid_points_registration(x, y, weights, fp64=False):
    """(s, R, T) minimising sum w |s R x + T - y|^2 (init_im_poses.py:797-800 -> roma.rigid_points_registration(compute_scaling=True)):
    weighted Umeyama, sums in fp64; the result is cast to fp32 unless fp64 (geo4d_amd.evaluation's sim(3) trajectory alignment)."""
    x, y, w = x.reshape(-1, 3).double(), y.reshape(-1, 3).double(), weights.reshape(-1).double()
    w = w / w.sum()
    xm, ym = (w[:, None] * x).sum(0), (w[:, None] * y).sum(0)
    xc, yc = x - xm, y - ym
    # 3 x 3 weighted covariance as nine fp64 sums: `(w yc)^T @ xc` hands rocBLAS a dgemm with M = N = 3 and K = millions of points, which
    # took 64 ms per window at 16 x 320 x 512 (59 calls = 3.8 of the 3.9 s of a 128-frame clip's alignment init, tools/align_init_profile.py)
    # (row by row: three [N, 3] temporaries instead of one [N, 3, 3] = 190 MB per 16 x 320 x 512 window)
    wy = w[:, None] * yc
    cov = torch.stack([(wy[:, i:i + 1] * xc).sum(0) for i in range(3)])
    U, S, Vt = torch.linalg.svd(cov.cpu())
    d = torch.sign(torch.det(U @ Vt))
    D = torch.diag(torch.stack([torch.ones(()).double(), torch.ones(()).double(), d]))
    R = (U @ D @ Vt).to(x.device)
    s = (S * torch.diagonal(D)).sum().to(x.device) / (w * (xc * xc).sum(-1)).sum()
    T = ym - s * (R @ xm)
    return (s, R, T) if fp64 else (s.float(), R.float(), T.float())


def estimate_focal_weiszfeld(rays, pp=None, iters=10):
    """Focal of each map in `rays` [B, H, W, 3] (point map or ray-direction map) = argmin_f sum | pixel - f (x, y) / z |: closed-form L2
    start, then `iters` rounds of least squares re-weighted by the inverse residual. What align_group uses to initialise the focals
    from the ray maps (init_im_poses.py:133-136 -> estimate_focal :810-817 -> dust3r/post_process.py:12-60, focal_mode='weiszfeld',
    without its optional clipping). Host-side initialisation math: a dozen reductions per clip, any device."""
    B, H, W, _ = rays.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=rays.device), torch.arange(W, device=rays.device), indexing="ij")
    pp = torch.tensor([W / 2, H / 2], device=rays.device).expand(B, 2) if pp is None else pp
    px = torch.stack([xs, ys], -1).reshape(1, H * W, 2).float() - pp.reshape(B, 1, 2)
    r = rays.reshape(B, H * W, 3).float()
    q = (r[..., :2] / r[..., 2:3]).nan_to_num(posinf=0, neginf=0)
    qp, qq = (q * px).sum(-1), q.square().sum(-1)
    f = qp.mean(1) / qq.mean(1)
    for _ in range(iters):
        w = (px - f.view(B, 1, 1) * q).norm(dim=-1).clip(min=1e-8).reciprocal()
        f = (w * qp).mean(1) / (w * qq).mean(1)
    return f


def align_origin_and_rpe(est, ref):
    """The two evo pieces of ``_set_traj`` (optimizer_group.py:242-268 -> dust3r/utils/vo_eval.py:174-266), restated (evo is not
    installed): ``PosePath3D.align_origin`` = left-multiply the estimate by P = ref_0 est_0^-1, and the RPE rotation metric
    (delta = 1 frame, all pairs, rotation_angle_deg): rmse of the angle of (Q_i^-1 Q_{i+1})^-1 (P_i^-1 P_{i+1}).
    est, ref [S, 4, 4] float64 ndarrays -> (P [4, 4], rmse in degrees). Pinned on closed-form cases (tests/test_align_closed_form_cpu.py)."""
    Pm = ref[0] @ np.linalg.inv(est[0])
    al = Pm[None] @ est
    ang = [rotation_angle_deg(E) for E in relative_pose_errors(al, ref)]
    return Pm, float(np.sqrt(np.mean(np.square(ang))))


def relative_pose_errors(est, ref):
    """evo's RPE error matrices for delta = 1 frame, all pairs: E_k = (Q_k^-1 Q_{k+1})^-1 (P_k^-1 P_{k+1}), P = est, Q = ref [S, 4, 4]."""
    return [np.linalg.inv(np.linalg.inv(ref[k]) @ ref[k + 1]) @ (np.linalg.inv(est[k]) @ est[k + 1]) for k in range(len(est) - 1)]


def rotation_angle_deg(E):
    """Rotation angle of the 3 x 3 block of E in degrees (evo's rotation_angle_deg pose relation)."""
    return np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1.0, 1.0)))


def conf_trf(mode):
    """get_conf_trf (dust3r/cloud_opt/commons.py:70-81)."""
    if mode == "log":
        return torch.log
    if mode == "sqrt":
        return torch.sqrt
    if mode == "m1":
        return lambda x: x - 1
    if mode in ("id", "none"):
        return lambda x: x
    raise ValueError(f"bad mode for {mode=}")


def lr_at(t, schedule, lr_base, lr_min):
    """commons.py:102-110."""
    if schedule == "cosine":
        return lr_min + (lr_base - lr_min) * (1 + np.cos(t * np.pi)) / 2
    if schedule == "linear":
        return lr_base + (lr_min - lr_base) * t
    raise ValueError(f"bad lr schedule={schedule!r}")


class GroupAligner:
    MAX_SLOTS = 6          # csrc/align.hip MAXS: windows per image the fused residual kernel unrolls

    def __init__(self, groups, pred, conf, shared_focal=True, temporal_smoothing_weight=0.0, translation_weight=0.1, base_scale=0.5,
                 conf_clamp=10.0, chunk_pixels=4096, inverse_depth=None, traj=None, depth_traj_start_iter=150, shard=None, optimize_pp=False):
        """groups: list of G lists of S image indices; pred [G, S, H, W, 3], conf [G, S, H, W] fp32 on the HIP device;
        inverse_depth [G, S, H, W(, 1)] (the decoded inverse-depth modality mapped to [0, 1]) and traj [G, S, 4, 4] (every window's
        camera-to-world matrices in its own frame, N2) switch the two late terms on (pred_pts['inverse_depthmap'] / ['traj'],
        scripts/evaluation/test_geo4d.py:498-501). optimize_pp: one principal point per image, (W/2, H/2) + 10 im_pp, optimised with the
        other camera parameters (optimizer_group.py:37, 67-68, 210-211); off (default), and without a preset_principal_point, there is no
        `im_pp` parameter at all and every camera keeps the image centre."""
        if not pred.is_cuda:
            raise _lib.Geo4DNativeError("geo4d_amd.align.GroupAligner runs only on a HIP device (there is no CPU fallback)")
        self.lib = _lib.load()
        G, S, H, W, _ = pred.shape
        self.groups, self.G, self.S, self.H, self.W = [list(g) for g in groups], G, S, H, W
        self.n = 1 + max(max(g) for g in self.groups)
        self.dev = pred.device
        self.pred = pred.reshape(G * S, H * W, 3).float().contiguous()
        self.conf = conf.reshape(G * S, H * W).float().contiguous()
        self.shared_focal, self.tsw, self.tw, self.base_scale, self.conf_clamp = shared_focal, temporal_smoothing_weight, translation_weight, base_scale, conf_clamp
        self.norm_pw_scale = True
        e_all = [i for g in self.groups for i in g]
        if any(not any(i == img for i in e_all) for img in range(self.n)):
            raise ValueError("every image must belong to at least one window")
        self.shard = shard
        if shard is not None and not shard.local_groups:
            raise ValueError(f"rank {shard.rank} of {shard.world} owns no window of this {G}-window clip: build the shard with "
                             "align_dist.make_shard (it falls back to the replicated optimisation when windows < ranks)")
        local = set(range(G)) if shard is None else set(shard.local_groups)
        self.local_groups = sorted(local)
        self.primary = shard is None or shard.primary          # evaluates the pose-only terms (temporal smoothing, trajectory)
        slots = [[s for s, i in enumerate(e_all) if i == img and (s // S) in local] for img in range(self.n)]
        self.max_slots = max(len(s) for s in slots)
        if self.max_slots > self.MAX_SLOTS:
            raise NotImplementedError(f"an image belongs to {self.max_slots} windows; the fused residual kernel handles {self.MAX_SLOTS} "
                                      "(window stride >= 3 at 16 frames per window)")
        self.n_local_slots = sum(len(s) for s in slots)
        ptr = np.concatenate([[0], np.cumsum([len(s) for s in slots])]).astype(np.int32)
        self.slot_ptr = torch.from_numpy(ptr).to(self.dev)
        self.slot_idx = torch.tensor([s for lst in slots for s in lst], dtype=torch.int32, device=self.dev)
        self.slot_order = torch.tensor([s for lst in slots for s in lst], dtype=torch.long, device=self.dev)   # CSR position -> slot
        self.slot_group = torch.tensor([s // S for s in range(G * S)], dtype=torch.long, device=self.dev)
        all_slots = [[s for s, i in enumerate(e_all) if i == img] for img in range(self.n)]      # every window's slots (not shard-restricted)
        self._img_slot_ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in all_slots])]).astype(np.int32), device=self.dev)
        self._img_slot_idx = torch.tensor([x for lst in all_slots for x in lst], dtype=torch.int32, device=self.dev)
        order = [s for lst in slots for s in lst]                  # CSR entry -> slot; per window: its entries, ascending (align_small.hip)
        by_group = [[e for e, s in enumerate(order) if s // S == g] for g in range(G)]
        self._group_ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(b) for b in by_group])]).astype(np.int32), device=self.dev)
        self._group_entries = torch.tensor([e for b in by_group for e in b] or [0], dtype=torch.int32, device=self.dev)
        self.chunk = chunk_pixels
        f0 = FOCAL_BREAK * math.log(max(H, W))
        z = lambda *s: torch.zeros(s, device=self.dev)
        self.P = {"im_depthmaps": z(self.n, H * W), "im_poses": torch.cat([z(self.n, 3), torch.ones(self.n, 1, device=self.dev), z(self.n, 3)], 1),
                  "im_focals": torch.full((1 if shared_focal else self.n, 1), f0, device=self.dev),
                  "pw_poses": torch.cat([z(G, 3), torch.ones(G, 1, device=self.dev), z(G, 4)], 1)}
        need = self.lib.geo4d_align_workspace(self.n, G * S, H, W, self.chunk)
        self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        self._img_sums, self._slot_sums = z(self.n, 14), z(G * S, 14)
        self._grad_ld = z(self.n, H * W)
        self._pp = torch.tensor([W / 2, H / 2], device=self.dev)       # the image centre; the principal points: get_principal_points()
        self.optimize_pp = bool(optimize_pp)
        if self.optimize_pp:
            self.P["im_pp"] = z(self.n, 2)
        self._pp_sums = None                     # [n, 2] dL/dpp of the residual kernel's principal-point form (made on first use)
        self.invdepth = None if inverse_depth is None else inverse_depth.reshape(G * S, H * W).float().contiguous()
        self.traj = None if traj is None else traj.reshape(G, S, 4, 4).float().to(self.dev)
        self.start_iter = depth_traj_start_iter
        self.state = None                        # after the start iteration: dict(invalid_depth_groups, valid_traj_groups)
        self.frozen = set()                      # parameter names Adam leaves alone (preset_focal(..., requires_grad=False) -> {"im_focals"})
        self.slot_img = torch.tensor(e_all, dtype=torch.int32, device=self.dev)
        self.e_all = torch.tensor(e_all, dtype=torch.long, device=self.dev)
        if self.invdepth is not None:
            self.P["s_depth"], self.P["t_depth"] = torch.ones(G, 1, device=self.dev), z(G, 1)
        if self.traj is not None:
            self.P["traj_align_poses"] = torch.cat([z(G, 3), torch.ones(G, 1, device=self.dev), z(G, 4)], 1)
        # scene state the export reads (geo4d_amd/scene_export.py): Geo4D builds its scene with conf='id' and the class defaults
        # min_conf_thr = 3, thr_for_init_conf = False (base_opt_group.py:104-170); the confidence maps are built on first use
        self.conf_mode, self.min_conf_thr, self.thr_for_init_conf = "id", 3, False
        self.imgs = None                         # [n, H, W, 3] RGB in [0, 1] (post_optimization(imgs=...))
        self.dynamic_masks = None                # [n, H, W] bool: the moving pixels (geo4d_amd.motion.segment_motion)
        self.fused = None                        # the voxel-merged cloud of geo4d_amd.fusion.fuse_scene (a dict)
        self.tsdf = None                         # the TSDF surface points of geo4d_amd.tsdf.tsdf_scene (a dict)
        self._conf_maps = None                   # (im_conf, init_conf_maps)
        self._all_depthmaps = True               # False while a sharded alignment holds only this rank's images' final depth maps

    def _late_keys(self):
        """Parameters that receive gradients only once their term is on (torch.optim.Adam skips them until then)."""
        if self.state is None:
            return ()
        keys = ("s_depth", "t_depth") if self.invdepth is not None else ()
        return keys + (("traj_align_poses",) if self.traj is not None and len(self.state["valid_traj_groups"]) else ())

    def _pp_grad_on(self):
        """True when the principal points are optimised: `im_pp` exists and no preset froze it."""
        return "im_pp" in self.P and "im_pp" not in self.frozen

    def _get_msk_indices(self, msk):
        """optimizer_group.py:169-182: None = every image, an int, a list / array of indices, or a boolean mask of length n."""
        if msk is None:
            return list(range(self.n))
        if isinstance(msk, int):
            return [msk]
        m = np.asarray(msk.cpu() if torch.is_tensor(msk) else msk)
        if m.dtype == np.bool_:
            if len(m) != self.n:
                raise ValueError(f"msk: a boolean mask must have one entry per image ({self.n}), got {len(m)}")
            return np.where(m)[0].tolist()
        if np.issubdtype(m.dtype, np.integer):
            idx = m.reshape(-1).tolist()
            if any(i < 0 or i >= self.n for i in idx):
                raise ValueError(f"msk: image indices must lie in [0, {self.n})")
            return idx
        raise ValueError(f"bad msk={msk!r}")

    def preset_principal_point(self, known_pp, msk=None):
        """Set the principal points of the images `msk` selects to `known_pp` ([k, 2] pixels, or a list of k pairs) and freeze ALL of them
        (optimizer_group.py:159-167, 203-208: im_pp = (pp - (W/2, H/2)) / 10, then im_pp.requires_grad_(False)). Unlike the reference this
        works without optimize_pp: there `_no_grad` asserts that the parameter still requires a gradient, which im_pp never does with
        optimize_pp=False - an accident of how the reference marks "not yet set", not a rule about principal points."""
        idx = self._get_msk_indices(msk)
        pp = torch.as_tensor(np.asarray([np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.float64) for v in known_pp])
                             if isinstance(known_pp, (list, tuple)) else known_pp).detach().to("cpu", torch.float32)
        if pp.dim() != 2 or tuple(pp.shape) != (len(idx), 2):
            raise ValueError(f"preset_principal_point: expected [{len(idx)}, 2] pixel coordinates, got shape {tuple(pp.shape)}")
        if not bool(torch.isfinite(pp).all()):
            raise ValueError("preset_principal_point: non-finite principal point")
        if "im_pp" not in self.P:
            self.P["im_pp"] = torch.zeros(self.n, 2, device=self.dev)
        self.P["im_pp"][torch.as_tensor(idx, dtype=torch.long, device=self.dev)] = ((pp - self._pp.cpu()) / 10).to(self.dev)
        self.frozen.add("im_pp")
        return self

    def preset_focal(self, known_focals, msk=None):
        """optimizer_group.py:146-157 with requires_grad=False: focals in pixels for the images `msk` selects; the shared focal takes their
        mean. Frozen when every image was given (as the reference freezes); init_from_group then keeps them."""
        idx = self._get_msk_indices(msk)
        f = torch.as_tensor([float(v) for v in known_focals], dtype=torch.float32)
        if f.numel() != len(idx) or not bool((torch.isfinite(f) & (f > 0)).all()):
            raise ValueError(f"preset_focal: expected {len(idx)} positive focals")
        if self.shared_focal:
            self.P["im_focals"][:] = FOCAL_BREAK * math.log(float(f.mean()))
        else:
            self.P["im_focals"][torch.as_tensor(idx, dtype=torch.long, device=self.dev), 0] = (FOCAL_BREAK * torch.log(f)).to(self.dev)
        if len(idx) == self.n:
            self.frozen.add("im_focals")
        return self

    def preset_intrinsics(self, known_intrinsics, msk=None, use_pp=False):
        """optimizer_group.py:137-144: focal = mean of each K's diagonal, frozen (preset_focal); the principal point K[:2, 2] as well when
        optimize_pp is on (the reference's rule) or `use_pp` is passed."""
        K = torch.as_tensor(known_intrinsics).detach().float().cpu() if not isinstance(known_intrinsics, (list, tuple)) else \
            torch.stack([torch.as_tensor(k).detach().float().cpu() for k in known_intrinsics])
        if K.dim() == 2:
            K = K[None]
        if K.dim() != 3 or tuple(K.shape[1:]) != (3, 3):
            raise ValueError(f"preset_intrinsics: expected [k, 3, 3], got shape {tuple(K.shape)}")
        self.preset_focal([float((k[0, 0] + k[1, 1]) / 2) for k in K], msk)
        if self.optimize_pp or use_pp:
            self.preset_principal_point(K[:, :2, 2], msk)
        return self

    # ---- parameter -> geometry (tiny device tensors, differentiable) -----------------------------------------------------------
    def get_principal_points(self):
        """[n, 2] pixels: (W/2, H/2) + 10 im_pp (optimizer_group.py:210-211); the image centre for every image when there is no im_pp."""
        if "im_pp" not in self.P:
            return self._pp.expand(self.n, 2)
        return self._pp + 10 * self.P["im_pp"]

    def _init_pp(self, idx=None):
        """What the initialisations hand on as `pp`: None (= the image centre, today's path untouched) without im_pp, else the principal
        points [n, 2] or, with an image index, that image's [2]."""
        if "im_pp" not in self.P:
            return None
        pp = self.get_principal_points().detach()
        return pp if idx is None else pp[idx]

    def get_focals(self):
        lf = self.P["im_focals"]
        return (lf.expand(self.n, 1) / FOCAL_BREAK).exp()

    def get_im_poses(self):
        p = self.P["im_poses"]
        return quat_to_rotmat(p[:, :4]), signed_expm1(p[:, 4:7])

    def get_pw_scale(self):
        ls = self.P["pw_poses"][:, -1]
        scale = ls.exp()
        if self.norm_pw_scale:
            scale = scale * (math.log(self.base_scale) - ls.mean()).exp()
        return scale

    def get_pw_poses(self):
        p = self.P["pw_poses"]
        s = self.get_pw_scale().view(-1, 1, 1)
        return quat_to_rotmat(p[:, :4]) * s, signed_expm1(p[:, 4:7]) * s.view(-1, 1)      # scales rotation AND translation

    def get_depthmaps(self):
        return self.P["im_depthmaps"].exp().reshape(self.n, self.H, self.W)

    def get_im_poses_matrix(self):
        R, t = self.get_im_poses()
        M = torch.eye(4, device=self.dev).repeat(self.n, 1, 1)
        M[:, :3, :3], M[:, :3, 3] = R, t
        return M

    def get_pts3d(self):
        """World points [n, H, W, 3] from depth / pose / focal (optimizer_group.py:407-417)."""
        R, t = self.get_im_poses()
        f = self.get_focals().reshape(self.n, 1, 1)
        ys, xs = torch.meshgrid(torch.arange(self.H, device=self.dev), torch.arange(self.W, device=self.dev), indexing="ij")
        grid = torch.stack([xs, ys], -1).reshape(1, -1, 2).float()
        d = self.P["im_depthmaps"].exp().unsqueeze(-1)
        cam = torch.cat([d * (grid - self.get_principal_points()[:, None]) / f, d], -1)
        return (cam @ R.transpose(1, 2) + t[:, None]).reshape(self.n, self.H, self.W, 3)

    # ---- scene state of the export (base_opt_group.py:160-170, 237-242, 327-331, 353-359, 371-381; optimizer_group.py:213-219) ----
    def _slot_max_conf(self):
        """[n, H, W]: per image the maximum of its windows' confidences over every slot that holds it, from zeros, slots in window order
        (_compute_single_img_conf_group); the un-sharded slot CSR, so every rank builds the same maps."""
        ptr = self._img_slot_ptr.tolist()
        idx = self._img_slot_idx.long()
        out = torch.zeros(self.n, self.H * self.W, device=self.dev)
        for k in range(max(b - a for a, b in zip(ptr, ptr[1:]))):
            imgs = [i for i in range(self.n) if ptr[i + 1] - ptr[i] > k]
            rows = torch.tensor(imgs, dtype=torch.long, device=self.dev)
            slots = idx[torch.tensor([ptr[i] + k for i in imgs], dtype=torch.long, device=self.dev)]
            out[rows] = torch.maximum(out[rows], self.conf[slots])
        return out.reshape(self.n, self.H, self.W)

    def _conf_state(self):
        if self._conf_maps is None:
            im_conf = self._slot_max_conf()
            self._conf_maps = (im_conf, im_conf.clone())
        return self._conf_maps

    @property
    def im_conf(self):
        """[n, H, W] fp32 per-image confidence; clean_pointcloud rewrites it in place."""
        return self._conf_state()[0]

    @property
    def init_conf_maps(self):
        """[n, H, W] fp32 copy of the initial im_conf that clean_pointcloud never touches."""
        return self._conf_state()[1]

    def get_conf(self, mode=None):
        return conf_trf(self.conf_mode if mode is None else mode)(self.im_conf)

    def get_init_conf(self, mode=None):
        return conf_trf(self.conf_mode if mode is None else mode)(self.init_conf_maps)

    def get_masks(self):
        """[n, H, W] bool: conf > min_conf_thr on init_conf_maps (thr_for_init_conf) or on im_conf. With thr_for_init_conf the masks
        do not see clean_pointcloud, as in the reference."""
        return (self.init_conf_maps if self.thr_for_init_conf else self.im_conf) > self.min_conf_thr

    def get_intrinsics(self):
        """[n, 3, 3]: the focals on the diagonal, the principal points of get_principal_points() ((W/2, H/2) unless optimised or preset)."""
        K = torch.zeros((self.n, 3, 3), device=self.dev)
        f = self.get_focals().detach().flatten()
        K[:, 0, 0] = K[:, 1, 1] = f
        K[:, :2, 2] = self.get_principal_points().detach()
        K[:, 2, 2] = 1
        return K

    def gather_depthmaps(self):
        """Sharded alignment: every image's depth map from the rank that owns it (a collective: call it on every rank). A no-op without a shard."""
        if self.shard is not None:
            self.P["im_depthmaps"].copy_(self.shard.gather_depthmaps(self.P["im_depthmaps"]))
        self._all_depthmaps = True
        return self

    def require_all_depthmaps(self, what):
        if not self._all_depthmaps:
            raise RuntimeError(f"{what} needs every image's depth map, but this rank of a sharded alignment holds only the images it owns: "
                               "call scene.gather_depthmaps() on every rank first")

    @torch.no_grad()
    def clean_pointcloud(self, tol=0.001, bad_conf=0):
        """clean_depth of get_3D_model_from_scene (base_opt_group.py:371-381, 630-665) on the HIP device: lowers im_conf, in place, where a
        pixel lies in front of another image's depth and is less confident. Returns self."""
        from . import scene_export
        scene_export.check_tol(tol)
        self.require_all_depthmaps("clean_pointcloud")
        cams = torch.linalg.inv(self.get_im_poses_matrix())
        new = scene_export.clean_pointcloud(self.im_conf, self.get_intrinsics(), cams, self.get_depthmaps(), self.get_pts3d(), tol=tol,
                                            bad_conf=bad_conf)
        self.im_conf.copy_(new)
        return self

    # ---- one loss / gradient evaluation ---------------------------------------------------------------------------------------
    def _small(self):
        """The descriptor of the two small-parameter launches (csrc/align_small.hip) for the CURRENT parameter tensors."""
        sm = _lib.AlignSmall()
        P = self.P
        sm.im_poses, sm.im_focals, sm.pw_poses = P["im_poses"].data_ptr(), P["im_focals"].data_ptr(), P["pw_poses"].data_ptr()
        sm.cams, sm.slot_trf = self._cams.data_ptr(), self._trf.data_ptr()
        sm.img_sums, sm.slot_sums, sm.group_sums = self._img_sums.data_ptr(), self._slot_sums.data_ptr(), self._group_sums.data_ptr()
        sm.group_ptr, sm.group_entries = self._group_ptr.data_ptr(), self._group_entries.data_ptr()
        sm.scale_terms = self._scale_terms.data_ptr()
        g = self._small_grads
        sm.grad_im_poses, sm.grad_im_focals, sm.grad_pw_poses, sm.loss = g["im_poses"].data_ptr(), g["im_focals"].data_ptr(), g["pw_poses"].data_ptr(), self._loss.data_ptr()
        sm.n_imgs, sm.n_groups, sm.n_slots, sm.slots_per_group, sm.n_listed_slots = self.n, self.G, self.G * self.S, self.S, self.n_local_slots
        sm.n_focals, sm.norm_pw_scale = P["im_focals"].shape[0], int(self.norm_pw_scale)
        sm.focal_break, sm.base_scale, sm.ppx, sm.ppy = FOCAL_BREAK, self.base_scale, self.W / 2, self.H / 2
        sm.smooth_weight, sm.translation_weight = (self.tsw if self.primary else 0.0), self.tw
        return sm

    def _pp_buffers(self):
        """The principal-point form's extra state, made on first use (before any capture: the loop's first iteration is eager): the
        [n, 2] sums and a workspace with room for their per-chunk partials."""
        if self._pp_sums is None:
            self._pp_sums = torch.zeros(self.n, 2, device=self.dev)
            need = self.lib.geo4d_align_pp_workspace(self.n, self.G * self.S, self.H, self.W, self.chunk)
            if self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)

    def loss_and_grads(self):
        """Returns (loss 0-dim device tensor, dict of gradients shaped like self.P; parameters of terms that are off are absent).
        With principal points (optimize_pp or a preset) one more launch writes every image's own (ppx, ppy) into cams after the refresh;
        while they are optimised the residual kernel runs in its principal-point form (two more image sums, one more reduction) and a
        last small launch scales the sums to dL/dim_pp.
        Five launches: parameters -> cams / window transforms / (s, t) per slot (align_refresh), the fused residual kernel + its two
        fixed-order reductions, gradient sums -> parameter gradients (align_small_grads: the chain rule through quaternions / signed-log
        translations / log focal / normalised log scales, the temporal-smoothing term and the trajectory term, csrc/align_small.hip). `GEO4D_ALIGN_CHAIN=torch` selects round 2's autograd chain instead."""
        if TORCH_CHAIN:
            return self._loss_and_grads_torch()
        late = self._late_keys()
        z = lambda *s: torch.zeros(s, device=self.dev)
        if getattr(self, "_cams", None) is None:
            self._cams, self._trf, self._loss = z(self.n, 16), z(self.G * self.S, 12), z(1)
            self._group_sums, self._scale_terms = torch.zeros(self.G, 14, device=self.dev, dtype=torch.float64), torch.zeros(self.G, device=self.dev, dtype=torch.float64)
            self._small_grads = {"im_poses": z(self.n, 7), "im_focals": torch.zeros_like(self.P["im_focals"]), "pw_poses": z(self.G, 8),
                                 "s_depth": z(self.G, 1), "t_depth": z(self.G, 1)}
        sm = self._small()
        depth_on = "s_depth" in late
        traj_on = "traj_align_poses" in late
        if depth_on:
            if getattr(self, "_slot_st", None) is None:
                self._slot_st = z(self.G * self.S, 3)
            sm.grad_s_depth, sm.grad_t_depth = self._small_grads["s_depth"].data_ptr(), self._small_grads["t_depth"].data_ptr()
            sm.slot_st, sm.s_depth, sm.t_depth, sm.depth_ok = self._slot_st.data_ptr(), self.P["s_depth"].data_ptr(), self.P["t_depth"].data_ptr(), self._depth_ok.data_ptr()
        if traj_on:
            if "traj_align_poses" not in self._small_grads:
                self._small_grads["traj_align_poses"] = z(self.G, 8)
            if self.primary:                                       # pose-only term: one rank evaluates it
                sm.traj, sm.traj_align, sm.traj_valid = self._traj_full.data_ptr(), self.P["traj_align_poses"].data_ptr(), self._traj_valid.data_ptr()
                sm.slot_img, sm.img_slot_ptr, sm.img_slot_idx = self.slot_img.data_ptr(), self._img_slot_ptr.data_ptr(), self._img_slot_idx.data_ptr()
                sm.grad_traj, sm.traj_weight = self._small_grads["traj_align_poses"].data_ptr(), 0.005
        _lib.check(self.lib.geo4d_align_refresh(C.byref(sm), ops._stream()), "geo4d_align_refresh")
        pp_on = self._pp_grad_on()
        if "im_pp" in self.P:                                      # per-image principal points over the centre the refresh wrote
            _lib.check(self.lib.geo4d_align_set_pp(self._cams.data_ptr(), self.P["im_pp"].data_ptr(), self.n, self.W / 2, self.H / 2, ops._stream()),
                       "geo4d_align_set_pp")
        if pp_on:
            self._pp_buffers()
            if "im_pp" not in self._small_grads:
                self._small_grads["im_pp"] = z(self.n, 2)
        a = _lib.Align()
        a.pred, a.conf, a.logdepth, a.cams, a.slot_trf = self.pred.data_ptr(), self.conf.data_ptr(), self.P["im_depthmaps"].data_ptr(), self._cams.data_ptr(), self._trf.data_ptr()
        a.slot_ptr, a.slot_idx = self.slot_ptr.data_ptr(), self.slot_idx.data_ptr()
        a.grad_logdepth, a.img_sums, a.slot_sums = self._grad_ld.data_ptr(), self._img_sums.data_ptr(), self._slot_sums.data_ptr()
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        a.n_imgs, a.n_slots, a.H, a.W, a.chunk_pixels, a.max_slots_per_image = self.n, self.G * self.S, self.H, self.W, self.chunk, self.max_slots
        a.conf_clamp, a.inv_area = self.conf_clamp, 1.0 / float(self.G * self.S * self.H * self.W)
        if depth_on:
            a.invdepth, a.slot_st, a.depth_weight = self.invdepth.data_ptr(), self._slot_st.data_ptr(), 2.0 * a.inv_area
        if pp_on:                                                  # the principal-point form: + dL/dpp per image, then dL/dim_pp = 10 dL/dpp
            _lib.check(self.lib.geo4d_align_residual_pp(C.byref(a), self._pp_sums.data_ptr(), ops._stream()), "geo4d_align_residual_pp")
            _lib.check(self.lib.geo4d_align_pp_grads(self._pp_sums.data_ptr(), self._small_grads["im_pp"].data_ptr(), self.n, ops._stream()),
                       "geo4d_align_pp_grads")
        else:
            _lib.check(self.lib.geo4d_align_residual(C.byref(a), ops._stream()), "geo4d_align_residual")
        _lib.check(self.lib.geo4d_align_small_grads(C.byref(sm), ops._stream()), "geo4d_align_small_grads")
        loss = self._loss[0]
        grads = {k: self._small_grads[k] for k in ("im_poses", "im_focals", "pw_poses") + (("im_pp",) if pp_on else ())
                 + (("s_depth", "t_depth") if depth_on else ()) + (("traj_align_poses",) if traj_on else ())}
        grads["im_depthmaps"] = self._grad_ld
        if self.shard is not None:
            loss, grads = self.shard.reduce(loss, grads)        # one all-reduce: loss, small gradients, depth gradients of shared images
        return loss, grads

    def _loss_and_grads_torch(self):
        """Round 2's form of loss_and_grads: the chain rule from the gradient sums to the parameters by autograd over tiny tensors
        (~450 launches per iteration). Kept as the independent cross-check of csrc/align_small.hip (tests) and for A/B."""
        late = self._late_keys()
        pp_on = self._pp_grad_on()
        small = {k: self.P[k].detach().clone().requires_grad_(True) for k in ("im_poses", "im_focals", "pw_poses") + (("im_pp",) if pp_on else ()) + late}
        saved, self.P = self.P, dict(self.P, **small)
        try:
            R, t = self.get_im_poses()
            f = self.get_focals()
            sR, st = self.get_pw_poses()
            pp = self.get_principal_points()
        finally:
            self.P = saved
        cams = torch.cat([R.reshape(self.n, 9), t, f, pp, torch.zeros(self.n, 1, device=self.dev)], 1).detach().contiguous()
        trf = torch.cat([sR.reshape(self.G, 9), st], 1).detach()[self.slot_group].contiguous()
        a = _lib.Align()
        a.pred, a.conf, a.logdepth, a.cams, a.slot_trf = self.pred.data_ptr(), self.conf.data_ptr(), self.P["im_depthmaps"].data_ptr(), cams.data_ptr(), trf.data_ptr()
        a.slot_ptr, a.slot_idx = self.slot_ptr.data_ptr(), self.slot_idx.data_ptr()
        a.grad_logdepth, a.img_sums, a.slot_sums = self._grad_ld.data_ptr(), self._img_sums.data_ptr(), self._slot_sums.data_ptr()
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        a.n_imgs, a.n_slots, a.H, a.W, a.chunk_pixels, a.max_slots_per_image = self.n, self.G * self.S, self.H, self.W, self.chunk, self.max_slots
        a.conf_clamp, a.inv_area = self.conf_clamp, 1.0 / float(self.G * self.S * self.H * self.W)
        depth_on = "s_depth" in late
        if depth_on:
            slot_st = torch.cat([small["s_depth"].detach(), small["t_depth"].detach(), self._depth_ok], 1)[self.slot_group].contiguous()
            a.invdepth, a.slot_st, a.depth_weight = self.invdepth.data_ptr(), slot_st.data_ptr(), 2.0 * a.inv_area
        if pp_on:
            self._pp_buffers()
            a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
            _lib.check(self.lib.geo4d_align_residual_pp(C.byref(a), self._pp_sums.data_ptr(), ops._stream()), "geo4d_align_residual_pp")
        else:
            _lib.check(self.lib.geo4d_align_residual(C.byref(a), ops._stream()), "geo4d_align_residual")
        I = self._img_sums
        # slot sums come back in CSR (image-major) order: put them in slot order, then add the S frames of each window
        # (with a shard only this rank's slots are listed: rows past n_local_slots are not written)
        Ssum = torch.zeros_like(self._slot_sums).index_copy_(0, self.slot_order, self._slot_sums[:self.n_local_slots]).reshape(self.G, self.S, -1).sum(1)
        loss = I[:, 13].sum()
        # chain rule through the tiny parameter -> matrix maps: d loss = <dL/dR, dR> + <dL/dt, dt> + dL/df df + <dL/dsR, dsR> + <dL/dst, dst>
        surrogate = (I[:, :9].reshape(self.n, 3, 3) * R).sum() + (I[:, 9:12] * t).sum() + (I[:, 12:13] * f).sum() + \
            (Ssum[:, :9].reshape(self.G, 3, 3) * sR).sum() + (Ssum[:, 9:12] * st).sum()
        if pp_on:
            surrogate = surrogate + (self._pp_sums * pp).sum()
        if depth_on:
            surrogate = surrogate + (Ssum[:, 12:13] * small["s_depth"]).sum() + (Ssum[:, 13:14] * small["t_depth"]).sum()
        eye = torch.eye(3, device=self.dev)
        if "traj_align_poses" in late and self.primary:
            # optimizer_group.py:496-512: T_g [R_k | e^l t_k] against the cameras of the window's images (rigid inverse written out)
            vg, idx = self._traj_vg, self._traj_idx          # device index tensors made once at the start-up (capturable)
            tap = small["traj_align_poses"].index_select(0, vg)
            Ra, ta, sc = quat_to_rotmat(tap[:, :4]), signed_expm1(tap[:, 4:7]), tap[:, 7].exp()
            Rk, tk = self._traj_R, self._traj_t
            Rm = Ra[:, None] @ Rk
            tm = (Ra[:, None] @ (tk * sc[:, None, None])[..., None])[..., 0] + ta[:, None]
            Rm, tm = Rm.reshape(-1, 3, 3), tm.reshape(-1, 3)
            rel_R = Rm.transpose(1, 2) @ R[idx]
            rel_t = (Rm.transpose(1, 2) @ (t[idx] - tm)[:, :, None])[:, :, 0]
            ltraj = 0.005 * (torch.norm(rel_R - eye, dim=(1, 2)) + torch.norm(rel_t, dim=1) * self.tw).sum()
            surrogate = surrogate + ltraj
            loss = loss + ltraj.detach()
        if self.tsw > 0 and self.n > 1 and self.primary:
            # relative_pose_loss (optimizer_group.py:529-541): inverse(RT1) @ RT2 with RT rigid, so inverse = [R^T | -R^T t]
            # (no batched LU on the device: keeps the iteration capturable)
            Rt = R[:-1].transpose(1, 2)
            rel_R, rel_t = Rt @ R[1:], (Rt @ (t[1:] - t[:-1])[:, :, None])[:, :, 0]
            smooth = (torch.norm(rel_R - eye, dim=(1, 2)) + torch.norm(rel_t, dim=1) * self.tw).sum()
            surrogate = surrogate + self.tsw * smooth
            loss = loss + self.tsw * smooth.detach()
        surrogate.backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in small.items()}
        grads["im_depthmaps"] = self._grad_ld
        if self.shard is not None:
            loss, grads = self.shard.reduce(loss, grads)        # one all-reduce: loss, small gradients, depth gradients of shared images
        return loss, grads

    # ---- start-up of the two late terms -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _lad_fit(self, target, active, lr, iters, ws):
        G, n = self.G, self.S * self.H * self.W
        st, counts = torch.empty(G, 2, device=self.dev), torch.zeros(G, 2, dtype=torch.int32, device=self.dev)
        info = torch.empty(G, 2, device=self.dev)
        act = None if active is None else torch.tensor(active, dtype=torch.uint8, device=self.dev)
        _lib.check(self.lib.geo4d_lad_fit(self.invdepth.data_ptr(), target.data_ptr(), G, n, None if act is None else act.data_ptr(), lr, iters,
                                          1e-6, st.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "geo4d_lad_fit")
        self.lad_steps = info[:, 0].tolist()                 # Adam steps each window took before the reference's stop test fired
        _lib.check(self.lib.geo4d_lad_delta(self.invdepth.data_ptr(), target.data_ptr(), self.conf.data_ptr(), st.data_ptr(), G, n, 0.5,
                                            self.conf_clamp, 0.05, counts.data_ptr(), ops._stream()), "geo4d_lad_delta")
        c = counts.double().cpu()
        return st, (c[:, 0] / c[:, 1]).tolist()

    @torch.no_grad()
    def _set_st_depth(self):
        """optimizer_group.py:333-372. Sets s_depth / t_depth; returns the windows dropped from the term."""
        G, S, HW = self.G, self.S, self.H * self.W
        target = torch.empty(G * S, HW, device=self.dev)
        _lib.check(self.lib.geo4d_lad_target(self.P["im_depthmaps"].data_ptr(), self.slot_img.data_ptr(), target.data_ptr(), G * S, HW, ops._stream()),
                   "geo4d_lad_target")
        ws = torch.empty(self.lib.geo4d_lad_workspace(G, S * HW), dtype=torch.uint8, device=self.dev)
        mine = None if self.shard is None else [1 if g in set(self.local_groups) else 0 for g in range(G)]    # a rank fits its own windows
        st, best = self._lad_fit(target, mine, 1e-2, 5000, ws)
        retry = [1 if (b < 0.8 and (mine is None or mine[g])) else 0 for g, b in enumerate(best)]
        if any(retry):
            for lr in (1e-4, 1e-3):
                st2, d2 = self._lad_fit(target, retry, lr, 3000, ws)
                for g in range(G):
                    if retry[g] and d2[g] > best[g]:
                        st[g], best[g] = st2[g], d2[g]
        if self.shard is not None:
            tab = torch.cat([st, torch.tensor(best, device=self.dev, dtype=st.dtype).reshape(G, 1).nan_to_num()], 1)
            tab = self.shard.merge_rows(tab.nan_to_num(), self.local_groups)
            st, best = tab[:, :2].contiguous(), tab[:, 2].tolist()
        self.P["s_depth"].copy_(st[:, :1])
        self.P["t_depth"].copy_(st[:, 1:])
        self.depth_delta = best
        return [g for g in range(G) if best[g] < 0.3]

    @torch.no_grad()
    def _set_traj(self):
        """optimizer_group.py:242-268 (evo's align_origin and RPE rotation restated: oracle/align.py header). Host side: G x S 4x4."""
        R, t = self.get_im_poses()
        im = np.tile(np.eye(4), (self.n, 1, 1))
        im[:, :3, :3], im[:, :3, 3] = R.double().cpu().numpy(), t.double().cpu().numpy()
        scale = self.get_pw_scale().double().cpu().numpy()
        traj = self.traj.double().cpu().numpy()
        valid = []
        for g, grp in enumerate(self.groups):
            est = traj[g].copy()
            est[:, :3, 3] *= scale[g]
            ref = im[grp]
            Pm, rpe = align_origin_and_rpe(est, ref)
            self.P["traj_align_poses"][g, :4] = rotmat_to_quat(torch.from_numpy(Pm[:3, :3])).to(self.dev)
            self.P["traj_align_poses"][g, 4:7] = signed_log1p(torch.from_numpy(Pm[:3, 3])).float().to(self.dev)
            self.P["traj_align_poses"][g, 7] = float(np.log(scale[g]))
            if rpe < 4:
                valid.append(g)
        return valid

    def start_depth_traj(self):
        """What forward() does at epoch == depth_traj_start_iter (optimizer_group.py:470-503)."""
        self.set_state(self._set_st_depth() if self.invdepth is not None else [], self._set_traj() if self.traj is not None else [])
        return self.state

    def set_state(self, invalid_depth_groups, valid_traj_groups):
        """Which windows take part in the late terms (normally decided by start_depth_traj)."""
        self.state = dict(invalid_depth_groups=list(invalid_depth_groups), valid_traj_groups=list(valid_traj_groups))
        ok = torch.ones(self.G, 1)
        ok[self.state["invalid_depth_groups"]] = 0
        self._depth_ok = ok.to(self.dev)
        if self.traj is not None and len(valid_traj_groups):
            vg = torch.tensor(self.state["valid_traj_groups"], dtype=torch.long, device=self.dev)
            self._traj_vg = vg
            valid = torch.zeros(self.G, dtype=torch.int32)
            valid[self.state["valid_traj_groups"]] = 1
            self._traj_valid = valid.to(self.dev)
            self._traj_full = self.traj.reshape(self.G * self.S, 16).float().contiguous()
            self._traj_idx = self.e_all.reshape(self.G, self.S).index_select(0, vg).reshape(-1)
            self._traj_R, self._traj_t = self.traj.index_select(0, vg)[:, :, :3, :3].contiguous(), self.traj.index_select(0, vg)[:, :, :3, 3].contiguous()

    # ---- optimisation loop (base_opt_group.py:553-626) --------------------------------------------------------------------------
    def compute_global_alignment(self, niter=300, lr=0.01, lr_min=1e-3, schedule="cosine", history=False, use_graph=True):
        """Adam (betas 0.9 / 0.9, eps 1e-8, bias-corrected: torch.optim.Adam's arithmetic) under the reference's schedule. One
        iteration = fused residual kernel + tiny chain rule + fused Adam on the depth maps + Adam on the small parameters, with
        lr and the bias corrections read from device tables indexed by a device counter — so ONE captured hipGraph is replayed
        with no host work in between (`use_graph`; the eager loop runs the same kernels). With the late terms the loop is two such
        phases around the start-up at iteration `depth_traj_start_iter` (which synchronises with the host once)."""
        b1 = b2 = 0.9
        eps = 1e-8
        if self.shard is not None and self.shard.active:
            use_graph = False                                  # the per-iteration all-reduce runs on RCCL's stream: eager launches
            self._all_depthmaps = False
        steps = torch.arange(1, niter + 1, dtype=torch.float64)
        lrs = torch.tensor([lr_at(it / niter, schedule, lr, lr_min) for it in range(niter)], dtype=torch.float64)
        table = torch.stack([lrs, 1 - b1 ** steps, (1 - b2 ** steps).sqrt()], 1).float().to(self.dev)            # [niter, 3]
        has_late = self.invdepth is not None or self.traj is not None
        # iteration at which the late terms (and their parameters' Adam moments) start; 0 when a previous call already started them
        start = 0 if self.state is not None else (min(self.start_iter, niter) if has_late else niter)
        lsteps = (steps - start).clamp_min(1)                                  # a late parameter's own step count
        table_late = torch.stack([lrs, 1 - b1 ** lsteps, (1 - b2 ** lsteps).sqrt()], 1).float().to(self.dev)
        idx = torch.zeros((1,), dtype=torch.long, device=self.dev)
        hyper, hyper_late = torch.zeros(3, device=self.dev), torch.zeros(3, device=self.dev)
        mom = {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in self.P.items()}
        losses = torch.zeros(niter, device=self.dev)

        def iteration():
            hyper.copy_(table.index_select(0, idx)[0])
            hyper_late.copy_(table_late.index_select(0, idx)[0])
            loss, grads = self.loss_and_grads()
            losses.index_copy_(0, idx, loss.reshape(1))
            d, (m, v) = self.P["im_depthmaps"], mom["im_depthmaps"]
            _lib.check(self.lib.geo4d_adam_step_dev(d.data_ptr(), grads["im_depthmaps"].data_ptr(), m.data_ptr(), v.data_ptr(), d.numel(),
                                                    hyper.data_ptr(), b1, b2, eps, ops._stream()), "geo4d_adam_step_dev")
            late = self._late_keys()
            for k in ("im_poses", "im_focals", "pw_poses") + (("im_pp",) if self._pp_grad_on() else ()) + late:   # a few dozen numbers each
                if k in self.frozen:
                    continue
                g, (m, v), h = grads[k].contiguous(), mom[k], hyper_late if k in late else hyper
                _lib.check(self.lib.geo4d_adam_step_dev(self.P[k].data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), self.P[k].numel(),
                                                        h.data_ptr(), b1, b2, eps, ops._stream()), "geo4d_adam_step_dev")
            idx.add_(1)

        def run(count):
            done = 0
            if use_graph and count > 2:
                try:
                    iteration()                             # eager first iteration (allocator warm-up), then capture the second
                    done = 1
                    g = torch.cuda.CUDAGraph()
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                            iteration()
                    torch.cuda.current_stream().wait_stream(side)
                    for _ in range(count - 1):          # capturing records, it does not run
                        g.replay()
                    done = count
                except RuntimeError:                        # an op that cannot be captured on this build: finish eagerly
                    torch.cuda.synchronize()
                    done = None
            return done

        def run_phase(first, last):
            done = run(last - first)
            if done is None:
                done = int(idx.item()) - first
            for _ in range(done, last - first):
                iteration()

        if self.state is None:
            run_phase(0, start)
            if has_late and start < niter:
                self.start_depth_traj()
                run_phase(start, niter)
        else:                                               # terms already started (a second call continues with them on)
            run_phase(0, niter)
        self.gather_depthmaps()                                # every image's depth map from the rank that owns it
        hist = losses.tolist() if history else None
        return float(losses[-1]) if niter else float("inf"), hist

    # ---- initialisation (init_im_poses.py:82-181, 569-635) ----------------------------------------------------------------------
    @torch.no_grad()
    def init_from_group(self, traj, focal=None, raymaps=None, pose_init="traj", niter_PnP=100, pnp_seed=0, pnp_backend="host"):
        """pose_init = "pnp": the reference's initialisation (init_im_poses.align_group :82-214): windows chained by registration
        WITHOUT overwriting an image's first estimate, every camera from seeded RANSAC-PnP of its chained point map against the
        pixel grid (geo4d_amd/pnp.py, confidence > 0.5), tried at the image's ray-map focal and -/+ 3 % of the image size; images of
        the FIRST window take the winning candidate as their focal, the others keep the ray-map estimate (as the reference's
        `if im_focals[img_idx] is None` leaves them); the shared focal is the mean. `traj` is then only used by the trajectory term.
        pose_init = "prefix": the initialisation the reference's command line actually runs (use_raymap = False ->
        init_im_poses.align_group_prefix :226-405), which needs no ray maps: one focal per window from its reference frame's point map
        alone (geometry.recover_focal_pixels on the device), windows chained WITH overwriting, PnP per image started at its predecessor's
        focal (see _init_prefix). `traj` and `raymaps` are not used by it.
        pose_init = "traj" (default): cameras from the Plücker ray maps instead (below).
        traj [G, S, 4, 4]: camera-to-world of every frame in its window's own frame (the Plücker cameras of N2);
        focal: pixels; raymaps [G, S, H, W, 3] (pred_pts['raydir']): when given and `focal` is None, every image's focal is the
        Weiszfeld estimate on its first ray map and the shared focal their mean, as align_group / init_from_pts3d_group do
        (init_im_poses.py:133-136, 183-185, 627-628); with neither, the focal is estimated from window 0's first point map.
        pnp_backend: "host" (default, geo4d_amd/pnp.py in numpy) or "device" (ops.pnp_ransac, csrc/pnp.hip: the same solver hypothesis
        for hypothesis, the image chain enqueued without host copies; see _init_prefix / _init_pnp). Used by "pnp" and "prefix" only."""
        if pnp_backend not in ("host", "device"):
            raise ValueError(f"pnp_backend={pnp_backend!r}: 'host' or 'device'")
        if focal is None and "im_focals" in self.frozen:         # preset_focal / preset_intrinsics before the initialisation: keep it
            focal = float(self.get_focals()[0]) if self.shared_focal else self.get_focals().detach().flatten().clone()
        G, S, H, W = self.G, self.S, self.H, self.W
        pred = self.pred.reshape(G, S, H * W, 3)
        conf = self.conf.reshape(G, S, H * W)
        pts3d, conf_list, im_poses = [None] * self.n, [None] * self.n, [None] * self.n
        done = set()
        if pose_init == "pnp":
            return self._init_pnp(pred, conf, focal, raymaps, niter_PnP, pnp_seed, pnp_backend)
        if pose_init == "prefix":
            return self._init_prefix(pred, conf, focal, niter_PnP, pnp_seed, pnp_backend)
        if pose_init != "traj":
            raise ValueError(f"pose_init={pose_init!r}: 'traj', 'pnp' or 'prefix'")
        for k, i in enumerate(self.groups[0]):
            pts3d[i], conf_list[i], im_poses[i] = pred[0, k].clone(), conf[0, k].clone(), traj[0, k].clone().float()
            done.add(i)
        for g in range(1, G):
            grp = self.groups[g]
            seen = [k for k, i in enumerate(grp) if i in done]
            assert seen and grp[0] in done, "the first image of every window must belong to an earlier window"
            s, R, T = rigid_points_registration(pred[g, seen], torch.stack([pts3d[grp[k]] for k in seen]),
                                                torch.stack([conf[g, k] * conf_list[grp[k]] for k in seen]))
            for k, i in enumerate(grp):       # later windows overwrite earlier estimates, as the reference does
                pts3d[i], conf_list[i] = s * (pred[g, k] @ R.t()) + T, conf[g, k].clone()
                done.add(i)
                M = torch.eye(4, device=self.dev)
                M[:3, :3] = R @ traj[g, k, :3, :3].float()
                M[:3, 3] = s * (R @ traj[g, k, :3, 3].float()) + T
                im_poses[i] = M
        # pairwise poses: register every window onto the chained cloud
        for g, grp in enumerate(self.groups):
            s, R, T = rigid_points_registration(pred[g], torch.stack([pts3d[i] for i in grp]), torch.stack([conf[g, k] * conf_list[i] for k, i in enumerate(grp)]))
            self.P["pw_poses"][g, :4] = rotmat_to_quat(R).to(self.dev)
            self.P["pw_poses"][g, 4:7] = signed_log1p(T / s)
            self.P["pw_poses"][g, 7] = torch.log(s)
        sf = float((math.log(self.base_scale) - self.P["pw_poses"][:, -1].mean()).exp()) if self.norm_pw_scale else 1.0
        if focal is None and raymaps is not None:
            first = {}
            for g, grp in enumerate(self.groups):
                for k, i in enumerate(grp):
                    first.setdefault(i, (g, k))
            rm = raymaps.reshape(G, S, H, W, 3)
            per_image = estimate_focal_weiszfeld(torch.stack([rm[g, k] for g, k in (first[i] for i in range(self.n))]).to(self.dev), pp=self._init_pp())
            per_image = torch.where(torch.isfinite(per_image) & (per_image > 0), per_image, torch.full_like(per_image, max(H, W) / (2.0 * math.tan(math.radians(30.0)))))
            self.init_focals = per_image
            focal = float(per_image.mean()) if self.shared_focal else per_image
        if focal is None:
            p0, ys, xs = pred[0, 0], *torch.meshgrid(torch.arange(H, device=self.dev), torch.arange(W, device=self.dev), indexing="ij")
            pp0 = self._init_pp(self.groups[0][0])                  # window 0's first image
            u, v = (xs.reshape(-1).float() - (W / 2 if pp0 is None else pp0[0])), (ys.reshape(-1).float() - (H / 2 if pp0 is None else pp0[1]))
            ok = (p0[:, 2] > 1e-6) & (conf[0, 0] > 0.5)
            fx = (u * p0[:, 2] / p0[:, 0])[ok & (u.abs() > W / 8)]
            fy = (v * p0[:, 2] / p0[:, 1])[ok & (v.abs() > H / 8)]
            cand = torch.cat([fx[torch.isfinite(fx)], fy[torch.isfinite(fy)]])
            focal = float(cand.median()) if cand.numel() else float(max(H, W))
        # degenerate predictions (e.g. the synthetic noise maps of bench.py's clip mode) can yield a non-positive / non-finite estimate, whose
        # log the reference would carry into the optimisation as NaN: fall back to the 60-degree field of view dust3r's estimator is scaled by
        fbase = max(H, W) / (2.0 * math.tan(math.radians(30.0)))
        if torch.is_tensor(focal):
            focal = torch.where(torch.isfinite(focal) & (focal > 0), focal, torch.full_like(focal, fbase))
            self.P["im_focals"][:, 0] = FOCAL_BREAK * torch.log(focal)
        else:
            if not (math.isfinite(focal) and focal > 0):
                focal = fbase
            self.P["im_focals"][:] = FOCAL_BREAK * math.log(focal)
        sky = 0.0
        for i in range(self.n):
            M = im_poses[i].clone()
            M[:3, 3] *= sf
            Rw, tw = M[:3, :3], M[:3, 3]
            depth = ((pts3d[i] * sf - tw) @ Rw)[:, 2]                      # z of R^T (X - t)
            skym = conf_list[i] < 1e-4
            if i == 0:
                sky = depth.max()
            depth = torch.where(skym, torch.as_tensor(sky, device=self.dev), depth)
            self.P["im_depthmaps"][i] = depth.clamp_min(1e-6).log().nan_to_num(neginf=0)
            self.P["im_poses"][i, :4] = rotmat_to_quat(Rw).to(self.dev)
            self.P["im_poses"][i, 4:7] = signed_log1p(tw)
        return self


class _DevicePnp:
    """What the device backend of the "pnp" / "prefix" initialisations keeps: the sampler's tables of every (window, frame) slot, uploaded
    once (the masked-pixel counts come from ONE reduction and ONE host copy before the chain starts), the per-image focals (NaN = unset)
    and camera-to-world poses (identity = unset) as device arrays ops.pnp_ransac writes in place on success, and the status words."""

    def __init__(self, scene, conf, niter_PnP, seed):
        from . import ops, pnp
        G, S = scene.G, scene.S
        counts = (conf > 0.5).sum(-1).reshape(-1).cpu().tolist()                              # the one host wait before the chain
        self.tables = ops.PnpTables([pnp.sample_tables(n, niter_PnP, seed) for n in counts], counts, niter_PnP, scene.dev)
        self.scene, self.iterations = scene, int(niter_PnP)
        self.focals = torch.full((scene.n,), float("nan"), device=scene.dev, dtype=torch.float64)
        self.poses = torch.eye(4, device=scene.dev, dtype=torch.float64).repeat(scene.n, 1, 1)
        self.status = torch.full((G * S,), -1, device=scene.dev, dtype=torch.int32)          # -1: the slot was not solved
        self.delta = 0.03 * max(scene.H, scene.W)                                            # fast_pnp's -/+ 3 % of the image size
        self.pp = None                                                                       # one principal point per call (geo4d_pnp_ransac's ppx, ppy)
        pp = scene._init_pp()
        if pp is not None:
            pp = pp.cpu()
            if bool((pp != pp[0]).any()):
                raise ValueError("pnp_backend='device' takes ONE principal point per launch (geo4d_pnp_ransac's ppx, ppy), but the preset "
                                 "principal points differ between images: use pnp_backend='host'")
            self.pp = (float(pp[0, 0]), float(pp[0, 1]))

    def solve(self, slots, points, conf, base, focal_out, pose_out):
        """One launch for the `slots` (flat window * S + frame indices) with points [B, H W, 3], conf [B, H W], base focals [B] fp64."""
        from . import ops
        sc, B = self.scene, len(slots)
        cand = torch.stack([base, -self.delta + base, self.delta + base], 1)                 # fast_pnp: [focal] + geomspace(-d + focal, d + focal, 2)
        _, _, status, _ = ops.pnp_ransac(points.reshape(B, sc.H, sc.W, 3), conf.reshape(B, sc.H, sc.W), cand, self.tables.rows(slots),
                                         iterations=self.iterations, pp=self.pp, out=(focal_out, pose_out))
        if slots == list(range(slots[0], slots[0] + B)):
            self.status[slots[0]:slots[0] + B] = status
        else:
            self.status[torch.as_tensor(slots, device=sc.dev)] = status

    def finish(self):
        """The one copy at the end: (status words [G, S], focals as the host path's list (None = unset), poses as its fp32 list)."""
        sc = self.scene
        host = torch.cat([self.status.double(), self.focals]).cpu()
        status = host[:sc.G * sc.S].to(torch.int32).reshape(sc.G, sc.S)
        focals = [None if math.isnan(f) else f for f in host[sc.G * sc.S:].tolist()]
        return status, focals, [M.float() for M in self.poses]


def host_pp(scene, i):
    """Image i's principal point for the host PnP backend (pnp.fast_pnp's `pp`): None = the image centre when the scene has no im_pp."""
    pp = scene._init_pp(i)
    return None if pp is None else pp.cpu().numpy()


def _record_pnp_status(self, status):
    """pnp_status [G, S] int32 of the last "pnp" / "prefix" initialisation: -1 slot not solved, 0 solved, else the failure (the device
    backend's status bits of ops.pnp_ransac; the host backend knows only success, and records 1 for any failure)."""
    self.pnp_status = status


def _init_pnp(self, pred, conf, focal, raymaps, niter_PnP, seed, backend="host"):
    """GroupAligner.init_from_group(pose_init="pnp"): align_group + init_from_pts3d_group of the reference (see the docstring there).
    backend "device": the first window's images in one ops.pnp_ransac launch, every later window's newly seen images in one launch, base
    focals from estimate_focal_weiszfeld kept on the device; results are applied only where the host code applies them (an image's
    first pose, the focal of first-window images). A base focal the solver cannot use (no ray maps: the host would search 63 candidates)
    reruns the whole initialisation on the host."""
    from . import pnp
    G, S, H, W = self.G, self.S, self.H, self.W
    pts3d, conf_list, im_poses, im_focals = [None] * self.n, [None] * self.n, [None] * self.n, [None] * self.n
    rm = None if raymaps is None else raymaps.reshape(G, S, H, W, 3)

    def ray_pp(i):                                                          # [1, 2] principal point of image i (None: the centre)
        pp = self._init_pp(i)
        return None if pp is None else pp[None]
    if backend == "device":
        dp = _DevicePnp(self, conf, niter_PnP, seed)

        def launch(g, ks, first_window):
            idx = torch.as_tensor([self.groups[g][k] for k in ks], device=self.dev)
            # per image, as the host path calls it: a batched reduction may round differently, and the candidates must be the same bits
            base = (torch.cat([estimate_focal_weiszfeld(rm[g, k][None].to(self.dev), pp=ray_pp(self.groups[g][k])) for k in ks]).double() if rm is not None
                    else torch.full((len(ks),), float("nan"), device=self.dev, dtype=torch.float64))
            fo, po = base.clone(), dp.poses[idx]
            dp.solve([g * S + k for k in ks], torch.stack([pts3d[self.groups[g][k]] for k in ks]), conf[g, ks], base, fo, po)
            dp.focals[idx] = fo if first_window else base
            dp.poses[idx] = po
        for k, i in enumerate(self.groups[0]):
            pts3d[i], conf_list[i] = pred[0, k].clone(), conf[0, k].clone()
        launch(0, list(range(len(self.groups[0]))), True)
        for g in range(1, G):
            grp = self.groups[g]
            assert pts3d[grp[0]] is not None, "the first image of every window must belong to an earlier window"
            seen = [k for k, i in enumerate(grp) if pts3d[i] is not None]
            s, R, T = rigid_points_registration(pred[g, seen], torch.stack([pts3d[grp[k]] for k in seen]),
                                                torch.stack([conf[g, k] * conf_list[grp[k]] for k in seen]))
            new = [k for k, i in enumerate(grp) if pts3d[i] is None]
            for k in new:
                pts3d[grp[k]], conf_list[grp[k]] = s * (pred[g, k] @ R.t()) + T, conf[g, k].clone()
            if new:
                launch(g, new, False)
        status, im_focals, im_poses = dp.finish()
        if bool(((status > 0) & ((status & 4) != 0)).any()):
            return self._init_pnp(pred, conf, focal, raymaps, niter_PnP, seed, "host")
        _record_pnp_status(self, status)
        return self._finish_group_init(pred, conf, pts3d, conf_list, im_poses, im_focals, focal)
    ok = torch.full((G, S), -1, dtype=torch.int32)

    def ray_focal(g, k):
        return None if rm is None else float(estimate_focal_weiszfeld(rm[g, k][None].to(self.dev), pp=ray_pp(self.groups[g][k]))[0])

    def run_pnp(i, g, k):
        msk = (conf[g, k] > 0.5).reshape(H, W).cpu().numpy()
        return pnp.fast_pnp(pts3d[i].reshape(H, W, 3).double().cpu().numpy(), im_focals[i], msk, pp=host_pp(self, i), niter_PnP=niter_PnP, seed=seed)
    done = set()
    for k, i in enumerate(self.groups[0]):                                  # the first window is the world frame
        pts3d[i], conf_list[i] = pred[0, k].clone(), conf[0, k].clone()
        im_focals[i] = ray_focal(0, k)
        res = run_pnp(i, 0, k)
        ok[0, k] = 0 if res else 1
        if res:
            im_focals[i], im_poses[i] = res[0], torch.from_numpy(res[1]).float().to(self.dev)
        if im_poses[i] is None:
            im_poses[i] = torch.eye(4, device=self.dev)
        done.add(i)
    for g in range(1, G):
        grp = self.groups[g]
        assert grp[0] in done, "the first image of every window must belong to an earlier window"
        seen = [k for k, i in enumerate(grp) if i in done]
        s, R, T = rigid_points_registration(pred[g, seen], torch.stack([pts3d[grp[k]] for k in seen]),
                                            torch.stack([conf[g, k] * conf_list[grp[k]] for k in seen]))
        for k, i in enumerate(grp):
            if pts3d[i] is None:                                            # an image keeps its FIRST chained estimate
                pts3d[i], conf_list[i] = s * (pred[g, k] @ R.t()) + T, conf[g, k].clone()
                done.add(i)
            if im_focals[i] is None:
                im_focals[i] = ray_focal(g, k)
            # the PnP result is only used where pose / focal are still unset (both assignments below are `is None`-guarded, as in the
            # reference) and the solver's sampler is re-seeded per call: skipping the call for already-initialised images (~3 of 4
            # occurrences at stride 4) changes nothing but the start-up time (host-side numpy RANSAC)
            res = None
            if im_poses[i] is None or im_focals[i] is None:
                res = run_pnp(i, g, k)
                ok[g, k] = 0 if res else 1
            if res:
                if im_poses[i] is None:
                    im_poses[i] = torch.from_numpy(res[1]).float().to(self.dev)
                if im_focals[i] is None:
                    im_focals[i] = res[0]
            if im_poses[i] is None:
                im_poses[i] = torch.eye(4, device=self.dev)
    _record_pnp_status(self, ok)
    return self._finish_group_init(pred, conf, pts3d, conf_list, im_poses, im_focals, focal)


def _finish_group_init(self, pred, conf, pts3d, conf_list, im_poses, im_focals, focal):
    """init_from_pts3d_group (init_im_poses.py:569-635) on the chained clouds: pairwise poses, scale normalisation, depth maps, camera
    poses and the focal(s)."""
    H, W = self.H, self.W
    for g, grp in enumerate(self.groups):                                   # pairwise poses: every window onto the chained cloud
        s, R, T = rigid_points_registration(pred[g], torch.stack([pts3d[i] for i in grp]), torch.stack([conf[g, k] * conf_list[i] for k, i in enumerate(grp)]))
        self.P["pw_poses"][g, :4] = rotmat_to_quat(R).to(self.dev)
        self.P["pw_poses"][g, 4:7] = signed_log1p(T / s)
        self.P["pw_poses"][g, 7] = torch.log(s)
    sf = float((math.log(self.base_scale) - self.P["pw_poses"][:, -1].mean()).exp()) if self.norm_pw_scale else 1.0
    self.init_focals = torch.tensor([f if f is not None else float(max(H, W)) for f in im_focals], device=self.dev)
    if focal is not None:
        self.P["im_focals"][:] = FOCAL_BREAK * (torch.log(focal) if torch.is_tensor(focal) else math.log(focal))
    elif self.shared_focal:
        self.P["im_focals"][:] = FOCAL_BREAK * math.log(float(self.init_focals.mean()))
    else:
        self.P["im_focals"][:, 0] = FOCAL_BREAK * torch.log(self.init_focals)
    sky = 0.0
    for i in range(self.n):
        M = im_poses[i].clone()
        M[:3, 3] *= sf
        Rw, tw = M[:3, :3], M[:3, 3]
        depth = ((pts3d[i] * sf - tw) @ Rw)[:, 2]
        skym = conf_list[i] < 1e-4
        if i == 0:
            sky = depth.max()
        depth = torch.where(skym, torch.as_tensor(sky, device=self.dev), depth)
        self.P["im_depthmaps"][i] = depth.clamp_min(1e-6).log().nan_to_num(neginf=0)
        self.P["im_poses"][i, :4] = rotmat_to_quat(Rw).to(self.dev)
        self.P["im_poses"][i, 4:7] = signed_log1p(tw)
    return self


GroupAligner._init_pnp = _init_pnp
GroupAligner._finish_group_init = _finish_group_init


def filter_outlier_focals(focal_group):
    """init_im_poses.align_group_prefix :264-269 on the per-window focals (pixels): the mean over focals above 30 replaces every focal
    whose relative distance to that mean exceeds 0.6. Returns (filtered copy, mean)."""
    focal_group = focal_group.clone()
    mean = focal_group[focal_group > 30].mean()
    focal_group[torch.abs(focal_group - mean) / mean > 0.6] = mean
    return focal_group, mean


def _init_prefix(self, pred, conf, focal, niter_PnP, seed, backend="host"):
    """GroupAligner.init_from_group(pose_init="prefix"): align_group_prefix + init_from_pts3d_group of the reference.
      1. the reference frame of every window, z - min(z) + 1 with ONE min over all of them (:259-260), pixels with confidence > 0.5, the
         shift / focal solve at full resolution (:261) -> one focal in pixels per window (:262-263), outliers replaced (:264-269);
         a map the solver cannot fit takes the reference's `except` path: PnP without a focal on window 0's first frame, one focal
         for all windows (:272-277). Device-resident up to the G focals and status words, which cross to the host in one copy.
      2. window 0 is the world frame; later windows are registered onto the chained cloud and OVERWRITE the point map and confidence
         of the images they share with it (:347-355).
      3. every image of every window: RANSAC-PnP started at `temp_focal` = the window's focal for its reference frame, else the current
         focal of the PREVIOUS image (:307-311, 372-376); pose and focal are overwritten on success (:381-388).
    backend "device": step 3 through ops.pnp_ransac in the same order, one launch per image (B = 1, C = 3). The candidates are built on the
    device from the device-resident focal array the previous launch wrote (or left alone, when it failed: the earlier window's value
    stays), so between the masked-pixel counts copied up front and the status words copied at the end the PnP chain reads nothing back;
    the window registrations of step 2 keep their own 3 x 3 host solve. A start focal that is unset or unusable (where the host would
    search 63 candidates) reruns the whole initialisation on the host. The `except` path of step 1 stays on the host.
    Principal points: the PnP of step 3 (and of the `except` path) takes each image's own; step 1's focal / shift solve has no
    principal-point argument (nor has the reference's point_map_to_depth) and stays centred - its focal is only PnP's first candidate."""
    from . import geometry, pnp
    G, S, H, W = self.G, self.S, self.H, self.W
    pts3d, conf_list, im_poses, im_focals = [None] * self.n, [None] * self.n, [None] * self.n, [None] * self.n
    ref_pts = self.pred.reshape(G, S, H, W, 3)[:, 0]                            # strided views: solved in place
    ref_conf = self.conf.reshape(G, S, H, W)[:, 0]
    z_offset = (1.0 - ref_pts[..., 2].min()).reshape(1)
    focal_px, status = geometry.recover_focal_pixels(ref_pts, ref_conf, (H, W), z_offset=z_offset, return_status=True)
    host = torch.stack([focal_px, status.float()]).cpu()                        # the one copy: 2 G numbers
    self.prefix_focals_raw = host[0].clone()
    if bool((host[1] != 0).any()):
        res = pnp.fast_pnp(pred[0, 0].reshape(H, W, 3).double().cpu().numpy(), None, (conf[0, 0] > 0.5).reshape(H, W).cpu().numpy(),
                           pp=host_pp(self, self.groups[0][0]), niter_PnP=niter_PnP, seed=seed)
        focal_group = [res[0] if res else max(H, W) / (2.0 * math.tan(math.radians(30.0)))] * G
    else:
        focal_group = filter_outlier_focals(host[0])[0].numpy().tolist()
    self.prefix_focals = torch.tensor(focal_group)

    def run_pnp(i, g, k, temp_focal):
        msk = (conf[g, k] > 0.5).reshape(H, W).cpu().numpy()
        return pnp.fast_pnp(pts3d[i].reshape(H, W, 3).double().cpu().numpy(), temp_focal, msk, pp=host_pp(self, i), niter_PnP=niter_PnP, seed=seed)
    done = set()
    dp = _DevicePnp(self, conf, niter_PnP, seed) if backend == "device" else None
    window_focals = torch.tensor(focal_group, dtype=torch.float64, device=self.dev) if dp else None
    ok = torch.full((G, S), -1, dtype=torch.int32)
    for g, grp in enumerate(self.groups):
        if g:
            assert grp[0] in done, "the first image of every window must belong to an earlier window"
            seen = [k for k, i in enumerate(grp) if i in done]
            s, R, T = rigid_points_registration(pred[g, seen], torch.stack([pts3d[grp[k]] for k in seen]),
                                                torch.stack([conf[g, k] * conf_list[grp[k]] for k in seen]))
        for k, i in enumerate(grp):
            if dp:                                                   # the same bookkeeping on the device-resident focal array
                if g == 0:
                    if k == 0:
                        dp.focals[i] = window_focals[0]
                    pts3d[i], conf_list[i] = pred[0, k].clone(), conf[0, k].clone()
                    temp = dp.focals[i - 1:i] if i != 0 else dp.focals[i:i + 1]
                else:
                    pts3d[i], conf_list[i] = s * (pred[g, k] @ R.t()) + T, conf[g, k].clone()
                    temp = window_focals[g:g + 1] if k == 0 else dp.focals[i - 1:i]
                done.add(i)
                dp.solve([g * S + k], pts3d[i][None], conf[g, k][None], temp.clone(), dp.focals[i:i + 1], dp.poses[i:i + 1])
                continue
            if g == 0:
                if k == 0:
                    im_focals[i] = focal_group[0]
                pts3d[i], conf_list[i] = pred[0, k].clone(), conf[0, k].clone()
                temp_focal = im_focals[i - 1] if i != 0 else im_focals[i]
            else:
                pts3d[i], conf_list[i] = s * (pred[g, k] @ R.t()) + T, conf[g, k].clone()
                temp_focal = focal_group[g] if k == 0 else im_focals[i - 1]
            done.add(i)
            res = run_pnp(i, g, k, temp_focal)
            ok[g, k] = 0 if res else 1
            if res:
                im_focals[i], im_poses[i] = res[0], torch.from_numpy(res[1]).float().to(self.dev)
            if im_poses[i] is None:
                im_poses[i] = torch.eye(4, device=self.dev)
    if dp:
        ok, im_focals, im_poses = dp.finish()
        if bool(((ok > 0) & ((ok & 4) != 0)).any()):
            return self._init_prefix(pred, conf, focal, niter_PnP, seed, "host")
    _record_pnp_status(self, ok)
    return self._finish_group_init(pred, conf, pts3d, conf_list, im_poses, im_focals, focal)


GroupAligner._init_prefix = _init_prefix


def post_optimization(slices, maps, traj, args=None, conf_optimize=True, lr=0.03, align=True, intrinsics=None,
                      use_raymap=True, use_inverse_depthmap=True, use_traj=True, pointmap_vae_used=True, depth_traj_start_iter=150,
                      sharded=None, pose_init="traj", imgs=None, pnp_backend="host", optimize_pp=False, principal_points=None):
    """The consumer of the gathered clip: ``post_optimization`` of scripts/evaluation/test_geo4d.py:30-51 with the pred_list its
    window loop builds (:446-501). ``slices`` / ``maps [n_windows, 11, T, H, W]`` / ``traj [n_windows, T, 4, 4]`` are what
    ``pipeline.run_clip(..., with_cameras=True)`` returns; ``args`` = the config's ``postprocess`` tree (a dict or any object with
    n_iter / pose_schedule / temporal_smoothing_weight / translation_weight / not_shared_focal / use_gt_focal attributes; None =
    the shipped values). ``sharded``: None = shard the optimisation over the ranks of the default process group when there is one
    (align_dist.AlignShard: every rank evaluates its block of windows, one all-reduce per iteration), False = replicate it.
    Returns the optimised ``GroupAligner`` (``get_depthmaps`` / ``get_im_poses_matrix`` / ``get_focals``).
    ``intrinsics [n_images, 3, 3]`` presets the focals and freezes them (scene.preset_focal(..., requires_grad=False) in the script).
    ``imgs``: the clip's frames in [-1, 1] (``[1, 3, T, H, W]`` as run_clip takes them, ``[3, T, H, W]`` or ``[T, 3, H, W]``) or uint8,
    kept as ``scene.imgs`` [n, H, W, 3] in [0, 1] (dust3r.utils.image.rgb) for the export (geo4d_amd/scene_export.py).
    ``pose_init``: "traj" (default, Plücker cameras), "pnp" (align_group, the reference's opt_raydir branch) or "prefix"
    (align_group_prefix, what the reference's script runs with its use_raymap = False): GroupAligner.init_from_group.
    ``pnp_backend``: "host" (default) or "device", the RANSAC-PnP backend of the "pnp" and "prefix" initialisations.
    ``optimize_pp``: optimise one principal point per image (the reference's ``optimize_pp``, forwarded to the optimiser by its
    ``post_optimization(**kwargs)``), starting at the image centre unless preset. ``principal_points``: ``[n_images, 2]`` pixels, or
    ``"intrinsics"`` = ``intrinsics[:, :2, 2]``: preset and frozen (``scene.preset_principal_point``) BEFORE the initialisation, the
    reference's order. With both defaults the principal points stay at the image centre, also when ``intrinsics`` is passed."""
    from .pipeline import postprocess_window
    groups = [list(range(s.start, s.stop)) for s in slices]
    n_images = 1 + max(max(g) for g in groups)
    if isinstance(principal_points, str):
        if principal_points != "intrinsics":
            raise ValueError(f"principal_points={principal_points!r}: an [n_images, 2] array of pixels or 'intrinsics'")
        if intrinsics is None:
            raise ValueError("principal_points='intrinsics' needs intrinsics")
        principal_points = torch.as_tensor(intrinsics)[:, :2, 2]
    if principal_points is not None:
        principal_points = torch.as_tensor(principal_points).detach().float().cpu()
        if tuple(principal_points.shape) != (n_images, 2):
            raise ValueError(f"principal_points: expected [{n_images}, 2] pixel coordinates, got shape {tuple(principal_points.shape)}")
    get = (lambda k, d: args.get(k, d)) if isinstance(args, dict) else (lambda k, d: getattr(args, k, d))
    if args is None:
        get = lambda k, d: d
    post = [postprocess_window(m[None], pointmap_vae_used=pointmap_vae_used) for m in maps]
    conf = torch.stack([p["conf"][..., 0] for p in post])
    if not conf_optimize:
        conf = torch.ones_like(conf)
    shard = None
    if sharded or (sharded is None and torch.distributed.is_available() and torch.distributed.is_initialized()
                   and torch.distributed.get_world_size() > 1):
        from .align_dist import make_shard
        shard = make_shard(groups, 1 + max(max(g) for g in groups))     # None when the clip has fewer windows than ranks (replicated run)
    scene = GroupAligner(groups, torch.stack([p["pts3d"] for p in post]), conf, shard=shard,
                         shared_focal=not get("not_shared_focal", False) and not get("use_gt_focal", False),
                         temporal_smoothing_weight=get("temporal_smoothing_weight", 0.015), translation_weight=get("translation_weight", 1.0),
                         inverse_depth=torch.stack([p["inverse_depthmap"] for p in post]) if use_inverse_depthmap else None,
                         traj=traj if use_traj else None, depth_traj_start_iter=depth_traj_start_iter, optimize_pp=optimize_pp)
    if principal_points is not None:
        scene.preset_principal_point(principal_points)
    focal = None
    if intrinsics is not None:
        per_image = (intrinsics[:, 0, 0] + intrinsics[:, 1, 1]) / 2.0
        focal = per_image.to(scene.dev).float() if not scene.shared_focal else float(per_image.float().mean())
    scene.init_from_group(traj, focal=focal, raymaps=torch.stack([p["raymap"] for p in post]) if use_raymap else None, pose_init=pose_init,
                          pnp_backend=pnp_backend)
    if intrinsics is not None:
        scene.frozen.add("im_focals")
    if imgs is not None:
        scene.imgs = rgb_frames(imgs, scene.n, scene.H, scene.W).to(scene.dev)
    if align:
        scene.compute_global_alignment(niter=get("n_iter", 500), schedule=get("pose_schedule", "linear"), lr=lr)
    return scene


def rgb_frames(frames, n, H, W):
    """dust3r.utils.image.rgb on a clip -> [n, H, W, 3] fp32 in [0, 1]: floats x * 0.5 + 0.5 clipped, uint8 x / 255. Layouts: [1, 3, T, H, W]
    and [3, T, H, W] (load_video_batch / run_clip), [T, 3, H, W] (rgb's own), [T, H, W, 3]."""
    x = torch.as_tensor(frames)
    if x.dim() == 5 and x.shape[0] == 1:
        x = x[0]
    if x.dim() == 4 and x.shape[1] == 3 and x.shape[-1] != 3:
        x = x.permute(0, 2, 3, 1)
    elif x.dim() == 4 and x.shape[0] == 3 and x.shape[-1] != 3:
        x = x.permute(1, 2, 3, 0)
    if tuple(x.shape) != (n, H, W, 3):
        raise ValueError(f"imgs: expected {n} frames of {H} x {W} RGB, got shape {tuple(torch.as_tensor(frames).shape)}")
    x = x.float() / 255 if x.dtype == torch.uint8 else (x.float() * 0.5 + 0.5).clip(0, 1)
    return x.contiguous()
