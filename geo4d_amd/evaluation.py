"""Video-depth and camera-pose evaluation against ground truth: what ``scripts/evaluation/infer_geo4d.py`` runs after
``post_optimization`` (:514-545 depth, :559-610 pose, :612-621 averages), behind the call surface of the two functions it binds.

* ``depth_evaluation`` = ``dust3r/depth_eval.py depth_evaluation`` (:147-355) for the alignments the Geo4D entry scripts use: the
  least-absolute-deviation fit ``align_with_lad2`` (with and without ``align_mask``) and the default median scaling. The hot part runs
  in csrc/depth_eval.hip and csrc/align.hip: an order-preserving compaction of the valid pixels, the bit-exact ``torch.median`` radix
  select and the one-launch-per-iteration Adam LAD fit, then one fused metrics + error-map pass that reads (s, t) from the device.
  There is no CPU fallback.
* ``eval_metrics`` = ``dust3r/utils/vo_eval.py eval_metrics`` (:174-258): ATE and RPE under evo's sim(3) alignment, restated in fp64
  numpy (evo is not a dependency).
* ``evaluate_scene`` / ``average_depth_metrics``: the glue of infer_geo4d.py around them.
* ``cloud_metrics`` / ``scene_cloud_metrics``: accuracy, completeness, Chamfer distance and precision / recall / F-score of a point
  cloud against a ground-truth cloud, on the nearest-neighbour search of csrc/nearest.hip (``geo4d_amd.nearest``). The reference has
  no such step; the rule is this project's own (include/geo4d_hip.h, tests/nearest_restatement.py).
"""
import math
import os

import numpy as np
import torch

from . import _lib, io, ops
from .align import relative_pose_errors, rigid_points_registration, rotation_angle_deg
from .fusion import fuse_points
from .motion import segment_motion
from .nearest import _cloud, check_cloud, check_radius, nearest_points
from .scene_view import MOTION, scene_view

DEPTH_KEYS = ("Abs Rel", "Sq Rel", "RMSE", "Log RMSE", "δ < 1.25", "δ < 1.25^2", "δ < 1.25^3")


def _as_tensor(x):
    return torch.from_numpy(x) if isinstance(x, np.ndarray) else x


def depth_evaluation(predicted_depth_original, ground_truth_depth_original, max_depth=80, custom_mask=None, post_clip_min=None,
                     post_clip_max=None, pre_clip_min=None, pre_clip_max=None, align_with_lstsq=False, align_with_lad=False,
                     align_with_lad2=False, lr=1e-4, max_iters=1000, use_gpu=True, align_with_scale=False, disp_input=False, align_mask=None,
                     return_st=False):
    """depth_eval.py depth_evaluation (:147-355) on the HIP device -> (results, error map, s * pred + t, gt where valid).

    ``results`` has the reference's keys ('Abs Rel', 'Sq Rel', 'RMSE', 'Log RMSE', the three δ ratios, 'valid_pixels', and 's' / 't' with
    ``return_st``). Valid pixels are ``gt > 0`` (and ``gt < max_depth`` unless it is None); the fit uses those inside ``align_mask``, the
    metrics those inside ``custom_mask``; the error map covers every valid pixel. The maps have the shape the reference gives them
    (``[T * h, w]`` for a ``[T, h, w]`` input). Depths are fp32. ``use_gpu=True`` moves the inputs to the current device as the reference
    does; CPU inputs with ``use_gpu=False`` raise (there is no CPU path). The host waits twice: for the number of fit pixels (the median
    and the fit are sized by it) and for the final sums. No fit pixel raises ValueError (the reference fails inside torch.median); no
    metric pixel gives the reference's all-zero metrics. The median-scaling path reports s = the scale, t = 0 under ``return_st``."""
    for flag, name in ((align_with_lstsq, "align_with_lstsq"), (align_with_lad, "align_with_lad"), (align_with_scale, "align_with_scale"),
                       (disp_input, "disp_input")):
        if flag:
            raise NotImplementedError(f"depth_evaluation: {name} is not implemented (only align_with_lad2 and the default median scaling, "
                                      "which are what the Geo4D evaluation scripts use)")
    pred, gt = _as_tensor(predicted_depth_original), _as_tensor(ground_truth_depth_original)
    custom_mask, align_mask = _as_tensor(custom_mask), _as_tensor(align_mask)
    if pred.dim() == 3:                                   # :177-183
        w = pred.shape[-1]
        pred, gt = pred.reshape(-1, w), gt.reshape(-1, w)
    if use_gpu:
        pred, gt = pred.cuda(), gt.cuda()
    if not (pred.is_cuda and gt.is_cuda):
        raise _lib.Geo4DNativeError("geo4d_amd.evaluation.depth_evaluation runs only on a HIP device (there is no CPU fallback)")
    if pred.shape != gt.shape:
        raise ValueError(f"depth_evaluation: prediction {tuple(pred.shape)} and ground truth {tuple(gt.shape)} differ in shape")
    if custom_mask is not None and custom_mask.numel() != gt.numel():
        raise ValueError("depth_evaluation: custom_mask must have the ground truth's shape")
    if align_mask is not None and align_mask.numel() != gt.numel():
        raise ValueError("depth_evaluation: align_mask must have the ground truth's shape")
    dev = gt.device
    pf, gf = pred.detach().float().contiguous().reshape(-1), gt.detach().float().contiguous().reshape(-1)
    dmask = lambda m: None if m is None else m.to(dev).reshape(-1)
    lib = _lib.load()

    pv, gv, count = ops.masked_select(pf, gf, max_depth=max_depth, mask=dmask(align_mask), pre_clip_min=pre_clip_min, pre_clip_max=pre_clip_max)
    n = int(count.item())
    if n == 0:
        raise ValueError("depth_evaluation: no valid ground-truth pixel to align with (gt > 0, gt < max_depth, align_mask)")
    if align_with_lad2:
        st = torch.empty(2, device=dev, dtype=torch.float32)
        need = lib.geo4d_lad_workspace(1, n)
        ws = torch.empty((need + 7) // 8, device=dev, dtype=torch.float64)
        _lib.check(lib.geo4d_lad_fit(pv.data_ptr(), gv.data_ptr(), 1, n, None, float(lr), int(max_iters), 1e-6, st.data_ptr(), None,
                                     ws.data_ptr(), need, ops._stream()), "geo4d_lad_fit")
    else:                                                 # median scaling (:242-245, :265-268): scale = median(gt) / median(pred), no shift
        med = torch.empty(2, device=dev, dtype=torch.float32)
        ws = torch.empty(260, device=dev, dtype=torch.int32)
        for k, x in enumerate((gv, pv)):
            _lib.check(lib.geo4d_lower_median(x.data_ptr(), 1, n, med[k:].data_ptr(), ws.data_ptr(), ws.numel() * 4, ops._stream()),
                       "geo4d_lower_median")
        st = torch.stack([med[0] / med[1], torch.zeros((), device=dev)])

    sums, err, aligned = ops.depth_metrics(pf, gf, st, max_depth=max_depth, custom_mask=dmask(custom_mask), pre_clip_min=pre_clip_min,
                                           pre_clip_max=pre_clip_max, post_clip_min=post_clip_min, post_clip_max=post_clip_max, aligned=True)
    valid = (gf > 0) if max_depth is None else (gf > 0) & (gf < max_depth)
    gt_map = torch.where(valid, gf, torch.zeros_like(gf))
    host = torch.cat([sums, st.double()]).cpu().tolist()
    S, (s, t) = host[:8], host[8:]
    m = int(S[7])
    if m == 0:
        vals = [0] * 7
    else:
        vals = [S[0] / m, S[1] / m, math.sqrt(S[2] / m), math.sqrt(S[3] / m), S[4] / m, S[5] / m, S[6] / m]
    results = dict(zip(DEPTH_KEYS, vals))
    results["valid_pixels"] = m
    if return_st:
        results["s"], results["t"] = s, t
    shape = gt.shape
    return results, err.reshape(shape), aligned.reshape(shape), gt_map.reshape(shape)


def average_depth_metrics(results):
    """infer_geo4d.py:612-621: every metric averaged over sequences weighted by their 'valid_pixels'."""
    return {k: np.average([r[k] for r in results], weights=[r["valid_pixels"] for r in results]) for k in results[0] if k != "valid_pixels"}


# ---- camera poses ------------------------------------------------------------------------------------------------------------------
def _tum_to_mats(poses):
    from scipy.spatial.transform import Rotation
    poses = np.asarray(poses, dtype=np.float64)
    M = np.tile(np.eye(4), (len(poses), 1, 1))
    M[:, :3, :3] = Rotation.from_quat(poses[:, [4, 5, 6, 3]]).as_matrix()      # x y z qw qx qy qz -> scipy's x y z w
    M[:, :3, 3] = poses[:, :3]
    return M


def _associate(ref_t, est_t, max_diff=0.01):
    """evo sync.associate_trajectories: every stamp of the shorter trajectory matched to the nearest stamp of the longer one within max_diff."""
    est_longer = len(est_t) > len(ref_t)
    short, long_ = (ref_t, est_t) if est_longer else (est_t, ref_t)
    i_short, i_long = [], []
    for i, ts in enumerate(short):
        j = int(np.argmin(np.abs(long_ - ts)))
        if abs(long_[j] - ts) <= max_diff:
            i_short.append(i)
            i_long.append(j)
    if not i_short:
        raise ValueError("eval_metrics: no matching timestamps between the estimate and the reference")
    return (i_short, i_long) if est_longer else (i_long, i_short)


def _sim3_fit(est, ref):
    """(s, R, T) fp64 of the Umeyama sim(3) that takes the estimated positions onto the reference ones (unit weights): x -> s R x + T."""
    x, y = torch.from_numpy(est[:, :3, 3]), torch.from_numpy(ref[:, :3, 3])
    cov = ((y - y.mean(0)).T @ (x - x.mean(0))).numpy() / len(x)
    if np.count_nonzero(np.linalg.svd(cov, compute_uv=False) > np.finfo(np.float64).eps) < 2:     # evo's GeometryException
        raise ValueError("eval_metrics: degenerate covariance rank, Umeyama alignment is not possible")
    return tuple(v.numpy() for v in rigid_points_registration(x, y, torch.ones(len(x), dtype=torch.float64), fp64=True))


def _sim3_align(est, ref):
    """evo PosePath3D.align(correct_scale=True): Umeyama sim(3) of the estimated positions onto the reference ones (unit weights), applied
    to the whole estimated poses."""
    s, R, T = _sim3_fit(est, ref)
    out = est.copy()
    out[:, :3, :3] = R @ est[:, :3, :3]
    out[:, :3, 3] = s * est[:, :3, 3] @ R.T + T
    return out


def _matched_poses(pred_traj, gt_traj, sample_stride=1):
    """(reference poses, estimated poses) as [N, 4, 4] fp64, matched by timestamp as eval_metrics matches them."""
    ep, et = np.asarray(pred_traj[0], dtype=np.float64)[::sample_stride], np.asarray(pred_traj[1], dtype=np.float64).reshape(-1)[::sample_stride]
    rp, rt = np.asarray(gt_traj[0], dtype=np.float64)[::sample_stride], np.asarray(gt_traj[1], dtype=np.float64).reshape(-1)[::sample_stride]
    if len(et) == len(rt):
        et = rt
    i_ref, i_est = _associate(rt, et)
    return _tum_to_mats(rp[i_ref]), _tum_to_mats(ep[i_est])


def trajectory_sim3(pred_traj, gt_traj, sample_stride=1):
    """The 4 x 4 fp64 matrix [[s R, T], [0, 1]] of the sim(3) eval_metrics fits between the trajectories (Umeyama, estimated positions
    onto the reference's): what takes the estimate's world into the ground truth's. A degenerate trajectory raises ValueError."""
    ref, est = _matched_poses(pred_traj, gt_traj, sample_stride)
    s, R, T = _sim3_fit(est, ref)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, T
    return M


def eval_metrics(pred_traj, gt_traj, seq="", filename="", sample_stride=1):
    """vo_eval.py eval_metrics (:174-258) -> (ATE, RPE translation, RPE rotation in degrees), fp64 on the host.

    Trajectories are TUM-style ``[poses [N, 7] (x y z qw qx qy qz), timestamps [N]]`` pairs (``io.get_tum_poses``). As the reference:
    estimate timestamps are replaced by the reference's when the lengths agree, then matched to them (evo's associate, 0.01 s);
    ATE = evo ``ape(translation_part, align=True, correct_scale=True)``: Umeyama sim(3) of the estimated onto the reference positions,
    then the RMSE of the position errors; RPE = evo ``rpe(delta=1 frame, all_pairs=True, align=True, correct_scale=True)``: the same
    sim(3), then the RMSE over consecutive pairs of the translation norm and the rotation angle of (Q_i^-1 Q_{i+1})^-1 (P_i^-1 P_{i+1}).
    ``filename`` (when given) receives a short plain-text summary, not evo's printed report. A degenerate trajectory raises ValueError."""
    ref, est = _matched_poses(pred_traj, gt_traj, sample_stride)
    al = _sim3_align(est, ref)
    ate = float(np.sqrt(np.mean(np.sum((al[:, :3, 3] - ref[:, :3, 3]) ** 2, -1))))
    E = relative_pose_errors(al, ref)
    if not E:
        raise ValueError("eval_metrics: RPE needs at least two poses")
    rpe_trans = float(np.sqrt(np.mean([np.sum(e[:3, 3] ** 2) for e in E])))
    rpe_rot = float(np.sqrt(np.mean([rotation_angle_deg(e) ** 2 for e in E])))
    if filename:
        with open(filename, "w+") as f:
            f.write(f"Seq: {seq} \n\n")
            f.write(f"APE w.r.t. translation part (m), sim(3) Umeyama alignment\n    rmse\t{ate}\n    poses\t{len(ref)}\n\n")
            f.write(f"RPE w.r.t. rotation angle in degrees (deg), for delta = 1 (frames) using consecutive pairs, sim(3) Umeyama alignment\n"
                    f"    rmse\t{rpe_rot}\n    pairs\t{len(E)}\n\n")
            f.write(f"RPE w.r.t. translation part (m), for delta = 1 (frames) using consecutive pairs, sim(3) Umeyama alignment\n"
                    f"    rmse\t{rpe_trans}\n    pairs\t{len(E)}\n")
    return ate, rpe_trans, rpe_rot


# ---- the evaluation entry's glue -------------------------------------------------------------------------------------------------
def evaluate_scene(scene, gt_depth, *, dataset, gt_traj=None, seq="", out_dir=None, align_mask=None):
    """What infer_geo4d.py does after post_optimization: the scene's depth maps resized (bicubic) to the ground-truth size [T, OH, OW],
    scored by depth_evaluation with the dataset's arguments (kitti: max_depth=None, defaults; any other dataset: max_depth=70,
    post_clip_max=70, lr=1e-2, 5000 iterations, and ``align_mask`` - the scene's per-pixel validity [T, H, W], resized the same way and
    thresholded at > 0.8 - restricting the fit); with ``gt_traj`` ([poses, timestamps] as eval_metrics takes them) ATE / RPE of the
    scene's camera-to-world poses. With ``out_dir``, appends the reference's ``{out_dir}/{seq}/_error_log_depth.txt`` and
    ``_error_log.txt`` lines and writes ``{out_dir}/{seq}_eval_metric.txt``. Returns {'depth': results, 'error_map': [T, OH, OW],
    'ate', 'rpe_trans', 'rpe_rot'} (the pose entries None without gt_traj; 0 when eval_metrics fails, as the reference's try block)."""
    depth = scene.get_depthmaps()
    depth = torch.stack(list(depth)) if isinstance(depth, (list, tuple)) else depth
    depth = depth.detach().float().contiguous()
    gt = _as_tensor(gt_depth).to(depth.device).float()
    T, OH, OW = gt.shape[-3:]
    if depth.shape[0] != T:
        raise ValueError(f"evaluate_scene: {depth.shape[0]} depth maps for {T} ground-truth frames")
    pred = ops.bicubic_resize(depth, (OH, OW))
    if dataset == "kitti":
        res, err, _, _ = depth_evaluation(pred.reshape(-1), gt.reshape(-1), max_depth=None, align_with_lad2=True, use_gpu=True)
    else:
        am = None
        if align_mask is not None:
            am = ops.bicubic_resize(_as_tensor(align_mask).to(depth.device).reshape(depth.shape).float().contiguous(), (OH, OW)) > 0.8
            am = am.reshape(-1)
        res, err, _, _ = depth_evaluation(pred.reshape(-1), gt.reshape(-1), max_depth=70, align_with_lad2=True, use_gpu=True, post_clip_max=70,
                                          lr=1e-2, max_iters=5000, align_mask=am)
    out = {"depth": res, "error_map": err.reshape(T, OH, OW), "ate": None, "rpe_trans": None, "rpe_rot": None}
    if out_dir is not None:
        os.makedirs(os.path.join(out_dir, seq), exist_ok=True)
        with open(os.path.join(out_dir, seq, "_error_log_depth.txt"), "a") as f:
            f.write(f"{seq}_{res}\n")
    if gt_traj is not None:
        pred_traj = io.get_tum_poses(scene.get_im_poses_matrix())
        try:
            metric_file = os.path.join(out_dir, f"{seq}_eval_metric.txt") if out_dir is not None else ""
            ate, rpe_trans, rpe_rot = eval_metrics(pred_traj, gt_traj, seq=seq, filename=metric_file, sample_stride=1)
        except ValueError as e:                          # infer_geo4d.py:583-591
            print(f"Error: {e}")
            ate, rpe_trans, rpe_rot = 0, 0, 0
        out.update(ate=ate, rpe_trans=rpe_trans, rpe_rot=rpe_rot)
        if out_dir is not None:
            with open(os.path.join(out_dir, seq, "_error_log.txt"), "a") as f:
                f.write(f"{dataset}-{seq: <16} | ATE: {ate:.5f}, RPE trans: {rpe_trans:.5f}, RPE rot: {rpe_rot:.5f}\n")
                f.write(f"{ate:.5f}\n{rpe_trans:.5f}\n{rpe_rot:.5f}\n")
    return out


# ---- the 3D result ------------------------------------------------------------------------------------------------------------------
def _thresholds(thresholds, max_dist):
    """The thresholds as floats (None: (max_dist,)); ValueError unless 0 < t <= max_dist for each."""
    ts = (max_dist,) if thresholds is None else tuple(thresholds)
    try:
        ts = tuple(float(t) for t in ts)
    except (TypeError, ValueError):
        raise ValueError(f"cloud_metrics: thresholds must be numbers, got {thresholds!r}") from None
    if not ts or not all(0 < t <= max_dist for t in ts):
        raise ValueError(f"cloud_metrics: thresholds must be a non-empty sequence with 0 < t <= max_dist = {max_dist:g}, got {thresholds!r}")
    return ts


@torch.no_grad()
def cloud_metrics(pred, gt, *, max_dist, thresholds=None, voxel=None, pred_mask=None, gt_mask=None):
    """Accuracy, completeness, Chamfer distance and precision / recall / F-score of a predicted cloud against a ground-truth cloud, on the
    HIP device (geo4d_amd.nearest; the rule of include/geo4d_hip.h). The clouds must already be in one frame: the figures are only as
    meaningful as the alignment handed in.

    pred [Np, 3], gt [Ng, 3], the masks [N] bool (None: all). A point takes part when its mask is set and its coordinates are finite
    (`n_pred`, `n_gt`). One nearest-neighbour query runs in each direction with the radius `max_dist`. Per point, d = sqrt(dist2) in
    fp32 when a neighbour was found within `max_dist`, else `max_dist`: the truncated distance. `accuracy` is the float64 mean of d
    over the predicted points (pred -> gt), `completeness` over the ground truth's (gt -> pred), `chamfer` their half-sum. Per threshold
    t of `thresholds` (None: (max_dist,); 0 < t <= max_dist): `within_pred[k]` / `within_gt[k]` count the points with a neighbour at
    dist2 <= t * t (fp32), `precision[k]` = within_pred / n_pred, `recall[k]` = within_gt / n_gt, `fscore[k]` = 2 P R / (P + R), 0 when
    P + R = 0. `unmatched_pred` / `unmatched_gt` count the points without a neighbour within `max_dist`. `pred_dist` / `gt_dist` fp32
    per input row hold d (NaN where the row took no part), for colouring a cloud by its error. `voxel`: both clouds are first reduced
    with fuse_points(reduce="mean") at that voxel (evaluating downsampled clouds is standard practice, and it keeps the cells small:
    the time grows with the points per cell); the per-row outputs then belong to the reduced clouds, returned as `pred_points` /
    `gt_points`. The thresholds' default is untried on real predictions. Either side without a taking-part point raises ValueError,
    and so do points outside the cell grid (|x| >= 2^20 max_dist)."""
    who = "cloud_metrics"
    r = check_radius(max_dist, who, "max_dist")
    ts = _thresholds(thresholds, r)
    check_cloud(pred, pred_mask, who, "pred"), check_cloud(gt, gt_mask, who, "gt")
    pred, pred_mask = _cloud(pred, pred_mask, who, "pred")
    gt, gt_mask = _cloud(gt, gt_mask, who, "gt")
    if voxel is not None:
        pred, pred_mask = fuse_points(pred, mask=pred_mask, voxel=voxel)["points"], None
        gt, gt_mask = fuse_points(gt, mask=gt_mask, voxel=voxel)["points"], None
    sides = {}
    for name, q, qm, ref, rm in (("pred", pred, pred_mask, gt, gt_mask), ("gt", gt, gt_mask, pred, pred_mask)):
        took = torch.isfinite(q).all(1) if qm is None else torch.isfinite(q).all(1) & qm.to(torch.bool)
        nn = nearest_points(q, ref, radius=r, query_mask=qm, reference_mask=rm)
        matched = nn["index"] >= 0
        # sqrt in fp64 rounded to fp32 is the correctly rounded fp32 square root whatever the device's fp32 sqrt does
        d = torch.where(matched, nn["dist2"].double().sqrt().float(), torch.full_like(nn["dist2"], r))
        t2 = [(torch.tensor(t, dtype=torch.float32) * torch.tensor(t, dtype=torch.float32)).item() for t in ts]
        within = [(matched & (nn["dist2"] <= x)).sum() for x in t2]
        sides[name] = (took, matched, d, within)
    host = torch.stack([x.double() for name in ("pred", "gt") for x in
                        (sides[name][0].sum(), (sides[name][0] & ~sides[name][1]).sum(),
                         torch.where(sides[name][0], sides[name][2], torch.zeros_like(sides[name][2])).double().sum(), *sides[name][3])]).tolist()
    K = len(ts)
    (n_pred, un_pred, sum_pred, *w_pred), (n_gt, un_gt, sum_gt, *w_gt) = host[:3 + K], host[3 + K:]
    n_pred, n_gt = int(n_pred), int(n_gt)
    if n_pred == 0 or n_gt == 0:
        raise ValueError(f"cloud_metrics: no point takes part on the {'predicted' if n_pred == 0 else 'ground-truth'} side (mask set and "
                         "finite coordinates)")
    acc, comp = sum_pred / n_pred, sum_gt / n_gt
    P, R = [int(w) / n_pred for w in w_pred], [int(w) / n_gt for w in w_gt]
    out = dict(max_dist=r, thresholds=list(ts), n_pred=n_pred, n_gt=n_gt, accuracy=acc, completeness=comp, chamfer=0.5 * (acc + comp),
               within_pred=[int(w) for w in w_pred], within_gt=[int(w) for w in w_gt], precision=P, recall=R,
               fscore=[2 * p * q / (p + q) if p + q > 0 else 0.0 for p, q in zip(P, R)], unmatched_pred=int(un_pred), unmatched_gt=int(un_gt))
    nan = float("nan")
    out["pred_dist"] = torch.where(sides["pred"][0], sides["pred"][2], torch.full_like(sides["pred"][2], nan))
    out["gt_dist"] = torch.where(sides["gt"][0], sides["gt"][2], torch.full_like(sides["gt"][2], nan))
    if voxel is not None:
        out["pred_points"], out["gt_points"] = pred, gt
    return out


@torch.no_grad()
def scene_cloud_metrics(scene, gt_points, *, max_dist, thresholds=None, transform=None, gt_traj=None, voxel=None, motion=None, min_conf_thr=3,
                        thr_for_init_conf=True, is_msk=True, out_dir=None, seq=""):
    """cloud_metrics of an aligned GroupAligner's points against a ground-truth cloud gt_points [Ng, 3].

    The scene's points and mask are taken as fuse_scene takes them, through scene_view (`min_conf_thr` / `thr_for_init_conf` /
    `is_msk`, restricted by `motion`). They are moved by `transform` (4 x 4, [[s R, T], [0, 1]]: scale folded in) when given; else,
    with `gt_traj` ([poses, timestamps] as eval_metrics takes them), by the sim(3) eval_metrics fits between the scene's trajectory and
    that one (trajectory_sim3); with neither they are not moved. The move is pts @ (s R).T + T in fp32 with torch on the device.
    With `out_dir`, writes {out_dir}/{seq}_cloud_metric.txt. Returns cloud_metrics' dict plus `transform` (the 4 x 4 fp64 array used,
    or None)."""
    if motion not in MOTION:
        raise ValueError(f"scene_cloud_metrics: motion must be one of {MOTION}, got {motion!r}")
    if transform is not None and gt_traj is not None:
        raise ValueError("scene_cloud_metrics: give `transform` or `gt_traj`, not both")
    if transform is not None:
        transform = np.asarray(torch.as_tensor(transform).detach().cpu().numpy(), dtype=np.float64)
        if transform.shape != (4, 4) or not np.isfinite(transform).all():
            raise ValueError(f"scene_cloud_metrics: transform must be a finite 4 x 4 matrix, got shape {transform.shape}")
    view = scene_view(scene, "scene_cloud_metrics", min_conf_thr=min_conf_thr, thr_for_init_conf=thr_for_init_conf, is_msk=is_msk,
                      motion=motion, segment=segment_motion)
    msk = view.mask()
    if transform is None and gt_traj is not None:
        transform = trajectory_sim3(io.get_tum_poses(view.poses), gt_traj)
    pts = view.pts3d.reshape(-1, 3).float()
    if transform is not None:
        M = torch.from_numpy(transform).to(view.dev).float()
        pts = pts @ M[:3, :3].T + M[:3, 3]
    gt = _as_tensor(gt_points)
    out = cloud_metrics(pts, gt.to(view.dev) if torch.is_tensor(gt) and gt.dim() == 2 else gt, max_dist=max_dist, thresholds=thresholds,
                        voxel=voxel, pred_mask=None if msk is None else msk.reshape(-1))
    out["transform"] = transform
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"{seq}_cloud_metric.txt"), "w") as f:
            f.write(f"Seq: {seq} \n\n")
            f.write(f"Cloud metrics, truncated at max_dist = {out['max_dist']:g}; {out['n_pred']} predicted and {out['n_gt']} ground-truth points\n")
            f.write(f"    accuracy\t{out['accuracy']}\n    completeness\t{out['completeness']}\n    chamfer\t{out['chamfer']}\n")
            f.write(f"    unmatched\t{out['unmatched_pred']} predicted, {out['unmatched_gt']} ground truth\n")
            for k, t in enumerate(out["thresholds"]):
                f.write(f"    at {t:g}:\tprecision {out['precision'][k]}\trecall {out['recall'][k]}\tfscore {out['fscore'][k]}\n")
    return out
