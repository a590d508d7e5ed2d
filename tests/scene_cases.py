"""The GroupAligners the scene GPU tests share (export, motion, fusion, TSDF, renderer, mesh clean-up): the tiny aligned scene of
tests/golden/align_tiny.pt and an aligner whose parameters are the truth of a tests/motion_restatement.py synthetic scene."""
import math
import os

import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tiny_aligner_and_fixture(dev):
    """(the tiny aligned scene at its fixture's initial parameters, the fixture)."""
    from geo4d_amd.align import GroupAligner
    a_fix = torch.load(os.path.join(G, "align_tiny.pt"), weights_only=False)
    a = GroupAligner(a_fix["groups"], a_fix["pred"].to(dev), a_fix["conf"].squeeze(-1).to(dev), shared_focal=True,
                     temporal_smoothing_weight=a_fix["kw"]["temporal_smoothing_weight"], translation_weight=a_fix["kw"]["translation_weight"])
    for k, v in a_fix["init"].items():
        a.P[k] = v.clone().to(dev)
    return a, a_fix


def tiny_aligner(dev):
    """The tiny aligned scene alone."""
    return tiny_aligner_and_fixture(dev)[0]


def truth_aligner(dev, s):
    """A GroupAligner whose parameters are the synthetic scene's truth: its depth maps, cameras and focal."""
    from geo4d_amd.align import FOCAL_BREAK, GroupAligner, rotmat_to_quat, signed_log1p
    n, H, W = s["n"], s["H"], s["W"]
    a = GroupAligner([list(range(n))], torch.zeros((1, n, H, W, 3), device=dev), torch.full((1, n, H, W), 5.0, device=dev))
    a.P["im_depthmaps"].copy_(torch.from_numpy(s["depth"]).to(dev).reshape(n, -1).log())
    c2w = torch.from_numpy(s["cams2world"])
    for k in range(n):
        a.P["im_poses"][k, :4] = rotmat_to_quat(c2w[k, :3, :3]).float().to(dev)
        a.P["im_poses"][k, 4:7] = signed_log1p(c2w[k, :3, 3].float()).to(dev)
    a.P["im_focals"][:] = FOCAL_BREAK * math.log(float(s["K"][0, 0, 0]))
    return a
