"""The `dust3r/inference.py` call surface (reference: dust3r/inference.py:27-179,
dust3r/utils/device.py:10-75) on the host, with a stub pairwise model: batching, collation, the batch-size-1 fallback for images of
different sizes, symmetrised batches. No GPU, no reference import (the behaviours are stated here as plain expectations)."""
import numpy as np
import torch

from geo4d_amd import dust3r_inference as di


def _view(i, h=4, w=6):
    g = torch.Generator().manual_seed(i)
    return {"img": torch.randn((1, 3, h, w), generator=g), "true_shape": np.int32([[h, w]]), "idx": i, "instance": str(i)}


class StubModel:
    """pred1['pts3d'] = mean colour of view1 per pixel; pred2['pts3d_in_other_view'] = view2 - view1 means: enough to see which inputs
    reached the model, in which order, and how many calls were made."""
    def __init__(self):
        self.batch_sizes = []

    def __call__(self, v1, v2):
        self.batch_sizes.append(v1["img"].shape[0])
        a, b = v1["img"].mean(1, keepdim=True).permute(0, 2, 3, 1), v2["img"].mean(1, keepdim=True).permute(0, 2, 3, 1)
        return {"pts3d": a.expand(-1, -1, -1, 3), "conf": torch.ones_like(a[..., 0])}, {"pts3d_in_other_view": (b - a).expand(-1, -1, -1, 3)}


def test_inference_batches_and_collates():
    pairs = [(_view(2 * k), _view(2 * k + 1)) for k in range(5)]
    m = StubModel()
    out = di.inference(pairs, m, "cpu", batch_size=2, verbose=False)
    assert m.batch_sizes == [2, 2, 1]
    assert set(out) == {"view1", "view2", "pred1", "pred2", "loss"} and out["loss"] is None
    assert out["view1"]["img"].shape == (5, 3, 4, 6) and out["pred1"]["pts3d"].shape == (5, 4, 6, 3)
    for k in range(5):
        assert torch.equal(out["view1"]["img"][k], pairs[k][0]["img"][0]) and torch.equal(out["view2"]["img"][k], pairs[k][1]["img"][0])
        want = pairs[k][1]["img"][0].mean(0) - pairs[k][0]["img"][0].mean(0)
        assert torch.allclose(out["pred2"]["pts3d_in_other_view"][k, ..., 0], want, atol=1e-6)
    assert out["view1"]["idx"] == [0, 2, 4, 6, 8] and out["view2"]["instance"] == ["1", "3", "5", "7", "9"]       # scalars chain as lists
    assert torch.is_tensor(out["view1"]["true_shape"]) and out["view1"]["true_shape"].shape == (5, 2)           # numpy -> concatenated tensor
    assert di.get_pred_pts3d(out["view1"], out["pred1"]) is out["pred1"]["pts3d"]
    assert di.get_pred_pts3d(out["view2"], out["pred2"], use_pose=True) is out["pred2"]["pts3d_in_other_view"]


def test_inference_mixed_sizes_forces_batch_one_and_lists():
    pairs = [(_view(0), _view(1)), (_view(2, 5, 7), _view(3, 5, 7))]
    assert not di.check_if_same_size(pairs) and di.check_if_same_size(pairs[:1])
    m = StubModel()
    out = di.inference(pairs, m, "cpu", batch_size=8, verbose=False)
    assert m.batch_sizes == [1, 1]
    assert isinstance(out["view1"]["img"], list) and [tuple(t.shape) for t in out["view1"]["img"]] == [(3, 4, 6), (3, 5, 7)]
    assert [tuple(t.shape) for t in out["pred1"]["pts3d"]] == [(4, 6, 3), (5, 7, 3)]


def test_collate_and_to_cpu_edge_cases():
    assert di.collate_with_cat([]) == [] and di.collate_with_cat([None, None]) is None
    assert di.collate_with_cat([1, 2]) == [1, 2] and di.collate_with_cat([[1], [2, 3]]) == [1, 2, 3]
    t = di.collate_with_cat([(torch.zeros(1, 2), {"a": torch.ones(1)}), (torch.ones(2, 2), {"a": torch.zeros(3)})])
    assert isinstance(t, list) and t[0].shape == (3, 2) and t[1]["a"].shape == (4,)
    moved = di.to_cpu({"a": (torch.ones(2), np.zeros(3)), "b": [None, "s", 3]})
    assert isinstance(moved["a"], tuple) and torch.is_tensor(moved["a"][1]) and moved["b"] == [None, "s", 3]


def test_symmetrized_batch_and_loss_hook():
    v1, v2 = di.collate_with_cat([(_view(0), _view(1)), (_view(2), _view(3))])
    s1, s2 = di.make_batch_symmetric((v1, v2))
    assert s1["img"].shape[0] == 4 and torch.equal(s1["img"][0], v1["img"][0]) and torch.equal(s1["img"][1], v2["img"][0])
    assert torch.equal(s2["img"][0], v2["img"][0]) and s1["idx"] == [0, 1, 2, 3] and s2["idx"] == [1, 0, 3, 2]
    res = di.loss_of_one_batch((v1, v2), StubModel(), lambda a, b, p1, p2: p1["pts3d"].sum() * 0 + 7.0, "cpu", symmetrize_batch=True)
    assert float(res["loss"]) == 7.0 and res["pred1"]["pts3d"].shape[0] == 4
    assert di.loss_of_one_batch((v1, v2), StubModel(), None, "cpu", ret="pred2")["pts3d_in_other_view"].shape[0] == 2


def _reference_pts3d_cases():
    """The reference's own get_pred_pts3d (dust3r/inference.py:110-132) on the six cases of the test below: inputs and outputs stored by
    `python tests/golden/generate.py dust3r_pts3d`."""
    import os
    return torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dust3r_pts3d.pt"), weights_only=False)


def test_get_pred_pts3d_all_branches_match_the_reference():
    """`use_pose` goes through camera_pose (it used to return the untransformed points) and the
    depth + pseudo_focal branch exists. Expectations are closed-form, and the reference's own get_pred_pts3d (dust3r/inference.py:110-132)
    on the same inputs is checked beside them (tests/golden/dust3r_pts3d.pt)."""
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 5, 7
    pts = torch.randn((B, H, W, 3), generator=g)
    ang = torch.tensor([0.3, -1.1])
    pose = torch.eye(4).repeat(B, 1, 1)
    pose[:, 0, 0], pose[:, 0, 2], pose[:, 2, 0], pose[:, 2, 2] = ang.cos(), ang.sin(), -ang.sin(), ang.cos()
    pose[:, :3, 3] = torch.randn((B, 3), generator=g)
    depth = torch.rand((B, H, W), generator=g) + 0.5
    focal2 = torch.rand((B, 2, H, W), generator=g) * 50 + 100
    K = torch.eye(3).repeat(B, 1, 1)
    K[:, 0, 2], K[:, 1, 2] = torch.tensor([3.2, 2.9]), torch.tensor([2.1, 1.7])
    cases = [({}, {"pts3d": pts}, False), ({}, {"pts3d": pts, "camera_pose": pose}, True),
             ({}, {"depth": depth, "pseudo_focal": focal2[:, 0]}, False),
             ({"camera_intrinsics": K}, {"depth": depth, "pseudo_focal": focal2, "camera_pose": pose}, True),
             ({"camera_intrinsics": K}, {"depth": depth, "pseudo_focal": focal2[:, :1]}, False),
             ({}, {"pts3d_in_other_view": pts, "camera_pose": pose}, True)]
    ref = _reference_pts3d_cases()
    assert len(ref) == len(cases)
    for (gt, pred, use_pose), rc in zip(cases, ref):
        assert rc["use_pose"] == use_pose and rc["gt"].keys() == gt.keys() and rc["pred"].keys() == pred.keys()
        assert all(torch.equal(rc["gt"][k], gt[k]) for k in gt) and all(torch.equal(rc["pred"][k], pred[k]) for k in pred)   # same inputs
        got = di.get_pred_pts3d(gt, pred, use_pose=use_pose)
        if "pts3d_in_other_view" in pred:
            want = pts
        else:
            if "depth" in pred:
                f = pred["pseudo_focal"]
                fx = f if f.ndim == 3 else f[:, 0]
                fy = f if f.ndim == 3 else (f[:, 1] if f.shape[1] == 2 else f[:, 0])
                cx = gt["camera_intrinsics"][:, 0, 2].view(B, 1, 1) if gt else torch.full((B, 1, 1), (W - 1) / 2)
                cy = gt["camera_intrinsics"][:, 1, 2].view(B, 1, 1) if gt else torch.full((B, 1, 1), (H - 1) / 2)
                u, v = torch.arange(W).view(1, 1, W) - cx, torch.arange(H).view(1, H, 1) - cy
                want = torch.stack([depth * u / fx, depth * v / fy, depth], -1)
            else:
                want = pts
            if use_pose:
                want = torch.einsum("bij,bhwj->bhwi", pose[:, :3, :3], want) + pose[:, None, None, :3, 3]
        assert torch.allclose(got, want, atol=1e-5), (list(pred), use_pose)
        assert torch.allclose(got, rc["out"], atol=1e-6), (list(pred), use_pose)
    import pytest
    with pytest.raises(AssertionError):
        di.get_pred_pts3d({}, {"pts3d": pts}, use_pose=True)           # camera_pose missing: the reference asserts
    with pytest.raises(AssertionError):
        di.get_pred_pts3d({}, {"pts3d_in_other_view": pts}, use_pose=False)
