"""Scene export on the HIP path (geo4d_amd/scene_export.py + csrc/scene_export.hip): the scene state of GroupAligner, clean_pointcloud
against the REFERENCE's own results (tests/golden/scene_export.pt, tests/golden/generate_scene.py), the point / face compactions
against boolean indexing and the reference's faces, the glb files and save_scene's results folder."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from scene_cases import tiny_aligner_and_fixture as _aligner

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fix():
    return torch.load(os.path.join(G, "scene_export.pt"), weights_only=False)


def _glb(path):
    data = open(path, "rb").read()
    magic, ver, total = struct.unpack("<4sII", data[:12])
    assert magic == b"glTF" and ver == 2 and total == len(data)
    jlen, jtype = struct.unpack("<I4s", data[12:20])
    assert jtype == b"JSON"
    doc = json.loads(data[20:20 + jlen])
    blen, btype = struct.unpack("<I4s", data[20 + jlen:28 + jlen])
    assert btype == b"BIN\x00"
    return doc, data[28 + jlen:28 + jlen + blen]


def test_im_conf_is_the_max_over_window_slots(dev):
    a, a_fix = _aligner(dev)
    conf = a_fix["conf"].squeeze(-1)
    ref = torch.zeros((a.n,) + tuple(conf.shape[-2:]))
    for g, grp in enumerate(a_fix["groups"]):
        for k, img in enumerate(grp):
            ref[img] = torch.maximum(ref[img], conf[g, k])
    assert torch.equal(a.im_conf.cpu(), ref) and torch.equal(a.init_conf_maps.cpu(), ref)
    assert a.im_conf.data_ptr() != a.init_conf_maps.data_ptr()
    assert torch.equal(a.get_conf().cpu(), ref) and torch.equal(a.get_conf("log"), a.im_conf.log())
    # get_masks follows thr_for_init_conf both ways: after lowering im_conf only the im_conf masks change
    a.min_conf_thr = float(ref.median())
    a.im_conf[:, :, : a.W // 2] = 0
    a.thr_for_init_conf = True
    assert torch.equal(a.get_masks().cpu(), ref > a.min_conf_thr)
    a.thr_for_init_conf = False
    low = ref.clone()
    low[:, :, : a.W // 2] = 0
    assert torch.equal(a.get_masks().cpu(), low > a.min_conf_thr)
    K = a.get_intrinsics().cpu()
    f = a.get_focals().detach().cpu().flatten()
    assert torch.equal(K[:, 0, 0], f) and torch.equal(K[:, 1, 1], f) and torch.equal(K[:, 2, 2], torch.ones(a.n))
    assert torch.equal(K[:, 0, 2], torch.full((a.n,), a.W / 2)) and torch.equal(K[:, 1, 2], torch.full((a.n,), a.H / 2))


def _near_boundary(s, i, p, tol):
    """True when pixel p of image i sits, for some j, within 1e-3 px of a rounding boundary or 1e-5 relative of the depth test (fp64)."""
    n, H, W = s["conf"].shape
    x = s["pts3d"][i].reshape(-1, 3)[p].double()
    for j in range(n):
        if j == i:
            continue
        c = s["cams"][j].double()
        q = c[:3, :3] @ x + c[:3, 3]
        k = s["K"][j].double() @ q
        uv = k[:2] / k[2]
        if ((uv - uv.floor() - 0.5).abs() < 1e-3).any():
            return True
        u, v = torch.round(uv).long().tolist()
        if q[2] > 0 and 0 <= u < W and 0 <= v < H:
            d = (1 - tol) * float(s["depth"][j, v, u])
            if abs(float(q[2]) - d) <= 1e-5 * abs(d):
                return True
    return False


@pytest.mark.parametrize("key", [(0.001, 0.0), (0.05, 0.0), (0.01, 0.5)])
def test_clean_pointcloud_matches_reference(dev, fix, key):
    from geo4d_amd import scene_export
    s = fix["occl"]
    ref = s["cleaned"][key]
    got = scene_export.clean_pointcloud(s["conf"].to(dev), s["K"].to(dev), s["cams"].to(dev), s["depth"].to(dev), s["pts3d"].to(dev),
                                        tol=key[0], bad_conf=key[1]).cpu()
    diff = (got != ref).reshape(len(ref), -1).nonzero().tolist()
    print(f"[clean {key}] {int((ref != s['conf']).sum())} cleaned, {len(diff)} differ")
    assert int((got != s["conf"]).sum()) > 500
    assert len(diff) <= max(2, 1e-4 * ref.numel())
    for i, p in diff:
        assert _near_boundary(s, i, p, key[0]), (i, p)


def test_clean_pointcloud_keeps_the_reference_loop_order(dev, fix):
    from geo4d_amd import scene_export
    s = fix["order"]
    assert not torch.equal(s["cleaned"], s["one_pass"])          # the case tells the sequential answer from the one-pass one
    got = scene_export.clean_pointcloud(s["conf"].to(dev), s["K"].to(dev), s["cams"].to(dev), s["depth"].to(dev), s["pts3d"].to(dev)).cpu()
    assert torch.equal(got, s["cleaned"])


def test_clean_pointcloud_exact_scene_bit_exact(dev):
    """Dyadic depths / translations / focal: every product and sum is exact, so the HIP result equals the torch loop bit for bit."""
    from geo4d_amd import scene_export
    from tools.scene_export_bench import torch_clean
    g = torch.Generator().manual_seed(3)
    n, H, W, f = 12, 20, 28, 16.0
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grid = torch.stack([xs - W // 2, ys - H // 2], -1).float()
    depth = torch.tensor([2.0, 3.0, 4.0, 6.0, 8.0])[torch.randint(0, 5, (n, H, W), generator=g)]
    t = torch.randint(-8, 9, (n, 3), generator=g).float() / 8
    pts = torch.cat([depth[..., None] * grid / f, depth[..., None]], -1) + t[:, None, None]
    cams = torch.eye(4).repeat(n, 1, 1)
    cams[:, :3, 3] = -t
    K = torch.zeros(n, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W // 2, H // 2, 1
    conf = torch.randint(1, 17, (n, H, W), generator=g).float() / 2
    ref = torch_clean(conf, K, cams, depth, pts, tol=0.001, bad_conf=0.25)
    got = scene_export.clean_pointcloud(conf.to(dev), K.to(dev), cams.to(dev), depth.to(dev), pts.to(dev), tol=0.001, bad_conf=0.25).cpu()
    assert int((ref != conf).sum()) > 100
    assert torch.equal(got, ref)


def test_group_aligner_clean_pointcloud(dev):
    """The method: torch.linalg.inv of the poses, get_intrinsics / get_depthmaps / get_pts3d, im_conf rewritten in place, init maps kept."""
    from geo4d_amd import scene_export
    a, _ = _aligner(dev)
    init = a.im_conf.clone()
    ptr = a.im_conf.data_ptr()
    want = scene_export.clean_pointcloud(init, a.get_intrinsics(), torch.linalg.inv(a.get_im_poses_matrix()), a.get_depthmaps(),
                                         a.get_pts3d(), tol=0.01)
    assert a.clean_pointcloud(tol=0.01) is a
    assert a.im_conf.data_ptr() == ptr and torch.equal(a.im_conf, want) and torch.equal(a.init_conf_maps, init)
    with pytest.raises(ValueError):
        a.clean_pointcloud(tol=1.0)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 17, 23), (4, 64, 80)])
def test_scene_points_is_boolean_indexing(dev, shape):
    from geo4d_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    pts = torch.randn(shape + (3,), generator=g)
    rgb = torch.rand(shape + (3,), generator=g) * 1.2 - 0.1
    mask = torch.rand(shape, generator=g) < 0.6
    for m in (mask, None):
        p, c, cnt = ops.scene_points(pts.to(dev), rgb.to(dev), None if m is None else m.to(dev))
        k = int(cnt.item())
        sel = torch.ones(shape, dtype=torch.bool) if m is None else m
        assert k == int(sel.sum()) and torch.equal(p[:k].cpu(), pts[sel])
        q = np.clip(rgb[sel].numpy() * 255.0 + 0.5, 0, 255).astype(np.uint8)
        assert np.array_equal(c[:k, :3].cpu().numpy(), q) and bool((c[:k, 3] == 255).all())


@pytest.mark.parametrize("name", ["random", "structured"])
def test_mesh_faces_match_reference(dev, fix, name):
    from geo4d_amd import ops
    n, H, W = fix["faces"]["shape"]
    case = fix["faces"]["cases"][name]
    faces, cnt = ops.scene_mesh_faces(case["mask"].to(dev), n, H, W, dev)
    k = int(cnt.item())
    assert k == len(case["faces"]) and torch.equal(faces[:k].cpu().long(), case["faces"])
    faces, cnt = ops.scene_mesh_faces(None, n, H, W, dev)
    assert int(cnt.item()) == 4 * n * (H - 1) * (W - 1)


def test_pointcloud_glb_is_save_glb(dev, tmp_path):
    from geo4d_amd import io, scene_export
    a, _ = _aligner(dev)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(2)).to(dev)
    thr = float(a.im_conf.median())
    path = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, min_conf_thr=thr, as_pointcloud=True, save_name="pc")
    assert path == os.path.join(str(tmp_path), "pc.glb")
    ref = io.save_glb(str(tmp_path / "ref.glb"), a.imgs, a.get_pts3d(), a.init_conf_maps > thr, a.get_focals().detach(),
                      a.get_im_poses_matrix().detach(), cam_color=scene_export.camera_colors(a.n))
    assert open(path, "rb").read() == open(ref, "rb").read()
    doc, _ = _glb(path)
    assert doc["accessors"][0]["count"] == int((a.init_conf_maps > thr).sum())
    # clean_depth with thr_for_init_conf=False: the masks see the cleaned confidences
    p2 = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, min_conf_thr=thr, as_pointcloud=True, clean_depth=True,
                                              thr_for_init_conf=False, save_name="pc2")
    assert _glb(p2)[0]["accessors"][0]["count"] == int((a.im_conf > thr).sum()) <= int((a.init_conf_maps > thr).sum())


def test_mesh_glb(dev, tmp_path):
    from geo4d_amd import ops, scene_export
    a, _ = _aligner(dev)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    thr = float(a.im_conf.median())
    path = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, min_conf_thr=thr, as_pointcloud=False, transparent_cams=True)
    doc, binary = _glb(path)
    prim = doc["meshes"][0]["primitives"][0]
    assert prim["mode"] == 4
    faces, cnt = ops.scene_mesh_faces(a.init_conf_maps > thr, a.n, a.H, a.W, dev)
    k = int(cnt.item())
    acc = doc["accessors"][prim["indices"]]
    assert acc["componentType"] == 5125 and acc["count"] == 3 * k > 0
    view = doc["bufferViews"][acc["bufferView"]]
    idx = np.frombuffer(binary, np.uint32, count=acc["count"], offset=view["byteOffset"])
    assert np.array_equal(idx, faces[:k].cpu().numpy().reshape(-1).astype(np.uint32))
    assert doc["accessors"][prim["attributes"]["POSITION"]]["count"] == a.n * a.H * a.W
    assert len(doc["meshes"]) == 1 + a.n                                          # + one camera glyph per image


def test_save_scene_writes_the_results_folder(dev, tmp_path):
    from geo4d_amd import io, scene_export
    a, _ = _aligner(dev)
    video = torch.rand((1, 3, a.n, a.H, a.W), generator=torch.Generator().manual_seed(6)) * 2 - 1
    with pytest.raises(ValueError):                                              # no RGB frames yet
        scene_export.save_scene(a, str(tmp_path), "seq")
    d = scene_export.save_scene(a, str(tmp_path), "seq", imgs=video)
    assert d == os.path.join(str(tmp_path), "seq")
    assert torch.equal(a.imgs.cpu(), (video[0].permute(1, 2, 3, 0) * 0.5 + 0.5).clip(0, 1))
    names = set(os.listdir(d))
    for want in ["seq.glb", "pred_traj.txt", "pred_focal.txt", "pred_intrinsics.txt", "colored_depth_maps.gif"]:
        assert want in names, want
    for i in range(a.n):
        for want in (f"frame_{i:04d}.npy", f"frame_colordepth_{i:04d}.png", f"conf_{i}.npy", f"init_conf_{i}.npy", f"frame_{i:04d}.png"):
            assert want in names, want
        assert np.load(os.path.join(d, f"frame_{i:04d}.npy")).shape == (a.H, a.W)
        assert np.load(os.path.join(d, f"conf_{i}.npy")).shape == (a.H, a.W)
    poses, stamps = io.load_tum_traj(os.path.join(d, "pred_traj.txt"))
    assert poses.shape == (a.n, 7) and np.array_equal(stamps, np.arange(a.n))
    np.testing.assert_allclose(poses[:, :3], a.get_im_poses_matrix()[:, :3, 3].cpu().numpy(), atol=1e-6)
    assert np.loadtxt(os.path.join(d, "pred_intrinsics.txt")).shape == (a.n, 9)
    assert np.loadtxt(os.path.join(d, "pred_focal.txt")).shape == (a.n,)
    doc, _ = _glb(os.path.join(d, "seq.glb"))
    assert doc["accessors"][0]["count"] == a.n * a.H * a.W                         # is_msk=False keeps every pixel
