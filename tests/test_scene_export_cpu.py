"""Scene export without a GPU (geo4d_amd/scene_export.py, geo4d_amd/io.py): the glb container of the indexed mesh primitive, the new C ABI
entry points in the header and the ctypes table, and the argument errors raised before any device work."""
import json
import os
import re
import struct

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("geo4d_scene_clean", "geo4d_scene_points_workspace", "geo4d_scene_points", "geo4d_scene_mesh_faces_workspace",
       "geo4d_scene_mesh_faces")


def _chunks(data):
    magic, ver, total = struct.unpack("<4sII", data[:12])
    assert magic == b"glTF" and ver == 2 and total == len(data)
    jlen, jtype = struct.unpack("<I4s", data[12:20])
    blen, btype = struct.unpack("<I4s", data[20 + jlen:28 + jlen])
    assert jtype == b"JSON" and btype == b"BIN\x00" and jlen % 4 == 0 and blen % 4 == 0 and 28 + jlen + blen == total
    return json.loads(data[20:20 + jlen]), data[28 + jlen:]


def test_mesh_primitive_layout(tmp_path):
    from geo4d_amd import io
    n, H, W = 2, 3, 4
    pos = np.arange(n * H * W * 3, dtype=np.float32).reshape(-1, 3) / 7
    col = (np.arange(n * H * W * 4) % 251).astype(np.uint8).reshape(-1, 4)
    faces = np.array([[0, 1, 4], [4, 1, 0], [13, 14, 17]], np.int32)
    c2w = np.tile(np.eye(4), (n, 1, 1))
    c2w[1, :3, 3] = [0.5, 0, 0]
    path = io.write_scene_glb(str(tmp_path / "m.glb"), [io.mesh_geometry(pos, col, faces)], np.full(n, 10.0), c2w, (W, H), show_cam=False)
    doc, binary = _chunks(open(path, "rb").read())
    assert len(doc["meshes"]) == 1 and len(doc["nodes"]) == 1
    prim = doc["meshes"][0]["primitives"][0]
    assert prim["mode"] == 4 and set(prim) == {"attributes", "mode", "indices"}
    acc = doc["accessors"]
    p, c, ix = acc[prim["attributes"]["POSITION"]], acc[prim["attributes"]["COLOR_0"]], acc[prim["indices"]]
    assert (p["componentType"], p["type"], p["count"]) == (5126, "VEC3", n * H * W)
    assert p["min"] == [float(v) for v in pos.min(0)] and p["max"] == [float(v) for v in pos.max(0)]
    assert (c["componentType"], c["type"], c["count"], c["normalized"]) == (5121, "VEC4", n * H * W, True)
    assert (ix["componentType"], ix["type"], ix["count"]) == (5125, "SCALAR", 9)
    views = doc["bufferViews"]
    assert views[ix["bufferView"]]["target"] == 34963 and views[p["bufferView"]]["target"] == 34962
    read = lambda a, dt, k: np.frombuffer(binary, dt, count=a["count"] * k, offset=views[a["bufferView"]]["byteOffset"])
    assert np.array_equal(read(p, np.float32, 3).reshape(-1, 3), pos)
    assert np.array_equal(read(c, np.uint8, 4).reshape(-1, 4), col)
    assert np.array_equal(read(ix, np.uint32, 1), faces.reshape(-1).astype(np.uint32))
    for v in views:
        assert v["byteOffset"] % 4 == 0


def test_point_glb_unchanged_by_the_writer_split(tmp_path):
    """save_glb = host compaction + write_scene_glb: the POINTS primitive carries no indices and the file is what the split writer makes."""
    from geo4d_amd import io
    g = torch.Generator().manual_seed(0)
    n, H, W = 2, 4, 5
    imgs, pts = torch.rand((n, H, W, 3), generator=g), torch.randn((n, H, W, 3), generator=g)
    masks = torch.rand((n, H, W), generator=g) < 0.5
    c2w = torch.eye(4).repeat(n, 1, 1)
    a = open(io.save_glb(str(tmp_path / "a.glb"), imgs, pts, masks, torch.full((n,), 9.0), c2w), "rb").read()
    col = np.clip(imgs[masks].numpy() * 255.0 + 0.5, 0, 255).astype(np.uint8)
    col = np.concatenate([col, np.full((len(col), 1), 255, np.uint8)], 1)
    b = open(io.write_scene_glb(str(tmp_path / "b.glb"), [dict(mode=0, positions=pts[masks].numpy(), colors=col)], np.full(n, 9.0),
                                c2w.numpy(), (W, H)), "rb").read()
    assert a == b
    doc, _ = _chunks(a)
    assert "indices" not in doc["meshes"][0]["primitives"][0] and len(doc["meshes"]) == 1 + n


def test_new_symbols_in_header_and_ctypes_table():
    from geo4d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geo4d_hip.h")).read()
    declared = set(re.findall(r"\b(geo4d_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
    assert int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 9


def test_argument_errors_before_device_work():
    from geo4d_amd import _lib, scene_export
    assert scene_export.get_3D_model_from_scene("/nonexistent", True, None) is None
    with pytest.raises(NotImplementedError):
        scene_export.get_3D_model_from_scene("/nonexistent", True, object(), mask_sky=True)
    z = torch.zeros(2, 3, 4)
    args = (z, torch.eye(3).repeat(2, 1, 1), torch.eye(4).repeat(2, 1, 1), z, torch.zeros(2, 3, 4, 3))
    for tol in (1.0, -0.1, 2.0, float("nan")):
        with pytest.raises(ValueError):
            scene_export.clean_pointcloud(*args, tol=tol)
    with pytest.raises(_lib.Geo4DNativeError):                                   # no CPU fallback
        scene_export.clean_pointcloud(*args, tol=0.001)


def test_rgb_frames_layouts():
    from geo4d_amd.align import rgb_frames
    g = torch.Generator().manual_seed(1)
    x = torch.rand((4, 5, 6, 3), generator=g) * 2.4 - 1.2                          # [T, H, W, 3], some values beyond [-1, 1]
    want = (x * 0.5 + 0.5).clip(0, 1)
    for v in (x, x.permute(0, 3, 1, 2), x.permute(3, 0, 1, 2), x.permute(3, 0, 1, 2)[None]):
        assert torch.equal(rgb_frames(v, 4, 5, 6), want)
    u8 = (torch.rand((4, 5, 6, 3), generator=g) * 255).to(torch.uint8)
    assert torch.equal(rgb_frames(u8, 4, 5, 6), u8.float() / 255)
    with pytest.raises(ValueError):
        rgb_frames(x, 3, 5, 6)
