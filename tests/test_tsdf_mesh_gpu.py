"""The surface nets on the HIP path (ops.tsdf_mesh_extract, geo4d_amd/tsdf.py tsdf_mesh + csrc/tsdf_mesh.hip) against their numpy
restatement (tests/tsdf_mesh_restatement.py), bit for bit: hand-made fields that reach every branch, the synthetic scenes (the
restatement is fed the device's own field, so nothing is excusable), determinism, that tsdf_points still gives what it gave, and what
is built on the mesh: tsdf_scene(mesh=True), the export's `tsdf_mesh` and save_scene's `tsdf_mesh_static`."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import motion_restatement as mr
import tsdf_mesh_restatement as tm
import tsdf_restatement as tr
from scene_cases import tiny_aligner as _aligner, truth_aligner as _synthetic_aligner
from test_tsdf_gpu import _compare, _gpu

pytestmark = pytest.mark.gpu
KEYS = ("vertices", "rgba", "weight", "faces")


def _t(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _extract(dev, K, f, Wt, col, voxel=0.1, min_weight=4.0):
    """ops.tsdf_mesh_extract on numpy arrays; the outputs as numpy, shapes and dtypes checked."""
    from geo4d_amd import ops
    v, c, w, fa = ops.tsdf_mesh_extract(_t(dev, K), _t(dev, f), _t(dev, Wt), _t(dev, col), voxel=voxel, min_weight=min_weight)
    torch.cuda.synchronize()
    V, T = len(v), len(fa)
    assert v.dtype == torch.float32 and tuple(v.shape) == (V, 3) and w.dtype == torch.float32 and tuple(w.shape) == (V,)
    assert fa.dtype == torch.int32 and tuple(fa.shape) == (T, 3) and fa.device.type == "cuda"
    assert (c is None) == (col is None) and (c is None or (c.dtype == torch.uint8 and tuple(c.shape) == (V, 4)))
    return dict(vertices=v.cpu().numpy(), rgba=None if c is None else c.cpu().numpy(), weight=w.cpu().numpy(), faces=fa.cpu().numpy())


def _same(tag, got, ref):
    print(f"[tsdf mesh {tag}] V {len(ref['vertices'])}, T {len(ref['faces'])}, {int((ref['crossing'] & ~ref['used']).sum())} cells with a sign "
          "change and no vertex")
    for k in KEYS:
        assert (got[k] is None and ref[k] is None) or (got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k])), (tag, k)


# ---- 1. hand-made fields -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colours", [False, True])
@pytest.mark.parametrize("origin", [0, (1 << 20) - 6, -(1 << 20) + 1])
def test_sphere_block_at_the_ends_of_the_grid(dev, origin, colours):
    """At the upper end + E_a carries out of a full key field, at the lower end - E_a gives the field 0: neither finds a neighbour."""
    K, f, Wt, col = tm.sphere_block((origin,) * 3, colours=colours)
    ref = tm.mesh(K, f, Wt, col, 1.0, 4.0)
    assert len(ref["vertices"]) == 74 and len(ref["faces"]) == 144
    _same(f"sphere at {origin}", _extract(dev, K, f, Wt, col, voxel=1.0), ref)


def test_plane_random_holes_and_ties(dev):
    K, f, Wt, col = tm.plane_block()
    ref = tm.mesh(K, f, Wt, col, 0.1, 4.0)
    assert len(ref["faces"]) == 18 and (f == 0).any()
    _same("plane", _extract(dev, K, f, Wt, col), ref)
    K, f, Wt, col = tm.random_block(5, 4)
    ref = tm.mesh(K, f, Wt, col, 0.1, 4.0)
    assert len(ref["faces"]) == 108 and (tm.edge_counts(ref["faces"])[1] > 2).sum() == 15 and (ref["crossing"] & ~ref["used"]).sum() == 1
    _same("dense random 5^3", _extract(dev, K, f, Wt, col), ref)
    K, f, Wt, col = tm.random_block(8, 6, holes=0.03, weak=0.03)
    ref = tm.mesh(K, f, Wt, col, 0.1, 4.0)
    assert 450 < len(K) < 512 and (Wt < 4).sum() > 5 and len(ref["faces"]) >= 20 and (ref["crossing"] & ~ref["used"]).sum() >= 1
    _same("8^3 with holes and weak voxels", _extract(dev, K, f, Wt, col), ref)
    K, f, Wt, col = tm.random_block(5, 1)
    f = np.where(f >= 0, np.float32(0.5), np.float32(-0.5))                          # every |f| ties: the lowest corner gives the colour
    ref = tm.mesh(K, f, Wt, col, 0.1, 4.0)
    assert len(ref["faces"]) >= 20 and len(np.unique(ref["rgba"], axis=0)) > 10
    _same("ties", _extract(dev, K, f, Wt, col), ref)


def test_min_weight_is_inclusive(dev):
    """A tenth of the sphere block's voxels weigh exactly min_weight: all of them are live, the mesh is the whole sphere."""
    K, f, Wt, col = tm.sphere_block(colours=True)
    Wt = np.where(np.random.default_rng(2).random(len(K)) < 0.1, np.float32(5), np.float32(8))
    ref = tm.mesh(K, f, Wt, col, 0.1, 5.0)
    assert len(ref["faces"]) == 144 and ref["weight"].min() == 5.0 and ref["weight"].max() == 8.0
    _same("min_weight 5", _extract(dev, K, f, Wt, col, min_weight=5.0), ref)
    above = float(np.nextafter(np.float32(5), np.float32(6)))
    ref = tm.mesh(K, f, Wt, col, 0.1, above)
    assert len(ref["faces"]) < 144
    _same("min_weight just above 5", _extract(dev, K, f, Wt, col, min_weight=above), ref)


@pytest.mark.parametrize("colours", [False, True])
def test_nothing_to_mesh_gives_empty_outputs(dev, colours):
    """M = 0, M = 1, one complete cell without a sign change, and 1-thick slabs of 257 and 513 voxels (two and three blocks, every pair
    a sign change, no complete cell): empty outputs of the right shapes and dtypes (_extract checks them)."""
    K8, _ = tm.block_keys((2, 2, 2))
    fields = [tm.slab(0), tm.slab(1), (K8, np.full(8, 0.25, np.float32), np.full(8, 8, np.float32), None), tm.slab(257), tm.slab(513)]
    for K, f, Wt, _ in fields:
        col = np.full((len(K), 4), 7, np.uint8) if colours else None
        got = _extract(dev, K, f, Wt, col)
        assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["weight"].shape == (0,), len(K)
        assert (got["rgba"].shape == (0, 4)) if colours else got["rgba"] is None


def test_row_offsets_outside_the_output_write_nothing(dev):
    """The vertices and faces launches given offsets that are not this field's (every vertex id -1, every quad row Q): no row is
    written, nothing faults."""
    from geo4d_amd import _lib, ops
    lib = _lib.load()
    K, f, Wt, _ = (_t(dev, x) for x in tm.sphere_block())
    M, (V, Q), stream = len(K), (74, 72), ops._stream()
    complete, used = (torch.empty(M, device=dev, dtype=torch.uint8) for _ in range(2))
    counts = torch.empty(M, device=dev, dtype=torch.int32)
    _lib.check(lib.geo4d_tsdf_mesh_cells(K.data_ptr(), M, f.data_ptr(), Wt.data_ptr(), 4.0, complete.data_ptr(), stream), "cells")
    _lib.check(lib.geo4d_tsdf_mesh_count(K.data_ptr(), M, complete.data_ptr(), counts.data_ptr(), used.data_ptr(), stream), "count")
    assert int(counts.sum()) == Q and int(used.sum()) == V and int((complete != 0).sum()) == 117
    no_vertex, no_quad = torch.full((M,), -1, device=dev, dtype=torch.int64), torch.full((M,), Q, device=dev, dtype=torch.int64)
    good_vertex = (torch.cumsum(used, 0, dtype=torch.int64) - used).contiguous()
    vert, w = torch.full((V, 3), 7.0, device=dev), torch.full((V,), 7.0, device=dev)
    faces = torch.full((2 * Q, 3), -7, device=dev, dtype=torch.int32)
    _lib.check(lib.geo4d_tsdf_mesh_vertices(K.data_ptr(), M, f.data_ptr(), Wt.data_ptr(), 0, used.data_ptr(), no_vertex.data_ptr(), V, 1.0,
                                            vert.data_ptr(), 0, w.data_ptr(), stream), "vertices")
    for first_quad, first_vertex in ((no_quad, good_vertex), ((torch.cumsum(counts, 0, dtype=torch.int64) - counts).contiguous(), no_vertex)):
        _lib.check(lib.geo4d_tsdf_mesh_faces(K.data_ptr(), M, f.data_ptr(), complete.data_ptr(), counts.data_ptr(), first_quad.data_ptr(),
                                             first_vertex.data_ptr(), Q, V, faces.data_ptr(), stream), "faces")
    torch.cuda.synchronize()
    assert (vert == 7.0).all() and (w == 7.0).all() and (faces == -7).all()


# ---- 2. the synthetic scenes ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return dict(clean=tr.static_scene(0.0), noisy=tr.static_scene(0.02))


def _mesh(dev, s, **kw):
    from geo4d_amd import tsdf
    out = tsdf.tsdf_mesh(_t(dev, s["pts3d"]), _t(dev, s["depth"]), _t(dev, s["static"]), s["cams2world"], s["K"], _t(dev, s["rgba"]),
                         voxel=s["voxel"], **kw)
    torch.cuda.synchronize()
    assert sorted(out) == sorted(KEYS + ("voxels", "dropped", "overflow", "voxel")) and out["dropped"] == 0 and out["overflow"] == 0
    return out


def _field(dev, s):
    """The device's own field of scene dict `s`, as numpy: (K, f, Wt, col)."""
    from geo4d_amd import ops
    from geo4d_amd.scene_view import views_of
    views = views_of(s["cams2world"], s["K"]).to(dev)
    K, f, wt, col, M, dropped = ops.tsdf_field(_t(dev, s["pts3d"]), _t(dev, s["depth"]), _t(dev, s["static"]), views, _t(dev, s["centres"]),
                                               _t(dev, s["rgba"]), voxel=float(np.float32(s["voxel"])))
    assert dropped == 0 and M == len(K)
    return K.cpu().numpy(), f.cpu().numpy(), wt.cpu().numpy(), col.cpu().numpy()


@pytest.mark.parametrize("which", ["clean", "noisy"])
def test_synthetic_scenes_match_the_restatement_on_the_devices_field(dev, scenes, which):
    s = scenes[which]
    got = _mesh(dev, s)
    K, f, Wt, col = _field(dev, s)
    ref = tm.mesh(K, f, Wt, col, s["voxel"], 4.0)
    assert got["voxels"] == len(K) and len(ref["vertices"]) > 900 and len(ref["faces"]) > 1800
    _same(which, {k: got[k].cpu().numpy() for k in KEYS}, ref)
    assert int(got["faces"].max()) < len(got["vertices"]) and int(got["faces"].min()) == 0


def test_two_runs_and_two_capacities_are_equal(dev, scenes):
    s = scenes["noisy"]
    cap = tr.default_capacity(int(s["static"].sum()))
    runs = [_mesh(dev, s, capacity=c) for c in (None, None, cap, 2 * cap)]
    assert len(runs[0]["faces"]) > 1800
    for r in runs[1:]:
        assert r["voxels"] == runs[0]["voxels"]
        for k in KEYS:
            assert torch.equal(r[k], runs[0][k]), k


@pytest.mark.parametrize("which", ["clean", "noisy"])
def test_tsdf_points_gives_what_it_gave(dev, scenes, which):
    """tsdf_points now goes through ops.tsdf_field: the same points, bit for bit, as the restatement of the points' rule."""
    s = scenes[which]
    got = _gpu(dev, s, s["static"], s["rgba"], voxel=s["voxel"])
    assert _compare(which, got, s["out"], s, s["static"], None, voxel=s["voxel"]) == 0


# ---- 3. the scene level ------------------------------------------------------------------------------------------------------------------
def _first_primitive(path):
    """(the glb's JSON document, its first primitive)."""
    data = open(path, "rb").read()
    doc = json.loads(data[20:20 + struct.unpack("<I", data[12:16])[0]])
    return doc, doc["meshes"][0]["primitives"][0]


def _is_the_mesh(path, surf):
    doc, prim = _first_primitive(path)
    V, T = len(surf["vertices"]), len(surf["faces"])
    assert V > 0 and T > 0 and prim["mode"] == 4 and "COLOR_0" in prim["attributes"]
    assert doc["accessors"][prim["attributes"]["POSITION"]]["count"] == V and doc["accessors"][prim["attributes"]["COLOR_0"]]["count"] == V
    idx = doc["accessors"][prim["indices"]]
    assert idx["count"] == 3 * T and idx["componentType"] == 5125


def test_tsdf_scene_with_a_mesh(dev):
    from geo4d_amd import tsdf
    s0 = mr.synthetic_scene(noise=0.02)
    tiny, synthetic = _aligner(dev), _synthetic_aligner(dev, s0)
    for a, kw in ((tiny, dict(min_conf_thr=float(tiny.im_conf.median()), min_weight=1.0, trunc=2)), (synthetic, dict(is_msk=False))):
        a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
        plain = dict(tsdf.tsdf_scene(a, **kw))
        assert sorted(plain) == ["dropped", "overflow", "points", "rgba", "voxel", "voxels", "weight"]
        got = tsdf.tsdf_scene(a, mesh=True, **kw)
        assert got is a.tsdf and sorted(got) == sorted(list(plain) + ["vertices", "faces", "vertex_rgba", "vertex_weight"])
        for k in plain:
            assert torch.equal(got[k], plain[k]) if torch.is_tensor(plain[k]) else got[k] == plain[k], k
        V, T = len(got["vertices"]), len(got["faces"])
        assert tuple(got["vertex_rgba"].shape) == (V, 4) and tuple(got["vertex_weight"].shape) == (V,) and got["faces"].dtype == torch.int32
        if T:
            assert int(got["faces"].min()) == 0 and int(got["faces"].max()) == V - 1
    assert T > 1000                                                                 # the synthetic aligner's wall


def test_export_and_save_scene_write_the_mesh(dev, tmp_path):
    """tsdf_mesh=None is today's glb byte for byte; with it the glb's first primitive is the indexed mesh. save_scene(tsdf_mesh_static=
    True) writes <seq>_static_tsdf_mesh.glb and nothing else, and every other file stays byte-identical."""
    from geo4d_amd import scene_export
    s0 = mr.synthetic_scene(noise=0.02)
    a = _synthetic_aligner(dev, s0)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    for kw in (dict(as_pointcloud=True), dict(as_pointcloud=False)):
        plain = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="plain", **kw)
        none = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="none", tsdf_mesh=None, **kw)
        assert a.tsdf is None and open(plain, "rb").read() == open(none, "rb").read()
    path = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="surface", tsdf_mesh=True, as_pointcloud=False, motion="static")
    _is_the_mesh(path, a.tsdf)
    assert os.path.getsize(path) < os.path.getsize(plain) / 4                       # one surface, not n sheets of H W pixels
    voxel = 1.5 * a.tsdf["voxel"]
    path = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="fixed", tsdf_mesh=voxel, as_pointcloud=False)
    assert a.tsdf["voxel"] == float(np.float32(voxel))
    _is_the_mesh(path, a.tsdf)
    with pytest.raises(ValueError, match="tsdf_mesh writes triangles"):
        scene_export.get_3D_model_from_scene(str(tmp_path), True, a, tsdf_mesh=0.05, as_pointcloud=True)
    b = _synthetic_aligner(dev, s0)
    video = torch.rand((1, 3, b.n, b.H, b.W), generator=torch.Generator().manual_seed(6)) * 2 - 1
    base = scene_export.save_scene(b, str(tmp_path / "base"), "seq", imgs=video)
    assert b.dynamic_masks is None and b.tsdf is None
    full = scene_export.save_scene(b, str(tmp_path / "full"), "seq", imgs=video, tsdf_mesh_static=True)
    names = sorted(os.listdir(base))
    assert sorted(os.listdir(full)) == sorted(names + ["seq_static_tsdf_mesh.glb"])
    for f in names:
        assert open(os.path.join(base, f), "rb").read() == open(os.path.join(full, f), "rb").read(), f
    assert b.dynamic_masks is not None                                              # it segmented motion first
    _is_the_mesh(os.path.join(full, "seq_static_tsdf_mesh.glb"), b.tsdf)
