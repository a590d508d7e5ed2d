"""The corner table and its consumers on the HIP path (ops.mesh_adjacency, ops.mesh_smooth_step, ops.mesh_vertex_normals,
geo4d_amd/mesh.py + csrc/mesh_smooth.hip) against their numpy restatement (tests/mesh_smooth_restatement.py), with np.array_equal on
offsets, corners, boundary, the normals and the smoothed vertices and nothing excused: the hand cases, the smallest shapes at which the
fill, either sort path and the gathers can go wrong, determinism, and what is built on them: tsdf_mesh / tsdf_scene, the export,
save_scene and render_scene on the scene with a planted floater."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import mesh_components_restatement as mc
import mesh_smooth_restatement as ms
import tsdf_mesh_restatement as tm
import tsdf_restatement as tr
from scene_cases import truth_aligner as _synthetic_aligner
from test_mesh_components_cpu import INT_MAX, INT_MIN, bad_index_mesh, fan, percolation_mesh, random_mesh, strip
from test_mesh_smooth_cpu import HAND_CASES

pytestmark = pytest.mark.gpu
EVERY_ROW_BY_A_WAVE, EVERY_ROW_BY_A_THREAD = 0, 1 << 30


def _t(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _positions(Nv, seed=5):
    """O(1) coordinates away from zero."""
    return (np.random.default_rng(seed).random((Nv, 3)) + 0.5).astype(np.float32)


def _adjacency(dev, faces, Nv, mask=None, long_row=None):
    """ops.mesh_adjacency on numpy inputs; the three device tensors, shapes and dtypes checked."""
    from geo4d_amd import ops
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    out = ops.mesh_adjacency(_t(dev, faces), Nv, None if mask is None else _t(dev, np.asarray(mask, dtype=bool)), long_row=long_row)
    torch.cuda.synchronize()
    offsets, corners, boundary = out
    assert offsets.dtype == torch.int32 and tuple(offsets.shape) == (Nv + 1,) and corners.dtype == torch.int32 and corners.dim() == 1
    assert boundary.dtype == torch.uint8 and tuple(boundary.shape) == (Nv,) and all(o.device.type == "cuda" for o in out)
    return out


def _same(tag, dev, vertices, faces, mask=None, long_row=None, s=0.5):
    """Table, boundary, normals, a free and a pinned step of the device equal the restatement's; returns the restatement's table."""
    from geo4d_amd import ops
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    Nv = len(vertices)
    got = _adjacency(dev, faces, Nv, mask, long_row)
    ref = ms.adjacency(faces, Nv, mask)
    print(f"[mesh smooth {tag}] Nv {Nv}, T {len(faces)}: E {len(ref[1])}, longest row {int(np.diff(ref[0]).max()) if Nv else 0}, "
          f"{int(ref[2].sum())} boundary vertices")
    for name, g, r in zip(("offsets", "corners", "boundary"), got, ref):
        assert tuple(g.shape) == r.shape and np.array_equal(g.cpu().numpy(), r), (tag, name)
    tv, tf = _t(dev, vertices), _t(dev, faces)
    normals = ops.mesh_vertex_normals(tv, tf, got[0], got[1])
    assert np.array_equal(normals.cpu().numpy(), ms.normals(vertices, faces, ref[0], ref[1])), (tag, "normals")
    for pinned in (None, ref[2]):
        out = ops.mesh_smooth_step(tv, tf, got[0], got[1], s, None if pinned is None else got[2])
        assert (Nv == 0 or out.data_ptr() != tv.data_ptr()) and out.dtype == torch.float32 and tuple(out.shape) == (Nv, 3)
        assert np.array_equal(out.cpu().numpy(), ms.step(vertices, faces, ref[0], ref[1], s, pinned)), (tag, "step", pinned is not None)
    assert np.array_equal(tv.cpu().numpy(), vertices)                                # a step never writes its input
    return ref


# ---- 1. the table and its consumers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_hand_cases(dev, case):
    name, vertices, faces, mask, offsets, corners, boundary, normals, stepped = case
    from geo4d_amd import ops
    got = _adjacency(dev, faces, len(vertices), mask)
    assert [g.cpu().tolist() for g in got] == [offsets, corners, boundary], name
    tv, tf = _t(dev, np.asarray(vertices, dtype=np.float32)), _t(dev, np.asarray(faces, dtype=np.int32))
    if normals is not None:
        assert np.array_equal(ops.mesh_vertex_normals(tv, tf, got[0], got[1]).cpu().numpy(), np.asarray(normals, dtype=np.float32)), name
    if stepped is not None:
        assert np.array_equal(ops.mesh_smooth_step(tv, tf, got[0], got[1], 0.5).cpu().numpy(), np.asarray(stepped, dtype=np.float32)), name
    _same(name, dev, vertices, faces, mask)


def test_nothing_and_next_to_nothing(dev):
    from geo4d_amd import mesh
    none = np.zeros((0, 3), np.int32)
    for faces, Nv in ((none, 0), (none, 7), ([[0, 0, 0]], 0), ([[0, 1, 2]], 0)):
        v = _positions(Nv)
        off, cor, b = _same("empty", dev, v, faces)
        assert off.tolist() == [0] * (Nv + 1) and len(cor) == 0 and not b.any()
        tv, tf = _t(dev, v), _t(dev, np.asarray(faces, dtype=np.int32).reshape(-1, 3))
        assert torch.equal(mesh.smooth_mesh(tv, tf, iterations=2), tv) and not mesh.vertex_normals(tv, tf).any()
        assert mesh.mesh_adjacency(tf, Nv)["entries"] == 0


@pytest.mark.parametrize("T", [255, 256, 257])
def test_round_the_block_size(dev, T):
    rng = np.random.default_rng(T)
    _same(f"random {T}", dev, _positions(300), random_mesh(rng, 300, T))
    _same(f"random {T} masked", dev, _positions(T), random_mesh(rng, T, T), rng.random(T) < 0.7)
    _same(f"more vertices than faces {T}", dev, _positions(1000), random_mesh(rng, 1000, T))
    _same(f"vertices round the block size {T}", dev, _positions(T), random_mesh(rng, T, 700))


def test_bad_indices_of_every_kind(dev):
    faces, Nv = bad_index_mesh()
    assert {-1, Nv, INT_MAX, INT_MIN} <= set(faces.reshape(-1).tolist())
    assert _same("bad indices", dev, _positions(Nv), faces)[0][-1] == 3 * 260
    _same("bad indices masked", dev, _positions(Nv), faces, np.arange(len(faces)) % 3 != 0)


def test_both_row_paths_give_the_same_table(dev):
    """fan(300): a hub row of 300 entries beside rows of 1 to 2; random faces on 40 vertices: rows of about 45 and repeated indices."""
    rng = np.random.default_rng(2)
    for tag, (faces, Nv) in (("fan 300, hub highest", fan(300, True)), ("fan 300, hub lowest", fan(300, False)),
                             ("crowded", (random_mesh(rng, 40, 600), 40))):
        v = _positions(Nv)
        tables = []
        for long_row in (EVERY_ROW_BY_A_WAVE, None, EVERY_ROW_BY_A_THREAD, 1, 5):
            _same(f"{tag}, long_row {long_row}", dev, v, faces, long_row=long_row)
            tables.append(_adjacency(dev, faces, Nv, long_row=long_row))
        for other in tables[1:]:
            assert all(torch.equal(a, b) for a, b in zip(tables[0], other))
    masked = rng.random(600) < 0.5
    _same("crowded, masked, by waves", dev, _positions(40), faces, masked, long_row=EVERY_ROW_BY_A_WAVE)


@pytest.mark.parametrize("hub_high", [True, False])
def test_fan_of_2000_triangles(dev, hub_high):
    faces, Nv = fan(2000, hub_high)
    ref = _same(f"fan 2000, hub {'highest' if hub_high else 'lowest'}", dev, _positions(Nv), faces)
    assert int(np.diff(ref[0]).max()) == 2000 and ref[2].all()                       # an open fan: the rim, and the hub through the rim's two ends


def test_strip_of_4097_triangles(dev):
    faces, Nv = strip(4097, "random")
    ref = _same("strip", dev, _positions(Nv), faces)
    assert ref[0][-1] == 3 * 4097 and ref[2].all()                                   # every vertex of a strip is on its boundary


def test_percolation_mesh_with_repeated_indices(dev):
    faces, Nv = percolation_mesh()
    _same("percolation", dev, _positions(Nv), faces)
    _same("percolation masked", dev, _positions(Nv), faces, np.random.default_rng(1).random(len(faces)) < 0.8)


def _mesh_select(dev, vertices, faces, keep):
    from geo4d_amd import ops
    out = ops.mesh_select(_t(dev, vertices), _t(dev, faces), _t(dev, keep))
    return out[0].cpu().numpy(), out[3].cpu().numpy()


def test_the_tsdf_test_blocks_and_what_mesh_select_makes_of_them(dev):
    v, f = ms.noisy_icosphere()
    assert not _same("icosphere", dev, v, f)[2].any()
    mask = ~(f == 0).any(1)
    ref = _same("icosphere, vertex 0 masked", dev, v, f, mask)
    assert ref[2].sum() == 5 and ref[0][1] == 0
    _same("icosphere, selected", dev, *_mesh_select(dev, v, f, mask))
    m = tm.mesh(*tm.sphere_block((0, 0, 0), colours=True), 1.0, 4.0)
    assert not _same("sphere block", dev, m["vertices"], m["faces"])[2].any()       # closed: no boundary
    m = tm.mesh(*tm.random_block(8, 6, holes=0.03, weak=0.03), 0.1, 4.0)
    ref = _same("8^3 block", dev, m["vertices"], m["faces"])
    _, undirected = tm.edge_counts(m["faces"])
    assert (undirected > 2).any() and 0 < ref[2].sum() < len(ref[2])                 # non-manifold edges, holes
    keep = np.arange(len(m["faces"])) % 3 != 0
    _same("8^3 block, selected", dev, *_mesh_select(dev, m["vertices"], m["faces"], keep))


# ---- 2. smoothing ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy_wall():
    s = tr.static_scene(0.02)
    o = s["out"]
    m = tm.mesh(o["K"], o["f"], o["Wt"], o["col"], s["voxel"], tr.DEFAULTS["min_weight"])
    return m["vertices"], m["faces"]


@pytest.mark.parametrize("iterations,pin,mu", [(1, True, -0.53), (2, True, -0.53), (10, True, -0.53), (10, False, -0.53), (2, False, -0.53),
                                               (3, True, 0), (3, False, 0.0)])
def test_smoothing_the_noisy_wall(dev, noisy_wall, iterations, pin, mu):
    from geo4d_amd import mesh
    v, f = noisy_wall
    tv, tf = _t(dev, v), _t(dev, f)
    got = mesh.smooth_mesh(tv, tf, iterations=iterations, mu=mu, pin_boundary=pin)
    ref = ms.smooth(v, f, iterations=iterations, mu=mu, pin_boundary=pin)
    assert got.dtype == torch.float32 and got.data_ptr() != tv.data_ptr() and np.array_equal(tv.cpu().numpy(), v)
    assert np.array_equal(got.cpu().numpy(), ref)
    boundary = ms.adjacency(f, len(v))[2] == 1
    assert np.array_equal(ref[boundary], v[boundary]) == pin and not np.array_equal(ref[~boundary], v[~boundary])
    assert np.array_equal(mesh.vertex_normals(got, tf).cpu().numpy(), ms.vertex_normals(ref, f))


def test_a_nan_spreads_as_the_restatement_says(dev, noisy_wall):
    from geo4d_amd import mesh
    v, f = noisy_wall
    v = v.copy()
    v[600, 2] = np.nan
    got = mesh.smooth_mesh(_t(dev, v), _t(dev, f), iterations=2, pin_boundary=False).cpu().numpy()
    ref = ms.smooth(v, f, iterations=2, pin_boundary=False)
    assert 4 < np.isnan(ref).any(1).sum() < len(v) and np.array_equal(got, ref, equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    n = mesh.vertex_normals(_t(dev, v), _t(dev, f)).cpu().numpy()
    assert np.array_equal(n, ms.vertex_normals(v, f)) and (n[600] == 0).all()


def test_two_runs_a_passed_table_and_no_iterations(dev, noisy_wall):
    from geo4d_amd import mesh
    v, f = noisy_wall
    tv, tf = _t(dev, v), _t(dev, f)
    first = mesh.smooth_mesh(tv, tf, iterations=4)
    assert torch.equal(first, mesh.smooth_mesh(tv, tf, iterations=4))
    table = mesh.mesh_adjacency(tf, len(v))
    again = mesh.mesh_adjacency(tf, len(v))
    assert sorted(table) == ["boundary", "corners", "entries", "offsets"] and table["boundary"].dtype == torch.bool
    assert table["entries"] == 3 * len(f) and all(torch.equal(table[k], again[k]) for k in ("offsets", "corners", "boundary"))
    assert torch.equal(mesh.smooth_mesh(tv, tf, iterations=4, adjacency=table), first)
    assert torch.equal(mesh.vertex_normals(first, tf, adjacency=table), mesh.vertex_normals(first, tf))   # the table outlives the smoothing
    assert torch.equal(mesh.vertex_normals(tv, tf), mesh.vertex_normals(tv, tf))
    assert mesh.smooth_mesh(tv, tf, iterations=0) is tv and mesh.smooth_mesh(tv, tf, iterations=0, adjacency=table) is tv
    mask = np.arange(len(f)) % 5 != 0
    masked = mesh.smooth_mesh(tv, tf, iterations=2, face_mask=_t(dev, mask))
    assert np.array_equal(masked.cpu().numpy(), ms.smooth(v, f, iterations=2, face_mask=mask))
    assert np.array_equal(mesh.vertex_normals(tv, tf, face_mask=_t(dev, mask)).cpu().numpy(), ms.vertex_normals(v, f, mask))
    with pytest.raises(ValueError, match="adjacency does not fit"):
        mesh.smooth_mesh(tv[:-1], tf, iterations=1, adjacency=table)


# ---- 3. up the stack ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floater():
    return mc.floater_scene()


def _tsdf_mesh(dev, s, **kw):
    from geo4d_amd import tsdf
    out = tsdf.tsdf_mesh(_t(dev, s["pts3d"]), _t(dev, s["depth"]), _t(dev, s["static"]), s["cams2world"], s["K"], _t(dev, s["rgba"]),
                         voxel=s["voxel"], **kw)
    torch.cuda.synchronize()
    return out


def _restated(filtered, iterations, pin=True):
    """(smoothed vertices, their normals) of the restatement on the device's own (filtered) mesh."""
    v, f = filtered["vertices"].cpu().numpy(), filtered["faces"].cpu().numpy()
    p = ms.smooth(v, f, iterations=iterations, pin_boundary=pin)
    return p, ms.vertex_normals(p, f)


def test_tsdf_mesh_smooths_after_the_filter_and_adds_normals(dev, floater):
    filtered = _tsdf_mesh(dev, floater, min_component_fraction=0.05)
    got = _tsdf_mesh(dev, floater, min_component_fraction=0.05, smooth_iterations=3, normals=True)
    assert sorted(got) == sorted(list(filtered) + ["normals"]) and filtered["removed_faces"] == 48
    p, n = _restated(filtered, 3)
    assert np.array_equal(got["vertices"].cpu().numpy(), p) and np.array_equal(got["normals"].cpu().numpy(), n)
    assert not torch.equal(got["vertices"], filtered["vertices"]) and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
    for k in ("rgba", "weight", "faces"):
        assert torch.equal(got[k], filtered[k]), k
    free = _tsdf_mesh(dev, floater, min_component_fraction=0.05, smooth_iterations=3, smooth_pin_boundary=False)
    assert "normals" not in free and np.array_equal(free["vertices"].cpu().numpy(), _restated(filtered, 3, pin=False)[0])
    only = _tsdf_mesh(dev, floater, normals=True)                                    # no filter, no smoothing: the raw mesh's normals
    raw = _tsdf_mesh(dev, floater)
    assert torch.equal(only["vertices"], raw["vertices"]) and np.array_equal(only["normals"].cpu().numpy(), _restated(raw, 0)[1])
    none = _tsdf_mesh(dev, floater, smooth_iterations=0)
    assert sorted(none) == sorted(raw) and torch.equal(none["vertices"], raw["vertices"])
    with pytest.raises(ValueError, match="iterations must be an integer >= 0"):
        _tsdf_mesh(dev, floater, smooth_iterations=-1)


@pytest.fixture()
def aligner(dev, floater):
    a = _synthetic_aligner(dev, floater)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(9)).to(dev)
    return a


def test_tsdf_scene_smooths_its_mesh_and_leaves_the_points(dev, aligner):
    from geo4d_amd import tsdf
    filtered = dict(tsdf.tsdf_scene(aligner, is_msk=False, mesh=True, min_component_fraction=0.05))
    got = tsdf.tsdf_scene(aligner, is_msk=False, mesh=True, min_component_fraction=0.05, smooth_iterations=3, normals=True)
    assert got is aligner.tsdf and sorted(got) == sorted(list(filtered) + ["vertex_normals"])
    p, n = _restated(filtered, 3)
    assert np.array_equal(got["vertices"].cpu().numpy(), p) and np.array_equal(got["vertex_normals"].cpu().numpy(), n)
    for k in ("points", "rgba", "weight", "vertex_rgba", "vertex_weight", "faces"):
        assert torch.equal(got[k], filtered[k]), k
    for kw in (dict(smooth_iterations=3), dict(normals=True), dict(smooth_pin_boundary=False)):
        with pytest.raises(ValueError, match="pass mesh=True"):
            tsdf.tsdf_scene(aligner, is_msk=False, **kw)


def _first_primitive(path):
    data = open(path, "rb").read()
    n_json = struct.unpack("<I", data[12:16])[0]
    doc = json.loads(data[20:20 + n_json])
    return doc, doc["meshes"][0]["primitives"][0], data[20 + n_json + 8:]


def _holds_normals(path, V, T):
    doc, prim, binary = _first_primitive(path)
    assert V > 0 and T > 0 and prim["mode"] == 4 and sorted(prim["attributes"]) == ["COLOR_0", "NORMAL", "POSITION"]
    pos, col, nrm = (doc["accessors"][prim["attributes"][k]] for k in ("POSITION", "COLOR_0", "NORMAL"))
    idx = doc["accessors"][prim["indices"]]
    assert pos["count"] == col["count"] == nrm["count"] == V and nrm["type"] == "VEC3" and nrm["componentType"] == 5126
    assert idx["count"] == 3 * T and idx["componentType"] == 5125
    view = doc["bufferViews"][nrm["bufferView"]]
    assert view["target"] == 34962
    n = np.frombuffer(binary[view["byteOffset"]:view["byteOffset"] + view["byteLength"]], dtype=np.float32).reshape(V, 3)
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 1e-6
    return n


def test_export_and_save_scene_write_normal(dev, floater, tmp_path):
    from geo4d_amd import scene_export
    a = _synthetic_aligner(dev, floater)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    kw = dict(as_pointcloud=False, is_msk=False, tsdf_mesh=True, motion="static")
    asked = dict(smooth_iterations=3, normals=True)
    new = dict(asked, min_component_fraction=0.05)                                   # the filter leaves no vertex without a face
    path = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="smooth", **kw, **new)
    n = _holds_normals(path, len(a.tsdf["vertices"]), len(a.tsdf["faces"]))
    assert np.array_equal(n, a.tsdf["vertex_normals"].cpu().numpy()) and a.tsdf["removed_faces"] > 0
    # the defaults, named or not, write the same bytes
    defaults = dict(smooth_iterations=None, smooth_pin_boundary=True, normals=False)
    plain = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="plain", **kw)
    assert "vertex_normals" not in a.tsdf
    named = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name="named", **kw, **defaults)
    assert open(plain, "rb").read() == open(named, "rb").read()
    assert "NORMAL" not in _first_primitive(plain)[1]["attributes"]
    video = torch.rand((1, 3, a.n, a.H, a.W), generator=torch.Generator().manual_seed(6)) * 2 - 1
    base = scene_export.save_scene(a, str(tmp_path / "base"), "seq", imgs=video, tsdf_mesh_static=True, tsdf_static=True)
    named = scene_export.save_scene(a, str(tmp_path / "named"), "seq", imgs=video, tsdf_mesh_static=True, tsdf_static=True, **defaults)
    names = sorted(os.listdir(base))
    assert sorted(os.listdir(named)) == names and "seq_static_tsdf_mesh.glb" in names
    for f in names:
        assert open(os.path.join(base, f), "rb").read() == open(os.path.join(named, f), "rb").read(), f
    # given, they reach the mesh's glb and no other file
    smooth = scene_export.save_scene(a, str(tmp_path / "smooth"), "seq", imgs=video, tsdf_mesh_static=True, tsdf_static=True, **new)
    assert sorted(os.listdir(smooth)) == names
    for f in names:
        same = open(os.path.join(base, f), "rb").read() == open(os.path.join(smooth, f), "rb").read()
        assert same == (f != "seq_static_tsdf_mesh.glb"), f
    _holds_normals(os.path.join(smooth, "seq_static_tsdf_mesh.glb"), len(a.tsdf["vertices"]), len(a.tsdf["faces"]))
    for more in (dict(as_pointcloud=True), dict(as_pointcloud=True, tsdf_voxel=True), dict(as_pointcloud=True, fuse_voxel=True),
                 dict(as_pointcloud=False)):
        with pytest.raises(ValueError, match="are for the TSDF surface mesh alone"):
            scene_export.get_3D_model_from_scene(str(tmp_path), True, a, is_msk=False, **more, **asked)


def test_render_scene_draws_the_smoothed_mesh(dev, aligner):
    from geo4d_amd import render
    a = aligner
    before = render.render_scene(a, "cameras", is_msk=False, static_mesh=True)
    raw = dict(a.tsdf)
    a.tsdf = None
    after = render.render_scene(a, "cameras", is_msk=False, static_mesh=True, smooth_iterations=3)
    p, _ = _restated(raw, 3)
    assert np.array_equal(a.tsdf["vertices"].cpu().numpy(), p) and torch.equal(a.tsdf["faces"], raw["faces"])
    assert "vertex_normals" not in a.tsdf
    assert not torch.equal(after["depth"], before["depth"])
    face = after["face"]
    assert int(face.min()) >= -1 and int(face.max()) < len(raw["faces"]) and int((face >= 0).sum()) > 1000
    for kw in (dict(smooth_iterations=3), dict(smooth_pin_boundary=False)):
        with pytest.raises(ValueError, match="pass static_mesh"):
            render.render_scene(a, "cameras", is_msk=False, **kw)
