"""Mesh components and selection on the HIP path (ops.mesh_components, ops.mesh_select, geo4d_amd/mesh.py + csrc/mesh_components.hip)
against their numpy restatement (tests/mesh_components_restatement.py), exactly, on all four component outputs and all five selection
outputs: the hand cases, the smallest shapes at which the union-find, the counters and the compaction can go wrong, determinism under
face permutation, and what is built on them: tsdf_mesh / tsdf_scene, the export, save_scene and render_scene on a scene with a planted
floater."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import mesh_components_restatement as mc
import tsdf_mesh_restatement as tm
from scene_cases import truth_aligner as _synthetic_aligner
from test_mesh_components_cpu import (HAND_CASES, INT_MAX, INT_MIN, bad_index_mesh, fan, islands_and_strip, percolation_mesh, random_mesh,
                                      strip)

pytestmark = pytest.mark.gpu
NAMES = ("vertex_component", "face_component", "component_vertices", "component_faces")


def _t(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _components(dev, faces, Nv, mask=None):
    """ops.mesh_components on numpy inputs; numpy outputs, shapes and dtypes checked."""
    from geo4d_amd import ops
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    out = ops.mesh_components(_t(dev, faces), Nv, None if mask is None else _t(dev, np.asarray(mask, dtype=bool)))
    torch.cuda.synchronize()
    assert all(o.dtype == torch.int32 and o.device.type == "cuda" and o.dim() == 1 for o in out)
    assert len(out[0]) == Nv and len(out[1]) == len(faces) and len(out[2]) == len(out[3])
    return [o.cpu().numpy() for o in out]


def _same(tag, dev, faces, Nv, mask=None):
    got, ref = _components(dev, faces, Nv, mask), mc.components(faces, Nv, mask)
    print(f"[mesh components {tag}] Nv {Nv}, T {len(np.asarray(faces).reshape(-1, 3))}: {len(ref[2])} components, largest "
          f"{int(ref[3].max()) if len(ref[3]) else 0} faces, {int((ref[0] < 0).sum())} untouched vertices, {int((ref[1] < 0).sum())} faces not valid")
    for name, g, r in zip(NAMES, got, ref):
        assert g.shape == r.shape and np.array_equal(g, r), (tag, name)
    return ref


def _select(dev, vertices, faces, keep, rgba=None, weight=None):
    from geo4d_amd import ops
    out = ops.mesh_select(_t(dev, vertices), _t(dev, np.asarray(faces, dtype=np.int32).reshape(-1, 3)), _t(dev, np.asarray(keep, dtype=bool)),
                          _t(dev, rgba), _t(dev, weight))
    torch.cuda.synchronize()
    V, T = len(out[0]), len(out[3])
    assert out[0].dtype == torch.float32 and tuple(out[0].shape) == (V, 3) and out[3].dtype == torch.int32 and tuple(out[3].shape) == (T, 3)
    assert out[4].dtype == torch.int32 and tuple(out[4].shape) == (V,)
    assert (out[1] is None) == (rgba is None) and (out[1] is None or (out[1].dtype == torch.uint8 and tuple(out[1].shape) == (V, 4)))
    assert (out[2] is None) == (weight is None) and (out[2] is None or (out[2].dtype == torch.float32 and tuple(out[2].shape) == (V,)))
    return [None if o is None else o.cpu().numpy() for o in out]


def _same_selection(tag, dev, vertices, faces, keep, rgba=None, weight=None):
    got, ref = _select(dev, vertices, faces, keep, rgba, weight), mc.select(vertices, faces, keep, rgba, weight)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert (g is None and r is None) or (g.shape == r.shape and np.array_equal(g, r)), (tag, k)
    return ref


def _attributes(Nv, seed=5):
    rng = np.random.default_rng(seed)
    return rng.random((Nv, 3)).astype(np.float32), rng.integers(0, 256, (Nv, 4), dtype=np.uint8), rng.random(Nv).astype(np.float32)


# ---- 1. components ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_hand_cases(dev, case):
    name, faces, Nv, mask, vc, fc, cv, cf = case
    got = _components(dev, faces, Nv, mask)
    for g, want in zip(got, (vc, fc, cv, cf)):
        assert g.tolist() == want, name


def test_nothing_and_next_to_nothing(dev):
    none = np.zeros((0, 3), np.int32)
    for faces, Nv in ((none, 0), (none, 7), ([[0, 0, 0]], 0), ([[0, 1, 2]], 0)):
        vc, fc, cv, cf = _same("empty", dev, faces, Nv)
        assert (vc == -1).all() and (fc == -1).all() and len(cv) == 0 and len(cf) == 0
    assert _same("one face", dev, [[2, 0, 1]], 3)[3].tolist() == [1]
    assert _same("one face, all masked", dev, [[2, 0, 1]], 3, [0])[3].tolist() == []
    assert _same("one face out of range", dev, [[2, 0, 3]], 3)[3].tolist() == []


@pytest.mark.parametrize("T", [255, 256, 257])
def test_round_the_block_size(dev, T):
    rng = np.random.default_rng(T)
    _same(f"random {T}", dev, random_mesh(rng, 300, T), 300)
    _same(f"random {T} masked", dev, random_mesh(rng, T, T), T, rng.random(T) < 0.7)
    _same(f"more vertices than faces {T}", dev, random_mesh(rng, 1000, T), 1000)


@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
def test_strip_of_4097_triangles(dev, order):
    """Long paths, halving and every link direction: one component whatever the naming."""
    faces, Nv = strip(4097, order)
    assert _same(f"strip {order}", dev, faces, Nv)[3].tolist() == [4097]


@pytest.mark.parametrize("hub_high", [True, False])
def test_fan_of_2000_triangles_contends_on_one_root(dev, hub_high):
    faces, Nv = fan(2000, hub_high)
    ref = _same(f"fan, hub {'highest' if hub_high else 'lowest'}", dev, faces, Nv)
    assert ref[3].tolist() == [2000] and ref[2].tolist() == [2002]


def test_many_roots_beside_one_heavy_counter(dev):
    faces, Nv = islands_and_strip()
    ref = _same("islands and strip", dev, faces, Nv)
    assert ref[3].tolist() == [1] * 1000 + [3000]
    perm = np.random.default_rng(0).permutation(len(faces))                          # waves whose lanes do not share a component
    _same("islands and strip, shuffled", dev, faces[perm], Nv)


def test_raster_ordered_sheet_with_holes(dev):
    """A 64 x 64 sheet in raster order with a random 30 % of its pixels masked, built by the export's own face kernel."""
    from geo4d_amd import ops
    mask = np.random.default_rng(7).random((1, 64, 64)) >= 0.3
    faces, count = ops.scene_mesh_faces(_t(dev, mask), 1, 64, 64, torch.device(dev))
    faces = faces[:int(count)].cpu().numpy()
    ref = _same("sheet", dev, faces, 64 * 64)
    assert len(faces) > 1000 and len(ref[3]) > 5 and ref[3].max() > 500 and (ref[0] < 0).sum() >= (~mask).sum()


def test_percolation_mesh_and_a_face_mask(dev):
    faces, Nv = percolation_mesh()
    assert len(_same("percolation", dev, faces, Nv)[3]) == 320
    _same("percolation masked", dev, faces, Nv, np.random.default_rng(1).random(len(faces)) < 0.8)


def test_bad_indices_of_every_kind(dev):
    faces, Nv = bad_index_mesh()
    assert {-1, Nv, INT_MAX, INT_MIN} <= set(faces.reshape(-1).tolist())
    ref = _same("bad indices", dev, faces, Nv)
    assert (ref[1] < 0).sum() == 40
    _same("bad indices masked", dev, faces, Nv, np.arange(len(faces)) % 3 != 0)


def test_the_tsdf_test_blocks(dev):
    m = tm.mesh(*tm.sphere_block((0, 0, 0), colours=True), 1.0, 4.0)
    assert _same("sphere block", dev, m["faces"], len(m["vertices"]))[3].tolist() == [144]
    m = tm.mesh(*tm.random_block(8, 6, holes=0.03, weak=0.03), 0.1, 4.0)
    assert _same("8^3 block", dev, m["faces"], len(m["vertices"]))[3].tolist() == [392]


def test_two_runs_and_five_face_orders_agree(dev):
    faces, Nv = percolation_mesh()
    mask = np.random.default_rng(1).random(len(faces)) < 0.9
    first = _components(dev, faces, Nv, mask)
    for a, b in zip(first, _components(dev, faces, Nv, mask)):
        assert np.array_equal(a, b)
    for seed in range(5):
        perm = np.random.default_rng(seed).permutation(len(faces))
        got = _components(dev, faces[perm], Nv, mask[perm])
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1][perm])
        assert np.array_equal(got[2], first[2]) and np.array_equal(got[3], first[3])
    sheet, n = strip(4097, "random")
    base = _components(dev, sheet, n)
    for seed in range(5):
        perm = np.random.default_rng(seed).permutation(len(sheet))
        got = _components(dev, sheet[perm], n)
        assert all(np.array_equal(g, b) for g, b in zip(got, (base[0], base[1][perm], base[2], base[3])))


# ---- 2. selection ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", ["none", "rgba", "weight", "both"])
def test_selection_of_a_checkerboard_of_components(dev, attributes):
    faces, Nv = percolation_mesh()
    vertices, rgba, weight = _attributes(Nv)
    rgba, weight = rgba if attributes in ("rgba", "both") else None, weight if attributes in ("weight", "both") else None
    fc = mc.components(faces, Nv)[1]
    ref = _same_selection("checkerboard", dev, vertices, faces, fc % 2 == 0, rgba, weight)
    assert 0 < len(ref[3]) < len(faces) and 0 < len(ref[0]) < Nv
    faces, Nv = islands_and_strip()
    vertices, rgba2, weight2 = _attributes(Nv)
    fc = mc.components(faces, Nv)[1]
    _same_selection("islands", dev, vertices, faces, fc % 2 == 1, None if rgba is None else rgba2, None if weight is None else weight2)


def test_selection_of_everything_nothing_and_bad_faces(dev):
    faces, Nv = strip(4097, "random")
    vertices, rgba, weight = _attributes(Nv)
    got = _select(dev, vertices, faces, np.ones(len(faces), bool), rgba, weight)     # every vertex is referenced: the mesh itself
    for g, want in zip(got, (vertices, rgba, weight, faces, np.arange(Nv, dtype=np.int32))):
        assert np.array_equal(g, want)
    for v, f, keep in ((vertices, faces, np.zeros(len(faces), bool)), (vertices, np.zeros((0, 3), np.int32), np.zeros(0, bool)),
                       (np.zeros((0, 3), np.float32), faces, np.ones(len(faces), bool))):
        a = len(v)
        got = _same_selection("nothing", dev, v, f, keep, rgba[:a], weight[:a])
        assert got[0].shape == (0, 3) and got[1].shape == (0, 4) and got[2].shape == (0,) and got[3].shape == (0, 3) and got[4].shape == (0,)
    bad, Nb = bad_index_mesh()
    vertices, rgba, weight = _attributes(Nb)
    ref = _same_selection("bad indices", dev, vertices, bad, np.ones(len(bad), bool), rgba, weight)
    assert len(ref[3]) == 260
    for T in (255, 256, 257):
        rng = np.random.default_rng(T)
        f = random_mesh(rng, 600, T)
        _same_selection(f"random {T}", dev, *_attributes(600)[:1], f, rng.random(T) < 0.5)


def test_remove_small_components_on_the_islands(dev):
    from geo4d_amd import mesh
    faces, Nv = islands_and_strip()
    vertices, rgba, weight = _attributes(Nv)
    tv, tf, tc, tw = _t(dev, vertices), _t(dev, faces), _t(dev, rgba), _t(dev, weight)
    labels = mesh.mesh_components(tf, Nv)
    assert labels["components"] == 1001 and sorted(labels) == sorted(NAMES + ("components",))
    out = mesh.remove_small_components(tv, tf, min_faces=2, rgba=tc, weight=tw)
    assert (out["components"], out["kept_components"], out["removed_faces"], out["removed_vertices"]) == (1001, 1, 1000, 3000)
    ref = mc.select(vertices, faces, np.arange(len(faces)) >= 1000, rgba, weight)
    for k, r in zip(("vertices", "rgba", "weight", "faces", "vertex_index"), ref):
        assert np.array_equal(out[k].cpu().numpy(), r), k
    out = mesh.remove_small_components(tv, tf, keep_largest=3)                       # the strip, then the two lowest islands
    assert out["kept_components"] == 3 and out["rgba"] is None and out["weight"] is None
    assert np.array_equal(out["faces"].cpu().numpy(), mc.select(vertices, faces, (np.arange(len(faces)) < 2) | (np.arange(len(faces)) >= 1000))[3])
    out = mesh.remove_small_components(tv, tf, min_fraction=1.0, face_mask=_t(dev, np.arange(len(faces)) % 2 == 0))
    assert out["kept_components"] == 1 and out["removed_faces"] == len(faces) - 1500  # the strip's even faces still hang together
    same = mesh.remove_small_components(tv, tf, rgba=tc)
    assert same["vertices"] is tv and same["faces"] is tf and same["rgba"] is tc


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


def _selection_of(raw, vertex_rgba="rgba", vertex_weight="weight", **rule):
    """The restatement's filtered mesh of an unfiltered device mesh: (the five selection outputs, component face counts, kept flags)."""
    v, f = raw["vertices"].cpu().numpy(), raw["faces"].cpu().numpy()
    _, fc, _, cf = mc.components(f, len(v))
    keep = mc.keep_components(cf, **rule)
    return mc.select(v, f, np.append(keep, False)[fc], raw[vertex_rgba].cpu().numpy(), raw[vertex_weight].cpu().numpy()), cf, keep


def test_tsdf_mesh_drops_the_floater(dev, floater):
    raw = _tsdf_mesh(dev, floater)
    got = _tsdf_mesh(dev, floater, min_component_fraction=0.05)
    assert sorted(got) == sorted(list(raw) + ["components", "kept_components", "removed_faces"])
    far = mc.off_wall(raw["vertices"].cpu().numpy()) > 0.5
    ref, cf, keep = _selection_of(raw, min_fraction=0.05)
    print(f"[mesh components tsdf_mesh] V {len(raw['vertices'])}, T {len(raw['faces'])}, components {cf.tolist()}, {far.sum()} vertices far from the wall")
    assert far.sum() >= 1 and len(cf) >= 2 and cf.argmax() == 0 and not far[mc.components(raw["faces"].cpu().numpy(), len(far))[0] == 0].any()
    assert (got["components"], got["kept_components"], got["removed_faces"]) == (len(cf), int(keep.sum()), int(cf[~keep].sum()))
    assert (got["components"], got["removed_faces"]) == (2, 48)                      # what the restatement's field gives (the CPU test)
    assert (mc.off_wall(got["vertices"].cpu().numpy()) <= 0.5).all()
    for k, r in zip(("vertices", "rgba", "weight", "faces"), ref):
        assert np.array_equal(got[k].cpu().numpy(), r), k
    both = _tsdf_mesh(dev, floater, min_component_faces=49, min_component_fraction=0.001)
    assert both["removed_faces"] == 48 and torch.equal(both["faces"], got["faces"]) and torch.equal(both["vertices"], got["vertices"])
    kept = _tsdf_mesh(dev, floater, min_component_faces=48)
    assert kept["removed_faces"] == 0 and torch.equal(kept["faces"], raw["faces"]) and torch.equal(kept["rgba"], raw["rgba"])


@pytest.fixture()
def aligner(dev, floater):
    a = _synthetic_aligner(dev, floater)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(9)).to(dev)
    return a


def test_tsdf_scene_filters_its_mesh_and_leaves_the_points(dev, aligner):
    from geo4d_amd import tsdf
    raw = dict(tsdf.tsdf_scene(aligner, is_msk=False, mesh=True))
    got = tsdf.tsdf_scene(aligner, is_msk=False, mesh=True, min_component_fraction=0.05)
    assert got is aligner.tsdf and sorted(got) == sorted(list(raw) + ["components", "kept_components", "removed_faces"])
    ref, cf, keep = _selection_of(raw, "vertex_rgba", "vertex_weight", min_fraction=0.05)
    assert got["components"] == len(cf) >= 2 and got["removed_faces"] == int(cf[~keep].sum()) > 0 and got["kept_components"] == keep.sum()
    for k, r in zip(("vertices", "vertex_rgba", "vertex_weight", "faces"), ref):
        assert np.array_equal(got[k].cpu().numpy(), r), k
    for k in ("points", "rgba", "weight"):
        assert torch.equal(got[k], raw[k]), k
    assert (mc.off_wall(raw["vertices"].cpu().numpy()) > 0.5).any() and (mc.off_wall(got["vertices"].cpu().numpy()) <= 0.5).all()
    with pytest.raises(ValueError, match="pass mesh=True"):
        tsdf.tsdf_scene(aligner, is_msk=False, min_component_faces=3)


def _first_primitive(path):
    data = open(path, "rb").read()
    doc = json.loads(data[20:20 + struct.unpack("<I", data[12:16])[0]])
    return doc, doc["meshes"][0]["primitives"][0]


def _holds(path, V, T):
    doc, prim = _first_primitive(path)
    assert V > 0 and T > 0 and prim["mode"] == 4 and "COLOR_0" in prim["attributes"]
    pos, col, idx = doc["accessors"][prim["attributes"]["POSITION"]], doc["accessors"][prim["attributes"]["COLOR_0"]], doc["accessors"][prim["indices"]]
    assert pos["count"] == V and pos["type"] == "VEC3" and pos["componentType"] == 5126 and col["count"] == V
    assert idx["count"] == 3 * T and idx["componentType"] == 5125 and idx["type"] == "SCALAR"


def test_export_filters_either_mesh(dev, aligner, tmp_path):
    from geo4d_amd import ops, scene_export
    a, out = aligner, str(tmp_path)
    kw = dict(as_pointcloud=False, is_msk=False)
    scene_export.get_3D_model_from_scene(out, True, a, save_name="raw", tsdf_mesh=True, **kw)
    raw = dict(a.tsdf)
    path = scene_export.get_3D_model_from_scene(out, True, a, save_name="clean", tsdf_mesh=True, min_component_fraction=0.05, **kw)
    assert a.tsdf["removed_faces"] > 0 and len(a.tsdf["faces"]) == len(raw["faces"]) - a.tsdf["removed_faces"]
    _holds(path, len(a.tsdf["vertices"]), len(a.tsdf["faces"]))
    _holds(os.path.join(out, "raw.glb"), len(raw["vertices"]), len(raw["faces"]))
    # the per-image sheets under a speckled mask: the islands go, and the glb holds only the vertices its faces name
    a.tsdf = None
    speckle = torch.from_numpy(np.random.default_rng(3).random((a.n, a.H, a.W)) < 0.55).to(dev)
    a.get_masks = lambda: speckle
    faces, count = ops.scene_mesh_faces(speckle, a.n, a.H, a.W, a.dev)
    faces = faces[:int(count)].cpu().numpy()
    _, fc, _, cf = mc.components(faces, a.n * a.H * a.W)
    keep = mc.keep_components(cf, min_faces=20)
    assert len(cf) > 50 and 0 < keep.sum() < len(cf)
    sel = mc.select(np.zeros((a.n * a.H * a.W, 3), np.float32), faces, keep[fc])
    sheets = dict(as_pointcloud=False, is_msk=True)
    path = scene_export.get_3D_model_from_scene(out, True, a, save_name="sheets", min_component_faces=20, **sheets)
    _holds(path, len(sel[0]), len(sel[3]))
    _holds(scene_export.get_3D_model_from_scene(out, True, a, save_name="all", **sheets), a.n * a.H * a.W, len(faces))
    assert a.tsdf is None
    with pytest.raises(ValueError, match="remove pieces of a mesh"):
        scene_export.get_3D_model_from_scene(out, True, a, as_pointcloud=True, min_component_faces=20)


def test_defaults_write_the_same_bytes(dev, floater, tmp_path):
    from geo4d_amd import scene_export
    none = dict(min_component_faces=None, min_component_fraction=None)
    a = _synthetic_aligner(dev, floater)
    a.imgs = torch.rand((a.n, a.H, a.W, 3), generator=torch.Generator().manual_seed(4)).to(dev)
    for i, kw in enumerate((dict(as_pointcloud=True), dict(as_pointcloud=False), dict(as_pointcloud=False, tsdf_mesh=True, motion="static"))):
        plain = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name=f"plain{i}", **kw)
        named = scene_export.get_3D_model_from_scene(str(tmp_path), True, a, save_name=f"named{i}", **kw, **none)
        assert open(plain, "rb").read() == open(named, "rb").read(), kw
    assert "components" not in a.tsdf
    video = torch.rand((1, 3, a.n, a.H, a.W), generator=torch.Generator().manual_seed(6)) * 2 - 1
    base = scene_export.save_scene(a, str(tmp_path / "base"), "seq", imgs=video, tsdf_mesh_static=True)
    named = scene_export.save_scene(a, str(tmp_path / "named"), "seq", imgs=video, tsdf_mesh_static=True, **none)
    names = sorted(os.listdir(base))
    assert sorted(os.listdir(named)) == names and "seq_static_tsdf_mesh.glb" in names
    for f in names:
        assert open(os.path.join(base, f), "rb").read() == open(os.path.join(named, f), "rb").read(), f
    # given, they reach the mesh's glb and no other file
    raw = dict(a.tsdf)
    clean = scene_export.save_scene(a, str(tmp_path / "clean"), "seq", imgs=video, tsdf_mesh_static=True, min_component_fraction=0.05)
    assert sorted(os.listdir(clean)) == names and a.tsdf["removed_faces"] > 0
    for f in names:
        same = open(os.path.join(base, f), "rb").read() == open(os.path.join(clean, f), "rb").read()
        assert same == (f != "seq_static_tsdf_mesh.glb"), f
    _holds(os.path.join(clean, "seq_static_tsdf_mesh.glb"), len(a.tsdf["vertices"]), len(a.tsdf["faces"]))
    assert len(a.tsdf["faces"]) == len(raw["faces"]) - a.tsdf["removed_faces"]


def test_render_scene_draws_no_removed_triangle(dev, aligner):
    from geo4d_amd import render
    a = aligner
    before = render.render_scene(a, "cameras", is_msk=False, static_mesh=True)
    raw = dict(a.tsdf)
    (ref_v, _, _, ref_f, _), cf, keep = _selection_of(raw, "vertex_rgba", "vertex_weight", min_fraction=0.05)
    fc = mc.components(raw["faces"].cpu().numpy(), len(raw["vertices"]))[1]
    removed = ~np.append(keep, False)[fc]                                            # per old face
    old_face = before["face"].cpu().numpy()
    showed = (old_face >= 0) & removed[np.maximum(old_face, 0)]
    assert removed.sum() > 0 and showed.sum() > 0                                    # the floater is in the picture
    a.tsdf = None
    after = render.render_scene(a, "cameras", is_msk=False, static_mesh=True, min_component_fraction=0.05)
    assert a.tsdf["removed_faces"] == removed.sum() and np.array_equal(a.tsdf["faces"].cpu().numpy(), ref_f)
    new_face = after["face"].cpu().numpy()
    assert new_face.max() < len(ref_f)
    old_row = np.flatnonzero(~removed)[np.maximum(new_face, 0)]                      # the drawn triangles as rows of the unfiltered mesh
    assert not removed[old_row][new_face >= 0].any()
    drawn = ref_v[ref_f[np.unique(new_face[new_face >= 0])].reshape(-1)]
    assert (mc.off_wall(drawn) <= 0.5).all()
    untouched = ~showed                                                              # where the floater was not in front, nothing changes
    assert np.array_equal(old_row[untouched & (old_face >= 0)], old_face[untouched & (old_face >= 0)])
    assert torch.equal(after["depth"][torch.from_numpy(untouched).to(dev)], before["depth"][torch.from_numpy(untouched).to(dev)])
    again = render.render_scene(a, "cameras", is_msk=False, static_mesh=True)        # reuses scene.tsdf as found: the filtered mesh
    assert torch.equal(again["face"], after["face"])
    with pytest.raises(ValueError, match="pass static_mesh"):
        render.render_scene(a, "cameras", is_msk=False, min_component_faces=5)


def test_render_mesh_with_a_face_mask_equals_the_selected_mesh(dev, floater):
    from geo4d_amd import mesh, render
    raw = _tsdf_mesh(dev, floater)
    labels = mesh.mesh_components(raw["faces"], len(raw["vertices"]))
    assert labels["components"] == 2
    keep = labels["face_component"] == 0
    sel = mesh.remove_small_components(raw["vertices"], raw["faces"], keep_largest=1, rgba=raw["rgba"])
    assert sel["removed_faces"] == int((~keep).sum()) == 48
    c2w, K = torch.from_numpy(floater["cams2world"][:4]), torch.from_numpy(floater["K"][:4])
    size = (floater["H"], floater["W"])
    masked = render.render_mesh(raw["vertices"], raw["faces"], c2w, K, size, colors=raw["rgba"], face_mask=keep, shade=0.3)
    chosen = render.render_mesh(sel["vertices"], sel["faces"], c2w, K, size, colors=sel["rgba"], shade=0.3)
    whole = render.render_mesh(raw["vertices"], raw["faces"], c2w, K, size, colors=raw["rgba"], shade=0.3)
    assert torch.equal(masked["depth"], chosen["depth"]) and torch.equal(masked["rgb"], chosen["rgb"])
    assert not torch.equal(whole["depth"], chosen["depth"]) and int((chosen["face"] >= 0).sum()) > 1000
