"""The mesh-components rule without a GPU: its numpy restatement (tests/mesh_components_restatement.py) against scipy's connected
components and hand-written expectations, the properties the rule promises, geo4d_amd.mesh's keep rule on size arrays alone, a TSDF
scene with a planted floater built with the TSDF restatements, and the host side of the HIP path (the geo4d_mesh_* symbols): ABI
agreement, host-side argument validation and the Python errors. tests/test_mesh_components_gpu.py asserts the device against the same
restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_components_restatement as mc
import tsdf_mesh_restatement as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geo4d_mesh_components_hook", "geo4d_mesh_components_flatten", "geo4d_mesh_components_count", "geo4d_mesh_select_mark",
           "geo4d_mesh_select_gather")
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31

# (name, faces, Nv, face_mask, vertex_component, face_component, component_vertices, component_faces)
HAND_CASES = [
    ("two disjoint triangles", [[0, 1, 2], [3, 4, 5]], 6, None, [0, 0, 0, 1, 1, 1], [0, 1], [3, 3], [1, 1]),
    ("two triangles sharing one vertex", [[0, 1, 2], [2, 3, 4]], 5, None, [0, 0, 0, 0, 0], [0, 0], [5], [2]),
    ("two triangles sharing an edge", [[3, 1, 2], [2, 1, 0]], 4, None, [0, 0, 0, 0], [0, 0], [4], [2]),
    ("repeated indices", [[4, 4, 1], [2, 2, 2], [0, 3, 3]], 5, None, [0, 1, 2, 0, 1], [1, 2, 0], [2, 2, 1], [1, 1, 1]),
    ("indices -1 and Nv", [[0, 1, -1], [1, 2, 4], [2, 3, 3], [4, 0, 0]], 4, None, [-1, -1, 0, 0], [-1, -1, 0, -1], [2], [1]),
    ("a masked face", [[0, 1, 2], [2, 3, 4], [4, 5, 6]], 7, [1, 0, 1], [0, 0, 0, -1, 1, 1, 1], [0, -1, 1], [3, 3], [1, 1]),
    ("an untouched vertex between touched ones", [[0, 2, 4], [5, 6, 6]], 7, None, [0, -1, 0, -1, 0, 1, 1], [0, 1], [3, 2], [1, 1]),
]


# ---- the meshes both test files use ------------------------------------------------------------------------------------------------------
def random_mesh(rng, Nv, T):
    return rng.integers(0, Nv, size=(T, 3)).astype(np.int32)


def percolation_mesh():
    """Nv = 3000 with 1100 random faces, near the threshold where one large piece forms beside hundreds of small ones. 1100 faces of
    three different random vertices are far above it (two links per face: measured 58 components, one of 1010 faces), so 800 of the
    faces, at random rows, repeat their second index, (a, b, b), and are one link each: 2 * 800 + 6 * 300 = 3400 link ends on 3000
    vertices, 1.13 per vertex. Seed 11: 320 components, the largest of 407 faces."""
    rng = np.random.default_rng(11)
    f = random_mesh(rng, 3000, 1100)
    f[300:, 2] = f[300:, 1]
    return f[rng.permutation(1100)], 3000


def strip(n, order):
    """n triangles (i, i + 1, i + 2) over n + 2 vertices named ascending, descending or at random: long paths and every link direction."""
    ids = dict(ascending=np.arange(n + 2), descending=np.arange(n + 2)[::-1], random=np.random.default_rng(3).permutation(n + 2))[order]
    return np.stack([ids[:-2], ids[1:-1], ids[2:]], 1).astype(np.int32), n + 2


def fan(n, hub_high):
    """n triangles round one vertex, the highest or the lowest index: every thread contends on one root."""
    hub = n + 1 if hub_high else 0
    rim = np.arange(1, n + 2) - (1 if hub_high else 0)
    return np.stack([np.full(n, hub), rim[:-1], rim[1:]], 1).astype(np.int32), n + 2


def islands_and_strip():
    """1000 disjoint triangles and one 3000-face strip behind them: many roots beside one heavy counter."""
    tri = np.arange(3000).reshape(1000, 3)
    s, n = strip(3000, "ascending")
    return np.concatenate([tri, s + 3000]).astype(np.int32), 3000 + n


def bad_index_mesh():
    """A strip with faces naming -1, Nv, INT32_MAX and INT32_MIN mixed in."""
    f, Nv = strip(300, "random")
    f = f.copy()
    rng = np.random.default_rng(4)
    rows, cols = rng.choice(300, 40, replace=False), rng.integers(0, 3, 40)
    f[rows, cols] = np.array([-1, Nv, INT_MAX, INT_MIN], dtype=np.int64)[np.arange(40) % 4].astype(np.int32)
    return f, Nv


def scipy_components(faces, Nv, face_mask=None):
    """(labels [Nv] with -1 for untouched vertices, in ascending order of smallest vertex; face labels) from scipy's connected components."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f, ok = mc.valid_faces(faces, Nv, face_mask)
    f = f[ok]
    rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    _, lab = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(Nv, Nv)), directed=False)
    touched = np.zeros(Nv, dtype=bool)
    touched[f.reshape(-1)] = True
    first = {}
    for v in np.flatnonzero(touched):                                  # ascending: a label's first vertex is its smallest
        first.setdefault(lab[v], len(first))
    vertex = np.array([first[lab[v]] if touched[v] else -1 for v in range(Nv)], dtype=np.int32).reshape(Nv)
    face = np.full(len(ok), -1, dtype=np.int32)
    face[ok] = vertex[f[:, 0]]
    return vertex, face


def _agrees_with_scipy(faces, Nv, mask=None):
    vc, fc, cv, cf = mc.components(faces, Nv, mask)
    sv, sf = scipy_components(faces, Nv, mask)
    assert np.array_equal(vc, sv) and np.array_equal(fc, sf)
    C = int(vc.max()) + 1 if (vc >= 0).any() else 0
    assert len(cv) == len(cf) == C
    assert np.array_equal(cv, np.bincount(sv[sv >= 0], minlength=C)) and np.array_equal(cf, np.bincount(sf[sf >= 0], minlength=C))
    return cv, cf


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_restatement_agrees_with_scipy_on_random_meshes():
    rng = np.random.default_rng(0)
    for k in range(50):
        Nv, T = int(rng.integers(1, 401)), int(rng.integers(0, 501))
        faces = rng.integers(-1, Nv + 1, size=(T, 3)) if k % 3 == 0 else random_mesh(rng, Nv, T)
        _agrees_with_scipy(faces, Nv, rng.integers(0, 2, T) if k % 4 == 0 else None)


def test_restatement_agrees_with_scipy_near_the_percolation_threshold():
    faces, Nv = percolation_mesh()
    cv, cf = _agrees_with_scipy(faces, Nv)
    print(f"[mesh components percolation] {len(cf)} components, largest {cf.max()} faces, {(cf == 1).sum()} single faces")
    assert len(cf) > 100 and cf.max() > 100 and (len(cf), int(cf.max())) == (320, 407)


@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_hand_cases(case):
    _, faces, Nv, mask, vc, fc, cv, cf = case
    got = mc.components(faces, Nv, mask)
    for g, want in zip(got, (vc, fc, cv, cf)):
        assert g.dtype == np.int32 and g.tolist() == want
    _agrees_with_scipy(faces, Nv, mask)


def test_bad_indices_of_every_kind_are_no_faces():
    faces, Nv = bad_index_mesh()
    bad = ((faces < 0) | (faces >= Nv)).any(1)
    assert bad.sum() == 40 and set(faces[bad][(faces[bad] < 0) | (faces[bad] >= Nv)].tolist()) == {-1, Nv, INT_MAX, INT_MIN}
    vc, fc, cv, cf = mc.components(faces, Nv)
    assert (fc[bad] == -1).all() and (fc[~bad] >= 0).all() and len(cf) > 1 and cf.sum() == 260
    _agrees_with_scipy(faces, Nv)


def test_face_order_changes_nothing_but_the_order_of_face_component():
    faces, Nv = percolation_mesh()
    mask = np.random.default_rng(1).random(len(faces)) < 0.9
    vc, fc, cv, cf = mc.components(faces, Nv, mask)
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(len(faces))
        got = mc.components(faces[perm], Nv, mask[perm])
        assert np.array_equal(got[0], vc) and np.array_equal(got[1], fc[perm]) and np.array_equal(got[2], cv) and np.array_equal(got[3], cf)


def test_selection_keeps_order_references_every_vertex_and_is_idempotent():
    faces, Nv = percolation_mesh()
    rng = np.random.default_rng(2)
    vertices = rng.random((Nv, 3)).astype(np.float32)
    rgba, weight = rng.integers(0, 256, (Nv, 4), dtype=np.uint8), rng.random(Nv).astype(np.float32)
    _, fc, _, cf = mc.components(faces, Nv)
    keep = (fc % 2 == 0)
    v, c, w, f, idx = mc.select(vertices, faces, keep, rgba, weight)
    assert f.dtype == np.int32 and idx.dtype == np.int32 and len(f) == keep.sum() and len(v) == len(idx) == len(c) == len(w)
    assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)   # in range, every vertex referenced
    assert (np.diff(idx) > 0).all() and np.array_equal(idx[f], faces[keep])          # vertex order kept, face order kept, same triangles
    assert np.array_equal(v, vertices[idx]) and np.array_equal(c, rgba[idx]) and np.array_equal(w, weight[idx])
    again = mc.select(v, f, np.ones(len(f), bool), c, w)
    for a, b in zip(again[:4], (v, c, w, f)):
        assert np.array_equal(a, b)
    assert np.array_equal(again[4], np.arange(len(v)))
    # a kept face with a bad index is no face; nothing kept gives nothing
    bad, Nb = bad_index_mesh()
    out = mc.select(np.zeros((Nb, 3), np.float32), bad, np.ones(len(bad), bool))
    assert len(out[3]) == 260 and out[1] is None and out[2] is None
    none = mc.select(vertices, faces, np.zeros(len(faces), bool), rgba)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 4) and none[3].shape == (0, 3) and none[4].shape == (0,)


# ---- the keep rule -----------------------------------------------------------------------------------------------------------------------
def test_keep_rule_on_the_sizes_alone():
    from fractions import Fraction
    from geo4d_amd.mesh import keep_rule
    assert keep_rule([4, 16], min_fraction=0.25) == [True, True]                    # exactly at the boundary: 4 * 4 >= 1 * 16
    assert keep_rule([3, 16], min_fraction=0.25) == [False, True]
    assert keep_rule([4, 16], min_fraction=float(np.nextafter(0.25, 1))) == [False, True]
    assert keep_rule([1, 3], min_fraction=Fraction(1, 3)) == [True, True]           # no float rounds a third
    assert keep_rule([1, 3], min_fraction=1 / 3) == [True, True] and 1 / 3 < Fraction(1, 3)
    assert keep_rule([10 ** 9, 2 * 10 ** 9 - 1], min_fraction=0.5) == [True, True]
    assert keep_rule([10 ** 9 - 1, 2 * 10 ** 9 - 1], min_fraction=0.5) == [False, True]
    assert keep_rule([5, 9, 2], min_fraction=1) == [False, True, False] and keep_rule([9, 5, 9], min_fraction=1.0) == [True, False, True]
    assert keep_rule([5, 9, 2], min_faces=5) == [True, True, False] and keep_rule([5, 9, 2], min_faces=1) == [True] * 3
    assert keep_rule([7, 9, 7, 7], keep_largest=2) == [True, True, False, False]   # ties go to the lower id
    assert keep_rule([7, 9, 7, 7], keep_largest=3) == [True, True, True, False] and keep_rule([7, 9], keep_largest=5) == [True, True]
    assert keep_rule([7, 9, 7, 7], keep_largest=3, min_faces=8) == [False, True, False, False]
    assert keep_rule([2, 40, 3, 40, 1], min_faces=2, min_fraction=0.05, keep_largest=3) == [False, True, True, True, False]
    assert keep_rule([], min_faces=3, min_fraction=0.5, keep_largest=1) == [] and keep_rule([3, 1]) == [True, True]
    assert keep_rule(np.array([4, 16], dtype=np.int32), min_fraction=0.25) == [True, True]
    for sizes, kw in [([4, 16], dict(min_fraction=0.25)), ([7, 9, 7, 7], dict(keep_largest=2)), ([2, 40, 3], dict(min_faces=3, min_fraction=0.05))]:
        assert keep_rule(sizes, **kw) == mc.keep_components(sizes, **kw).tolist()
    for kw in [dict(min_faces=0), dict(min_faces=-3), dict(min_faces=2.5), dict(min_faces=True), dict(min_fraction=0), dict(min_fraction=0.0),
               dict(min_fraction=-0.1), dict(min_fraction=1.0001), dict(min_fraction=float("nan")), dict(min_fraction="half"),
               dict(keep_largest=0), dict(keep_largest=-1), dict(keep_largest=1.5)]:
        with pytest.raises(ValueError, match=next(iter(kw))):
            keep_rule([1, 2], **kw)


# ---- the TSDF's meshes -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floater():
    return mc.floater_scene()


def test_floater_scene_loses_its_plate_and_nothing_else(floater):
    """Measured: V = 994, T = 1790 in 2 components of 1742 (the wall) and 48 faces (the plate, 0.98 in front of the wall: 40 vertices,
    34 of them more than 0.5 from the wall, the other 6 on the rim that the depth step behind the plate's silhouette pulls back); 0.05
    of the wall's faces is 87.1, so the plate goes and the wall stays."""
    from geo4d_amd.mesh import keep_rule
    m = floater["mesh"]
    V, T = len(m["vertices"]), len(m["faces"])
    vc, fc, cv, cf = mc.components(m["faces"], V)
    far = mc.off_wall(m["vertices"]) > 0.5
    print(f"[mesh components floater] V {V}, T {T}, components {cf.tolist()} faces / {cv.tolist()} vertices, {far.sum()} vertices far from the wall")
    assert (m["weight"][far] >= 4).all()                                             # the plate is seen by at least min_weight cameras
    assert len(cf) == 2 and cf.tolist() == [1742, 48] and cv.tolist() == [954, 40]
    assert far.sum() == 34 and (vc[far] == 1).all() and not far[vc == 0].any()       # the largest component is the wall
    assert mc.off_wall([0.0, -0.8, 3.0])[0] > 4 * floater["voxel"]                   # the plate's plane: detached by more than the truncation
    keep = keep_rule(cf, min_fraction=0.05)
    assert keep == [True, False]
    v, c, w, f, idx = mc.select(m["vertices"], m["faces"], np.array(keep)[fc], m["rgba"], m["weight"])
    assert T - len(f) == 48 and V - len(v) == 40 and len(np.unique(f)) == len(v)
    assert (mc.off_wall(v) <= 0.5).all()
    assert mc.components(f, len(v))[3].tolist() == [1742]
    # an implementation that returns the mesh unfiltered fails here
    assert not (mc.off_wall(m["vertices"]) <= 0.5).all()


def test_the_tsdf_test_blocks():
    m = tm.mesh(*tm.sphere_block((0, 0, 0), colours=True), 1.0, 4.0)
    vc, fc, cv, cf = mc.components(m["faces"], len(m["vertices"]))
    assert cv.tolist() == [74] and cf.tolist() == [144] and (vc == 0).all() and (fc == 0).all()
    m = tm.mesh(*tm.random_block(8, 6, holes=0.03, weak=0.03), 0.1, 4.0)
    vc, fc, cv, cf = mc.components(m["faces"], len(m["vertices"]))
    assert (len(m["vertices"]), len(m["faces"])) == (230, 392) and cv.tolist() == [230] and cf.tolist() == [392]


# ---- ABI and host ------------------------------------------------------------------------------------------------------------------------
def test_symbols_agree_between_header_binding_and_library():
    from geo4d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geo4d_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.geo4d_abi_version() == _lib.ABI_VERSION == 9 == int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1))


def test_bad_arguments_are_refused_on_the_host():
    """Every refusal is -EINVAL with the function's name in the message and comes before any device work: the pointers below are not
    device memory."""
    from geo4d_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    big = 1 << 31

    def hook(faces=p, T=10, Nv=10, mask=None, parent=p, touched=p):
        return lib.geo4d_mesh_components_hook(faces, T, Nv, mask, parent, touched, None)

    for kw in [dict(faces=None), dict(parent=None), dict(touched=None), dict(T=-1), dict(Nv=-1), dict(T=big), dict(Nv=big)]:
        assert hook(**kw) == -22 and b"mesh_components_hook" in lib.geo4d_last_error(), kw

    def flatten(parent=p, touched=p, Nv=10, root=p, is_root=p):
        return lib.geo4d_mesh_components_flatten(parent, touched, Nv, root, is_root, None)

    for kw in [dict(parent=None), dict(touched=None), dict(root=None), dict(is_root=None), dict(Nv=-1), dict(Nv=big)]:
        assert flatten(**kw) == -22 and b"mesh_components_flatten" in lib.geo4d_last_error(), kw

    def count(faces=p, T=10, Nv=10, mask=None, root=p, first=p, C=3, vc=p, fc=p, cv=p, cf=p):
        return lib.geo4d_mesh_components_count(faces, T, Nv, mask, root, first, C, vc, fc, cv, cf, None)

    for kw in [dict(faces=None), dict(root=None), dict(first=None), dict(vc=None), dict(fc=None), dict(cv=None), dict(cf=None), dict(T=-1),
               dict(Nv=-1), dict(T=big), dict(Nv=big), dict(C=-1), dict(C=11)]:
        assert count(**kw) == -22 and b"mesh_components_count" in lib.geo4d_last_error(), kw

    def mark(faces=p, T=10, Nv=10, keep=p, keep_vertex=p, kept=p):
        return lib.geo4d_mesh_select_mark(faces, T, Nv, keep, keep_vertex, kept, None)

    for kw in [dict(faces=None), dict(keep=None), dict(keep_vertex=None), dict(kept=None), dict(T=-1), dict(Nv=-1), dict(T=big), dict(Nv=big)]:
        assert mark(**kw) == -22 and b"mesh_select_mark" in lib.geo4d_last_error(), kw

    def gather(vertices=p, rgba=None, weight=None, faces=p, T=10, Nv=10, keep_vertex=p, kept=p, first_vertex=p, first_face=p, V=5, F=5, out=p,
               rgba_out=None, weight_out=None, faces_out=p, index=p):
        return lib.geo4d_mesh_select_gather(vertices, rgba, weight, faces, T, Nv, keep_vertex, kept, first_vertex, first_face, V, F, out,
                                            rgba_out, weight_out, faces_out, index, None)

    for kw in [dict(vertices=None), dict(faces=None), dict(keep_vertex=None), dict(kept=None), dict(first_vertex=None), dict(first_face=None),
               dict(out=None), dict(faces_out=None), dict(index=None), dict(rgba_out=p), dict(weight_out=p), dict(T=-1), dict(Nv=-1),
               dict(T=big), dict(Nv=big), dict(V=-1), dict(V=11), dict(F=-1), dict(F=11)]:
        assert gather(**kw) == -22 and b"mesh_select_gather" in lib.geo4d_last_error(), kw
    # nothing to do is no error and no launch
    assert hook(T=0) == 0 and hook(Nv=0) == 0 and flatten(Nv=0) == 0 and count(T=0) == 0 and count(Nv=0, C=0) == 0 and count(C=0) == 0
    assert mark(T=0) == 0 and mark(Nv=0) == 0 and gather(V=0, F=0) == 0 and gather(T=0, F=0) == 0 and gather(Nv=0, V=0) == 0


# ---- Python errors -----------------------------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_any_device_work(tmp_path):
    import inspect
    import torch
    from geo4d_amd import _lib, mesh, ops, render, tsdf
    from geo4d_amd.scene_export import get_3D_model_from_scene
    faces, vertices = torch.tensor([[0, 1, 2]], dtype=torch.int32), torch.zeros((3, 3))
    with pytest.raises(_lib.Geo4DNativeError, match="no CPU fallback"):
        ops.mesh_components(faces, 3)
    with pytest.raises(_lib.Geo4DNativeError, match="no CPU fallback"):
        ops.mesh_select(vertices, faces, torch.ones(1, dtype=torch.bool))
    with pytest.raises(_lib.Geo4DNativeError, match="no CPU fallback"):
        mesh.remove_small_components(vertices, faces, min_faces=2)
    for kw in (dict(min_faces=0), dict(min_fraction=0.0), dict(min_fraction=1.5), dict(keep_largest=0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            mesh.remove_small_components(vertices, faces, **kw)
    same = mesh.remove_small_components(vertices, faces)                             # no constraint: the inputs' own tensors, no launch
    assert same["vertices"] is vertices and same["faces"] is faces and same["rgba"] is None and same["removed_faces"] == 0
    for kw in (dict(min_component_faces=5), dict(min_component_fraction=0.1)):
        for more in (dict(as_pointcloud=True), dict(as_pointcloud=True, fuse_voxel=0.1), dict(as_pointcloud=True, tsdf_voxel=0.1)):
            with pytest.raises(ValueError, match="min_component_faces / min_component_fraction remove pieces of a mesh"):
                get_3D_model_from_scene(str(tmp_path), True, None, **kw, **more)
        assert get_3D_model_from_scene(str(tmp_path), True, None, as_pointcloud=False, **kw) is None
        assert get_3D_model_from_scene(str(tmp_path), True, None, as_pointcloud=False, tsdf_mesh=True, **kw) is None
        with pytest.raises(ValueError, match="pass mesh=True"):
            tsdf.tsdf_scene(object(), **kw)
    with pytest.raises(ValueError, match="min_fraction must lie in"):
        get_3D_model_from_scene(str(tmp_path), True, None, as_pointcloud=False, min_component_fraction=2)
    with pytest.raises(ValueError, match="min_faces must be an integer >= 1"):
        tsdf.tsdf_scene(object(), mesh=True, min_component_faces=0)
    assert os.listdir(tmp_path) == []
    for fn in (tsdf.tsdf_mesh, tsdf.tsdf_scene, get_3D_model_from_scene, render.render_scene):
        par = inspect.signature(fn).parameters
        assert par["min_component_faces"].default is None and par["min_component_fraction"].default is None, fn
