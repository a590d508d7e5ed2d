"""The surface-nets rule without a GPU: its numpy restatement (tests/tsdf_mesh_restatement.py) on the synthetic scene of
tests/tsdf_restatement.py (what the mesh is worth, and the properties the rule promises) and on hand-made fields, and the host side of
the HIP path (the geo4d_tsdf_mesh_* symbols, geo4d_amd/scene_export.py): ABI agreement, host-side argument validation and the Python
errors. tests/test_tsdf_mesh_gpu.py asserts the device against the same restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

import tsdf_mesh_restatement as tm
import tsdf_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geo4d_tsdf_mesh_cells", "geo4d_tsdf_mesh_count", "geo4d_tsdf_mesh_vertices", "geo4d_tsdf_mesh_faces")


def _scene(noise):
    s = tr.static_scene(noise)
    o = s["out"]
    s["mesh"] = tm.mesh(o["K"], o["f"], o["Wt"], o["col"], s["voxel"], tr.DEFAULTS["min_weight"])
    return s


@pytest.fixture(scope="module")
def clean():
    return _scene(0.0)


@pytest.fixture(scope="module")
def noisy():
    return _scene(0.02)


def off_plane(p):
    """Distance of points [N, 3] to the wall -0.2 x + z = 4."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return np.abs(-0.2 * p[:, 0] + p[:, 2] - 4.0) / np.sqrt(1.04)


def rms_near(p):
    """(RMS distance to the wall over the points within 0.5 of it, how many are farther)."""
    d = off_plane(p)
    return float(np.sqrt((d[d < 0.5] ** 2).mean())), int((d >= 0.5).sum())


def normals(mesh):
    v, fa = mesh["vertices"].astype(np.float64), mesh["faces"]
    return np.cross(v[fa[:, 1]] - v[fa[:, 0]], v[fa[:, 2]] - v[fa[:, 0]])


def facing_away(s):
    """The triangles whose normal does not point to the mean camera centre."""
    v, fa = s["mesh"]["vertices"].astype(np.float64), s["mesh"]["faces"]
    cam = s["centres"].astype(np.float64).mean(0)
    return int(((normals(s["mesh"]) * (cam - v[fa[:, 0]])).sum(1) <= 0).sum())


# ---- what the mesh is worth ----------------------------------------------------------------------------------------------------------------
def test_clean_wall_is_one_oriented_sheet(clean):
    """Measured: 10 950 voxels, V = 1 016, T = 1 880, vertex RMS 0.0013 against 0.0017 for the TSDF points."""
    m = clean["mesh"]
    got, far = rms_near(m["vertices"])
    pts, _ = rms_near(clean["out"]["points"])
    directed, undirected = tm.edge_counts(m["faces"])
    print(f"[tsdf mesh clean] {len(clean['out']['K'])} voxels -> V {len(m['vertices'])}, T {len(m['faces'])}; RMS {got:.4f} against {pts:.4f} points, "
          f"{far} far, {facing_away(clean)} facing away, {(undirected > 2).sum()} edges in more than two triangles")
    assert len(clean["out"]["K"]) == 10950 and len(m["vertices"]) == 1016 and len(m["faces"]) == 1880
    assert got <= pts
    assert far == 0 and (off_plane(m["vertices"]) <= 0.5).all()
    assert (np.linalg.norm(normals(m), axis=1) > 0).all()                           # no degenerate triangle
    assert facing_away(clean) == 0
    assert (directed == 1).all() and (undirected <= 2).all()


def test_noisy_wall_is_smoother_than_the_points(noisy):
    """Measured: V = 1 226, T = 2 306, RMS 0.0171 against 0.0250 for the points and 0.0789 raw, 39 triangles facing away, 21 of 3 531
    edges in more than two triangles, 0 vertices far."""
    m = noisy["mesh"]
    got, far = rms_near(m["vertices"])
    pts, _ = rms_near(noisy["out"]["points"])
    raw, _ = rms_near(noisy["pts3d"][noisy["static"]])
    _, undirected = tm.edge_counts(m["faces"])
    away, crowded = facing_away(noisy), int((undirected > 2).sum())
    print(f"[tsdf mesh noisy] V {len(m['vertices'])}, T {len(m['faces'])}; RMS {got:.4f} against {pts:.4f} points and {raw:.4f} raw, {far} far, "
          f"{away} facing away, {crowded} of {len(undirected)} edges in more than two triangles")
    assert len(m["vertices"]) == 1226 and len(m["faces"]) == 2306
    assert got <= pts and got <= 0.5 * raw
    assert away <= 0.05 * len(m["faces"]) and crowded <= 0.02 * len(undirected)
    assert far == 0


# ---- properties of the rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["clean", "noisy"])
def test_properties_of_the_rule(which, clean, noisy):
    s = dict(clean=clean, noisy=noisy)[which]
    m, out, v = s["mesh"], s["out"], np.float32(s["voxel"])
    V, T, Q = len(m["vertices"]), len(m["faces"]), len(m["quad_m"])
    assert m["vertices"].dtype == np.float32 and m["faces"].dtype == np.int32 and m["rgba"].shape == (V, 4) and m["weight"].shape == (V,)
    assert m["faces"].min() >= 0 and m["faces"].max() < V and len(np.unique(m["faces"])) == V   # in range, every vertex referenced
    X0 = tr.voxel_centres(out["K"][m["cell"]], v)
    upper = X0 + v
    assert (m["vertices"] >= X0).all() and (m["vertices"] <= upper + np.spacing(upper)).all()   # inside the closed cube of its cell
    assert (np.diff(out["K"][m["cell"]]) > 0).all()                                 # vertex rows ascend in cell key
    assert (np.diff(m["quad_m"] * 3 + m["quad_axis"]) > 0).all()                    # quads ascend in (m, a)
    assert T == 2 * Q and Q <= len(out["points"]) and len(out["points"]) == (1095 if which == "clean" else 1389)
    assert m["complete"][m["cell"]].all() and m["crossing"][m["cell"]].all() and (m["weight"] >= 4).all() and (m["rgba"][:, 3] == 255).all()
    unused = int((m["crossing"] & ~m["used"]).sum())                                # a sign change, and no quad: no vertex
    assert unused == (0 if which == "clean" else 16) and int(m["crossing"].sum()) == V + unused
    # every quad is a sign change the points' extraction found as well
    pairs = set(zip(out["m"].tolist(), out["axis"].tolist()))
    assert all(p in pairs for p in zip(m["quad_m"].tolist(), m["quad_axis"].tolist()))


@pytest.mark.parametrize("origin", [0, (1 << 20) - 6, -(1 << 20) + 1])
def test_sphere_block_is_a_closed_surface_wherever_it_lies(origin):
    """A 6^3 block around a sphere: 216 voxels, 117 complete cells, 74 vertices, 144 triangles and every edge in exactly two
    triangles. The same at the upper end of the grid, where + E_a carries out of a full field, and at the lower end, where - E_a gives the
    field 0: neither may find a neighbour."""
    K, f, Wt, col = tm.sphere_block((origin,) * 3, colours=True)
    cells = tr.cells_of(K)
    assert len(K) == 216 and (np.diff(K) > 0).all() and cells.min() == origin and cells.max() == origin + 5
    m = tm.mesh(K, f, Wt, col, 1.0, 4.0)
    directed, undirected = tm.edge_counts(m["faces"])
    assert int(m["complete"].sum()) == 117 and len(m["vertices"]) == 74 and len(m["faces"]) == 144
    assert (directed == 1).all() and (undirected == 2).all()
    # outward: the inside is negative
    v, fa = m["vertices"].astype(np.float64), m["faces"]
    middle = origin + 3.0                                                            # voxel 1: centres at cell + 0.5
    assert ((normals(m) * (v[fa[:, 0]] - middle)).sum(1) > 0).all()
    base = tm.mesh(*tm.sphere_block((0, 0, 0), colours=True), 1.0, 4.0)
    assert np.array_equal(m["faces"], base["faces"]) and np.array_equal(m["rgba"], base["rgba"]) and np.array_equal(m["cell"], base["cell"])


def test_hand_made_fields():
    """The other fields tests/test_tsdf_mesh_gpu.py runs on the device, and what they are there for."""
    m = tm.mesh(*tm.plane_block(), 0.1, 4.0)
    directed, undirected = tm.edge_counts(m["faces"])
    assert len(m["faces"]) == 18 and (directed == 1).all() and (undirected == 1).sum() == 12      # an open boundary
    K, f, Wt, col = tm.random_block(5, 4)
    m = tm.mesh(K, f, Wt, col, 0.1, 4.0)
    _, undirected = tm.edge_counts(m["faces"])
    assert len(m["faces"]) == 108 and (undirected > 2).sum() == 15 and (m["crossing"] & ~m["used"]).sum() == 1
    for M in (0, 1, 257, 513):
        m = tm.mesh(*tm.slab(M), 0.1, 4.0)
        assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3) and m["weight"].shape == (0,) and not m["complete"].any()
    K8, _ = tm.block_keys((2, 2, 2))
    m = tm.mesh(K8, np.full(8, 0.25, np.float32), np.full(8, 8, np.float32), None, 0.1, 4.0)
    assert m["complete"].tolist() == [True] + [False] * 7 and m["faces"].shape == (0, 3) and m["rgba"] is None


# ---- ABI and host ------------------------------------------------------------------------------------------------------------------------
def test_mesh_symbols_agree_between_header_binding_and_library():
    from geo4d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geo4d_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
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
    nan, inf = float("nan"), float("inf")

    def cells(keys=p, M=10, f=p, wt=p, min_weight=4.0, complete=p):
        return lib.geo4d_tsdf_mesh_cells(keys, M, f, wt, min_weight, complete, None)

    for kw in [dict(keys=None), dict(f=None), dict(wt=None), dict(complete=None), dict(M=-1), dict(M=1 << 31), dict(min_weight=0.0),
               dict(min_weight=-1.0), dict(min_weight=nan)]:
        assert cells(**kw) == -22 and b"tsdf_mesh_cells" in lib.geo4d_last_error(), kw

    def count(keys=p, M=10, complete=p, counts=p, used=p):
        return lib.geo4d_tsdf_mesh_count(keys, M, complete, counts, used, None)

    for kw in [dict(keys=None), dict(complete=None), dict(counts=None), dict(used=None), dict(M=-1), dict(M=1 << 31)]:
        assert count(**kw) == -22 and b"tsdf_mesh_count" in lib.geo4d_last_error(), kw

    def vertices(keys=p, M=10, f=p, wt=p, rgba=None, used=p, first=p, V=5, voxel=0.1, out=p, rgba_out=None, w=p):
        return lib.geo4d_tsdf_mesh_vertices(keys, M, f, wt, rgba, used, first, V, voxel, out, rgba_out, w, None)

    for kw in [dict(keys=None), dict(f=None), dict(wt=None), dict(used=None), dict(first=None), dict(out=None), dict(w=None), dict(rgba_out=p),
               dict(M=-1), dict(M=1 << 31), dict(V=-1), dict(V=11), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan), dict(voxel=inf)]:
        assert vertices(**kw) == -22 and b"tsdf_mesh_vertices" in lib.geo4d_last_error(), kw
    assert vertices(voxel=nan) == -22 and b"voxel" in lib.geo4d_last_error()

    def faces(keys=p, M=10, f=p, complete=p, counts=p, first_quad=p, first_vertex=p, Q=5, V=5, out=p):
        return lib.geo4d_tsdf_mesh_faces(keys, M, f, complete, counts, first_quad, first_vertex, Q, V, out, None)

    for kw in [dict(keys=None), dict(f=None), dict(complete=None), dict(counts=None), dict(first_quad=None), dict(first_vertex=None),
               dict(out=None), dict(M=-1), dict(M=1 << 31), dict(Q=-1), dict(Q=31), dict(V=-1), dict(V=11)]:
        assert faces(**kw) == -22 and b"tsdf_mesh_faces" in lib.geo4d_last_error(), kw
    # nothing to do is no error and no launch
    assert cells(M=0) == 0 and count(M=0) == 0 and vertices(M=0, V=0) == 0 and vertices(V=0) == 0 and faces(M=0, Q=0, V=0) == 0 and faces(Q=0) == 0


# ---- Python errors -----------------------------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_any_device_work(tmp_path):
    import motion_restatement as mr
    import torch
    from geo4d_amd import _lib, ops, tsdf
    from geo4d_amd.scene_export import get_3D_model_from_scene
    kw = dict(as_pointcloud=False)
    with pytest.raises(ValueError, match="tsdf_mesh writes triangles, fuse_voxel and tsdf_voxel write points"):
        get_3D_model_from_scene(str(tmp_path), True, None, as_pointcloud=True, fuse_voxel=0.1, tsdf_mesh=True)
    with pytest.raises(ValueError, match="tsdf_mesh writes triangles, fuse_voxel and tsdf_voxel write points"):
        get_3D_model_from_scene(str(tmp_path), True, None, as_pointcloud=True, tsdf_voxel=0.1, tsdf_mesh=0.1)
    with pytest.raises(ValueError, match="tsdf_mesh.*as_pointcloud=False"):
        get_3D_model_from_scene(str(tmp_path), True, None, as_pointcloud=True, tsdf_mesh=True)
    with pytest.raises(ValueError, match="tsdf_mesh with motion='dynamic'"):
        get_3D_model_from_scene(str(tmp_path), True, None, motion="dynamic", tsdf_mesh=0.05, **kw)
    with pytest.raises(ValueError, match="tsdf_voxel.*as_pointcloud"):                # the existing refusal stays
        get_3D_model_from_scene(str(tmp_path), True, None, tsdf_voxel=True, **kw)
    assert get_3D_model_from_scene(str(tmp_path), True, None, tsdf_mesh=True, motion="static", **kw) is None
    assert get_3D_model_from_scene(str(tmp_path), True, None, tsdf_mesh=None, **kw) is None and os.listdir(tmp_path) == []
    s = mr.synthetic_scene(n=2, H=4, W=5)
    args = [torch.from_numpy(s["pts3d"]), torch.from_numpy(s["depth"]), torch.from_numpy(s["valid"]), s["cams2world"], s["K"]]
    with pytest.raises(_lib.Geo4DNativeError, match="only on a HIP device"):
        tsdf.tsdf_mesh(*args, voxel=0.1)
    for bad, msg in [(dict(voxel=0.1, trunc=9), r"trunc must be an integer number of voxels in 1\.\.8"), (dict(voxel=0.1, min_weight=0), "min_weight must be > 0"),
                     (dict(voxel=float("nan")), "voxel must be finite and > 0"), (dict(voxel=0.1, near=-1), "near must be >= 0"),
                     (dict(voxel=0.1, capacity=100), "capacity must be a power of two")]:
        with pytest.raises(ValueError, match=msg):
            tsdf.tsdf_mesh(*args, **bad)
    with pytest.raises(ValueError, match="moving part has no TSDF"):
        tsdf.tsdf_scene(object(), motion="dynamic", mesh=True)
    K, f, Wt, _ = tm.sphere_block()
    with pytest.raises(_lib.Geo4DNativeError):
        ops.tsdf_mesh_extract(torch.from_numpy(K), torch.from_numpy(f), torch.from_numpy(Wt), voxel=0.1)
    with pytest.raises(_lib.Geo4DNativeError):
        ops.tsdf_field(args[0], args[1], args[2], torch.zeros(2, 16), torch.zeros(2, 3), voxel=0.1)
