"""The corner-table rule without a GPU: its numpy restatement (tests/mesh_smooth_restatement.py) on the TSDF meshes of the synthetic
wall and on a noisy icosphere (what smoothing and the normals are worth, measured against the raw mesh), hand cases with the expected
outputs written out, the properties the table promises, and the host side of the HIP path (the geo4d_mesh_adjacency_*,
geo4d_mesh_boundary, geo4d_mesh_smooth_step and geo4d_mesh_vertex_normals symbols): ABI agreement, host-side argument validation, the
Python errors and the NORMAL attribute of the glb writer. tests/test_mesh_smooth_gpu.py asserts the device against the same
restatement."""
import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest

import mesh_smooth_restatement as ms
import tsdf_mesh_restatement as tm
import tsdf_restatement as tr
from test_mesh_components_cpu import INT_MAX, INT_MIN, bad_index_mesh, random_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geo4d_mesh_adjacency_count", "geo4d_mesh_adjacency_fill", "geo4d_mesh_adjacency_sort", "geo4d_mesh_boundary",
           "geo4d_mesh_smooth_step", "geo4d_mesh_vertex_normals")
WALL = np.array([-0.2, 0.0, 1.0]) / np.sqrt(1.04)                                   # the wall -0.2 x + z = 4 of the synthetic scene
R3 = float(np.float32(1) / np.sqrt(np.float32(3)))

SQUARE = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]
TETRA = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
FINS = [[0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, -1, 0]]
UP = [0, 0, 1]
# (name, vertices, faces, face_mask, offsets, corners, boundary, normals (None: not written out), the vertices after one free step
# with s = 0.5 (None: not written out))
HAND_CASES = [
    ("one triangle", SQUARE[:3], [[0, 1, 2]], None, [0, 1, 2, 3], [0, 1, 2], [1, 1, 1], [UP, UP, UP],
     [[0.25, 0.25, 0], [0.5, 0.25, 0], [0.25, 0.5, 0]]),
    ("two triangles sharing an edge", SQUARE, [[0, 1, 2], [2, 1, 3]], None, [0, 1, 3, 5, 6], [0, 1, 4, 2, 3, 5], [1, 1, 1, 1], [UP] * 4,
     [[0.25, 0.25, 0], [0.625, 0.375, 0], [0.375, 0.625, 0], [0.75, 0.75, 0]]),
    ("a closed tetrahedron", TETRA, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], None, [0, 3, 6, 9, 12],
     [0, 3, 6, 2, 4, 9, 1, 8, 10, 5, 7, 11], [0, 0, 0, 0], [[-R3, -R3, -R3], [1, 0, 0], [0, 1, 0], [0, 0, 1]], None),
    ("a bow-tie sharing one vertex", [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 2, 0]], [[0, 1, 2], [2, 3, 4]], None,
     [0, 1, 2, 4, 5, 6], [0, 1, 2, 3, 4, 5], [1, 1, 1, 1, 1], [UP] * 5, None),
    ("three triangles on one edge", FINS, [[0, 1, 2], [0, 1, 3], [0, 1, 4]], None, [0, 3, 6, 7, 8, 9], [0, 3, 6, 1, 4, 7, 2, 5, 8],
     [1, 1, 1, 1, 1], None, None),
    # the same three closed by four more faces: the edge (0, 1) is still in three triangles, every other edge in two, nothing is open
    ("three triangles on one edge, closed", FINS, [[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 2, 3], [0, 3, 4], [1, 3, 2], [1, 4, 3]], None,
     [0, 5, 10, 13, 18, 21], [0, 3, 6, 9, 12, 1, 4, 7, 15, 18, 2, 10, 17, 5, 11, 13, 16, 20, 8, 14, 19], [0, 0, 0, 0, 0], None, None),
    ("(a, a, b) and (a, a, a)", [[0, 0, 0], [1, 0, 0], [5, 5, 5]], [[1, 1, 0], [2, 2, 2]], None, [0, 1, 3, 6], [2, 0, 1, 3, 4, 5], [0, 0, 0],
     [[0, 0, 0]] * 3, [[0.5, 0, 0], [0.5, 0, 0], [5, 5, 5]]),
    ("indices -1, Nv, INT_MAX and INT_MIN", SQUARE, [[0, 1, -1], [1, 2, 4], [2, 3, 3], [4, 0, 0], [INT_MAX, 0, 1], [INT_MIN, 1, 2]], None,
     [0, 0, 0, 1, 3], [6, 7, 8], [0, 0, 0, 0], [[0, 0, 0]] * 4, [[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 1, 0]]),
    ("a mask hiding everything", SQUARE[:3], [[0, 1, 2]], [0], [0, 0, 0, 0], [], [0, 0, 0], [[0, 0, 0]] * 3, SQUARE[:3]),
]


def everything(vertices, faces, mask=None, s=0.5):
    """(offsets, corners, boundary, normals, one free step) of the restatement."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    offsets, corners, boundary = ms.adjacency(faces, len(v), mask)
    return offsets, corners, boundary, ms.normals(v, faces, offsets, corners), ms.step(v, faces, offsets, corners, s)


def radius(p):
    return np.linalg.norm(np.asarray(p, dtype=np.float64), axis=1)


def angles_to(n, axis):
    """Degrees between unit normals [N, 3] and the line along `axis`."""
    return np.degrees(np.arccos(np.clip(np.abs(np.asarray(n, dtype=np.float64) @ axis), 0, 1)))


def off_wall(p):
    return np.abs(np.asarray(p, dtype=np.float64) @ (WALL * np.sqrt(1.04)) - 4.0) / np.sqrt(1.04)


def face_cross(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    return np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])


def facing_away(s, vertices):
    """The triangles whose normal does not point to the mean camera centre (tests/test_tsdf_mesh_cpu.py's count)."""
    fa = s["mesh"]["faces"]
    cam = s["centres"].astype(np.float64).mean(0)
    return int(((face_cross(vertices, fa) * (cam - np.asarray(vertices, dtype=np.float64)[fa[:, 0]])).sum(1) <= 0).sum())


def wall_scene(noise):
    s = tr.static_scene(noise)
    o = s["out"]
    s["mesh"] = tm.mesh(o["K"], o["f"], o["Wt"], o["col"], s["voxel"], tr.DEFAULTS["min_weight"])
    return s


def wall_figures(tag, s):
    """The raw and the smoothed (10 iterations, pinned) mesh of a wall scene, measured: dict of the figures, printed."""
    v, f = s["mesh"]["vertices"], s["mesh"]["faces"]
    offsets, corners, boundary = ms.adjacency(f, len(v))
    p = ms.smooth(v, f, iterations=10)
    inner = boundary == 0
    out = dict(v=v, p=p, boundary=boundary)
    for name, q in (("raw", v), ("smooth", p)):
        n = ms.normals(q, f, offsets, corners)
        a = angles_to(n[inner], WALL)
        out[name] = dict(rms=float(np.sqrt((off_wall(q) ** 2).mean())), angle=float(a.mean()), p95=float(np.percentile(a, 95)),
                         away=facing_away(s, q), flat=int((np.linalg.norm(face_cross(q, f), axis=1) == 0).sum()), normals=n)
    out["moved"] = float(np.linalg.norm(p.astype(np.float64) - v, axis=1).max() / s["voxel"])
    print(f"[mesh smooth {tag}] V {len(v)}, T {len(f)}, {int(boundary.sum())} boundary vertices, valence <= {int(np.diff(offsets).max())}; "
          + "; ".join(f"{k}: RMS {o['rms']:.4f}, normal angle mean {o['angle']:.2f} p95 {o['p95']:.1f} deg, {o['away']} facing away, "
                      f"{o['flat']} of zero area" for k, o in out.items() if k in ("raw", "smooth"))
          + f"; largest displacement {out['moved']:.3f} voxel")
    return out


# ---- what the rule is worth ----------------------------------------------------------------------------------------------------------------
def test_noisy_wall_gets_closer_to_the_wall_and_its_normals_too():
    """Measured (fp32 numpy): V 1 226, T 2 306, 186 boundary vertices, valence <= 10. Raw: RMS to the wall 0.0171, mean normal angle
    6.45 deg (p95 17.7), 39 triangles facing away. After 10 pinned iterations: RMS 0.0142, mean angle 4.48 deg (p95 11.2), 39 facing
    away, largest displacement 0.351 voxel, no triangle of zero area."""
    s = wall_scene(0.02)
    w = wall_figures("noisy wall", s)
    assert w["smooth"]["rms"] <= w["raw"]["rms"]
    assert w["smooth"]["angle"] < w["raw"]["angle"]
    pinned = w["boundary"] == 1
    assert pinned.sum() > 0 and np.array_equal(w["p"][pinned], w["v"][pinned]) and not np.array_equal(w["p"][~pinned], w["v"][~pinned])
    assert w["moved"] < 1.0
    assert w["smooth"]["away"] <= 0.05 * len(s["mesh"]["faces"])
    assert w["smooth"]["flat"] == 0


def test_clean_wall_stays_clean():
    """Measured: V 1 016, T 1 880, 150 boundary vertices. RMS 0.0013 -> 0.0011, mean normal angle 0.33 -> 0.23 deg, nothing facing
    away."""
    s = wall_scene(0.0)
    w = wall_figures("clean wall", s)
    assert w["smooth"]["rms"] <= w["raw"]["rms"]
    assert w["smooth"]["away"] == 0 and w["raw"]["away"] == 0
    assert w["smooth"]["angle"] < 1.0 and w["raw"]["angle"] < 1.0
    for k in ("raw", "smooth"):
        assert np.abs(radius(w[k]["normals"]) - 1).max() <= 1e-6, k


def test_taubin_keeps_the_size_of_a_noisy_icosphere_and_lambda_alone_does_not():
    """Measured: V 162, T 320; raw mean radius 1.0006, std 0.0288; Taubin (10 iterations) 1.0087, std 0.0120; lam alone 0.798."""
    v, f = ms.noisy_icosphere()
    assert v.shape == (162, 3) and f.shape == (320, 3) and not ms.adjacency(f, 162)[2].any()
    raw, taubin, shrunk = radius(v), radius(ms.smooth(v, f, iterations=10)), radius(ms.smooth(v, f, iterations=10, mu=0))
    print(f"[mesh smooth icosphere] radius raw {raw.mean():.4f} +- {raw.std():.4f}, Taubin {taubin.mean():.4f} +- {taubin.std():.4f}, "
          f"lam alone {shrunk.mean():.4f} +- {shrunk.std():.4f}")
    assert abs(taubin.mean() - raw.mean()) <= 0.02 * raw.mean()
    assert shrunk.mean() < 0.85 * raw.mean()
    assert taubin.std() <= 0.6 * raw.std()
    clean, f = ms.icosphere()
    n = ms.vertex_normals(clean.astype(np.float32), f)
    cos = (n.astype(np.float64) * clean).sum(1)
    print(f"[mesh smooth icosphere] smallest cosine of a normal with its radius {cos.min():.6f}")
    assert (cos >= 0.999).all()


def test_icosphere_with_the_faces_at_vertex_0_masked_out():
    v, f = ms.noisy_icosphere()
    mask = ~(f == 0).any(1)
    ring = np.unique(f[~mask])
    ring = ring[ring != 0]
    assert (~mask).sum() == 5 and len(ring) == 5
    offsets, corners, boundary = ms.adjacency(f, len(v), mask)
    assert np.array_equal(np.flatnonzero(boundary), ring)
    assert offsets[0] == offsets[1] == 0 and offsets[-1] == 3 * mask.sum()
    assert np.array_equal(ms.normals(v, f, offsets, corners)[0], np.zeros(3, np.float32))
    for pin in (True, False):
        p = ms.smooth(v, f, iterations=3, pin_boundary=pin, face_mask=mask)
        assert np.array_equal(p[0], v[0]) and np.array_equal(p[ring], v[ring]) == pin and not np.array_equal(p[1:], v[1:])


# ---- hand cases --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_hand_cases(case):
    _, vertices, faces, mask, offsets, corners, boundary, normals, stepped = case
    got = everything(vertices, faces, mask)
    assert got[0].dtype == np.int32 and got[0].tolist() == offsets
    assert got[1].dtype == np.int32 and got[1].tolist() == corners
    assert got[2].dtype == np.uint8 and got[2].tolist() == boundary
    assert got[3].dtype == np.float32 and got[4].dtype == np.float32
    if normals is not None:
        assert np.array_equal(got[3], np.asarray(normals, dtype=np.float32))
    if stepped is not None:
        assert np.array_equal(got[4], np.asarray(stepped, dtype=np.float32))
    # an independent statement of the normals: float64 sums of the valid faces' cross products
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    ok = ((f >= 0) & (f < len(v))).all(1) & (True if mask is None else np.asarray(mask, dtype=bool))
    want = np.zeros_like(v)
    for t in np.flatnonzero(ok):
        for k in range(3):
            want[f[t, k]] += face_cross(v, f[t:t + 1])[0]
    length = np.linalg.norm(want, axis=1, keepdims=True)
    assert np.allclose(got[3], np.where(length > 0, want / np.where(length > 0, length, 1), 0), atol=1e-6)
    pinned = ms.step(np.asarray(vertices, np.float32), faces, got[0], got[1], 0.5, np.ones(len(v), np.uint8))
    assert np.array_equal(pinned, np.asarray(vertices, np.float32))


def test_closed_tetrahedron_has_outward_normals_and_the_shared_edge_makes_no_boundary():
    off, cor, b, n, _ = everything(TETRA, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    assert ((n.astype(np.float64) * (np.asarray(TETRA) - np.mean(TETRA, 0))).sum(1) > 0).all() and not b.any()
    # three triangles on the edge (0, 1): at both ends the other end stands three times and only the wing tips stand once
    faces = [[0, 1, 2], [0, 1, 3], [0, 1, 4]]
    off, cor, b = ms.adjacency(faces, 5)
    v, w, _ = ms.neighbours(faces, 5, off, cor)
    assert w[v == 0].tolist() == [1, 2, 1, 3, 1, 4] and w[v == 1].tolist() == [2, 0, 3, 0, 4, 0] and w[v == 2].tolist() == [0, 1]
    assert b.tolist() == [1] * 5
    # with the wing tips joined up nothing stands once although (0, 1) is still in three triangles
    assert not ms.adjacency(HAND_CASES[5][2], 5)[2].any()


def test_non_finite_coordinates_spread_one_ring_per_step():
    v, f = ms.noisy_icosphere()
    v = v.copy()
    v[7, 1] = np.nan
    off, cor, _ = ms.adjacency(f, len(v))
    ring = np.unique(f[(f == 7).any(1)])
    one = ms.step(v, f, off, cor, 0.5)
    assert np.isnan(one[ring, 1]).all() and np.isfinite(np.delete(one, ring, 0)).all() and np.isfinite(one[:, [0, 2]]).all()
    n = ms.normals(v, f, off, cor)
    assert (n[ring] == 0).all() and np.abs(radius(np.delete(n, ring, 0)) - 1).max() < 1e-6     # a NaN sum has no finite length: zero


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def test_table_properties_on_random_meshes():
    rng = np.random.default_rng(5)
    for k in range(6):
        Nv, T = int(rng.integers(1, 300)), int(rng.integers(0, 600))
        faces = rng.integers(-1, Nv + 1, size=(T, 3)).astype(np.int32) if k % 2 else random_mesh(rng, Nv, T)
        mask = rng.integers(0, 2, T) if k % 3 == 0 else None
        offsets, corners, boundary = ms.adjacency(faces, Nv, mask)
        ok = ((faces >= 0) & (faces < Nv)).all(1) & (True if mask is None else mask != 0)
        assert offsets[0] == 0 and offsets[-1] == 3 * ok.sum() == len(corners) and (np.diff(offsets) >= 0).all()
        assert sorted(corners.tolist()) == (3 * np.flatnonzero(ok)[:, None] + np.arange(3)).reshape(-1).tolist()
        for v in range(Nv):
            row = corners[offsets[v]:offsets[v + 1]]
            assert (np.diff(row) > 0).all() and (faces.reshape(-1)[row] == v).all()
        for seed in range(5):
            perm = np.random.default_rng(seed).permutation(T)
            o2, c2, b2 = ms.adjacency(faces[perm], Nv, None if mask is None else mask[perm])
            assert np.array_equal(o2, offsets) and np.array_equal(b2, boundary)
            rows = lambda fa, o, c: [sorted(map(tuple, fa[c[o[v]:o[v + 1]] // 3].tolist())) for v in range(Nv)]
            assert rows(faces[perm], o2, c2) == rows(faces, offsets, corners)            # the same faces round every vertex
    faces, Nv = bad_index_mesh()
    offsets, corners, _ = ms.adjacency(faces, Nv)
    assert offsets[-1] == 3 * 260


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
    buf, buf2 = (ctypes.c_double * 4096)(), (ctypes.c_double * 4096)()
    p, q = ctypes.addressof(buf), ctypes.addressof(buf2)
    big, third = 1 << 31, ((1 << 31) + 2) // 3                                      # 3 * third >= 2^31 > 3 * (third - 1)
    sizes = [dict(T=-1), dict(Nv=-1), dict(T=big), dict(Nv=big), dict(T=third, E=0)]
    entries = [dict(E=-1), dict(E=31)]

    def count(faces=p, T=10, Nv=10, mask=None, degree=p, E=0):
        return lib.geo4d_mesh_adjacency_count(faces, T, Nv, mask, degree, None)

    for kw in [dict(faces=None), dict(degree=None)] + sizes:
        assert count(**kw) == -22 and b"mesh_adjacency_count" in lib.geo4d_last_error(), kw

    def fill(faces=p, T=10, Nv=10, mask=None, offsets=p, E=30, cursor=p, corners=p):
        return lib.geo4d_mesh_adjacency_fill(faces, T, Nv, mask, offsets, E, cursor, corners, None)

    for kw in [dict(faces=None), dict(offsets=None), dict(cursor=None), dict(corners=None)] + sizes + entries:
        assert fill(**kw) == -22 and b"mesh_adjacency_fill" in lib.geo4d_last_error(), kw

    def sort(offsets=p, T=10, Nv=10, E=30, unsorted=p, corners=q, long_row=32):
        return lib.geo4d_mesh_adjacency_sort(offsets, T, Nv, E, unsorted, corners, long_row, None)

    for kw in [dict(offsets=None), dict(unsorted=None), dict(corners=None), dict(corners=p), dict(long_row=-1)] + sizes + entries:
        assert sort(**kw) == -22 and b"mesh_adjacency_sort" in lib.geo4d_last_error(), kw

    def boundary(faces=p, T=10, Nv=10, offsets=p, corners=p, E=30, long_row=32, out=p):
        return lib.geo4d_mesh_boundary(faces, T, Nv, offsets, corners, E, long_row, out, None)

    for kw in [dict(faces=None), dict(offsets=None), dict(corners=None), dict(out=None), dict(long_row=-1)] + sizes + entries:
        assert boundary(**kw) == -22 and b"mesh_boundary" in lib.geo4d_last_error(), kw

    def step(vertices=p, faces=p, T=10, Nv=10, offsets=p, corners=p, E=30, pinned=None, s=0.5, out=q):
        return lib.geo4d_mesh_smooth_step(vertices, faces, T, Nv, offsets, corners, E, pinned, s, out, None)

    for kw in [dict(vertices=None), dict(faces=None), dict(offsets=None), dict(corners=None), dict(out=None), dict(out=p),
               dict(s=float("nan")), dict(s=float("inf")), dict(s=-float("inf")), dict(s=1e39)] + sizes + entries:
        assert step(**kw) == -22 and b"mesh_smooth_step" in lib.geo4d_last_error(), kw

    def normals(vertices=p, faces=p, T=10, Nv=10, offsets=p, corners=p, E=30, out=q):
        return lib.geo4d_mesh_vertex_normals(vertices, faces, T, Nv, offsets, corners, E, out, None)

    for kw in [dict(vertices=None), dict(faces=None), dict(offsets=None), dict(corners=None), dict(out=None)] + sizes + entries:
        assert normals(**kw) == -22 and b"mesh_vertex_normals" in lib.geo4d_last_error(), kw
    # nothing to do is no error and no launch
    for fn in (count, fill, sort, boundary, step, normals):
        assert fn(T=0, E=0) == 0 and fn(Nv=0) == 0, fn
    assert fill(E=0) == 0 and sort(E=0) == 0


# ---- Python errors -----------------------------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_any_device_work(tmp_path):
    import inspect
    import torch
    from geo4d_amd import _lib, mesh, ops, render, tsdf
    from geo4d_amd.scene_export import get_3D_model_from_scene
    faces, vertices = torch.tensor([[0, 1, 2]], dtype=torch.int32), torch.zeros((3, 3))
    offsets, corners = torch.tensor([0, 1, 2, 3], dtype=torch.int32), torch.tensor([0, 1, 2], dtype=torch.int32)
    for call in (lambda: ops.mesh_adjacency(faces, 3), lambda: ops.mesh_smooth_step(vertices, faces, offsets, corners, 0.5),
                 lambda: ops.mesh_vertex_normals(vertices, faces, offsets, corners), lambda: mesh.mesh_adjacency(faces, 3),
                 lambda: mesh.vertex_normals(vertices, faces), lambda: mesh.smooth_mesh(vertices, faces, iterations=1)):
        with pytest.raises(_lib.Geo4DNativeError, match="no CPU fallback"):
            call()
    assert mesh.smooth_mesh(vertices, faces, iterations=0) is vertices               # nothing to do: the input itself, no launch
    for kw, what in [(dict(iterations=-1), "iterations"), (dict(iterations=2.5), "iterations"), (dict(iterations=True), "iterations"),
                     (dict(iterations=None), "iterations"), (dict(lam=0), "lam"), (dict(lam=1.5), "lam"), (dict(lam=-0.5), "lam"),
                     (dict(lam=float("nan")), "lam"), (dict(lam="half"), "lam"), (dict(mu=0.1), "mu"), (dict(mu=-1.5), "mu"),
                     (dict(mu=float("nan")), "mu")]:
        with pytest.raises(ValueError, match=what + " must"):
            mesh.smooth_mesh(vertices, faces, **kw)
    table = dict(offsets=offsets, corners=corners, boundary=torch.zeros(3, dtype=torch.bool), entries=3)
    for bad in (dict(table, offsets=offsets[:-1]), dict(table, boundary=torch.zeros(4, dtype=torch.bool)), dict(table, entries=2),
                dict(table, corners=torch.zeros(4, dtype=torch.int32), entries=4), {"offsets": offsets}, 7):
        with pytest.raises(ValueError, match="adjacency does not fit"):
            mesh.smooth_mesh(vertices, faces, iterations=0, adjacency=bad)
        with pytest.raises(ValueError, match="adjacency does not fit"):
            mesh.vertex_normals(vertices, faces, adjacency=bad)
    for kw in (dict(smooth_iterations=3), dict(normals=True), dict(smooth_pin_boundary=False)):
        for more in (dict(as_pointcloud=True), dict(as_pointcloud=True, fuse_voxel=0.1), dict(as_pointcloud=True, tsdf_voxel=0.1),
                     dict(as_pointcloud=False)):
            with pytest.raises(ValueError, match="are for the TSDF surface mesh alone"):
                get_3D_model_from_scene(str(tmp_path), True, None, **kw, **more)
        assert get_3D_model_from_scene(str(tmp_path), True, None, as_pointcloud=False, tsdf_mesh=True, **kw) is None
        with pytest.raises(ValueError, match="pass mesh=True"):
            tsdf.tsdf_scene(object(), **kw)
    with pytest.raises(ValueError, match="iterations must be an integer >= 0"):
        get_3D_model_from_scene(str(tmp_path), True, None, as_pointcloud=False, tsdf_mesh=True, smooth_iterations=-2)
    with pytest.raises(ValueError, match="iterations must be an integer >= 0"):
        tsdf.tsdf_scene(object(), mesh=True, smooth_iterations=1.5)
    assert os.listdir(tmp_path) == []
    for fn in (tsdf.tsdf_mesh, tsdf.tsdf_scene, get_3D_model_from_scene, render.render_scene):
        par = inspect.signature(fn).parameters
        assert par["smooth_iterations"].default is None and par["smooth_pin_boundary"].default is True, fn
        assert fn is render.render_scene or par["normals"].default is False, fn
    assert "normals" not in inspect.signature(render.render_scene).parameters


def test_glb_writer_adds_normal_only_when_given():
    from geo4d_amd import io
    rng = np.random.default_rng(0)
    pos, col = rng.random((5, 3)).astype(np.float32), rng.integers(0, 256, (5, 4), dtype=np.uint8)
    faces = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (5, 1))
    plain = io.mesh_geometry(pos, col, faces)
    assert sorted(plain) == sorted(io.mesh_geometry(pos, col, faces, None)) == ["colors", "indices", "mode", "positions"]
    eye = np.eye(4)
    old = io._glb_bytes([dict(mode=4, positions=pos, colors=col, indices=faces)], eye)
    assert io._glb_bytes([plain], eye) == old == io._glb_bytes([dict(plain, normals=None)], eye)
    data = io._glb_bytes([io.mesh_geometry(pos, col, faces, nrm)], eye)
    n_json = struct.unpack("<I", data[12:16])[0]
    doc = json.loads(data[20:20 + n_json])
    prim = doc["meshes"][0]["primitives"][0]
    assert sorted(prim["attributes"]) == ["COLOR_0", "NORMAL", "POSITION"] and prim["mode"] == 4
    acc = doc["accessors"][prim["attributes"]["NORMAL"]]
    assert acc["count"] == 5 and acc["type"] == "VEC3" and acc["componentType"] == 5126 and "normalized" not in acc
    view = doc["bufferViews"][acc["bufferView"]]
    assert view["target"] == 34962 and view["byteLength"] == 60
    start = 20 + n_json + 8 + view["byteOffset"]
    assert np.array_equal(np.frombuffer(data[start:start + 60], dtype=np.float32).reshape(5, 3), nrm)
    assert doc["accessors"][prim["attributes"]["POSITION"]]["count"] == 5 and doc["accessors"][prim["indices"]]["count"] == 6
    with pytest.raises(ValueError, match="normals must be"):
        io._glb_bytes([io.mesh_geometry(pos, col, faces, nrm[:4])], eye)
