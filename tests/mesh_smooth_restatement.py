"""The rule of geo4d_amd/csrc/mesh_smooth.hip (include/geo4d_hip.h) in numpy, followed literally: the sorted corner table of an indexed
triangle mesh and its three consumers, boundary vertices, the Taubin smoothing step and area-weighted vertex normals. Every float
operation is one correctly rounded fp32 `+ - * /` or square root in the order the kernels write them (no fused multiply-add), so the
device is compared with `np.array_equal`.

valid:     face t is valid iff face_mask[t] != 0 (or there is no mask) and its three indices lie in [0, Nv). It may repeat an index.
table:     an entry is e = 3 t + k for a valid face t and corner k and belongs to vertex faces[t][k]; offsets int32 [Nv + 1] is the
           exclusive prefix sum of the entries per vertex, corners int32 [E] holds each vertex's entries ascending in e. A face that
           names v twice appears twice in v's row.
neighbours of v: walk v's row in order; of each entry (t, k) take a = faces[t][(k + 1) % 3], then b = faces[t][(k + 2) % 3]; skip
           those equal to v; m is the list's length. A neighbour seen from two faces stands twice.
boundary:  boundary[v] = 1 iff some id occurs exactly once in v's list.
step(s):   S = 0; for each w of the list in order S_c = S_c + p[w]_c; then p'[v]_c = p[v]_c + s * (S_c / (float) m - p[v]_c). v keeps its
           bits if m = 0 or it is pinned. Jacobi: p' is another array.
smoothing: `iterations` times a step with lam, then (mu != 0) a step with mu; pinned = boundary when pin_boundary.
normals:   n(t) = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x) with e1 = p1 - p0, e2 = p2 - p0 in the face's own order;
           N = 0, then N_c = N_c + n(t)_c over v's row in order; len2 = (Nx Nx + Ny Ny) + Nz Nz; N_c / sqrtf(len2) if len2 > 0 and
           finite, else (0, 0, 0).
offsets, boundary and the multiset of each row do not depend on the order of the faces (up to the renaming of t); the float outputs
are functions of the mesh as given: another face order sums in another order and may change last bits.
"""
import numpy as np

from mesh_components_restatement import valid_faces


def adjacency(faces, Nv, face_mask=None):
    """(offsets int32 [Nv + 1], corners int32 [E], boundary uint8 [Nv])"""
    faces, ok = valid_faces(faces, Nv, face_mask)
    entries = (3 * np.flatnonzero(ok)[:, None] + np.arange(3)[None, :]).reshape(-1)             # ascending
    owner = faces.reshape(-1)[entries]
    corners = entries[np.argsort(owner, kind="stable")].astype(np.int32)                        # by vertex, ascending within a row
    offsets = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=Nv)[:Nv])]).astype(np.int32)
    v, w = neighbours(faces, Nv, offsets, corners)[:2]
    boundary = np.zeros(Nv, dtype=np.uint8)
    if len(v):
        pair, count = np.unique(v * Nv + w, return_counts=True)
        boundary[pair[count == 1] // Nv] = 1
    return offsets, corners, boundary


def neighbours(faces, Nv, offsets, corners):
    """(v, w, j): every neighbour-list item in the table's order: its vertex, the neighbour's id and its place in v's list."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.asarray(corners, dtype=np.int64)
    t, k = e // 3, e % 3
    own = np.repeat(np.arange(Nv), np.diff(np.asarray(offsets, dtype=np.int64)))
    assert len(e) == 0 or np.array_equal(faces[t, k], own)
    v = np.repeat(own, 2)
    w = np.stack([faces[t, (k + 1) % 3], faces[t, (k + 2) % 3]], 1).reshape(-1)                 # a, then b, entry after entry
    keep = w != v
    v, w = v[keep], w[keep]
    m = np.bincount(v, minlength=Nv)[:Nv] if Nv else np.zeros(0, np.int64)
    first = np.cumsum(m) - m
    return v, w, np.arange(len(v)) - first[v]


def step(vertices, faces, offsets, corners, s, pinned=None):
    """One Jacobi step with factor s: fp32 [Nv, 3]."""
    p = np.ascontiguousarray(vertices, dtype=np.float32)
    Nv = len(p)
    v, w, j = neighbours(faces, Nv, offsets, corners)
    m = np.bincount(v, minlength=Nv)[:Nv] if Nv else np.zeros(0, np.int64)
    S = np.zeros((Nv, 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for turn in range(int(m.max()) if Nv and len(v) else 0):        # the turn-th neighbour of every vertex that has one: each sum
            now = j == turn                                             # grows in its own list's order
            S[v[now]] = S[v[now]] + p[w[now]]
        moved = m > 0
        if pinned is not None:
            moved &= np.asarray(pinned).reshape(-1) == 0
        out = p.copy()
        mean = S[moved] / m[moved].astype(np.float32)[:, None]
        out[moved] = p[moved] + np.float32(s) * (mean - p[moved])
    assert out.dtype == np.float32
    return out


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, face_mask=None):
    p = np.ascontiguousarray(vertices, dtype=np.float32)
    offsets, corners, boundary = adjacency(faces, len(p), face_mask)
    pinned = boundary if pin_boundary else None
    for _ in range(iterations):
        p = step(p, faces, offsets, corners, lam, pinned)
        if mu != 0:
            p = step(p, faces, offsets, corners, mu, pinned)
    return p


def face_normals(vertices, faces, rows):
    """n(t) fp32 [len(rows), 3] of the faces `rows` (all valid), un-normalised, in the rule's order of operations."""
    p = np.ascontiguousarray(vertices, dtype=np.float32)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[rows]
    with np.errstate(all="ignore"):
        e1, e2 = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    assert n.dtype == np.float32
    return n


def normals(vertices, faces, offsets, corners):
    """Area-weighted unit vertex normals fp32 [Nv, 3]; (0, 0, 0) where the sum has no finite positive length."""
    p = np.ascontiguousarray(vertices, dtype=np.float32)
    Nv = len(p)
    offsets, t = np.asarray(offsets, dtype=np.int64), np.asarray(corners, dtype=np.int64) // 3
    n = face_normals(p, faces, t)
    own = np.repeat(np.arange(Nv), np.diff(offsets))
    place = np.arange(len(t)) - offsets[:-1][own]
    N = np.zeros((Nv, 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for turn in range(int(np.diff(offsets).max()) if Nv and len(t) else 0):
            now = place == turn
            N[own[now]] = N[own[now]] + n[now]
        len2 = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        ok = (len2 > 0) & np.isfinite(len2)
        out = np.zeros((Nv, 3), dtype=np.float32)
        out[ok] = N[ok] / np.sqrt(len2[ok])[:, None]
    assert out.dtype == np.float32
    return out


def vertex_normals(vertices, faces, face_mask=None):
    offsets, corners, _ = adjacency(faces, len(vertices), face_mask)
    return normals(vertices, faces, offsets, corners)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions=2):
    """(vertices float64 [V, 3] on the unit sphere, faces int32 [T, 3] counter-clockwise seen from outside): V = 12, 42, 162, ..."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1),
         (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, dtype=np.int32)


def noisy_icosphere(subdivisions=2, sigma=0.03, seed=0):
    """The icosphere with every radius times (1 + sigma N(0, 1)): (vertices fp32, faces)."""
    v, f = icosphere(subdivisions)
    r = 1 + sigma * np.random.default_rng(seed).standard_normal(len(v))
    return (v * r[:, None]).astype(np.float32), f
