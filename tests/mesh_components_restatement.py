"""The rule of geo4d_amd/csrc/mesh_components.hip (include/geo4d_hip.h) in numpy, followed literally: a serial union-find with the
smaller root on top. Integer arithmetic only.

valid:  face t is valid iff face_mask[t] != 0 (or there is no mask) and its three indices lie in [0, Nv). (a, a, b) connects a and b,
        (a, a, a) touches a alone.
joined: two vertices are connected iff a chain of valid faces links them, consecutive faces sharing at least one vertex.
labels: a vertex no valid face names gets vertex_component -1; the root of a component is its smallest vertex index; components are
        numbered 0 .. C - 1 in ascending order of root; face_component is the component of the face's vertices, -1 for a face that is
        not valid; component_vertices / component_faces count touched vertices and valid faces.
select: face t is kept iff keep_face[t] != 0 and its indices lie in [0, Nv); a vertex is kept iff a kept face names it; kept vertices
        and faces keep their relative order; faces are rewritten to the new rows; vertex_index is the old row of every new one.
"""
import numpy as np


def valid_faces(faces, Nv, face_mask=None):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < Nv)).all(axis=1)
    if face_mask is not None:
        ok &= np.asarray(face_mask).reshape(-1) != 0
    return faces, ok


def components(faces, Nv, face_mask=None):
    """(vertex_component int32 [Nv], face_component int32 [T], component_vertices int32 [C], component_faces int32 [C])"""
    faces, ok = valid_faces(faces, Nv, face_mask)
    parent = list(range(Nv))
    touched = np.zeros(Nv, dtype=bool)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:                                          # shorten the path: the sets stay what they are
            parent[x], x = r, parent[x]
        return r

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for (i0, i1, i2), valid in zip(faces.tolist(), ok.tolist()):
        if not valid:
            continue
        touched[[i0, i1, i2]] = True
        union(i0, i1)
        union(i1, i2)
    root = np.arange(Nv, dtype=np.int64)
    for v in range(Nv):                                                # parent[v] <= v: the parent's root is already known
        root[v] = root[parent[v]]
    is_root = touched & (root == np.arange(Nv))
    dense = np.cumsum(is_root) - is_root                               # exclusive prefix sum: ascending order of root
    C = int(is_root.sum())
    vertex_component = np.where(touched, dense[root] if Nv else 0, -1).astype(np.int32) if Nv else np.zeros(0, np.int32)
    face_component = np.full(len(faces), -1, dtype=np.int32)
    if ok.any():
        face_component[ok] = vertex_component[faces[ok, 0]]
    component_vertices = np.bincount(vertex_component[vertex_component >= 0], minlength=C).astype(np.int32)
    component_faces = np.bincount(face_component[face_component >= 0], minlength=C).astype(np.int32)
    return vertex_component, face_component, component_vertices, component_faces


def select(vertices, faces, keep_face, rgba=None, weight=None):
    """(vertices [V', 3], rgba [V', 4] or None, weight [V'] or None, faces int32 [T', 3], vertex_index int32 [V'])"""
    vertices = np.asarray(vertices)
    Nv = len(vertices)
    faces, kept = valid_faces(faces, Nv, keep_face)
    keep_vertex = np.zeros(Nv, dtype=bool)
    keep_vertex[faces[kept].reshape(-1)] = True
    new_row = np.cumsum(keep_vertex) - keep_vertex
    vertex_index = np.flatnonzero(keep_vertex).astype(np.int32)
    new_faces = new_row[faces[kept]].astype(np.int32).reshape(-1, 3)
    return (vertices[keep_vertex], None if rgba is None else np.asarray(rgba)[keep_vertex],
            None if weight is None else np.asarray(weight)[keep_vertex], new_faces, vertex_index)


def keep_components(component_faces, min_faces=None, min_fraction=None, keep_largest=None):
    """bool [C]: geo4d_amd.mesh.keep_rule's statement, on python integers: c >= min_faces, c * den >= num * max for the fraction num / den
    as given, and among the keep_largest largest, ties toward the lower id."""
    from fractions import Fraction
    c = [int(x) for x in np.asarray(component_faces).reshape(-1)]
    keep = [True] * len(c)
    if min_faces is not None:
        keep = [k and x >= min_faces for k, x in zip(keep, c)]
    if min_fraction is not None and c:
        fr = Fraction(min_fraction)
        keep = [k and x * fr.denominator >= fr.numerator * max(c) for k, x in zip(keep, c)]
    if keep_largest is not None:
        top = set(sorted(range(len(c)), key=lambda i: (-c[i], i))[:keep_largest])
        keep = [k and i in top for i, k in enumerate(keep)]
    return np.array(keep, dtype=bool)


# ---- the floater scene -------------------------------------------------------------------------------------------------------------------
def floater_scene(half=0.35, centre=(0.0, -0.8, 3.0)):
    """tsdf_restatement.static_scene(0.0)'s clean wall with a small static square plate planted in front of it: the plate lies in the
    plane z = centre[2] (the wall is near z = 4, so it is detached by more than the truncation of 4 voxels of about 0.13), is 2 * half
    wide (five voxels), lies above the moving sphere's path and is seen by every camera. Returns the scene dict with `out` (the TSDF
    rule) and `mesh` (the surface-nets rule) of the restatements."""
    import motion_restatement as mr
    import tsdf_mesh_restatement as tm
    import tsdf_restatement as tr
    s = mr.synthetic_scene(noise=0.0)
    n, H, W = s["n"], s["H"], s["W"]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth, pts3d = s["depth"].astype(np.float64), s["pts3d"].astype(np.float64)
    for i in range(n):
        Kc, R, c = s["K"][i], s["cams2world"][i, :3, :3], s["cams2world"][i, :3, 3]
        d = np.stack([(xs - Kc[0, 2]) / Kc[0, 0], (ys - Kc[1, 2]) / Kc[1, 1], np.ones_like(xs)], -1) @ R.T
        t = (centre[2] - c[2]) / d[..., 2]
        p = c + t[..., None] * d
        hit = (np.abs(p[..., 0] - centre[0]) < half) & (np.abs(p[..., 1] - centre[1]) < half) & (t > 0) & (t < depth[i])
        depth[i] = np.where(hit, t, depth[i])
        pts3d[i] = np.where(hit[..., None], p, pts3d[i])
    s["depth"], s["pts3d"] = depth.astype(np.float32), pts3d.astype(np.float32)
    s["static"] = s["valid"] & ~mr.segment(s["pts3d"], s["depth"], s["valid"], s["cams2world"], s["K"])
    s["voxel"] = 2 * np.median(s["depth"][s["static"]] / 60)
    s["views"], s["centres"] = mr.views_of(s["cams2world"], s["K"]), tr.centres_of(s["cams2world"])
    s["rgba"] = np.random.default_rng(8).integers(0, 256, size=(n, H, W, 4), dtype=np.uint8)
    o = s["out"] = tr.tsdf(s["pts3d"], s["depth"], s["static"], s["views"], s["centres"], s["rgba"], voxel=s["voxel"])
    s["mesh"] = tm.mesh(o["K"], o["f"], o["Wt"], o["col"], s["voxel"], tr.DEFAULTS["min_weight"])
    return s


def off_wall(p):
    """Distance of points [N, 3] to the wall -0.2 x + z = 4."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return np.abs(-0.2 * p[:, 0] + p[:, 2] - 4.0) / np.sqrt(1.04)
