"""Clean-up of indexed triangle meshes on the HIP device: label the connected pieces and drop the small ones (csrc/mesh_components.hip);
smooth the vertices and give them normals from one corner table (csrc/mesh_smooth.hip).

Every TSDF of noisy depth leaves debris: small detached patches in front of and behind the real surface. ``mesh_components`` labels
the pieces of any mesh (a lock-free union-find, one thread per face), ``remove_small_components`` keeps the pieces that are large
enough and returns the mesh of their faces with the unreferenced vertices gone. ``tsdf.tsdf_mesh``, ``tsdf.tsdf_scene(mesh=True)``,
``get_3D_model_from_scene``, ``save_scene`` and ``render_scene(static_mesh=...)`` take ``min_component_faces`` /
``min_component_fraction`` and apply it to the mesh they make. The reference has no such step and nothing is ported. The rule is stated
in include/geo4d_hip.h and restated in numpy in tests/mesh_components_restatement.py; it is integer arithmetic, so the result is a
function of the mesh alone.

A piece's size is its number of faces. On a surface-nets mesh every triangle is about half a voxel face, so the count is the area in
voxel units. Limits: vertex connectivity (two pieces touching in one vertex are one piece); int32 indices; no areas, bounding boxes or
other float measures; nobody has tried the thresholds on real predictions.

``mesh_adjacency`` builds the corner table: for each vertex, sorted, the corners of the faces around it, and which vertices lie on the
mesh's boundary. ``smooth_mesh`` runs Taubin (lambda | mu) smoothing on it, which takes the voxel-scale staircase out of a surface-nets
mesh and all but keeps its size (a noisy unit sphere: 0.8 % after 10 iterations, where lam alone loses 20 %), and
``vertex_normals`` gives area-weighted unit normals. ``tsdf_mesh``, ``tsdf_scene(mesh=True)``,
``get_3D_model_from_scene(tsdf_mesh=...)``, ``save_scene`` and ``render_scene(static_mesh=...)`` take ``smooth_iterations`` /
``smooth_pin_boundary`` (and, but for the renderer, ``normals``). The rule is stated in include/geo4d_hip.h and restated in numpy in
tests/mesh_smooth_restatement.py. Every float is gathered per vertex in the table's order, so the results are bitwise reproducible;
they are functions of the mesh as given: another face order sums in another order and may change last bits. Limits: time is linear in
the largest valence; a normal is zero where the sum of its faces' cross products vanishes; int32 indices and 3 T < 2^31; uniform
weights per face (no cotangent weights, no feature preservation); nobody has tried the defaults on real predictions.
"""
from fractions import Fraction
from numbers import Integral, Real

import torch

from . import ops


def check_keep_args(min_faces=None, min_fraction=None, keep_largest=None, who="remove_small_components"):
    """ValueError for min_faces < 1, min_fraction outside (0, 1] or keep_largest < 1 (None: no constraint)."""
    for value, what in ((min_faces, "min_faces"), (keep_largest, "keep_largest")):
        if value is not None and (isinstance(value, bool) or not isinstance(value, Integral) or value < 1):
            raise ValueError(f"{who}: {what} must be an integer >= 1, got {value!r}")
    if min_fraction is not None and (isinstance(min_fraction, bool) or not isinstance(min_fraction, (Real, Fraction))
                                     or not 0 < min_fraction <= 1):
        raise ValueError(f"{who}: min_fraction must lie in (0, 1], got {min_fraction!r}")


def keep_rule(component_faces, min_faces=None, min_fraction=None, keep_largest=None):
    """list of bool [C]: which components stay, from their face counts alone, in integers. A component is kept iff its count c >=
    min_faces, c * den >= num * max(counts) for min_fraction = num / den exactly as given (a float stands for its exact binary value), and
    it is among the keep_largest largest, ties toward the lower component id. Arguments left at None do not constrain."""
    check_keep_args(min_faces, min_fraction, keep_largest)
    counts = [int(c) for c in (component_faces.tolist() if hasattr(component_faces, "tolist") else component_faces)]
    keep = [True] * len(counts)
    if min_faces is not None:
        keep = [k and c >= min_faces for k, c in zip(keep, counts)]
    if min_fraction is not None and counts:
        fraction, largest = Fraction(min_fraction), max(counts)
        keep = [k and c * fraction.denominator >= fraction.numerator * largest for k, c in zip(keep, counts)]
    if keep_largest is not None:
        top = set(sorted(range(len(counts)), key=lambda i: (-counts[i], i))[:keep_largest])
        keep = [k and i in top for i, k in enumerate(keep)]
    return keep


@torch.no_grad()
def mesh_components(faces, n_vertices, face_mask=None):
    """dict(vertex_component int32 [Nv], face_component int32 [T], component_vertices int32 [C], component_faces int32 [C],
    components = C) of the mesh faces int32 [T, 3] over n_vertices vertices on the HIP device (ops.mesh_components): vertices joined by
    a chain of valid faces sharing a vertex are one component, numbered in ascending order of their smallest vertex; -1 marks a vertex
    that no valid face names and a face that is masked out (`face_mask` [T] bool) or has an index outside [0, n_vertices)."""
    vc, fc, cv, cf = ops.mesh_components(faces, n_vertices, face_mask)
    return dict(vertex_component=vc, face_component=fc, component_vertices=cv, component_faces=cf, components=int(cv.shape[0]))


@torch.no_grad()
def remove_small_components(vertices, faces, *, min_faces=None, min_fraction=None, keep_largest=None, rgba=None, weight=None, face_mask=None):
    """dict(vertices, rgba, weight, faces, vertex_index, components, kept_components, removed_faces, removed_vertices): the mesh without
    its small pieces. vertices fp32 [Nv, 3], faces int32 [T, 3], rgba uint8 [Nv, 4] / weight fp32 [Nv] (None: none) on the HIP device.

    A component (mesh_components) is kept by keep_rule: at least `min_faces` faces, at least `min_fraction` of the largest component's
    faces (compared in integers), and among the `keep_largest` largest; None does not constrain. The result holds the faces of the kept
    components and the vertices they name, both in their old order (ops.mesh_select); `vertex_index` int32 [V'] is the old row of every
    new vertex, `removed_faces` / `removed_vertices` count what went (invalid faces and unreferenced vertices included). With all three
    None nothing is launched and the inputs' own tensors come back (`vertex_index`, `components` and `kept_components` None)."""
    check_keep_args(min_faces, min_fraction, keep_largest)
    if min_faces is None and min_fraction is None and keep_largest is None:
        return dict(vertices=vertices, rgba=rgba, weight=weight, faces=faces, vertex_index=None, components=None, kept_components=None,
                    removed_faces=0, removed_vertices=0)
    _, face_component, _, component_faces = ops.mesh_components(faces, vertices.shape[0], face_mask)
    keep = keep_rule(component_faces, min_faces, min_fraction, keep_largest)
    keep_component = torch.tensor(keep + [False], dtype=torch.bool, device=faces.device)     # the last row answers for -1
    keep_face = keep_component[face_component.long()]
    v, col, w, f, vertex_index = ops.mesh_select(vertices, faces, keep_face, rgba, weight)
    return dict(vertices=v, rgba=col, weight=w, faces=f, vertex_index=vertex_index, components=len(keep), kept_components=sum(keep),
                removed_faces=int(faces.shape[0] - f.shape[0]), removed_vertices=int(vertices.shape[0] - v.shape[0]))


def check_smooth_args(iterations=0, lam=0.5, mu=-0.53, who="smooth_mesh"):
    """ValueError for iterations not an integer >= 0, lam outside (0, 1] or mu outside [-1, 0]."""
    if isinstance(iterations, bool) or not isinstance(iterations, Integral) or iterations < 0:
        raise ValueError(f"{who}: iterations must be an integer >= 0, got {iterations!r}")
    if isinstance(lam, bool) or not isinstance(lam, Real) or not 0 < lam <= 1:
        raise ValueError(f"{who}: lam must lie in (0, 1], got {lam!r}")
    if isinstance(mu, bool) or not isinstance(mu, Real) or not -1 <= mu <= 0:
        raise ValueError(f"{who}: mu must lie in [-1, 0], got {mu!r}")


def _table(adjacency, faces, n_vertices, face_mask, who):
    """The corner table to work on: `adjacency` (a mesh_adjacency dict, whose shapes must fit the mesh) or a fresh one."""
    if adjacency is None:
        return mesh_adjacency(faces, n_vertices, face_mask)
    try:
        offsets, corners, boundary = adjacency["offsets"], adjacency["corners"], adjacency["boundary"]
        fits = (tuple(offsets.shape) == (n_vertices + 1,) and tuple(boundary.shape) == (n_vertices,) and corners.dim() == 1
                and corners.shape[0] == adjacency["entries"] <= 3 * faces.shape[0])
    except (KeyError, TypeError, AttributeError):
        fits = False
    if not fits:
        raise ValueError(f"{who}: adjacency does not fit a mesh of {n_vertices} vertices and {faces.shape[0]} faces; pass what "
                         "mesh_adjacency(faces, n_vertices) returns")
    return adjacency


@torch.no_grad()
def mesh_adjacency(faces, n_vertices, face_mask=None):
    """dict(offsets int32 [Nv + 1], corners int32 [E], boundary bool [Nv], entries = E) of the mesh faces int32 [T, 3] over n_vertices
    vertices on the HIP device (ops.mesh_adjacency): the corner table. Entry e = 3 t + k stands for corner k of face t and lies in the row
    of vertex faces[t][k]; row v is corners[offsets[v]:offsets[v + 1]], ascending, so the table is a function of the mesh alone. A face
    that is masked out (`face_mask` [T] bool) or has an index outside [0, n_vertices) has no entries. `boundary` marks the vertices with a
    neighbour that only one face joins them to. Moving vertices leaves the table valid: smooth_mesh and vertex_normals take it as
    `adjacency`."""
    offsets, corners, boundary = ops.mesh_adjacency(faces, n_vertices, face_mask)
    return dict(offsets=offsets, corners=corners, boundary=boundary.view(torch.bool), entries=int(corners.shape[0]))


@torch.no_grad()
def vertex_normals(vertices, faces, *, face_mask=None, adjacency=None):
    """fp32 [Nv, 3]: area-weighted unit vertex normals of the mesh vertices fp32 [Nv, 3], faces int32 [T, 3] on the HIP device
    (ops.mesh_vertex_normals): the sum of the faces' cross products (p1 - p0) x (p2 - p0) round the vertex, whose lengths are twice
    the areas, normalised; (0, 0, 0) where the sum has no finite positive length, as for a vertex no valid face names. `adjacency`: a
    mesh_adjacency dict of this mesh to reuse (then `face_mask` is not looked at)."""
    table = _table(adjacency, faces, vertices.shape[0], face_mask, "vertex_normals")
    return ops.mesh_vertex_normals(vertices, faces, table["offsets"], table["corners"])


@torch.no_grad()
def smooth_mesh(vertices, faces, *, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, face_mask=None, adjacency=None):
    """fp32 [Nv, 3]: the vertices after `iterations` iterations of Taubin smoothing on the HIP device (ops.mesh_smooth_step). Each
    iteration moves every vertex by `lam` times the way to the mean of its neighbours and then, unless `mu` is 0, by `mu` (negative:
    away from it), which undoes the shrinking of the first step. The neighbours of v are the other two vertices of every face round
    v, so the weights count faces: a neighbour seen from two faces counts twice, and the mean is that of the opposite edges' midpoints;
    nothing is de-duplicated. `pin_boundary` keeps the boundary vertices (mesh_adjacency) where they are, bit for bit, as every vertex
    without neighbours stays; non-finite coordinates spread as IEEE arithmetic says. Every step reads one buffer and writes another; the
    input is never written. `iterations=0` launches nothing and returns `vertices` itself. `adjacency`: a mesh_adjacency dict of this
    mesh to reuse (then `face_mask` is not looked at): a step moves no vertex between faces, so the table outlives the smoothing."""
    check_smooth_args(iterations, lam, mu)
    if adjacency is not None:
        _table(adjacency, faces, vertices.shape[0], face_mask, "smooth_mesh")
    if iterations == 0:
        return vertices
    table = _table(adjacency, faces, vertices.shape[0], face_mask, "smooth_mesh")
    pinned = table["boundary"] if pin_boundary else None
    p, spare = vertices, [torch.empty_like(vertices), torch.empty_like(vertices)]
    for _ in range(iterations):
        for s in (lam, mu):
            if s != 0:
                p = ops.mesh_smooth_step(p, faces, table["offsets"], table["corners"], s, pinned, out=spare[0])
                spare.reverse()
    return p
