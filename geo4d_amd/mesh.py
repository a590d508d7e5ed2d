"""Clean-up of indexed triangle meshes on the HIP device (csrc/mesh_components.hip): label the connected pieces, drop the small ones.

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
