"""The triangle raster and the mesh resolve of geo4d_amd/csrc/render_mesh.hip restated in numpy (helper of tests/test_render_mesh_cpu.py,
tests/test_render_mesh_gpu.py and tools/render_mesh_bench.py): the vertices projected in float32 in the documented op order, coverage
in int64, the weights as one float64 division rounded to float32, per pixel the minimum key over every candidate. The points' part
(splat, fill, quantise) is tests/render_restatement.py's. No GPU, no geo4d_amd import."""
import numpy as np

import render_restatement as rr

EMPTY, F = rr.EMPTY, rr.F
GUARD = F(65536)


def project_vertices(vertices, view, near=1e-3):
    """(ok, cam float32 [Nv, 3], iz, X int64, Y int64) per vertex: steps 1 to 3 of the rule as far as one vertex decides them."""
    M = np.asarray(view, dtype=F)
    P = np.asarray(vertices, dtype=F).reshape(-1, 3)
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        xc, yc, zc = [((M[4 * r] * X + M[4 * r + 1] * Y) + M[4 * r + 2] * Z) + M[4 * r + 3] for r in range(3)]
        ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc > F(near))
        u = M[12] * (xc / zc) + M[14]
        v = M[13] * (yc / zc) + M[15]
        ok &= (np.abs(u) < GUARD) & (np.abs(v) < GUARD)                            # NaN fails
        iz = F(1) / zc
        sx = np.floor(u * F(256) + F(0.5))
        sy = np.floor(v * F(256) + F(0.5))
    return ok, np.stack([xc, yc, zc], 1), iz, np.where(ok, sx, 0).astype(np.int64), np.where(ok, sy, 0).astype(np.int64)


def edge(ax, ay, bx, by, sx, sy):
    return (bx - ax) * (sy - ay) - (by - ay) * (sx - ax)


def setup(vertices, faces, view, size, face_mask=None, near=1e-3, cull_back=False):
    """Steps 1 to 6 for every triangle of one view: dict(keep [T], X, Y int64 [T, 3], iz float32 [T, 3], cam [T, 3, 3], A int64 > 0,
    neg, area (the raw signed A), box int64 [T, 4] = x0, x1, y0, y1 inclusive)."""
    H, W = size
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    Nv = np.asarray(vertices).reshape(-1, 3).shape[0]
    inb = ((faces >= 0) & (faces < Nv)).all(1)
    f = np.where(inb[:, None], faces, 0)
    if Nv == 0:
        vertices = np.full((1, 3), np.nan, dtype=F)                                 # something to gather from; no index is in bounds
    ok, cam, iz, X, Y = project_vertices(vertices, view, near)
    keep = inb & ok[f].all(1)
    if face_mask is not None:
        keep &= np.asarray(face_mask).reshape(-1).astype(bool)
    X, Y = X[f], Y[f]
    area = edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    keep &= area != 0
    if cull_back:
        keep &= ~(area > 0)
    box = np.stack([np.maximum(0, (X.min(1) + 255) >> 8), np.minimum(W - 1, X.max(1) >> 8),
                    np.maximum(0, (Y.min(1) + 255) >> 8), np.minimum(H - 1, Y.max(1) >> 8)], 1)
    return dict(keep=keep, X=X, Y=Y, iz=iz[f], cam=cam[f], A=np.abs(area), neg=area < 0, area=area, box=box)


def weights(s, t, x, y):
    """(covered, w float32 [n, 3], zc float32 [n]) of triangles t (array or scalar) at pixels (x, y) (arrays)."""
    X, Y = s["X"][t], s["Y"][t]
    sx, sy = np.asarray(x, dtype=np.int64) * 256, np.asarray(y, dtype=np.int64) * 256
    col = lambda a, k: a[..., k]
    E = np.stack([edge(col(X, 1), col(Y, 1), col(X, 2), col(Y, 2), sx, sy), edge(col(X, 2), col(Y, 2), col(X, 0), col(Y, 0), sx, sy),
                  edge(col(X, 0), col(Y, 0), col(X, 1), col(Y, 1), sx, sy)], -1)
    E = np.where(np.asarray(s["neg"][t])[..., None], -E, E)
    covered = (E >= 0).all(-1)
    with np.errstate(all="ignore"):
        w = (E.astype(np.float64) / np.asarray(s["A"][t], dtype=np.float64)[..., None]).astype(F)
        iz = s["iz"][t]
        q = ((w[..., 0] * col(iz, 0)) + (w[..., 1] * col(iz, 1))) + (w[..., 2] * col(iz, 2))
        zc = (F(1) / q).astype(F)
    return covered, w, zc


def candidates(s, t):
    """(pixel x, pixel y, zc) of what triangle t writes: steps 6 and 7."""
    x0, x1, y0, y1 = s["box"][t]
    if not s["keep"][t] or x0 > x1 or y0 > y1:
        e = np.zeros(0, dtype=np.int64)
        return e, e, np.zeros(0, dtype=F)
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    xx, yy = xx.reshape(-1), yy.reshape(-1)
    covered, _, zc = weights(s, t, xx, yy)
    m = covered & (zc > 0)
    return xx[m], yy[m], zc[m]


def raster(keys, vertices, faces, views, face_mask=None, near=1e-3, cull_back=False, id_base=0):
    """keys uint64 [V, H, W] (rr.splat's, or all EMPTY) with every triangle's candidates merged in by the minimum."""
    keys = keys.copy()
    V, H, W = keys.shape
    for vi in range(V):
        s = setup(vertices, faces, views[vi], (H, W), face_mask, near, cull_back)
        flat = keys[vi].reshape(-1)
        for t in np.nonzero(s["keep"])[0]:
            x, y, zc = candidates(s, t)
            k = (zc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(id_base + t)
            pix = y * W + x
            flat[pix] = np.minimum(flat[pix], k)                                    # one triangle names a pixel once
    return keys


def vertex_colors(colors, mesh_color, Nv):
    """float32 [Nv, 3]: uint8 rgba as u8 / 255, float as given, None as the uniform colour."""
    if colors is None:
        return np.tile(np.asarray(mesh_color, dtype=F), (Nv, 1))
    colors = np.asarray(colors)
    if colors.dtype == np.uint8:
        return colors[:, :3].astype(F) / F(255)
    return colors.astype(F)


def resolve(keys, point_colors, N, vertices, faces, views, colors=None, mesh_color=(0.7, 0.7, 0.7), shade=0.0, near=1e-3,
            background=(1, 1, 1)):
    """(rgb uint8 [V, H, W, 3], depth float32, index int32, face int32 [V, H, W]) of keys drawn with id_base = N."""
    V, H, W = keys.shape
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    T, Nv = len(faces), np.asarray(vertices).reshape(-1, 3).shape[0]
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hit = keys != EMPTY
    is_pt = hit & (ids < N)
    is_tri = hit & (ids >= N) & (ids - N < T)
    depth = np.where(is_pt | is_tri, (keys >> np.uint64(32)).astype(np.uint32).view(F), F(0)).astype(F)
    col = np.tile(np.asarray(background, dtype=F), (V, H, W, 1))
    if N:
        col[is_pt] = np.asarray(point_colors, dtype=F).reshape(-1, 3)[ids[is_pt]]
    vc = vertex_colors(colors, mesh_color, Nv)
    shade = F(shade)
    for vi in range(V):
        y, x = np.nonzero(is_tri[vi])
        if len(y) == 0:
            continue
        t = ids[vi, y, x] - N
        s = setup(vertices, faces, views[vi], (H, W), None, near, False)
        covered, w, zr = weights(s, t, x, y)
        assert s["keep"][t].all() and covered.all() and (zr > 0).all()              # a triangle key sits only where the raster wrote it
        d = depth[vi, y, x]
        with np.errstate(all="ignore"):
            b = (w * s["iz"][t]) * d[:, None]
            c = vc[faces[t]]                                                        # [n, 3 vertices, 3 channels]
            out = (b[:, 0, None] * c[:, 0] + b[:, 1, None] * c[:, 1]) + b[:, 2, None] * c[:, 2]
            if shade > 0:
                cam = s["cam"][t]
                e1, e2 = cam[:, 1] - cam[:, 0], cam[:, 2] - cam[:, 0]
                nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
                ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
                nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
                len2 = (nx * nx + ny * ny) + nz * nz
                lam = np.where(len2 > 0, np.abs(nz) / np.sqrt(len2), F(0)).astype(F)
                g = (F(1) - shade) + shade * lam
                out = out * g[:, None]
        col[vi, y, x] = out.astype(F)
    return (rr.quantise(col), depth, np.where(is_pt, ids, -1).astype(np.int32), np.where(is_tri, ids - N, -1).astype(np.int32))


def render(vertices, faces, cams2world, K, size, colors=None, mesh_color=(0.7, 0.7, 0.7), shade=0.0, cull_back=False, face_mask=None,
           points=None, point_colors=None, mask=None, radius=None, sources=None, max_size=9, fill=0, near=1e-3, background=(1, 1, 1)):
    """geo4d_amd.render.render_mesh on numpy arrays: splat, fill, raster, resolve."""
    H, W = size
    views = rr.views_of(cams2world, K)
    N = 0
    keys = np.full((len(views), H, W), EMPTY, dtype=np.uint64)
    if points is not None:
        points = np.asarray(points, dtype=F)
        n_img = points.shape[0] if points.ndim > 2 else 1
        N = points.reshape(-1, 3).shape[0]
        if sources is None:
            sources = [list(range(n_img))] * len(views)
        keys = rr.fill(rr.splat(points, views, sources, N // n_img, size, mask, radius, near, max_size), fill)
    keys = raster(keys, vertices, faces, views, face_mask, near, cull_back, N)
    rgb, depth, index, face = resolve(keys, point_colors, N, vertices, faces, views, colors, mesh_color, shade, near, background)
    return dict(rgb=rgb, depth=depth, index=index, face=face, keys=keys)
