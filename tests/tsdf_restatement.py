"""The TSDF rule of geo4d_amd/csrc/tsdf.hip restated in numpy (helper of tests/test_tsdf_cpu.py, tests/test_tsdf_gpu.py): float32
arithmetic in the documented op order, np.unique for the marked set, one vectorised pass per image for the integration, np.searchsorted
for the neighbours. No GPU, no geo4d_amd import.

Inputs: pts3d [n, H, W, 3], depth [n, H, W], valid [n, H, W], views [n, 16] (motion_restatement.views_of), camera centres [n, 3], rgba
  [n, H, W, 4] u8 or None, weight [n, H, W] or None (every weight is 1), voxel v > 0, T in 1..8 with trunc = float32(T) * v, near >= 0,
  min_weight > 0.
1. Mark. Pixel (i, p) takes part iff it is valid, its point P and depth are finite and depth > near. d = P - C_i,
  s = (v * 0.5) / depth; for k = -2T .. 2T the sample is P_a + (float32(k) * s) * d_a and its cell floor(sample_a / v). A sample whose
  cell does not satisfy |c| < 2^20 on every axis is counted in `dropped`; the others' keys (cx + 2^20) << 42 | (cy + 2^20) << 21 |
  (cz + 2^20) form a set, K = its sorted content. `table_insert` replays the device's open-addressing table one key at a time.
2. Integrate. Voxel m has centre X_a = (float32(c_a) + 0.5) * v. For j = 0 .. n-1 in that order: xc = ((r00 X + r01 Y) + r02 Z) + t0,
  likewise yc, zc; skip unless all are finite and zc > near; u = fx (xc / zc) + cx, v likewise; column = floor(u + 0.5), row =
  floor(v + 0.5), inside / outside decided in float; skip unless j's pixel is valid, its depth finite and its weight w finite and > 0;
  sd = depth - zc; skip if sd < -trunc; t = min(1, sd / trunc); D += w * t; Wt += w; if sd <= trunc: C_k += w * float32(rgba_k),
  Wc += w. f = D / Wt; colour uint8(clip(floor(C_k / Wc + 0.5), 0, 255)), 0 when Wc == 0; alpha 255.
3. Extract. A voxel is live iff Wt >= min_weight and |f| < 1. For each live m and axis a = 0, 1, 2 with a live neighbour m' at cell
  c + e_a and (f >= 0) != (f' >= 0): one point at X_a + (f / (f - f')) * v on axis a (the centre's coordinates on the other two), the
  colour of the voxel of smaller |f| (m on ties), weight min(Wt, Wt'). Rows in (m, a) order."""
import numpy as np

import motion_restatement as mr

F = np.float32
LIMIT = 1 << 20
STEP = (1 << 42, 1 << 21, 1)
DEFAULTS = dict(trunc=4, min_weight=4.0, near=1e-3)


def centres_of(cams2world):
    """[n, 3] float32: the camera centres, column 3 of cams2world."""
    return np.asarray(cams2world, dtype=np.float64).reshape(-1, 4, 4)[:, :3, 3].astype(F)


def taking_part(pts3d, depth, valid, near):
    """bool [n, H, W]: valid, point and depth finite, depth > near."""
    pts3d, depth = np.asarray(pts3d, dtype=F), np.asarray(depth, dtype=F)
    with np.errstate(invalid="ignore"):
        return np.asarray(valid, dtype=bool) & np.isfinite(pts3d).all(-1) & np.isfinite(depth) & (depth > F(near))


def default_capacity(taking):
    """The power of two at or above 4 x the taking-part pixels."""
    return 1 << max(4 * int(taking) - 1, 0).bit_length()


def samples(pts3d, depth, valid, centres, voxel, T, near):
    """(S float32 [N, 4T + 1, 3]: the samples of the N taking-part pixels in (image, pixel) order, cells float32 likewise)."""
    pts3d, depth, centres, v = np.asarray(pts3d, dtype=F), np.asarray(depth, dtype=F), np.asarray(centres, dtype=F), F(voxel)
    part = taking_part(pts3d, depth, valid, near)
    P = pts3d[part]
    img = np.nonzero(part)[0]
    d = P - centres[img]
    s = (v * F(0.5)) / depth[part]
    k = np.arange(-2 * T, 2 * T + 1).astype(F)
    with np.errstate(all="ignore"):
        S = P[:, None, :] + (k[None, :] * s[:, None])[:, :, None] * d[:, None, :]
        return S.astype(F), np.floor(S / v).astype(F)


def keys_of(cells):
    c = cells.astype(np.int64)
    return ((c[..., 0] + LIMIT) << 42) | ((c[..., 1] + LIMIT) << 21) | (c[..., 2] + LIMIT)


def cells_of(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return np.stack([(keys >> 42) - LIMIT, ((keys >> 21) & 0x1fffff) - LIMIT, (keys & 0x1fffff) - LIMIT], -1)


def mark_keys(pts3d, depth, valid, centres, voxel, T, near):
    """(keys int64 [S]: the key of every in-range sample, in (image, pixel, k) order; dropped int)."""
    _, c = samples(pts3d, depth, valid, centres, voxel, T, near)
    c = c.reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        inside = (np.abs(c) < F(LIMIT)).all(1)                                       # NaN fails
    return keys_of(c[inside]), int((~inside).sum())


def mark(pts3d, depth, valid, centres, voxel, T, near):
    """(K int64 [M] sorted, dropped int): the marked set."""
    keys, dropped = mark_keys(pts3d, depth, valid, centres, voxel, T, near)
    return np.unique(keys), dropped


def mix64(h):
    m = (1 << 64) - 1
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & m
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & m
    h ^= h >> 33
    return h


def table_insert(keys, capacity):
    """The device's table replayed one sample at a time, in the order given: linear probing from mix64(key) & (capacity - 1), at most
    `capacity` probes. (occupied keys sorted int64, overflow = the samples that found no home)."""
    assert capacity >= 1 and capacity & (capacity - 1) == 0
    uniq, first, counts = np.unique(np.asarray(keys, dtype=np.int64), return_index=True, return_counts=True)
    table, overflow = {}, 0
    for r in np.argsort(first, kind="stable"):                                       # repeats of a key probe the same way
        key = int(uniq[r])
        at = mix64(key) & (capacity - 1)
        for _ in range(capacity):
            seen = table.setdefault(at, key)
            if seen == key:
                break
            at = (at + 1) & (capacity - 1)
        else:
            overflow += int(counts[r])
    return np.array(sorted(table.values()), dtype=np.int64), overflow


def voxel_centres(K, voxel):
    return ((cells_of(K).astype(F) + F(0.5)) * F(voxel)).astype(F)


def observe(X, j, depth, valid, views, weight, trunc, near):
    """Image j seen from the voxel centres X [M, 3]: (ok [M] bool: the image adds to the voxel, row, col int64, w, sd, u, v float32)."""
    H, W = depth.shape[1:]
    xc, yc, zc, u, v = mr.project(X, views[j])
    with np.errstate(all="ignore"):
        ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc > F(near))
        col, row = np.floor(u + F(0.5)), np.floor(v + F(0.5))
        ok &= (col >= 0) & (col < F(W)) & (row >= 0) & (row < F(H))                  # in float, before any cast; NaN fails
        ci, ri = np.where(ok, col, 0).astype(np.int64), np.where(ok, row, 0).astype(np.int64)
        dj = depth[j][ri, ci]
        w = np.ones(len(X), dtype=F) if weight is None else weight[j][ri, ci]
        ok &= valid[j][ri, ci] & np.isfinite(dj) & np.isfinite(w) & (w > 0)
        sd = dj - zc
        ok &= ~(sd < -trunc)
    return ok, ri, ci, w, sd, u, v


def integrate(K, depth, valid, views, rgba, weight, voxel, T, near):
    """(f float32 [M], Wt float32 [M], col uint8 [M, 4] or None) of the voxels K."""
    depth, valid, views = np.asarray(depth, dtype=F), np.asarray(valid, dtype=bool), np.asarray(views, dtype=F)
    weight = None if weight is None else np.asarray(weight, dtype=F)
    trunc = F(T) * F(voxel)
    X = voxel_centres(K, voxel)
    M = len(K)
    D, Wt, Wc, C = np.zeros(M, F), np.zeros(M, F), np.zeros(M, F), np.zeros((M, 3), F)
    for j in range(len(depth)):
        ok, ri, ci, w, sd, _, _ = observe(X, j, depth, valid, views, weight, trunc, near)
        with np.errstate(all="ignore"):
            t = np.minimum(F(1), sd / trunc)
            D = np.where(ok, D + w * t, D).astype(F)
            Wt = np.where(ok, Wt + w, Wt).astype(F)
            if rgba is not None:
                inner = ok & (sd <= trunc)
                C = np.where(inner[:, None], C + w[:, None] * rgba[j][ri, ci, :3].astype(F), C).astype(F)
                Wc = np.where(inner, Wc + w, Wc).astype(F)
    with np.errstate(all="ignore"):
        f = (D / Wt).astype(F)
        col = None
        if rgba is not None:
            q = np.clip(np.floor(C / Wc[:, None] + F(0.5)), F(0), F(255))
            col = np.concatenate([np.where(Wc[:, None] > 0, q, 0).astype(np.uint8), np.full((M, 1), 255, np.uint8)], 1)
    return f, Wt, col


def live_of(f, Wt, min_weight):
    with np.errstate(invalid="ignore"):
        return (Wt >= F(min_weight)) & (np.abs(f) < F(1))                            # NaN (Wt = 0) fails


def extract(K, f, Wt, col, voxel, min_weight):
    """dict(points float32 [P, 3], rgba uint8 [P, 4] or None, weight float32 [P], m int64 [P], m2 int64 [P], axis int64 [P])."""
    v = F(voxel)
    live = live_of(f, Wt, min_weight)
    X = voxel_centres(K, voxel)
    c = cells_of(K)
    rows = []
    for a in range(3 if len(K) else 0):
        target = K + STEP[a]
        at = np.minimum(np.searchsorted(K, target), len(K) - 1)
        found = (c[:, a] + 1 < LIMIT) & (K[at] == target)                            # a carry out of the field is no neighbour
        hit = found & live & live[at] & ((f >= 0) != (f[at] >= 0))
        m = np.nonzero(hit)[0]
        rows.append(np.stack([m, np.full_like(m, a), at[m]], 1))
    rows = np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    m, a, m2 = rows[:, 0], rows[:, 1], rows[:, 2]
    pts = X[m].copy()
    with np.errstate(all="ignore"):
        pts[np.arange(len(m)), a] = X[m, a] + (f[m] / (f[m] - f[m2])) * v
    pick = np.where(np.abs(f[m2]) < np.abs(f[m]), m2, m)
    return dict(points=pts.astype(F), rgba=None if col is None else col[pick], weight=np.minimum(Wt[m], Wt[m2]).astype(F), m=m, m2=m2, axis=a)


def tsdf(pts3d, depth, valid, views, centres, rgba=None, weight=None, *, voxel, trunc=4, min_weight=4.0, near=1e-3, capacity=None):
    """The whole rule: dict(points, rgba, weight, voxels, dropped, overflow, K, f, Wt, col, m, m2, axis). `capacity`: None marks with
    np.unique; a power of two replays the table (table_insert) and reports its overflow."""
    assert 1 <= trunc <= 8 and int(trunc) == trunc and min_weight > 0 and near >= 0 and np.isfinite(F(voxel)) and F(voxel) > 0
    pts3d, depth, valid = np.asarray(pts3d, dtype=F), np.asarray(depth, dtype=F), np.asarray(valid, dtype=bool)
    if capacity is None:
        (K, dropped), overflow = mark(pts3d, depth, valid, centres, voxel, trunc, near), 0
    else:
        keys, dropped = mark_keys(pts3d, depth, valid, centres, voxel, trunc, near)
        K, overflow = table_insert(keys, capacity)
    f, Wt, col = integrate(K, depth, valid, views, rgba, weight, voxel, trunc, near)
    out = extract(K, f, Wt, col, voxel, min_weight)
    out.update(voxels=len(K), dropped=dropped, overflow=overflow, K=K, f=f, Wt=Wt, col=col)
    return out


def excusable(pts3d, depth, valid, views, centres, weight, K, *, voxel, trunc=4, near=1e-3):
    """bool [M]: the voxels of K on which the device may differ from this restatement: marked by a sample within 1e-4 voxel
    of a cell boundary (its cell and the cell across that boundary), or holding an observation projected within 1e-4 px of a rounding boundary or with sd within 4
    ulp of +-trunc."""
    depth, valid, views = np.asarray(depth, dtype=F), np.asarray(valid, dtype=bool), np.asarray(views, dtype=F)
    weight = None if weight is None else np.asarray(weight, dtype=F)
    S, c = samples(pts3d, depth, valid, centres, voxel, trunc, near)
    S, c = S.reshape(-1, 3).astype(np.float64), c.reshape(-1, 3)
    with np.errstate(all="ignore"):
        t = S / np.float64(F(voxel))
        edge = np.abs(t - np.round(t)) < 1e-4
        inside = (np.abs(c) < F(LIMIT)).all(1)
        side = np.where(np.round(t) <= c.astype(np.float64), -1, 1)                # the cell across the boundary the sample is near
    near_cells = set()
    for r in np.nonzero(edge.any(1) & inside)[0]:
        base = c[r].astype(np.int64)
        steps = [(0, int(side[r, a])) if edge[r, a] else (0,) for a in range(3)]
        for dx in steps[0]:
            for dy in steps[1]:
                for dz in steps[2]:
                    near_cells.add((base[0] + dx, base[1] + dy, base[2] + dz))
    out = np.array([tuple(x) in near_cells for x in cells_of(K)], dtype=bool) if near_cells else np.zeros(len(K), bool)
    tr = F(trunc) * F(voxel)
    X = voxel_centres(K, voxel)
    for j in range(len(depth)):
        ok, _, _, _, sd, u, v = observe(X, j, depth, valid, views, weight, tr, near)
        with np.errstate(all="ignore"):
            e = np.stack([u + F(0.5), v + F(0.5)], 1).astype(np.float64)
            px = (np.abs(e - np.round(e)) < 1e-4).any(1) & np.isfinite(e).all(1)
            bound = (np.abs(np.abs(sd) - tr) <= 4 * np.spacing(tr)) & np.isfinite(sd)
        out |= px | bound                                                           # also where the image did not add: it might on the device
    return out


# ---- the synthetic scene -----------------------------------------------------------------------------------------------------------------
def static_scene(noise=0.0, band=False, **tsdf_kw):
    """motion_restatement.synthetic_scene with its static part by the motion rule's defaults (`static`), the default voxel
    2 * median(depth / 60) over it, views, centres, random colours `rgba`, and `out` = the rule at the defaults (or `tsdf_kw`)."""
    s = mr.synthetic_scene(noise=noise, band=band)
    s["static"] = s["valid"] & ~mr.segment(s["pts3d"], s["depth"], s["valid"], s["cams2world"], s["K"])
    s["voxel"] = 2 * np.median(s["depth"][s["static"]] / 60)
    s["views"], s["centres"] = mr.views_of(s["cams2world"], s["K"]), centres_of(s["cams2world"])
    s["rgba"] = np.random.default_rng(8).integers(0, 256, size=(s["n"], s["H"], s["W"], 4), dtype=np.uint8)
    s["out"] = tsdf(s["pts3d"], s["depth"], s["static"], s["views"], s["centres"], s["rgba"], voxel=s["voxel"], **tsdf_kw)
    return s
