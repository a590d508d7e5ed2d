"""The renderer of geo4d_amd/csrc/render.hip restated in numpy (helper of tests/test_render_cpu.py, tests/test_render_gpu.py and
tools/render_bench.py): float32 arithmetic in the documented op order, every (pixel, point) candidate listed, one lexsort by
(pixel, depth bits, id), first entry per pixel. No GPU, no geo4d_amd import."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
F = np.float32


def views_of(cams2world, K):
    """[V, 16] float32: rows 0..2 of inv(cams2world) (fp64 4x4 algebra), then fx, fy, cx, cy."""
    w2c = np.linalg.inv(np.asarray(cams2world, dtype=np.float64).reshape(-1, 4, 4))
    K = np.asarray(K, dtype=np.float64).reshape(-1, 3, 3)
    return np.concatenate([w2c[:, :3, :].reshape(-1, 12), K[:, 0, 0:1], K[:, 1, 1:2], K[:, 0, 2:3], K[:, 1, 2:3]], 1).astype(F)


def project(points, view, ids, mask=None, radius=None, near=1e-3, max_size=9, ulp=(0, 0)):
    """Per listed point id: (keep, u, v, zc, s) in float32, the kernel's op order. ulp = (du, dv) moves u / v by that many float32 steps
    (the seed check of the GPU test)."""
    M = np.asarray(view, dtype=F)
    P = np.asarray(points, dtype=F).reshape(-1, 3)[ids]
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        cam = [((M[4 * r] * X + M[4 * r + 1] * Y) + M[4 * r + 2] * Z) + M[4 * r + 3] for r in range(3)]
        xc, yc, zc = cam
        keep = np.isfinite(P).all(1) & np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc)
        if mask is not None:
            keep &= np.asarray(mask).reshape(-1)[ids].astype(bool)
        keep &= ~(zc <= F(near))
        u = M[12] * (xc / zc) + M[14]
        v = M[13] * (yc / zc) + M[15]
        for arr, d in ((u, ulp[0]), (v, ulp[1])):
            for _ in range(abs(d)):
                arr[...] = np.nextafter(arr, F(np.inf if d > 0 else -np.inf))
        s = np.ones(len(ids), dtype=np.int64)
        if radius is not None:
            sf = np.ceil(F(2) * np.asarray(radius, dtype=F).reshape(-1)[ids] * M[12] / zc)
            s = np.where(sf >= F(max_size), max_size, np.where(sf >= F(1), np.nan_to_num(sf, nan=1.0, posinf=1.0, neginf=1.0), 1)).astype(np.int64)
    return keep, u, v, zc, s


def _start(u, s, size):
    """(ok, first pixel) along one axis: floor(u - 0.5 (s - 1) + 0.5), decided in float32 before the cast."""
    with np.errstate(all="ignore"):
        c0 = np.floor(u - F(0.5) * (s - 1).astype(F) + F(0.5))
        ok = (c0 < F(size)) & (c0 + s.astype(F) > F(0))
    return ok, np.where(ok, c0, 0).astype(np.int64)


def splat(points, views, sources, pts_per_image, size, mask=None, radius=None, near=1e-3, max_size=9, ulp=(0, 0)):
    """uint64 keys [V, H, W] (EMPTY where nothing landed): sources = per view the list of source images."""
    H, W = size
    out = np.full((len(views), H * W), EMPTY, dtype=np.uint64)
    for vi, view in enumerate(views):
        if len(sources[vi]) == 0:
            continue
        ids = np.concatenate([np.arange(s * pts_per_image, (s + 1) * pts_per_image, dtype=np.int64) for s in sources[vi]])
        keep, u, v, zc, s = project(points, view, ids, mask, radius, near, max_size, ulp)
        okx, x0 = _start(u, s, W)
        oky, y0 = _start(v, s, H)
        keep &= okx & oky
        ids, x0, y0, s, zc = ids[keep], x0[keep], y0[keep], s[keep], zc[keep]
        bits = zc.astype(F).view(np.uint32).astype(np.uint64)
        pix, cid, cbits = [], [], []
        for dy in range(int(s.max()) if len(s) else 0):
            for dx in range(int(s.max())):
                x, y = x0 + dx, y0 + dy
                m = (dx < s) & (dy < s) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
                pix.append((y * W + x)[m]); cid.append(ids[m]); cbits.append(bits[m])
        if not pix:
            continue
        pix, cid, cbits = np.concatenate(pix), np.concatenate(cid), np.concatenate(cbits)
        order = np.lexsort((cid, cbits, pix))
        pix, cid, cbits = pix[order], cid[order], cbits[order]
        first = np.ones(len(pix), dtype=bool)
        first[1:] = pix[1:] != pix[:-1]
        out[vi, pix[first]] = (cbits[first] << np.uint64(32)) | cid[first].astype(np.uint64)
    return out.reshape(len(views), H, W)


def fill(keys, passes):
    """`passes` times: an empty pixel takes the minimum key of its 3 x 3 neighbours inside its view."""
    keys = keys.copy()
    V, H, W = keys.shape
    for _ in range(passes):
        pad = np.full((V, H + 2, W + 2), EMPTY, dtype=np.uint64)
        pad[:, 1:-1, 1:-1] = keys
        best = np.minimum.reduce([pad[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
        keys = np.where(keys == EMPTY, best, keys)
    return keys


def quantise(c):
    """float RGB in [0, 1] -> uint8: clip(c * 255 + 0.5, 0, 255) truncated, in float32 (ops.scene_points' rounding)."""
    return np.clip(np.asarray(c, dtype=F) * F(255) + F(0.5), 0, 255).astype(np.uint8)


def resolve(keys, colors, background=(1, 1, 1)):
    """(rgb uint8 [V, H, W, 3], depth float32 [V, H, W], index int32 [V, H, W])."""
    hit = keys != EMPTY
    idx = np.where(hit, keys & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F), F(0)).astype(F)
    rgb = np.where(hit[..., None], quantise(np.asarray(colors).reshape(-1, 3))[idx], quantise(background))
    return rgb.astype(np.uint8), depth, np.where(hit, idx, -1).astype(np.int32)


def render(points, colors, cams2world, K, size, mask=None, radius=None, sources=None, near=1e-3, max_size=9, fill_passes=0,
           background=(1, 1, 1), ulp=(0, 0)):
    """geo4d_amd.render.render_points on numpy arrays; points [n_img, ..., 3] (or [N, 3] = one image)."""
    points = np.asarray(points, dtype=F)
    n_img = points.shape[0] if points.ndim > 2 else 1
    N = points.reshape(-1, 3).shape[0]
    views = views_of(cams2world, K)
    if sources is None:
        sources = [list(range(n_img))] * len(views)
    keys = fill(splat(points, views, sources, N // n_img, size, mask, radius, near, max_size, ulp), fill_passes)
    rgb, depth, index = resolve(keys, colors, background)
    return dict(rgb=rgb, depth=depth, index=index, keys=keys)
