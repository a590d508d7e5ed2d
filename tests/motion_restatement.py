"""The motion rule of geo4d_amd/csrc/motion.hip restated in numpy (helper of tests/test_motion_cpu.py, tests/test_motion_gpu.py and
tools/motion_bench.py): float32 arithmetic in the documented op order, vectorised over the pixels of one (image, voter) pair, plus the
synthetic scene the defaults were chosen on (a static wall, a sphere that crosses in front of it). No GPU, no geo4d_amd import."""
import numpy as np

F = np.float32
DEFAULTS = dict(radius=8, tol=0.05, min_votes=2, ratio=0.25)


def views_of(cams2world, K):
    """[n, 16] float32: rows 0..2 of inv(cams2world) (fp64 4x4 algebra), then fx, fy, cx, cy (geo4d_amd.scene_view.views_of)."""
    w2c = np.linalg.inv(np.asarray(cams2world, dtype=np.float64).reshape(-1, 4, 4))
    K = np.asarray(K, dtype=np.float64).reshape(-1, 3, 3)
    return np.concatenate([w2c[:, :3, :].reshape(-1, 12), K[:, 0, 0:1], K[:, 1, 1:2], K[:, 0, 2:3], K[:, 1, 2:3]], 1).astype(F)


def depth_range(depth, valid):
    """(dmin, dmax) float32 [n, H, W]: minimum / maximum of depth over the valid pixels of the 3 x 3 neighbourhood inside the image.
    A NaN depth never wins a comparison (fmin / fmax); a neighbourhood without a valid finite depth keeps (+inf, -inf)."""
    depth, valid = np.asarray(depth, dtype=F), np.asarray(valid, dtype=bool)
    n, H, W = depth.shape
    lo = np.full((n, H + 2, W + 2), np.inf, dtype=F)
    hi = np.full((n, H + 2, W + 2), -np.inf, dtype=F)
    lo[:, 1:-1, 1:-1] = np.where(valid, depth, F(np.inf))
    hi[:, 1:-1, 1:-1] = np.where(valid, depth, F(-np.inf))
    dmin = np.fmin.reduce([lo[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    dmax = np.fmax.reduce([hi[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return dmin.astype(F), dmax.astype(F)


def project(P, M):
    """World points P [N, 3] float32 through view floats M [16]: (xc, yc, zc, u, v) float32 in the kernel's op order."""
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        xc, yc, zc = [((M[4 * r] * X + M[4 * r + 1] * Y) + M[4 * r + 2] * Z) + M[4 * r + 3] for r in range(3)]
        u = M[12] * (xc / zc) + M[14]
        v = M[13] * (yc / zc) + M[15]
    return xc, yc, zc, u, v


def pair_votes(P, M, dmin_j, dmax_j, valid_j, tol, near):
    """One voter j for the points P [N, 3] of another image: (voted [N] bool, cls [N] int: 0 consistent, 1 free, 2 occluded; undefined
    where not voted, zc, u, v, dmin * lo, dmax * hi at the pixel hit)."""
    H, W = valid_j.shape
    lo, hi = F(1) - F(tol), F(1) + F(tol)
    xc, yc, zc, u, v = project(P, M)
    with np.errstate(all="ignore"):
        ok = np.isfinite(P).all(1) & np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc > F(near))
        col, row = np.floor(u + F(0.5)), np.floor(v + F(0.5))
        ok &= (col >= 0) & (col < F(W)) & (row >= 0) & (row < F(H))                # in float, before any cast; NaN fails
        ci, ri = np.where(ok, col, 0).astype(np.int64), np.where(ok, row, 0).astype(np.int64)
        ok &= valid_j[ri, ci]
        a, b = dmin_j[ri, ci] * lo, dmax_j[ri, ci] * hi
        cls = np.where(zc < a, 1, np.where(zc > b, 2, 0))
    return ok, cls, zc, u, v, a, b


def votes(pts3d, depth, valid, views, radius=8, tol=0.05, near=1e-3, images=None):
    """uint8 [n, H, W, 3] = (consistent, free, occluded) counts of every pixel over the voters 0 < |j - i| <= radius. `images`: only
    these images' pixels are voted on (the others stay 0); tools/motion_bench.py times one."""
    pts3d, valid, views = np.asarray(pts3d, dtype=F), np.asarray(valid, dtype=bool), np.asarray(views, dtype=F)
    n, H, W, _ = pts3d.shape
    dmin, dmax = depth_range(depth, valid)
    out = np.zeros((n, H * W, 3), dtype=np.int64)
    for i in (range(n) if images is None else images):
        P = pts3d[i].reshape(-1, 3)
        own = valid[i].reshape(-1)
        for j in range(max(0, i - radius), min(n - 1, i + radius) + 1):
            if j == i:
                continue
            ok, cls = pair_votes(P, views[j], dmin[j], dmax[j], valid[j], tol, near)[:2]
            ok &= own
            for c in range(3):
                out[i, :, c] += ok & (cls == c)
    assert out.max() <= 254
    return out.reshape(n, H, W, 3).astype(np.uint8)


def dynamic_mask(v, min_votes=2, ratio=0.25):
    """bool [n, H, W]: free >= min_votes and free >= ratio (consistent + free), compared in float32."""
    c, f = v[..., 0].astype(F), v[..., 1].astype(F)
    return (f >= F(min_votes)) & (f >= F(ratio) * (c + f))


def segment(pts3d, depth, valid, cams2world, K, radius=8, tol=0.05, min_votes=2, ratio=0.25, near=1e-3):
    return dynamic_mask(votes(pts3d, depth, valid, views_of(cams2world, K), radius, tol, near), min_votes, ratio)


def excusable(pts3d, depth, valid, views, where, radius=8, tol=0.05, near=1e-3):
    """For the pixels `where` = (i, y, x) index arrays: True where some voter j of the pixel projects it within 1e-4 px of a rounding
    boundary, or sees zc within 4 ulp of dmin * lo or dmax * hi - the only pixels on which the device may differ from `votes`."""
    pts3d, valid, views = np.asarray(pts3d, dtype=F), np.asarray(valid, dtype=bool), np.asarray(views, dtype=F)
    n = len(pts3d)
    dmin, dmax = depth_range(depth, valid)
    out = []
    for i, y, x in zip(*where):
        P = pts3d[i, y, x][None]
        ok_any = False
        for j in range(max(0, i - radius), min(n - 1, i + radius) + 1):
            if j == i:
                continue
            _, _, zc, u, v, a, b = pair_votes(P, views[j], dmin[j], dmax[j], valid[j], tol, near)
            with np.errstate(all="ignore"):
                edge = np.array([u[0] + F(0.5), v[0] + F(0.5)], dtype=np.float64)
                near_edge = bool((np.abs(edge - np.round(edge)) < 1e-4).any())
                near_bound = bool(np.abs(zc[0] - a[0]) <= 4 * np.spacing(np.abs(a[0])) or np.abs(zc[0] - b[0]) <= 4 * np.spacing(np.abs(b[0])))
            ok_any |= near_edge or near_bound
        out.append(ok_any)
    return out


# ---- the synthetic scene -----------------------------------------------------------------------------------------------------------------
def synthetic_scene(noise=0.0, n=12, H=48, W=64, band=False):
    """A static wall (the plane -0.2 x + z = 4) and a sphere of radius 0.5 whose centre is (-0.8 + 0.15 i, 0.1, 2.5) at frame i, seen by
    n cameras with f = 60 and the principal point at (W/2, H/2): camera i sits at (0.03 i, 0.01 i, 0), turned about y by 0.02 i.
    Everything in float64; depth (= the ray parameter of the nearest hit along R ((x - cx) / f, (y - cy) / f, 1), i.e. camera z),
    times 1 + noise * N(0, 1) of default_rng(0), and the world points on those rays are cast to float32 at the end. `truth` marks the
    pixels whose ray hits the sphere first. band: valid is False, and depth and points are NaN, in columns < 5 and rows >= 40."""
    f, cx, cy = 60.0, W / 2, H / 2
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(xs - cx) / f, (ys - cy) / f, np.ones_like(xs)], -1)
    c2w = np.tile(np.eye(4), (n, 1, 1))
    depth = np.empty((n, H, W))
    truth = np.zeros((n, H, W), dtype=bool)
    dirs = np.empty((n, H, W, 3))
    normal = np.array([-0.2, 0.0, 1.0])
    for i in range(n):
        a = 0.02 * i
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        c = np.array([0.03 * i, 0.01 * i, 0.0])
        c2w[i, :3, :3], c2w[i, :3, 3] = R, c
        d = ray @ R.T
        dirs[i] = d
        t_wall = (4.0 - normal @ c) / (d @ normal)
        s = np.array([-0.8 + 0.15 * i, 0.1, 2.5])
        qa, qb, qc = (d * d).sum(-1), 2 * (d @ (c - s)), (c - s) @ (c - s) - 0.25
        disc = qb * qb - 4 * qa * qc
        with np.errstate(invalid="ignore"):
            t_sph = np.where(disc > 0, (-qb - np.sqrt(np.maximum(disc, 0))) / (2 * qa), np.inf)
        t_sph = np.where(t_sph > 0, t_sph, np.inf)
        truth[i] = t_sph < t_wall
        depth[i] = np.minimum(t_sph, t_wall)
    if noise:
        depth = depth * (1 + noise * np.random.default_rng(0).standard_normal((n, H, W)))
    pts3d = c2w[:, None, None, :3, 3] + depth[..., None] * dirs
    valid = np.ones((n, H, W), dtype=bool)
    if band:                                                       # an invalid band: the first five columns and the rows from 40 on
        valid[:, :, :5] = False
        valid[:, 40:, :] = False
        depth = np.where(valid, depth, np.nan)
        pts3d = np.where(valid[..., None], pts3d, np.nan)
    K = np.tile(np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]]), (n, 1, 1))
    return dict(pts3d=pts3d.astype(F), depth=depth.astype(F), valid=valid, cams2world=c2w, K=K, truth=truth, n=n, H=H, W=W)


def iou(a, b):
    return float((a & b).sum()) / max(float((a | b).sum()), 1.0)
