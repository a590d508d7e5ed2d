"""The fusion rule of geo4d_amd/csrc/fuse.hip restated in numpy (helper of tests/test_fusion_cpu.py, tests/test_fusion_gpu.py and
tools/fusion_bench.py): float32 arithmetic in the documented op order, np.unique on the voxel keys, int64 np.add.at for the per-voxel
sums, float64 for the final position. No GPU, no geo4d_amd import.

Which points take part: point i takes part iff mask[i], X, Y, Z are finite, its weight w (when given) is finite and > 0, and per axis
  the cell c = floor(X / v) satisfies |c| < 2^20. A point that fails only the last condition is counted in `dropped`.
Voxel key: (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20); key order is lexicographic (cx, cy, cz) order, the output order.
Per point: q_a = (int)clamp(floor((X_a - c_a v) / v * 65536 + 0.5), 0, 65535) (clamped as a float, then cast),
  wq = (int)clamp(floor(w * 128 + 0.5), 1, 32767); without weights w = 1.
Per voxel, integer sums: count, sw = sum wq, sq_a = sum wq q_a, sc_k = sum wq rgba_k (k = 0..2).
mean: pos_a = float32((float64(c_a) + float64(sq_a) / (float64(sw) * 65536)) * float64(v)); colour (sc_k + sw // 2) // sw, alpha 255;
  weight float32(float64(sw) / (128 * count)).
best: the input point of highest weight, the lowest row on ties, copied bit for bit; count is still the voxel's count.
min_count = k: voxels with count < k are left out, after the reduction."""
import numpy as np

F = np.float32
LIMIT = 1 << 20


def cells(points, voxel):
    """float32 [N, 3] cell indices floor(X / v) (NaN / inf where the division gives them)."""
    with np.errstate(all="ignore"):
        return np.floor(np.asarray(points, dtype=F) / F(voxel)).astype(F)


def taking_part(points, weight, mask, voxel):
    """(part [N] bool, dropped int): the points that take part, and how many fail only the cell range."""
    points = np.asarray(points, dtype=F).reshape(-1, 3)
    ok = np.ones(len(points), dtype=bool) if mask is None else np.asarray(mask, dtype=bool).copy()
    ok &= np.isfinite(points).all(1)
    if weight is not None:
        w = np.asarray(weight, dtype=F)
        with np.errstate(invalid="ignore"):
            ok &= np.isfinite(w) & (w > 0)
    with np.errstate(invalid="ignore"):
        inside = (np.abs(cells(points, voxel)) < F(LIMIT)).all(1)
    return ok & inside, int((ok & ~inside).sum())


def quantise(points, weight, voxel):
    """(c int64 [N, 3], q int64 [N, 3], wq int64 [N]) of taking-part points."""
    points, v = np.asarray(points, dtype=F), F(voxel)
    c = cells(points, voxel)
    q = np.floor((points - c * v) / v * F(65536) + F(0.5))
    q = np.clip(q, F(0), F(65535)).astype(np.int64)
    w = np.ones(len(points), dtype=F) if weight is None else np.asarray(weight, dtype=F)
    with np.errstate(over="ignore"):
        wq = np.clip(np.floor(w * F(128) + F(0.5)), F(1), F(32767)).astype(np.int64)
    return c.astype(np.int64), q, wq


def fuse(points, rgba=None, weight=None, mask=None, *, voxel, reduce="mean", min_count=1):
    """dict(points float32 [M, 3], rgba uint8 [M, 4] or None, weight float32 [M], count int32 [M], dropped int, sums): the rule above.
    `sums` = dict(key, sw, sq, sc) of the voxels before min_count, for the tests that compare the integer sums."""
    assert reduce in ("mean", "best") and min_count >= 1 and np.isfinite(F(voxel)) and F(voxel) > 0
    points = np.asarray(points, dtype=F).reshape(-1, 3)
    part, dropped = taking_part(points, weight, mask, voxel)
    rows = np.nonzero(part)[0]
    P = points[rows]
    W = None if weight is None else np.asarray(weight, dtype=F)[rows]
    C = None if rgba is None else np.asarray(rgba, dtype=np.uint8)[rows]
    c, q, wq = quantise(P, W, voxel)
    key = ((c[:, 0] + LIMIT) << 42) | ((c[:, 1] + LIMIT) << 21) | (c[:, 2] + LIMIT)
    ukey, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    M = len(ukey)
    count = np.zeros(M, dtype=np.int64)
    sw = np.zeros(M, dtype=np.int64)
    sq = np.zeros((M, 3), dtype=np.int64)
    sc = np.zeros((M, 3), dtype=np.int64)
    np.add.at(count, inv, 1)
    np.add.at(sw, inv, wq)
    np.add.at(sq, inv, wq[:, None] * q)
    if C is not None:
        np.add.at(sc, inv, wq[:, None] * C[:, :3].astype(np.int64))
    uc = np.stack([(ukey >> 42) - LIMIT, ((ukey >> 21) & 0x1fffff) - LIMIT, (ukey & 0x1fffff) - LIMIT], 1)
    if reduce == "mean":
        pos = ((uc.astype(np.float64) + sq.astype(np.float64) / (sw.astype(np.float64) * 65536.0)[:, None]) * np.float64(F(voxel))).astype(F)
        col = None
        if C is not None:
            col = np.concatenate([((sc + (sw // 2)[:, None]) // sw[:, None]).astype(np.uint8), np.full((M, 1), 255, dtype=np.uint8)], 1)
        wout = (sw.astype(np.float64) / (128.0 * count.astype(np.float64))).astype(F)
    else:
        wf = np.ones(len(rows), dtype=F) if W is None else W
        order = np.lexsort((rows, -wf.astype(np.float64), inv))          # by voxel, then weight falling, then row rising
        first = order[np.concatenate([[True], inv[order][1:] != inv[order][:-1]])] if len(order) else order
        pos, wout = P[first], wf[first]
        col = None if C is None else C[first]
    keep = count >= min_count
    return dict(points=pos[keep].reshape(-1, 3), rgba=None if col is None else col[keep].reshape(-1, 4), weight=wout[keep],
                count=count[keep].astype(np.int32), dropped=dropped, sums=dict(key=ukey, sw=sw, sq=sq, sc=sc, count=count))


def excusable(points, voxel, rows=None):
    """bool per point of `rows` (None: all): within 1e-4 * voxel of a cell boundary on some axis - the only input points whose cell the
    device might decide differently from this restatement."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    p = p if rows is None else p[rows]
    with np.errstate(all="ignore"):
        t = p / np.float64(F(voxel))
        return (np.abs(t - np.round(t)) < 1e-4).any(1)


def default_voxel(depth, focal, mask=None):
    """2 * the lower median of depth / focal in float32 over `mask` (geo4d_amd.fusion.default_voxel): depth [n, H, W], focal [n]."""
    r = np.asarray(depth, dtype=F) / np.asarray(focal, dtype=F).reshape(-1, 1, 1)
    r = np.sort(r.reshape(-1) if mask is None else r[np.asarray(mask, dtype=bool)])
    return 2.0 * float(r[(len(r) - 1) // 2])
