"""The nearest-neighbour rule of include/geo4d_hip.h (geo4d_amd/csrc/nearest.hip), the cloud metrics and the radius outlier rule built
on it, restated in numpy. All float arithmetic is float32 in the kernel's written order (numpy rounds every operation, as the kernel
does with contraction off), so the device is compared with this by np.array_equal.

Rule: the cell side is r; a point's cell is floor(X / r) per axis and takes part iff |c| < 2^20 on every axis. A point takes part iff
its mask is set, its coordinates are finite and its cell takes part; one that fails only the last is counted in `dropped`. The
candidates of a query are the taking-part reference rows whose integer cell differs from the query's by at most 1 on every axis
(without its own row when exclude_same_row). d2 = (dx dx + dy dy) + dz dz with dx = Qx - Rx; j is within iff d2 <= r * r. count = the
candidates within; index = the one with the smallest (d2, j), or -1; dist2 = its d2, or +inf. A query that takes no part gets
(-1, +inf, 0)."""
import numpy as np

F = np.float32
LIMIT = 1 << 20
CHUNK = 512


def cells(points, r):
    """float32 [N, 3]: floor(X / r), the division in float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor(np.asarray(points, dtype=F).reshape(-1, 3) / F(r))


def taking_part(points, mask, r):
    """(takes part bool [N], dropped int, integer cells int64 [N, 3] (0 where the point takes no part))."""
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    ok = np.ones(len(p), bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    ok = ok & np.isfinite(p).all(1)
    c = cells(p, r)
    with np.errstate(invalid="ignore"):
        inside = (np.abs(c) < F(LIMIT)).all(1)
    dropped = int((ok & ~inside).sum())
    ok = ok & inside
    return ok, dropped, np.where(ok[:, None], c, 0).astype(np.int64)


def query(reference, points, r, *, reference_mask=None, query_mask=None, exclude_same_row=False, cell_free=False):
    """dict(index int32 [Nq], dist2 float32 [Nq], count int32 [Nq], dropped_reference, dropped_query). cell_free: the candidates are
    every taking-part reference row (rule 7's other definition), the cells deciding only who takes part."""
    R, Q = np.asarray(reference, dtype=F).reshape(-1, 3), np.asarray(points, dtype=F).reshape(-1, 3)
    r = F(r)
    r2 = r * r
    r_ok, r_drop, r_cell = taking_part(R, reference_mask, r)
    q_ok, q_drop, q_cell = taking_part(Q, query_mask, r)
    index, dist2, count = np.full(len(Q), -1, np.int32), np.full(len(Q), np.inf, F), np.zeros(len(Q), np.int32)
    rows = np.flatnonzero(r_ok)
    Rt, Rc = R[rows], r_cell[rows]
    if len(rows):
        for s in range(0, len(Q), CHUNK):
            q, qc, ok = Q[s:s + CHUNK], q_cell[s:s + CHUNK], q_ok[s:s + CHUNK]
            with np.errstate(invalid="ignore", over="ignore"):
                dx, dy, dz = (q[:, None, a] - Rt[None, :, a] for a in range(3))
                d2 = (dx * dx + dy * dy) + dz * dz
                within = d2 <= r2
            cand = ok[:, None] & np.ones(len(rows), bool)[None, :]
            if not cell_free:
                cand = cand & (np.abs(qc[:, None, :] - Rc[None, :, :]) <= 1).all(2)
            if exclude_same_row:
                cand = cand & (rows[None, :] != np.arange(s, s + len(q))[:, None])
            within = within & cand
            count[s:s + CHUNK] = within.sum(1)
            d = np.where(within, d2, F(np.inf))
            best = d.min(1)
            first = np.argmax(d == best[:, None], 1)                                # rows ascend, so the first minimum is the lowest row
            found = within.any(1)
            index[s:s + CHUNK] = np.where(found, rows[first], -1)
            dist2[s:s + CHUNK] = np.where(found, best, F(np.inf))
    return dict(index=index, dist2=dist2, count=count, dropped_reference=r_drop, dropped_query=q_drop)


def radius_outliers(points, r, min_neighbours, mask=None):
    """keep bool [N]: count >= min_neighbours with the cloud as its own reference and its own row left out."""
    return query(points, points, r, reference_mask=mask, query_mask=mask, exclude_same_row=True)["count"] >= int(min_neighbours)


def cloud_metrics(pred, gt, max_dist, thresholds=None, pred_mask=None, gt_mask=None):
    """The metrics rule: the truncated distances d = sqrt(dist2) (float32) if matched else max_dist, their float64 means, the integer
    counts within each threshold (dist2 <= t * t in float32), precision / recall / F-score."""
    r = F(max_dist)
    ts = [F(t) for t in ((max_dist,) if thresholds is None else thresholds)]
    out = {}
    for name, q, qm, ref, rm in (("pred", pred, pred_mask, gt, gt_mask), ("gt", gt, gt_mask, pred, pred_mask)):
        took = taking_part(q, qm, r)[0]
        nn = query(ref, q, r, reference_mask=rm, query_mask=qm)
        matched = nn["index"] >= 0
        d = np.where(matched, np.sqrt(np.where(matched, nn["dist2"], F(0))), r).astype(F)
        out[name] = dict(n=int(took.sum()), mean=float(d[took].astype(np.float64).mean()) if took.any() else float("nan"),
                         unmatched=int((took & ~matched).sum()), within=[int((matched & (nn["dist2"] <= t * t)).sum()) for t in ts],
                         dist=np.where(took, d, F(np.nan)).astype(F))
    P = [w / out["pred"]["n"] for w in out["pred"]["within"]]
    R = [w / out["gt"]["n"] for w in out["gt"]["within"]]
    return dict(n_pred=out["pred"]["n"], n_gt=out["gt"]["n"], accuracy=out["pred"]["mean"], completeness=out["gt"]["mean"],
                chamfer=0.5 * (out["pred"]["mean"] + out["gt"]["mean"]), within_pred=out["pred"]["within"], within_gt=out["gt"]["within"],
                precision=P, recall=R, fscore=[2 * p * q / (p + q) if p + q > 0 else 0.0 for p, q in zip(P, R)],
                unmatched_pred=out["pred"]["unmatched"], unmatched_gt=out["gt"]["unmatched"], pred_dist=out["pred"]["dist"],
                gt_dist=out["gt"]["dist"])


def near_the_shell(reference, points, r, rel=1e-5):
    """bool [Nq]: some finite reference point's float64 distance from the query lies within a relative `rel` of r: the only queries
    rule 7's comparison may excuse."""
    R, Q = np.asarray(reference, dtype=np.float64).reshape(-1, 3), np.asarray(points, dtype=np.float64).reshape(-1, 3)
    R = R[np.isfinite(R).all(1)]
    out = np.zeros(len(Q), bool)
    for s in range(0, len(Q), CHUNK):
        with np.errstate(invalid="ignore"):
            d = np.sqrt(((Q[s:s + CHUNK, None, :] - R[None, :, :]) ** 2).sum(2))
            out[s:s + CHUNK] = (np.abs(d - float(r)) <= rel * float(r)).any(1)
    return out


def rule7_inputs():
    """The six inputs of rule 7's comparison: (name, reference, query, r) with 3 000 x 3 000 points, r = 0.1 and 0.25: uniform in
    [-1, 1]^3, on the lattice 0.1 k and on the lattice 0.05 k."""
    out = []
    for r in (0.1, 0.25):
        g = np.random.default_rng(7)
        uniform = lambda: g.uniform(-1, 1, size=(3000, 3)).astype(F)
        lattice = lambda step, n: (g.integers(-n, n + 1, size=(3000, 3)).astype(F) * F(step)).astype(F)
        out += [("uniform", uniform(), uniform(), r), ("lattice 0.1", lattice(0.1, 10), lattice(0.1, 10), r),
                ("lattice 0.05", lattice(0.05, 20), lattice(0.05, 20), r)]
    return out
