"""The device RANSAC-PnP backend without a GPU (csrc/pnp.hip, csrc/pnp_math.h, ops.pnp_ransac, pnp.sample_tables): the two C ABI entry
points in the header and the ctypes table, workspace sizes, argument errors raised before any device work, the sampler tables against
the solver's own stream, and the kernels' arithmetic - csrc/pnp_math.h compiled for the host (tests/pnp_math_host.cpp) and run serially -
against geo4d_amd/pnp.py hypothesis for hypothesis."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from geo4d_amd import pnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("geo4d_pnp_ransac_workspace", "geo4d_pnp_ransac")


def _up8(v):
    return (v + 7) // 8 * 8


def _workspace(B, C, H, W, I, maxp):
    """csrc/pnp.hip make_layout: hypotheses and refits (12 doubles each), sub-sampled points, then the int32 arrays, each padded to 8 bytes."""
    bc, hw = B * C, H * W
    chunks = min(max((hw + 4095) // 4096, 1), 64)
    return (bc * I * 96 + bc * 96 + B * maxp * 24 + _up8(B * hw * 4) + _up8(B * maxp * 4) + _up8(bc * I * 4) + _up8(B * 8) + _up8(bc * 4) +
            _up8(bc * chunks * 4))


def test_header_and_ctypes_table_agree_on_the_new_symbols():
    from geo4d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geo4d_hip.h")).read()
    assert int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 9     # symbols added, no struct changed
    lib = _lib.load()
    for name in NEW:
        m = re.search(r"\b(size_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/geo4d_hip.h"
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(m.group(2).split(",")), (name, m.group(2))
        assert (res is _lib.C.c_size_t) == (m.group(1) == "size_t")
        assert hasattr(lib, name)
    for shape in ((1, 3, 320, 512, 100, 4096), (16, 3, 24, 32, 50, 768), (4, 1, 3, 5, 7, 6), (2, 64, 48, 64, 60, 1024)):
        assert lib.geo4d_pnp_ransac_workspace(*shape) == _workspace(*shape), shape
    assert lib.geo4d_pnp_ransac_workspace(0, 3, 8, 8, 10, 64) == 0
    assert lib.geo4d_pnp_ransac_workspace(1, 65, 8, 8, 10, 64) == 0 and lib.geo4d_pnp_ransac_workspace(1, 3, 8, 8, 10, 5) == 0


def test_argument_errors_come_before_any_device_work():
    from geo4d_amd import _lib, ops
    lib = _lib.load()
    need = _workspace(1, 3, 2, 4, 8, 8)
    buf = (_lib.C.c_double * (need // 8 + 8))()
    p = _lib.C.addressof(buf)
    names = ("points", "ps", "conf", "cs", "thr", "cand", "ppx", "ppy", "reproj", "iters", "sample", "n", "m", "sub", "draws", "maxp", "B", "C", "H", "W",
             "focal", "c2w", "status", "info", "ws", "nbytes")
    good = dict(points=p, ps=24, conf=p, cs=8, thr=0.5, cand=p, ppx=2.0, ppy=1.0, reproj=5.0, iters=8, sample=6, n=p, m=p, sub=p, draws=p, maxp=8,
                B=1, C=3, H=2, W=4, focal=p, c2w=p, status=p, info=p, ws=p, nbytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.geo4d_pnp_ransac(*[a[k] for k in names], None)
    bads = [{k: None} for k in ("points", "conf", "cand", "n", "m", "sub", "draws", "focal", "c2w", "status", "info", "ws")]
    bads += [dict(B=0), dict(C=0), dict(C=65), dict(H=0), dict(W=0), dict(iters=0), dict(sample=5), dict(sample=7), dict(reproj=float("nan")),
             dict(thr=float("nan")), dict(maxp=5), dict(nbytes=need - 1), dict(ws=p + 4)]
    for bad in bads:
        assert call(**bad) == -22 and b"pnp_ransac" in lib.geo4d_last_error(), bad
    pts, conf = torch.zeros(1, 4, 6, 3), torch.ones(1, 4, 6)
    with pytest.raises(_lib.Geo4DNativeError):
        ops.pnp_ransac(pts, conf, torch.full((1, 3), 5.0, dtype=torch.float64), [pnp.sample_tables(24, 10)], iterations=10)


def _scene(n, seed):
    """tests/test_pnp_cpu.py's scene: exact projections under a known pose, 30 % of the pixels grossly displaced."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, 3)) * [2.0, 1.5, 1.0] + [0, 0, 5.0]
    ang = rng.uniform(-0.4, 0.4, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    R = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    t = rng.uniform(-0.5, 0.5, 3)
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    Xc = X @ R.T + t
    pix = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)
    bad = rng.choice(n, int(0.3 * n), replace=False)
    pix[bad] += rng.uniform(-200, 200, (len(bad), 2))
    return X, pix, K


@pytest.mark.parametrize("n", [5, 6, 300, 4096, 4097, 20000])
def test_the_tables_are_the_samplers_stream(n):
    X, pix, K = _scene(n, 1)
    want = pnp.solve_pnp_ransac(X, pix, K, iterations=40, reproj=5.0, seed=0)
    sub, draws = pnp.sample_tables(n, 40)
    got = pnp.solve_pnp_ransac(X, pix, K, iterations=40, reproj=5.0, seed=0, tables=(sub, draws))
    assert want[0] == got[0] == (n >= 300)                             # (5: too few points; 6 with an outlier: no consensus)
    if want[0]:
        assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2])
    assert np.array_equal(want[3], got[3])
    assert len(sub) == min(n, 4096) and np.all(np.diff(sub) > 0) and draws.shape == ((40, 6) if n >= 6 else (0, 6))
    assert pnp.sample_tables(n, 40)[0] is sub                           # cached by (n, iterations, seed, sample, max_points)
    if n >= 6:
        assert np.array_equal(pnp.sample_tables(n, 7)[1], draws[:7])    # a prefix of the same stream
        assert not np.array_equal(pnp.sample_tables(n, 40, seed=1)[1], draws)


def test_init_from_group_rejects_an_unknown_backend():
    from geo4d_amd.align import GroupAligner
    with pytest.raises(ValueError, match="pnp_backend"):
        GroupAligner.init_from_group(object.__new__(GroupAligner), None, pose_init="prefix", pnp_backend="bogus")


# ---- the kernels' arithmetic on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_solver(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pnp_math") / "pnp_math_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "geo4d_amd", "csrc"), os.path.join(ROOT, "tests", "pnp_math_host.cpp"), "-o", exe],
                   check=True, capture_output=True)

    def solve(Xs, pidx, draws, W, f, cx, cy, reproj):
        path = exe + ".in"
        with open(path, "wb") as fh:
            fh.write(struct.pack("<iii", len(Xs), W, len(draws)) + struct.pack("<dddd", f, cx, cy, reproj))
            fh.write(np.ascontiguousarray(Xs, "<f8").tobytes() + np.ascontiguousarray(pidx, "<i4").tobytes() + np.ascontiguousarray(draws, "<i4").tobytes())
        out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split("\n")
        ok, it, besti, sub_inl = (int(v) for v in out[0].split())
        v = np.array(out[1].split(), np.float64)
        return dict(ok=bool(ok), it=it, besti=besti, sub_inl=sub_inl, R=v[:9].reshape(3, 3), t=v[9:], counts=[int(c) for c in out[2].split()])
    return solve


@pytest.mark.parametrize("planar,max_points,noise", [(False, 4096, 0.0), (True, 1024, 0.0), (False, 1024, 0.004)])
def test_kernel_arithmetic_on_the_host_matches_the_solver(host_solver, planar, max_points, noise):
    """Every hypothesis's inlier count, the adaptive stop, the chosen hypothesis and the refitted pose of csrc/pnp_math.h against pnp.py on
    a 48 x 64 point map with 30 % outliers (the planar one refuses the DLT; the noisy one makes the refit run long). Counts are integers
    and must be equal; the pose differs by rounding (Jacobi versus LAPACK, moments versus per-point sums): 1e-9 is ten thousand times the
    1e-13 seen and ten thousand times below the solver's accuracy bar of 1e-5."""
    H, W, f, iterations, reproj = 48, 64, 60.0, 60, 5.0
    rng = np.random.default_rng(3)
    depth = 3.0 + 0.3 * np.arange(W)[None, :] / W + np.zeros((H, 1)) if planar else rng.uniform(2.0, 6.0, (H, W))
    grid = pnp.pixel_grid(H, W).astype(np.float64)
    cam = np.concatenate([(grid - [W / 2, H / 2]) / f * depth[..., None], depth[..., None]], -1)
    bad = rng.uniform(size=(H, W)) < 0.3
    cam[bad, :2] += rng.uniform(1.0, 3.0, (int(bad.sum()), 2)) * rng.choice([-1.0, 1.0], (int(bad.sum()), 2))
    cam += noise * rng.normal(size=cam.shape)
    msk = rng.uniform(size=(H, W)) > 0.2
    X, pix = cam.astype(np.float32)[msk].astype(np.float64), grid[msk]
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    sub, draws = pnp.sample_tables(len(X), iterations, 0, 6, max_points)
    ok, R, t, full = pnp.solve_pnp_ransac(X, pix, K, iterations=iterations, reproj=reproj, max_points=max_points, tables=(sub, draws))
    Xs, ps = X[sub], pix[sub]
    bs = np.concatenate([ps, np.ones((len(ps), 1))], 1) @ np.linalg.inv(K).T
    counts = []
    for d in draws:
        Rh, th = pnp.pnp_orthogonal_iteration(Xs[d], bs[d], iters=15)
        counts.append(int((pnp.reprojection_error(Xs, ps, K, Rh, th) < reproj).sum()))
    got = host_solver(Xs, np.flatnonzero(msk.reshape(-1))[sub], draws, W, f, W / 2, H / 2, reproj)
    assert ok and got["ok"] and got["counts"] == counts
    best, it, needed, besti = 0, 0, iterations, -1
    while it < min(iterations, needed):
        it += 1
        if counts[it - 1] > best:
            best, besti = counts[it - 1], it - 1
            p_all = (best / len(Xs)) ** 6
            needed = np.inf if p_all < 1e-9 else (0 if p_all >= 1 else np.log(1 - 0.99) / np.log(1 - p_all))
    assert (got["it"], got["besti"]) == (it, besti)
    assert got["sub_inl"] == int((pnp.reprojection_error(Xs, ps, K, R, t) < reproj).sum())
    print(f"[pnp_math on the host] it {it} best {besti} inliers {got['sub_inl']}; |R - host| {np.abs(got['R'] - R).max():.2e} |t - host| {np.abs(got['t'] - t).max():.2e}")
    assert np.abs(got["R"] - R).max() < 1e-9 and np.abs(got["t"] - t).max() < 1e-9


def test_tables_that_do_not_fit_are_refused_with_a_message():
    X, pix, K = _scene(300, 1)
    sub, draws = pnp.sample_tables(300, 10)
    with pytest.raises(ValueError, match="sample_tables"):
        pnp.solve_pnp_ransac(X, pix, K, iterations=40, tables=(sub, draws))            # fewer draws than iterations
    with pytest.raises(ValueError, match="sample_tables"):
        pnp.solve_pnp_ransac(X, pix, K, iterations=10, tables=pnp.sample_tables(299, 10))   # drawn for another count
    from geo4d_amd import _lib
    lib = _lib.load()
    assert lib.geo4d_pnp_ransac_workspace(1024, 64, 8, 8, 10, 64) > 0                    # sizes are defined past the launch limit ...
    buf = (_lib.C.c_double * 8)()
    p = _lib.C.addressof(buf)
    rc = lib.geo4d_pnp_ransac(p, 24, p, 8, 0.5, p, 2.0, 1.0, 5.0, 8, 6, p, p, p, p, 8, 1024, 64, 2, 4, p, p, p, p, p, 1 << 40, None)
    assert rc == -22 and b"pnp_ransac" in lib.geo4d_last_error()                          # ... but B * C = 65536 is refused before any launch
