"""The surface-nets rule of geo4d_amd/csrc/tsdf_mesh.hip restated in numpy (helper of tests/test_tsdf_mesh_cpu.py and
tests/test_tsdf_mesh_gpu.py): float32 arithmetic in the documented op order, np.searchsorted for every neighbour. No GPU, no geo4d_amd
import; keys, centres and liveness come from tests/tsdf_restatement.py.

Inputs: K int64 [M] sorted keys (cell index + 2^20 in three 21-bit fields), f float32 [M], Wt float32 [M], col uint8 [M, 4] or None,
  voxel v, min_weight. Live is tsdf_restatement.live_of; s(m) = f[m] >= 0; the step along axis a is E_a = (1 << 42, 1 << 21, 1)[a]. A
  key field of a real cell holds 1 .. 2^21 - 1: + E_a out of a full field carries into a field of value 0 and - E_a from 1 gives 0, and
  no cell has either key, so the key arithmetic (unsigned 64-bit, as on the device) needs no edge-of-grid test.
1. Cell m is the cube whose corners are the voxel centres with keys K[m] + ox E_0 + oy E_1 + oz E_2, o in {0, 1}^3, corner index
  4 ox + 2 oy + oz. It is complete iff all eight keys are in K and all eight voxels are live.
2. Face. For voxel m and axis a with m' = the row of K[m] + E_a: the pair qualifies if both are live and s(m) != s(m'). With
  b = (a + 1) % 3, c = (a + 2) % 3 the cells around that grid edge are r0 = m, r1 = m - E_b, r2 = m - E_b - E_c, r3 = m - E_c; one quad
  iff all four exist and are complete. Ring (r0, r1, r2, r3) if f[m] < 0, else (r0, r3, r2, r1); triangles (q0, q1, q2), (q0, q2, q3).
  Quads in (m, a) order, triangle rows 2 quad and 2 quad + 1.
3. Vertex. A cell is used iff a quad names it; used cells get ids 0 .. V-1 in order of m. For a = 0, 1, 2 and the other two axes'
  offsets (0, 0), (1, 0), (0, 1), (1, 1) (lower axis first): p = the corner with o_a = 0, q = the one with o_a = 1; if s(p) != s(q):
  t = f_p / (f_p - f_q), S += o with o_a replaced by t, cnt += 1. Vertex X0_k + (S_k / float32(cnt)) * v with X0 = the centre of voxel
  m. Colour: the corner of smallest |f|, the lowest corner index on ties. Weight: the minimum Wt of the eight corners."""
import numpy as np

import tsdf_restatement as tr

F = np.float32
U = np.uint64
STEP = tuple(U(s) for s in tr.STEP)
CORNERS = [(ox, oy, oz) for ox in (0, 1) for oy in (0, 1) for oz in (0, 1)]         # index 4 ox + 2 oy + oz
# (axis, corner p, corner q) of the twelve edges in the rule's order
EDGES = []
for _a in range(3):
    _lo, _hi = [k for k in range(3) if k != _a]
    for _ohi in (0, 1):
        for _olo in (0, 1):
            _o = [0, 0, 0]
            _o[_lo], _o[_hi] = _olo, _ohi
            _p = 4 * _o[0] + 2 * _o[1] + _o[2]
            EDGES.append((_a, _p, _p + (4, 2, 1)[_a]))


def find(K, target):
    """int64 [len(target)]: the row of each uint64 target in K (uint64, sorted), or -1."""
    if len(K) == 0:
        return np.full(len(target), -1, np.int64)
    at = np.minimum(np.searchsorted(K, target), len(K) - 1)
    return np.where(K[at] == target, at, -1).astype(np.int64)


def mesh(K, f, Wt, col, voxel, min_weight):
    """dict(vertices float32 [V, 3], rgba uint8 [V, 4] or None, weight float32 [V], faces int32 [T, 3], cell int64 [V] (the row m of
    each vertex), quad_m / quad_axis int64 [Q], complete bool [M], used bool [M], crossing bool [M] (complete and not all corners of
    one sign))."""
    K = np.asarray(K, dtype=np.int64).astype(U)
    f, Wt, v = np.asarray(f, dtype=F), np.asarray(Wt, dtype=F), F(voxel)
    M = len(K)
    live = tr.live_of(f, Wt, min_weight)
    s = f >= 0
    with np.errstate(over="ignore"):
        corner = np.stack([find(K, K + U(ox) * STEP[0] + U(oy) * STEP[1] + U(oz) * STEP[2]) for ox, oy, oz in CORNERS], 1) \
            if M else np.zeros((0, 8), np.int64)
        complete = (corner >= 0).all(1) & live[np.maximum(corner, 0)].all(1)
        quads = []
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            m2 = corner[:, (4, 2, 1)[a]]
            ring = np.stack([np.arange(M), find(K, K - STEP[b]), find(K, K - STEP[b] - STEP[c]), find(K, K - STEP[c])], 1)
            ok = (m2 >= 0) & live & live[np.maximum(m2, 0)] & (s != s[np.maximum(m2, 0)])
            ok &= (ring >= 0).all(1) & complete[np.maximum(ring, 0)].all(1)
            m = np.nonzero(ok)[0]
            r = ring[m]
            r = np.where((f[m] < 0)[:, None], r, r[:, [0, 3, 2, 1]])
            quads.append(np.concatenate([m[:, None], np.full((len(m), 1), a), r], 1))
    quads = np.concatenate(quads) if quads else np.zeros((0, 6), np.int64)
    quads = quads[np.lexsort((quads[:, 1], quads[:, 0]))]
    used = np.zeros(M, bool)
    used[quads[:, 2:].reshape(-1)] = True
    vid = np.cumsum(used) - 1
    q = vid[quads[:, 2:]]
    faces = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    cell = np.nonzero(used)[0]
    cr = corner[cell]                                                                # [V, 8], all >= 0
    fc, sc = f[cr], s[cr]
    S, cnt = np.zeros((len(cell), 3), F), np.zeros(len(cell), np.int64)
    with np.errstate(all="ignore"):
        for a, p, q_ in EDGES:
            cross = sc[:, p] != sc[:, q_]
            o = np.broadcast_to(np.array(CORNERS[p], dtype=F), (len(cell), 3)).copy()
            o[:, a] = fc[:, p] / (fc[:, p] - fc[:, q_])
            S = np.where(cross[:, None], S + o, S).astype(F)
            cnt += cross
        vertices = (tr.voxel_centres(K[cell].astype(np.int64), v) + (S / cnt.astype(F)[:, None]).astype(F) * v).astype(F)
    pick = cr[np.arange(len(cell)), np.argmin(np.abs(fc), 1)] if len(cell) else np.zeros(0, np.int64)
    some = np.maximum(corner, 0)
    crossing = complete & (s[some].any(1) != s[some].all(1))
    return dict(vertices=vertices.reshape(-1, 3), rgba=None if col is None else np.asarray(col)[pick].reshape(-1, 4),
                weight=Wt[cr].min(1).astype(F) if len(cell) else np.zeros(0, F), faces=faces, cell=cell, quad_m=quads[:, 0],
                quad_axis=quads[:, 1], complete=complete, used=used, crossing=crossing)


# ---- hand-made fields --------------------------------------------------------------------------------------------------------------------
def block_keys(shape, origin=(0, 0, 0)):
    """(K int64 sorted [nx ny nz], cells int64 [.., 3] in the same order) of a dense block of cells starting at cell index `origin`."""
    g = np.stack(np.meshgrid(*(np.arange(n) + o for n, o in zip(shape, origin)), indexing="ij"), -1).reshape(-1, 3)
    K = tr.keys_of(g)
    order = np.argsort(K)
    return K[order], g[order]


def sphere_block(origin=(0, 0, 0), n=6, radius=1.9, colours=False):
    """An n^3 block with f = the signed distance (in voxels) to a sphere about the block's middle, halved: negative inside. (K, f, Wt,
    col or None)."""
    K, g = block_keys((n, n, n), origin)
    d = (g - np.asarray(origin)).astype(np.float64) - (n - 1) / 2
    f = ((np.sqrt((d * d).sum(1)) - radius) / 2).astype(F)
    col = np.random.default_rng(3).integers(0, 256, size=(len(K), 4), dtype=np.uint8) if colours else None
    return K, f, np.full(len(K), 8, F), col


def plane_block(n=4):
    """An n^3 block cut by the plane 0.3 x - 0.5 y + 0.8 z = 0 through the centre of voxel (1, 1, 1), where f is exactly 0 (f = that
    expression in voxels, halved): an open surface that ends at the block's boundary."""
    K, g = block_keys((n, n, n))
    d = g.astype(np.float64) - 1
    return K, ((0.3 * d[:, 0] - 0.5 * d[:, 1] + 0.8 * d[:, 2]) / 2).astype(F), np.full(len(K), 8, F), None


def random_block(n=5, seed=0, holes=0.0, weak=0.0, colours=True):
    """A dense n^3 block of uniform random f in (-0.99, 0.99); a share `holes` of the keys removed and a share `weak` of the weights
    set to 3 (below the default min_weight), the others 4 .. 9."""
    rng = np.random.default_rng(seed)
    K, _ = block_keys((n, n, n))
    K = K[rng.random(len(K)) >= holes]
    f = rng.uniform(-0.99, 0.99, len(K)).astype(F)
    Wt = rng.integers(4, 10, len(K)).astype(F)
    Wt[rng.random(len(K)) < weak] = 3
    return K, f, Wt, rng.integers(0, 256, size=(len(K), 4), dtype=np.uint8) if colours else None


def slab(M):
    """The first M voxels (in key order) of a slab one voxel thick in x and 16 wide in z, f alternating in sign like a chessboard: y and
    z neighbours and sign changes everywhere, and no complete cell."""
    K, g = block_keys((1, -(-M // 16), 16))
    return K[:M], np.where((g[:M, 1] + g[:M, 2]) % 2, F(0.5), F(-0.5)).astype(F), np.full(M, 8, F), None


def edge_counts(faces):
    """(times each directed edge occurs, times each undirected edge occurs) as two int arrays."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    if len(e) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, directed = np.unique(e[:, 0] << 32 | e[:, 1], return_counts=True)
    e.sort(1)
    _, undirected = np.unique(e[:, 0] << 32 | e[:, 1], return_counts=True)
    return directed, undirected
