"""Host restatement (numpy only) of the counter-based Gaussian noise of ``geo4d_amd/csrc/elementwise.hip``.

With ``noise_seeds`` the sampler's initial noise x_T and the eta > 0 step noise are made on the device by Philox4x32-10 (Salmon, Moraes,
Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): the noise of element ``i`` of a sample is a pure function of
(seed, stream, step, draw, i). ``philox_normal_host`` reproduces on a CPU the exact noise a window received - to fp32 round-off of the device's
``logf`` / ``sqrtf`` / ``sincospif`` (a few ulp); the 32-bit words (``philox_words_host``) bit for bit.

  key     = (seed & 0xffffffff, seed >> 32)             the sample's 64-bit seed
  counter = (i // 4, step, stream, draw)                step = the ddim index (the row of the coefficient table), draw = variant of n_samples
                                                        stream 0 = initial noise x_T (drawn with step 0), 1 = step noise, 2 reserved
  element i takes output word i % 4; words (0, 1) and (2, 3) are two Box-Muller pairs (w_a, w_b):
  u1 = ((w_a >> 8) + 1) / 2^24 in (0, 1],  u2 = (w_b >> 8) / 2^24 in [0, 1),  r = sqrt(-2 ln u1)
  even word: r cos(2 pi u2),  odd word: r sin(2 pi u2);  |z| <= sqrt(48 ln 2) = 5.768, never NaN / Inf
"""
import numpy as np

STREAM_XT, STREAM_STEP = 0, 1          # counter word 2: initial noise x_T / DDIM step noise (2 is reserved)
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MAX_ABS_NORMAL = float(np.sqrt(48.0 * np.log(2.0)))


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds. ``counter``: 4 words, ``key``: 2 words - ints or uint32 arrays of one common shape. Returns 4 uint32
    arrays (0-d arrays for int inputs)."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for x in key]
    assert len(c) == 4 and len(k) == 2
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]         # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(PHILOX_W0)) & mask, (k[1] + np.uint64(PHILOX_W1)) & mask]
    return tuple(x.astype(np.uint32) for x in c)


def _words4(seed, stream, step, n, draw):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (int(n) + 3) // 4
    if not 0 < int(n) <= 1 << 34:
        raise ValueError(f"n = {n}: 1 .. 2^34 elements per sample")
    q = np.arange(nq, dtype=np.uint64)
    full = lambda v: np.full(nq, int(v) & 0xFFFFFFFF, dtype=np.uint64)
    return philox4x32_10((q, full(step), full(stream), full(draw)), (full(seed), full(seed >> 32)))


def philox_words_host(seed, stream, step, n, draw=0):
    """The raw 32-bit word of each of the first ``n`` elements: uint32 [n]."""
    return np.stack(_words4(seed, stream, step, n, draw), axis=1).reshape(-1)[:n]


def philox_normal_host(seed, stream, step, n, draw=0):
    """The first ``n`` standard normals of (seed, stream, step, draw): float64 [n], Box-Muller in fp64 on the exact uniforms. A prefix of
    every longer draw: element i does not depend on n."""
    w = _words4(seed, stream, step, n, draw)
    out = np.empty((w[0].shape[0], 4), dtype=np.float64)
    for pair in (0, 1):
        a, b = w[2 * pair].astype(np.float64), w[2 * pair + 1].astype(np.float64)
        u1 = (np.floor(a / 256.0) + 1.0) / 16777216.0
        u2 = np.floor(b / 256.0) / 16777216.0
        rad = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * pair] = rad * np.cos(2.0 * np.pi * u2)
        out[:, 2 * pair + 1] = rad * np.sin(2.0 * np.pi * u2)
    return out.reshape(-1)[:n]
