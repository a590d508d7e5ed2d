"""The 16-byte epilogue of conv_gemm's 16-bit output rows (gemm_epilogue.h geglu_wide16 / plain_wide16: two adjacent 16-column blocks
traded with v_permlane16_swap into one 16-byte store, the f16 clamp on the packed pair, the debug counter's test outside the loops)
against the 8-byte epilogue it replaces (`ops.EPI_WIDE = 0`, bit 6 of debug_ablate): the same bytes, compared with torch.equal on the raw
16-bit words (a NaN must be the same NaN), and the same saturation count.

The 8-byte path is pinned against torch / fp64 by the older files (test_gemm_epilogue_bits_gpu.py, test_f16x2_gpu.py, test_gemm_v2_gpu.py,
test_gemm_v3_gpu.py, test_presplit_gpu.py); here every output is also held to half an f16 ulp of fp64 math on the operands the kernel reads,
so that the two paths cannot be wrong together. Every output lives in a buffer wider and taller than the result (ldo > N), filled with a
sentinel: a 16-byte store that strays past column N or row M shows up there.

Shapes: K = 128 (4 slabs, the fewest the phased tiles take) or 256; M in {40, 72, 200} (a ragged last row block); N such that a wave tile
holds an odd block, a partial last pair, a whole pair plus a tail (wave tiles cut by N keep the 8-byte code - both sides of that choice run in
one launch); every tile with a 16-bit-row instantiation (hint 22 runs on 23, or on 25 for a GEGLU, for the two-pass type), each on the
production grid and on three persistent workgroups. 16-bit rows with a residual exist for bf16 only: plain f16 operands run on the first
generation, which has no register epilogue."""
import pytest
import torch
import torch.nn.functional as TF

from test_f16x2_gpu import a_seen, weight_seen
from test_gemm_v2_gpu import rnd

pytestmark = pytest.mark.gpu

PLAIN_TILES = [22, 23, 25, 27, 28, 71, 72, 73, 74]
GEGLU_TILES = [22, 25, 27, 71, 74]
SENTINEL = -1234.0


def bits(t):
    return t.contiguous().view(torch.int16)


def on_off(fn):
    """fn() -> tensor (or tuple of tensors) with the 16-byte epilogue and with the 8-byte one, each on the production grid and on three
    persistent workgroups: all four must hold the same bits. Returns the production result."""
    from geo4d_amd import ops
    res = []
    try:
        for wide in (1, 0):
            for grid in (0, 2):
                ops.EPI_WIDE, ops.DEBUG_ABLATE = wide, grid
                r = fn()
                res.append(r if isinstance(r, tuple) else (r,))
    finally:
        ops.EPI_WIDE, ops.DEBUG_ABLATE = 1, 0
    for name, r in zip(("wide, 3 workgroups", "8-byte", "8-byte, 3 workgroups"), res[1:]):
        for a, b in zip(res[0], r):
            assert a.dtype == b.dtype and torch.equal(bits(a), bits(b)), f"the 16-byte epilogue's result differs from: {name}"
    return res[0] if len(res[0]) > 1 else res[0][0]


def tile_run(x, wp, out, tile, bias=None, residual=None, act=0):
    """The tile the planner runs for the ops.linear launch with these arguments (a phased tile needs >= 4 K slabs, an even count;
    the two-pass type has no 256x256): a case that names a tile must say which kernel it really covers."""
    from geo4d_amd import ops
    p = ops.conv_gemm_descriptor(x, wp, out, M=x.shape[0], N=wp.shape[0], K=x.shape[1], Cin=x.shape[1], lda=x.stride(0), ldw=wp.stride(0),
                                 ldo=out.stride(0), bias=bias, residual=residual, ldr=residual.stride(0) if residual is not None else 0,
                                 act=act, tile_hint=tile, split_k=1)
    return ops.conv_gemm_plan(p).tile_hint


def framed(M, N, dtype, dev, extra=24):
    """A sentinel-filled [M + 16, N + extra] buffer and its [M, N] corner (row pitch N + extra: ldo > N, rows stay 16-byte aligned)."""
    buf = torch.full((M + 16, N + extra), SENTINEL, device=dev, dtype=dtype)
    return buf, buf[:M, :N]


def frame_untouched(buf, M, N):
    return bool((buf[M:] == SENTINEL).all()) and bool((buf[:, N:] == SENTINEL).all())


def half_ulp(got, ref, dtype):
    """|got - ref| within half an ulp of the 16-bit format (+ the fp32 accumulation error), as test_f16x2_gpu.py asks of the GEGLU rows"""
    u = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    return bool(((got.double() - ref).abs() <= ref.abs() * u + 1e-5 * float(ref.abs().max()) + 2.0 ** -24).all())


@pytest.mark.parametrize("tile", PLAIN_TILES)
def test_plain_f16_rows(dev, tile):
    """Two-pass f16 launches writing plain f16 rows (o_split = 2), alpha + column bias: the q | k, q | k | v and cross-attention q projections."""
    from geo4d_amd import ops, pack
    K = 128
    for M in (40, 72, 200):
        x = rnd((M, K), dev, M).to(torch.float16)
        for N in (8, 24, 40, 72, 136):
            w, b = rnd((N, K), dev, N, 0.1), rnd((N,), dev, N + 1)
            wp = pack.split_f16(w)
            ref = a_seen(x) @ weight_seen(wp).t()
            for bias in (b, None):
                buf, out = framed(M, N, torch.float16, dev)
                assert tile_run(x, wp, out, tile, bias) == (23 if tile == 22 else tile)

                def run():
                    buf.fill_(SENTINEL)
                    ops.linear(x, wp, bias, out=out, split_out="f16", tile_hint=tile, split_k=1)
                    return buf.clone()
                got = on_off(run)
                assert frame_untouched(got, M, N), f"tile {tile} M {M} N {N}: a store left the [M, N] corner"
                assert half_ulp(got[:M, :N], ref + (bias.double() if bias is not None else 0.0), torch.float16), f"tile {tile} M {M} N {N}"


@pytest.mark.parametrize("tile", GEGLU_TILES)
def test_geglu_f16_rows(dev, tile):
    """The GEGLU ff1 writing f16 rows: N = 64 (one value | gate group), 128, 192 (an odd group count), 320 (five groups: wave tiles of 64
    and 128 columns end inside N and beyond it)."""
    from geo4d_amd import ops, pack
    K = 256
    for M in (40, 72, 200):
        x = rnd((M, K), dev, 100 + M).to(torch.float16)
        for N in (64, 128, 192, 320):
            inner = N // 2
            w, b = rnd((N, K), dev, N, 0.1), rnd((N,), dev, N + 1)
            wp, bp = pack.pack_geglu_x2(w, b, "bf16x3m")
            wu = torch.empty((N, K), device=dev, dtype=torch.float64)
            wu[pack.geglu_perm(inner, dev)] = weight_seen(wp)
            for bias in (bp, None):
                buf, out = framed(M, inner, torch.float16, dev)
                assert tile_run(x, wp, out, tile, bias, act=2) == (25 if tile == 22 else tile)

                def run():
                    buf.fill_(SENTINEL)
                    ops.linear(x, wp, bias, act=2, out=out, split_out="f16", tile_hint=tile, split_k=1)
                    return buf.clone()
                got = on_off(run)
                assert frame_untouched(got, M, inner), f"tile {tile} M {M} N {N}: a store left the [M, N / 2] corner"
                h = a_seen(x) @ wu.t() + (b.double() if bias is not None else 0.0)
                assert half_ulp(got[:M, :inner], h[:, :inner] * TF.gelu(h[:, inner:]), torch.float16), f"tile {tile} M {M} N {N}"


@pytest.mark.parametrize("tile,act", [(25, 0), (25, 2), (28, 0), (71, 0), (71, 2), (72, 0)])
def test_batch_of_two_with_o_bs(dev, tile, act):
    """Batch 2: the second problem's rows start o_bs elements after the first's (a gap of 5 rows between them), its weights w_bs after."""
    from geo4d_amd import ops, pack
    M, K, N = 72, 128, 192 if act == 2 else 72
    nout = N // 2 if act == 2 else N
    ldo = nout + 24
    x = rnd((2 * M, K), dev, 7).to(torch.float16)
    w, b = rnd((2 * N, K), dev, 8, 0.1), rnd((N,), dev, 9)
    if act == 2:
        perm = pack.geglu_perm(nout, dev)
        wp, bp = pack.split_f16(torch.cat([w[:N][perm], w[N:][perm]])), b[perm].contiguous()
    else:
        wp, bp = pack.split_f16(w), b
    o_bs = (M + 5) * ldo
    buf = torch.empty((2 * (M + 5) + 16, ldo), device=dev, dtype=torch.float16)

    def run():
        buf.fill_(SENTINEL)
        ops.conv_gemm(x, wp, buf, M=M, N=N, K=K, Cin=K, lda=K, ldw=wp.stride(0), ldo=ldo, bias=bp, act=act, batch=2, a_bs=M * K,
                      w_bs=N * wp.stride(0), o_bs=o_bs, tile_hint=tile, split_k=1)
        return buf.clone()
    got = on_off(run)
    ws = weight_seen(wp)
    for z in range(2):
        rows = got[z * (M + 5): z * (M + 5) + M]
        h = a_seen(x[z * M:(z + 1) * M]) @ ws[z * N:(z + 1) * N].t() + bp.double()
        if act == 2:
            hu = torch.empty_like(h)
            hu[:, perm] = h
            h = hu[:, :nout] * TF.gelu(hu[:, nout:])
        assert half_ulp(rows[:, :nout], h, torch.float16), f"batch {z}"
        assert bool((rows[:, nout:] == SENTINEL).all()) and bool((got[z * (M + 5) + M: (z + 1) * (M + 5)] == SENTINEL).all()), f"batch {z}: stray store"
    assert bool((got[2 * (M + 5):] == SENTINEL).all())


@pytest.mark.parametrize("tile", PLAIN_TILES)
def test_bf16_rows_with_residual(dev, tile):
    """The bf16 mode's 16-bit rows (StoreRows16): alpha + column bias + a residual read with 16-byte loads through the same exchange, its row
    pitch (N + 8) different from the output's (N + 24); a residual pitch of N + 4 keeps rows 8-byte aligned only: the 8-byte code.
    K = 256: a bf16 slab is 64 elements, and the phased tiles take no fewer than 4. (256x256 and 64x128 keep the 8-byte epilogue.)"""
    from geo4d_amd import ops, pack
    K = 256
    for M in (40, 200):
        x = rnd((M, K), dev, 200 + M).to(torch.bfloat16)
        for N in (24, 40, 72, 136):
            w, b = rnd((N, K), dev, N, 0.1), rnd((N,), dev, N + 1)
            wp = pack.pack_linear(w, torch.bfloat16)
            for rpad in (8, 4):
                r = rnd((M, N + rpad), dev, N + 2).to(torch.bfloat16)[:, :N]
                buf, out = framed(M, N, torch.bfloat16, dev)
                assert tile_run(x, wp, out, tile, b, residual=r) == tile

                def run():
                    buf.fill_(SENTINEL)
                    ops.linear(x, wp, b, residual=r, out=out, tile_hint=tile, split_k=1)
                    return buf.clone()
                got = on_off(run)
                assert frame_untouched(got, M, N), f"tile {tile} M {M} N {N}: a store left the [M, N] corner"
                ref = x.double() @ wp.double().t() + b.double() + r.double()
                assert half_ulp(got[:M, :N], ref, torch.bfloat16), f"tile {tile} M {M} N {N} ldr {N + rpad}"


@pytest.mark.parametrize("tile", [22, 25, 27, 71, 74])
def test_bf16_rows_geglu(dev, tile):
    from geo4d_amd import ops, pack
    M, K, N = 72, 256, 192
    inner = N // 2
    x = rnd((M, K), dev, 300).to(torch.bfloat16)
    w, b = rnd((N, K), dev, 301, 0.1), rnd((N,), dev, 302)
    wp, bp = pack.pack_geglu(w, b, torch.bfloat16)
    buf, out = framed(M, inner, torch.bfloat16, dev)
    assert tile_run(x, wp, out, tile, bp, act=2) == tile

    def run():
        buf.fill_(SENTINEL)
        ops.linear(x, wp, bp, act=2, out=out, tile_hint=tile, split_k=1)
        return buf.clone()
    got = on_off(run)
    assert frame_untouched(got, M, inner)
    h = x.double() @ w.to(torch.bfloat16).double().t() + b.double()
    assert half_ulp(got[:M, :inner], h[:, :inner] * TF.gelu(h[:, inner:]), torch.bfloat16)


@pytest.mark.parametrize("tile", [25, 28, 72])
def test_saturation_plain(dev, tile):
    """Six outputs beyond the f16 range (three rows x two columns in different 4-column lanes, 480000 each), and NaN: both paths store
    +-65504 and the NaN, and count six clamped lanes. (A single NaN cannot come out of alpha * acc + bias from finite f16 operands - the
    fused multiply-add never overflows in the middle; a NaN bias makes column 9 NaN in every row. The GEGLU case below has exactly one.)"""
    from geo4d_amd import ops, pack
    M, K, N = 40, 128, 160
    x, w, b = rnd((M, K), dev, 400).to(torch.float16), rnd((N, K), dev, 401, 0.1), rnd((N,), dev, 402)
    x[:, 5] = 0.0
    w[:, 5] = 0.0
    for m in (3, 17, 38):
        x[m, 5] = 60000.0
    w[1, 5], w[30, 5] = 8.0, -8.0
    b[9] = float("nan")
    wp = pack.split_f16(w)
    cnt = torch.zeros(1, device=dev, dtype=torch.int64)

    def run():
        cnt.zero_()
        out = ops.linear(x, wp, b, split_out="f16", tile_hint=tile, split_k=1)
        return out, cnt.clone()
    old = ops.SAT_COUNTER
    try:
        ops.SAT_COUNTER = cnt
        out, n = on_off(run)
    finally:
        ops.SAT_COUNTER = old
    assert int(n.item()) == 6
    assert bool(torch.isnan(out[:, 9]).all()) and int(torch.isnan(out).sum()) == M
    for m in (3, 17, 38):
        assert float(out[m, 1]) == 65504.0 and float(out[m, 30]) == -65504.0
    assert int((out.float().abs() == 65504.0).sum()) == 6


@pytest.mark.parametrize("tile", [25, 27, 71])
def test_saturation_geglu(dev, tile):
    """An infinite bias on value column 3: value x gelu(gate) is +-inf in every row (clamped, counted: one lane per row) except row 11, whose
    gate is pushed to -50 where gelu is exactly zero: inf x 0 = the one NaN, kept by both paths. (M = 384 rows fill the 64-, 128- and
    192-row tiles: the counter also sees a wave tile's rows beyond M, whose accumulators are zero and whose bias is the same.)"""
    from geo4d_amd import ops, pack
    M, K, inner = 384, 128, 64
    x = rnd((M, K), dev, 500).to(torch.float16)
    w, b = rnd((2 * inner, K), dev, 501, 0.1), rnd((2 * inner,), dev, 502)
    x[:, 7] = 0.0
    w[:, 7] = 0.0
    x[11, 7], w[inner + 3, 7] = 100.0, -0.5
    b[3] = float("inf")
    wp, bp = pack.pack_geglu_x2(w, b, "bf16x3m")
    cnt = torch.zeros(1, device=dev, dtype=torch.int64)

    def run():
        cnt.zero_()
        out = ops.linear(x, wp, bp, act=2, split_out="f16", tile_hint=tile, split_k=1)
        return out, cnt.clone()
    old = ops.SAT_COUNTER
    try:
        ops.SAT_COUNTER = cnt
        out, n = on_off(run)
    finally:
        ops.SAT_COUNTER = old
    assert bool(torch.isnan(out[11, 3])) and int(torch.isnan(out).sum()) == 1
    others = torch.cat([out[:11, 3], out[12:, 3]]).float()
    assert bool((others.abs() == 65504.0).all()) and int(n.item()) == M - 1
    assert int((out.float().abs() == 65504.0).sum()) == M - 1
