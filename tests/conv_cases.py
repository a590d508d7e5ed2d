"""Case table and float64 reference of the conv_gemm geometry sweep (tests/test_conv_geometry_cpu.py, tests/test_conv_geometry_gpu.py).

A case is a dict with the keys F, T, Hin, Win, KT, KH, KW, stride, pad, pad_end, ups, Cin, Co, lda_extra (+ `name`, `catches`: the
mistake the case is there for, `wrong`: the deliberately mistaken references that must differ from the right one, and for the NCTHW
heads `out_nchw`, `nchw_channels`, `nchw_offset`). `Cin` counts 16-bit elements - one or two 128-byte K slabs per tap, four in the
`_c256` rows; the 4-byte element types (exact f32, bf16x3, two-pass f16) run the same case at Cin / 2, the same number of slabs (`cin_of`).

The third generation's own kernel takes an even number >= 4 of K slabs per split-K slice; every other launch on its hints runs the
second-generation twin. With K = taps x Cin that means: a 3x3 or temporal conv at two slabs per tap (18 / 6 slabs) at split_k 1 only;
a 1x1 needs Cin = 256 (4 slabs) and has no split_k 2 form below 8 slabs; split_k 2 needs four slabs per tap (the `_c256` 3x3 and
temporal rows). An even split always starts a slice at tap 0; split_k 3 of 18 or 36 slabs starts at taps 6 / 3.

The reference takes nothing from the library's gather: tokens -> NCHW / NCTHW in float64, F.interpolate(nearest, 2) for `ups`, F.pad
with the explicit asymmetric pads, F.conv2d / F.conv3d with padding = 0. The output size is whatever that convolution returns.

All data are small integers (activations [-4, 4], weights [-2, 2], bias and per-frame rowbias [-8, 8], residual [-16, 16]): with
K <= 9 * 256 every partial sum stays below 9 * 256 * 8 < 2^24, so fp32 accumulation is exact in every element type and order, and the kernels'
f32 output must EQUAL the reference - no tolerance."""
import functools
import types

import torch
import torch.nn.functional as TF


def _case(name, catches, wrong, *, F, Hin, Win, T=1, KT=1, KH=3, KW=3, stride=1, pad=1, pad_end=0, ups=1, Cin=128, Co=64, lda_extra=0, **extra):
    return dict(name=name, catches=catches, wrong=tuple(wrong), F=F, T=T, Hin=Hin, Win=Win, KT=KT, KH=KH, KW=KW, stride=stride, pad=pad,
                pad_end=pad_end, ups=ups, Cin=Cin, Co=Co, lda_extra=lda_extra, **extra)


def _temporal(B, T, HW, catches, wrong, Cin=128):
    return _case(f"t311_B{B}_T{T}_HW{HW}" + (f"_c{Cin}" if Cin != 128 else ""), catches, wrong, F=B * T, T=T, Hin=HW, Win=1, KT=3, KH=1, KW=1, pad=0, Cin=Cin)


NEIGHBOUR = "neighbour_frame"       # a tap that falls off the image reads the pixel the flat index lands on instead of zero
CASES = [
    # ---- 3x3, stride 1, pad 1 -----------------------------------------------------------------------------------------------------
    _case("k3s1p1_1x1", "image smaller than the kernel: 8 of 9 taps are padding, the ninth is the frame's only pixel", [NEIGHBOUR], F=40, Hin=1, Win=1),
    _case("k3s1p1_1x5", "one image row: every ky != 1 tap is padding; a row test against Hin that is off by one reads the next frame", [NEIGHBOUR], F=8, Hin=1, Win=5),
    _case("k3s1p1_5x1", "one image column: a kx = 0 / 2 tap that is not masked reads the pixel above / below", [NEIGHBOUR], F=8, Hin=5, Win=1),
    _case("k3s1p1_2x2", "a 256-row tile holds 64 whole frames and every tap of every row touches padding: the frame index of a row deep inside a tile", [NEIGHBOUR], F=70, Hin=2, Win=2),
    _case("k3s1p1_8x8", "even size, several frames per tile: the halo row of frame f + 1 inside the tile of frame f", [NEIGHBOUR], F=5, Hin=8, Win=8),
    _case("k3s1p1_9x7", "odd sizes: oy / ox from a row index that is no multiple of anything", [NEIGHBOUR], F=5, Hin=9, Win=7),
    _case("k3s1p1_9x7_co72", "ragged N (72 columns on 64- / 128-column tiles) on top of the odd geometry", [NEIGHBOUR], F=5, Hin=9, Win=7, Co=72),
    _case("k3s1p1_9x7_c256", "36 K slabs: the only 3x3 depth at which a split_k 2 slice (18 slabs) runs the third generation's own kernel, and split_k 3 starts a slice in the middle of the taps", [NEIGHBOUR], F=5, Hin=9, Win=7, Cin=256),
    # ---- 3x3, stride 2, pad 1 -----------------------------------------------------------------------------------------------------
    _case("k3s2p1_8x8", "stride 2 on an even size (the U-Net's down-samplers): the last tap column never touches padding; sampling must start at 0", ["stride_phase", NEIGHBOUR], F=6, Hin=8, Win=8, stride=2),
    _case("k3s2p1_6x10", "stride 2, even, not square: Hout / Wout swapped or derived from the wrong axis", ["stride_phase", NEIGHBOUR], F=5, Hin=6, Win=10, stride=2),
    _case("k3s2p1_9x7", "stride 2 on odd sizes: the last tap column IS padding", ["stride_phase", NEIGHBOUR], F=5, Hin=9, Win=7, stride=2),
    _case("k3s2p1_2x2", "stride 2, one output pixel per frame: 40 frames in one tile", ["stride_phase", NEIGHBOUR], F=40, Hin=2, Win=2, stride=2),
    _case("k3s2p1_1x1", "stride 2 on a single pixel", [NEIGHBOUR], F=40, Hin=1, Win=1, stride=2),
    # ---- 3x3, stride 2, pad 0, one zero row / column at the bottom / right only (the VAE encoder's Downsample) ----------------------
    _case("k3s2p0e1_8x8", "pad_end: the output is one row / column larger than without it, the zeros are at the END only", ["no_pad_end", "pad_end_at_start", NEIGHBOUR], F=6, Hin=8, Win=8, stride=2, pad=0, pad_end=1),
    _case("k3s2p0e1_6x10", "pad_end on a non-square even size", ["no_pad_end", "pad_end_at_start", NEIGHBOUR], F=5, Hin=6, Win=10, stride=2, pad=0, pad_end=1),
    _case("k3s2p0e1_7x9", "pad_end on odd sizes: the output size does NOT grow and the extra row is never read; padding put at the start instead shows", ["pad_end_at_start"], F=5, Hin=7, Win=9, stride=2, pad=0, pad_end=1),
    _case("k3s2p0e1_2x2", "pad_end on an image smaller than the kernel: the only output pixel exists because of it", ["no_pad_end", "pad_end_at_start", NEIGHBOUR], F=40, Hin=2, Win=2, stride=2, pad=0, pad_end=1),
    # ---- 3x3, stride 1, pad 1 on the nearest-2x up-sampled image -----------------------------------------------------------------------
    _case("k3s1p1u2_1x1", "up-sampling a single pixel: the bounds are those of the 2x2 image, not of the source", ["ups_source_bounds", NEIGHBOUR], F=40, Hin=1, Win=1, ups=2),
    _case("k3s1p1u2_3x5", "up-sampling odd sizes: source pixel = (index >> 1), not ((index + 1) >> 1)", ["ups_shift", "ups_source_bounds", NEIGHBOUR], F=5, Hin=3, Win=5, ups=2),
    _case("k3s1p1u2_4x4", "up-sampling an even size; a third-generation hint must run its second-generation twin", ["ups_shift", "ups_source_bounds", NEIGHBOUR], F=6, Hin=4, Win=4, ups=2, Cin=64),
    # ---- 1x1, stride 2, pad 0: no tap is ever padding -----------------------------------------------------------------------------------
    _case("k1s2p0_8x8", "a strided 1x1 is a gather, not the direct_rows shortcut: source row != output row", ["stride_phase"], F=6, Hin=8, Win=8, KH=1, KW=1, stride=2, pad=0),
    _case("k1s2p0_7x5", "the same on odd sizes", ["stride_phase"], F=6, Hin=7, Win=5, KH=1, KW=1, stride=2, pad=0, Cin=64),
    _case("k1s2p0_8x8_c256", "the strided 1x1 at 4 K slabs, the fewest the third generation's kernel takes (one or two slabs always run its second-generation twin)", ["stride_phase"], F=6, Hin=8, Win=8, KH=1, KW=1, stride=2, pad=0, Cin=256),
    # ---- column-slice views (lda > Cin) -----------------------------------------------------------------------------------------------
    _case("k1s1p0_lda", "direct_rows on a column slice: the row pitch is lda, not Cin, and the view starts at a column offset", ["lda_ignored"], F=5, Hin=9, Win=7, KH=1, KW=1, pad=0, lda_extra=64),
    _case("k1s1p0_lda_c256", "the 1x1 column slice at 4 K slabs: the third generation has no direct_rows shortcut, its window gather takes the pitch", ["lda_ignored"], F=5, Hin=9, Win=7, KH=1, KW=1, pad=0, Cin=256, lda_extra=64),
    _case("k3s1p1_lda", "the gather on a column slice: pixel index x lda", ["lda_ignored", NEIGHBOUR], F=5, Hin=9, Win=7, lda_extra=64),
    # ---- temporal (3,1,1), padding (1,0,0) -----------------------------------------------------------------------------------------------
    _temporal(3, 1, 12, "T = 1: both temporal neighbours are padding although frames f - 1 / f + 1 (other samples) exist", ["temporal_across_batch", "temporal_edge_replicated"]),
    _temporal(3, 2, 12, "T = 2: every frame has exactly one padded neighbour", ["temporal_across_batch", "temporal_edge_replicated"]),
    _temporal(2, 3, 70, "frame T - 1 of sample b must not leak into frame 0 of sample b + 1; 70 rows per frame straddle the tiles", ["temporal_across_batch", "temporal_edge_replicated"]),
    _temporal(1, 16, 1, "HW = 1: a frame is one row, the neighbouring frame is the neighbouring row", ["temporal_edge_replicated"]),
    _temporal(2, 16, 5, "a tile of 160 rows holds both samples", ["temporal_across_batch", "temporal_edge_replicated"]),
    _temporal(2, 3, 70, "12 K slabs: a split_k 2 slice of the temporal conv (6 slabs) on the third generation's own kernel, starting at a channel slab > 0", ["temporal_across_batch", "temporal_edge_replicated"], Cin=256),
    # ---- spatial conv with T = 2 written as NCTHW (first generation only) ----------------------------------------------------------------
    _case("nchw_co16", "the NCTHW epilogue: frame -> (sample, t) with T = 2", ["nchw_T_ignored", NEIGHBOUR], F=4, T=2, Hin=6, Win=5, Co=16, out_nchw=True, nchw_channels=16, nchw_offset=0),
    _case("nchw_co3_view", "3 channels into a channel-offset view of an 8-channel tensor: the other channels stay untouched", ["nchw_T_ignored", NEIGHBOUR], F=4, T=2, Hin=6, Win=5, Co=3, out_nchw=True, nchw_channels=8, nchw_offset=2),
    # ---- padding wider than (K - 1) / 2: exact or refused, never silently different --------------------------------------------------------
    # (at 4x6 with F = 8 a row whose first tap lies before its tile's first row's needs a tile that starts at row 40 + 48 k: no multiple of
    # 128 / 160 / 192 / 256 is one, so these two can only show a wrong bounds test; at 3x5 the 128- and 160-row tiles do hold such rows)
    _case("k3s1p2_4x6", "over-wide padding: two whole rows / columns of padding around the image, the output is larger than the input", [NEIGHBOUR], F=8, Hin=4, Win=6, pad=2),
    _case("k1s1p1_4x6", "a padded 1x1: no direct_rows shortcut although it has one tap and stride 1", [NEIGHBOUR], F=8, Hin=4, Win=6, KH=1, KW=1, pad=1),
    _case("k3s1p2_3x5", "over-wide padding where the first tap's pixel DEcreases inside a tile: frame f + 1 starts before the tile's first row did", ["wrapped_rows_zero", NEIGHBOUR], F=8, Hin=3, Win=5, pad=2),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def cin_of(case, wide):
    """Channels of the case for a 16-bit (`wide` False) / 4-byte element type: the same number of 128-byte K slabs."""
    return case["Cin"] // 2 if wide else case["Cin"]


def sampled_size(c):
    return c["Hin"] * c["ups"], c["Win"] * c["ups"]


def out_size(c):
    """(Hout, Wout) by the textbook formula (the reference takes them from the convolution it runs; the two are compared)."""
    Hs, Ws = sampled_size(c)
    return (Hs + 2 * c["pad"] + c["pad_end"] - c["KH"]) // c["stride"] + 1, (Ws + 2 * c["pad"] + c["pad_end"] - c["KW"]) // c["stride"] + 1


def first_tap_is_monotone(c):
    """The two conditions under which the pixel of a row's first tap never decreases with the row index (on the sampled image)."""
    Hs, Ws = sampled_size(c)
    Ho, Wo = out_size(c)
    return Wo - 1 <= Ws and (Ho - 1) * c["stride"] * Ws + (Wo - 1) * c["stride"] <= Hs * Ws


def rows_with_an_out_of_image_tap(c):
    """Number of output rows (of one sample) with at least one tap outside the image / the sample's T frames."""
    Hs, Ws = sampled_size(c)
    Ho, Wo = out_size(c)
    n = 0
    for t in range(c["T"]):
        for oy in range(Ho):
            for ox in range(Wo):
                iy0, ix0, t0 = oy * c["stride"] - c["pad"], ox * c["stride"] - c["pad"], t - c["KT"] // 2
                n += not (0 <= iy0 and iy0 + c["KH"] <= Hs and 0 <= ix0 and ix0 + c["KW"] <= Ws and 0 <= t0 and t0 + c["KT"] <= c["T"])
    return n


def _ints(shape, bound, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=g).double()


def _upsampled(img, c, shifted=False, source_bounds=False):
    if c["ups"] == 1:
        return img
    if shifted:
        iy = ((torch.arange(2 * c["Hin"]) + 1) // 2).clamp(max=c["Hin"] - 1)
        ix = ((torch.arange(2 * c["Win"]) + 1) // 2).clamp(max=c["Win"] - 1)
        up = img[:, :, iy][:, :, :, ix]
    else:
        up = TF.interpolate(img, scale_factor=2, mode="nearest")
    if source_bounds:
        up = up.clone()
        up[:, :, c["Hin"]:] = 0
        up[:, :, :, c["Win"]:] = 0
    return up


def conv_rows(c, x, w, mistake=None):
    """The convolution alone (no bias / rowbias / residual) of tokens `x` [F * Hin * Win, cin] with the weight `w` in nn.Conv2d /
    nn.Conv3d layout, as rows [F * Hout * Wout, Co] + (Hout, Wout). `mistake` names one deliberately wrong variant."""
    F_, T, cin = c["F"], c["T"], x.shape[1]
    if c["KT"] == 3:
        B, HW = F_ // T, c["Hin"]
        if mistake == "temporal_across_batch":
            B, T = 1, F_
        vol = x.reshape(B, T, HW, 1, cin).permute(0, 4, 1, 2, 3)
        vol = TF.pad(vol, (0, 0, 0, 0, 1, 1), mode="replicate" if mistake == "temporal_edge_replicated" else "constant")
        out = TF.conv3d(vol, w)                                    # [B, Co, T, HW, 1]
        return out.permute(0, 2, 3, 4, 1).reshape(F_ * HW, -1), (HW, 1)
    img = x.reshape(F_, c["Hin"], c["Win"], cin).permute(0, 3, 1, 2)
    img = _upsampled(img, c, shifted=mistake == "ups_shift", source_bounds=mistake == "ups_source_bounds")
    lo, hi = c["pad"], c["pad"] + c["pad_end"]
    if mistake == "no_pad_end":
        hi = c["pad"]
    elif mistake == "pad_end_at_start":
        lo, hi = hi, lo
    elif mistake == "stride_phase":
        lo, hi = lo - 1, hi + 1                                      # sampling starts at source pixel 1; a negative pad crops
    img = TF.pad(img, (lo, hi, lo, hi))
    if img.shape[-2] < c["KH"] or img.shape[-1] < c["KW"]:          # (a mistake can leave no output pixel at all)
        return torch.zeros((0, w.shape[0]), dtype=torch.float64), (0, 0)
    out = TF.conv2d(img, w, stride=c["stride"])
    return out.permute(0, 2, 3, 1).reshape(-1, out.shape[1]), tuple(out.shape[-2:])


def conv_rows_flat_index(c, x, w):
    """The mistake NEIGHBOUR: a gather that checks its FLAT pixel index only, so a tap that leaves the image reads the neighbouring
    row / frame (zero only beyond the tensor)."""
    F_, cin = c["F"], x.shape[1]
    Hs, Ws = sampled_size(c)
    Ho, Wo = out_size(c)
    img = _upsampled(x.reshape(F_, c["Hin"], c["Win"], cin).permute(0, 3, 1, 2), c).permute(0, 2, 3, 1).reshape(F_ * Hs * Ws, cin)
    f, oy, ox = torch.meshgrid(torch.arange(F_), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    out = torch.zeros((F_ * Ho * Wo, w.shape[0]), dtype=torch.float64)
    for ky in range(c["KH"]):
        for kx in range(c["KW"]):
            lin = ((f * Hs + oy * c["stride"] - c["pad"] + ky) * Ws + ox * c["stride"] - c["pad"] + kx).reshape(-1)
            ok = (lin >= 0) & (lin < img.shape[0])
            out += (img[lin.clamp(0, img.shape[0] - 1)] * ok[:, None]) @ w[:, :, ky, kx].t()
    return out


def conv_rows_wrapped(c, conv, tile_rows):
    """The mistake "wrapped_rows_zero": a tile addresses its rows relative to the first tap of its FIRST row with an unsigned offset;
    a row whose first tap lies before that one wraps out of the window and all its taps are staged as zeros."""
    Ho, Wo = out_size(c)
    m = torch.arange(c["F"] * Ho * Wo)
    f, rem = m // (Ho * Wo), m % (Ho * Wo)
    px0 = (f * c["Hin"] + (rem // Wo) * c["stride"] - c["pad"]) * c["Win"] + (rem % Wo) * c["stride"] - c["pad"]
    wrapped = px0 < px0[(m // tile_rows) * tile_rows]
    return conv * (~wrapped)[:, None], int(wrapped.sum())


def mistaken(c, data, mistake):
    """The convolution part of the reference under one named mistake, as rows (its shape may differ from the right one's)."""
    if mistake == NEIGHBOUR:
        return conv_rows_flat_index(c, data.x, data.w)
    if mistake == "lda_ignored":
        return conv_rows(c, data.x_wide[:, :data.x.shape[1]], data.w)[0]
    if mistake == "wrapped_rows_zero":
        return conv_rows_wrapped(c, data.conv, 128)[0]
    if mistake == "nchw_T_ignored":
        return to_ncthw(dict(c, T=1), data.conv).reshape(-1)
    return conv_rows(c, data.x, data.w, mistake)[0]


def to_ncthw(c, rows):
    """rows [F * HW, Co] -> [B, Co, T, Hout, Wout]"""
    Ho, Wo = out_size(c)
    return rows.reshape(c["F"] // c["T"], c["T"], Ho, Wo, rows.shape[1]).permute(0, 4, 1, 2, 3).contiguous()


@functools.lru_cache(maxsize=None)
def reference(name, wide):
    """Operands and float64 reference of case `name` at the channel count of the 16-bit (`wide` False) / 4-byte element types. Shared
    by every test of the case: nobody writes into it."""
    c = CASE_BY_NAME[name]
    cin, seed = cin_of(c, wide), 1000 * (sorted(CASE_BY_NAME).index(name) + 1) + int(wide)
    d = types.SimpleNamespace(case=c, cin=cin)
    rows_in = c["F"] * c["Hin"] * c["Win"]
    d.col0 = c["lda_extra"] // 2                                  # the view starts half the extra columns in
    d.x_wide = _ints((rows_in, cin + c["lda_extra"]), 4, seed)
    d.x = d.x_wide[:, d.col0:d.col0 + cin]
    d.w = _ints((c["Co"], cin, 3, 1, 1) if c["KT"] == 3 else (c["Co"], cin, c["KH"], c["KW"]), 2, seed + 1)
    d.bias = _ints((c["Co"],), 8, seed + 2)
    d.conv, (d.Hout, d.Wout) = conv_rows(c, d.x, d.w)
    M = d.conv.shape[0]
    assert M == c["F"] * d.Hout * d.Wout and (d.Hout, d.Wout) == out_size(c)
    d.rows = d.conv + d.bias
    d.rowbias = d.residual = None
    if c["KT"] == 1:                                              # (conv_temporal has no per-frame bias)
        d.rowbias = _ints((c["F"], c["Co"]), 8, seed + 3)
        d.rows = d.rows + d.rowbias.repeat_interleave(d.Hout * d.Wout, 0)
    if not c.get("out_nchw"):                                     # (the NCTHW heads have no residual)
        d.residual = _ints((M, c["Co"]), 16, seed + 4)
        d.rows = d.rows + d.residual
    d.ref = to_ncthw(c, d.rows) if c.get("out_nchw") else d.rows
    return d


def both_grids(fn):
    """fn() with the production grid and with 3 persistent workgroups (debug_ablate = 2: the tile loop, the next tile's prefetch and the
    gather state carried across tiles run on small shapes); returns the production result after checking that the two are equal."""
    from geo4d_amd import ops
    a = fn()
    ops.DEBUG_ABLATE = 2
    try:
        b = fn()
    finally:
        ops.DEBUG_ABLATE = 0
    assert torch.equal(a, b), "persistent-loop result differs from one-tile-per-workgroup result"
    return a
