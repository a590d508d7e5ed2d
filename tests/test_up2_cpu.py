"""CPU tests of the sub-pixel form of the Upsample convolutions (nearest 2x, then a 3x3 convolution with padding 1):
  * the identity itself, no library: the folded weights (pack.fold_up2) applied as four torch 2x2 convolutions on the source grid and
    interleaved by parity reproduce F.conv2d(F.interpolate(x, 2, "nearest"), w, padding=1) - in float64 to round-off, and exactly in
    float32 where inputs and weights are small integers; the row-mapping formula is a bijection onto the [F, 2H, 2W] token rows;
  * the planner of geo4d_conv_gemm_up2 through its pure-host query geo4d_conv_gemm_up2_plan, in the style of tests/test_gemm_plan.py:
    what it resolves, and its refusals (split-K, other element types, first-generation tiles, epilogues the mapped store does not carry).
Nothing here launches a kernel."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from geo4d_amd import pack

SOURCES = [(3, 5), (5, 8), (1, 1)]       # H x W, 2 frames each


def phases_then_interleave(x, w4, bias=None):
    """x [F, Cin, H, W], w4 [4, Cout, Cin, 2, 2] -> [F, Cout, 2H, 2W]: phase (py, px) pads 1 - py rows on top, py at the bottom
    (columns alike) and fills the output pixels of that parity."""
    n, _, H, W = x.shape
    out = x.new_zeros((n, w4.shape[1], 2 * H, 2 * W))
    for py in (0, 1):
        for px in (0, 1):
            xp = F.pad(x, (1 - px, px, 1 - py, py))
            out[:, :, py::2, px::2] = F.conv2d(xp, w4[2 * py + px].to(x.dtype), bias)
    return out


def reference(x, w, bias=None):
    return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, bias, padding=1)


@pytest.mark.parametrize("H,W", SOURCES)
def test_folded_phases_equal_upsample_then_conv_in_float64(H, W):
    g = torch.Generator().manual_seed(H * 31 + W)
    x = torch.randn((2, 6, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((5, 6, 3, 3), generator=g, dtype=torch.float64)
    b = torch.randn((5,), generator=g, dtype=torch.float64)
    w4 = pack.fold_up2(w.float().double())       # (fold_up2 rounds the sums to float32: give it float32-representable weights)
    ref = reference(x, w.float().double(), b)
    got = phases_then_interleave(x, w4.double(), b)
    # the folded weights carry one float32 rounding of a sum of up to 4 weights (2^-24 relative each), the rest is float64 round-off
    assert (got - ref).abs().max().item() <= 36 * 6 * 2.0 ** -24 * float(x.abs().max() * w.abs().max())
    # and with the sums kept in float64 nothing but round-off is left
    r = torch.tensor([[[1, 0, 0], [0, 1, 1]], [[1, 1, 0], [0, 0, 1]]], dtype=torch.float64)
    w4x = torch.stack([torch.einsum("ak,oikl,bl->oiab", r[py], w, r[px]) for py in (0, 1) for px in (0, 1)])
    assert torch.allclose(phases_then_interleave(x, w4x, b), reference(x, w, b), rtol=0, atol=1e-12)


@pytest.mark.parametrize("H,W", SOURCES)
def test_small_integer_operands_are_equal_in_float32(H, W):
    g = torch.Generator().manual_seed(H * 17 + W)
    x = torch.randint(-4, 5, (2, 8, H, W), generator=g).float()
    w = torch.randint(-3, 4, (7, 8, 3, 3), generator=g).float()
    w4 = pack.fold_up2(w)
    assert w4.dtype == torch.float32 and w4.shape == (4, 7, 8, 2, 2)
    assert torch.equal(w4, w4.round())
    assert torch.equal(phases_then_interleave(x, w4), reference(x, w))


@pytest.mark.parametrize("H,W", SOURCES)
def test_row_mapping_is_a_bijection_onto_the_upsampled_rows(H, W):
    nf = 2
    rows = []
    for py in (0, 1):
        for px in (0, 1):
            for m in range(nf * H * W):
                row = pack.up2_row(m, W, py, px)
                f, y, x = m // (H * W), (m % (H * W)) // W, m % W
                assert row == (f * 2 * H + 2 * y + py) * 2 * W + 2 * x + px       # token row of pixel (f, 2y + py, 2x + px)
                rows.append(row)
    assert sorted(rows) == list(range(nf * 4 * H * W))


def test_packed_phase_weights_are_the_folded_kernels_tap_major():
    g = torch.Generator().manual_seed(3)
    w = torch.randn((4, 32, 3, 3), generator=g)
    w4 = pack.pack_conv2d_up2(w, "f32")
    assert w4.shape == (4, 4, 4 * 32)
    assert torch.equal(w4, pack.fold_up2(w).permute(0, 1, 3, 4, 2).reshape(4, 4, 128))
    assert pack.pack_conv2d_up2(w, "bf16x3").shape == (4, 4, 2 * 4 * 32)       # pre-split: bf16 hi | lo


# ---- the planner ---------------------------------------------------------------------------------------------------------------------
def up2_descriptor(*, F_=16, H=20, W=32, Cin=640, N=640, phase=0, hint=72, a_split=1, dtype=3):
    from geo4d_amd import _lib
    p = _lib.ConvGemm()
    p.A, p.W, p.O, p.bias, p.zeros, p.workspace = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000
    p.workspace_bytes = 1 << 40
    p.M, p.N, p.K, p.Cin = F_ * H * W, N, 4 * Cin, Cin
    p.T, p.Hin, p.Win, p.Hout, p.Wout = 1, H, W, H, W
    p.KT, p.KH, p.KW, p.stride, p.ups = 1, 2, 2, 1, 1
    p.lda, p.ldw, p.ldo = Cin, 4 * Cin, N
    p.dtype, p.out_dtype, p.a_split, p.w_split = dtype, 0, a_split, 1 if dtype == 3 else 0
    p.alpha, p.tile_hint, p.split_k = 1.0, hint, 1
    if phase < 0:
        p.batch, p.w_bs = 4, N * 4 * Cin
    else:
        p.batch, p.ph, p.pw = 1, 1 - (phase >> 1), 1 - (phase & 1)
    return p


def up2_plan(p, src_w, phase):
    from geo4d_amd import _lib
    lib = _lib.load()
    plan = _lib.ConvGemmPlan()
    rc = lib.geo4d_conv_gemm_up2_plan(ctypes.byref(p), src_w, phase, ctypes.byref(plan))
    return (plan, "") if rc == 0 else (None, lib.geo4d_last_error().decode())


@pytest.mark.parametrize("phase", [0, 1, 2, 3, -1])
@pytest.mark.parametrize("hint,runs,rows", [(22, 22, 64), (23, 23, 80), (25, 25, 64), (71, 71, 0), (72, 72, 80)])
def test_plan_resolves_phase_and_batch_launches(phase, hint, runs, rows):
    plan, why = up2_plan(up2_descriptor(phase=phase, hint=hint), 32, phase)
    assert plan is not None, why
    # 20 x 32 = 640 source rows per frame: 64 and 80 divide them, the 96 rows of tile 71 do not (no sums there, the launch itself runs)
    assert (plan.tile_hint, plan.splits, plan.hot, plan.osplit, plan.colsum_rows) == (runs, 1, 2, 0, rows)
    raw, why = up2_plan(up2_descriptor(phase=phase, hint=hint, a_split=0), 32, phase)
    assert raw is not None and raw.hot == 1, why


def test_plan_sends_what_the_phased_stream_cannot_take_to_the_second_generation():
    # (K = 4 Cin is never an odd or short slab count; what remains is the 2 GB window of the activation operand)
    for hint, twin in ((72, 23), (71, 22)):
        p = up2_descriptor(F_=2, H=160, W=256, Cin=256, N=256, hint=hint)
        assert up2_plan(p, 256, 0)[0].tile_hint == hint
        p.lda = 8192        # 3 frames of 160 x 256 pixels x 32 KB rows: beyond the window
        assert up2_plan(p, 256, 0)[0].tile_hint == twin


def test_plan_refusals():
    def refused(p, src_w=32, phase=0):
        plan, why = up2_plan(p, src_w, phase)
        assert plan is None
        return why

    p = up2_descriptor()
    p.split_k = 2
    assert "no split-K" in refused(p)
    for dtype in (0, 1, 2):
        assert "bf16x3" in refused(up2_descriptor(dtype=dtype))
    p = up2_descriptor(dtype=4, a_split=2)
    p.w_split = 1
    assert refused(p)                                              # the two-pass f16 type: refused (by the descriptor checks or the planner)
    p = up2_descriptor()
    p.w_split = 0
    assert "pre-split weight" in refused(p)
    for hint in (0, 1, 13, 17):                                    # generation 1 (0 = the library's own scored choice)
        assert "tile hints 22, 23, 25, 71 and 72" in refused(up2_descriptor(hint=hint))
    for hint in (27, 28, 73, 74):                                  # later generations without the mapped epilogue
        assert "tile hints 22, 23, 25, 71 and 72" in refused(up2_descriptor(hint=hint))
    assert "src_w" in refused(up2_descriptor(), src_w=16)
    p = up2_descriptor()
    p.ups = 2
    assert "ups = 1" in refused(p)
    assert "phase" in refused(up2_descriptor(), phase=4)
    assert "batch" in refused(up2_descriptor(phase=1), phase=2)     # ph / pw of another phase
    assert "batch" in refused(up2_descriptor(phase=0), phase=-1)    # the batch form needs batch 4
    for field, value in (("act", 1), ("R", 0x70000000), ("rowbias", 0x70000000), ("bias_per_row", 1), ("out_dtype", 1), ("ldo", 642)):
        p = up2_descriptor()
        setattr(p, field, value)
        if field == "rowbias":
            p.rowbias_div = 640
        if field == "R":
            p.ldr = 640
        assert "column bias only" in refused(p), field
    p = up2_descriptor(hint=71)                                    # 96-row wave tiles do not divide a frame's 640 source rows
    p.gn_colsum = 0x70000000
    assert "gn_colsum" in refused(p)
    p = up2_descriptor(hint=72)
    p.gn_colsum = 0x70000000
    assert up2_plan(p, 32, 0)[0].colsum_rows == 80
