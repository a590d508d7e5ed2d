"""GPU tests of the sub-pixel Upsample convolution (ops.conv2d_up2 -> geo4d_conv_gemm_up2: four 2x2 phase convolutions on the source grid
whose rows land on the parities of the nearest-2x grid) against the gather form (ops.conv2d(ups=2)) and torch.

Exact: integer-valued operands as in tests/conv_cases.py (activations [-4, 4], weights [-2, 2] - a folded weight is a sum of at most 4 of
them -, bias [-8, 8]): with K = 4 Cin <= 256 every partial sum stays below 2^24, so all three must be EQUAL. Sources: F = 2 with 5 x 8
(a frame is 40 rows: blocks straddle frames), 3 x 5 (odd W: a tile's rows straddle source rows) and 20 x 32 (several tiles per phase);
Cin 32 / 64, N 64 / 96; with bias, into a column view with ldo > N, raw and pre-split A, tile hints 22, 23, 25, 71, 72, the four-launch
and the batch form; once more with three persistent workgroups (debug_ablate = 2).

Random data: N(0, 1) operands at 5 x 8 and 20 x 32 against a float64 torch reference. Both forms run the same three bf16 passes; the
phase form differs by one float32 rounding of each summed weight and by the summation order, so its relative L2 error may be at most 2x
the gather form's on the same inputs.

GroupNorm: the sums a phase-form launch emits (one buffer, the four phases interleaved) give the consumer GroupNorm the result of the
same GroupNorm on its own statistics pass, at the agreement tests/test_groupnorm_fused_gpu.py uses for re-ordered sums (relative L2
<= 2 x 2e-5 for f32 rows)."""
import functools
import types

import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu

SOURCES = [(5, 8), (3, 5), (20, 32)]
CHANNELS = [(32, 64), (64, 96)]          # (Cin, N)
HINTS = (22, 23, 25, 71, 72)
FORMS = ("phases", "batch")
F_ = 2


@functools.lru_cache(maxsize=None)
def reference(H, W, cin, n):
    """Integer operands and the float64 reference of the case, shared by every test of it: nobody writes into it."""
    c = cc._case(f"up2_{H}x{W}_c{cin}_n{n}", "", [], F=F_, Hin=H, Win=W, ups=2, Cin=cin, Co=n)
    seed = 7000 + 100 * H + 10 * W + cin + n
    d = types.SimpleNamespace(case=c)
    d.x = cc._ints((F_ * H * W, cin), 4, seed)
    d.w = cc._ints((n, cin, 3, 3), 2, seed + 1)
    d.bias = cc._ints((n,), 8, seed + 2)
    conv, (Ho, Wo) = cc.conv_rows(c, d.x, d.w)
    assert (Ho, Wo) == (2 * H, 2 * W)
    d.ref = (conv + d.bias).float()
    return d


def operands(d, dev, presplit):
    from geo4d_amd import ops, pack
    x = d.x.float().to(dev)
    w = d.w.float().to(dev)
    a = ops.presplit(x) if presplit else x
    return a, pack.pack_conv2d(w, "bf16x3"), pack.pack_conv2d_up2(w, "bf16x3"), d.bias.float().to(dev)


def column_view(rows, n, dev):
    return torch.full((rows, n + 32), -7.0, device=dev)[:, 16:16 + n]


def run_up2(a, w4, bias, H, W, n, hint, form, dev):
    from geo4d_amd import ops
    out = column_view(F_ * 4 * H * W, n, dev)
    got, Ho, Wo = ops.conv2d_up2(a, w4, bias, F=F_, Hin=H, Win=W, out=out, tile_hint=hint, form=form)
    assert (Ho, Wo) == (2 * H, 2 * W) and got is out
    return out


@pytest.mark.parametrize("presplit", [False, True], ids=["rawA", "splitA"])
@pytest.mark.parametrize("cin,n", CHANNELS)
@pytest.mark.parametrize("H,W", SOURCES)
def test_phase_form_equals_gather_form_and_torch(dev, H, W, cin, n, presplit):
    from geo4d_amd import ops
    d = reference(H, W, cin, n)
    a, w9, w4, bias = operands(d, dev, presplit)
    ref = d.ref.to(dev)
    gather, _, _ = ops.conv2d(a, w9, bias, F=F_, Hin=H, Win=W, KH=3, KW=3, pad=1, ups=2, tile_hint=25, split_k=1)
    assert torch.equal(gather, ref)
    for hint in HINTS:
        for form in FORMS:
            out = run_up2(a, w4, bias, H, W, n, hint, form, dev)
            assert torch.equal(out, ref), (hint, form, (out - ref).abs().max().item())
            assert torch.equal(out, gather), (hint, form)
            assert bool((out._base[:, :16] == -7.0).all()) and bool((out._base[:, 16 + n:] == -7.0).all()), "wrote outside its columns"


@pytest.mark.parametrize("presplit", [False, True], ids=["rawA", "splitA"])
def test_three_persistent_workgroups(dev, presplit):
    H, W, cin, n = 20, 32, 32, 96
    d = reference(H, W, cin, n)
    a, _, w4, bias = operands(d, dev, presplit)
    ref = d.ref.to(dev)
    for hint in HINTS:
        for form in FORMS:
            out = cc.both_grids(lambda: run_up2(a, w4, bias, H, W, n, hint, form, dev).clone())
            assert torch.equal(out, ref), (hint, form)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("H,W", [(5, 8), (20, 32)])
def test_random_data_error_against_float64(dev, H, W):
    from geo4d_amd import ops, pack
    cin, n = 64, 96
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn((F_ * H * W, cin), generator=g)
    w = torch.randn((n, cin, 3, 3), generator=g)
    b = torch.randn((n,), generator=g)
    c = cc._case("up2_random", "", [], F=F_, Hin=H, Win=W, ups=2, Cin=cin, Co=n)
    ref = cc.conv_rows(c, x.double(), w.double())[0] + b.double()
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    w9, w4 = pack.pack_conv2d(wd, "bf16x3"), pack.pack_conv2d_up2(wd, "bf16x3")
    for presplit in (False, True):
        a = ops.presplit(xd) if presplit else xd
        gather, _, _ = ops.conv2d(a, w9, bd, F=F_, Hin=H, Win=W, KH=3, KW=3, pad=1, ups=2, tile_hint=25, split_k=1)
        e_gather = rel_l2(gather.cpu(), ref)
        for form in FORMS:
            for hint in (25, 72):
                out, _, _ = ops.conv2d_up2(a, w4, bd, F=F_, Hin=H, Win=W, tile_hint=hint, form=form)
                e_phase = rel_l2(out.cpu(), ref)
                print(f"[{H}x{W} presplit={int(presplit)} {form} hint {hint}] rel L2 vs float64: gather {e_gather:.3e}  phase {e_phase:.3e}")
                assert e_phase <= 2 * e_gather, (e_phase, e_gather)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hint,rows", [(22, 64), (25, 64), (72, 80)])
def test_groupnorm_behind_a_phase_form_conv_takes_its_sums(dev, hint, rows, form):
    from geo4d_amd import _lib, ops, pack
    H, W, cin, n = 20, 32, 32, 64          # 640 source rows per frame: whole 64- and 80-row blocks
    g = torch.Generator().manual_seed(hint)
    x = (torch.randn((F_ * H * W, cin), generator=g) + 0.3).to(dev)
    w = torch.randn((n, cin, 3, 3), generator=g).to(dev)
    b = torch.randn((n,), generator=g).to(dev)
    gamma, beta = (torch.randn((n,), generator=g) + 1.0).to(dev), torch.randn((n,), generator=g).to(dev)
    out, Ho, Wo = ops.conv2d_up2(x, pack.pack_conv2d_up2(w, "bf16x3"), b, F=F_, Hin=H, Win=W, gn_stats=True, tile_hint=hint, form=form)
    assert out._gn_colsum_rows == rows and tuple(out._gn_colsum.shape) == (F_ * Ho * Wo // rows, n, 2)
    # every entry holds the sums of `rows` rows of ONE frame, and a frame's entries are contiguous
    per_frame = out._gn_colsum.double().reshape(F_, -1, n, 2).sum(1)
    v = out.double().reshape(F_, Ho * Wo, n)
    want = torch.stack([v.sum(1), (v * v).sum(1)], -1)
    assert torch.allclose(per_frame, want, rtol=1e-5, atol=1e-3)
    for fps in (1, 2):
        assert ops._gn_sources(out, fps * Ho * Wo), "the GroupNorm would not take the sums"
        from_sums = ops.groupnorm(out, gamma, beta, F=F_, HW=Ho * Wo, eps=1e-6, frames_per_stat=fps, silu=True)
        own_pass = ops.groupnorm(out, gamma, beta, F=F_, HW=Ho * Wo, eps=1e-6, frames_per_stat=fps, silu=True, path=_lib.GN_PATH_PARTIAL)
        e = rel_l2(from_sums, own_pass)
        print(f"[hint {hint} {form} fps {fps}] GroupNorm from the phase launch's sums vs its own statistics pass: rel L2 {e:.3e}")
        assert e <= 2 * 2e-5
