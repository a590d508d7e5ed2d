"""Exact conv geometry sweep of geo4d_conv_gemm: every row of tests/conv_cases.py in every element type, on tiles of all three kernel
generations (the table gather, the direct_rows shortcut, the third generation's buffer-window gather), with split-K 1 and 2 (3 as well on
the third generation's hints) and, from the second generation on, also under three persistent workgroups. Which rows reach the third
generation's own kernel, and at which split, follows from their K slabs (tests/conv_cases.py); the tests assert it per row. The data are small integers, so every launch must EQUAL the float64
reference. A (mode, tile, split) the library has no kernel for must be refused with an error; nothing is skipped.

Each test prints one `[conv-geometry]` line: launches that ran, expected refusals, third-generation hints that ran natively / were
redirected to their second-generation twin by the planner."""
import types

import pytest
import torch

import conv_cases as cc
from conv_cases import both_grids
from test_presplit_gpu import make_split

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in cc.CASES]
BF16_HINTS = (0, 1, 17, 22, 23, 25, 27, 28, 71, 72, 73, 74)
# mode -> (4-byte K elements, tile hints that run, tile hints that must be refused: the later generations serve bf16 / bf16x3 / f16x2)
MODES = {
    "f32": (True, (0, 1, 4, 11, 16), (25, 72)),
    "f16": (False, (0, 1, 13), (25, 72)),
    "bf16": (False, BF16_HINTS, ()),
    "bf16x3": (True, BF16_HINTS, ()),                       # raw f32 activations x pre-split weight
    "bf16x3_presplit": (True, (25, 72, 74), ()),            # pre-split activations x pre-split weight
    "f16x2": (True, (0, 23, 25, 71, 72, 74), ()),           # two-pass f16: plain f16 rows x pack.split_f16 weight
}
ACT_DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "bf16x3": torch.float32, "f16x2": torch.float16}
SENTINEL = -8192.0      # what the channels outside an NCTHW view hold (a bf16 / f16 number)


def generation(hint):
    return 3 if hint >= 71 else 2 if hint >= 21 else 1


def tile_that_is_asked(mode, hint):
    return 25 if (mode == "f16x2" and hint == 0) else hint      # the two-pass type's default for small problems


def k_slabs(c):
    return c["KT"] * c["KH"] * c["KW"] * c["Cin"] // 64          # 128-byte K slabs: the same for the 16-bit and the 4-byte types


def is_refused(c, mode, hint, split):
    """What the library must refuse: later-generation tiles in the exact-f32 / f16 modes, NCTHW outputs beyond the first generation and
    in the two-pass type, split-K of an NCTHW output, split-K with fewer K slabs than the tile takes (the library's own tile choice,
    hints 0..5, splits only from 8 slabs per slice; an explicit tile needs one slab per slice)."""
    h = tile_that_is_asked(mode, hint)
    if mode in ("f32", "f16") and generation(h) > 1:
        return True
    if c.get("out_nchw") and (generation(h) > 1 or mode == "f16x2" or split > 1):
        return True
    if split > 1:
        return k_slabs(c) // split < (8 if h <= 5 else 1)
    return False


def runs_the_phased_stream(c, split):
    """A third-generation hint runs its own kernel on an even number >= 4 of K slabs per slice, no up-sampling, and a geometry in which
    the first tap's pixel never decreases with the row; the planner sends every other launch to the tile's second-generation twin."""
    ns = k_slabs(c)
    return c["ups"] == 1 and ns % split == 0 and (ns // split) % 2 == 0 and ns // split >= 4 and cc.first_tap_is_monotone(c)


def operands(c, d, mode, dev):
    from geo4d_amd import ops, pack
    o = types.SimpleNamespace()
    cin, col0 = d.cin, d.col0
    if mode == "bf16x3_presplit":
        o.x = make_split(d.x.float().contiguous().to(dev))                        # [rows, 2 cin]
        if c["lda_extra"]:
            wide = torch.full((o.x.shape[0], 2 * (cin + c["lda_extra"])), 3.0, device=dev, dtype=torch.bfloat16)
            wide[:, 2 * col0:2 * (col0 + cin)] = o.x.as_subclass(torch.Tensor)
            o.x = ops.SplitAct.wrap(wide[:, 2 * col0:2 * (col0 + cin)])
    else:
        o.x = d.x_wide.to(ACT_DTYPE[mode]).to(dev)[:, col0:col0 + cin]
    w = d.w.float().to(dev)
    if mode == "f16x2":
        o.w = pack.pack_conv3d_t_x2(w, "bf16x3m") if c["KT"] == 3 else pack.pack_conv2d_x2(w, "bf16x3m")
    else:
        how = "bf16x3" if mode.startswith("bf16x3") else ACT_DTYPE[mode]
        o.w = pack.pack_conv3d_t(w, how) if c["KT"] == 3 else pack.pack_conv2d(w, how)
    o.bias = d.bias.float().to(dev)
    o.rowbias = None if d.rowbias is None else d.rowbias.float().to(dev)
    o.residual = {} if d.residual is None else {t: d.residual.to(t).to(dev) for t in (torch.float32, torch.bfloat16, torch.float16)}
    return o


def launch(c, d, o, hint, split, out_dtype=torch.float32):
    from geo4d_amd import ops
    dev = o.bias.device
    res = o.residual.get(out_dtype)
    if c["KT"] == 3:
        out = torch.empty((d.rows.shape[0], c["Co"]), device=dev, dtype=out_dtype)
        return ops.conv_temporal(o.x, o.w, o.bias, B=c["F"] // c["T"], T=c["T"], HW=c["Hin"], residual=res, out=out, tile_hint=hint, split_k=split)
    kw = dict(F=c["F"], Hin=c["Hin"], Win=c["Win"], KH=c["KH"], KW=c["KW"], stride=c["stride"], pad=c["pad"], pad_end=c["pad_end"], ups=c["ups"],
              T=c["T"], rowbias=o.rowbias, rowbias_div=d.Hout * d.Wout, residual=res, out_dtype=out_dtype, tile_hint=hint, split_k=split)
    full = None
    if c.get("out_nchw"):
        full = torch.full((c["F"] // c["T"], c["nchw_channels"], c["T"], d.Hout, d.Wout), SENTINEL, device=dev, dtype=out_dtype)
        kw.update(out=full[:, c["nchw_offset"]:c["nchw_offset"] + c["Co"]], out_nchw=True, nchw_channels=c["nchw_channels"])
    out, Ho, Wo = ops.conv2d(o.x, o.w, o.bias, **kw)
    assert (Ho, Wo) == (d.Hout, d.Wout), f"ops.conv2d says {Ho} x {Wo}, the padded reference convolution {d.Hout} x {d.Wout}"
    return out if full is None else full


def expected(c, d, dev, dtype):
    """The reference in the output's layout and type; an NCTHW case: the whole tensor, sentinel channels included."""
    ref = d.ref.to(dtype).to(dev)
    if not c.get("out_nchw"):
        return ref
    full = torch.full((ref.shape[0], c["nchw_channels"]) + tuple(ref.shape[2:]), SENTINEL, device=dev, dtype=dtype)
    full[:, c["nchw_offset"]:c["nchw_offset"] + c["Co"]] = ref
    return full


def assert_exact(c, d, got, want, label, exact_want=None):
    if got.shape == want.shape and torch.equal(got, want):
        return
    assert got.shape == want.shape, f"{label}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    bad = (got != want).nonzero()
    kind = ""
    if exact_want is not None:      # a 16-bit output: are only values wrong that the type cannot hold, i.e. is it the rounding?
        inexact = want.double() != exact_want
        kind = " (ROUNDING finding: only values the output type cannot represent differ)" if bool(inexact[tuple(bad.t())].all()) else " (geometry: representable values differ)"
    where = []
    for idx in bad[:6].tolist():
        if c.get("out_nchw"):
            b, ch, t, oy, ox = idx
            f = b * c["T"] + t
        else:
            (m, ch), hw = idx, d.Hout * d.Wout
            f, oy, ox = m // hw, (m % hw) // d.Wout, m % d.Wout
        where.append(f"(frame {f}, oy {oy}, ox {ox}, channel {ch}): got {got[tuple(idx)].item()} want {want[tuple(idx)].item()}")
    raise AssertionError(f"{c['name']} {label}: {len(bad)} of {want.numel()} elements differ{kind}; first: " + "; ".join(where))


def library_runs_the_phased_stream(c):
    """The planner's own answer for the case's geometry on a third-generation hint at split_k 1, observed through
    geo4d_conv_gemm_colsum_rows: hint 73 emits GroupNorm sums per 128 rows, its second-generation twin per 64. The rule looks at the
    geometry of a frame, not at the number of frames, so the query uses 128 frames per sample (M a multiple of both)."""
    import ctypes
    from geo4d_amd import _lib
    from test_gemm_plan import FORMATS, descriptor
    Ho, Wo = cc.out_size(c)
    M, K = 128 * c["T"] * Ho * Wo, c["KT"] * c["KH"] * c["KW"] * c["Cin"]
    p = descriptor(f"{M}x{c['Co']}x{K}|c{c['Cin']}|t{c['KT']}{c['KH']}{c['KW']}s{c['stride']}u{c['ups']}", 1, c["T"], Ho, Wo, FORMATS[1], 73, 1, 0, 0, 0)
    p.Hin, p.Win, p.ph, p.pw, p.pt, p.lda = c["Hin"], c["Win"], c["pad"], c["pad"], c["KT"] // 2, c["Cin"] + c["lda_extra"]
    rows = _lib.load().geo4d_conv_gemm_colsum_rows(ctypes.byref(p))
    assert rows in (64, 128), rows
    return rows == 128


SPLITS = (1, 2)
V3_SPLITS = (1, 2, 3)       # 18 / 36 slabs in three slices: the third generation's mid-K start at a tap > 0


def expected_counts(c):
    """(launches that run, refusals) of a case, from its K slabs. Asked: 45 (mode, tile) pairs - 7 + 5 + 12 + 12 + 3 + 6, four of them
    later-generation tiles in the exact-f32 / f16 modes - at split_k 1 and 2, and the 15 on a third-generation hint at split_k 3: 105.
    Always refused: those four at every split they are asked at (hint 25 twice, hint 72 three times: 10). The library's own tile choice (hints 0, 1, 4 of the first-generation modes: 9 pairs)
    splits only from 8 slabs per slice; an explicit tile needs one slab per slice. NCTHW: the 14 first-generation pairs, unsplit."""
    ns = k_slabs(c)
    if c.get("out_nchw"):
        return 14, 91
    if ns >= 16:
        return 95, 10
    if ns >= 3:
        return 86, 19
    if ns == 2:
        return 73, 32            # no split_k 3
    return 41, 64                # one slab: no split at all


@pytest.mark.parametrize("name", NAMES)
def test_every_mode_and_tile_is_exact(dev, name):
    c = cc.CASE_BY_NAME[name]
    tally = dict(ran=0, refused=0, v3_native=0, v3_redirected=0)
    # which kernel a third-generation hint really runs: at split_k 1 the library's answer, which the rule written out above must match;
    # a split launch emits its sums from the reduce kernel, so there only the rule can say
    native = {s: runs_the_phased_stream(c, s) for s in V3_SPLITS}
    if not c.get("out_nchw"):
        assert library_runs_the_phased_stream(c) == native[1], name
        native[1] = library_runs_the_phased_stream(c)
    for mode, (wide, hints, refused_hints) in MODES.items():
        d = cc.reference(name, wide)
        o = operands(c, d, mode, dev)
        want = expected(c, d, dev, torch.float32)
        for hint in hints + refused_hints:
            for split in (V3_SPLITS if generation(hint) == 3 else SPLITS):
                label = f"{mode} tile {hint} split_k {split}"
                if is_refused(c, mode, hint, split):
                    if mode == "f16x2" and c.get("out_nchw"):      # refused by an assertion of ops.conv_gemm before the library is asked
                        with pytest.raises(AssertionError, match="two-pass f16 GEMM writes plain f32 rows or plain f16 rows"):
                            launch(c, d, o, hint, split)
                    else:
                        with pytest.raises(RuntimeError):
                            launch(c, d, o, hint, split)
                    tally["refused"] += 1
                    continue
                assert hint not in refused_hints, label
                run = lambda: launch(c, d, o, hint, split)
                got = both_grids(run) if tile_that_is_asked(mode, hint) >= 22 else run()
                assert_exact(c, d, got, want, label)
                tally["ran"] += 1
                if generation(hint) == 3:
                    tally["v3_native" if native[split] else "v3_redirected"] += 1
    print(f"[conv-geometry] {name}: " + " ".join(f"{k}={v}" for k, v in tally.items()))
    assert (tally["ran"], tally["refused"]) == expected_counts(c), tally
    # 13 third-generation (mode, tile) pairs per split; every geometry the phased stream can take at all is run on it
    ran3 = 0 if c.get("out_nchw") else 13 * sum(k_slabs(c) // s >= 1 for s in V3_SPLITS)
    assert tally["v3_native"] == (0 if c.get("out_nchw") else 13 * sum(native.values())) and tally["v3_native"] + tally["v3_redirected"] == ran3, tally
    if c["ups"] == 1 and cc.first_tap_is_monotone(c) and k_slabs(c) >= 4 and k_slabs(c) % 2 == 0 and not c.get("out_nchw"):
        assert tally["v3_native"] >= 13, tally


def test_which_rows_never_reach_the_third_generation_kernel():
    """Exactly these: up-sampled and over-wide geometries (the planner's rule), NCTHW heads (first generation only), and rows with fewer
    than 4 or an odd number of K slabs - the 1x1 rows at one or two slabs (their `_c256` twins do run it) and the 9-slab ups row."""
    never = {c["name"] for c in cc.CASES if c.get("out_nchw") or not any(runs_the_phased_stream(c, s) for s in V3_SPLITS)}
    assert never == {"k3s1p1u2_1x1", "k3s1p1u2_3x5", "k3s1p1u2_4x4", "k1s2p0_8x8", "k1s2p0_7x5", "k1s1p0_lda", "nchw_co16", "nchw_co3_view",
                     "k3s1p2_4x6", "k1s1p1_4x6", "k3s1p2_3x5"}
    at_split_2 = {c["name"] for c in cc.CASES if not c.get("out_nchw") and runs_the_phased_stream(c, 2)}
    assert at_split_2 == {"k3s1p1_9x7_c256", "t311_B2_T3_HW70_c256"}


@pytest.mark.parametrize("name", NAMES)
def test_16_bit_outputs_round_the_exact_answer(dev, name):
    """bf16 / f16 rows out on the library's own tile and on hint 25: the reference rounded to the type by torch (round to nearest even,
    once, after bias / rowbias / residual)."""
    c = cc.CASE_BY_NAME[name]
    d = cc.reference(name, False)
    tally = dict(ran=0, refused=0)
    for mode in ("bf16", "f16"):
        o = operands(c, d, mode, dev)
        dtype = ACT_DTYPE[mode]
        want = expected(c, d, dev, dtype)
        exact = expected(c, d, dev, torch.float64)
        for hint in (0, 25):
            if is_refused(c, mode, hint, 1):
                with pytest.raises(RuntimeError):
                    launch(c, d, o, hint, 1, dtype)
                tally["refused"] += 1
                continue
            run = lambda: launch(c, d, o, hint, 1, dtype)
            got = both_grids(run) if hint >= 22 else run()
            assert got.dtype == dtype
            assert_exact(c, d, got, want, f"{mode} rows out, tile {hint}", exact)
            tally["ran"] += 1
    print(f"[conv-geometry-16] {name}: " + " ".join(f"{k}={v}" for k, v in tally.items()))
    assert tally == (dict(ran=2, refused=2) if c.get("out_nchw") else dict(ran=3, refused=1))
