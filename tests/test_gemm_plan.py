"""CPU tests of the conv_gemm planner (csrc/gemm_plan.h) through geo4d_conv_gemm_colsum_rows, which is pure host code: the answer
for every launch of a sweep equals the answer the library gave BEFORE the planner existed, when the query was a computation of its
own next to the launch path.

tests/golden/gemm_colsum_rows.json was recorded with this module run as a script (`python tests/test_gemm_plan.py OUT.json`) with
GEO4D_HIP_LIB pointing at libgeo4d_hip.so built from the commit before the planner (cbd54cf); it holds one comma-separated string
of answers per (shape, element type, output type, operand format), in the order of `variants()`.

The sweep: element types 1 (bf16), 3 (bf16x3), 4 (two-pass f16); every hint of ops._CANDIDATES; split_k 1, 2, 4 and an uneven 3;
act 0 (none), 1 (SiLU), 2 (GEGLU); residual on / off; o_split 0 and, where the element type has one, 1 (bf16x3) / 2 (two-pass f16);
shapes of the tuning table, among them M not a multiple of the wave-tile rows (40960 on 96 rows, 640 on 96), odd K-slab counts
(2880 / 64 = 45 for bf16, 288 / 32 = 9 for the 4-byte types), ups = 2, batch 16 and frames of 5 x 8 = 40 rows (a multiple of 8, not
of 32). The query validates nothing: it is asked about descriptors the launch refuses too (GEGLU with a residual, the two-pass type
on a first-generation hint) and the recorded answers cover those as well. The workspace is a fake pointer of 2^40 bytes so that
split-K is never refused for the size of a buffer this test does not own (the old query did not look at the workspace)."""
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_colsum_rows.json")

# (M x N x K, Cin, taps KT KH KW, stride, ups, batch) as in the tuning table's keys + the geometry the key does not carry: T, Hout, Wout
SHAPES = [
    ("40960x320x2880|c320|t133s1u1", 1, 16, 40, 64),       # level 0 conv 3x3: 16 frames of 40 x 64
    ("10240x640x5760|c640|t133s1u1", 1, 16, 20, 32),
    ("2560x1280x11520|c1280|t133s1u2", 1, 16, 10, 16),     # nearest-2x upsample folded into the gather
    ("2560x640x5760|c640|t133s2u1", 1, 16, 10, 16),        # stride 2
    ("640x1280x11520|c1280|t133s1u1", 1, 16, 5, 8),        # 40 rows per frame
    ("640x1280x3840|c1280|t311s1u1", 1, 16, 5, 8),         # temporal conv
    ("640x10240x1280|c1280|t111s1u1", 1, 16, 5, 8),        # the GEGLU projection's shape
    ("122880x320x288|c32|t133s1u1", 1, 48, 40, 64),        # 9 K slabs of 32
    ("1280x160x1280|c1280|t111s1u1", 16, 1, 1280, 1),      # batched
    ("77x12480x1024|c1024|t111s1u1", 1, 1, 77, 1),         # M % 32 != 0 (the context projections)
]
SPLITS = (1, 2, 4, 3)
ACTS = (0, 1, 2)
# (dtype, out_dtype, a_split, w_split, o_splits)
FORMATS = [(1, 1, 0, 0, (0,)), (1, 0, 0, 0, (0,)), (3, 0, 0, 1, (0,)), (3, 0, 1, 1, (0, 1)), (4, 0, 2, 1, (0, 2))]


def hints():
    from geo4d_amd import ops
    return sorted({t for t, _ in ops._CANDIDATES})


def variants():
    return [(h, s, a, r, o) for h in hints() for s in SPLITS for a in ACTS for r in (0, 1) for o in (0, 1, 2)]


def descriptor(shape, batch, T, Hout, Wout, fmt, hint, split, act, res, o_split):
    from geo4d_amd import _lib
    M, N, K, Cin, KT, KH, KW, stride, ups = (int(x) for x in re.match(r"(\d+)x(\d+)x(\d+)\|c(\d+)\|t(\d)(\d)(\d)s(\d)u(\d)$", shape).groups())
    dtype, out_dtype, a_split, w_split, _ = fmt
    nout = N // 2 if act == 2 else N
    p = _lib.ConvGemm()
    p.A, p.W, p.O, p.bias, p.zeros, p.workspace = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000
    p.R = 0x70000000 if res else 0
    p.workspace_bytes = 1 << 40
    p.M, p.N, p.K, p.Cin, p.batch = M, N, K, Cin, batch
    p.T, p.Hout, p.Wout = T, Hout, Wout
    p.Hin, p.Win = (Hout * stride) // ups, (Wout * stride) // ups
    p.KT, p.KH, p.KW, p.pt, p.ph, p.pw, p.stride, p.ups = KT, KH, KW, KT // 2, KH // 2, KW // 2, stride, ups
    p.lda, p.ldw, p.ldo, p.ldr = Cin, K, nout, (nout if res else 0)
    p.a_bs, p.w_bs, p.o_bs, p.r_bs = M * Cin, N * K, M * nout, (M * nout if res else 0)
    p.dtype, p.out_dtype, p.a_split, p.w_split, p.o_split = dtype, out_dtype, a_split, w_split, o_split
    p.act, p.alpha, p.tile_hint, p.split_k = act, 1.0, hint, split
    return p


def sweep(lib):
    """{row key: [answers in the order of variants(), o_split values the format does not have left out]}"""
    out = {}
    for shape, batch, T, Hout, Wout in SHAPES:
        for fmt in FORMATS:
            key = f"{shape}|b{batch}|d{fmt[0]}o{fmt[1]}x{fmt[2]}{fmt[3]}"
            out[key] = [lib.geo4d_conv_gemm_colsum_rows(ctypes.byref(descriptor(shape, batch, T, Hout, Wout, fmt, h, s, a, r, o)))
                        for h, s, a, r, o in variants() if o in fmt[4]]
    return out


def test_sweep_shapes_come_from_the_tuning_table():
    table = json.load(open(os.path.join(ROOT, "geo4d_amd", "tuning", "gfx950.json")))
    for shape, batch, *_ in SHAPES:
        assert any(f"|{shape}|" in k and k.split("|")[5] == f"b{batch}" for k in table), shape


def test_colsum_rows_answers_as_before_the_planner():
    from geo4d_amd import _lib, ops
    golden = json.load(open(GOLDEN))
    got = sweep(_lib.load())
    assert set(got) == set(golden)
    n = 0
    for key, answers in got.items():
        want = [int(x) for x in golden[key].split(",")]
        asked = [v for v in variants() if v[4] in next(f for f in FORMATS if key.endswith(f"d{f[0]}o{f[1]}x{f[2]}{f[3]}"))[4]]
        assert len(want) == len(answers) == len(asked)
        wrong = [(v, w, g) for v, w, g in zip(asked, want, answers) if w != g]
        assert not wrong, (key, len(wrong), wrong[:8])      # ((hint, split_k, act, residual, o_split), recorded, now)
        n += len(answers)
    assert n > 20000
    # the table holds zero and non-zero answers for every generation
    seen = {}
    for key, row in golden.items():
        fmt = next(f for f in FORMATS if key.endswith(f"d{f[0]}o{f[1]}x{f[2]}{f[3]}"))
        for v, w in zip([v for v in variants() if v[4] in fmt[4]], row.split(",")):
            seen.setdefault(ops._generation(v[0]), set()).add(int(w) > 0)
    assert seen == {1: {False, True}, 2: {False, True}, 3: {False, True}}, seen


def geometry_descriptor(Hin, Win, KH, KW, ph, pw, frames, Cin=128, stride=1, hint=73):
    """bf16 rows in, f32 rows out, hint 73 (256 x 128 on 2 x 4 waves: 128 rows per gn_colsum entry; its second-generation twin 25: 64)."""
    Hout, Wout = (Hin + 2 * ph - KH) // stride + 1, (Win + 2 * pw - KW) // stride + 1
    M, K = frames * Hout * Wout, KH * KW * Cin
    p = descriptor(f"{M}x64x{K}|c{Cin}|t1{KH}{KW}s{stride}u1", 1, 1, Hout, Wout, FORMATS[1], hint, 1, 0, 0, 0)
    p.Hin, p.Win, p.ph, p.pw = Hin, Win, ph, pw
    return p


def test_geometries_whose_rows_walk_backwards_leave_the_third_generation():
    """The third generation addresses a tile's rows with unsigned offsets from the first tap of the tile's first row, so it may only take
    geometries in which that pixel never decreases with the row: Wout - 1 <= Win and ((Hout - 1) Win + Wout - 1) stride <= Hin Win.
    Descriptors on both sides of each condition, told apart by the rows per gn_colsum entry of the tile that really runs (128 on hint
    73, 64 on its second-generation twin); every one has an even number >= 4 of K slabs and M a multiple of 128."""
    from geo4d_amd import _lib
    lib = _lib.load()
    rows = lambda p: lib.geo4d_conv_gemm_colsum_rows(ctypes.byref(p))
    native = [geometry_descriptor(8, 8, 3, 3, 1, 1, 16),                  # the networks' 3x3, pad 1
              geometry_descriptor(8, 8, 3, 3, 1, 1, 32, stride=2),        # stride 2
              geometry_descriptor(7, 3, 2, 3, 1, 0, 16),                  # both conditions with equality: Hout = Hin + 1, Wout = 1
              geometry_descriptor(8, 8, 1, 2, 0, 1, 16, Cin=256)]         # a 1x2 kernel with pad (0, 1): Wout - 1 == Win, again with equality in both
    redirected = [geometry_descriptor(8, 8, 3, 3, 2, 2, 32),              # 3x3 with pad 2: both conditions broken
                  geometry_descriptor(8, 8, 3, 3, 2, 1, 16),              # rows only: Hout = Hin + 2 (the second condition)
                  geometry_descriptor(8, 8, 3, 3, 0, 2, 32),              # columns only: Wout - 1 = 9 > Win, 5 * 8 + 9 <= 64 (the first condition)
                  geometry_descriptor(8, 8, 3, 3, 1, 2, 16),              # pad (1, 2): both again, the second by one pixel (65 > 64)
                  geometry_descriptor(6, 6, 1, 1, 1, 1, 2, Cin=256)]      # a padded 1x1 (both)
    for p in native + redirected:
        assert p.M % 128 == 0 and (p.K // 64) % 2 == 0 and p.K // 64 >= 4, (p.M, p.K)
    assert [rows(p) for p in native] == [128] * len(native)
    assert [rows(p) for p in redirected] == [64] * len(redirected)
    for p in native + redirected:      # the second-generation tile itself answers 64 either way
        p.tile_hint = 25
        assert rows(p) == 64


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from geo4d_amd import _lib
    rows = {k: ",".join(str(x) for x in v) for k, v in sweep(_lib.load()).items()}
    with open(sys.argv[1], "w") as f:
        json.dump(rows, f, indent=0, sort_keys=True)
    print(len(rows), "rows,", sum(len(v.split(",")) for v in rows.values()), "answers")
