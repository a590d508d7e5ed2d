"""CPU tests of the conv_gemm planner (csrc/gemm_plan.h) through its pure-host queries geo4d_conv_gemm_plan, geo4d_conv_gemm_tiles and
geo4d_conv_gemm_colsum_rows, and of the host policy on top of it in ops.py (_tuned_config, _f16_rows_config). No test here launches a
descriptor that the plan accepts. First the oldest query: the colsum_rows answer for every launch of a sweep equals the answer the
library gave BEFORE the planner existed, when the query was a computation of its own next to the launch path.

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
GOLDEN_PLANS = os.path.join(ROOT, "tests", "golden", "gemm_plans.json")
GOLDEN_REFUSALS = os.path.join(ROOT, "tests", "golden", "gemm_refusals.json")

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


def sweep(lib, query=None):
    """{row key: [answers of `query(descriptor)` in the order of variants(), o_split values the format does not have left out]}"""
    query = query or (lambda p: lib.geo4d_conv_gemm_colsum_rows(ctypes.byref(p)))
    out = {}
    for shape, batch, T, Hout, Wout in SHAPES:
        for fmt in FORMATS:
            key = f"{shape}|b{batch}|d{fmt[0]}o{fmt[1]}x{fmt[2]}{fmt[3]}"
            out[key] = [query(descriptor(shape, batch, T, Hout, Wout, fmt, h, s, a, r, o)) for h, s, a, r, o in variants() if o in fmt[4]]
    return out


def asked_of(key):
    """The variants() a row of sweep() holds answers for."""
    fmt = next(f for f in FORMATS if key.endswith(f"d{f[0]}o{f[1]}x{f[2]}{f[3]}"))
    return [v for v in variants() if v[4] in fmt[4]]


def plan_of(lib, p):
    """(_lib.ConvGemmPlan, 0) of the descriptor, or (None, return code) where the library refuses it."""
    from geo4d_amd import _lib
    plan = _lib.ConvGemmPlan()
    rc = lib.geo4d_conv_gemm_plan(ctypes.byref(p), ctypes.byref(plan))
    return (plan, 0) if rc == 0 else (None, rc)


def plan_answer(lib, p):
    """One answer of the plan sweep as the golden file spells it: "hint/splits/hot/osplit/colsum_rows", or the return code of a refusal."""
    plan, rc = plan_of(lib, p)
    return str(rc) if plan is None else f"{plan.tile_hint}/{plan.splits}/{plan.hot}/{plan.osplit}/{plan.colsum_rows}"


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
    assert [plan_of(lib, p)[0].tile_hint for p in native] == [73] * len(native)              # the plan says so itself
    assert [plan_of(lib, p)[0].tile_hint for p in redirected] == [25] * len(redirected)
    assert [rows(p) for p in native] == [128] * len(native)
    assert [rows(p) for p in redirected] == [64] * len(redirected)
    for p in native + redirected:      # the second-generation tile itself answers 64 either way
        p.tile_hint = 25
        assert rows(p) == 64


def test_plan_answers_as_the_parent_planner_did():
    """geo4d_conv_gemm_plan = validate() + resolve() for every descriptor of the sweep above (same SHAPES, FORMATS and variants(), more
    than 20000 descriptors): return code, and where accepted the tile that runs, splits, operand-layout variant, producer-format output
    and colsum_rows equal what the commit BEFORE validate() moved into the planner (4a2fcbb) decided inside geo4d_conv_gemm.

    tests/golden/gemm_plans.json was recorded from that commit without launching anything: a stand-alone host library (g++, no HIP)
    made of its gemm.hip's descriptor checks - the lines between `const geo4d_conv_gemm_t& p = *pp;` and `const Plan plan = resolve(p);`
    copied verbatim into a function - followed by its gemm_plan.h's resolve(), exporting `int parent_plan(const geo4d_conv_gemm_t*, int
    out[5])` (return code; hint, splits, hot, osplit, colsum_rows). This module run as `python tests/test_gemm_plan.py plans
    RECORDER.so OUT.json` fills the descriptors with the same `descriptor()` the test uses and writes one comma-separated string per
    (shape, element type, output type, operand format) in the order of `variants()`: "hint/splits/hot/osplit/colsum_rows" per
    accepted descriptor, the return code per refused one (nothing else is compared there)."""
    from geo4d_amd import _lib
    lib = _lib.load()
    golden = json.load(open(GOLDEN_PLANS))
    got = sweep(lib, lambda p: (plan_answer(lib, p), lib.geo4d_conv_gemm_colsum_rows(ctypes.byref(p))))
    assert set(got) == set(golden)
    n = accepted = 0
    for key, answers in got.items():
        want, asked = golden[key].split(","), asked_of(key)
        assert len(want) == len(answers) == len(asked)
        wrong = [(v, w, g) for v, w, (g, _) in zip(asked, want, answers) if w != g]
        assert not wrong, (key, len(wrong), wrong[:8])      # ((hint, split_k, act, residual, o_split), recorded, now)
        # where the plan accepts, the older query gives the same colsum_rows
        wrong = [(v, g, rows) for v, (g, rows) in zip(asked, answers) if "/" in g and int(g.split("/")[4]) != rows]
        assert not wrong, (key, len(wrong), wrong[:8])
        n += len(answers)
        accepted += sum("/" in g for g, _ in answers)
    assert n > 20000 and 2000 < accepted < n - 2000, (n, accepted)      # the sweep holds plenty of both


def refusal_base(**kw):
    """bf16 rows x bf16 weight -> bf16 rows, 256 x 256 x 512 as one frame of 256 x 1 pixels, hint 25: accepted as it stands."""
    p = descriptor("256x256x512|c512|t111s1u1", 1, 1, 256, 1, FORMATS[0], 25, 1, 0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


PTR = 0x70000000
X3SPLIT = dict(dtype=3, out_dtype=0, a_split=1, w_split=1)        # bf16x3, pre-split x pre-split, f32 rows
TWO_PASS = dict(dtype=4, out_dtype=0, a_split=2, w_split=1)       # two-pass f16
# One descriptor per distinct message of validate() (19) and resolve() (9 of its 10: "o_split is a bf16x3 / f16x2 option" cannot be reached
# through validate(), whose o_split check refuses every such descriptor first - only geo4d_conv_gemm_colsum_rows gets there).
REFUSALS = [
    ("bad_dtype", dict(dtype=5)),
    ("split_flags_on_a_plain_type", dict(a_split=1)),
    ("two_pass_without_f16_rows", dict(TWO_PASS, a_split=1)),
    ("o_split_with_split_k", dict(X3SPLIT, o_split=1, split_k=2)),
    ("empty_problem", dict(M=0)),
    ("too_many_taps", dict(KT=2, KH=3, KW=3)),
    ("cin_not_a_slab_multiple", dict(Cin=500)),
    ("unaligned_operand_rows", dict(lda=513)),
    ("rows_not_whole_frames", dict(Hout=100)),
    ("frames_not_a_multiple_of_T", dict(Hout=128, T=3)),
    ("too_many_input_pixels", dict(Hout=1, Hin=65536, Win=256)),
    ("bad_ups", dict(ups=3)),
    ("geglu_with_residual", dict(act=2, R=PTR, ldr=128)),
    ("unknown_act", dict(act=4)),
    ("gelu_with_residual", dict(act=3, R=PTR, ldr=256)),
    ("rowbias_without_div", dict(rowbias=PTR)),
    ("batch_too_large", dict(batch=65536)),
    ("no_zeros", dict(zeros=0)),
    ("unaligned_workspace", dict(workspace=0x60000008)),
    # resolve()
    ("later_generations_refuse_f32", dict(dtype=0, out_dtype=0)),
    ("later_generations_refuse_ncthw", dict(out_nchw=1)),
    ("no_scored_tile_takes_it", dict(tile_hint=5, act=2)),
    ("split_k_without_workspace", dict(split_k=2, workspace=0)),
    ("unknown_tile_hint", dict(tile_hint=30)),
    ("geglu_on_narrow_wave_tiles", dict(tile_hint=23, act=2)),
    ("f16_rows_with_residual", dict(TWO_PASS, o_split=2, R=PTR, ldr=256)),
    ("presplit_out_with_unaligned_residual", dict(X3SPLIT, o_split=1, R=PTR, ldr=1)),
    ("colsum_from_16_bit_rows", dict(gn_colsum=PTR)),
]


def refusals(lib, query):
    """[[name, return code, message]] of `query(pointer to descriptor)` for every case of REFUSALS"""
    out = []
    for name, kw in REFUSALS:
        rc = query(ctypes.byref(refusal_base(**kw)))
        out.append([name, rc, lib.geo4d_last_error().decode() if rc else ""])
    return out


def test_refusals_keep_their_code_and_message():
    """tests/golden/gemm_refusals.json holds (name, return code, message) of geo4d_conv_gemm itself for the REFUSALS, recorded from the
    library of the commit before validate() moved (4a2fcbb; its checks run before any device call): `python tests/test_gemm_plan.py
    refusals LIBRARY.so OUT.json`. Every case is refused by the plan query FIRST, with the recorded code and
    message, and only then handed to the launch, which must say the same."""
    from geo4d_amd import _lib
    lib = _lib.load()
    golden = json.load(open(GOLDEN_REFUSALS))
    assert [g[0] for g in golden] == [name for name, _ in REFUSALS]
    assert len({g[2] for g in golden}) == len(golden) == 28 and all(g[1] == -22 and g[2].startswith("conv_gemm: ") for g in golden)
    assert plan_of(lib, refusal_base())[0].tile_hint == 25         # the base itself is fine: every case is refused for what it changes
    plan = _lib.ConvGemmPlan()
    by_plan = refusals(lib, lambda p: lib.geo4d_conv_gemm_plan(p, ctypes.byref(plan)))
    assert by_plan == golden
    assert refusals(lib, lambda p: lib.geo4d_conv_gemm(p, None)) == golden       # (all refused above: nothing is launched)
    assert lib.geo4d_conv_gemm_plan(None, ctypes.byref(plan)) == -22 and lib.geo4d_conv_gemm_plan(ctypes.byref(refusal_base()), None) == -22


def test_tile_table_rows_are_what_the_plan_runs():
    from geo4d_amd import _lib
    lib = _lib.load()
    rows = (_lib.ConvGemmTile * 64)()
    n = lib.geo4d_conv_gemm_tiles(rows, 64)
    assert n == 18 == lib.geo4d_conv_gemm_tiles(None, 0) and [t.tile_hint for t in rows[:n]] == hints()
    two = (_lib.ConvGemmTile * 2)()
    assert lib.geo4d_conv_gemm_tiles(two, 2) == 18 and [t.tile_hint for t in two] == [1, 2]       # (cap is respected)
    for t in rows[:n]:
        # bf16, 1280 x 1280 x 512 (8 K slabs: even and >= 4, so the third generation takes it), un-split: every tile runs it natively
        p = descriptor("1280x1280x512|c512|t111s1u1", 1, 1, 1280, 1, FORMATS[0], t.tile_hint, 1, 0, 0, 0)
        plan, rc = plan_of(lib, p)
        assert rc == 0 and (plan.tile_hint, plan.bm, plan.bn, plan.wm, plan.wn) == (t.tile_hint, t.bm, t.bn, t.wm, t.wn), t.tile_hint
        gen = 3 if t.tile_hint >= 71 else 2 if t.tile_hint >= 21 else 1          # generation(hint) of gemm_plan.h
        assert t.generation == plan.generation == gen
        assert t.geglu == int((t.bn // t.wn) % 64 == 0) and t.bn % t.wn == 0


def test_f16_row_geglu_goes_to_the_nearest_tile_that_takes_one():
    from geo4d_amd import _lib, ops
    want = {22: 25, 23: 25, 25: 25, 27: 27, 28: 27, 71: 71, 72: 71, 73: 74, 74: 74}
    tiles = ops._tiles()
    assert set(tiles) == set(hints()) and all(isinstance(t, _lib.ConvGemmTile) for t in tiles.values())
    for h in hints():
        target = want[h] if h >= 21 else h
        for s in (0, 1, 2, 8):
            assert ops._f16_rows_config((h, s), 2) == (target, min(s, 1))
            assert ops._f16_rows_config((h, s), 0) == (h, min(s, 1))
        if h >= 21:
            assert tiles[target].geglu == 1 and tiles[target].generation == tiles[h].generation
    assert ops._f16_rows_config((0, 0), 2) == (0, 0) and ops._f16_rows_config((0, 4), 0) == (0, 1)


def test_tuned_config_borrowing(monkeypatch):
    """ops._tuned_config on a literal table: whose entry a launch without one of its own runs on."""
    from geo4d_amd import ops
    monkeypatch.setattr(ops, "TUNE_EXACT", 0)
    yes, no = (lambda: True), (lambda: False)
    base = "3/0|640x1280x3840|c1280|t311s1u1|a0r0n0|b1"
    table = {base + "|x11": (71, 2), base + "|x01": (25, 4), base + "|x10": (27, 1), base + "|x11o": (74, 1)}
    cfg = lambda key, o_split, may, code=3, t=table: ops._tuned_config(t, key, code, 1, 1, o_split, may)
    assert cfg(base + "|x11o", 1, no) == (74, 1) and cfg(base + "|x11", 0, yes) == (71, 2)          # its own entry wins
    # a pre-split bf16x3 key borrows |x11 (pre-split output only), then |x01, then |x10
    own = {k: v for k, v in table.items() if not k.endswith("o")}
    assert cfg(base + "|x11o", 1, no, t={k: v for k, v in own.items() if "|x11" not in k}) == (25, 1)      # (split dropped, see below)
    assert cfg(base + "|x11", 0, no, t={base + "|x01": (25, 4), base + "|x10": (27, 1)}) == (25, 4)
    assert cfg(base + "|x11", 0, no, t={base + "|x10": (27, 1)}) == (27, 1)
    assert cfg(base + "|x11", 0, no, t={}) is None
    assert cfg(base + "|x11", 0, no, t={base + "|x11o": (74, 1)}) is None                            # ("o" entries are never lent)
    # a borrowed split > 1 with a pre-split output: the tile without the split, or a measurement where that is allowed
    assert cfg(base + "|x11o", 1, no, t=own) == (71, 1)
    assert cfg(base + "|x11o", 1, yes, t=own) is None
    assert cfg(base + "|x11o", 1, yes, t={base + "|x11": (73, 1)}) == (73, 1)
    monkeypatch.setattr(ops, "TUNE_EXACT", 1)                                                       # tools/tune_gemm.py: no borrowing while measuring
    assert cfg(base + "|x11", 0, yes, t={base + "|x01": (25, 4)}) is None and cfg(base + "|x11", 0, no, t={base + "|x01": (25, 4)}) == (25, 4)
    monkeypatch.setattr(ops, "TUNE_EXACT", 0)
    # a two-pass f16 key borrows the bf16x3 entry of the same shape - when nothing may be measured, and only second / third generation tiles
    k4 = "4" + base[1:]
    x2 = lambda t, o_split, may, key=k4 + "|x11": ops._tuned_config(t, key, 4, 2, 1, o_split, may)
    assert x2({base + "|x11": (72, 2)}, 0, no) == (72, 2)
    assert x2({base + "|x11": (72, 2)}, 0, yes) is None
    assert x2({base + "|x11": (11, 2)}, 0, no) is None and x2({base + "|x11": (17, 1)}, 0, no) is None
    assert x2({base + "|x11o": (72, 2)}, 2, no, key=k4 + "|x11o") == (72, 1)                         # (f16 rows out: no split-K form)
    assert x2({base + "|x11": (72, 2), k4 + "|x11": (25, 1)}, 0, no) == (25, 1)                      # its own entry wins


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from geo4d_amd import _lib
    if sys.argv[1] == "plans":            # plans RECORDER.so OUT.json (see test_plan_answers_as_the_parent_planner_did)
        rec = ctypes.CDLL(sys.argv[2])
        out5 = (ctypes.c_int * 5)()

        def recorded(p):
            rc = rec.parent_plan(ctypes.byref(p), out5)
            return str(rc) if rc else "/".join(str(x) for x in out5)
        rows = {k: ",".join(v) for k, v in sweep(None, recorded).items()}
    elif sys.argv[1] == "refusals":       # refusals LIBRARY.so OUT.json (an older library lacks the newer queries: plain ctypes, not _lib.load())
        lib = ctypes.CDLL(sys.argv[2])
        lib.geo4d_last_error.restype = ctypes.c_char_p
        rows = refusals(lib, lambda p: lib.geo4d_conv_gemm(p, None))
    else:
        rows = {k: ",".join(str(x) for x in v) for k, v in sweep(_lib.load()).items()}
    with open(sys.argv[-1], "w") as f:
        json.dump(rows, f, indent=0, sort_keys=True)
    print(len(rows), "rows,", sum(len(v.split(",")) for v in rows.values()) if isinstance(rows, dict) else "", "answers")
