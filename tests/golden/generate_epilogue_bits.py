"""Bit-identity cases for the conv_gemm epilogues (first-generation direct / staged paths, the register epilogue's fast and generic
paths of the second / third generation, the split-K reduce kernels), and the recorder of their expected values.

    python tests/golden/generate_epilogue_bits.py [--out tests/golden/gemm_epilogue_bits.json] [--dump DIR] [--only SUBSTR]

Run it on an MI355X AT THE COMMIT WHOSE BITS ARE THE REFERENCE (the parent of an epilogue refactor) and commit the JSON;
tests/test_gemm_epilogue_bits_gpu.py re-runs the same cases and compares the SHA-256 of the output bytes (and of the gn_colsum bytes
where the launch emits them), so the expected values never come from the code under test. `--dump DIR` also saves every tensor
(`<case>.pt`) so that a mismatch can be diffed by hand.

Every case launches through geo4d_amd.ops with an explicit tile_hint and split_k (the tuning table plays no part); inputs are drawn on
the CPU from a seeded torch.Generator. Cases of the persistent generations run twice: with the production grid and with
debug_ablate = 2 (three workgroups, so the small shapes walk the tile loop).

Shapes: M = 200 (ragged against every tile height), N = 192 (ragged against 128 / 256 / 320 columns, a multiple of 64 for GEGLU), four
K slabs (eight with split_k = 2: the phased kernel needs an even count >= 4 per split); gn_colsum cases use M = 256, or 320 on the
80-row wave tiles."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_epilogue_bits.json")
M, N = 200, 192
GEN1_EVEN, GEN1_ODD = 1, 5            # 128x128 (two 32-column blocks per wave), 128x32 (one)
V2_EVEN, V2_ODD = 25, 23              # 128x128 (64x64 wave tiles: four 16-column blocks), 160x320 (80x80: five)
V3_EVEN, V3_ODD = 74, 72              # 128x256 (64x64), 160x320 (80x80)
PERSISTENT = (V2_EVEN, V2_ODD, V3_EVEN, V3_ODD)
GEGLU_TILES = (V2_EVEN, V3_EVEN)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


# ---- operand formats ------------------------------------------------------------------------------------------------------------------
# mode -> (activation of f32 values, weight packer name suffix). "x3" = raw f32 rows x pre-split weight, "x3pre" = pre-split rows x
# pre-split weight (the only form that can write the pre-split output), "f16x2" = the two-pass f16 type.
def act_of(x, mode, dev):
    from geo4d_amd import ops, pack
    if mode == "x3pre":
        return ops.SplitAct.wrap(pack.split_bf16(x).to(dev))
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "x3": torch.float32, "f16x2": torch.float16}[mode]
    return x.to(dt).contiguous().to(dev)


def pack_mode(mode):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "x3": "bf16x3", "x3pre": "bf16x3", "f16x2": "bf16x3m"}[mode]


def packed(kind, w, mode, b=None):
    from geo4d_amd import pack
    x2 = "_x2" if mode == "f16x2" else ""
    fn = getattr(pack, f"pack_{kind}{x2}")
    return fn(w, b, pack_mode(mode)) if kind == "geglu" else fn(w, pack_mode(mode))


def kslab(mode):
    return 64 if mode in ("bf16", "f16") else 32


def row_dtype(mode, out_dtype=None):
    return out_dtype or {"bf16": torch.bfloat16, "f16": torch.float16}.get(mode, torch.float32)


# ---- one launch -----------------------------------------------------------------------------------------------------------------------
def linear_case(dev, mode, tile, *, split=1, m=M, n=N, slabs=4, bias=True, bias_per_row=False, table=False, res=False, act=0, gn=False,
                out_dtype=None, split_out=False, pitch=None, seed=1):
    """out = epilogue(x @ w^T): every epilogue option of a plain GEMM. `pitch`: row pitch of the output (and residual) in elements -
    a column-offset-free view of a wider buffer, for the unaligned paths. Returns {"out": ..., "colsum": ...}."""
    from geo4d_amd import ops
    k = kslab(mode) * slabs * split
    x = act_of(rnd((m, k), seed), mode, dev)
    wf, bf = rnd((n, k), seed + 1, 0.05), rnd((n,), seed + 2)
    if act == 2:
        w, b = packed("geglu", wf, mode, bf)
        w, b = w.to(dev), b.to(dev)
    else:
        w, b = packed("linear", wf, mode).to(dev), bf.to(dev)
    nout = n // 2 if act == 2 else n
    rdt = row_dtype(mode, out_dtype)
    if split_out:
        out = ops.new_split(m, nout, dev, "f16" if mode == "f16x2" else "bf16")
    else:
        out = torch.zeros((m, pitch or nout), device=dev, dtype=rdt)[:, :nout]
    kw = dict(act=act, tile_hint=tile, split_k=split, gn_stats=gn)
    if bias_per_row:
        kw.update(bias=rnd((m,), seed + 3).to(dev), bias_per_row=True)
    elif bias:
        kw.update(bias=b)
    if table:                          # row-bias table: one row per 50 output rows
        kw.update(rowbias=rnd(((m + 49) // 50, n), seed + 4).to(dev), rowbias_div=50)
    if res:
        r = torch.zeros((m, pitch or nout), device=dev, dtype=torch.float32 if split_out else rdt)[:, :nout]
        r.copy_(rnd((m, nout), seed + 5))
        kw.update(residual=r, ldr=ops._ld(r))
    ops.conv_gemm(x, w, out, M=m, N=n, K=k, Cin=k, lda=ops._ld(x), ldw=ops._ld(w), ldo=ops._ld(out), **kw)
    return finish(out, gn)


def conv1x1_case(dev, mode, tile, *, split, F, H, W, n, gn=True, seed=40):
    """A 1x1 convolution with a frame geometry, so that a split-K launch's reduce emits gn_colsum (32 rows, or 8 where a frame's rows
    are a multiple of 8 but not of 32): column bias + row-bias table + residual."""
    from geo4d_amd import ops
    c = kslab(mode) * 4 * split
    x = act_of(rnd((F * H * W, c), seed), mode, dev)
    w, b = packed("conv2d", rnd((n, c, 1, 1), seed + 1, 0.05), mode).to(dev), rnd((n,), seed + 2).to(dev)
    emb, r = rnd((F, n), seed + 3).to(dev), rnd((F * H * W, n), seed + 4).to(row_dtype(mode)).to(dev)
    out = ops.conv2d(x, w, b, F=F, Hin=H, Win=W, KH=1, KW=1, rowbias=emb, rowbias_div=H * W, residual=r, tile_hint=tile, split_k=split, gn_stats=gn)[0]
    return finish(out, gn)


def conv3x3_case(dev, mode, tile, *, split=1, seed=60):
    """3x3, padding 1, stride 2, T = 2, row-bias table per frame, residual: 4 frames of 15 x 13 -> 8 x 7 = 224 output rows (the gather table
    of the first two generations, the tap masks of the third); 18 K slabs."""
    from geo4d_amd import ops
    F, H, W, c = 4, 15, 13, kslab(mode) * 2
    x = act_of(rnd((F * H * W, c), seed), mode, dev)
    w, b = packed("conv2d", rnd((N, c, 3, 3), seed + 1, 0.03), mode).to(dev), rnd((N,), seed + 2).to(dev)
    emb, r = rnd((F, N), seed + 3).to(dev), rnd((F * 56, N), seed + 4).to(row_dtype(mode)).to(dev)
    out = ops.conv2d(x, w, b, F=F, Hin=H, Win=W, KH=3, KW=3, stride=2, pad=1, T=2, rowbias=emb, rowbias_div=56, residual=r, tile_hint=tile, split_k=split)[0]
    return finish(out, False)


def temporal_case(dev, mode, tile, seed=70):
    """3-tap temporal convolution, 2 clips of 5 frames of 21 pixels = 210 rows, residual; 6 K slabs."""
    from geo4d_amd import ops
    B, T, HW, c = 2, 5, 21, kslab(mode) * 2
    x = act_of(rnd((B * T * HW, c), seed), mode, dev)
    w, b = packed("conv3d_t", rnd((N, c, 3, 1, 1), seed + 1, 0.05), mode).to(dev), rnd((N,), seed + 2).to(dev)
    r = rnd((B * T * HW, N), seed + 3).to(row_dtype(mode)).to(dev)
    return finish(ops.conv_temporal(x, w, b, B=B, T=T, HW=HW, residual=r, tile_hint=tile, split_k=1), False)


def ncthw_case(dev, mode, tile, seed=80):
    """The NCTHW head: 3x3, N = 3, T = 2 (first generation's direct path: lanes along pixels)."""
    from geo4d_amd import ops
    F, H, W, c = 4, 9, 7, kslab(mode)
    x = act_of(rnd((F * H * W, c), seed), mode, dev)
    w, b = packed("conv2d", rnd((3, c, 3, 3), seed + 1, 0.05), mode).to(dev), rnd((3,), seed + 2).to(dev)
    return finish(ops.conv2d(x, w, b, F=F, Hin=H, Win=W, KH=3, KW=3, pad=1, T=2, out_nchw=True, tile_hint=tile, split_k=1)[0], False)


def finish(out, gn):
    res = {"out": out.as_subclass(torch.Tensor).contiguous()}
    if gn:
        cs = getattr(out, "_gn_colsum", None)
        assert cs is not None, "this launch was meant to emit gn_colsum"
        res["colsum"] = cs
        res["colsum_rows"] = torch.tensor([out._gn_colsum_rows])
    return res


# ---- the case list --------------------------------------------------------------------------------------------------------------------
def build_cases():
    """name -> (function, args, kwargs, persistent?, gn_fused_level)"""
    cases = {}

    def add(name, fn, tile, mode, level=1, **kw):
        assert name not in cases, name
        cases[name] = (fn, (mode, tile), kw, tile in PERSISTENT, level)

    # first generation -----------------------------------------------------------------------------------------------------------------
    for t in (GEN1_EVEN, GEN1_ODD):
        for mode in ("bf16", "f32"):
            add(f"g1/direct_ncthw/{mode}/t{t}", ncthw_case, t, mode)
            add(f"g1/direct_pitch193_silu_res/{mode}/t{t}", linear_case, t, mode, act=1, res=True, pitch=193)
            add(f"g1/direct_pitch193_table_rowbias/{mode}/t{t}", linear_case, t, mode, bias_per_row=True, table=True, pitch=193)
        for mode in ("f32", "bf16", "f16", "x3"):
            add(f"g1/staged_res/{mode}/t{t}", linear_case, t, mode, res=True)
            add(f"g1/staged_gn/{mode}/t{t}", linear_case, t, mode, level=2, m=256, res=True, gn=True)
        add(f"g1/staged_table_rowbias_silu/bf16/t{t}", linear_case, t, "bf16", bias_per_row=True, table=True, act=1)
        add(f"g1/staged_gelu/bf16/t{t}", linear_case, t, "bf16", act=3)
        add(f"g1/conv3x3/bf16/t{t}", conv3x3_case, t, "bf16")
        add(f"g1/temporal/x3/t{t}", temporal_case, t, "x3")
    for mode in ("f32", "bf16", "x3"):
        add(f"g1/staged_geglu/{mode}/t{GEN1_EVEN}", linear_case, GEN1_EVEN, mode, act=2)
    add(f"g1/direct_pitch97_geglu/bf16/t{GEN1_EVEN}", linear_case, GEN1_EVEN, "bf16", act=2, pitch=97)
    add("g1/staged_res/bf16/t16", linear_case, 16, "bf16", res=True)                 # 10 waves, five 32-column blocks per wave
    add("g1/conv3x3/x3/t16", conv3x3_case, 16, "x3")
    for mode in ("bf16", "f32"):                                                     # split-K: raw slabs + splitk_reduce_kernel
        add(f"g1/splitk_table_res_silu/{mode}/t16", linear_case, 16, mode, split=2, table=True, res=True, act=1)
        add(f"g1/splitk_rowbias_gelu/{mode}/t16", linear_case, 16, mode, split=2, bias_per_row=True, act=3)
    add(f"g1/splitk_res/bf16/t{GEN1_EVEN}", linear_case, GEN1_EVEN, "bf16", split=2, slabs=8, res=True)

    # register epilogue ----------------------------------------------------------------------------------------------------------------
    for t in PERSISTENT:
        gm = 320 if t in (V2_ODD, V3_ODD) else 256
        # wide f32 plain path: each option alone and together, with and without gn_colsum
        add(f"reg/wide_none/x3/t{t}", linear_case, t, "x3", bias=False)
        add(f"reg/wide_bias/x3/t{t}", linear_case, t, "x3")
        add(f"reg/wide_rowbias/x3/t{t}", linear_case, t, "x3", bias_per_row=True)
        add(f"reg/wide_table/x3/t{t}", linear_case, t, "x3", bias=False, table=True)
        add(f"reg/wide_res/x3/t{t}", linear_case, t, "x3", bias=False, res=True)
        add(f"reg/wide_gn/x3/t{t}", linear_case, t, "x3", bias=False, m=gm, gn=True)
        add(f"reg/wide_bias_table_res_gn/x3/t{t}", linear_case, t, "x3", table=True, res=True, m=gm, gn=True)
        add(f"reg/wide_rowbias_table_res_gn/x3pre/t{t}", linear_case, t, "x3pre", bias_per_row=True, table=True, res=True, m=gm, gn=True)
        add(f"reg/wide_bias_res/f16x2/t{t}", linear_case, t, "f16x2", res=True)
        # the other fast paths
        add(f"reg/presplit_plain_res/x3pre/t{t}", linear_case, t, "x3pre", res=True, split_out=True)
        add(f"reg/rows16_res/bf16/t{t}", linear_case, t, "bf16", res=True)
        add(f"reg/rows16_res/bf16_to_f16/t{t}", linear_case, t, "bf16", res=True, out_dtype=torch.float16)
        add(f"reg/f16rows_plain/f16x2/t{t}", linear_case, t, "f16x2", split_out=True)
        # generic path
        for mode in ("x3", "bf16"):
            add(f"reg/generic_silu_res/{mode}/t{t}", linear_case, t, mode, act=1, res=True)
            add(f"reg/generic_gelu/{mode}/t{t}", linear_case, t, mode, act=3)
        add(f"reg/generic_rows16_table_rowbias_res/bf16/t{t}", linear_case, t, "bf16", bias_per_row=True, table=True, res=True)
        add(f"reg/generic_presplit_silu/x3pre/t{t}", linear_case, t, "x3pre", act=1, split_out=True)
        # split-K: the partial slabs, then the plain reduce and both column-sum reduces
        add(f"reg/splitk_table_res_silu/x3/t{t}", linear_case, t, "x3", split=2, table=True, res=True, act=1)
        add(f"reg/splitk_res/bf16/t{t}", linear_case, t, "bf16", split=2, res=True)
        add(f"reg/splitk_colsum32/x3/t{t}", conv1x1_case, t, "x3", split=2, F=2, H=16, W=8, n=N)
        add(f"reg/splitk_colsum8/x3/t{t}", conv1x1_case, t, "x3", split=2, F=5, H=5, W=8, n=256)
        add(f"reg/splitk_colsum32/f16x2/t{t}", conv1x1_case, t, "f16x2", split=2, F=2, H=16, W=8, n=N)
        # convolutions
        for mode in ("bf16", "x3", "f16x2"):
            add(f"reg/conv3x3/{mode}/t{t}", conv3x3_case, t, mode)
        add(f"reg/conv3x3_splitk/x3/t{t}", conv3x3_case, t, "x3", split=3)
        add(f"reg/temporal/bf16/t{t}", temporal_case, t, "bf16")
        add(f"reg/temporal/x3pre/t{t}", temporal_case, t, "x3pre")
    for t in GEGLU_TILES:
        add(f"reg/wide_geglu/x3/t{t}", linear_case, t, "x3", act=2)
        add(f"reg/wide_geglu_nobias/x3/t{t}", linear_case, t, "x3", act=2, bias=False)
        add(f"reg/presplit_geglu/x3pre/t{t}", linear_case, t, "x3pre", act=2, split_out=True)
        add(f"reg/rows16_geglu/bf16/t{t}", linear_case, t, "bf16", act=2)
        add(f"reg/rows16_geglu/bf16_to_f16/t{t}", linear_case, t, "bf16", act=2, out_dtype=torch.float16)
        add(f"reg/f16rows_geglu/f16x2/t{t}", linear_case, t, "f16x2", act=2, split_out=True)
        add(f"reg/wide_geglu/f16x2/t{t}", linear_case, t, "f16x2", act=2)
    for t in (V2_EVEN, V2_ODD):          # unaligned row pitch: scalar stores (the phased tiles hand such launches to these two)
        for mode in ("x3", "bf16"):
            add(f"reg/generic_pitch193_res/{mode}/t{t}", linear_case, t, mode, res=True, pitch=193)
            add(f"reg/generic_pitch193_table_silu/{mode}/t{t}", linear_case, t, mode, table=True, act=1, pitch=193)
    for mode in ("x3", "bf16"):
        add(f"reg/generic_pitch97_geglu/{mode}/t{V2_EVEN}", linear_case, V2_EVEN, mode, act=2, pitch=97)
    return cases


CASES = build_cases()


def run_case(name, dev):
    """{key: tensor} of one case; the persistent generations add the same keys with `@3wg` from the three-workgroup run."""
    from geo4d_amd import ops
    fn, args, kw, persistent, level = CASES[name]
    old = ops.GN_FUSED_STATS, ops.DEBUG_ABLATE
    try:
        ops.GN_FUSED_STATS = level
        res = {k: v.cpu() for k, v in fn(dev, *args, **kw).items()}
        if persistent:
            ops.DEBUG_ABLATE = 2
            res.update({k + "@3wg": v.cpu() for k, v in fn(dev, *args, **kw).items()})
        torch.cuda.synchronize()
    finally:
        ops.GN_FUSED_STATS, ops.DEBUG_ABLATE = old
    return res


def digest(t):
    t = t.contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def digests(res):
    return {k: digest(v) for k, v in sorted(res.items())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=JSON_PATH)
    ap.add_argument("--dump", default=None, help="directory that receives every case's tensors as <case>.pt")
    ap.add_argument("--only", default=None, help="run only the cases whose name contains this")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    names = [n for n in CASES if not a.only or a.only in n]
    table, failed = {}, []
    for n in names:
        try:
            res = run_case(n, dev)
        except (RuntimeError, AssertionError) as e:      # a refused launch: the case list is wrong, nothing is recorded for it
            failed.append((n, f"{type(e).__name__}: {e}"))
            continue
        table[n] = digests(res)
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            torch.save(res, os.path.join(a.dump, n.replace("/", "__") + ".pt"))
    if not a.only:
        with open(a.out, "w") as f:
            json.dump(table, f, indent=0, sort_keys=True)
            f.write("\n")
    print(f"{len(table)} cases recorded, {len(failed)} failed")
    for n, e in failed:
        print("FAILED", n, e)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
