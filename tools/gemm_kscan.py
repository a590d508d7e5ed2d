#!/usr/bin/env python3
"""Per-tile fixed cost vs per-slab slope of conv_gemm on plain linears: one (M, N) at several K, for given (tile, split) hints and epilogues
(bf16x3, pre-split operands, what the U-Net runs). t(K) = fixed + slope * K/32: `fixed` is prologue + epilogue + launch, `slope` the K loop.
usage (GPU box): python tools/gemm_kscan.py [--dtype bf16x3]
--dtype f16x2: the launches of the bf16x3m mode that write plain f16 rows (two-pass f16, o_split = 2) - the GEGLU ff1, q | k, q | k | v and
cross-attention q projections of levels 0 / 1 / 2, each on the tuning table's tile for K = C, at K = C, 2 C, 4 C, 8 C; fixed part and slope
by least squares over the four (profiles/epilogue_wide.md)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geo4d_amd import ops, pack  # noqa: E402
from tools.gemm_bench import plan_takes  # noqa: E402


def time_launches(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def table_config(x, wp, bias, act):
    """(tile_hint, split_k) the tuning table gives the f16-row linear of these operands (nothing is launched; ops.AUTOTUNE is off in
    this mode, so a shape without an entry answers (0, 0) instead of being measured)."""
    M, K, N = x.shape[0], x.shape[1], wp.shape[0]
    out = torch.empty((M, N // 2 if act == 2 else N), device=x.device, dtype=torch.float16)
    p = ops.conv_gemm_descriptor(x, wp, out, M=M, N=N, K=K, Cin=K, lda=x.stride(0), ldw=wp.stride(0), ldo=out.stride(0), bias=bias, act=act)
    return ops._launch_config(p, None)


def scan_f16_rows(iters):
    ops.AUTOTUNE = False
    dev = torch.device("cuda:0")
    for level, (M, C) in enumerate(((40960, 320), (10240, 640), (2560, 1280))):
        for label, N, act in (("geglu", 8 * C, 2), ("q|k", 2 * C, 0), ("q|k|v", 3 * C, 0), ("cross q", C, 0)):
            ks, row, cfg = [C, 2 * C, 4 * C, 8 * C], [], None
            for K in ks:
                x = torch.randn((M, K), device=dev).to(torch.float16)
                w, b = torch.randn((N, K), device=dev) / K ** 0.5, torch.randn((N,), device=dev)
                wp, bp = pack.pack_geglu_x2(w, b, "bf16x3m") if act == 2 else (pack.split_f16(w), b)
                del w
                if cfg is None:
                    cfg = table_config(x, wp, bp, act)
                    if cfg[0] == 0:
                        break
                row.append(time_launches(lambda: ops.linear(x, wp, bp, act=act, split_out="f16", tile_hint=cfg[0], split_k=max(cfg[1], 1)), iters))
                del x, wp
            if len(row) < len(ks):
                print(f"L{level} {label:8s} M={M:6d} N={N:5d}: no table entry", flush=True)
                continue
            slabs = [k / 32 for k in ks]
            ms, mt = sum(slabs) / 4, sum(row) / 4
            slope = sum((s - ms) * (t - mt) for s, t in zip(slabs, row)) / sum((s - ms) ** 2 for s in slabs)
            print(f"L{level} {label:8s} M={M:6d} N={N:5d} t{cfg[0]}: " + "  ".join(f"K{k}={v:7.1f}" for k, v in zip(ks, row)) +
                  f"  us | slope {slope:6.3f} us/slab | fixed {mt - slope * ms:6.1f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16x3", help="bf16x3 | bf16 | f16x2 (the bf16x3m mode's launches that write f16 rows)")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.dtype == "f16x2":
        return scan_f16_rows(a.iters)
    x3 = a.dtype == "bf16x3"
    dev = torch.device("cuda:0")
    dt = torch.float32 if x3 else torch.bfloat16
    cases = [  # (label, M, N, [(tile, split) ...], [act ...])
        ("L0 geglu-like", 40960, 2560, [(71, 1), (13, 1), (22, 1), (74, 1)], [0, 2]),
        ("L0 qkv-like", 40960, 960, [(2, 1), (71, 1), (72, 1), (25, 1)], [0]),
        ("L0 proj-like", 40960, 320, [(16, 1), (72, 1), (23, 1)], [0]),
        ("L1 proj-like", 10240, 640, [(4, 1), (1, 1), (17, 1), (25, 1), (74, 1)], [0]),
        ("L2 proj-like", 2560, 1280, [(4, 1), (1, 1), (3, 1), (25, 2), (28, 1)], [0]),
    ]
    for label, M, N, cfgs, acts in cases:
        for act in acts:
            for tile, split in cfgs:
                row = []
                for K in (320, 640, 1280, 2560):
                    x = torch.randn((M, K), device=dev).to(dt)
                    w = torch.randn((N, K), device=dev) / K ** 0.5
                    b = torch.randn((N,), device=dev)
                    if x3:
                        xa, wp = ops.SplitAct.wrap(pack.split_bf16(x)), pack.split_bf16(w)
                    else:
                        xa, wp = x, w.to(dt)
                    so = bool(x3 and act == 2)
                    fn = lambda: ops.linear(xa, wp, b, act=act, tile_hint=tile, split_k=split, split_out=so)
                    if not plan_takes(fn):
                        row.append(None)
                        continue
                    for _ in range(3):
                        fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    row.append(e0.elapsed_time(e1) * 1e3 / a.iters)
                if any(v is None for v in row):
                    print(f"{label:14s} M={M:6d} N={N:5d} act={act} t{tile}/s{split}: n/a")
                    continue
                slope = (row[3] - row[1]) / ((2560 - 640) / 32)            # us per 32-k slab
                fixed = row[1] - slope * 640 / 32
                pf = 3 * 2.0 * M * N * 32 / slope / 1e9 if x3 else 2.0 * M * N * 32 / slope / 1e9      # MFMA-issued PF/s... (TF/s / 1000)
                print(f"{label:14s} M={M:6d} N={N:5d} act={act} t{tile}/s{split}: " + "  ".join(f"K{k}={v:7.1f}" for k, v in zip((320, 640, 1280, 2560), row)) +
                      f"  us | slope {slope:6.2f} us/slab = {pf:6.0f} TF/s issued in the loop | fixed {fixed:6.1f} us", flush=True)


if __name__ == "__main__":
    main()
