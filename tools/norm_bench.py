#!/usr/bin/env python3
"""GroupNorm / LayerNorm op timing at the shapes of the Geo4D hot path (HIP events on the launch stream).
GB/s counts the algorithmic traffic: GroupNorm = 2 reads + 1 write of the tensor, LayerNorm = 1 read + 1 write.
Back-to-back eager calls: below ~30 us per op the number is the Python call overhead, not the GPU.
usage (GPU box): python tools/norm_bench.py [--dtype bf16]

--sweep: the launch sequences of a GroupNorm that has producer column sums (ops.groupnorm path / fuse fraction / workgroup floor), each
timed as 20 GroupNorms captured in one hipGraph and replayed (us per GroupNorm: kernels + boundaries, no Python): the two-launch
sequence three times (its own spread), the sliced form, and the fused form per (fraction, floor). Shapes: the U-Net's and the VAE
decoder's (F, HW, C, frames_per_stat, rows per sum entry of each source), or --shapes FILE (a JSON list of such tuples, e.g. recorded from a forward).
usage: python tools/norm_bench.py --sweep [--shapes FILE] [--fractions 0.125,0.25,0.5,1] [--floors 256,1024]"""
import argparse, json, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geo4d_amd import ops

GN = [("unet L0 320ch", 16, 2560, 320), ("unet L0 640ch (skip concat)", 16, 2560, 640), ("unet L1 640ch", 16, 640, 640),
      ("unet L2 1280ch", 16, 160, 1280), ("unet L3 1280ch", 16, 40, 1280),
      ("vae 512ch @40x64", 16, 2560, 512), ("vae 512ch @80x128", 16, 10240, 512), ("vae 256ch @160x256", 16, 40960, 256),
      ("vae 128ch @320x512", 16, 163840, 128)]
LN = [("L0", 40960, 320), ("L1", 10240, 640), ("L2", 2560, 1280)]


def timeit(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


# (F, HW, C, frames_per_stat, [(rows per entry, channels) per sum source], output format): f32 storage, as the headline mode runs them
SWEEP = [(16, HW, C, fps, [(rows, C)], "f16") for HW, C in ((2560, 320), (640, 640), (160, 1280), (40, 1280)) for fps in (1, 16)
         for rows in (8, 32, 64, 128) if (fps * HW) % rows == 0 and (rows != 8 or HW == 40)] + \
        [(16, 2560, 960, 1, [(64, 640), (64, 320)], "f16"), (16, 640, 1920, 1, [(64, 1280), (32, 640)], "f16"),
         (16, 160, 2560, 1, [(32, 1280), (32, 1280)], "f16"), (16, 40, 2560, 1, [(8, 1280), (8, 1280)], "f16")] + \
        [(16, HW, C, 1, [(rows, C)], "f16") for HW, C in ((2560, 512), (10240, 512), (40960, 256), (163840, 128)) for rows in (64, 128)]


def graph_us(fn, per_graph=20, replays=10):
    """us per call of `fn`, `per_graph` calls captured in one hipGraph (no Python between the kernels), `replays` timed replays."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    for _ in range(3):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * per_graph)


def sweep(a):
    from geo4d_amd import _lib
    dev = torch.device("cuda:0")
    shapes = json.load(open(a.shapes)) if a.shapes else SWEEP
    fracs = [float(v) for v in a.fractions.split(",")]
    floors = [int(v) for v in a.floors.split(",")]
    names = {1: "partial", 2: "cols", 3: "fused", 4: "sliced"}
    cols = [f"f{fr:g}/w{fl}" for fr in fracs for fl in floors]
    print(f"{'F x HW x C fps rows':44s} {'parent x3 (us)':>22s} {'sliced':>8s} " + " ".join(f"{c:>22s}" for c in cols) + "   default")
    rows_out = []
    for F, HW, C, fps, srcs, fmt in shapes:
        M = F * HW
        x = torch.randn((M, C), device=dev) * 2 + 0.5
        g, b = torch.randn(C, device=dev), torch.randn(C, device=dev)
        out = ops.new_split(M, C, dev, fmt) if fmt else torch.empty_like(x)
        views, c0 = [], 0
        for rows, nc in srcs:
            v = x[:, c0:c0 + nc] if len(srcs) > 1 else x
            t = v.double().reshape(M // rows, rows, nc)
            v._gn_colsum = torch.stack([t.sum(1), (t * t).sum(1)], -1).float().contiguous()
            v._gn_colsum_rows, v._gn_colsum_tag = rows, (v.data_ptr(), v._version)
            views.append(v)
            c0 += nc
        if len(srcs) > 1:
            ops.concat_parts(x, *views)
        kw = dict(F=F, HW=HW, eps=1e-5, frames_per_stat=fps, silu=True, out=out)

        def plan_of(path):
            q = ops._gn_descriptor(x, out, g, b, F=F, HW=HW, eps=1e-5, groups=32, frames_per_stat=fps, silu=True,
                                   split_out={None: 0, "bf16": 1, "f16": 2}[fmt], sources=ops._gn_sources(x, fps * HW), path=path)
            return ops.groupnorm_plan(q)
        old = ops.GN_ONE_LAUNCH
        ops.GN_ONE_LAUNCH = 0           # the parent's sequence: gn_finalize_cols + gn_apply, or the three passes for a concatenated input
        parent = [graph_us(lambda: ops.groupnorm(x, g, b, **kw)) for _ in range(3)]
        ref = out.clone()
        ops.GN_ONE_LAUNCH = old
        sl = graph_us(lambda: ops.groupnorm(x, g, b, path=_lib.GN_PATH_SLICED, **kw))
        err = ((out.float() - ref.float()).norm() / ref.float().norm()).item()
        cells = []
        for fr in fracs:
            for fl in floors:
                ops.GN_TUNE = (fr, fl)
                pl = plan_of(0)
                if pl.path != _lib.GN_PATH_FUSED:
                    cells.append(f"{'-> ' + names[pl.path]:>22s}")
                    continue
                us = graph_us(lambda: ops.groupnorm(x, g, b, **kw))
                err = max(err, ((out.float() - ref.float()).norm() / ref.float().norm()).item())
                cells.append(f"{us:7.1f} R{pl.rows_per_wg}x{pl.nchunk}c{pl.channel_slices}".rjust(22))
        ops.GN_TUNE = (0.0, 0)
        pl = plan_of(0)
        dflt = graph_us(lambda: ops.groupnorm(x, g, b, **kw))
        name = f"{F} x {HW} x {C} fps{fps} rows{'+'.join(str(r) for r, _ in srcs)}"
        print(f"{name:44s} {' '.join(f'{p:6.1f}' for p in parent):>22s} {sl:8.1f} " + " ".join(cells) + f"   {names[pl.path]} {dflt:.1f}  (max rel diff {err:.1e})")
        rows_out.append({"shape": [F, HW, C, fps, srcs], "parent_us": parent, "sliced_us": sl, "default": names[pl.path], "default_us": dflt})
        del x, out, views
    if a.json:
        json.dump(rows_out, open(a.json, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--fractions", default="0.125,0.25,0.5,1")
    ap.add_argument("--floors", default="256,1024")
    ap.add_argument("--json", default=None, help="--sweep: also write the rows to this file")
    a = ap.parse_args()
    if a.sweep:
        return sweep(a)
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    dev = torch.device("cuda:0")
    print(f"{'groupnorm':34s} {'fps':>4s} {'MB':>8s} {'us':>9s} {'TB/s':>8s}")
    for name, F, HW, C in GN:
        x = torch.randn((F * HW, C), device=dev).to(dt)
        g, b = torch.randn(C, device=dev), torch.randn(C, device=dev)
        out = torch.empty_like(x)
        for fps in ((1, 16) if name.startswith("unet") else (1,)):
            us = timeit(lambda: ops.groupnorm(x, g, b, F=F, HW=HW, eps=1e-5, frames_per_stat=fps, silu=True, out=out), a.iters)
            mb = x.numel() * x.element_size() / 1e6
            print(f"{name:34s} {fps:4d} {mb:8.1f} {us:9.1f} {3 * mb / us:8.2f}")
    print(f"{'layernorm':34s} {'':>4s} {'MB':>8s} {'us':>9s} {'TB/s':>8s}")
    for name, M, C in LN:
        x = torch.randn((M, C), device=dev).to(dt)
        g, b = torch.randn(C, device=dev), torch.randn(C, device=dev)
        out = torch.empty_like(x)
        us = timeit(lambda: ops.layernorm(x, g, b, out=out), a.iters)
        mb = x.numel() * x.element_size() / 1e6
        print(f"{name:34s} {'':4s} {mb:8.1f} {us:9.1f} {2 * mb / us:8.2f}")


if __name__ == "__main__":
    main()
