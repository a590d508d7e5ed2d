#!/usr/bin/env python3
"""Stochastic DDIM (eta = 1, the entry scripts' default and the "better visual results" setting of scripts/infer_geo4d.sh:29-32) at the bench.py
default size (one 16 x 320 x 512 window, bf16x3m, random weights): ms per DDIM step of
  (a) eta 1, torch.randn step noise: eager steps (the behaviour without noise_seeds),
  (b) eta 1, noise_seeds: counter-based noise made in the update kernel, the step captured into a hipGraph,
  (c) eta 0, captured (orientation: (b) should land at (c) + the noise arithmetic),
without guidance and with 2-way CFG 7.5, plus (b) and (c) at two windows per batch, unguided and guided, as denoised latent frames/s.
One process, one GPU; two passes over the variants, each variant warmed up by one full call and then timed `repeats` times with HIP events
around a call of S steps; the table quotes the median of a variant's calls and their spread. Same-process pairs only (box-to-box spread: README).
usage (GPU box): python tools/eta_bench.py [steps] [repeats] [--out table.md]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    argv = [a for a in sys.argv[1:]]
    out_path = argv.pop(argv.index("--out") + 1) if "--out" in argv else None
    argv = [a for a in argv if a != "--out"]
    S = int(argv[0]) if len(argv) > 0 else 10
    R = int(argv[1]) if len(argv) > 1 else 3
    dev = torch.device("cuda:0")
    model, _ = bench.build("bf16x3m", dev)
    from geo4d_amd.ddim import DDIMSampler
    T, h, w = 16, 40, 64
    g = torch.Generator().manual_seed(5)

    def inputs(B):
        mk = lambda: {"c_crossattn": [torch.randn((B, 77 + 16 * T, 1024), generator=g).to(dev)], "c_concat": [zc]}
        zc = torch.randn((B, 4, T, h, w), generator=g).to(dev)
        return dict(cond=mk(), uc=mk(), x_T=torch.randn((B, 16, T, h, w), generator=g).to(dev), fs=torch.full((B,), 24, dtype=torch.long, device=dev))
    data = {1: inputs(1), 2: inputs(2)}

    def variant(eta, seeded, cfg, B=1):
        s = DDIMSampler(model)        # one sampler per variant: each keeps its own captured step
        d = data[B]
        kw = dict(S=S, conditioning=d["cond"], batch_size=B, shape=[16, T, h, w], verbose=False, eta=eta, fs=d["fs"], x_T=d["x_T"],
                  timestep_spacing="uniform_trailing", guidance_rescale=0.7)
        if cfg:
            kw.update(unconditional_guidance_scale=7.5, unconditional_conditioning=d["uc"])
        if seeded:
            kw["noise_seeds"] = [123 * 1000003 + i for i in range(B)]
        return lambda: s.sample(**kw)[0]

    rows = []
    for cfg in (False, True):
        tag = "2-way CFG 7.5" if cfg else "CFG 1"
        rows += [(f"(a) eta 1, torch.randn noise, eager [{tag}]", variant(1.0, False, cfg), 1),
                 (f"(b) eta 1, noise_seeds, captured [{tag}]", variant(1.0, True, cfg), 1),
                 (f"(c) eta 0, captured [{tag}]", variant(0.0, False, cfg), 1)]
    rows += [("(b) eta 1, noise_seeds, captured, 2 windows per batch [CFG 1]", variant(1.0, True, False, 2), 2),
             ("(c) eta 0, captured, 2 windows per batch [CFG 1]", variant(0.0, False, False, 2), 2)]
    # guided clips batch windows too (run_clip hands every conditioning dict one row per window): the step is then ONE forward of 2 x 2 rows.
    # Compare with the one-window guided rows (b) / (c) above - the same process, the same guidance
    rows += [("(b) eta 1, noise_seeds, captured, 2 windows per batch [2-way CFG 7.5]", variant(1.0, True, True, 2), 2),
             ("(c) eta 0, captured, 2 windows per batch [2-way CFG 7.5]", variant(0.0, False, True, 2), 2)]
    # A variant's calls run back to back after a warm-up call of its own (which packs weights, fills the context K/V cache and captures
    # the step): the eager guided variant allocates new K/V buffers per call, and an eviction from the U-Net's K/V cache makes every
    # sampler capture again, which must not land in another variant's timed call. Two passes over the list expose drift.
    times = {name: [] for name, _, _ in rows}
    for _ in range(2):
        for name, run, _ in rows:
            run()
            torch.cuda.synchronize()
            for _ in range(R):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / S)
    lines = [f"| variant ({S} steps per call, median of {2 * R} calls, HIP events) | ms per DDIM step | min .. max | denoised latent frames/s |", "|---|---|---|---|"]
    for name, _, B in rows:
        t = times[name]
        med = statistics.median(t)
        lines.append(f"| {name} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | {1e3 * T * B / med / S:.2f} |")
    table = "\n".join(lines)
    print(table, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
