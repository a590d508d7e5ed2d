#!/usr/bin/env python3
"""Wall time of depth_evaluation (geo4d_amd/evaluation.py) on a Sintel-size sequence (50 x 436 x 1024 = 22.3 M pixels) with the
Sintel / Bonn arguments of scripts/evaluation/infer_geo4d.py:541 (lad2, max_depth 70, post_clip_max 70, lr 1e-2, 5000 Adam
iterations, an align_mask) against a plain-torch restatement of the reference's path (boolean indexing, torch.median,
absolute_value_scaling2 with its per-iteration .item(), the torch metrics and error map: depth_eval.py:112-145, 147-355), on the same
GPU and the same seeded inputs. Also reports the LAD loop alone (geo4d_lad_fit) as bytes/s over the 8 bytes per pixel each Adam
iteration reads. Prints one JSON line.
usage: depth_eval_bench.py [--iters 5000] [--frames 50]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geo4d_amd import _lib, ops  # noqa: E402
from geo4d_amd.evaluation import depth_evaluation  # noqa: E402

KEYS = ("Abs Rel", "Sq Rel", "RMSE", "Log RMSE", "δ < 1.25", "δ < 1.25^2", "δ < 1.25^3")


def torch_reference_path(pred, gt, align_mask, lr, iters):
    mask = (gt > 0) & (gt < 70)
    p, g = pred[mask], gt[mask]
    am = align_mask[mask]
    pa, ga = p[am], g[am]
    s0 = (torch.median(ga) / torch.median(pa)).item()
    s = torch.tensor([s0], requires_grad=True, device=pred.device)
    t = torch.tensor([0.0], requires_grad=True, device=pred.device)
    opt = torch.optim.Adam([s, t], lr=lr)
    prev = None
    for _ in range(iters):
        opt.zero_grad()
        loss = torch.sum(torch.abs(s * pa + t - ga))
        loss.backward()
        opt.step()
        if prev is not None and torch.abs(prev - loss) < 1e-6:
            break
        prev = loss.item()
    s, t = s.detach().item(), t.detach().item()
    a = torch.clamp(s * p + t, max=70)
    res = [torch.mean(torch.abs(a - g) / g).item(), torch.mean((a - g) ** 2 / g).item(), torch.sqrt(torch.mean((a - g) ** 2)).item()]
    a = torch.clamp(a, min=1e-5)
    res.append(torch.sqrt(torch.mean((torch.log(a) - torch.log(g)) ** 2)).item())
    r = torch.maximum(a / g, g / a)
    res += [torch.mean((r < 1.25 ** k).float()).item() for k in (1, 2, 3)]
    err = torch.where(mask, torch.abs(pred * s + t - gt) / gt, torch.zeros_like(gt))
    torch.cuda.synchronize()
    return dict(zip(KEYS, res)), s, t, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--frames", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T, H, W = args.frames, 436, 1024
    g = torch.Generator(device=dev).manual_seed(0)
    gt = 0.5 + 79.5 * torch.rand((T, H, W), generator=g, device=dev) ** 2
    gt[torch.rand((T, H, W), generator=g, device=dev) < 0.05] = 0
    pred = ((gt.clamp(min=0.5) - 0.4) / 2.7 + 0.2 * torch.randn((T, H, W), generator=g, device=dev)).abs() + 1e-3
    am = torch.rand((T, H, W), generator=g, device=dev) < 0.85
    pred, gt, am = pred.reshape(-1), gt.reshape(-1), am.reshape(-1)
    kw = dict(max_depth=70, align_with_lad2=True, post_clip_max=70, lr=1e-2, max_iters=args.iters, align_mask=am, return_st=True)

    depth_evaluation(pred, gt, **dict(kw, max_iters=10))                     # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res, err, _, _ = depth_evaluation(pred, gt, **kw)
    torch.cuda.synchronize()
    hip_ms = (time.perf_counter() - t0) * 1e3

    # the LAD loop alone, on the compacted fit vector
    lib = _lib.load()
    pv, gv, cnt = ops.masked_select(pred, gt, max_depth=70, mask=am)
    n = int(cnt.item())
    st = torch.empty(2, device=dev)
    info = torch.empty(2, device=dev)
    need = lib.geo4d_lad_workspace(1, n)
    ws = torch.empty((need + 7) // 8, device=dev, dtype=torch.float64)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(lib.geo4d_lad_fit(pv.data_ptr(), gv.data_ptr(), 1, n, None, 1e-2, args.iters, 1e-6, st.data_ptr(), info.data_ptr(), ws.data_ptr(),
                                 need, ops._stream()), "geo4d_lad_fit")
    e1.record()
    torch.cuda.synchronize()
    lad_ms = e0.elapsed_time(e1)
    steps = int(info[0].item())

    torch_reference_path(pred, gt, am, 1e-2, 10)                              # warm-up
    t0 = time.perf_counter()
    tres, ts, tt, terr = torch_reference_path(pred, gt, am, 1e-2, args.iters)
    torch_ms = (time.perf_counter() - t0) * 1e3

    out = dict(tool="depth_eval_bench", frames=T, H=H, W=W, pixels=T * H * W, fit_pixels=n, iters=args.iters, lad_steps=steps,
               hip_ms=round(hip_ms, 2), torch_ms=round(torch_ms, 2), speedup=round(torch_ms / hip_ms, 2),
               lad_ms=round(lad_ms, 2), lad_GBps=round(8.0 * n * (steps + 1) / (lad_ms * 1e-3) / 1e9, 1),
               s=res["s"], t=res["t"], torch_s=ts, torch_t=tt,
               abs_rel=res["Abs Rel"], torch_abs_rel=tres["Abs Rel"], delta1=res["δ < 1.25"], torch_delta1=tres["δ < 1.25"],
               err_map_max_diff=float((err - terr).abs().max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
