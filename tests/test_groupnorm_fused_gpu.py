"""GroupNorm from producer column sums without a statistics round trip (norm.hip gn_apply_sums_kernel / gn_slice_sums_kernel, reached
through ops.groupnorm -> geo4d_groupnorm2). The sum buffers are built by hand from the input, so no GEMM runs here.

Every case is compared with torch.nn.functional.group_norm in float64 on the same input, at the bound tests/test_kernels_gpu.py applies to
GroupNorm for the same OUTPUT format (relative L2 <= 2 x TOL: 4e-5 for f32 rows - the pre-split bf16 hi | lo image decodes to f32 values -,
1.2e-2 for bf16, 2e-3 for f16 rows), and with the two-launch sequence (gn_finalize_cols + gn_apply: ops.GN_ONE_LAUNCH = 0) at that bound.
Checked on every case: the library's own choice (fused where the plan fuses), FUSED forced, SLICED forced; two identical calls are
torch.equal. Further: two sum sources with unequal channel halves and unequal rows per entry; a stale tag falls back to the statistics
pass; the f16 saturation counter counts as the unfused path does."""
import math

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 6e-3, torch.float16: 1e-3}      # tests/test_kernels_gpu.py; GroupNorm is checked at scale 2.0 there
SCALE = 2.0


def rnd(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def check(name, got, ref, out_dtype):
    e = rel(got, ref)
    print(f"[{name}] rel_l2={e:.3e} tol={TOL[out_dtype] * SCALE:.1e}")
    assert math.isfinite(e) and e <= TOL[out_dtype] * SCALE, f"{name}: rel_l2 {e:.3e} > {TOL[out_dtype] * SCALE:.1e}"


def attach_sums(t, rows, garbage=False):
    """What conv_gemm(gn_stats=True) leaves on its output: [M / rows][C][2] fp32 (sum, sum of squares) per row block, and the staleness tag."""
    M, C = t.shape
    v = t.double().reshape(M // rows, rows, C)
    cs = torch.stack([v.sum(1), (v * v).sum(1)], -1).float().contiguous()
    t._gn_colsum = torch.full_like(cs, 1.0e4) if garbage else cs
    t._gn_colsum_rows = rows
    t._gn_colsum_tag = (t.data_ptr(), t._version)
    return t


def decode(out, C):
    """plain rows, f16 rows or the pre-split bf16 hi | lo image -> f32 values."""
    from geo4d_amd import ops
    if isinstance(out, ops.SplitAct):
        v = out.as_subclass(torch.Tensor).reshape(out.shape[0], C // 8, 2, 8).float()
        return (v[:, :, 0] + v[:, :, 1]).reshape(out.shape[0], C)
    return out.float()


def reference(x, g, b, F, HW, fps, eps, silu):
    C = x.shape[1]
    x5 = x.double().reshape(F // fps, fps * HW, C).permute(0, 2, 1)
    r = TF.group_norm(x5, 32, g.double(), b.double(), eps)
    if silu:
        r = TF.silu(r)
    return r.permute(0, 2, 1).reshape(F * HW, C)


# (F, HW, C, frames_per_stat, rows per sum entry, SiLU, split_out, input dtype, column views)
CASES = [
    (2, 40, 64, 1, 8, True, 0, torch.float32, False),
    (2, 40, 64, 2, 8, False, 2, torch.float32, False),
    (16, 64, 320, 1, 64, True, 1, torch.float32, False),         # per-frame, a single block per statistic
    (16, 64, 64, 16, 8, True, 0, torch.float32, False),
    (16, 64, 1280, 16, 32, True, 2, torch.float32, False),
    (2, 64, 1280, 2, 64, False, 1, torch.float32, False),
    (16, 160, 1280, 1, 32, True, 2, torch.float32, False),       # the plan raises R (56 rows: chunks of 56, 56, 48 - a ragged last chunk) and cuts 16 channel slices
    (16, 160, 1280, 1, 8, True, 1, torch.float32, False),
    (16, 160, 1280, 16, 80, True, 1, torch.float32, False),
    (16, 160, 320, 1, 32, False, 0, torch.float32, False),
    (2, 160, 320, 2, 80, True, 2, torch.float32, False),
    (16, 40, 1280, 16, 64, True, 2, torch.float32, False),
    (16, 40, 320, 1, 8, True, 0, torch.float32, True),           # ldx, ldy > C
    (16, 160, 320, 16, 32, True, 2, torch.float32, True),
    (16, 160, 320, 1, 80, True, 0, torch.bfloat16, False),
    (2, 64, 320, 2, 32, True, 0, torch.float16, False),
]
IDS = [f"F{c[0]}-HW{c[1]}-C{c[2]}-fps{c[3]}-rows{c[4]}-silu{int(c[5])}-split{c[6]}-{str(c[7]).split('.')[-1]}{'-view' if c[8] else ''}" for c in CASES]


def make_case(dev, case):
    F, HW, C, fps, rows, silu, split, dtype, view = case
    M = F * HW
    if view:
        x = (rnd((M, C + 64), dev, 11) * 2 + 0.7).to(dtype)[:, 32:32 + C]
    else:
        x = (rnd((M, C), dev, 11) * 2 + 0.7).to(dtype)
    g, b = rnd((C,), dev, 12) + 1.0, rnd((C,), dev, 13)
    return attach_sums(x, rows), g, b


def run(x, g, b, case, path=None):
    from geo4d_amd import ops
    F, HW, C, fps, rows, silu, split, dtype, view = case
    out = None
    if view:
        odt = torch.float16 if split == 2 else dtype
        out = torch.zeros((F * HW, C + 64), device=x.device, dtype=odt)[:, 32:32 + C]
    so = {0: False, 1: True, 2: "f16"}[split]
    return ops.groupnorm(x, g, b, F=F, HW=HW, eps=1e-5, frames_per_stat=fps, silu=silu, out=out, split_out=None if view else so, path=path)


def planned(x, g, b, case):
    """the library's plan for this call (the same host function the launch runs)"""
    from geo4d_amd import ops
    F, HW, C, fps, rows, silu, split, dtype, view = case
    q = ops._gn_descriptor(x, x, g, b, F=F, HW=HW, eps=1e-5, groups=32, frames_per_stat=fps, silu=silu, split_out=0,
                           sources=ops._gn_sources(x, fps * HW), path=0)
    q.base.split_out = split            # (the plan reads the output format for its bytes per row; no output exists here)
    return ops.groupnorm_plan(q)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_groupnorm_from_sums_every_path(dev, case):
    from geo4d_amd import _lib, ops
    F, HW, C, fps, rows, silu, split, dtype, view = case
    x, g, b = make_case(dev, case)
    out_dtype = torch.float16 if split == 2 else dtype
    ref = reference(x, g, b, F, HW, fps, 1e-5, silu)
    old = ops.GN_ONE_LAUNCH
    try:
        ops.GN_ONE_LAUNCH = 0
        two = decode(run(x, g, b, case), C)                       # gn_finalize_cols + gn_apply
    finally:
        ops.GN_ONE_LAUNCH = old
    check("two-launch vs float64", two, ref, out_dtype)
    for name, path in (("plan", None), ("fused", _lib.GN_PATH_FUSED), ("sliced", _lib.GN_PATH_SLICED)):
        y = run(x, g, b, case, path)
        y2 = run(x, g, b, case, path)
        assert torch.equal(y.as_subclass(torch.Tensor), y2.as_subclass(torch.Tensor)), f"{name}: two identical calls differ"
        got = decode(y, C)
        check(f"{name} vs float64", got, ref, out_dtype)
        check(f"{name} vs two-launch", got, two, out_dtype)


def test_the_cases_reach_every_branch_of_the_plan(dev):
    """Over CASES the library's own choice fuses and slices, cuts channels into slices, raises R above the default chunk and leaves a
    ragged last chunk (so the parametrised test above has run those branches)."""
    from geo4d_amd import _lib
    seen = []
    for case in CASES:
        x, g, b = make_case(dev, case)
        pl = planned(x, g, b, case)
        F, HW = case[0], case[1]
        r0 = max(4, (((HW * F + 1023) // 1024) + 3) // 4 * 4)
        seen.append((pl.path, pl.channel_slices, pl.rows_per_wg > r0, pl.path == _lib.GN_PATH_FUSED and HW % pl.rows_per_wg != 0 and pl.nchunk > 1, pl.stat_slices))
    print(seen)
    assert any(s[0] == _lib.GN_PATH_FUSED for s in seen) and any(s[0] == _lib.GN_PATH_SLICED for s in seen)
    assert any(s[0] == _lib.GN_PATH_FUSED and s[1] > 1 for s in seen), "no case with channel slices"
    assert any(s[0] == _lib.GN_PATH_FUSED and s[2] for s in seen), "no case with R raised by the host"
    assert any(s[3] for s in seen), "no case with a ragged last chunk"
    assert any(s[4] > 1 for s in seen), "no case with more than one statistics slice"


@pytest.mark.parametrize("fps", [1, 2])
@pytest.mark.parametrize("split", [0, 2])
def test_two_sum_sources_unequal_halves_and_rows(dev, fps, split):
    """A channel concatenation 320 | 640 (30 channels per group: group 10 straddles the two halves), the left producer's sums per 8 rows, the
    right one's per 32: statistics from both == the statistics pass over the buffer == float64."""
    from geo4d_amd import _lib, ops
    F, HW, Cl, Cr = 2, 64, 320, 640
    C = Cl + Cr
    buf = rnd((F * HW, C), dev, 21) * 2 + 0.7
    buf[:, Cl:] = buf[:, Cl:] * 3 - 1.0                      # the halves have different statistics
    left, right = attach_sums(buf[:, :Cl], 8), attach_sums(buf[:, Cl:], 32)
    ops.concat_parts(buf, left, right)
    g, b = rnd((C,), dev, 22) + 1.0, rnd((C,), dev, 23)
    so = {0: False, 2: "f16"}[split]
    kw = dict(F=F, HW=HW, eps=1e-5, frames_per_stat=fps, silu=True, split_out=so)
    src = ops._gn_sources(buf, fps * HW)
    assert [(s[1], s[2], s[3]) for s in src] == [(8, 0, Cl), (32, Cl, Cr)]
    out_dtype = torch.float16 if split == 2 else torch.float32
    ref = reference(buf, g, b, F, HW, fps, 1e-5, True)
    three = ops.groupnorm(buf.clone(), g, b, **kw).float()   # the clone carries no parts: gn_partial + gn_finalize + gn_apply
    check("three-pass vs float64", three, ref, out_dtype)
    for name, path in (("plan", None), ("fused", _lib.GN_PATH_FUSED), ("sliced", _lib.GN_PATH_SLICED)):
        y = ops.groupnorm(buf, g, b, path=path, **kw)
        assert torch.equal(y, ops.groupnorm(buf, g, b, path=path, **kw))
        check(f"two sources {name} vs float64", y.float(), ref, out_dtype)
        check(f"two sources {name} vs three-pass", y.float(), three, out_dtype)
    # the switch off: a concatenated input runs its own statistics pass, as before
    old = ops.GN_ONE_LAUNCH
    try:
        ops.GN_ONE_LAUNCH = 0
        assert ops._gn_sources(buf, fps * HW) == []
        assert torch.equal(ops.groupnorm(buf, g, b, **kw).float(), three)
    finally:
        ops.GN_ONE_LAUNCH = old
    # one half without sums (or with stale ones): the statistics pass again
    right._gn_colsum = torch.full_like(right._gn_colsum, 1.0e4)
    right._gn_colsum_tag = (right.data_ptr(), right._version - 1)
    assert ops._gn_sources(buf, fps * HW) == []
    assert torch.equal(ops.groupnorm(buf, g, b, **kw).float(), three)


def test_stale_sums_fall_back_to_the_statistics_pass(dev):
    """Sums whose tag no longer matches the tensor (it was modified in place after the GEMM wrote it) are ignored: the sums planted here
    are wrong on purpose, so using them would miss the reference by far."""
    from geo4d_amd import ops
    F, HW, C = 16, 40, 320
    x = attach_sums(rnd((F * HW, C), dev, 31) * 2 + 0.7, 8, garbage=True)
    g, b = rnd((C,), dev, 32) + 1.0, rnd((C,), dev, 33)
    ref = reference(x, g, b, F, HW, 1, 1e-5, True)
    wrong = ops.groupnorm(x, g, b, F=F, HW=HW, eps=1e-5, silu=True)
    assert rel(wrong, ref) > 0.1, "fresh sums are used (and these are wrong)"
    x.add_(0.0)                                              # bumps the version: the tag is stale
    assert ops._gn_sources(x, HW) == []
    y = ops.groupnorm(x, g, b, F=F, HW=HW, eps=1e-5, silu=True)
    check("stale tag", y, ref, torch.float32)
    assert torch.equal(y, ops.groupnorm(x.clone(), g, b, F=F, HW=HW, eps=1e-5, silu=True))


def test_f16_saturation_counter_counts_as_the_unfused_path(dev):
    from geo4d_amd import _lib, ops
    F, HW, C = 2, 64, 64
    x = attach_sums(rnd((F * HW, C), dev, 41), 8)
    x_plain = x.clone()
    gamma, beta = torch.full((C,), 3.0e4, device=dev), torch.zeros((C,), device=dev)
    kw = dict(F=F, HW=HW, eps=1e-5, split_out="f16")
    counts = {}
    old = ops.SAT_COUNTER
    try:
        for name, (t, path) in {"three-pass": (x_plain, None), "two-launch": (x, _lib.GN_PATH_COLS), "fused": (x, _lib.GN_PATH_FUSED),
                                "sliced": (x, _lib.GN_PATH_SLICED), "plan": (x, None)}.items():
            cnt = torch.zeros(1, device=dev, dtype=torch.int64)
            ops.SAT_COUNTER = cnt
            y = ops.groupnorm(t, gamma, beta, path=path, **kw)
            counts[name] = int(cnt.item())
            assert float(y.float().abs().max()) == 65504.0
        ops.SAT_COUNTER = None
        cnt = torch.zeros(1, device=dev, dtype=torch.int64)
        ops.groupnorm(x, gamma, beta, path=_lib.GN_PATH_FUSED, **kw)
        assert int(cnt.item()) == 0, "no counter, no counting"
    finally:
        ops.SAT_COUNTER = old
    print(counts)
    assert counts["two-launch"] > 0 and len(set(counts.values())) == 1, counts
