"""GPU tests of the conv_gemm front-end in ops.py against the plan query (csrc/gemm_plan.h): ops.conv_gemm_descriptor builds the
descriptor the launch always got, a launch without a hint runs what geo4d_conv_gemm_plan says, redirected launches report the tile
that really runs, and the GroupNorm column sums a launch attaches have the plan's rows per entry. Shapes are the smallest that still
cover more than one workgroup tile, a ragged M and the K-slab counts on both sides of the third generation's rule (even and >= 4)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def rnd(shape, dev, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(dtype)


@pytest.fixture
def no_tuning(monkeypatch):
    """No autotuning and an empty tuning table: a launch that names no tile is the library's own choice."""
    from geo4d_amd import ops
    ops._tune_table()
    monkeypatch.setattr(ops, "AUTOTUNE", False)
    monkeypatch.setattr(ops, "_TUNE", {})
    return ops


def descriptor_cases(ops, dev):
    """name -> (a, w, out, keyword arguments of conv_gemm): one call per operand format."""
    z = lambda shape, dtype: torch.zeros(shape, device=dev, dtype=dtype)
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    M, N, K = 96, 64, 128
    split = lambda t: t.as_subclass(ops.SplitAct)
    x2w = ops.X2Weight.wrap(z((N, 2 * K), f16), 0.25)
    geo = dict(M=M, N=N, K=K, Cin=K)
    return {
        "bf16": (z((M, K), bf), z((N, K), bf), z((M, N), bf), dict(geo, lda=K, ldw=K, ldo=N, bias=z((N,), f32), residual=z((M, N), bf), ldr=N, act=1)),
        "f32_x3_batched": (z((3, M, K), f32), z((3, N, K), f32), z((3, M, N), f32),
                           dict(geo, lda=K, ldw=K, ldo=N, batch=3, a_bs=M * K, w_bs=N * K, o_bs=M * N, x3=True, alpha=0.5)),
        "raw_f32_x_split_w": (z((M, K), f32), z((N, 2 * K), bf), z((M, N), f32),
                              dict(geo, lda=K, ldw=2 * K, ldo=N, rowbias=z((2, N), f32), rowbias_div=48, tile_hint=25, split_k=2)),
        "split_act_x_split_w_split_out": (split(z((M, 2 * K), bf)), z((N, 2 * K), bf), split(z((M, 2 * N), bf)),
                                          dict(geo, lda=2 * K, ldw=2 * K, ldo=2 * N, residual=z((M, N), f32), ldr=N)),
        "split_w_as_A_batched": (z((N, 2 * K), bf), split(z((3 * M, 2 * K), bf)), split(z((3, N, 2 * M), bf)),
                                 dict(M=N, N=M, K=K, Cin=K, lda=2 * K, ldw=2 * K, ldo=2 * M, batch=3, a_bs=0, w_bs=M * 2 * K, o_bs=N * 2 * M)),
        "f16_rows_x_x2weight_f32_out": (z((M, K), f16), x2w, z((M, N), f32), dict(geo, lda=K, ldw=2 * K, ldo=N, bias=z((N,), f32), alpha=2.0)),
        "f16_rows_x_x2weight_f16_out": (z((M, K), f16), x2w, z((M, N // 2), f16), dict(geo, lda=K, ldw=2 * K, ldo=N // 2, act=2)),
        "conv3x3_stride2_ncthw": (z((2 * 8 * 8, 64), bf), z((N, 9 * 64), bf), z((1, N, 2, 4, 4), bf),
                                  dict(M=32, N=N, K=9 * 64, Cin=64, lda=64, ldw=9 * 64, ldo=N, T=2, Hin=8, Win=8, Hout=4, Wout=4, KH=3, KW=3, ph=1, pw=1,
                                       stride=2, out_nchw=True)),
    }


POINTERS = ("A", "W", "O", "bias", "rowbias", "R", "zeros", "workspace", "gn_colsum", "sat_count")
# The non-pointer fields of the geo4d_conv_gemm_t that conv_gemm handed to the library for each of descriptor_cases() at the commit before the
# builder was split off (4a2fcbb), written down from one run of that commit with the lib.geo4d_conv_gemm call intercepted. Fields not listed are 0.
# a plain linear's geometry, batch and alpha: what every case below starts from
LINEAR = dict(workspace_bytes=268435456, batch=1, T=1, Hin=1, Win=1, Hout=1, Wout=1, KT=1, KH=1, KW=1, stride=1, ups=1, alpha=1.0)
PARENT_FIELDS = {
    "bf16": dict(LINEAR, lda=128, ldw=128, ldo=64, ldr=64, M=96, N=64, K=128, Cin=128, act=1, dtype=1, out_dtype=1),
    "f32_x3_batched": dict(LINEAR, lda=128, ldw=128, ldo=64, a_bs=12288, w_bs=8192, o_bs=6144, M=96, N=64, K=128, batch=3, Cin=128, dtype=3, alpha=0.5),
    "raw_f32_x_split_w": dict(LINEAR, lda=128, ldw=128, ldo=64, ldrb=64, M=96, N=64, K=128, Cin=128, rowbias_div=48, dtype=3, tile_hint=25, split_k=2, w_split=1),
    "split_act_x_split_w_split_out": dict(LINEAR, lda=128, ldw=128, ldo=64, ldr=64, M=96, N=64, K=128, Cin=128, dtype=3, a_split=1, w_split=1, o_split=1),
    "split_w_as_A_batched": dict(LINEAR, lda=128, ldw=128, ldo=96, w_bs=12288, o_bs=6144, M=64, N=96, K=128, batch=3, Cin=128, dtype=3, a_split=1, w_split=1, o_split=1),
    "f16_rows_x_x2weight_f32_out": dict(LINEAR, lda=128, ldw=128, ldo=64, M=96, N=64, K=128, Cin=128, dtype=4, alpha=0.5, a_split=2, w_split=1),
    "f16_rows_x_x2weight_f16_out": dict(LINEAR, lda=128, ldw=128, ldo=32, M=96, N=64, K=128, Cin=128, act=2, dtype=4, alpha=0.25, a_split=2, w_split=1, o_split=2),
    "conv3x3_stride2_ncthw": dict(LINEAR, lda=64, ldw=576, ldo=64, M=32, N=64, K=576, Cin=64, T=2, Hin=8, Win=8, Hout=4, Wout=4, KH=3, KW=3, ph=1, pw=1, stride=2, dtype=1, out_dtype=1, out_nchw=1),
}


def fields_of(p):
    return {name: getattr(p, name) for name, _ in type(p)._fields_ if name not in POINTERS and getattr(p, name) != 0}


def test_descriptor_builder_fills_what_conv_gemm_always_passed(dev):
    from geo4d_amd import ops
    ws, zeros = ops.workspace(dev)
    cases = descriptor_cases(ops, dev)
    assert set(cases) == set(PARENT_FIELDS)
    for name, (a, w, out, kw) in cases.items():
        p = ops.conv_gemm_descriptor(a, w, out, **kw)
        assert fields_of(p) == PARENT_FIELDS[name], name
        want = dict(A=a.data_ptr(), W=w.data_ptr(), O=out.data_ptr(), zeros=zeros.data_ptr(), workspace=ws.data_ptr(), gn_colsum=None, sat_count=None)
        for nm in ("bias", "rowbias"):
            want[nm] = kw[nm].data_ptr() if nm in kw else None
        want["R"] = kw["residual"].data_ptr() if "residual" in kw else None
        assert {nm: getattr(p, nm) for nm in POINTERS} == want, name


def gemm_case(ops, dev, kind, M, N, K, batch=1, act=0, f16_out=False, split_out=False):
    """(a, w, fresh-output factory, keyword arguments of conv_gemm) with fixed-seed normal inputs."""
    from geo4d_amd import pack
    nout = N // 2 if act == 2 else N
    x, wt = rnd((batch * M, K), dev, 11), rnd((batch * N, K), dev, 12, scale=K ** -0.5)
    kw = dict(M=M, N=N, K=K, Cin=K, Hin=M, Hout=M, act=act, bias=rnd((N,), dev, 13), batch=batch)
    if kind == "bf16":
        a, w, odt = x.to(torch.bfloat16), wt.to(torch.bfloat16), torch.bfloat16
    elif kind == "f16x2":
        a, w, odt = x.to(torch.float16), pack.split_f16(wt), (torch.float16 if f16_out else torch.float32)
    else:                   # bf16x3: raw f32 rows, or pre-split rows, against a pre-split weight
        a, w, odt = (ops.SplitAct.wrap(pack.split_bf16(x)) if kind == "x3split" else x), pack.split_bf16(wt), torch.float32
    if split_out:
        new = lambda: ops.new_split(batch * M, nout, dev)
    else:
        new = lambda: torch.empty((batch * M, nout), device=dev, dtype=odt)
    ldo = new().stride(0)
    kw.update(lda=a.stride(0), ldw=w.stride(0), ldo=ldo, a_bs=M * a.stride(0), w_bs=N * w.stride(0), o_bs=M * ldo)
    return a, w, new, kw


def bits(t):
    return t.as_subclass(torch.Tensor)


@pytest.mark.parametrize("kind,M,N,K,batch,extra,hint", [
    ("bf16", 256, 128, 256, 1, {}, None),
    ("bf16", 77, 128, 256, 1, {}, None),                               # M not a multiple of 32
    ("bf16", 96, 64, 128, 3, {}, None),
    ("f16x2", 128, 128, 256, 1, {}, 25),
    ("f16x2", 128, 128, 256, 1, dict(act=2, f16_out=True), 25),
    ("x3raw", 256, 128, 128, 1, {}, None),
], ids=["bf16", "bf16-ragged-M", "bf16-batch3", "f16x2", "f16x2-geglu-f16-rows", "bf16x3-raw-A"])
def test_the_default_launch_runs_what_the_plan_says(dev, no_tuning, kind, M, N, K, batch, extra, hint):
    ops = no_tuning
    a, w, new, kw = gemm_case(ops, dev, kind, M, N, K, batch, **extra)
    plan = ops.conv_gemm_plan(ops.conv_gemm_descriptor(a, w, new(), **kw))
    assert plan.tile_hint > 0 and plan.splits >= 1 and (hint is None or plan.tile_hint == hint), (plan.tile_hint, plan.splits)
    by_default = ops.conv_gemm(a, w, new(), **kw)
    as_planned = ops.conv_gemm(a, w, new(), tile_hint=plan.tile_hint, split_k=plan.splits, **kw)
    assert torch.equal(by_default, as_planned), (plan.tile_hint, plan.splits)
    assert bool(torch.isfinite(by_default.float()).all()) and float(by_default.float().abs().max()) > 0.1


@pytest.mark.parametrize("kind,K,asked,runs,split_out", [("bf16", 256, 73, 73, False),      # 4 K slabs
                                                         ("bf16", 192, 73, 25, False),      # 3: an odd count leaves the third generation
                                                         ("x3split", 128, 1, 25, True)],    # a pre-split output leaves the first
                         ids=["native-73", "73-to-25", "1-to-25"])
def test_redirected_launches_report_the_tile_that_runs(dev, no_tuning, kind, K, asked, runs, split_out):
    ops = no_tuning
    a, w, new, kw = gemm_case(ops, dev, kind, 256, 128, K, split_out=split_out)
    plan = ops.conv_gemm_plan(ops.conv_gemm_descriptor(a, w, new(), tile_hint=asked, split_k=1, **kw))
    assert (plan.tile_hint, plan.splits, plan.osplit) == (runs, 1, int(split_out))
    got = ops.conv_gemm(a, w, new(), tile_hint=asked, split_k=1, **kw)
    assert torch.equal(bits(got), bits(ops.conv_gemm(a, w, new(), tile_hint=runs, split_k=1, **kw)))
    assert float(bits(got).float().abs().max()) > 0.1


@pytest.mark.parametrize("hint,split,rows", [(25, 1, 64), (73, 1, 128), (1, 1, 32), (25, 2, 32)], ids=["25", "73", "1", "25-split2"])
def test_column_sums_follow_the_plan(dev, no_tuning, monkeypatch, hint, split, rows):
    """bf16x3, raw f32 rows x pre-split weight -> f32 rows with gn_stats: the sums attached to the output have the plan's rows per entry
    (wave-tile rows of the second / third generation, 32 from the first generation's epilogue and from a split-K reduce launch) and
    equal per-block sums of the output itself to 2e-6 relative L2, the bound tests/test_bf16x3_gpu.py holds these sums to. Level 2 of
    GN_FUSED_STATS lets the first-generation hint emit them too; at the default level it attaches none, at level 0 nobody does."""
    ops = no_tuning
    M, N, K = 256, 128, 128
    a, w, new, kw = gemm_case(ops, dev, "x3raw", M, N, K)
    plan = ops.conv_gemm_plan(ops.conv_gemm_descriptor(a, w, new(), tile_hint=hint, split_k=split, **kw))
    assert (plan.tile_hint, plan.splits, plan.colsum_rows) == (hint, split, rows)
    for level in (2, 1, 0):
        monkeypatch.setattr(ops, "GN_FUSED_STATS", level)
        out = ops.conv_gemm(a, w, new(), tile_hint=hint, split_k=split, gn_stats=True, **kw)
        if level == 0 or (level == 1 and plan.generation == 1):
            assert getattr(out, "_gn_colsum", None) is None, level
            continue
        assert out._gn_colsum_rows == plan.colsum_rows and out._gn_colsum.shape == (M // rows, N, 2), level
        o = out.double().reshape(M // rows, rows, N)
        ref = torch.stack([o.sum(1), (o ** 2).sum(1)], -1).float()
        err = ((out._gn_colsum - ref).norm() / ref.norm()).item()
        print(f"[colsum hint {hint} split {split} level {level}] rel_l2={err:.3e} tol=2e-6")
        assert err < 2e-6, (level, err)
        assert torch.equal(out, ops.conv_gemm(a, w, new(), tile_hint=hint, split_k=split, **kw)), level      # the sums do not change the output
