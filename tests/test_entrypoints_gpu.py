"""Direct parity tests for the entry points of include/geo4d_hip.h that only the end-to-end fixtures reached: the erf-GELU epilogue of
geo4d_conv_gemm (act = 3) on every kernel generation, the causal row softmax, embed_tokens, gather_timestep / advance_index, the two
Adam steps, ddim_step beyond one grid, linear_small beyond one pass, the temporal attention at every T, and one transformer block of the
OpenCLIP towers at ViT-H-14 size.

Conventions of tests/test_kernels_gpu.py: seeded CPU generators, a check() that prints rel_l2 / max_abs / tol for every case, and
references in fp64 computed from the rounded operands the kernel multiplies. Tolerances are the per-mode ones of the sibling files
(test_kernels_gpu.py for the first generation and the memory-bound kernels, test_bf16x3_gpu.py 5e-5, test_gemm_v2_gpu.py 3e-5 for bf16x3
on the second / third generation, test_f16x2_gpu.py 1e-5 against the operands the two-pass GEMM sees, test_frontend_gpu.py for the block).
Every refusal case is rejected by the host code before any launch."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest
import torch

from test_f16x2_gpu import a_seen, split_f16_act, weight_seen
from test_gemm_v2_gpu import both_grids
from test_presplit_gpu import check_split

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TOL = {torch.float32: 2e-5, torch.bfloat16: 6e-3, torch.float16: 1e-3}


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def check_tol(name, got, ref, tol, what=""):
    e = rel(got, ref)
    m = (got.double() - ref.double()).abs().max().item()
    print(f"[{name}] {what} rel_l2={e:.3e} max_abs={m:.3e} tol={tol:.1e}")
    assert math.isfinite(e) and e <= tol, f"{name}: rel_l2 {e:.3e} > {tol:.1e}"
    return e


def check(name, got, ref, dtype, scale=1.0):
    return check_tol(name, got, ref, TOL[dtype] * scale, f"dtype={dtype}")


def rnd(shape, dev, dtype, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(dtype)


# ---- 1. erf-GELU epilogue of geo4d_conv_gemm (act = 3) ---------------------------------------------------------------------------------
G1_TILES, G2_TILES, G3_TILES = [0, 1, 3, 5, 11, 13], [22, 23, 25, 27, 28], [71, 72, 73, 74]
GELU_CASES = ([(t, m) for t in G1_TILES for m in ("f32", "bf16", "f16", "bf16x3")] + [(0, "f16x2")] +       # (hint 0 of the two-pass mode = the library's pick)
              [(t, m) for t in G2_TILES + G3_TILES for m in ("bf16", "bf16x3", "f16x2")])
# first generation: test_kernels_gpu.py / test_bf16x3_gpu.py; second / third: test_gemm_v2_gpu.py / test_f16x2_gpu.py
GELU_TOL = {(1, "f32"): 2e-5, (1, "bf16"): 6e-3, (1, "f16"): 1e-3, (1, "bf16x3"): 5e-5, (1, "f16x2"): 1e-5,
            (2, "bf16"): 6e-3, (2, "bf16x3"): 3e-5, (2, "f16x2"): 1e-5}


def gelu64(h):
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))


def gemm_operands(mode, x, w):
    """(A operand, packed W, A as multiplied fp64, W as multiplied fp64) of one compute mode for f32 x [M, K], w [N, K]."""
    from geo4d_amd import pack
    if mode == "f32":
        return x, w, x.double(), w.double()
    if mode in ("bf16", "f16"):
        dt = torch.bfloat16 if mode == "bf16" else torch.float16
        return x.to(dt), pack.pack_linear(w, dt), x.to(dt).double(), w.to(dt).double()
    if mode == "bf16x3":          # ~16 mantissa bits of both operands: the sibling files compare with the unrounded operands
        return x, pack.pack_linear(w, "bf16x3"), x.double(), w.double()
    wp = pack.split_f16(w)        # f16x2: plain f16 activation rows x an f16 hi + lo weight
    return split_f16_act(x), wp, a_seen(x), weight_seen(wp)


@pytest.mark.parametrize("tile,mode", GELU_CASES)
def test_gelu_epilogue(dev, tile, mode):
    """out = gelu(x . W^T + b), pre-activations spanning about +-6 (sigma 2), ragged M, N % 8 == 0: the vectorised epilogue of every tile
    unsplit, and the split-K reduce kernel (split_k = 2) on a deep-K shape."""
    from geo4d_amd import ops
    tol = GELU_TOL[(1 if tile < 22 else 2, mode)]
    for M, K, N, split in ((333, 512, 136, 1), (150, 2048, 72, 2)):
        x = rnd((M, K), dev, torch.float32, 400 + split)
        w = rnd((N, K), dev, torch.float32, 410 + split, 2.0 / math.sqrt(K))
        b = rnd((N,), dev, torch.float32, 420 + split, 0.5)
        a, wp, a64, w64 = gemm_operands(mode, x, w)
        run = lambda: ops.linear(a, wp, b, act=3, tile_hint=tile, split_k=split)
        out = both_grids(run) if tile >= 22 else run()
        h = a64 @ w64.t() + b.double()
        assert float(h.abs().max()) > 6.0 and float(h.std()) > 1.5          # the pre-activation does span the range
        assert out.shape == (M, N)
        check_tol(f"gelu tile{tile} split{split}", out, gelu64(h), tol, mode)


@pytest.mark.parametrize("tile,split,K", [(0, 1, 64), (1, 2, 512)])
def test_gelu_pointwise_accuracy(dev, tile, split, K):
    """erf_as (common.h: Abramowitz-Stegun 7.1.26 over v_rcp / v_exp) point by point: exact-f32 mode, W = identity, so the pre-activation is
    x itself and the output is gelu(x) up to the epilogue. |got - ref| <= 0.5 |x| 3e-7 + 2^-22 |ref|: 3e-7 on erf = twice the 1.5e-7 the
    formula is known for (the margin covers the 1-ulp v_rcp / v_exp and the fp32 evaluation), 2^-22 |ref| = the roundings of the two
    products around it. Both the tile epilogue and the split-K reduce kernel (K = 512: a split needs 8 slabs; x . 1 + 0 stays exact).
    Measured on MI355X: max |got - ref| = 4.62e-7, i.e. 4.61e-7 as an error of erf (both paths) - the fp32 evaluation triples the formula's
    own 1.5e-7, inside the bound."""
    from geo4d_amd import ops
    grid = torch.linspace(-8.0, 8.0, 65536 - 2, dtype=torch.float64)
    x = torch.cat([grid, torch.tensor([0.0, -0.0], dtype=torch.float64)]).float().reshape(65536 // K, K).to(dev)
    out = ops.linear(x, torch.eye(K, device=dev), None, act=3, tile_hint=tile, split_k=split)
    ref = gelu64(x.double())
    err = (out.double() - ref).abs()
    bound = 0.5 * x.double().abs() * 3e-7 + 2.0 ** -22 * ref.abs()
    i = int((err / bound.clamp_min(1e-30)).argmax())
    as_erf = (err / (0.5 * x.double().abs()).clamp_min(1e-30))[x.abs() > 1e-3].max().item()
    print(f"[gelu pointwise tile{tile} split{split}] max |got - ref| = {err.max().item():.3e}; as an error of erf (|x| > 1e-3): {as_erf:.3e}; "
          f"worst point x = {x.flatten()[i].item():.6f}: err {err.flatten()[i].item():.3e} vs bound {bound.flatten()[i].item():.3e}")
    assert bool((out[x == 0] == 0).all())
    assert bool((err <= bound).all()), f"gelu(x) at x = {x.flatten()[i].item()}: {err.flatten()[i].item():.3e} > {bound.flatten()[i].item():.3e}"


def test_gelu_refusals(dev):
    """gemm.hip: GELU lives in the vectorised epilogue only - a residual, an NCTHW output or N % 8 != 0 is refused, not mis-computed."""
    from geo4d_amd import ops
    M, K, N = 64, 64, 64
    x, w, b = rnd((M, K), dev, torch.float32, 430), rnd((N, K), dev, torch.float32, 431, 0.1), rnd((N,), dev, torch.float32, 432)
    ops.linear(x, w, b, act=3)                                             # the same launch without the offending argument is served
    with pytest.raises(RuntimeError):
        ops.linear(x, w, b, act=3, residual=rnd((M, N), dev, torch.float32, 433))
    with pytest.raises(RuntimeError):
        ops.conv2d(x, w, b, F=1, Hin=8, Win=8, KH=1, KW=1, T=1, act=3, out_nchw=True)
    with pytest.raises(RuntimeError):
        ops.linear(x, w[:60], b[:60].contiguous(), act=3)


# ---- 2. causal row softmax ------------------------------------------------------------------------------------------------------------
SENTINEL = 7.5          # exact in every output type


def softmax_ref(x, scale, period):
    s = x.double() * scale
    if period:
        rows, cols = s.shape
        r = torch.arange(rows, device=x.device)[:, None] % period
        masked = torch.arange(cols, device=x.device)[None, :] > r
        s = s.masked_fill(masked, float("-inf"))
        return torch.softmax(s, -1), masked
    return torch.softmax(s, -1), None


def run_softmax(dev, x, scale, dtype, period, ldy):
    from geo4d_amd import ops
    rows, cols = x.shape
    buf = torch.full((rows, ldy), SENTINEL, device=dev, dtype=dtype)
    ops.softmax_rows(x, scale, dtype, out=buf[:, :cols], causal_period=period)
    return buf


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(16 * 77, 77, 77, 128), (3 * 300, 300, 300, 320), (2 * 40, 64, 40, 64), (4 * 257, 257, 0, 320)])
def test_softmax_rows_causal(dev, dtype, case):
    """The three properties the text tower relies on: the masked tail inside `cols` is exact zeros, the columns [cols, ldy) of a wider
    output row (K padding of the P.V GEMM) are untouched, row 0 of every period sees one column. 300 and 257 columns walk the strided
    column loop of the 256-thread row kernel; (80, 64, 40) has period < cols; period 0 is the plain kernel on a wider output."""
    rows, cols, period, ldy = case
    x = rnd((rows, cols), dev, torch.float32, 440) * 4
    buf = run_softmax(dev, x, 0.25, dtype, period, ldy)
    ref, masked = softmax_ref(x, 0.25, period)
    out = buf[:, :cols]
    check(f"softmax causal {case}", out, ref, dtype)
    assert torch.equal(buf[:, cols:], torch.full((rows, ldy - cols), SENTINEL, device=dev, dtype=dtype)), "columns beyond `cols` were written"
    if period:
        assert bool((out[masked] == 0).all()), "masked entries must be exact zeros"
        assert bool((out[~masked] > 0).any())
        first = out[::period]
        assert bool((first[:, 0] == 1).all()) and bool((first[:, 1:] == 0).all()), "row 0 of a period sees column 0 only"
        # a row deep in a period sees exactly r % period + 1 columns (a bound off by one moves this count)
        r = rows - 1
        assert int((out[r] != 0).sum()) <= min(cols, r % period + 1) and float(out[r, min(cols - 1, r % period)]) > 0


@pytest.mark.parametrize("period", [77, 0])
def test_softmax_rows_large_scores(dev, period):
    """Scores of magnitude 1e4 (both signs) stay finite and match: the row maximum is subtracted before the exponential."""
    rows, cols, ldy = 4 * 77, 77, 80
    g = torch.Generator(device="cpu").manual_seed(441)
    x = (1e4 * torch.sign(torch.randn((rows, cols), generator=g)) + 3 * torch.randn((rows, cols), generator=g)).to(dev)
    buf = run_softmax(dev, x, 1.0, torch.float32, period, ldy)
    ref, masked = softmax_ref(x, 1.0, period)
    assert bool(torch.isfinite(buf).all())
    check(f"softmax 1e4 period {period}", buf[:, :cols], ref, torch.float32)
    assert bool((buf[:, cols:] == SENTINEL).all())
    if period:
        assert bool((buf[:, :cols][masked] == 0).all())


# ---- 3. embed_tokens ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [1024, 320])
def test_embed_tokens(dev, dtype, width):
    """out[(b n)] = table[id] + pos[n] in fp32, stored with the round-to-nearest-even conversion every kernel of the library uses
    (test_layout_and_concat holds tokens_from_ncthw to torch.equal with .to(dtype) on the same store): bit-equal to torch. Ids outside
    [0, vocab) read row 0 (include/geo4d_hip.h); 2^32 + 5 would land on row 5 if the id were truncated to 32 bits."""
    from geo4d_amd import ops
    B, n_ctx, vocab = 3, 77, 1000
    table, pos = rnd((vocab, width), dev, torch.float32, 450), rnd((n_ctx, width), dev, torch.float32, 451, 0.3)
    g = torch.Generator(device="cpu").manual_seed(452)
    tokens = torch.randint(0, vocab, (B, n_ctx), generator=g, dtype=torch.int64)
    tokens[0, :7] = torch.tensor([0, vocab - 1, vocab, -1, 2 ** 32 + 5, -(2 ** 40), 2 ** 62])
    tokens[2, -1] = vocab + 3
    tokens = tokens.to(dev)
    out = ops.embed_tokens(tokens, table, pos, dtype)
    safe = torch.where((tokens >= 0) & (tokens < vocab), tokens, torch.zeros_like(tokens))
    ref = (table[safe] + pos[None]).reshape(B * n_ctx, width).to(dtype)
    assert out.shape == ref.shape and out.dtype == dtype
    bad = (out != ref).any(1).nonzero().flatten().tolist()
    print(f"[embed_tokens] dtype={dtype} width={width} rows differing from torch: {bad}")
    assert torch.equal(out, ref)


def test_round_to_nearest_even_matches_torch_cpu():
    """The equality test_embed_tokens relies on, for the conversion semantics alone: torch's .to(bfloat16 / float16) is round-to-nearest-even
    with ties to even (checked on exact ties), which is what the hardware conversion behind Elem<T>::st does."""
    for dt, bits in ((torch.bfloat16, 8), (torch.float16, 11)):
        ulp = 2.0 ** (1 - bits)                     # spacing in [1, 2)
        ties = torch.tensor([1.0 + 0.5 * ulp, 1.0 + 1.5 * ulp, 1.0 + 2.5 * ulp, -(1.0 + 0.5 * ulp)])
        want = torch.tensor([1.0, 1.0 + 2 * ulp, 1.0 + 2 * ulp, -1.0])
        assert torch.equal(ties.to(dt).float(), want)


# ---- 4. gather_timestep / advance_index -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4, 1024])
def test_gather_timestep_and_advance_index(dev, B):
    from geo4d_amd import ops
    S = 50
    table = (torch.arange(S, dtype=torch.int64) * 20 + 19 + (torch.arange(S, dtype=torch.int64) % 2) * (2 ** 33)).to(dev)     # 64-bit payloads
    for start, delta, want in ((1, -1, 0), (S - 2, 1, S - 1), (S - 1, -(S - 1), 0), (0, S - 1, S - 1)):
        idx = torch.tensor([start], device=dev, dtype=torch.int32)
        ops.advance_index(idx, delta)
        assert idx.item() == want
        buf = torch.full((B + 8,), -7, device=dev, dtype=torch.int64)
        ops.gather_timestep(idx, table, buf[:B])
        assert bool((buf[:B] == table[want]).all()) and bool((buf[B:] == -7).all()), f"B={B} row {want}"
        assert idx.item() == want                    # the gather does not move the index


def test_gather_timestep_refusals(dev):
    from geo4d_amd import _lib, ops
    lib = _lib.load()
    idx = torch.zeros(1, device=dev, dtype=torch.int32)
    table = torch.arange(4, device=dev, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.gather_timestep(idx, table, torch.zeros(1025, device=dev, dtype=torch.int64))
    ts = torch.zeros(4, device=dev, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        _lib.check(lib.geo4d_gather_timestep(idx.data_ptr(), None, ts.data_ptr(), 4, ops._stream()), "geo4d_gather_timestep")
    with pytest.raises(RuntimeError):
        _lib.check(lib.geo4d_advance_index(None, 1, ops._stream()), "geo4d_advance_index")


# ---- 5. Adam --------------------------------------------------------------------------------------------------------------------------
ADAM_STEPS = 50


def f32(v):
    return float(np.float32(v))


def adam_inputs(n):
    """Start values and ADAM_STEPS gradients (CPU, fp32): a tenth of the entries of every step are zero, a tenth of 1e-12 scale."""
    g = torch.Generator(device="cpu").manual_seed(460 + n % 1000)
    p0 = torch.randn(n, generator=g)
    grads = []
    for _ in range(ADAM_STEPS):
        gr = torch.randn(n, generator=g)
        u = torch.rand(n, generator=g)
        gr = torch.where(u < 0.1, torch.zeros_like(gr), torch.where(u < 0.2, gr * 1e-12, gr))
        grads.append(gr)
    return p0, grads


def adam_fp64(p0, grads, lr, b1, b2, eps):
    """torch.optim.Adam (no weight decay, no amsgrad) restated in fp64 on the fp32 inputs."""
    p, m, v = p0.double(), torch.zeros_like(p0, dtype=torch.float64), torch.zeros_like(p0, dtype=torch.float64)
    for t, g in enumerate(grads, 1):
        g = g.double()
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - (lr / (1 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    return p, m, v


def adam_torch_fp32(p0, grads, lr, b1, b2, eps):
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    for g in grads:
        p.grad = g.clone()
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


def host_hyper(lr, b1, b2, t):
    """{lr, 1 - beta1^t, sqrt(1 - beta2^t)} in fp32 as geo4d_adam_step derives them (align.hip: powf, sqrtf)."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    bc1 = np.float32(1.0) - np.float32(libm.powf(b1, float(t)))
    bc2 = np.float32(1.0) - np.float32(libm.powf(b2, float(t)))
    return [lr, float(bc1), float(np.sqrt(bc2))]


@pytest.mark.parametrize("n", [1, 255, 4099, 163840])
def test_adam_steps(dev, n):
    """geo4d_adam_step and geo4d_adam_step_dev over 50 steps against torch.optim.Adam restated in fp64: parameters and both moments may be
    at most 4x as far from the fp64 trajectory as torch's own fp32 Adam on the CPU is, plus 1e-7 relative (the factor allows another
    legitimate operation order). adam_kernel and adam_dev_kernel (align.hip) are the same arithmetic on {lr, bias corrections}, so with the
    hyper-parameters built like the host entry point builds them the two trajectories are bit-equal."""
    from geo4d_amd import _lib, ops
    lib = _lib.load()
    lr, b1, b2, eps = f32(0.01), f32(0.9), f32(0.999), f32(1e-8)
    p0, grads = adam_inputs(n)
    ref = adam_fp64(p0, grads, lr, b1, b2, eps)
    tch = adam_torch_fp32(p0, grads, lr, b1, b2, eps)
    host = [p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    devs = [p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    for t, g in enumerate(grads, 1):
        gd = g.to(dev)
        _lib.check(lib.geo4d_adam_step(host[0].data_ptr(), gd.data_ptr(), host[1].data_ptr(), host[2].data_ptr(), n, lr, b1, b2, eps, t,
                                       ops._stream()), "geo4d_adam_step")
        hyper = torch.tensor(host_hyper(lr, b1, b2, t), dtype=torch.float32).to(dev)
        _lib.check(lib.geo4d_adam_step_dev(devs[0].data_ptr(), gd.data_ptr(), devs[1].data_ptr(), devs[2].data_ptr(), n, hyper.data_ptr(), b1, b2,
                                           eps, ops._stream()), "geo4d_adam_step_dev")
    torch.cuda.synchronize()
    for what, got in (("adam_step", host), ("adam_step_dev", devs)):
        for name, k, r, c in zip(("param", "exp_avg", "exp_avg_sq"), got, ref, tch):
            dk, dt = rel(k.cpu(), r), rel(c, r)
            print(f"[{what} n={n}] {name}: kernel vs fp64 {dk:.3e}   torch fp32 vs fp64 {dt:.3e}   bound {4 * dt + 1e-7:.3e}")
            assert math.isfinite(dk) and dk <= 4 * dt + 1e-7, f"{what} n={n} {name}: {dk:.3e} > 4 x {dt:.3e} + 1e-7"
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), host, devs):
        assert torch.equal(a, b), f"adam_step and adam_step_dev differ in {name}"


def test_adam_refusals(dev):
    """`step` counts from 1 (geo4d_adam_step; geo4d_adam_step_dev has no step argument: its bias corrections come in `hyper`, which must
    not be null); empty tensors and null pointers are refused."""
    from geo4d_amd import _lib, ops
    lib = _lib.load()
    p, g, m, v = (torch.zeros(8, device=dev) for _ in range(4))
    hyper = torch.tensor([0.01, 0.1, 0.03], device=dev)
    args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
    for step, n in ((0, 8), (-1, 8), (1, 0)):
        with pytest.raises(RuntimeError):
            _lib.check(lib.geo4d_adam_step(*args, n, 0.01, 0.9, 0.999, 1e-8, step, ops._stream()), "geo4d_adam_step")
    for h, n in ((None, 8), (hyper.data_ptr(), 0)):
        with pytest.raises(RuntimeError):
            _lib.check(lib.geo4d_adam_step_dev(*args, n, h, 0.9, 0.999, 1e-8, ops._stream()), "geo4d_adam_step_dev")
    assert all(float(t.abs().max()) == 0 for t in (p, m, v))


# ---- 6. ddim_step ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096 * 256 + 777, 2359296])
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("with_x0", [True, False])
def test_ddim_step_grid_stride(dev, n, with_noise, with_x0):
    """More elements than the 4096 x 256 threads of the capped grid (n = 2 359 296 = a 576 x 1024 window's latent): the grid-stride loop,
    its ragged last pass, the optional noise / pred_x0 pointers, a coefficient row in the middle of a table whose other rows would be
    visibly wrong, and nothing written past n."""
    from geo4d_amd import ops
    pad = 64
    xb, x0b = torch.full((n + pad,), SENTINEL, device=dev), torch.full((n + pad,), SENTINEL, device=dev)
    xb[:n] = rnd((n,), dev, torch.float32, 470)
    v = rnd((n,), dev, torch.float32, 471)
    nz = rnd((n,), dev, torch.float32, 472)
    xr = xb[:n].clone()
    row = [0.6, 0.8, 0.9, 0.7, 0.5, 0.1]
    coef = torch.tensor([[1e3] * 6, [-5.0] * 6, row, [0.0] * 6, [7.0] * 6], device=dev)
    idx = torch.tensor([2], device=dev, dtype=torch.int32)
    ops.ddim_step(xb[:n], v, coef, idx, noise=nz if with_noise else None, pred_x0=x0b[:n] if with_x0 else None)
    sa, s1, rs, sp, dc, sg = (float(c) for c in coef[2].double().cpu())
    e_t = sa * v.double() + s1 * xr.double()
    p0 = (sa * xr.double() - s1 * v.double()) * rs
    xp = sp * p0 + dc * e_t + (sg * nz.double() if with_noise else 0.0)
    check_tol(f"ddim x_prev n={n} noise={with_noise} x0={with_x0}", xb[:n], xp, 2e-6)
    if with_x0:
        check_tol(f"ddim pred_x0 n={n}", x0b[:n], p0, 2e-6)
    else:
        assert bool((x0b == SENTINEL).all())
    assert bool((xb[n:] == SENTINEL).all()) and bool((x0b[n:] == SENTINEL).all()), "ddim_step wrote past n"
    assert idx.item() == 2


# ---- 7. linear_small ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 8, 9, 17])
@pytest.mark.parametrize("N,K", [(301, 100), (1280, 320)])
def test_linear_small_passes_and_ragged_shapes(dev, M, N, K):
    """M > 8 walks the 8-rows-per-pass loop (9 and 17 leave a ragged last pass), K = 100 is not a multiple of the 64 lanes, N = 301 not
    of the 4 waves of a workgroup; `add` is a column view of a wider tensor; every act_in / act_out combination."""
    from geo4d_amd import ops
    x = rnd((M, K), dev, torch.float32, 480)
    w, b = rnd((N, K), dev, torch.float32, 481, 1.0 / math.sqrt(K)), rnd((N,), dev, torch.float32, 482)
    wide = rnd((M, N + 16), dev, torch.float32, 483)
    add = wide[:, 8:8 + N]
    silu = lambda t: t / (1.0 + torch.exp(-t))
    for act_in in (False, True):
        for act_out in (False, True):
            obuf = torch.full((M, N + 4), SENTINEL, device=dev)
            ops.linear_small(x, w, b, add=add, act_in=act_in, act_out=act_out, out=obuf[:, :N])
            h = (silu(x.double()) if act_in else x.double()) @ w.double().t() + b.double()
            ref = (silu(h) if act_out else h) + add.double()
            check(f"linear_small M={M} N={N} K={K} act_in={act_in} act_out={act_out}", obuf[:, :N], ref, torch.float32)
            assert bool((obuf[:, N:] == SENTINEL).all())
    plain = ops.linear_small(x, w)                      # no bias, no add
    check(f"linear_small M={M} N={N} K={K} plain", plain, x.double() @ w.double().t(), torch.float32)


# ---- 8. temporal attention ------------------------------------------------------------------------------------------------------------
def temporal_ref(qkv, B, T, HW, H, scale):
    f = qkv.double().reshape(B, T, HW, 3, H, 64).permute(3, 0, 2, 4, 1, 5)      # [3, B, HW, H, T, 64]
    o = torch.softmax(f[0] @ f[1].transpose(-1, -2) * scale, -1) @ f[2]
    return o.permute(0, 3, 1, 2, 4).reshape(B * T * HW, H * 64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", [(1, 1, 1), (2, 7, 3), (1, 37, 5)])
def test_temporal_attention_every_T(dev, dtype, geom):
    """T = 1, 2, 3, 8, 15, 16 frames: the zero-filled frame slots, the key mask and the write guard of the 16-slot kernel; one unit, and
    185 units (not a multiple of the 4 per workgroup); q / k / v are column views of one fused projection; the output is pre-filled, so
    an element its unit did not write, or one written by another unit, shows in the full-tensor comparison. f32 also in the pre-split
    output format (the bf16x3 mode's to_out operand)."""
    from geo4d_amd import ops
    B, HW, H = geom
    C_ = H * 64
    for T in (1, 2, 3, 8, 15, 16):
        rows = B * T * HW
        qkv = rnd((rows, 3 * C_), dev, dtype, 490 + T)
        out = torch.full((rows, C_), 1e4, device=dev, dtype=dtype)
        ops.temporal_attention(qkv[:, :C_], qkv[:, C_:2 * C_], qkv[:, 2 * C_:], B=B, T=T, HW=HW, H=H, scale=0.125, out=out)
        check(f"temporal attn {geom} T={T}", out, temporal_ref(qkv, B, T, HW, H, 0.125), dtype, scale=2.0)
        if dtype == torch.float32:
            sp = ops.temporal_attention(qkv[:, :C_], qkv[:, C_:2 * C_], qkv[:, 2 * C_:], B=B, T=T, HW=HW, H=H, scale=0.125, split_out=True)
            assert isinstance(sp, ops.SplitAct) and sp.shape == (rows, 2 * C_)
            check_split(f"temporal attn {geom} T={T} split_out", sp, out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [15, 16])
def test_temporal_attention_large_logit_and_refusal(dev, dtype, T):
    """A key 4x a query (logit ~ 4 |q|^2 / 8 = 32 above the rest): the softmax must subtract the maximum. T = 17 is refused."""
    from geo4d_amd import ops
    B, HW, H = 2, 7, 3
    C_ = H * 64
    rows = B * T * HW
    qkv = rnd((rows, 3 * C_), dev, dtype, 495)
    t5 = qkv.reshape(B, T, HW, 3, H, 64)
    t5[1, T - 1, 4, 1, 2] = (t5[1, 3, 4, 0, 2].float() * 4).to(dtype)         # key of the LAST frame = 4 x query of frame 3, same unit
    t5[0, 0, 0, 1, 0] = (t5[0, 0, 0, 0, 0].float() * 4).to(dtype)
    out = torch.full((rows, C_), 1e4, device=dev, dtype=dtype)
    ops.temporal_attention(qkv[:, :C_], qkv[:, C_:2 * C_], qkv[:, 2 * C_:], B=B, T=T, HW=HW, H=H, scale=0.125, out=out)
    assert bool(torch.isfinite(out.float()).all())
    check(f"temporal attn spike T={T}", out, temporal_ref(qkv, B, T, HW, H, 0.125), dtype, scale=2.0)
    big = rnd((B * 17 * HW, 3 * C_), dev, dtype, 496)
    with pytest.raises(RuntimeError):
        ops.temporal_attention(big[:, :C_], big[:, C_:2 * C_], big[:, 2 * C_:], B=B, T=17, HW=HW, H=H, scale=0.125)


# ---- 9. one transformer block at ViT-H-14 size ---------------------------------------------------------------------------------------
BLOCK_MODES = [("f32", 2e-4), ("bf16x3", 2e-4), ("bf16x3m", 2e-4), ("f16", 1e-2), ("bf16", 5e-2)]        # = test_frontend_gpu.MODES
TOWERS = {"text": dict(w=1024, heads=16, N=77, B=2, causal=True), "vision": dict(w=1280, heads=16, N=257, B=1, causal=False)}
_block_cache = {}


def block_case(tower, storage):
    """(state dict, input tokens rounded to the storage type, fp64 CPU result of oracle.clip._resblock) of one tower."""
    from geo4d_amd.encoders import _block_shapes
    from oracle.clip import _resblock
    from oracle.params import seeded_state_dict
    key = (tower, storage)
    if key not in _block_cache:
        c = TOWERS[tower]
        shapes = {}
        _block_shapes(lambda n, s: shapes.__setitem__(n, s), "blk", c["w"])
        sd = seeded_state_dict(shapes)
        g = torch.Generator(device="cpu").manual_seed(500)
        x = torch.randn((c["B"] * c["N"], c["w"]), generator=g).to(storage)
        mask = torch.full((c["N"], c["N"]), float("-inf"), dtype=torch.float64).triu_(1) if c["causal"] else None      # text_transformer_forward's
        with torch.no_grad():
            ref = _resblock({k: v.double() for k, v in sd.items()}, "blk", x.double().reshape(c["B"], c["N"], c["w"]), c["heads"], mask)
        _block_cache[key] = (sd, x, ref.reshape(c["B"] * c["N"], c["w"]))
    return _block_cache[key]


@pytest.mark.parametrize("mode,tol", BLOCK_MODES)
@pytest.mark.parametrize("tower", ["text", "vision"])
def test_vit_block_at_vit_h_14_size(dev, tower, mode, tol):
    """encoders._vit_block at the real widths: 16 heads of 64 (text, 77 tokens, causal) and of 80 (vision, 257 tokens) - the head
    dimension zero-padded to the K slab, the batched Q.K^T whose batch stride (dp) is smaller than its row pitch (2 heads dp), the
    softmax over more columns than the row kernel has threads, P.V over a zero-padded K, the GELU epilogue at N = 4 w. The tolerances
    of test_frontend_gpu.py bound whole towers; one block must meet them."""
    from conftest import cpu_threads
    from geo4d_amd.encoders import _pack_block, _vit_block
    from geo4d_amd.precision import resolve
    cpu_threads()
    prec = resolve(mode)
    c = TOWERS[tower]
    sd, x, ref = block_case(tower, prec.storage)
    with torch.no_grad():
        e = _pack_block({k: v.to(dev) for k, v in sd.items()}, "blk", c["w"], c["heads"], prec)
        y = _vit_block(e, x.to(dev), c["B"], c["N"], c["heads"], prec, c["causal"])
    assert y.shape == ref.shape and y.dtype == prec.storage
    check_tol(f"vit block {tower}", y.cpu(), ref, tol, f"mode={mode}")
    delta = rel(y.cpu(), x)          # the block does something: its output is not its input
    assert delta > 0.1, delta
