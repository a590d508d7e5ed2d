"""Counter-based device noise on the GPU: geo4d_philox_fill against the numpy restatement (geo4d_amd/noise.py) bit for bit (words) and to
fp32 round-off (normals), row independence, the fused geo4d_ddim_step_rng against fill + geo4d_ddim_step bit for bit, the sampler at
eta = 1 against the oracle on the same noise (captured == eager), run_clip(step_noise="device") batched == one window at a time, and
classifier-free guidance assembled by image_guided_synthesis itself."""
import functools
import os

import numpy as np
import pytest
import torch

from geo4d_amd import noise
from oracle import ddim as oddim
from oracle import unet as ounet
from oracle.params import seeded_state_dict
from test_parity_gpu import _diffusion, load, rel

pytestmark = pytest.mark.gpu

SEEDS = [123 * 1000003, (7 << 32) | 12345, 2 ** 63 - 2]         # run_clip's window 0 at seed 123; two seeds with a high key word
SIZES = [1, 5, 1030, 4096]                                        # scalar path (a lone element, one ragged quad, 257.5 quads) and whole quads
COUNTERS = [(0, 0, 0), (49, 1, 0), (7, 1, 2)]                     # (step, stream, draw)
BIG = 4096 * 256 * 4 + 8                                          # two quads more than the capped grid covers in one pass
PAD = 64
I_SENT, F_SENT = -1234567, 7.5


@functools.lru_cache(maxsize=None)
def host_words(seed, stream, step, n, draw):
    return noise.philox_words_host(seed, stream, step, n, draw)


@functools.lru_cache(maxsize=None)
def host_normals(seed, stream, step, n, draw):
    return noise.philox_normal_host(seed, stream, step, n, draw)


def seeds_dev(seeds, dev):
    return torch.tensor(list(seeds), dtype=torch.int64, device=dev)


def fill(dev, seeds, n, step, stream, draw, *, raw, scale=1.0, step_on_device=False):
    """philox_fill into the front of a sentinel-padded buffer; returns ([B, n] view, the padding)."""
    from geo4d_amd import ops
    B = len(seeds)
    buf = torch.full((B * n + PAD,), I_SENT if raw else F_SENT, device=dev, dtype=torch.int32 if raw else torch.float32)
    out = buf[:B * n].view(B, n)
    st = torch.tensor([step], device=dev, dtype=torch.int32) if step_on_device else step
    ops.philox_fill(out, seeds_dev(seeds, dev), step=st, stream_id=stream, draw=draw, scale=scale, raw=raw)
    if step_on_device:
        assert st.item() == step
    return out, buf[B * n:]


def normals_close(got, ref, what):
    """|dev - ref| <= 2e-6 max(1, |ref|): both uniforms are exact in fp32 and logf / sqrtf / sincospif are 1-2 ulp functions, so the
    composite is ~5 ulp = 6e-7 relative; 2e-6 leaves a 3x margin."""
    got = got.double().cpu().numpy()
    assert np.isfinite(got).all(), what
    excess = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"[{what}] worst |dev - ref| / max(1, |ref|) = {excess.max():.3e} (bound 2e-6), max |z| = {np.abs(got).max():.3f}")
    assert excess.max() <= 2e-6, what
    assert np.abs(got).max() <= noise.MAX_ABS_NORMAL * (1 + 2e-6)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("step_on_device", [False, True])
def test_raw_words_are_bit_identical_to_the_host_reference(dev, n, step_on_device):
    for step, stream, draw in COUNTERS:
        out, pad = fill(dev, SEEDS, n, step, stream, draw, raw=True, step_on_device=step_on_device)
        got = out.cpu().numpy().view(np.uint32)
        for b, seed in enumerate(SEEDS):
            assert np.array_equal(got[b], host_words(seed, stream, step, n, draw)), (n, step, stream, draw, b)
        assert bool((pad == I_SENT).all()), "philox_fill wrote past the buffer"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("step_on_device", [False, True])
def test_normals_match_the_host_reference(dev, n, step_on_device):
    for step, stream, draw in COUNTERS:
        out, pad = fill(dev, SEEDS, n, step, stream, draw, raw=False, step_on_device=step_on_device)
        ref = np.stack([host_normals(seed, stream, step, n, draw) for seed in SEEDS])
        normals_close(out, ref, f"philox normals n={n} step={step} stream={stream} draw={draw} device_step={step_on_device}")
        assert bool((pad == F_SENT).all()), "philox_fill wrote past the buffer"


def test_fill_beyond_the_capped_grid(dev):
    """More quads than the 4096 x 256 threads of the capped grid: the grid-stride loop's second, ragged pass (first and last 4096
    elements compared; q = element / 4 runs to 2^20 + 1)."""
    seed, (step, stream, draw) = SEEDS[1], COUNTERS[2]
    words, wpad = fill(dev, [seed], BIG, step, stream, draw, raw=True)
    z, zpad = fill(dev, [seed], BIG, step, stream, draw, raw=False, step_on_device=True)
    rw, rz = host_words(seed, stream, step, BIG, draw), host_normals(seed, stream, step, BIG, draw)
    got = words[0].cpu().numpy().view(np.uint32)
    for sl in (slice(0, 4096), slice(BIG - 4096, BIG)):
        assert np.array_equal(got[sl], rw[sl])
        normals_close(z[0, sl], rz[sl], f"philox normals n={BIG} [{sl.start}:{sl.stop}]")
    assert bool(torch.isfinite(z).all()) and bool((wpad == I_SENT).all()) and bool((zpad == F_SENT).all())


def test_scale_multiplies_exactly(dev):
    for n in (1030, 4096):
        one, _ = fill(dev, SEEDS, n, 7, 1, 2, raw=False)
        for scale in (0.5, 1.7):
            scaled, _ = fill(dev, SEEDS, n, 7, 1, 2, raw=False, scale=scale)
            assert torch.equal(scaled, one * torch.tensor(scale, device=dev, dtype=torch.float32)), (n, scale)


@pytest.mark.parametrize("n", [1030, 4096])
@pytest.mark.parametrize("raw", [True, False])
def test_rows_of_a_batch_are_independent(dev, n, raw):
    batch, _ = fill(dev, SEEDS, n, 49, 1, 0, raw=raw)
    for b, seed in enumerate(SEEDS):
        alone, _ = fill(dev, [seed], n, 49, 1, 0, raw=raw)
        assert torch.equal(batch[b:b + 1], alone), (n, raw, b)
    assert not torch.equal(batch[0], batch[1])


def test_rows_off_a_16_byte_boundary_take_the_scalar_path_with_the_same_bits(dev):
    """n % 4 == 0 but the base pointer is 4 bytes past a 16-byte boundary: no row starts aligned, so no quad store may be used."""
    from geo4d_amd import ops
    n, seeds = 4096, seeds_dev(SEEDS, dev)
    for raw, sent in ((True, I_SENT), (False, F_SENT)):
        aligned, _ = fill(dev, SEEDS, n, 7, 1, 2, raw=raw)
        buf = torch.full((3 * n + PAD,), sent, device=dev, dtype=aligned.dtype)
        out = buf[1:1 + 3 * n].view(3, n)
        assert out.data_ptr() % 16 == 4
        ops.philox_fill(out, seeds, step=7, stream_id=1, draw=2, raw=raw)
        assert torch.equal(out, aligned) and buf[0].item() == sent and bool((buf[1 + 3 * n:] == sent).all())


# the coefficient table of test_entrypoints_gpu.py::test_ddim_step_grid_stride: the row in use sits between rows that would be visibly wrong
COEF = [[1e3] * 6, [-5.0] * 6, [0.6, 0.8, 0.9, 0.7, 0.5, 0.1], [0.0] * 6, [7.0] * 6]


@pytest.mark.parametrize("n", [1030, 16 * 4 * 8 * 8])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("with_x0", [True, False])
def test_fused_step_equals_fill_then_ddim_step(dev, n, B, with_x0):
    from geo4d_amd import ops
    gen = torch.Generator().manual_seed(n + B)
    seeds, draw, scale = seeds_dev(SEEDS[:B], dev), 2, 0.9
    coef = torch.tensor(COEF, device=dev)
    idx = torch.tensor([2], device=dev, dtype=torch.int32)
    x_init, v = torch.randn((B, n), generator=gen).to(dev), torch.randn((B, n), generator=gen).to(dev)

    def padded():
        xb, pb = torch.full((B * n + PAD,), F_SENT, device=dev), torch.full((B * n + PAD,), F_SENT, device=dev)
        xb[:B * n] = x_init.reshape(-1)
        return xb, pb, xb[:B * n].view(B, n), (pb[:B * n].view(B, n) if with_x0 else None)
    xb1, pb1, x1, p1 = padded()
    ops.ddim_step_rng(x1, v, coef, idx, seeds, draw=draw, noise_scale=scale, pred_x0=p1)
    xb2, pb2, x2, p2 = padded()
    nz = torch.empty((B, n), device=dev)
    ops.philox_fill(nz, seeds, step=idx, stream_id=ops.NOISE_STREAM_STEP, draw=draw, scale=scale)
    ops.ddim_step(x2, v, coef, idx, noise=nz, pred_x0=p2)
    assert torch.equal(xb1, xb2) and torch.equal(pb1, pb2), f"fused != fill + ddim_step: {rel(x1, x2):.3e}"
    assert bool((xb1[B * n:] == F_SENT).all()) and bool((pb1[B * n:] == F_SENT).all()), "ddim_step_rng wrote past n"
    assert with_x0 or bool((pb1 == F_SENT).all())
    assert idx.item() == 2
    # and it is the update it claims to be: fp64 on the host reference's normals (ddim_step's own 2e-6 of test_entrypoints_gpu.py)
    sa, s1, rs, sp, dc, sg = COEF[2]
    z = torch.from_numpy(np.stack([host_normals(s, 1, 2, n, draw) for s in SEEDS[:B]])) * scale
    xd, vd = x_init.double().cpu(), v.double().cpu()
    p0 = (sa * xd - s1 * vd) * rs
    assert rel(x1, sp * p0 + dc * (sa * vd + s1 * xd) + sg * z) < 2e-6
    if with_x0:
        assert rel(p1, p0) < 2e-6


def test_entry_points_refuse_null_seeds_and_empty_rows_before_any_launch(dev):
    from geo4d_amd import _lib, ops
    lib = _lib.load()
    x, v = torch.full((2, 16), 3.0, device=dev), torch.ones((2, 16), device=dev)
    coef, idx, seeds = torch.tensor(COEF, device=dev), torch.tensor([2], device=dev, dtype=torch.int32), seeds_dev(SEEDS[:2], dev)
    s = ops._stream()
    for bad in (dict(seeds=None), dict(n=0), dict(n=-4), dict(B=0), dict(x=None)):
        a = dict(x=x.data_ptr(), seeds=seeds.data_ptr(), B=2, n=16)
        a.update(bad)
        with pytest.raises(RuntimeError, match="ddim_step_rng"):
            _lib.check(lib.geo4d_ddim_step_rng(a["x"], v.data_ptr(), None, coef.data_ptr(), idx.data_ptr(), a["seeds"], a["B"], a["n"], 0, 1.0, s),
                       "geo4d_ddim_step_rng")
        with pytest.raises(RuntimeError, match="philox_fill"):
            _lib.check(lib.geo4d_philox_fill(a["x"], 0, a["seeds"], a["B"], a["n"], None, 0, 1, 0, 1.0, s), "geo4d_philox_fill")
    with pytest.raises(RuntimeError, match="philox_fill"):
        _lib.check(lib.geo4d_philox_fill(x.data_ptr(), 2, seeds.data_ptr(), 2, 16, None, 0, 1, 0, 1.0, s), "geo4d_philox_fill")   # unknown kind
    assert bool((x == 3.0).all())


def test_seeded_stochastic_ddim_matches_oracle_and_is_captured(dev):
    """eta = 1 with noise_seeds: the step noise of ddim index k is philox_normal_host(seed, 1, k), so the oracle loop (pinned to the
    reference at eta = 1 by tests/golden/ddim_eta_tiny.pt) can be fed the same noise in the order the indices are visited; the captured
    run (one capture, S - 1 replays) and the eager run agree bit for bit."""
    from geo4d_amd.ddim import DDIMSampler
    g = load("ddim_eta_tiny.pt")
    m, u, _ = _diffusion(dev, "f32")
    size, S, seed = tuple(g["x_T"].shape), g["S"], 20240229
    cond = {"c_crossattn": [g["context"].to(dev)], "c_concat": [g["c_concat"].to(dev)]}
    kw = dict(S=S, conditioning=cond, batch_size=1, shape=list(size[1:]), verbose=False, eta=g["eta"], unconditional_guidance_scale=1.0,
              unconditional_conditioning=None, fs=g["fs"].to(dev), x_T=g["x_T"].to(dev), timestep_spacing="uniform_trailing",
              guidance_rescale=0.7, noise_seeds=[seed])
    captured, eager = DDIMSampler(m, use_graph=True), DDIMSampler(m, use_graph=False)
    out_g, _ = captured.sample(**kw)
    out_e, _ = eager.sample(**kw)
    assert captured._static is not None and captured._static["g"] is not None, "the eta > 0 step was not captured"
    assert eager._static is None
    assert torch.equal(out_g, out_e)
    out_r, _ = captured.sample(**dict(kw, noise_seeds=torch.tensor([seed])))      # replays the captured graph; seeds as a tensor
    assert torch.equal(out_r, out_g)
    usd = seeded_state_dict(u["shapes"])
    visited = iter(range(S - 1, -1, -1))

    def apply_model(x, t):
        return ounet.unet_forward(usd, g["unet_config"], torch.cat([x, g["c_concat"]], 1), t, g["context"], g["fs"])
    ref = oddim.ddim_sample(apply_model, oddim.make_schedule(), oddim.make_scale_arr(), S, g["x_T"], eta=g["eta"],
                            noise_fn=lambda shape: torch.from_numpy(noise.philox_normal_host(seed, noise.STREAM_STEP, next(visited),
                                                                                             int(np.prod(shape[1:])))).float().reshape(shape))
    e = rel(out_g, ref)
    print(f"[ddim eta=1, device noise from noise_seeds] rel_l2 vs oracle = {e:.3e}")
    assert e < 2e-4
    assert not torch.equal(captured.sample(**dict(kw, noise_seeds=[seed + 1]))[0], out_g)
    with pytest.raises(ValueError):
        eager.sample(**dict(kw, strict_rng=True))
    # x_T from the generator's stream 0 when none is passed
    out_x, inter = eager.sample(**dict(kw, x_T=None))
    x_T = torch.from_numpy(noise.philox_normal_host(seed, noise.STREAM_XT, 0, int(np.prod(size[1:])))).reshape(size)
    assert (inter["x_inter"][0].double().cpu() - x_T).abs().max().item() <= 2e-6 * noise.MAX_ABS_NORMAL and torch.isfinite(out_x).all()


@pytest.mark.parametrize("mode,tol", [("f32", 2e-5), ("bf16x3", 2e-4)])
def test_run_clip_device_noise_window_batch_matches_one_window_at_a_time(dev, mode, tol):
    """eta = 1 with step_noise="device": the noise of a window is bit-identical whether it is denoised alone or as a row of a batch, so
    window_batch = 2 differs from 1 only by what test_run_clip_window_batch_matches_one_window_at_a_time already bounds at eta = 0 (GEMM
    tile choice follows M); its clip, its tolerances."""
    from geo4d_amd.pipeline import run_clip
    m, u, _ = _diffusion(dev, mode)
    gen = torch.Generator().manual_seed(18)
    video = (torch.rand((1, 3, 22, 64, 64), generator=gen) * 2 - 1).to(dev)
    ctx = torch.randn((1, 77 + 16 * 16, u["unet_config"]["context_dim"]), generator=gen).to(dev)
    kw = dict(ddim_steps=3, ddim_eta=1.0, step_noise="device")
    slices, one = run_clip(m, video, ctx, window_batch=1, seed=77, **kw)
    _, two = run_clip(m, video, ctx, window_batch=2, seed=77, **kw)
    assert [(s.start, s.stop) for s in slices] == [(0, 16), (4, 20), (6, 22)] and one.shape == two.shape == (3, 11, 16, 64, 64)
    errs = [rel(two[i], one[i]) for i in range(3)]
    print(f"[run_clip eta 1 device noise, window_batch 2 vs 1] mode={mode} per-window rel_l2 {['%.2e' % e for e in errs]} (tol {tol:.0e})")
    assert max(errs) < tol and torch.isfinite(two).all()
    _, other = run_clip(m, video, ctx, window_batch=2, seed=78, **kw)
    assert not any(torch.equal(other[i], two[i]) for i in range(3))
    with pytest.raises(ValueError):
        run_clip(m, video, ctx, **dict(kw, step_noise="host"))


def test_guided_synthesis_builds_its_unconditional_conditioning(dev):
    """CFG 7.5, eta 1, device noise, straight from the script's arguments: image_guided_synthesis builds cond AND the unconditional dicts
    (test_geo4d.py:171-197) and equals the same call given all of them assembled by hand - 2-way and 3-way (multiple_cond_cfg)."""
    from geo4d_amd.diffusion import LatentVisualDiffusion
    from geo4d_amd.pipeline import image_guided_synthesis
    from geo4d_amd.tokenizer import SimpleTokenizer
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    u = torch.load(os.path.join(G, "unet_tiny.pt"), weights_only=False)
    v = torch.load(os.path.join(G, "vae_tiny.pt"), weights_only=False)
    cd = u["unet_config"]["context_dim"]
    vae_cfg = {"target": "geo4d_amd.vae.AutoencoderKL", "params": dict(ddconfig=v["ddconfig"], lossconfig=None, embed_dim=4,
                                                                       adaptorconfig=v["adaptorconfig"], compute_dtype="f32")}
    m = LatentVisualDiffusion(       # the tiny front-end model of test_frontend_gpu.py::test_synthesis_builds_its_own_context
        unet_config={"target": "geo4d_amd.unet.UNetModel", "params": dict(u["unet_config"], compute_dtype="f32")}, first_stage_config=vae_cfg,
        cond_stage_config={"target": "geo4d_amd.encoders.FrozenOpenCLIPEmbedder", "params": dict(layer="penultimate", width=cd, layers=2, heads=2, vocab_size=49408)},
        img_cond_stage_config={"target": "geo4d_amd.encoders.FrozenOpenCLIPImageEmbedderV2", "params": dict(width=160, layers=2, heads=2, image_size=56)},
        image_proj_stage_config={"target": "geo4d_amd.encoders.Resampler", "params": dict(dim=128, depth=1, dim_head=64, heads=2, num_queries=16,
                                                                                          embedding_dim=160, output_dim=cd, video_length=4)},
        parameterization="v", conditioning_key="hybrid", rescale_betas_zero_snr=True, linear_start=0.00085, linear_end=0.012,
        use_dynamic_rescale=True, base_scale=0.7, scale_factor=0.18215, perframe_ae=True, modality="pc_ray_cross_depth", channels=16).to(dev)
    m.cond_stage_model.tokenizer = SimpleTokenizer(merges=[])        # "a" needs a merge table: the empty one (byte symbols only) will do
    gen = torch.Generator().manual_seed(3)
    B, T = 1, 4
    videos = (torch.rand((B, 3, T, 64, 64), generator=gen) * 2 - 1).to(dev)
    shape = [B, 16, T, 8, 8]
    kw = dict(n_samples=1, ddim_steps=3, ddim_eta=1.0, fs=24, timestep_spacing="uniform_trailing", guidance_rescale=0.7,
              unconditional_guidance_scale=7.5, noise_seeds=[5], text_input=True)

    def run(**extra):
        torch.manual_seed(5)                     # the VAE encode's posterior sampling
        return image_guided_synthesis(m, ["a"], videos, shape, **dict(kw, **extra))
    ctx = m.context_for(["a"], image=videos[:, :, 0])
    uc_emb = m.get_learned_conditioning([""])
    assert not torch.equal(uc_emb, ctx[:, :uc_emb.shape[1]])         # the prompt is not blanked
    uc_img_emb = m.image_proj_model(m.embedder(torch.zeros_like(videos[:, :, 0])))
    by_hand = dict(cond={"c_crossattn": [ctx]}, unconditional_conditioning={"c_crossattn": [torch.cat([uc_emb, uc_img_emb], 1)]})
    a, b = run(), run(**by_hand)
    assert a.shape == (B, 1, 11, T, 64, 64) and torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, run(unconditional_guidance_scale=1.0 + 1e-3))          # guidance is on
    uc_2 = {"c_crossattn": [torch.cat([uc_emb, ctx[:, uc_emb.shape[1]:]], 1)]}
    a3 = run(multiple_cond_cfg=True, cfg_img=2.0)
    b3 = run(multiple_cond_cfg=True, cfg_img=2.0, unconditional_conditioning_img_nonetext=uc_2, **by_hand)
    assert torch.isfinite(a3).all() and torch.equal(a3, b3) and not torch.equal(a3, a)
    # two variants: noise_draw = 0, 1 -> different samples, the first equal to the single-variant run
    two = run(n_samples=2)
    assert torch.equal(two[:, 0], a[:, 0]) and not torch.equal(two[:, 1], two[:, 0])
    # what still cannot be served: a caller-supplied cond with guidance on and no unconditional dicts
    with pytest.raises(NotImplementedError):
        run(cond={"c_crossattn": [ctx]})
    with pytest.raises(NotImplementedError):
        run(multiple_cond_cfg=True, cfg_img=2.0, **by_hand)
