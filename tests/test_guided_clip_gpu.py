"""Classifier-free guidance for whole clips on the device: run_clip(window_batch = 2) under 2-way / 3-way guidance, at eta 0 and at eta 1 with
device noise, against one window at a time; the unconditional contexts run_clip builds itself; replay determinism; the sampler's row check.

Tolerance of "k windows batched == one at a time" under guidance scale s. The guided output is s e_c - (s - 1) e_u (3-way with cfg_img = s:
the same two weights), so a per-evaluation discrepancy eps grows to at most (2 s - 1) eps. eps per mode is the bound of the unguided
tests/test_parity_gpu.py::test_run_clip_window_batch_matches_one_window_at_a_time (f32 2e-5, bf16x3 2e-4, bf16x3m 1e-3): at s = 2 the bounds
are 6e-5 / 6e-4 / 3e-3, and f32 at s = 7.5 gets 14 x 2e-5 = 2.8e-4. Conditional and unconditional contexts are random and DIFFERENT per
window, so a row mix-up is an O(1) error."""
import os

import pytest
import torch

from oracle.params import seeded_state_dict

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = {"f32": 2e-5, "bf16x3": 2e-4, "bf16x3m": 1e-3}
STARTS = (0, 4, 6)              # 22 frames: windows (0,16) (4,20) (6,22)


def load(name):
    return torch.load(os.path.join(G, name), weights_only=False)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _diffusion(dev, mode, frontend=False):
    """The tiny LatentVisualDiffusion of tests/test_parity_gpu.py; ``frontend``: with the tiny encoders of tests/test_frontend_gpu.py (T = 16)."""
    from geo4d_amd.diffusion import LatentVisualDiffusion
    u, v = load("unet_tiny.pt"), load("vae_tiny.pt")
    cd = u["unet_config"]["context_dim"]
    extra = {}
    if frontend:
        extra = dict(
            cond_stage_config={"target": "geo4d_amd.encoders.FrozenOpenCLIPEmbedder", "params": dict(layer="penultimate", width=cd, layers=2, heads=2, vocab_size=49408)},
            img_cond_stage_config={"target": "geo4d_amd.encoders.FrozenOpenCLIPImageEmbedderV2", "params": dict(width=160, layers=2, heads=2, image_size=56)},
            image_proj_stage_config={"target": "geo4d_amd.encoders.Resampler", "params": dict(dim=128, depth=1, dim_head=64, heads=2, num_queries=16,
                                                                                              embedding_dim=160, output_dim=cd, video_length=16)})
    vae_cfg = {"target": "geo4d_amd.vae.AutoencoderKL",
               "params": dict(ddconfig=v["ddconfig"], lossconfig={"target": "torch.nn.Identity"}, embed_dim=4,
                              adaptorconfig=v["adaptorconfig"], compute_dtype=mode)}
    m = LatentVisualDiffusion(unet_config={"target": "geo4d_amd.unet.UNetModel", "params": dict(u["unet_config"], compute_dtype=mode)},
                              first_stage_config=vae_cfg, parameterization="v", conditioning_key="hybrid",
                              rescale_betas_zero_snr=True, linear_start=0.00085, linear_end=0.012, use_dynamic_rescale=True,
                              base_scale=0.7, scale_factor=0.18215, perframe_ae=True, modality="pc_ray_cross_depth", channels=16, **extra)
    m.model.diffusion_model.load_state_dict(seeded_state_dict(u["shapes"]), strict=True)
    m.first_stage_model.load_state_dict(seeded_state_dict(v["shapes"]), strict=True)
    return m.to(dev), cd


@pytest.fixture(scope="module")
def rig(dev):
    """Per mode: the model, the 22-frame 64x64 clip and three per-window-distinct context callables (conditional, unconditional, image-only)."""
    built = {}

    def get(mode):
        if mode not in built:
            m, cd = _diffusion(dev, mode)
            gen = torch.Generator().manual_seed(18)
            video = (torch.rand((1, 3, 22, 64, 64), generator=gen) * 2 - 1).to(dev)
            first = [float(video[0, 0, s, 0, 0]) for s in STARTS]
            assert len(set(first)) == 3

            def per_window():
                table = {f: torch.randn((1, 77 + 16 * 16, cd), generator=gen).to(dev) for f in first}
                return lambda frames: table[float(frames[0, 0, 0, 0, 0])]
            built[mode] = (m, video, per_window(), per_window(), per_window())
        return built[mode]
    return get


def _compare(tag, mode, bound, one, two):
    assert one.shape == two.shape == (3, 11, 16, 64, 64)
    errs = [rel(two[i], one[i]) for i in range(3)]
    print(f"[guided run_clip window_batch 2 vs 1, {tag}] mode={mode} per-window rel_l2 {['%.2e' % e for e in errs]} (bound {bound:.1e})")
    assert torch.isfinite(two).all() and torch.isfinite(one).all()
    assert max(errs) < bound


@pytest.mark.parametrize("mode,scale", [("f32", 2.0), ("bf16x3", 2.0), ("bf16x3m", 2.0), ("f32", 7.5)])
def test_two_way_guided_window_batch_matches_one_window_at_a_time(rig, mode, scale):
    """eta 0, 2-way guidance: groups 2 + 1 (ragged last group); the cameras follow."""
    from geo4d_amd.pipeline import run_clip
    m, video, ctx, uc, _ = rig(mode)
    bound = (2 * scale - 1) * EPS[mode]
    kw = dict(ddim_steps=3, seed=77, with_cameras=True, unconditional_guidance_scale=scale, uncond_context=uc)
    slices, one, traj1 = run_clip(m, video, ctx, window_batch=1, **kw)
    _, two, traj2 = run_clip(m, video, ctx, window_batch=2, **kw)
    assert [(s.start, s.stop) for s in slices] == [(0, 16), (4, 20), (6, 22)]
    _compare(f"2-way s={scale}", mode, bound, one, two)
    assert traj2.shape == (3, 16, 4, 4) and torch.allclose(traj2, traj1, atol=50 * bound)
    if mode == "f32" and scale == 2.0:          # sensitivity: what the unconditional rows contribute is far above the bound, so wrong rows cannot pass
        _, off = run_clip(m, video, ctx, window_batch=2, ddim_steps=3, seed=77)
        gap = [rel(off[i], two[i]) for i in range(3)]
        print(f"[guided vs unguided clip] per-window rel_l2 {['%.2e' % e for e in gap]}")
        assert min(gap) > 10 * bound


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16x3m"])
def test_three_way_guided_window_batch_matches_one_window_at_a_time(rig, mode):
    from geo4d_amd.pipeline import run_clip
    m, video, ctx, uc, uc3 = rig(mode)
    scale = 2.0
    kw = dict(ddim_steps=3, seed=77, unconditional_guidance_scale=scale, multiple_cond_cfg=True, cfg_img=2.0, uncond_context=uc,
              uncond_context_img_nonetext=uc3)
    _, one = run_clip(m, video, ctx, window_batch=1, **kw)
    _, two = run_clip(m, video, ctx, window_batch=2, **kw)
    _compare("3-way s=2 cfg_img=2", mode, (2 * scale - 1) * EPS[mode], one, two)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16x3m"])
def test_guided_eta1_device_noise_window_batch_matches_one_window_at_a_time(rig, mode):
    from geo4d_amd.pipeline import run_clip
    m, video, ctx, uc, _ = rig(mode)
    scale = 2.0
    kw = dict(ddim_steps=3, ddim_eta=1.0, step_noise="device", unconditional_guidance_scale=scale, uncond_context=uc)
    _, one = run_clip(m, video, ctx, window_batch=1, seed=77, **kw)
    _, two = run_clip(m, video, ctx, window_batch=2, seed=77, **kw)
    _compare("2-way s=2 eta 1 device noise", mode, (2 * scale - 1) * EPS[mode], one, two)
    _, other = run_clip(m, video, ctx, window_batch=2, seed=78, **kw)
    assert not any(torch.equal(other[i], two[i]) for i in range(3))


def test_guided_clip_is_deterministic_across_calls(rig):
    """A second call with the same arguments replays the sampler's captured step (one window at a time: the first window of the second call
    finds the graph the last window of the first call left) and gives the same bits; so does the batched form."""
    from geo4d_amd.ddim import DDIMSampler
    from geo4d_amd.pipeline import run_clip
    m, video, ctx, uc, _ = rig("f32")
    kw = dict(ddim_steps=3, seed=77, unconditional_guidance_scale=2.0, uncond_context=uc)
    _, a1 = run_clip(m, video, ctx, window_batch=1, **kw)
    sampler = m.__dict__["_geo4d_samplers"][DDIMSampler]
    graph = sampler._static["g"]
    assert graph is not None
    _, b1 = run_clip(m, video, ctx, window_batch=1, **kw)
    assert sampler._static["g"] is graph and torch.equal(a1, b1)
    _, a2 = run_clip(m, video, ctx, window_batch=2, **kw)
    _, b2 = run_clip(m, video, ctx, window_batch=2, **kw)
    assert torch.equal(a2, b2)


def test_run_clip_builds_its_unconditional_contexts(dev):
    """Nothing supplied, front-end present: run_clip builds the unconditional contexts like image_guided_synthesis does (test_geo4d.py:171-197)
    and equals the same call given them by hand - batched (callables over unconditional_contexts) and one window at a time (the 1-row dicts
    through **kwargs, today's usage)."""
    from geo4d_amd.pipeline import run_clip, unconditional_contexts
    from geo4d_amd.tokenizer import SimpleTokenizer
    m, cd = _diffusion(dev, "f32", frontend=True)
    m.cond_stage_model.tokenizer = SimpleTokenizer(merges=[])
    gen = torch.Generator().manual_seed(18)
    video = (torch.rand((1, 3, 22, 64, 64), generator=gen) * 2 - 1).to(dev)
    ctx = lambda frames: m.context_for(["a"], image=frames[:, :, 0])
    kw = dict(ddim_steps=3, seed=77, prompts=("a",), unconditional_guidance_scale=7.5, multiple_cond_cfg=True, cfg_img=2.0)
    _, built2 = run_clip(m, video, ctx, window_batch=2, **kw)
    _, hand2 = run_clip(m, video, ctx, window_batch=2, uncond_context=lambda f: unconditional_contexts(m, ctx(f), f)[0],
                        uncond_context_img_nonetext=lambda f: unconditional_contexts(m, ctx(f), f)[1], **kw)
    assert built2.shape == (3, 11, 16, 64, 64) and torch.isfinite(built2).all() and torch.equal(built2, hand2)
    _, built1 = run_clip(m, video, ctx, window_batch=1, **kw)
    c = ctx(video[:, :, :16])
    uc_emb = m.get_learned_conditioning([""])
    assert not torch.equal(uc_emb, c[:, :uc_emb.shape[1]])            # the prompt is not blank
    uc_img_emb = m.image_proj_model(m.embedder(torch.zeros_like(video[:, :, 0])))
    _, hand1 = run_clip(m, video, ctx, window_batch=1, unconditional_conditioning={"c_crossattn": [torch.cat([uc_emb, uc_img_emb], 1)]},
                        unconditional_conditioning_img_nonetext={"c_crossattn": [torch.cat([uc_emb, c[:, uc_emb.shape[1]:]], 1)]}, **kw)
    assert torch.equal(built1, hand1)
    errs = [rel(built2[i], built1[i]) for i in range(3)]
    print(f"[run_clip builds its unconditional contexts] window_batch 2 vs 1, f32, 3-way s=7.5: per-window rel_l2 {['%.2e' % e for e in errs]}")
    _, two_way = run_clip(m, video, ctx, window_batch=2, **dict(kw, multiple_cond_cfg=False))
    assert not torch.equal(two_way, built2)


def test_sampler_refuses_mismatched_rows_on_the_device(rig, dev):
    from geo4d_amd.ddim import DDIMSampler
    m, video, ctx, uc, _ = rig("f32")
    c2 = torch.cat([ctx(video[:, :, s:s + 16]) for s in (0, 4)], 0)
    z = torch.zeros((2, 4, 16, 8, 8), device=dev)
    s = DDIMSampler(m)
    with pytest.raises(ValueError) as e:
        s.sample(S=3, batch_size=2, shape=[16, 16, 8, 8], conditioning={"c_crossattn": [c2], "c_concat": [z]}, verbose=False, eta=0.0,
                 unconditional_guidance_scale=2.0, unconditional_conditioning={"c_crossattn": [uc(video[:, :, :16])], "c_concat": [z]},
                 fs=torch.tensor([24, 24], device=dev), x_T=torch.zeros((2, 16, 16, 8, 8), device=dev), timestep_spacing="uniform_trailing",
                 guidance_rescale=0.7)
    assert "unconditional_conditioning['c_crossattn'] has 1 rows, batch_size is 2" in str(e.value)
    assert s._static is None and not hasattr(s, "coef")              # refused before any buffer or table was built: nothing launched
