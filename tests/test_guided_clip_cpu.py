"""Classifier-free guidance through run_clip, host side (no GPU): the unconditional conditioning dicts carry one row per window of a
batch, 1-row inputs are repeated, callables are evaluated per window; guidance off changes nothing; the front-end helper
unconditional_contexts restates test_geo4d.py:171-195; the sampler refuses a guidance dict whose row count is not the batch's."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

L_CTX, D_CTX = 333, 8          # 77 text + 16 x 16 image tokens


# ---- stubs: the model of tests/test_device_noise_cpu.py restated, and a synthesize that records what it was handed ---------------------
class _StubModel:
    class model:
        conditioning_key = "hybrid"

        class diffusion_model:
            out_channels = 16

    @staticmethod
    def encode_first_stage(videos):
        b, _, t, H, W = videos.shape
        return videos.mean(dim=1, keepdim=True).expand(b, 4, t, H, W)[..., ::8, ::8] + torch.randn((b, 4, t, H // 8, W // 8))


UC, UC3 = "unconditional_conditioning", "unconditional_conditioning_img_nonetext"


def _stub_decoder(model, samples, pointmap_vae=None):
    b, _, t, h, w = samples.shape
    return samples.mean(dim=(1, 3, 4)).reshape(b, 1, t, 1, 1).expand(b, 11, t, 8 * h, 8 * w).contiguous()


def _rows_synth(calls=None):
    """Sample-wise like the real sampler: row b depends on window b's frames, noise, video latent and on row b of EVERY conditioning dict."""
    def synth(model, prompts, videos, noise_shape, n_samples=1, x_T=None, cond=None, decode=True, **kw):
        if calls is not None:
            calls.append(dict(kw, batch=noise_shape[0], cond=cond))
        B, _, T, h, w = noise_shape
        if "c_concat" not in cond:
            cond = dict(cond, c_concat=[model.encode_first_stage(videos)])
        assert videos.shape[0] == B and x_T.shape[0] == B and cond["c_crossattn"][0].shape[0] == B and cond["c_concat"][0].shape[0] == B
        per = x_T.mean(dim=(1, 2, 3, 4)) + cond["c_crossattn"][0].mean(dim=(1, 2)) + cond["c_concat"][0].mean(dim=(1, 2, 3, 4))
        if kw.get("unconditional_guidance_scale", 1.0) != 1.0:
            for j, name in enumerate((UC, UC3)):
                if kw.get(name) is not None:
                    u = kw[name]["c_crossattn"][0]
                    assert u.shape[0] == B, (name, tuple(u.shape), B)
                    per = per + (3.0 + 2.0 * j) * u.mean(dim=(1, 2))
        lat = torch.zeros((B, 16, T, h, w)) + videos.mean(dim=(1, 3, 4)).reshape(B, 1, T, 1, 1) + per.reshape(B, 1, 1, 1, 1)
        return (_stub_decoder(model, lat) if decode else lat)[:, None]
    return synth


def _video():
    return torch.arange(1 * 3 * 22 * 16 * 16, dtype=torch.float32).reshape(1, 3, 22, 16, 16) / 1e4      # windows (0,16) (4,20) (6,22)


FIRST = [float(_video()[0, 0, s, 0, 0]) for s in (0, 4, 6)]       # the first frame's first pixel of each window


def _frame_code(offset):
    """A context callable whose every element encodes the window's first frame (+ offset): tells windows AND dicts apart."""
    return lambda frames: torch.full((1, L_CTX, D_CTX), float(frames[0, 0, 0, 0, 0]) + offset)


def _clip(model=_StubModel, **kw):
    from geo4d_amd.pipeline import run_clip
    calls = []
    slices, maps = run_clip(model, _video(), torch.ones((1, L_CTX, D_CTX)), ddim_steps=2, synthesize=_rows_synth(calls), seed=123, **kw)
    assert [(s.start, s.stop) for s in slices] == [(0, 16), (4, 20), (6, 22)] and maps.shape == (3, 11, 16, 16, 16)
    return calls, maps


def _rows_of(d):
    return [t.shape[0] for v in d.values() for t in (v if isinstance(v, (list, tuple)) else [v])]


# ---- batched guided rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("three_way", [False, True])
def test_guided_window_batch_hands_one_row_per_window_to_every_dict(three_way):
    kw = dict(unconditional_guidance_scale=7.5, uncond_context=_frame_code(100.0))
    if three_way:
        kw.update(multiple_cond_cfg=True, cfg_img=2.0, uncond_context_img_nonetext=_frame_code(200.0))
    calls, two = _clip(window_batch=2, **kw)
    assert [c["batch"] for c in calls] == [2, 1]
    groups = [[0, 1], [2]]
    for c, wis in zip(calls, groups):
        names = [UC] + ([UC3] if three_way else [])
        for d in [c["cond"]] + [c[n] for n in names]:
            assert isinstance(d, dict) and set(_rows_of(d)) == {c["batch"]}
        for name, off in zip(names, (100.0, 200.0)):
            u = c[name]["c_crossattn"][0]
            assert u.shape == (len(wis), L_CTX, D_CTX)
            for j, wi in enumerate(wis):                 # row j belongs to window j of the group
                assert torch.equal(u[j], torch.full((L_CTX, D_CTX), FIRST[wi] + off)), (name, j, wi)
        if not three_way:
            assert c.get(UC3) is None
    calls1, one = _clip(window_batch=1, **kw)
    assert [c["batch"] for c in calls1] == [1, 1, 1]
    assert torch.equal(one, two) and len({float(one[i].mean()) for i in range(3)}) == 3
    _, off = _clip(window_batch=2)
    assert not torch.equal(off, two)                     # the stub does look at the unconditional rows


# ---- 1-row inputs are repeated -----------------------------------------------------------------------------------------------------------------
def test_one_row_tensor_and_one_row_dict_are_repeated_to_the_batch():
    t = torch.arange(L_CTX * D_CTX, dtype=torch.float32).reshape(1, L_CTX, D_CTX) / 100
    calls_t, maps_t = _clip(window_batch=2, unconditional_guidance_scale=7.5, uncond_context=t)
    uc = {"c_crossattn": [t.clone()]}
    uc3 = {"c_crossattn": [t.clone() + 1]}
    calls_d, maps_d = _clip(window_batch=2, unconditional_guidance_scale=7.5, multiple_cond_cfg=True, cfg_img=2.0,
                            **{UC: uc, UC3: uc3})
    for calls in (calls_t, calls_d):
        assert [c["batch"] for c in calls] == [2, 1]
        for c in calls:
            got = c[UC]["c_crossattn"][0]
            assert got.shape == (c["batch"], L_CTX, D_CTX) and all(torch.equal(got[j], t[0]) for j in range(c["batch"]))
    for c in calls_d:
        got = c[UC3]["c_crossattn"][0]
        assert got.shape == (c["batch"], L_CTX, D_CTX) and all(torch.equal(got[j], t[0] + 1) for j in range(c["batch"]))
    assert uc["c_crossattn"][0].shape == (1, L_CTX, D_CTX)           # the caller's dict is not modified
    # one window at a time: the dict reaches synthesize unchanged
    calls_1, maps_1 = _clip(window_batch=1, unconditional_guidance_scale=7.5, multiple_cond_cfg=True, cfg_img=2.0, **{UC: uc, UC3: uc3})
    assert [c["batch"] for c in calls_1] == [1, 1, 1]
    for c in calls_1:
        assert set(c[UC]) == {"c_crossattn"} and torch.equal(c[UC]["c_crossattn"][0], uc["c_crossattn"][0])
        assert set(c[UC3]) == {"c_crossattn"} and torch.equal(c[UC3]["c_crossattn"][0], uc3["c_crossattn"][0])
    assert torch.equal(maps_1, maps_d)
    # both forms at once, and a row count that is neither 1 nor the batch's, are refused
    with pytest.raises(ValueError):
        _clip(unconditional_guidance_scale=7.5, uncond_context=t, **{UC: uc})
    with pytest.raises(ValueError):
        _clip(window_batch=2, unconditional_guidance_scale=7.5, uncond_context=t.repeat(3, 1, 1))


# ---- guidance off ----------------------------------------------------------------------------------------------------------------------------
def test_guidance_off_adds_no_keys_and_changes_nothing():
    calls1, maps1 = _clip(window_batch=1)
    calls2, maps2 = _clip(window_batch=2)
    assert [c["batch"] for c in calls1] == [1, 1, 1] and [c["batch"] for c in calls2] == [2, 1]
    assert all(UC not in c and UC3 not in c and set(c["cond"]) <= {"c_crossattn", "c_concat"} for c in calls1 + calls2)
    assert torch.equal(maps1, maps2)
    # the context arguments are not looked at with guidance off (scale 1.0 is the default)
    calls3, maps3 = _clip(window_batch=2, uncond_context=_frame_code(100.0), uncond_context_img_nonetext=_frame_code(200.0))
    assert all(UC not in c and UC3 not in c for c in calls3) and torch.equal(maps3, maps2)
    assert [sorted(c) for c in calls3] == [sorted(c) for c in calls2]


# ---- nothing to build the unconditional contexts from -----------------------------------------------------------------------------------------
def test_guidance_without_unconditional_inputs_or_front_end_is_refused_before_any_synthesis():
    from geo4d_amd.pipeline import run_clip
    calls = []
    for extra in ({}, dict(multiple_cond_cfg=True, cfg_img=2.0, uncond_context=torch.zeros((1, L_CTX, D_CTX)))):
        with pytest.raises(ValueError) as e:
            run_clip(_StubModel, _video(), torch.ones((1, L_CTX, D_CTX)), ddim_steps=2, synthesize=_rows_synth(calls), seed=123, window_batch=2,
                     unconditional_guidance_scale=7.5, **extra)
        assert "uncond_context" in str(e.value) and "uncond_context_img_nonetext" in str(e.value)
    assert calls == []


# ---- the front-end helper ------------------------------------------------------------------------------------------------------------------------
class _FrontEnd(_StubModel):
    """Fixed fake encoders: n_img image tokens per sample (per frame under cross_attention), n_text text tokens."""
    cross_attention = False
    uncond_type = "empty_seq"
    n_text, n_img, width = 3, 5, 4

    def __init__(self):
        self.seen = []

    def embedder(self, img):
        self.seen.append(("embedder", tuple(img.shape), float(img.abs().sum())))
        return torch.full((img.shape[0], 2, 6), 0.25) + img.mean(dim=(1, 2, 3)).reshape(-1, 1, 1)

    def image_proj_model(self, emb):
        self.seen.append(("image_proj_model", tuple(emb.shape)))
        ramp = torch.arange(self.n_img, dtype=torch.float32).reshape(1, -1, 1)
        if emb.dim() == 4:                      # per-frame tokens [b, t, l, c] -> [b, t * n_img, width]
            b, t = emb.shape[:2]
            return (emb.mean(dim=(2, 3)).reshape(b, t, 1, 1) + ramp.reshape(1, 1, -1, 1)).expand(b, t, self.n_img, self.width).reshape(b, -1, self.width)
        return emb.mean(dim=(1, 2)).reshape(-1, 1, 1).expand(emb.shape[0], self.n_img, self.width) + ramp

    def get_learned_conditioning(self, prompts):
        self.seen.append(("text", list(prompts)))
        return torch.stack([torch.full((self.n_text, self.width), 7.0 + len(p)) for p in prompts])


def test_unconditional_contexts_on_a_stub_front_end():
    from geo4d_amd.pipeline import unconditional_contexts, unconditional_parts
    m = _FrontEnd()
    B = 2
    videos = torch.rand((B, 3, 4, 8, 8), generator=torch.Generator().manual_seed(1)) + 1.0
    ctx = torch.randn((B, m.n_text + m.n_img, m.width), generator=torch.Generator().manual_seed(2))
    uc_img = torch.full((B, m.n_img, m.width), 0.25) + torch.arange(m.n_img, dtype=torch.float32).reshape(1, -1, 1)   # the zero image's tokens
    uc, uc3 = unconditional_contexts(m, ctx, videos)
    text = torch.full((B, m.n_text, m.width), 7.0)                                     # "" has length 0
    assert torch.equal(uc, torch.cat([text, uc_img], 1))                                # test_geo4d.py:172-184
    assert torch.equal(uc3, torch.cat([text, ctx[:, m.n_text:]], 1))                    # :192, the CONDITIONAL image tokens
    assert ("text", [""] * B) in m.seen and ("embedder", (B, 3, 8, 8), 0.0) in m.seen   # one ZERO image per sample, "" per sample
    m.uncond_type = "zero_embed"
    m.seen.clear()
    uc, uc3 = unconditional_contexts(m, ctx, videos)
    assert torch.equal(uc, torch.cat([torch.zeros_like(text), uc_img], 1))              # :175-176
    assert torch.equal(uc3, torch.cat([torch.zeros_like(text), ctx[:, m.n_text:]], 1))
    assert not any(s[0] == "text" for s in m.seen)
    # the pieces that do not depend on the window can be computed once and reused
    parts = unconditional_parts(m, ctx, videos)
    m.seen.clear()
    again = unconditional_contexts(m, ctx, videos, parts=parts)
    assert m.seen == [] and torch.equal(again[0], uc) and torch.equal(again[1], uc3)
    m.uncond_type = "learned"
    with pytest.raises(NotImplementedError):
        unconditional_contexts(m, ctx, videos)
    # cross_attention: every frame's ZERO image goes through the embedder, tokens per frame
    m.uncond_type, m.cross_attention = "empty_seq", True
    m.seen.clear()
    ctx_x = torch.randn((B, m.n_text + m.n_img * 4, m.width))
    uc, uc3 = unconditional_contexts(m, ctx_x, videos)
    assert ("embedder", (B * 4, 3, 8, 8), 0.0) in m.seen and ("image_proj_model", (B, 4, 2, 6)) in m.seen
    assert uc.shape == ctx_x.shape and torch.equal(uc3[:, m.n_text:], ctx_x[:, m.n_text:]) and torch.equal(uc[:, :m.n_text], text)


def test_run_clip_builds_the_unconditional_contexts_once_per_clip_from_the_front_end():
    """cross_attention False: "" and the zero image do not depend on the window - ONE pass through the fake encoders per clip; the third
    context carries each window's own conditional image tokens."""
    from geo4d_amd.pipeline import run_clip, unconditional_contexts

    class M(_FrontEnd):
        n_text, n_img, width = 77, 256, D_CTX
    m = M()
    ctx_fn = lambda frames: torch.full((1, L_CTX, D_CTX), float(frames[0, 0, 0, 0, 0]))
    calls = []
    run_clip(m, _video(), ctx_fn, ddim_steps=2, synthesize=_rows_synth(calls), seed=123, window_batch=2, unconditional_guidance_scale=7.5,
             multiple_cond_cfg=True, cfg_img=2.0)
    assert [s[0] for s in m.seen] == ["embedder", "image_proj_model", "text"]
    assert [c["batch"] for c in calls] == [2, 1]
    for c, wis in zip(calls, [[0, 1], [2]]):
        for j, wi in enumerate(wis):
            ctx = torch.full((1, L_CTX, D_CTX), FIRST[wi])
            uc, uc3 = unconditional_contexts(M(), ctx, _video()[:, :, :16])
            assert torch.equal(c[UC]["c_crossattn"][0][j:j + 1], uc) and torch.equal(c[UC3]["c_crossattn"][0][j:j + 1], uc3)
            assert torch.equal(c[UC3]["c_crossattn"][0][j, 77:], ctx[0, 77:])


# ---- the sampler refuses mismatched rows -------------------------------------------------------------------------------------------------------
class _SamplerStub:
    num_timesteps = 1000
    parameterization = "v"
    device = torch.device("cpu")
    applied = 0

    def apply_model(self, *a, **k):
        type(self).applied += 1
        raise AssertionError("apply_model must not be reached")


@pytest.mark.parametrize("multicond", [False, True])
def test_sampler_refuses_a_guidance_dict_with_the_wrong_row_count(multicond):
    from geo4d_amd.ddim import DDIMSampler
    from geo4d_amd.ddim_multiplecond import DDIMSampler as Multi
    s = (Multi if multicond else DDIMSampler)(_SamplerStub())
    mk = lambda rows: {"c_crossattn": [torch.zeros((rows, 13, 4))], "c_concat": [torch.zeros((rows, 4, 2, 2, 2))]}
    kw = dict(S=3, batch_size=2, shape=[16, 2, 2, 2], conditioning=mk(2), verbose=False, unconditional_guidance_scale=7.5, eta=0.0,
              fs=torch.tensor([24, 24]), x_T=torch.zeros((2, 16, 2, 2, 2)))
    with pytest.raises(ValueError) as e:
        s.sample(unconditional_conditioning=mk(1), unconditional_conditioning_img_nonetext=mk(2) if multicond else None, **kw)
    assert "unconditional_conditioning['c_crossattn']" in str(e.value) and "1 rows" in str(e.value) and "batch_size is 2" in str(e.value)
    if multicond:
        with pytest.raises(ValueError) as e:
            s.sample(unconditional_conditioning=mk(2), unconditional_conditioning_img_nonetext={"c_crossattn": [torch.zeros((2, 13, 4))],
                                                                                                "c_concat": [torch.zeros((3, 4, 2, 2, 2))]}, **kw)
        assert "unconditional_conditioning_img_nonetext['c_concat']" in str(e.value) and "3 rows" in str(e.value)
    assert _SamplerStub.applied == 0 and s._static is None and not hasattr(s, "coef")       # nothing was built


# ---- two gloo ranks ------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _guided(decode="local", window_batch=2, frames=22):
    from geo4d_amd.pipeline import run_clip
    video = torch.arange(1 * 3 * frames * 16 * 16, dtype=torch.float32).reshape(1, 3, frames, 16, 16) / 1e4       # 22 frames: 3 windows, 38: 7
    return run_clip(_StubModel, video, _frame_code(0.0), ddim_steps=2, synthesize=_rows_synth(), decode=decode, decoder=_stub_decoder,
                    window_batch=window_batch, unconditional_guidance_scale=7.5, multiple_cond_cfg=True, cfg_img=2.0,
                    uncond_context=_frame_code(100.0), uncond_context_img_nonetext=_frame_code(200.0))[1]


def _guided_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from geo4d_amd import dist as gd
    gd.init_from_env(backend="gloo")
    outs = [(f, _guided(d, 2, f).numpy()) for f in (22, 38) for d in ("local", "sharded")]
    q.put((rank, outs))                                # by value, as in tests/test_dist_cpu.py
    dist.barrier()
    dist.destroy_process_group()


def test_guided_window_batch_on_two_ranks_equals_one_rank():
    ref = {f: _guided("local", 1, f) for f in (22, 38)}
    for f, n in ((22, 3), (38, 7)):
        assert ref[f].shape == (n, 11, 16, 16, 16) and len({float(ref[f][i].mean()) for i in range(n)}) == n
        assert torch.equal(_guided("local", 2, f), ref[f]) and torch.equal(_guided("local", 3, f), ref[f])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_guided_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = [q.get(timeout=180) for _ in range(2)]
    [p.join(timeout=60) for p in procs]
    for rank, outs in res:
        assert len(outs) == 4
        for f, o in outs:
            assert torch.equal(torch.from_numpy(o), ref[f]), f"rank {rank}, {f} frames"
