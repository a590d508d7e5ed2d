"""Counter-based device noise, host side (no GPU): the numpy restatement of the generator (geo4d_amd/noise.py) against the Random123
known answers, its statistics, the prefix property, the header <-> binding tables, and the run_clip plumbing of step_noise="device"."""
import os
import re

import numpy as np
import pytest
import torch

from geo4d_amd import noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123 (Salmon et al.) known answers for philox4x32 with 10 rounds: counter, key, output
KAT = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]
words = lambda s: [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox4x32_10_known_answers(ctr, key, out):
    got = noise.philox4x32_10(words(ctr), words(key))
    assert [int(w) for w in got] == words(out)
    # the vectorised form the rest of the module uses: arrays of counters give the same words lane by lane
    arr = noise.philox4x32_10([np.full(3, w, dtype=np.uint32) for w in words(ctr)], [np.full(3, w, dtype=np.uint32) for w in words(key)])
    assert all(a.dtype == np.uint32 and a.tolist() == [w] * 3 for a, w in zip(arr, words(out)))


@pytest.fixture(scope="module")
def draws():
    """200 samples of 16384 normals: seeds 123 * 1000003 + s (run_clip's per-window seeds at seed = 123), stream 1, step s % 50."""
    return [noise.philox_normal_host(123 * 1000003 + s, noise.STREAM_STEP, s % 50, 16384) for s in range(200)]


def test_normals_have_unit_statistics_in_every_sample(draws):
    """Bounds for EVERY one of the 200 samples at n = 16384: the standard error of the mean is 1/128 = 0.0078 (0.04 = 5.1 sigma), of the
    standard deviation 1/sqrt(2 n) = 0.0055 (0.03 = 5.4 sigma); |z| <= sqrt(48 ln 2) follows from u1 >= 2^-24."""
    mean = max(abs(float(z.mean())) for z in draws)
    std = max(abs(float(z.std()) - 1.0) for z in draws)
    top = max(float(np.abs(z).max()) for z in draws)
    print(f"[philox normals, worst of 200 x 16384] |mean| {mean:.4f}  |std - 1| {std:.4f}  max |z| {top:.3f}")
    assert all(z.dtype == np.float64 and z.shape == (16384,) and np.isfinite(z).all() for z in draws)
    assert mean < 0.04 and std < 0.03 and top <= 5.768
    assert noise.MAX_ABS_NORMAL == pytest.approx(5.768, abs=1e-3)


def test_normals_are_uncorrelated_across_steps_seeds_and_neighbours():
    n, seed = 16384, 123 * 1000003
    corr = lambda a, b: abs(float(np.corrcoef(a, b)[0, 1]))
    base = noise.philox_normal_host(seed, noise.STREAM_STEP, 7, n)
    c_step = corr(base, noise.philox_normal_host(seed, noise.STREAM_STEP, 8, n))
    c_seed = corr(base, noise.philox_normal_host(seed + 1, noise.STREAM_STEP, 7, n))
    c_lag = corr(base[:-1], base[1:])
    print(f"[philox normals] |corr| two steps {c_step:.4f}  two seeds {c_seed:.4f}  lag 1 {c_lag:.4f}")
    assert max(c_step, c_seed, c_lag) < 0.03          # 1/sqrt(n) = 0.0078: 3.8 sigma
    # the other counter words separate streams as well: stream (x_T vs step noise) and draw (variant of n_samples)
    assert corr(base, noise.philox_normal_host(seed, noise.STREAM_XT, 7, n)) < 0.03
    assert corr(base, noise.philox_normal_host(seed, noise.STREAM_STEP, 7, n, draw=1)) < 0.03


def test_a_draw_is_a_prefix_of_every_longer_draw():
    long = noise.philox_normal_host(99, 1, 3, 4099, draw=2)
    wl = noise.philox_words_host(99, 1, 3, 4099, draw=2)
    for n in (1, 2, 3, 4, 5, 1030, 4096):
        assert np.array_equal(noise.philox_normal_host(99, 1, 3, n, draw=2), long[:n]), n
        assert np.array_equal(noise.philox_words_host(99, 1, 3, n, draw=2), wl[:n]), n
    assert wl.dtype == np.uint32
    # element i = word i % 4 of the call for counter (i // 4, step, stream, draw) under key (seed low, seed high)
    seed = (5 << 32) | 17
    w = noise.philox_words_host(seed, 1, 3, 12, draw=2)
    for i in (0, 5, 11):
        assert int(w[i]) == int(noise.philox4x32_10((i // 4, 3, 1, 2), (17, 5))[i % 4])
    with pytest.raises(ValueError):
        noise.philox_normal_host(1, 1, 0, 0)


def test_header_and_binding_list_the_two_entry_points():
    from geo4d_amd import _lib
    with open(os.path.join(ROOT, "include", "geo4d_hip.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(geo4d_[a-z_0-9]+)\s*\(", hdr))
    for name, nargs in (("geo4d_philox_fill", 11), ("geo4d_ddim_step_rng", 11)):
        assert name in declared and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 9     # symbols added, no struct changed


# ---- run_clip plumbing, with the stub model of tests/test_dist_cpu.py restated -------------------------------------------------------
class _StubModel:
    class model:
        conditioning_key = "hybrid"

        class diffusion_model:
            out_channels = 16

    @staticmethod
    def encode_first_stage(videos):
        b, _, t, H, W = videos.shape
        return videos.mean(dim=1, keepdim=True).expand(b, 4, t, H, W)[..., ::8, ::8] + torch.randn((b, 4, t, H // 8, W // 8))


def _recording_synth(calls):
    def synth(model, prompts, videos, noise_shape, n_samples=1, x_T=None, cond=None, decode=True, **kw):
        calls.append(dict(kw, batch=noise_shape[0]))
        B, _, T, h, w = noise_shape
        assert videos.shape[0] == B and x_T.shape[0] == B and cond["c_crossattn"][0].shape[0] == B
        return (torch.zeros((B, 11, T, 8 * h, 8 * w)) + x_T.mean(dim=(1, 2, 3, 4)).reshape(B, 1, 1, 1, 1))[:, None]
    return synth


def _clip(**kw):
    from geo4d_amd.pipeline import run_clip
    calls = []
    video = torch.arange(1 * 3 * 22 * 16 * 16, dtype=torch.float32).reshape(1, 3, 22, 16, 16) / 1e4      # 22 frames: windows (0,16) (4,20) (6,22)
    slices, maps = run_clip(_StubModel, video, torch.ones((1, 333, 8)), ddim_steps=2, synthesize=_recording_synth(calls), seed=123, **kw)
    assert len(slices) == 3 and maps.shape == (3, 11, 16, 16, 16)
    return calls, maps


def test_run_clip_device_step_noise_batches_windows_and_passes_their_seeds():
    wseed = [123 * 1000003 + wi for wi in range(3)]
    calls, maps = _clip(step_noise="device", ddim_eta=1.0, window_batch=2)
    assert [c["batch"] for c in calls] == [2, 1]
    assert [list(c["noise_seeds"]) for c in calls] == [wseed[0:2], wseed[2:3]]
    assert all("noise_generator" not in c and c["ddim_eta"] == 1.0 for c in calls)
    # a generator handed to run_clip is dropped too, and one window at a time carries the same seeds
    calls1, maps1 = _clip(step_noise="device", ddim_eta=1.0, window_batch=1, noise_generator=torch.Generator())
    assert [c["batch"] for c in calls1] == [1, 1, 1] and [list(c["noise_seeds"]) for c in calls1] == [[s] for s in wseed]
    assert all("noise_generator" not in c for c in calls1)
    assert torch.equal(maps, maps1)                 # x_T stays the per-window CPU draw


def test_run_clip_default_step_noise_is_one_window_at_a_time_without_seeds():
    calls, _ = _clip(ddim_eta=1.0, window_batch=2)
    assert [c["batch"] for c in calls] == [1, 1, 1] and all("noise_seeds" not in c for c in calls)
    calls, _ = _clip(step_noise="torch", ddim_eta=0.0, window_batch=2)       # eta = 0 batches as before, still no seeds
    assert [c["batch"] for c in calls] == [2, 1] and all("noise_seeds" not in c for c in calls)


def test_run_clip_rejects_an_unknown_step_noise():
    with pytest.raises(ValueError):
        _clip(step_noise="philox")
