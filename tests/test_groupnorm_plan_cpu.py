"""geo4d_groupnorm_plan: the pure host function that decides which launches a GroupNorm runs (norm.hip gn_plan; the launch calls the
same function, so Python and the launch cannot disagree). No GPU: the descriptors carry made-up (aligned) addresses.

  * the GroupNorms of one U-Net forward and one 4-modality decode of the headline mode (B = 1, T = 16, latent 40x64; the (HW, C, rows per
    sum entry, output format) tuples below were recorded from the engine) land where the sweep of profiles/groupnorm_one_launch.md puts
    them: per-frame statistics FUSED (one launch) at levels 1 - 3 and the middle block where the sums the launch re-reads stay small,
    the two-launch sequence at level 0 and in the VAE decoder (fusing measured slower there); across-time statistics SLICED at every
    level (fusing them measured slower than slicing, even at levels 2 - 3); a concatenated input with sums on both halves FUSED at
    levels 1 - 3 and SLICED otherwise - never the statistics pass over x;
  * the workspace the chosen path writes fits geo4d_groupnorm_workspace of the same arguments;
  * what the launch refuses the query refuses."""
import ctypes as C

import pytest

from geo4d_amd import _lib

PARTIAL, COLS, FUSED, SLICED = _lib.GN_PATH_PARTIAL, _lib.GN_PATH_COLS, _lib.GN_PATH_FUSED, _lib.GN_PATH_SLICED


def descriptor(F, HW, Cc, fps, srcs, *, dtype=_lib.F32, split_out=2, groups=32, path=0):
    q = _lib.GroupNorm2()
    p = q.base
    p.x, p.y, p.gamma, p.beta = 0x10000, 0x20000, 0x30000, 0x40000
    p.F, p.HW, p.C, p.groups, p.frames_per_stat, p.dtype, p.split_out, p.eps = F, HW, Cc, groups, fps, dtype, split_out, 1e-5
    p.ldx = p.ldy = Cc
    q.nsrc, c0 = len(srcs), 0
    for i, (rows, nc) in enumerate(srcs):
        q.src[i].colsum, q.src[i].rows, q.src[i].c0, q.src[i].channels = 0x50000 + 0x1000 * i, rows, c0, nc
        c0 += nc
    q.path = path
    return q


def plan(q):
    pl = _lib.GroupNormPlan()
    rc = _lib.load().geo4d_groupnorm_plan(C.byref(q), C.byref(pl))
    return rc, pl


# (F, HW, C, [(rows per entry, channels)], split_out) as recorded; split_out 1 = bf16 hi | lo (8 bytes per element read + written), 2 = f16 rows (6)
FUSED_4D = [(16, 640, 640, [(128, 640)], 1), (16, 640, 640, [(128, 640)], 2), (16, 640, 640, [(64, 640)], 2),
            (16, 160, 1280, [(32, 1280)], 1), (16, 160, 1280, [(32, 1280)], 2), (16, 160, 640, [(32, 640)], 2),
            (16, 40, 1280, [(8, 1280)], 1), (16, 40, 1280, [(8, 1280)], 2),
            (16, 640, 1280, [(64, 640), (64, 640)], 2), (16, 160, 1920, [(32, 1280), (32, 640)], 2), (16, 160, 2560, [(32, 1280), (32, 1280)], 2),
            (16, 40, 2560, [(8, 1280), (8, 1280)], 2)]
COLS_4D = [(16, 2560, 320, [(80, 320)], 1), (16, 2560, 320, [(80, 320)], 2), (16, 640, 320, [(32, 320)], 2), (16, 640, 640, [(32, 640)], 2),
           (16, 2560, 512, [(80, 512)], 0), (16, 2560, 512, [(80, 512)], 2), (16, 10240, 512, [(64, 512)], 2), (16, 40960, 512, [(64, 512)], 2),
           (16, 163840, 256, [(64, 256)], 2), (16, 163840, 128, [(128, 128)], 1), (16, 163840, 128, [(128, 128)], 2),
           (48, 2560, 512, [(64, 512)], 2), (48, 10240, 512, [(64, 512)], 2), (48, 40960, 512, [(64, 512)], 2), (48, 163840, 256, [(64, 256)], 2),
           (48, 163840, 128, [(128, 128)], 2)]
SLICED_4D = [(16, 2560, 640, [(80, 320), (80, 320)], 2), (16, 640, 960, [(64, 640), (32, 320)], 2)]
SLICED_5D = [(16, 2560, 320, [(80, 320)], 1), (16, 2560, 320, [(80, 320)], 2), (16, 640, 640, [(128, 640)], 2), (16, 640, 640, [(64, 640)], 1),
             (16, 160, 1280, [(32, 1280)], 1), (16, 160, 1280, [(32, 1280)], 2), (16, 40, 1280, [(8, 1280)], 2)]


def default_chunks(F, HW):
    r0 = max(4, min(1024, ((HW * F + 1023) // 1024 + 3) // 4 * 4))
    return r0, (HW + r0 - 1) // r0


@pytest.mark.parametrize("F,HW,Cc,srcs,so", FUSED_4D)
def test_per_frame_groupnorms_with_small_sums_run_one_launch(F, HW, Cc, srcs, so):
    rc, pl = plan(descriptor(F, HW, Cc, 1, srcs, split_out=so))
    assert rc == 0 and pl.path == FUSED and pl.launches == 1 and pl.workspace_bytes == 0, (pl.path, pl.rows_per_wg, pl.nchunk, pl.channel_slices)
    r0, nchunk0 = default_chunks(F, HW)
    # the launch keeps 1024 workgroups (or as many as the default chunks give); a slice is whole groups and whole 16-byte chunks
    assert F * pl.nchunk * pl.channel_slices >= min(1024, F * nchunk0)
    assert pl.rows_per_wg % 4 == 0 and pl.rows_per_wg >= r0 and pl.nchunk == (HW + pl.rows_per_wg - 1) // pl.rows_per_wg
    assert 32 % pl.channel_slices == 0 and (Cc // pl.channel_slices) % 4 == 0 and (pl.channel_slices == 1 or Cc // pl.channel_slices * 4 >= 256)
    # a workgroup's sum bytes are at most a quarter of its payload bytes, and the launch re-reads at most 12 MiB of sums
    sum_bytes = sum((HW // rows) * nc * 8 for rows, nc in srcs)
    assert sum_bytes <= 0.25 * pl.rows_per_wg * Cc * (4 + (2 if so == 2 else 4))
    assert F * pl.nchunk * sum_bytes <= 12 << 20


@pytest.mark.parametrize("F,HW,Cc,srcs,so", COLS_4D)
def test_per_frame_groupnorms_with_large_sums_keep_two_launches(F, HW, Cc, srcs, so):
    rc, pl = plan(descriptor(F, HW, Cc, 1, srcs, split_out=so))
    r0, nchunk0 = default_chunks(F, HW)
    assert rc == 0 and pl.path == COLS and pl.launches == 2 and (pl.rows_per_wg, pl.nchunk, pl.channel_slices) == (r0, nchunk0, 1)
    assert pl.workspace_bytes == _lib.load().geo4d_groupnorm_workspace(F, HW, 32, 1)


@pytest.mark.parametrize("F,HW,Cc,srcs,so", SLICED_4D)
def test_large_concatenated_inputs_are_sliced_not_re_read(F, HW, Cc, srcs, so):
    rc, pl = plan(descriptor(F, HW, Cc, 1, srcs, split_out=so))
    assert rc == 0 and pl.path == SLICED and pl.launches == 2 and pl.stat_slices == 1       # F x 32 = 512 (statistic, group) workgroups already
    assert pl.workspace_bytes == F * 32 * 16 <= _lib.load().geo4d_groupnorm_workspace(F, HW, 32, 1)


@pytest.mark.parametrize("F,HW,Cc,srcs,so", SLICED_5D)
def test_across_time_groupnorms_are_sliced(F, HW, Cc, srcs, so):
    rc, pl = plan(descriptor(F, HW, Cc, F, srcs, split_out=so))
    r0, nchunk0 = default_chunks(F, HW)
    assert rc == 0 and pl.path == SLICED and pl.launches == 2 and (pl.rows_per_wg, pl.nchunk, pl.channel_slices) == (r0, nchunk0, 1)
    assert 32 * pl.stat_slices >= 256, "at least one workgroup per CU sums the statistics"
    assert pl.workspace_bytes == 32 * pl.stat_slices * 16 <= _lib.load().geo4d_groupnorm_workspace(F, HW, 32, F)


def test_without_sums_the_statistics_pass_runs():
    for F, HW, Cc, fps in ((16, 2560, 960, 1), (16, 640, 1920, 1), (16, 40, 1280, 16), (48, 40960, 256, 1)):
        rc, pl = plan(descriptor(F, HW, Cc, fps, []))
        assert rc == 0 and pl.path == PARTIAL and pl.launches == 3 and pl.workspace_bytes == _lib.load().geo4d_groupnorm_workspace(F, HW, 32, fps)


def test_forced_paths_and_workspace():
    lib = _lib.load()
    for F, HW, Cc, fps, srcs in ((16, 2560, 320, 1, [(64, 320)]), (16, 40, 1280, 16, [(64, 1280)]), (2, 64, 960, 2, [(8, 320), (32, 640)]), (4, 1, 960, 2, [(1, 960)]),
                                 (48, 2560, 512, 1, [(128, 512)])):
        for path in (0, PARTIAL, COLS, FUSED, SLICED):
            rc, pl = plan(descriptor(F, HW, Cc, fps, srcs, path=path))
            assert rc == 0, lib.geo4d_last_error()
            if path == COLS:
                assert pl.path == (COLS if len(srcs) == 1 else PARTIAL)       # the two-launch sequence reads one full-width source
            elif path:
                assert pl.path == path
            assert pl.launches == {PARTIAL: 3, COLS: 2, FUSED: 1, SLICED: 2}[pl.path]
            assert pl.workspace_bytes <= lib.geo4d_groupnorm_workspace(F, HW, 32, fps)
            if pl.path == SLICED:
                assert 1 <= pl.stat_slices <= 64 and pl.workspace_bytes == (F // fps) * 32 * pl.stat_slices * 16
        rc, pl = plan(descriptor(F, HW, Cc, fps, []))
        assert rc == 0 and pl.path == PARTIAL and pl.launches == 3 and 0 < pl.workspace_bytes <= lib.geo4d_groupnorm_workspace(F, HW, 32, fps)
    # (pinned by tests/test_host_logic.py too: the workspace of the largest per-frame shape did not grow)
    assert lib.geo4d_groupnorm_workspace(16, 2560, 32, 1) == (16 * 64 * 32 * 3 + 16 * 32 * 2) * 4


def test_the_query_refuses_what_the_launch_refuses():
    lib = _lib.load()
    good = dict(F=16, HW=160, Cc=1280, fps=16, srcs=[(64, 1280)])

    def refused(mutate, **kw):
        args = dict(good)
        args.update(kw)
        q = descriptor(args["F"], args["HW"], args["Cc"], args["fps"], args["srcs"], **{k: v for k, v in args.items() if k in ("dtype", "split_out", "groups", "path")})
        if mutate:
            mutate(q)
        rc, _ = plan(q)
        rc2 = lib.geo4d_groupnorm2(C.byref(q), None)          # argument errors come before any launch
        assert rc == rc2 == -22, (rc, rc2, kw)
        assert b"groupnorm" in lib.geo4d_last_error()

    assert plan(descriptor(**{**good, "Cc": 1280}))[0] == 0
    refused(None, dtype=7)
    refused(None, Cc=1290)                                   # C % groups
    refused(None, groups=33, Cc=33 * 4)
    refused(None, fps=5)                                     # F % frames_per_stat
    refused(None, srcs=[(48, 1280)])                         # (frames_per_stat x HW) % rows
    refused(None, srcs=[(64, 640)])                          # the sources do not cover the channels
    refused(None, srcs=[(64, 640), (64, 320)])
    refused(None, dtype=_lib.BF16, split_out=1)              # the operand formats are written from f32 input
    refused(None, split_out=3)
    refused(None, path=9)
    refused(None, path=FUSED, srcs=[])                       # a forced sums path without sums
    refused(None, path=SLICED, srcs=[])
    refused(lambda q: setattr(q.base, "ldx", 1281))          # 16-byte rows
    refused(lambda q: setattr(q.base, "x", 0x10004))
    refused(lambda q: setattr(q.src[0], "colsum", 0x50004))
    refused(lambda q: setattr(q.src[0], "c0", 8))
    refused(lambda q: setattr(q, "nsrc", 3))
    refused(lambda q: setattr(q, "fuse_fraction", -1.0))
    # a workspace that is too small is the launch's own check: the query reports the size
    q = descriptor(16, 2560, 320, 16, [(64, 320)])
    rc, pl = plan(q)
    assert rc == 0 and pl.path == SLICED and pl.workspace_bytes > 0
    q.base.workspace, q.base.workspace_bytes = 0x60000, pl.workspace_bytes - 1
    assert lib.geo4d_groupnorm2(C.byref(q), None) == -22 and b"workspace" in lib.geo4d_last_error()
