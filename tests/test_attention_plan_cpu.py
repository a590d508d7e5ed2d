"""CPU tests of the attention planner (csrc/attention_plan.h) through geo4d_attention_plan, which is pure host code: for every
descriptor of a sweep the library's plan equals `expected()`, a transcription of the launch rules as geo4d_attention applied them
BEFORE the planner existed (an if-chain that rewrote `variant` in place, in that order), written here without calling the library.

The sweep: dtype 0..3 (f32, bf16, f16, bf16x3); one and two key/value sets; qkv_split 0 / 1; variant -1..6; Nq on both sides of
the 256-row and the 1024-row thresholds (Nk = Nq rounded up to a multiple of 8); a normal key pitch and one so large that a
(batch, head)'s keys leave the second kernel's 2 GB window. Pointers are fake and aligned; no kernel is launched: a refused descriptor
is also handed to geo4d_attention itself, which must refuse it with the same code and message before it touches the device."""
import ctypes
import itertools

import pytest

EINVAL, ENOTSUP = -22, -95
F32, BF16, F16, BF16X3 = 0, 1, 2, 3
H, B = 2, 3
BIG_LDK = 1 << 25          # (Nk + 64) * 2^25 elements >= 2^31 bytes for every Nk > 0 and both element sizes

MSG_ARGS = "attention: bad arguments"
MSG_HEAD = "attention: only d_head = 64 is built (yaml num_head_channels: 64)"
MSG_QO = "attention: q/o alignment"
MSG_KV = "attention: bad key/value segment"
MSG_ZEROS = "attention: `zeros` must point at 16 zero bytes"
MSG_GRID = "attention: grid too large"
MSG_SPLIT_OUT = "attention: split_out is the producer format of the 4-byte storage modes (f32 / bf16x3)"
MSG_QKV_SPLIT = "attention: qkv_split needs dtype bf16x3, one key/value set, Nk % 8 == 0, leading dimensions % 8 == 0 and 32-byte aligned bases"
MSG_VARIANT = "attention: unknown variant"
MSG_V45 = "attention: variants 4 / 5 take one key/value set in bf16 / f16 (4) or pre-split bf16x3"
MSG_WINDOW = "attention: variants 4 / 5 need one (batch, head)'s keys and V^T rows inside a 2 GB window"


def descriptor(dtype=BF16, nseg=1, qkv_split=0, variant=0, Nq=256, ldk=H * 64):
    from geo4d_amd import _lib
    p = _lib.Attention()
    nk = (Nq + 7) // 8 * 8
    p.q, p.o, p.zeros = 0x10000000, 0x20000000, 0x30000000
    p.ldq = p.ldo = H * 64
    for s, n in enumerate((nk, 16)[:nseg]):
        p.k[s], p.vt[s] = 0x40000000 + (s << 28), 0x60000000 + (s << 28)
        p.ldk[s], p.ldvt[s], p.vt_bs[s], p.Nk[s], p.kv_div[s] = ldk, n, H * 64 * n, n, 1
    p.B, p.H, p.Nq, p.nseg, p.head_dim, p.dtype, p.scale = B, H, Nq, nseg, 64, dtype, 0.125
    p.variant, p.qkv_split = variant, qkv_split
    return p


def expected(p):
    """(rc, message) of a refusal, or (kernel, nseg, qb, occ, ps, rows_per_wg, grid): the checks and the dispatch chain of the launch
    function in the order it made them."""
    aligned = lambda ptr, n: (ptr or 0) % n == 0
    b16, x3 = p.dtype in (BF16, F16), p.dtype == BF16X3
    esz = 2 if b16 else 4
    epc = 16 // esz
    if not (0 <= p.dtype <= 3) or p.B <= 0 or p.H <= 0 or p.Nq <= 0 or not (1 <= p.nseg <= 2):
        return EINVAL, MSG_ARGS
    if p.head_dim != 64:
        return ENOTSUP, MSG_HEAD
    if (p.ldq * esz) % 16 or (p.ldo * esz) % 16 or not aligned(p.q, 16) or not aligned(p.o, 16):
        return EINVAL, MSG_QO
    for s in range(p.nseg):
        if (p.Nk[s] <= 0 or p.kv_div[s] <= 0 or not p.k[s] or not p.vt[s] or (p.ldk[s] * esz) % 16 or (p.ldvt[s] * esz) % 16 or (p.vt_bs[s] * esz) % 16
                or not aligned(p.k[s], 16) or not aligned(p.vt[s], 16) or p.ldvt[s] < 0 or (p.Nk[s] + epc - 1) // epc * epc > p.ldvt[s]):
            return EINVAL, MSG_KV
    if not p.zeros or not aligned(p.zeros, 16):
        return EINVAL, MSG_ZEROS
    if p.H > 65535 or p.B > 65535:
        return EINVAL, MSG_GRID
    if p.split_out and esz != 4:
        return EINVAL, MSG_SPLIT_OUT
    if p.qkv_split and (not x3 or p.nseg != 1 or p.Nk[0] % 8 or p.ldq % 8 or p.ldk[0] % 8 or p.ldvt[0] % 8 or p.vt_bs[0] % 8
                        or not aligned(p.q, 32) or not aligned(p.k[0], 32) or not aligned(p.vt[0], 32)):
        return EINVAL, MSG_QKV_SPLIT
    variant = p.variant
    if variant < 0 or variant > 5:
        return EINVAL, MSG_VARIANT
    window_ok = p.nseg == 1 and ((p.Nk[0] + 64) * p.ldk[0] + 64) * esz < 2 ** 31 and (64 * p.ldvt[0] + p.Nk[0] + 64) * esz < 2 ** 31
    if variant == 0 and p.nseg == 1 and p.Nq >= 256 and window_ok and (b16 or (x3 and p.qkv_split)):
        variant = 5 if (x3 and p.Nq >= 1024) else 4
    if variant >= 4:
        if p.nseg != 1 or not ((b16 and variant == 4) or (x3 and p.qkv_split)):
            return EINVAL, MSG_V45
        if not window_ok:
            return EINVAL, MSG_WINDOW
        occ = 2 if b16 else 1 if variant == 4 else 2
        return 2, 1, 2, occ, int(x3), 256, ((p.Nq + 255) // 256, p.H, p.B)
    if variant == 0:
        variant = 3 if (p.nseg == 1 and b16) else 1
    if variant == 3 and p.nseg == 2:
        variant = 1
    if variant == 2 and not b16:
        variant = 1
    rows = 256 if variant == 3 else 128
    grid = ((p.Nq + rows - 1) // rows, p.H, p.B)
    ps = int(x3 and bool(p.qkv_split))
    if p.nseg == 2:
        return 1, 2, 1, 1, ps, rows, grid
    if variant == 3:
        return 1, 1, 2, 2, ps, rows, grid
    if b16 and variant == 2:
        return 1, 1, 1, 4, ps, rows, grid
    return 1, 1, 1, 1, ps, rows, grid


def ask(lib, p):
    """The library's answer in the form of expected()."""
    from geo4d_amd import _lib
    plan = _lib.AttentionPlan()
    rc = lib.geo4d_attention_plan(ctypes.byref(p), ctypes.byref(plan))
    if rc:
        return rc, lib.geo4d_last_error().decode()
    return plan.kernel, plan.nseg, plan.qb, plan.occ, plan.ps, plan.rows_per_wg, tuple(plan.grid)


def launch_refuses(lib, p):
    """geo4d_attention on a descriptor that must be refused: the checks come before any device call, so this needs no GPU."""
    rc = lib.geo4d_attention(ctypes.byref(p), None)
    assert rc != 0
    return rc, lib.geo4d_last_error().decode()


def test_plan_equals_the_launch_rules_over_the_sweep():
    from geo4d_amd import _lib
    lib = _lib.load()
    seen, refused = set(), set()
    for dtype, nseg, qs, variant, Nq, ldk in itertools.product(range(4), (1, 2), (0, 1), range(-1, 7), (40, 255, 256, 1023, 1024, 2560), (H * 64, BIG_LDK)):
        p = descriptor(dtype, nseg, qs, variant, Nq, ldk)
        want, got = expected(p), ask(lib, p)
        assert got == want, ((dtype, nseg, qs, variant, Nq, ldk), want, got)
        if len(want) == 2:
            refused.add(want)
            assert launch_refuses(lib, p) == want
            continue
        seen.add((dtype,) + want[:5])
        plan = _lib.AttentionPlan()
        assert lib.geo4d_attention_plan(ctypes.byref(p), ctypes.byref(plan)) == 0
        assert plan.rows_per_wg == 128 * plan.qb
        p.variant = plan.variant          # the effective variant, asked for explicitly, is the same launch
        assert 1 <= plan.variant <= 5 and ask(lib, p) == want, ((dtype, nseg, qs, variant, Nq, ldk), plan.variant)
    # every instantiation the library builds is reached, and nothing else: (dtype, kernel, nseg, qb, occ, ps)
    first = {(d, 1) + i + (0,) for d in range(4) for i in ((2, 1, 1), (1, 2, 2), (1, 1, 1))} | {(d, 1, 1, 1, 4, 0) for d in (BF16, F16)} | \
            {(BF16X3, 1, 1, 2, 2, 1), (BF16X3, 1, 1, 1, 1, 1)}
    second = {(BF16, 2, 1, 2, 2, 0), (F16, 2, 1, 2, 2, 0), (BF16X3, 2, 1, 2, 1, 1), (BF16X3, 2, 1, 2, 2, 1)}
    assert seen == first | second and len(seen) == 20
    assert refused == {(EINVAL, MSG_QKV_SPLIT), (EINVAL, MSG_VARIANT), (EINVAL, MSG_V45), (EINVAL, MSG_WINDOW)}


def _refusals():
    def case(msg, rc=EINVAL, **kw):
        def make(**fields):
            p = descriptor(**kw)
            for k, v in fields.items():
                if isinstance(v, tuple):
                    getattr(p, k)[v[0]] = v[1]
                else:
                    setattr(p, k, v)
            return p, rc, msg
        return make
    return {
        "no batch": case(MSG_ARGS)(B=0),
        "dtype 4": case(MSG_ARGS, dtype=4)(),
        "three key/value sets": case(MSG_ARGS)(nseg=3),
        "head_dim 32": case(MSG_HEAD, rc=ENOTSUP)(head_dim=32),
        "misaligned q": case(MSG_QO)(q=0x10000008),
        "f32 ldo % 4": case(MSG_QO, dtype=F32)(ldo=H * 64 + 2),
        "no keys": case(MSG_KV)(Nk=(0, 0)),
        "ldvt < Nk": case(MSG_KV)(ldvt=(0, 248)),
        "second set without vt": case(MSG_KV, nseg=2)(vt=(1, None)),
        "no zeros": case(MSG_ZEROS)(zeros=None),
        "B > 65535": case(MSG_GRID)(B=65536),
        "split_out on bf16": case(MSG_SPLIT_OUT)(split_out=1),
        "qkv_split with Nk % 8 != 0": case(MSG_QKV_SPLIT, dtype=BF16X3, qkv_split=1)(Nk=(0, 252)),
        "qkv_split on bf16": case(MSG_QKV_SPLIT, qkv_split=1)(),
        "qkv_split with a 16-byte aligned k": case(MSG_QKV_SPLIT, dtype=BF16X3, qkv_split=1)(k=(0, 0x40000010)),
        "variant 6": case(MSG_VARIANT, variant=6)(),
        "variant -1": case(MSG_VARIANT, variant=-1)(),
        "variant 5 on bf16": case(MSG_V45, variant=5)(),
        "variant 4 on f32": case(MSG_V45, dtype=F32, variant=4)(),
        "variant 4 on raw bf16x3": case(MSG_V45, dtype=BF16X3, variant=4)(),
        "variant 4 with two key/value sets": case(MSG_V45, nseg=2, variant=4)(),
        "variant 4 outside the window": case(MSG_WINDOW, variant=4, ldk=BIG_LDK)(),
        "variant 5 outside the window (V^T rows)": case(MSG_WINDOW, dtype=BF16X3, qkv_split=1, variant=5)(ldvt=(0, 1 << 24), vt_bs=(0, 1 << 31)),
    }


@pytest.mark.parametrize("name", list(_refusals()))
def test_refusals_keep_their_code_and_message(name):
    from geo4d_amd import _lib
    lib = _lib.load()
    p, rc, msg = _refusals()[name]
    assert expected(p) == (rc, msg)
    assert ask(lib, p) == (rc, msg)
    assert launch_refuses(lib, p) == (rc, msg)


def test_window_boundary_is_exact():
    """The default moves to the second kernel exactly while ((Nk + 64) ldk + 64) esz < 2^31 and (64 ldvt + Nk + 64) esz < 2^31."""
    from geo4d_amd import _lib
    lib = _lib.load()
    for dtype, qs, esz in ((BF16, 0, 2), (BF16X3, 1, 4)):
        nk = 256
        ldk_last = ((2 ** 31 // esz - 1 - 64) // (nk + 64)) // 8 * 8          # the largest pitch (a multiple of 8) inside the window
        ldvt_last = ((2 ** 31 // esz - 1 - nk - 64) // 64) // 8 * 8
        for field, last in (("ldk", ldk_last), ("ldvt", ldvt_last)):
            kernels = []
            for pitch in (last, last + 8):
                p = descriptor(dtype, 1, qs, 0, 256)
                getattr(p, field)[0] = pitch
                p.vt_bs[0] = H * 64 * p.ldvt[0]
                want = expected(p)
                assert ask(lib, p) == want
                kernels.append(want[0])
            assert kernels == [2, 1], (dtype, field, kernels)


def test_null_arguments():
    from geo4d_amd import _lib
    lib = _lib.load()
    plan = _lib.AttentionPlan()
    assert lib.geo4d_attention_plan(None, ctypes.byref(plan)) == EINVAL
    assert lib.geo4d_attention_plan(ctypes.byref(descriptor()), None) == EINVAL
