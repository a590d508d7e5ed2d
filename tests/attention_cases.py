"""Case table, float64 reference and rounding-point emulation of the attention geometry sweep (tests/test_attention_geometry_cpu.py,
tests/test_attention_geometry_gpu.py): geo4d_attention at the shapes the model issues besides square self-attention.

A case is a dict: name, group, B, Nq, sets = ((Nk, kv_div), ...), wide (q and K are column slices of wider buffers), vt_extra (V^T pitch
beyond the 16-byte round-up of Nk), gain (group E: the keys are built, E_GAIN per mode), only (the modes it is restricted to, or None). All cases have H = 2 heads of 64
channels and scale = 0.125; the data are seeded randn (group E: built, see `make_data`).

  A  text-only cross-attention as the U-Net issues it: 77 keys shared by the T = 3 frames of a sample (kv_div = 3), V^T padded to 80,
     K a column slice of a [Bs*77, 3C + 16] buffer at an offset that is 16-byte but not 32-byte aligned, q a slice of a wider buffer
  B  the resampler: 16 queries on 257 / 273 keys (5 key tiles, the last of 1 / 17 keys), V^T pitch 16 elements beyond the round-up
  C  key-count edges around 1, 8, 64 and 128 (and around 4 for the 4-byte storage modes), V^T pitch as in B
  D  two key/value sets (text + image keys, both orders; two full tiles; a ragged tile followed by a single key)
  E  the segment switch with the running maxima far apart: set 0's keys are +gain x the (batch, head)'s mean query, set 1's -gain x it,
     so every row's scores are ~ +32 gain in set 0 and ~ -32 gain in set 1. A running maximum / sum that survives the switch makes
     set 1's P = 2^(-92 gain) or less: its output vanishes. gain = 6 (scores +-190: P underflows to 0) in the 16-bit modes. The score
     of a 4-byte mode carries an ABSOLUTE error that grows with its size (fp32 accumulation at |raw score| ~ 1500: one ulp = 1.5e-5
     scaled; bf16x3: the 2^-17 relative error of both hi + lo operands), and softmax turns an absolute score error into a relative
     error of P: at gain 6 the emulation alone gives 4.5e-5 (f32) and 1.2e-4 (bf16x3) per row, above the bounds. Their gain is
     therefore the one at which the emulation has a third of the bound to spare: f32 1.5 (scores +-47, 9.7e-6), bf16x3 0.75 (+-24,
     2.7e-5) - still 2^-135 / 2^-69 for an unreset second softmax.

Modes: f32, bf16, f16, bf16x3 (raw f32 operands) and bf16x3ps (pre-split q / K / V^T: one set, Nk % 8 == 0, 32-byte aligned slices).

`reference` is plain float64; `emulate` is the same math with the kernels' rounding points (not their schedule); `geometry` is the
buffer layout of a (case, mode) in elements, shared by the GPU launches and by the CPU test's fake-pointer descriptors."""
import functools

import torch

H, C, SCALE = 2, 128, 0.125
MODES = ("f32", "bf16", "f16", "bf16x3", "bf16x3ps")
DTYPE_CODE = {"f32": 0, "bf16": 1, "f16": 2, "bf16x3": 3, "bf16x3ps": 3}
# per (batch, head, query row) bound of the GPU parity check: 2 x the project's attention tolerance (tests/test_kernels_gpu.py TOL,
# tests/test_bf16x3_gpu.py 5e-5), applied per row instead of over the whole output
BOUND = {"bf16": 1.2e-2, "f16": 2e-3, "f32": 4e-5, "bf16x3": 1e-4, "bf16x3ps": 1e-4}
MANT = {"bf16": 7, "f16": 10, "f32": 23, "bf16x3": 23, "bf16x3ps": 23}       # explicit mantissa bits of the OUTPUT type
E_GAIN = {"bf16": 6.0, "f16": 6.0, "f32": 1.5, "bf16x3": 0.75}          # group E (module docstring)
VARIANTS = (0, 1, 2, 3, 4, 5)
SENTINEL = 24576.0            # exact in every storage type
OUT_PAD = 8                   # guard columns on both sides of `out` (16 / 32 bytes: the slice start stays 16-byte aligned)
EXTRA_ROWS = 3                # rows after q / K / out that a launch must neither read into its result nor write


def four_byte(mode):
    return mode in ("f32", "bf16x3", "bf16x3ps")


def torch_dtype(mode):
    return {"bf16": torch.bfloat16, "f16": torch.float16}.get(mode, torch.float32)


def _case(name, group, B, Nq, sets, *, wide=False, vt_extra=0, gain=0.0, only=None):
    return dict(name=name, group=group, B=B, Nq=Nq, sets=tuple(sets), wide=wide, vt_extra=vt_extra, gain=gain, only=only)


def _table():
    T = 3
    cases = []
    for nq in (50, 128, 129, 256, 257, 300):
        cases.append(_case(f"A_nq{nq}", "A", 2 * T, nq, [(77, T)], wide=True))
    for nq in (50, 300):           # the pre-split form of A: Nk % 8 == 0
        cases.append(_case(f"A_nk80_nq{nq}", "A", 2 * T, nq, [(80, T)], wide=True, only=("bf16x3ps",)))
    for nk in (257, 273):
        cases.append(_case(f"B_nk{nk}", "B", 3, 16, [(nk, 1)], vt_extra=16))
    for nq in (33, 257):
        for nk in (1, 7, 8, 9, 63, 64, 65, 127, 128, 129):
            cases.append(_case(f"C_nq{nq}_nk{nk}", "C", 2, nq, [(nk, 1)], vt_extra=16))
        for nk in (3, 4, 5):
            cases.append(_case(f"C_nq{nq}_nk{nk}", "C", 2, nq, [(nk, 1)], vt_extra=16, only=("f32", "bf16x3")))
    pairs = (("text_img", ((77, T), (16, 1))), ("img_text", ((16, 1), (77, T))), ("full_full", ((64, 1), (64, 1))), ("ragged_one", ((65, 1), (1, 1))))
    for pname, pair in pairs:
        for nq in (50, 128, 129, 300):
            cases.append(_case(f"D_{pname}_nq{nq}", "D", 2 * T, nq, pair))
    cases.append(_case("E_far_maxima", "E", 2, 130, [(70, 1), (70, 1)], gain=True))
    return cases


CASES = _table()
BY_NAME = {c["name"]: c for c in CASES}
SPLIT_OUT_CASES = ("A_nq129", "B_nk273", "C_nq257_nk65", "D_text_img_nq129", "E_far_maxima")      # one per group (check 7)


def modes_of(case):
    """The modes a case runs in: pre-split operands take one key/value set with Nk % 8 == 0."""
    out = []
    for m in MODES:
        if case["only"] is not None and m not in case["only"]:
            continue
        if m == "bf16x3ps" and (len(case["sets"]) != 1 or case["sets"][0][0] % 8):
            continue
        out.append(m)
    return out


def case_modes():
    return [(c["name"], m) for c in CASES for m in modes_of(c)]


# ---- data ---------------------------------------------------------------------------------------------------------------------------

def storage_round(x, mode):
    """The values the kernel sees: 16-bit modes round q / k / v to their storage type; f32 and bf16x3 keep them."""
    return x.to(torch_dtype(mode)).float() if not four_byte(mode) else x


@functools.lru_cache(maxsize=None)
def make_data(name, mode, uniform=False):
    """(q [B*Nq, C], ((k [KB*Nk, C], v [KB*Nk, C], Nk, kv_div), ...)) as f32 CPU tensors holding the values the kernel sees.
    `uniform`: q = 0 and V from {-3, -1, 1, 3} (exact in bf16, lo half 0): every score is 0, every P exactly 1."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(1000 + CASES.index(c))
    B, Nq = c["B"], c["Nq"]
    q = torch.randn((B * Nq, C), generator=g)
    gain = E_GAIN[mode] if c["gain"] else 0.0
    if gain:
        # every query row = a fixed direction of +-2 per channel + noise; the keys of set 0 are +gain x the (batch, head)'s mean query,
        # those of set 1 -gain x it (+ unit noise): scores ~ +- 0.125 * gain * 64 * 4
        base = torch.randint(0, 2, (C,), generator=g).float() * 4 - 2
        q = base + 0.5 * q
    sets = []
    for s, (nk, div) in enumerate(c["sets"]):
        kb = B // div
        k = torch.randn((kb * nk, C), generator=g)
        v = torch.randn((kb * nk, C), generator=g)
        if gain:
            qm = q.reshape(B, Nq, C).mean(1)[torch.arange(kb) * div]
            k = k + (gain if s == 0 else -gain) * qm.repeat_interleave(nk, 0)
        if uniform:
            v = torch.randint(0, 4, (kb * nk, C), generator=g).float() * 2 - 3
        sets.append((storage_round(k, mode), storage_round(v, mode), nk, div))
    if uniform:
        q = torch.zeros_like(q)
    return storage_round(q, mode), tuple(sets)


# ---- reference and emulation --------------------------------------------------------------------------------------------------------

def _heads(x, b, n):
    return x.reshape(b, n, H, 64).permute(0, 2, 1, 3)


def _rows(x, b, n):
    return x.permute(0, 2, 1, 3).reshape(b * n, H * 64)


def reference(q, sets, B, H_, Nq, scale):
    """sum over sets of softmax(q k^T scale) v in float64, key batch b // kv_div. sets: (k, v, Nk, kv_div), V not transposed."""
    assert H_ == H
    qh = _heads(q.double(), B, Nq)
    out = torch.zeros_like(qh)
    for k, v, nk, div in sets:
        kb = torch.arange(B) // div
        kh, vh = _heads(k.double(), B // div, nk)[kb], _heads(v.double(), B // div, nk)[kb]
        out = out + torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1) @ vh
    return _rows(out, B, Nq)


def _split(x):
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def _mm(a, b, x3):
    """a @ b with fp32 accumulation; x3: the three products of the hi / lo bf16 split of both operands (lo x lo dropped)."""
    if not x3:
        return a @ b
    ah, al = _split(a)
    bh, bl = _split(b)
    return al @ bh + ah @ bl + ah @ bh


def emulate(q, sets, B, H_, Nq, scale, mode):
    """The kernels' arithmetic in torch on the CPU: fp32 scores (bf16x3: three bf16 products), exp2 with the scale folded into one
    fma, fp32 row sums of the UNROUNDED P, P rounded to the storage type (bf16x3: hi / lo split) before P.V, each set normalised by
    its own 1 / l and the sets summed in fp32, the output rounded to the storage type. The running maximum and sum are kept as state
    that is reset where a set begins, as the kernel does. A model of the arithmetic, not of the schedule."""
    assert H_ == H
    x3 = mode in ("bf16x3", "bf16x3ps")
    dt = torch_dtype(mode)
    c2 = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32))
    qh = _heads(q.float(), B, Nq)
    out = torch.zeros_like(qh)
    for k, v, nk, div in sets:
        m_run = torch.full((B, H, Nq), -float("inf"))        # state reset at the segment switch
        l_run = torch.zeros((B, H, Nq))
        kb = torch.arange(B) // div
        kh, vh = _heads(k.float(), B // div, nk)[kb], _heads(v.float(), B // div, nk)[kb]
        s = _mm(qh, kh.transpose(-1, -2), x3)
        m_new = torch.maximum(m_run, s.max(-1).values)
        l_run = l_run * torch.exp2((m_run - m_new) * c2)
        m_run = m_new
        mc = -(m_run * c2)
        p = torch.exp2((s.double() * c2.double() + mc.double()[..., None]).float())          # one fma: a single rounding
        l_run = l_run + p.sum(-1)
        pr = p if four_byte(mode) else p.to(dt).float()
        o = _mm(pr, vh, x3)
        out = out + o * (1.0 / l_run)[..., None]
    return _rows(out, B, Nq).to(dt).float()


def row_err(got, ref):
    """(worst relative L2 over the 64 channels of one (batch, head, query row), relative L2 over the whole output)."""
    g, r = got.double().reshape(-1, H, 64), ref.double().reshape(-1, H, 64)
    per_row = (g - r).norm(dim=-1) / r.norm(dim=-1)
    return per_row.max().item(), ((g - r).norm() / r.norm()).item()


def ulp(x, mode):
    """One unit in the last place of the mode's output type at |x| (float64 tensor)."""
    e = torch.frexp(x.abs().clamp_min(2.0 ** -120)).exponent - 1
    return torch.ldexp(torch.ones_like(x), e - MANT[mode])


def uniform_expected(sets, B, mode):
    """Uniform attention (q = 0): the exact output row of every (batch, head) = sum over sets of the mean of the key batch's V rows
    [B, C], and the tolerance per element. One set: 1 ulp of the output type (f32 outputs: 2, 1 / l is rounded before the multiply).
    Two sets: the two means are formed in fp32 and added in fp32 before the only rounding to the output type, so each mean brings
    its own fp32 error (2 ulp of f32 AT THE MEAN, which a cancelling sum does not shrink) on top of the bound at the sum."""
    means = [v.double().reshape(B // div, nk, C).mean(1)[torch.arange(B) // div] for _, v, nk, div in sets]
    exact = sum(means)
    tol = (2 if four_byte(mode) else 1) * ulp(exact, mode)
    if len(sets) == 2:
        tol = tol + sum(2 * ulp(m, "f32") for m in means)
    return exact, tol


# ---- layout -------------------------------------------------------------------------------------------------------------------------

def geometry(case, mode):
    """Buffer layout in ELEMENTS (a pre-split element is 4 bytes: a bf16 hi and a bf16 lo): es bytes per element, epc elements per 16
    bytes of a V^T row, off = column offset of the q / K slices, qW / kW = buffer widths, per set rup (Nk rounded up to 16 bytes) and
    pitch of a V^T row."""
    es = 4 if four_byte(mode) else 2
    epc = 8 if mode == "bf16x3ps" else 16 // es
    # 16-byte aligned, not 32-byte aligned: 8 x 2 bytes / 4 x 4 bytes; the pre-split form needs 32-byte aligned slices: 8 x 4 bytes
    off = 0 if not case["wide"] else 8 if (es == 2 or mode == "bf16x3ps") else 4
    g = dict(es=es, epc=epc, off=off, qW=C + 32 if case["wide"] else C, kW=3 * C + 16 if case["wide"] else C, sets=[])
    for nk, div in case["sets"]:
        rup = (nk + epc - 1) // epc * epc
        g["sets"].append(dict(Nk=nk, div=div, rup=rup, pitch=rup + case["vt_extra"]))
    return g


def fake_descriptor(case, mode, variant):
    """geo4d_attention_t of a (case, mode, variant) with fake pointers that have the real slices' alignment: for the planner only."""
    from geo4d_amd import _lib
    g = geometry(case, mode)
    p = _lib.Attention()
    p.q, p.o, p.zeros = 0x10000000 + g["off"] * g["es"], 0x20000000 + OUT_PAD * g["es"], 0x30000000
    p.ldq, p.ldo = g["qW"], C + 2 * OUT_PAD
    for s, gs in enumerate(g["sets"]):
        p.k[s], p.vt[s] = 0x40000000 + (s << 28) + g["off"] * g["es"], 0x60000000 + (s << 28)
        p.ldk[s], p.ldvt[s], p.vt_bs[s], p.Nk[s], p.kv_div[s] = g["kW"], gs["pitch"], C * gs["pitch"], gs["Nk"], gs["div"]
    p.B, p.H, p.Nq, p.nseg, p.head_dim, p.dtype, p.scale = case["B"], H, case["Nq"], len(g["sets"]), 64, DTYPE_CODE[mode], SCALE
    p.variant, p.qkv_split = variant, int(mode == "bf16x3ps")
    return p


def _store(buf, mode, dev):
    """An f32 CPU matrix in the mode's storage on `dev` (pre-split: the [8 x hi | 8 x lo] image, 2 bf16 per element)."""
    from geo4d_amd import pack
    if mode == "bf16x3ps":
        return pack.split_bf16(buf).to(dev)
    return buf.to(torch_dtype(mode)).to(dev)


def _cols(t, mode, c0, n):
    """Columns [c0, c0 + n) in elements of a stored matrix."""
    from geo4d_amd import ops
    if mode == "bf16x3ps":
        return ops.SplitAct.wrap(t[:, 2 * c0:2 * (c0 + n)])
    return t[:, c0:c0 + n]


def launch_args(case, mode, q, sets, dev, poison=()):
    """(q view, kv list for ops.attention, buffers) for (q, sets) laid out as `geometry` says. Everything a launch may not depend on is
    finite in a clean build (zeros in the V^T padding, 0.5 elsewhere); `poison` replaces it:
      "a"  V^T columns [Nk, rup): 1e4          "b"  V^T columns [rup, pitch): NaN
      "c"  K rows after the last key batch: NaN   "d"  q rows after B*Nq: NaN
    `buffers` = dict(q=..., k=[...], vt=[...]) holds the stored whole buffers (vt: [KB, C, pitch] in elements) for the isolation check."""
    g = geometry(case, mode)
    B, Nq, off = case["B"], case["Nq"], g["off"]
    per = 2 if mode == "bf16x3ps" else 1
    nan = float("nan")
    qbuf = torch.full((B * Nq + EXTRA_ROWS, g["qW"]), 0.5)
    qbuf[B * Nq:] = nan if "d" in poison else 0.5
    qbuf[:B * Nq, off:off + C] = q
    qst = _store(qbuf, mode, dev)
    bufs = dict(q=qst, k=[], vt=[])
    kv = []
    for (k, v, nk, div), gs in zip(sets, g["sets"]):
        kb = B // div
        kbuf = torch.full((kb * nk + EXTRA_ROWS, g["kW"]), 0.5)
        kbuf[kb * nk:] = nan if "c" in poison else 0.5
        kbuf[:kb * nk, off:off + C] = k
        vt = torch.zeros((kb, C, gs["pitch"]))
        vt[:, :, :nk] = v.reshape(kb, nk, C).permute(0, 2, 1)
        if "a" in poison:
            vt[:, :, nk:gs["rup"]] = 1e4
        if "b" in poison:
            vt[:, :, gs["rup"]:] = nan
        kst, vst = _store(kbuf, mode, dev), _store(vt.reshape(kb * C, gs["pitch"]), mode, dev)
        bufs["k"].append(kst)
        bufs["vt"].append(vst)
        kv.append((_cols(kst[:kb * nk], mode, off, C), _cols(vst, mode, 0, gs["pitch"]), nk, div, per * C * gs["pitch"]))
    return _cols(qst[:B * Nq], mode, off, C), kv, bufs


def isolated_args(case, mode, bufs, b, h):
    """The launch arguments of ONE (batch, head) on its own slices of the full launch's buffers (B = 1, H = 1, kv_div = 1)."""
    g = geometry(case, mode)
    Nq, off = case["Nq"], g["off"]
    per = 2 if mode == "bf16x3ps" else 1
    q = _cols(bufs["q"][b * Nq:(b + 1) * Nq], mode, off + 64 * h, 64)
    kv = []
    for s, gs in enumerate(g["sets"]):
        nk, kb = gs["Nk"], b // gs["div"]
        k = _cols(bufs["k"][s][kb * nk:(kb + 1) * nk], mode, off + 64 * h, 64)
        vt = _cols(bufs["vt"][s][kb * C + 64 * h:kb * C + 64 * (h + 1)], mode, 0, gs["pitch"])
        kv.append((k, vt, nk, 1, per * 64 * gs["pitch"]))
    return q, kv


def poisons_of(case, mode):
    """The poison builds that change something for this (case, mode): (a) needs Nk below its round-up, (b) a pitch beyond it."""
    g = geometry(case, mode)
    out = []
    if any(gs["rup"] > gs["Nk"] for gs in g["sets"]):
        out.append("a")
    if any(gs["pitch"] > gs["rup"] for gs in g["sets"]):
        out.append("b")
    return out + ["c", "d"]


def instantiations(case, mode, plan_of):
    """[(variant, (kernel, nseg, qb, occ, ps), plan)]: each DISTINCT instantiation the planner resolves variants 0..5 to, once, under the
    first variant that names it. `plan_of(variant)` returns the plan or raises where the planner refuses the variant."""
    from geo4d_amd import _lib
    seen, out = set(), []
    for variant in VARIANTS:
        try:
            plan = plan_of(variant)
        except _lib.Geo4DNativeError:
            continue
        key = (plan.kernel, plan.nseg, plan.qb, plan.occ, plan.ps)
        if key not in seen:
            seen.add(key)
            out.append((variant, key, plan))
    return out
