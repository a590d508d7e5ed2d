"""Torch-tensor front-ends of the C ABI (include/geo4d_hip.h).

PyTorch is plumbing only: it owns device memory (``torch.empty``) and the HIP stream. Every function takes 2-D
"token" views ``[rows, channels]`` (unit inner stride, arbitrary row pitch), hands raw device pointers to
libgeo4d_hip.so and returns immediately (stream ordered, hipGraph-capturable). There is no CPU/eager fallback:
tensors that are not on a HIP device raise.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import BF16, BF16X3, F16, F16X2, F32, Attention, AttentionPlan, ConvGemm, ConvGemmPlan, ConvGemmTile, GroupNorm2, GroupNormPlan
from .precision import resolve as _resolve_precision

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
_TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}


def dt_code(dtype):
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"geo4d_amd: unsupported dtype {dtype} (float32, bfloat16, float16 only)")


def k_align(dtype):
    """K / Cin granularity of conv_gemm in elements: one 128-byte LDS slab (4-byte elements for f32 and bf16x3)."""
    return 32 if _resolve_precision(dtype).storage == torch.float32 else 64


class X2Weight(torch.Tensor):
    """A pack.split_f16 weight: float16 [N, 2K] = f16 hi | lo per 8 K-elements of s * w, carrying alpha = 1 / s of its launch. A Tensor
    subclass so that the scale travels with the data: .to() / .clone() / .detach() / .contiguous() and same-shape views keep it (a
    plain attribute on a plain tensor was lost by all of them); slicing or reshaping gives a plain float16 tensor, which
    conv_gemm refuses as a two-pass weight."""
    _KEEP = {"to", "clone", "detach", "contiguous", "cuda", "cpu", "pin_memory"}

    @staticmethod
    def wrap(t, alpha):
        r = t.as_subclass(X2Weight)
        r._x2_alpha = float(alpha)
        return r

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        out = super().__torch_function__(func, types, args, kwargs or {})
        if isinstance(out, X2Weight):
            src = next((a for a in args if isinstance(a, X2Weight) and hasattr(a, "_x2_alpha")), None)
            if src is not None and getattr(func, "__name__", "") in cls._KEEP and out.shape == src.shape and out.dtype == torch.float16:
                out._x2_alpha = src._x2_alpha
            elif not hasattr(out, "_x2_alpha"):
                out = out.as_subclass(torch.Tensor)        # anything else is just a float16 matrix
        return out


def is_x2_weight(w):
    """A pack.split_f16 weight (X2Weight: float16 [N, 2K] = f16 hi | lo per 8 K-elements, carrying the 1 / scale of its launch)."""
    return isinstance(w, X2Weight) and w.dtype == torch.float16 and hasattr(w, "_x2_alpha")


def is_split(w, other):
    """True when `w` is a PRE-SPLIT bf16x3 operand (pack.split_bf16: bf16 [rows, 2K]) multiplied with a raw f32 operand."""
    return w.dtype == torch.bfloat16 and other.dtype == torch.float32


class SplitAct(torch.Tensor):
    """(The two-pass f16 consumers take PLAIN float16 rows since round 6 - an ordinary tensor, no wrapper: new_split(fmt="f16").)
    A bf16 [rows, 2K] activation in the pre-split bf16x3 operand format (per 8 K-elements: 8 x bf16 hi | 8 x bf16 lo), written by
    the producers that feed GEMMs (GroupNorm / LayerNorm / attention / GEGLU epilogue with split_out) so that conv_gemm does not
    split the fragments again in its K loop. A Tensor subclass only to make the format visible to conv_gemm; every other entry point
    of this module rejects it (`_dev`), and producers require a whole contiguous matrix as their split output (`_split_out_ok`).
    Plain torch ops on it (.float(), slicing at non-8-element offsets) still see a bf16 matrix: do not use them."""
    @staticmethod
    def wrap(t):
        return t.as_subclass(SplitAct)


def new_split(rows, k, device, fmt="bf16"):
    """The A operand a producer writes for the GEMM that follows. `fmt`: "bf16" = the pre-split bf16x3 operand format (SplitAct, bf16
    [rows, 2k]); "f16" = the two-pass f16 consumers' operand (dtype 4): PLAIN float16 rows [rows, k] - the activation is multiplied as
    one f16, so since round 6 nothing else is stored (round 5 wrote an f16 lo half beside it that no kernel read)."""
    if fmt == "f16":
        return torch.empty((rows, k), device=device, dtype=torch.float16)
    return SplitAct.wrap(torch.empty((rows, 2 * k), device=device, dtype=torch.bfloat16))


def split_fmt(split_out):
    """groupnorm(split_out=...) argument -> (ABI code, format name): False / None -> 0, True / "bf16" -> 1, "f16" -> 2."""
    if not split_out:
        return 0, None
    if split_out is True or split_out == "bf16":
        return 1, "bf16"
    if split_out == "f16":
        return 2, "f16"
    raise ValueError(f"split_out={split_out!r}: False, True / 'bf16' or 'f16'")


def act_k(x):
    """Channels (K elements) of an activation matrix: a SplitAct stores 2 bf16 per element."""
    return x.shape[1] // 2 if isinstance(x, SplitAct) else x.shape[1]


def kdim(w, other):
    """Logical K extent of a 2-D operand (a pre-split operand stores 2 bf16 / f16 per K element)."""
    return w.shape[1] // 2 if (is_split(w, other) or isinstance(other, SplitAct) or is_x2_weight(w)) else w.shape[1]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, what, split_ok=False):
    """Every operand goes through here: it must live on a HIP device, and a SplitAct (bf16 [rows, 2K] hi | lo image) may only reach
    the operands that understand the format - conv_gemm's A / W / out and the producers' `out`; anywhere else it would be silently
    reinterpreted as a bf16 matrix."""
    if not t.is_cuda:
        raise _lib.Geo4DNativeError(f"geo4d_amd.ops: `{what}` lives on {t.device}; the HIP path needs a GPU tensor "
                                    "(there is no CPU fallback)")
    if isinstance(t, SplitAct) and not split_ok:
        raise TypeError(f"geo4d_amd.ops: `{what}` is a pre-split bf16x3 activation (SplitAct); only GEMM operands take that format")
    return t


def _split_out_ok(out, rows):
    """Producers write the pre-split format with row-start-relative addressing (store_split4): the buffer must be the whole
    [rows, 2K] matrix - contiguous, starting at the row, 16-byte aligned - not a column-offset view of a wider one."""
    assert out.dim() == 2 and out.shape[0] == rows and out.is_contiguous() and out.data_ptr() % 16 == 0, \
        "a SplitAct output must be a contiguous [rows, 2K] matrix (no column-offset views)"


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _ld(t):
    assert t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1), f"need a [rows, cols] view with unit inner stride, got {t.shape} {t.stride()}"
    return t.stride(0)


_WS = {}
WORKSPACE_BYTES = 256 << 20
# (Round 6 built split-K WITHOUT the reduce launch - wave tickets, the last arrival of a (tile, wave) position sums the slabs and runs the
# epilogue, bit-equal to the reduce kernel - and measured it slower twice: with agent-scope release / acquire fences 6.37 -> 5.57 frames/s,
# with sc1 write-through slabs and no fence 6.31 -> 6.08. Removed; profiles/r06_splitk_fused.md.)

# ---- per-shape launch tuning ------------------------------------------------------------------------------------
# geo4d_conv_gemm has three kernel generations x tile shapes x split-K factors (include/geo4d_hip.h tile_hint); the C-side heuristic is a fallback. The host keeps a table
# problem-signature -> (tile_hint, split_k): loaded from geo4d_amd/tuning/gfx950.json (measured on MI355X by
# tools/tune_gemm.py) and, for shapes not in it, filled by timing the candidates on first eager use (never while a
# hipGraph is being captured). Every candidate computes the same sums in the same k order per output element
# (split-K only regroups them), so tuning never changes a GEMM's result beyond fp32 re-association. Since round 4 (GN_FUSED_STATS = 1)
# the tile choice ALSO sets the row granularity of the GroupNorm statistics its epilogue emits (32 ... 128 rows per entry), so the
# consumer GroupNorm - and with it the U-Net output - differs at fp32 round-off between tile choices: bit-reproducibility holds PER
# TUNING TABLE (the committed gfx950.json + whatever this process measured for shapes missing from it), not per candidate. Processes
# that must agree bit for bit (ranks comparing outputs, a captured graph against a later eager run of a shape first met during capture)
# need the same table: ship one (save_tuning) or set GEO4D_AUTOTUNE=0 / GEO4D_GN_FUSED=0.
import json as _json
import os as _os

_TUNE_PATH = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "tuning", "gfx950.json")
_TUNE = None
_CANDIDATES = [(1, 1), (2, 1), (3, 1), (4, 1), (11, 1), (13, 1), (16, 1), (17, 1), (17, 2), (16, 2), (17, 8), (1, 2), (1, 4), (1, 8), (11, 2), (11, 8), (13, 2), (13, 4), (3, 2), (4, 2), (4, 4), (3, 4), (2, 4), (5, 1),
               # second generation (gemm_kernel_v2.h: 16x16x32 MFMA, register epilogue, persistent workgroups; bf16 / bf16x3, no NCTHW outputs);
               # round 4 kept the five tiles the measured table selects
               (22, 1), (23, 1), (25, 1), (27, 1), (28, 1), (22, 2), (22, 4), (23, 2), (25, 2), (25, 4), (25, 8), (27, 2), (27, 4), (28, 2), (28, 4), (28, 8),
               # third generation (gemm_kernel_v3.h: phased K loop, counted DMA waits; 8-wave tiles, one workgroup per CU).
               # Splits that do not divide the K slabs evenly run on the second-generation twin inside the library.
               (71, 1), (72, 1), (73, 1), (74, 1), (71, 2), (72, 2), (73, 2), (74, 2), (71, 3), (72, 3), (73, 3), (74, 3), (71, 4), (73, 4), (74, 4),
               (71, 5), (73, 5), (74, 5), (73, 6), (74, 6), (73, 8), (74, 8), (73, 10), (74, 10)]
_TILE_ROWS = None


def _tiles():
    """{tile hint: its row (_lib.ConvGemmTile) of the library's tile table (csrc/gemm_plan.h)}, read once, on first use: importing this
    module does not load the library."""
    global _TILE_ROWS
    if _TILE_ROWS is None:
        rows = (ConvGemmTile * 64)()
        n = _lib.load().geo4d_conv_gemm_tiles(rows, len(rows))
        _TILE_ROWS = {t.tile_hint: t for t in rows[:n]}
        assert {t for t, _ in _CANDIDATES} == set(_TILE_ROWS)
    return _TILE_ROWS


def _generation(tile_hint):
    """1, 2 or 3; hint 0 (the library's own choice) and hints without a row count as the first generation."""
    t = _tiles().get(tile_hint)
    return t.generation if t is not None else 1


# GEO4D_AUTOTUNE=0: shapes missing from the tuning table run on the library's own tile choice instead of being measured on first eager use
AUTOTUNE = _os.environ.get("GEO4D_AUTOTUNE", "1") != "0"


def _env_level(name, default):
    """0 / 1 / 2 ... or the usual words: off / false / no -> 0, on / true / yes (and anything else that is not a number) -> 1."""
    v = _os.environ.get(name)
    if v is None or not v.strip():
        return default
    v = v.strip().lower()
    try:
        return int(v)
    except ValueError:
        return 0 if v in ("off", "false", "no", "none") else 1


# GEMM epilogues can emit the next GroupNorm's column sums (gn_stats=True call sites), which removes that GroupNorm's statistics pass
# over the tensor. 1 (default since round 4): where the second / third generation's fast epilogue does it per wave-tile row range at
# ~0.3 us per tile (f32 rows, i.e. the bf16x3 mode: same-box A/B +1.2 % frames/s, decode -2.5 %, profiles/r04_gn_fused_stats.md);
# 2: also on the first-generation tiles (round 2: measured slower there: -3.5 % bf16x3, -7 % bf16); 0: off.
GN_FUSED_STATS = _env_level("GEO4D_GN_FUSED", 1)
# 0: a GroupNorm with producer sums runs gn_finalize_cols + gn_apply and a concatenated input its own statistics pass (the launch
# sequence before the fused / sliced forms); 3 / 4: force _lib.GN_PATH_FUSED / GN_PATH_SLICED (tests, tools/norm_bench.py)
GN_ONE_LAUNCH = _env_level("GEO4D_GN_ONE_LAUNCH", 1)
GN_TUNE = (0.0, 0)     # tools/norm_bench.py: (fuse_fraction, min_workgroups) overrides of the library's defaults; 0 = default
# 0: split-K launches leave the GroupNorm statistics to the GroupNorm (the state before round 6, when their reduce launch learned to emit the sums)
SPLITK_COLSUM = _env_level("GEO4D_SPLITK_COLSUM", 1)
# tools/tune_gemm.py: measure a pre-split launch under its OWN key instead of borrowing the raw-activation entry of the same shape
TUNE_EXACT = _env_level("GEO4D_TUNE_EXACT", 0)
# (key, chosen (tile, split), ms per launch, finalists) of every shape autotuned in this process (tools/tune_gemm.py prints it)
TUNE_LOG = []
DEBUG_ABLATE = _env_level("GEO4D_DEBUG_ABLATE", 0)       # tests / A-B runs: 2 = three persistent workgroups; 16 + g = tile order with GROUP_M = g (17 = column-fastest)
# 0: 16-bit output rows keep the 8-byte epilogue (two stores per pair of 16-column blocks, the f16 clamp in f32, the debug counter tested per
# store) instead of the 16-byte one - same bits (tests/test_epilogue_wide_gpu.py), A/B: profiles/epilogue_wide.md. Bit 6 of debug_ablate.
EPI_WIDE = _env_level("GEO4D_EPI_WIDE", 1)
GEMM_TIMELINE = None   # set to a list to have conv_gemm bracket every launch with HIP events: (flops, start, end, MFMA passes per product)
ATTN_TIMELINE = None   # the same for the spatial self-attention launches (one key/value set) of ops.attention
SAT_COUNTER = None     # debug: an int64 [1] device tensor -> every f16-clamping store (GroupNorm / LayerNorm / GEGLU epilogue writing the two-pass
                       # GEMM's f16 operand) adds the lanes it clamped (|x| > 65504); tests assert 0 at full size. None in production.


def _on_timeline(timeline, launch, flops, passes):
    """bench.py's per-launch HIP-event timelines (GEMM_TIMELINE / ATTN_TIMELINE; never on while capturing): run `launch()` between two
    events and append (flops, start, end, MFMAs issued per product)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    timeline.append((flops, e0, e1, passes))


def _tune_table():
    global _TUNE
    if _TUNE is None:
        _TUNE = {}
        if _os.path.exists(_TUNE_PATH):
            with open(_TUNE_PATH) as f:
                _TUNE = {k: tuple(v) for k, v in _json.load(f).items() if v[0] == 0 or v[0] in _tiles()}     # (entries naming a retired tile hint are re-tuned)
    return _TUNE


def save_tuning(path=None):
    with open(path or _TUNE_PATH, "w") as f:
        _json.dump({k: list(v) for k, v in sorted(_tune_table().items())}, f, indent=0)


def _time_launches(launch, tile, split, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch(tile, split)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _autotune(launch, key, takes):
    """Two stages (round 4: a single 3-launch sample per candidate mis-ranked candidates that differ by 30-40 % when re-measured in
    isolation, profiles/r04_gemm_retune.md): (1) every candidate the plan accepts (`takes(tile, split)`), 4 launches after a warm-up;
    (2) the 6 fastest re-measured in three interleaved rounds of 12 launches, ranked by their best round (the chip's clock moves under
    load: the minimum is the least noisy estimate of what a launch costs inside a replayed graph)."""
    stage1 = []
    for tile, split in _CANDIDATES:
        if not takes(tile, split):
            continue
        try:
            launch(tile, split)
        except RuntimeError:       # (a launch error of an accepted plan: the launchers can return GEO4D_EIO)
            continue
        stage1.append((_time_launches(launch, tile, split, 4), tile, split))
    if not stage1:
        _tune_table()[key] = (0, 0)
        return (0, 0)
    stage1.sort()
    finalists = stage1[:6]
    best_of = {(t, s): float("inf") for _, t, s in finalists}
    for _ in range(3):
        for _, tile, split in finalists:
            best_of[(tile, split)] = min(best_of[(tile, split)], _time_launches(launch, tile, split, 12))
    best = min(best_of, key=best_of.get)
    _tune_table()[key] = best
    TUNE_LOG.append((key, best, best_of[best], [(t, s, round(v * 1e3, 1)) for (t, s), v in sorted(best_of.items(), key=lambda kv: kv[1])]))
    return best


def _tuned_config(table, key, code, a_split, w_split, o_split, may_measure):
    """(tile_hint, split_k) of the launch `key` from the tuning table - its own entry, or the entry of a launch with the same tile geometry -
    or None: no entry applies (the caller measures now if that is allowed, else the library chooses). `may_measure()`: whether timing
    candidates is allowed now (AUTOTUNE on, no capture running); only asked when `key` itself has no entry."""
    cfg = table.get(key)
    if cfg is None and code == BF16X3 and a_split and w_split and not (TUNE_EXACT and may_measure()):
        # pre-split activations: same tile geometry as the raw-activation launch of the same shape (table measured on those)
        base = key.split("|x")[0]
        cfg = (table.get(base + "|x11") if o_split else None) or table.get(base + "|x01") or table.get(base + "|x10")
        if cfg is not None and o_split and cfg[1] > 1:
            # the pre-split output has no split-K form (the reduce kernel writes plain f32): measure this launch on its own when
            # that is allowed, else keep the tile and drop the split
            cfg = None if may_measure() else (cfg[0], 1)
    if cfg is None and code == F16X2 and not may_measure():
        # no entry and no measuring now: the bf16x3 launch of the same shape is the same tile geometry and the same bytes
        cfg = table.get("3" + key[1:])
        if cfg is not None and _generation(cfg[0]) == 1:
            cfg = None                   # (the two-pass kernels exist on the second / third generation only: library default)
        elif cfg is not None and o_split and cfg[1] > 1:
            cfg = (cfg[0], 1)            # (a pre-split output has no split-K form)
    return cfg


# the nearest tile of the same generation that takes a GEGLU (wave tiles a multiple of 64 columns wide); a hint maps to itself unless listed
_GEGLU_NEIGHBOUR = {22: 25, 23: 25, 28: 27, 72: 71, 73: 74}


def _f16_rows_config(cfg, act):
    """The f16-row epilogue (o_split = 2) has no split-K, and its GEGLU form lives on the tiles whose wave tiles are a multiple of 64
    columns wide: a tile measured on, or borrowed from, another launch goes to its nearest such neighbour."""
    tile_hint, split_k = cfg
    return (_GEGLU_NEIGHBOUR.get(tile_hint, tile_hint) if act == 2 else tile_hint), min(split_k, 1)


def workspace(device):
    """One static fp32 scratch per device for split-K slabs (stream-ordered reuse; allocated outside graph capture)."""
    ws = _WS.get(device)
    if ws is None:
        ws = _WS[device] = (torch.empty(WORKSPACE_BYTES, device=device, dtype=torch.uint8),
                            torch.zeros(256, device=device, dtype=torch.uint8))
    return ws


def conv_gemm_descriptor(a, w, out, *, M, N, K, Cin, lda, ldw, ldo, T=1, Hin=1, Win=1, Hout=1, Wout=1, KT=1, KH=1, KW=1,
                         pt=0, ph=0, pw=0, stride=1, ups=1, bias=None, bias_per_row=False, rowbias=None, rowbias_div=0,
                         residual=None, ldr=0, act=0, out_nchw=False, alpha=1.0, batch=1, a_bs=0, w_bs=0, o_bs=0, r_bs=0,
                         tile_hint=0, split_k=0, x3=False):
    """The geo4d_conv_gemm_t of the launch `conv_gemm` makes for these arguments (gn_colsum null: conv_gemm offers the sums itself).
    `lda` / `ldw` / `a_bs` / `w_bs` are strides of the tensors as passed (torch elements). bf16x3 mode is selected by the
    operands: f32 activations against a pre-split bf16 weight (either side), or two f32 operands with `x3=True`."""
    _dev(a, "A", True); _dev(w, "W", True); _dev(out, "out", True)
    for opt, nm in ((bias, "bias"), (rowbias, "rowbias"), (residual, "residual")):
        if opt is not None:
            _dev(opt, nm)
    if isinstance(out, SplitAct) and batch == 1:
        _split_out_ok(out, M)
    a_split, w_split = is_split(a, w), is_split(w, a)
    assert not is_x2_weight(a), "a pack.split_f16 weight is the W operand"
    if isinstance(w, X2Weight):
        # two-pass f16 (dtype 4): plain f16 activation rows (GroupNorm / LayerNorm / GEGLU-epilogue output) x a pack.split_f16 weight (which carries its 1 / scale)
        assert is_x2_weight(w), "a two-pass weight without its scale"
        assert a.dtype == torch.float16 and not isinstance(a, SplitAct), "a pack.split_f16 weight multiplies plain float16 activation rows (the two-pass form has no raw-f32 launch)"
        assert out.dtype in (torch.float16, torch.float32) and not isinstance(out, SplitAct) and not out_nchw, "the two-pass f16 GEMM writes plain f32 rows or plain f16 rows"
        assert ldw % 2 == 0 and w_bs % 2 == 0
        a_split, w_split = 2, True
        code = F16X2
        alpha = alpha * w._x2_alpha
        ldw, w_bs = ldw // 2, w_bs // 2
    elif isinstance(a, SplitAct) or isinstance(w, SplitAct):     # pre-split activations x pre-split weights (bf16 storage, 4 bytes per K element)
        assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and lda % 2 == 0 and ldw % 2 == 0 and a_bs % 2 == 0 and w_bs % 2 == 0
        a_split = w_split = True
        code = BF16X3
        lda, a_bs, ldw, w_bs = lda // 2, a_bs // 2, ldw // 2, w_bs // 2
    elif a_split or w_split:
        code = BF16X3
        if a_split:
            assert lda % 2 == 0 and a_bs % 2 == 0
            lda, a_bs = lda // 2, a_bs // 2          # -> K elements (4 bytes each)
        else:
            assert ldw % 2 == 0 and w_bs % 2 == 0
            ldw, w_bs = ldw // 2, w_bs // 2
    else:
        assert a.dtype == w.dtype, (a.dtype, w.dtype)
        code = dt_code(a.dtype)
        if x3:
            assert a.dtype == torch.float32, "x3=True multiplies two f32 operands with the bf16x3 scheme"
            code = BF16X3
    p = ConvGemm()
    p.A, p.W, p.O = a.data_ptr(), w.data_ptr(), out.data_ptr()
    p.bias, p.rowbias, p.R = _ptr(bias), _ptr(rowbias), _ptr(residual)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous()
    if rowbias is not None:
        assert rowbias.dtype == torch.float32 and rowbias.dim() == 2 and rowbias.stride(1) == 1
        p.ldrb = rowbias.stride(0)
    if residual is not None:
        assert residual.dtype == (torch.float32 if isinstance(out, SplitAct) else out.dtype)      # (a SplitAct is f32 values in bf16 storage)
    p.lda, p.ldw, p.ldo, p.ldr = lda, ldw, ldo, ldr
    p.a_bs, p.w_bs, p.o_bs, p.r_bs = a_bs, w_bs, o_bs, r_bs
    p.M, p.N, p.K, p.batch, p.Cin = M, N, K, batch, Cin
    p.T, p.Hin, p.Win, p.Hout, p.Wout = T, Hin, Win, Hout, Wout
    p.KT, p.KH, p.KW, p.pt, p.ph, p.pw, p.stride, p.ups = KT, KH, KW, pt, ph, pw, stride, ups
    p.rowbias_div, p.bias_per_row, p.act = rowbias_div, int(bias_per_row), act
    p.dtype, p.out_dtype, p.out_nchw, p.tile_hint = code, (F32 if code == F16X2 else dt_code(out.dtype)), int(out_nchw), tile_hint
    p.alpha, p.split_k = alpha, split_k
    p.debug_ablate = DEBUG_ABLATE | (0 if EPI_WIDE else 64)
    p.a_split, p.w_split = int(a_split), int(w_split)
    p.o_split = 1 if isinstance(out, SplitAct) else 2 if (code == F16X2 and out.dtype == torch.float16) else 0
    if p.o_split == 1:
        assert code == BF16X3, "pre-split (bf16 hi | lo) outputs come from bf16x3 launches"
        assert ldo % 2 == 0 and o_bs % 2 == 0
        p.ldo, p.o_bs, p.out_dtype = ldo // 2, o_bs // 2, F32
    elif p.o_split == 2:            # plain f16 rows (clamped): ldo / o_bs stay in f16 elements
        assert residual is None and rowbias is None and not bias_per_row and act in (0, 2), "the f16-row epilogue of the two-pass GEMM: column bias (+ GEGLU) only"
    p.gn_colsum = 0
    p.sat_count = _ptr(SAT_COUNTER) if p.o_split == 2 else 0
    ws, zeros = workspace(a.device)
    p.workspace, p.workspace_bytes, p.zeros = ws.data_ptr(), ws.numel(), zeros.data_ptr()
    return p


def conv_gemm_plan(p):
    """What geo4d_conv_gemm would launch for this descriptor (_lib.ConvGemmPlan); raises where the launch would refuse it."""
    plan = ConvGemmPlan()
    _lib.check(_lib.load().geo4d_conv_gemm_plan(C.byref(p), C.byref(plan)), "geo4d_conv_gemm_plan")
    return plan


def _plan_on(p, tile_hint, split_k):
    """The plan of `p` launched on (tile_hint, split_k), or None where the library refuses that."""
    p.tile_hint, p.split_k = tile_hint, split_k
    plan = ConvGemmPlan()
    return plan if _lib.load().geo4d_conv_gemm_plan(C.byref(p), C.byref(plan)) == 0 else None


def _launch_config(p, launch, plan_on=_plan_on):
    """(tile_hint, split_k) of a launch that names neither: the tuning table's entry (own or borrowed), else measured now where that is
    allowed, else (0, 0) = the library's choice. `plan_on(p, tile, split)`: the plan query of the entry point that launches `p`."""
    def may_measure():
        return AUTOTUNE and not torch.cuda.is_current_stream_capturing()
    key = f"{p.dtype}/{p.out_dtype}|{p.M}x{p.N}x{p.K}|c{p.Cin}|t{p.KT}{p.KH}{p.KW}s{p.stride}u{p.ups}|a{p.act}r{int(bool(p.R))}n{p.out_nchw}|b{p.batch}"
    if p.dtype in (BF16X3, F16X2):
        key += f"|x{int(bool(p.a_split))}{p.w_split}" + ("o" if p.o_split else "")       # (dtype 4's "o" = its f16 rows)
    cfg = _tuned_config(_tune_table(), key, p.dtype, p.a_split, p.w_split, p.o_split, may_measure)
    if cfg is None and may_measure():
        cfg = _autotune(launch, key, lambda tile, split: plan_on(p, tile, split) is not None)
    cfg = cfg if cfg is not None else (0, 0)
    return _f16_rows_config(cfg, p.act) if p.o_split == 2 else cfg


def _offer_colsums(p, out, tile_hint, split_k):
    """The consumer GroupNorm's statistics pass, for free: per row block and column (sum, sum of squares) from the epilogue. The plan says
    how many rows one entry of THIS launch covers (32 for the first generation, the wave tile's rows for the second / third; 0 = this
    configuration cannot emit them - split-K, activations, unaligned rows: the GroupNorm then runs its own pass). Attaches the sums to
    `out` and `p` where the launch emits them; returns the (tile_hint, split_k) to launch."""
    def rows_on(tile, split):       # (a refused configuration offers nothing: the launch reports the refusal)
        return getattr(_plan_on(p, tile, split), "colsum_rows", 0)
    # what decides is the generation of the hint ASKED for (hint 0, the library's choice, counts as the first), not of the tile the plan runs
    rows = rows_on(tile_hint, split_k) if (_generation(tile_hint) > 1 or int(GN_FUSED_STATS) >= 2) else 0
    if split_k > 1 and not SPLITK_COLSUM:      # (A/B switch: round 6 lets a split-K launch's reduce kernel emit the sums)
        rows = 0
    if rows == 0 and int(GN_FUSED_STATS) >= 2:
        # mode 2 (A/B, tests): a tuned configuration that cannot emit the sums (split-K; a second / third generation tile on 16-bit rows)
        # gives way to an un-split first-generation launch, as this path did before round 4
        first = (tile_hint if _generation(tile_hint) == 1 else 0), 1
        rows = rows_on(*first)
        if rows > 0:
            tile_hint, split_k = first
    if rows > 0:
        split_k = split_k or 1           # (the library's own tile choice may not split a launch that emits the sums)
        cs = torch.empty((p.M // rows, p.N, 2), device=out.device, dtype=torch.float32)
        p.gn_colsum = cs.data_ptr()
        out._gn_colsum, out._gn_colsum_rows = cs, rows
        out._gn_colsum_tag = (out.data_ptr(), out._version)      # groupnorm() ignores the sums if the buffer was rewritten by torch since
    return tile_hint, split_k


def conv_gemm(a, w, out, *, tile_hint=0, split_k=0, gn_stats=False, **problem):
    """out = epilogue(alpha * gather(a) . w^T): `problem` = the keyword arguments of conv_gemm_descriptor. `tile_hint` / `split_k` both 0:
    the tuning table decides. `gn_stats`: offer the consumer GroupNorm this launch's column sums (out._gn_colsum)."""
    lib = _lib.load()
    p = conv_gemm_descriptor(a, w, out, tile_hint=tile_hint, split_k=split_k, **problem)
    if getattr(out, "_gn_colsum", None) is not None:       # sums of an EARLIER launch into this tensor object: this launch either sets fresh ones or leaves none
        out._gn_colsum, out._gn_colsum_rows, out._gn_colsum_tag = None, 32, None

    def launch(tile, split):
        p.tile_hint, p.split_k = tile, split
        _lib.check(lib.geo4d_conv_gemm(C.byref(p), _stream()), "geo4d_conv_gemm")

    if tile_hint == 0 and split_k == 0:
        tile_hint, split_k = _launch_config(p, launch)
    if gn_stats and GN_FUSED_STATS and not p.o_split and p.batch == 1 and out.dim() == 2 and out.shape[0] == p.M:
        tile_hint, split_k = _offer_colsums(p, out, tile_hint, split_k)
    if GEMM_TIMELINE is None:
        launch(tile_hint, split_k)
    else:
        _on_timeline(GEMM_TIMELINE, lambda: launch(tile_hint, split_k), 2.0 * p.M * p.N * p.K * p.batch, {BF16X3: 3, F16X2: 2}.get(p.dtype, 1))
    return out


def _out_dtype(x, out_dtype, w=None):
    """Default output dtype of a GEMM: f32 rows for the 4-byte modes' operand formats (a SplitAct, or f16 rows against a two-pass weight)."""
    return out_dtype or (torch.float32 if (isinstance(x, SplitAct) or (w is not None and is_x2_weight(w))) else x.dtype)


def linear(x, w, bias=None, *, residual=None, act=0, out=None, out_dtype=None, alpha=1.0, tile_hint=0, split_k=0, gn_stats=False,
           split_out=False):
    """x [M, K] (row pitch free), w packed [N, K]; GEGLU (act=2) returns [M, N/2]. `split_out` (bf16x3): the result is written as a
    SplitAct (the next GEMM's pre-split A operand)."""
    M, K = x.shape[0], act_k(x)
    N = w.shape[0]
    assert kdim(w, x) == K, (w.shape, x.shape)
    if out is None:
        nout = N // 2 if act == 2 else N
        out = new_split(M, nout, x.device, split_fmt(split_out)[1]) if split_out else torch.empty((M, nout), device=x.device, dtype=_out_dtype(x, out_dtype, w))
    return conv_gemm(x, w, out, M=M, N=N, K=K, Cin=K, lda=_ld(x), ldw=_ld(w), ldo=_ld(out), bias=bias,
                     residual=residual, ldr=_ld(residual) if residual is not None else 0, act=act, alpha=alpha,
                     tile_hint=tile_hint, split_k=split_k, gn_stats=gn_stats)


def conv2d(x, w, bias, *, F, Hin, Win, KH, KW, stride=1, pad=0, pad_end=0, ups=1, T=1, rowbias=None, rowbias_div=0,
           residual=None, act=0, out=None, out_dtype=None, out_nchw=False, nchw_channels=None, tile_hint=0, split_k=0, gn_stats=False):
    """x tokens [F*Hin*Win, Cin]; w packed [N, KH*KW*Cin]. Output tokens [F*Hout*Wout, N], or with out_nchw a
    [B, C, T, Hout, Wout] tensor (`out` may be a channel-offset view of a wider tensor with `nchw_channels` channels).
    `pad_end` = extra zero rows / columns at the bottom / right only (ae_modules.py:102-106 pads (0,1,0,1) before its
    stride-2 conv): the gather treats every out-of-image tap as zero, so only the output size changes."""
    Cin = act_k(x)
    N = w.shape[0]
    Hs, Ws = Hin * ups, Win * ups
    Hout = (Hs + 2 * pad + pad_end - KH) // stride + 1
    Wout = (Ws + 2 * pad + pad_end - KW) // stride + 1
    M = F * Hout * Wout
    assert x.shape[0] == F * Hin * Win, (x.shape, F, Hin, Win)
    assert kdim(w, x) == KH * KW * Cin, (w.shape, KH, KW, Cin)
    if out is None:
        if out_nchw:
            out = torch.empty((F // T, N, T, Hout, Wout), device=x.device, dtype=out_dtype or torch.float32)
        else:
            out = torch.empty((M, N), device=x.device, dtype=_out_dtype(x, out_dtype, w))
    conv_gemm(x, w, out, M=M, N=N, K=KH * KW * Cin, Cin=Cin, lda=_ld(x), ldw=_ld(w), ldo=(nchw_channels or N) if out_nchw else _ld(out), T=T,
              Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, KH=KH, KW=KW, ph=pad, pw=pad, stride=stride, ups=ups, bias=bias,
              rowbias=rowbias, rowbias_div=rowbias_div, residual=residual,
              ldr=_ld(residual) if residual is not None else 0, act=act, out_nchw=out_nchw, tile_hint=tile_hint,
              split_k=split_k, gn_stats=gn_stats)
    return out, Hout, Wout


# Nearest-2x + 3x3 convolutions (the Upsample layers) in their sub-pixel form: four 2x2 convolutions on the source grid, 4 / 9 of the
# multiplications of conv2d(ups=2) in the same three bf16 passes (include/geo4d_hip.h geo4d_conv_gemm_up2). GEO4D_UP_SUBPIXEL=0 keeps every
# call site on the gather form (A/B runs in one build). Measured on MI355X (profiles/upsample_subpixel.md section 2, us per conv, gather ->
# sub-pixel): U-Net 10x16 776 -> 288, 20x32 688 -> 298; VAE decoder (48 frames) 5041 -> 2505, 21173 -> 10267, 22410 -> 11375.
UP_SUBPIXEL = _env_level("GEO4D_UP_SUBPIXEL", 1)
# "batch": one launch, the phase in the batch index; "phases": four launches - never faster, and 2.4 - 7.6x slower at the U-Net's sources,
# where a phase alone under-fills the chip
UP2_FORM = _os.environ.get("GEO4D_UP2_FORM", "batch")
# source rows (F H W) below which the gather form stays. The U-Net's 5x8 source (640 rows) is 1.39x faster alone (239 -> 172 us, weights
# resident in the last-level cache) but SLOWER inside a replayed step (185 -> 202 us in the kernel trace): its four weights are 16/9 of
# the bytes and the launch is weight-bound. The next level (2560 rows) wins in both.
UP2_MIN_ROWS = 2048
_UP2_TILES = (22, 23, 25, 71, 72)
_UP2_SUMS_TILE = {71: 22}      # the 96-row blocks of tile 71 straddle frames of 2560 k source rows; tile 22 (64) was within 1.5 % of it wherever 71 won


def up_subpixel(x, w4, rows):
    """Does an Upsample conv of `rows` source rows run in the sub-pixel form? `w4`: its pack.pack_conv2d_up2 weight, None where the mode has none."""
    return bool(UP_SUBPIXEL) and w4 is not None and rows >= UP2_MIN_ROWS and (isinstance(x, SplitAct) or x.dtype == torch.float32)


def _up2_plan_on(p, src_w, phase):
    def plan_on(p_, tile_hint, split_k):
        if split_k != 1 or tile_hint not in _UP2_TILES:
            return None
        p_.tile_hint, p_.split_k = tile_hint, 1
        plan = ConvGemmPlan()
        return plan if _lib.load().geo4d_conv_gemm_up2_plan(C.byref(p_), src_w, phase, C.byref(plan)) == 0 else None
    return plan_on


def conv2d_up2(x, w4, bias, *, F, Hin, Win, out=None, gn_stats=False, tile_hint=0, form=None):
    """conv2d(x, w, bias, KH=3, KW=3, pad=1, ups=2) from the folded weight `w4` = pack.pack_conv2d_up2(w): [4, N, 4 Cin] in the bf16x3 operand
    format, phase 2 py + px major. x tokens [F*Hin*Win, Cin] (f32 rows or a SplitAct, shared by the four phases); returns (tokens
    [F*2Hin*2Win, N] f32, 2 Hin, 2 Win). `form`: UP2_FORM. `gn_stats`: as conv_gemm (one sum buffer for the four phases)."""
    lib = _lib.load()
    Cin, N, M = act_k(x), w4.shape[1], F * Hin * Win
    assert w4.dim() == 3 and w4.shape[0] == 4 and w4.stride(2) == 1 and kdim(w4[0], x) == 4 * Cin, (w4.shape, Cin)
    assert x.shape[0] == M, (x.shape, F, Hin, Win)
    if out is None:
        out = torch.empty((4 * M, N), device=x.device, dtype=torch.float32)
    assert out.dim() == 2 and out.shape[0] == 4 * M and out.dtype == torch.float32 and not isinstance(out, SplitAct)
    batched = (form or UP2_FORM) == "batch"
    p = conv_gemm_descriptor(x, w4[0], out, M=M, N=N, K=4 * Cin, Cin=Cin, lda=_ld(x), ldw=w4.stride(1), ldo=_ld(out), Hin=Hin, Win=Win,
                             Hout=Hin, Wout=Win, KH=2, KW=2, ph=1, pw=1, bias=bias, batch=4 if batched else 1,
                             w_bs=w4.stride(0) if batched else 0, tile_hint=tile_hint, split_k=1)
    if getattr(out, "_gn_colsum", None) is not None:
        out._gn_colsum, out._gn_colsum_rows, out._gn_colsum_tag = None, 32, None
    phases = (-1,) if batched else (0, 1, 2, 3)

    def launch(tile, split):
        p.tile_hint, p.split_k = tile, 1
        for ph in phases:
            if ph >= 0:
                p.W, p.ph, p.pw = w4[ph].data_ptr(), 1 - (ph >> 1), 1 - (ph & 1)
            _lib.check(lib.geo4d_conv_gemm_up2(C.byref(p), Win, ph, _stream()), "geo4d_conv_gemm_up2")

    plan_on = _up2_plan_on(p, Win, phases[0])
    if tile_hint == 0:
        tile_hint = _launch_config(p, launch, plan_on)[0] or (72 if M >= 8192 else 25)
    if gn_stats and GN_FUSED_STATS:
        rows = getattr(plan_on(p, tile_hint, 1), "colsum_rows", 0)
        if rows == 0 and tile_hint in _UP2_SUMS_TILE:      # the consumer's statistics pass over the up-sampled map costs more than the tile gains
            rows = getattr(plan_on(p, _UP2_SUMS_TILE[tile_hint], 1), "colsum_rows", 0)
            tile_hint = _UP2_SUMS_TILE[tile_hint] if rows > 0 else tile_hint
        if rows > 0:
            cs = torch.empty((4 * M // rows, N, 2), device=out.device, dtype=torch.float32)
            p.gn_colsum = cs.data_ptr()
            out._gn_colsum, out._gn_colsum_rows = cs, rows
            out._gn_colsum_tag = (out.data_ptr(), out._version)
    if GEMM_TIMELINE is None:
        launch(tile_hint, 1)
    else:
        _on_timeline(GEMM_TIMELINE, lambda: launch(tile_hint, 1), 2.0 * 4 * M * N * p.K, 3)
    return out, 2 * Hin, 2 * Win


def conv_temporal(x, w, bias, *, B, T, HW, residual=None, out=None, gn_stats=False, tile_hint=0, split_k=0):
    """nn.Conv3d kernel (3,1,1), padding (1,0,0) on tokens [(b t) hw, C]; w packed [N, 3*C]."""
    Cin = act_k(x)
    N = w.shape[0]
    M = B * T * HW
    assert x.shape[0] == M and kdim(w, x) == 3 * Cin
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=_out_dtype(x, None, w))
    return conv_gemm(x, w, out, M=M, N=N, K=3 * Cin, Cin=Cin, lda=_ld(x), ldw=_ld(w), ldo=_ld(out), T=T, Hin=HW, Win=1,
                     Hout=HW, Wout=1, KT=3, pt=1, bias=bias, residual=residual,
                     ldr=_ld(residual) if residual is not None else 0, gn_stats=gn_stats, tile_hint=tile_hint, split_k=split_k)


def batched_gemm(a, b, out, *, batch, M, N, K, a_bs, b_bs, o_bs, bias=None, bias_per_row=False, alpha=1.0, x3=False):
    """out[z] = alpha * a[z] @ b[z]^T (+bias); a [.., K] rows, b [.., K] rows (both K-major). `x3`: both operands are f32
    activations to be multiplied with the bf16x3 scheme (the VAE AttnBlock GEMMs of the bf16x3 mode)."""
    return conv_gemm(a, b, out, M=M, N=N, K=K, Cin=K, lda=_ld(a), ldw=_ld(b), ldo=_ld(out), batch=batch, a_bs=a_bs,
                     w_bs=b_bs, o_bs=o_bs, bias=bias, bias_per_row=bias_per_row, alpha=alpha, x3=x3)


_gn_ws = {}


def _gn_sums(t, stat_rows):
    """-> (colsum tensor, rows per entry) a GEMM launch left on this very tensor object, or None: absent, stale (the tensor was modified in
    place or re-viewed after the GEMM wrote it) or with blocks that straddle two statistics."""
    cs = getattr(t, "_gn_colsum", None)
    if cs is None or getattr(t, "_gn_colsum_tag", None) != (t.data_ptr(), t._version):
        return None
    rows = getattr(t, "_gn_colsum_rows", 32)
    if stat_rows % rows or tuple(cs.shape) != (t.shape[0] // rows, t.shape[1], 2):
        return None
    return cs, rows


def concat_parts(buf, left, right):
    """Record on a channel-concatenation buffer the two column views its producers write (FUSED_CONCAT): the GroupNorm that reads `buf`
    takes its statistics from the sums the two producing GEMM launches leave on those view objects."""
    buf._gn_parts = (left, right)


def _gn_sources(x, stat_rows):
    one = _gn_sums(x, stat_rows)
    if one is not None:
        return [(one[0], one[1], 0, x.shape[1])]
    parts = getattr(x, "_gn_parts", None)
    if not parts or not GN_ONE_LAUNCH:
        return []
    src, c0 = [], 0
    for v in parts:     # the views must still be the columns of x, in order, and carry fresh sums
        if v.dim() != 2 or v.shape[0] != x.shape[0] or v.stride() != x.stride() or v.data_ptr() != x.data_ptr() + c0 * x.element_size():
            return []
        sums = _gn_sums(v, stat_rows)
        if sums is None:
            return []
        src.append((sums[0], sums[1], c0, v.shape[1]))
        c0 += v.shape[1]
    return src if c0 == x.shape[1] else []


def _gn_descriptor(x, out, gamma, beta, *, F, HW, eps, groups, frames_per_stat, silu, split_out, sources, path):
    q = GroupNorm2()
    p = q.base
    p.x, p.y, p.gamma, p.beta = x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    p.ldx, p.ldy = _ld(x), (_ld(out) // 2 if split_out == 1 else _ld(out))
    p.split_out = int(split_out)
    p.sat_count = _ptr(SAT_COUNTER) if split_out == 2 else 0
    p.F, p.HW, p.C, p.groups, p.frames_per_stat = F, HW, x.shape[1], groups, frames_per_stat
    p.act, p.dtype, p.eps = int(silu), dt_code(x.dtype), eps
    q.nsrc = len(sources)
    for i, (cs, rows, c0, nc) in enumerate(sources):
        q.src[i].colsum, q.src[i].rows, q.src[i].c0, q.src[i].channels = cs.data_ptr(), rows, c0, nc
    q.path = path
    q.fuse_fraction, q.min_workgroups = GN_TUNE
    return q


def groupnorm_plan(q):
    """What geo4d_groupnorm2 would launch for this descriptor (_lib.GroupNormPlan); raises where the launch would refuse it."""
    plan = GroupNormPlan()
    _lib.check(_lib.load().geo4d_groupnorm_plan(C.byref(q), C.byref(plan)), "geo4d_groupnorm_plan")
    return plan


def groupnorm(x, gamma, beta, *, F, HW, eps, groups=32, frames_per_stat=1, silu=False, out=None, split_out=False, path=None):
    """`split_out` (f32 input of the bf16x3 mode): y is returned as a SplitAct, the pre-split A operand of the conv that follows -
    True / "bf16": bf16 hi | lo (three-pass bf16x3 consumer); "f16": f16 hi | lo (two-pass f16 consumer, pack.split_f16 weights).
    `path` (tests, tools): one of _lib.GN_PATH_*; default: GN_ONE_LAUNCH decides (the library's plan, or the two-launch sequence)."""
    lib = _lib.load()
    _dev(x, "x")
    assert not isinstance(x, SplitAct), "GroupNorm reads plain activations"
    Cc = x.shape[1]
    assert x.shape[0] == F * HW, (x.shape, F, HW)
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32
    if out is None:
        out = new_split(F * HW, Cc, x.device, split_fmt(split_out)[1]) if split_out else torch.empty((F * HW, Cc), device=x.device, dtype=x.dtype)
    split_out = 1 if isinstance(out, SplitAct) else 2 if (out.dtype == torch.float16 and x.dtype == torch.float32) else 0
    if split_out:
        assert x.dtype == torch.float32, "the GEMM-operand producer formats are written from f32 activations"
    if split_out == 1:
        _split_out_ok(out, F * HW)
    if path is None:
        path = {0: _lib.GN_PATH_COLS, 3: _lib.GN_PATH_FUSED, 4: _lib.GN_PATH_SLICED}.get(int(GN_ONE_LAUNCH), _lib.GN_PATH_AUTO)
    sources = _gn_sources(x, frames_per_stat * HW)
    if not sources:
        path = _lib.GN_PATH_PARTIAL
    q = _gn_descriptor(x, out, gamma, beta, F=F, HW=HW, eps=eps, groups=groups, frames_per_stat=frames_per_stat, silu=silu,
                       split_out=split_out, sources=sources, path=path)
    need = groupnorm_plan(q).workspace_bytes          # the same host function the launch runs: they cannot disagree
    if need:
        ws = torch.empty(need, device=x.device, dtype=torch.uint8)
        q.base.workspace, q.base.workspace_bytes = ws.data_ptr(), need
    _lib.check(lib.geo4d_groupnorm2(C.byref(q), _stream()), "geo4d_groupnorm2")
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None, split_out=False):
    lib = _lib.load()
    _dev(x, "x")
    assert not isinstance(x, SplitAct), "LayerNorm reads plain activations"
    M, Cc = x.shape
    if split_out or isinstance(out, SplitAct) or (out is not None and out.dtype == torch.float16 and x.dtype == torch.float32):
        assert x.dtype == torch.float32
        if out is None:
            out = new_split(M, Cc, x.device, split_fmt(split_out)[1])
        if isinstance(out, SplitAct):
            _split_out_ok(out, M)
            _lib.check(lib.geo4d_layernorm_split(x.data_ptr(), _ld(x), out.data_ptr(), _ld(out) // 2, M, Cc, eps, gamma.data_ptr(),
                                                 beta.data_ptr(), 1, 0, _stream()), "geo4d_layernorm_split")
        else:           # plain f16 rows: the two-pass GEMM's A operand
            assert out.dtype == torch.float16
            _lib.check(lib.geo4d_layernorm_split(x.data_ptr(), _ld(x), out.data_ptr(), _ld(out), M, Cc, eps, gamma.data_ptr(),
                                                 beta.data_ptr(), 2, _ptr(SAT_COUNTER), _stream()), "geo4d_layernorm_split")
        return out
    if out is None:
        out = torch.empty((M, Cc), device=x.device, dtype=x.dtype)
    _lib.check(lib.geo4d_layernorm(x.data_ptr(), _ld(x), out.data_ptr(), _ld(out), M, Cc, eps, gamma.data_ptr(),
                                   beta.data_ptr(), dt_code(x.dtype), _stream()), "geo4d_layernorm")
    return out


def softmax_rows(x, scale, out_dtype, out=None, causal_period=0):
    """softmax(scale * x) per row of fp32 scores; `out` may be a wider zero-initialised buffer (K padding of the next GEMM);
    `causal_period` > 0: row r only sees columns <= r % causal_period (text-transformer mask)."""
    lib = _lib.load()
    _dev(x, "x")
    assert x.dtype == torch.float32
    rows, cols = x.shape
    if out is None:
        out = torch.empty((rows, cols), device=x.device, dtype=out_dtype)
    if causal_period:
        _lib.check(lib.geo4d_softmax_rows_causal(x.data_ptr(), _ld(x), out.data_ptr(), _ld(out), rows, cols, scale,
                                                 dt_code(out.dtype), causal_period, _stream()), "geo4d_softmax_rows_causal")
    else:
        _lib.check(lib.geo4d_softmax_rows(x.data_ptr(), _ld(x), out.data_ptr(), _ld(out), rows, cols, scale,
                                          dt_code(out.dtype), _stream()), "geo4d_softmax_rows")
    return out


ATTN_VARIANT = int(_os.environ.get("GEO4D_ATTN_VARIANT", "0"))   # 0 = library default; 1..3 = A/B builds (include/geo4d_hip.h)


def attention_descriptor(q, kv, *, B, H, Nq, scale, out=None, x3=False, variant=None, split_out=False, qkv_split=False):
    """(geo4d_attention_t of the launch `attention` makes for these arguments, its output tensor)."""
    if qkv_split:
        assert len(kv) == 1 and all(isinstance(t, SplitAct) for t in (q, kv[0][0], kv[0][1])), "qkv_split takes SplitAct q / k / vt of one key/value set"
        assert q.dtype == torch.bfloat16
    per = 2 if qkv_split else 1       # a SplitAct holds 2 bf16 per element: torch's strides count bf16, the library's ld* / vt_bs elements
    _dev(q, "q", qkv_split)
    if out is None:
        out = new_split(B * Nq, H * 64, q.device) if split_out else torch.empty((B * Nq, H * 64), device=q.device, dtype=torch.float32 if qkv_split else q.dtype)
    split_out = isinstance(out, SplitAct)
    if split_out:
        _split_out_ok(out, B * Nq)
    p = Attention()
    p.q, p.o, p.ldq, p.ldo = q.data_ptr(), out.data_ptr(), _ld(q) // per, (_ld(out) // 2 if split_out else _ld(out))
    p.split_out, p.qkv_split = int(split_out), int(qkv_split)
    assert 1 <= len(kv) <= 2
    for i, (k, vt, nk, div, vt_bs) in enumerate(kv):
        assert k.dtype == q.dtype and vt.dtype == q.dtype
        _dev(k, "k", qkv_split); _dev(vt, "vt", qkv_split)
        assert all(n % per == 0 for n in (_ld(q), _ld(k), _ld(vt), vt_bs))
        p.k[i], p.vt[i], p.ldk[i], p.ldvt[i], p.vt_bs[i], p.Nk[i], p.kv_div[i] = k.data_ptr(), vt.data_ptr(), _ld(k) // per, _ld(vt) // per, vt_bs // per, nk, div
    p.zeros = workspace(q.device)[1].data_ptr()
    if x3 and not qkv_split:
        assert q.dtype == torch.float32, "x3 attention runs on f32 q / k / v^T"
    code = BF16X3 if (x3 or qkv_split) else dt_code(q.dtype)
    p.B, p.H, p.Nq, p.nseg, p.head_dim, p.dtype, p.scale = B, H, Nq, len(kv), 64, code, scale
    p.variant = ATTN_VARIANT if variant is None else variant
    return p, out


def attention_plan(p):
    """What geo4d_attention would launch for this descriptor (_lib.AttentionPlan); raises where the launch would refuse it."""
    plan = AttentionPlan()
    _lib.check(_lib.load().geo4d_attention_plan(C.byref(p), C.byref(plan)), "geo4d_attention_plan")
    return plan


def attention(q, kv, *, B, H, Nq, scale, out=None, x3=False, variant=None, split_out=False, qkv_split=False):
    """q [B*Nq, >=H*64] view; kv = list of (k, vt, Nk, kv_div, vt_bs): k [(B/kv_div)*Nk, >=H*64] view, vt = V TRANSPOSED
    as a [>=H*64, ld] view (row = channel, column = key) whose batch b' starts vt_bs elements after batch b'-1.
    `qkv_split` (bf16x3, one key/value set): q, k and vt are SplitAct views (bf16, 2 per element: what the projections wrote with
    split_out=True), strides / vt_bs in bf16 elements as torch reports them."""
    lib = _lib.load()
    p, out = attention_descriptor(q, kv, B=B, H=H, Nq=Nq, scale=scale, out=out, x3=x3, variant=variant, split_out=split_out, qkv_split=qkv_split)
    _launch_attention(lib, p)
    return out


def _launch_attention(lib, p):
    def launch():
        _lib.check(lib.geo4d_attention(C.byref(p), _stream()), "geo4d_attention")
    if ATTN_TIMELINE is not None and p.nseg == 1:
        _on_timeline(ATTN_TIMELINE, launch, 4.0 * p.B * p.H * p.Nq * p.Nk[0] * 64, 3 if p.dtype == BF16X3 else 1)
    else:
        launch()


def linear_t_batched(w, x, batch, rows, dtype_align=None, split_out=False):
    """Per-batch operand-swapped projection: x [batch*rows, K] -> out [batch, N, rows_pad] with out[b, n, m] =
    sum_k w[n, k] x[b*rows + m, k]; rows_pad = rows rounded up to a 16-byte multiple (zero filled). This is V^T per frame.
    `split_out` (bf16x3, pre-split x): out is a SplitAct [batch, N, 2*rows_pad] (rows_pad a multiple of 8) - V^T in the format the
    attention kernel takes with qkv_split."""
    N, K = w.shape[0], kdim(w, x)
    if split_out:
        assert isinstance(x, SplitAct)
        rp = (rows + 7) // 8 * 8
        out = SplitAct.wrap((torch.zeros if rp != rows else torch.empty)((batch, N, 2 * rp), device=x.device, dtype=torch.bfloat16))
        conv_gemm(w, x, out, M=N, N=rows, K=K, Cin=K, lda=_ld(w), ldw=_ld(x), ldo=2 * rp, batch=batch, a_bs=0, w_bs=rows * _ld(x), o_bs=N * 2 * rp)
        return out, rp
    odt = _out_dtype(x, None)
    epc = 4 if odt == torch.float32 else 8
    rp = (rows + epc - 1) // epc * epc
    out = (torch.zeros if rp != rows else torch.empty)((batch, N, rp), device=x.device, dtype=odt)
    conv_gemm(w, x, out, M=N, N=rows, K=K, Cin=K, lda=_ld(w), ldw=_ld(x), ldo=rp, batch=batch, a_bs=0, w_bs=rows * _ld(x), o_bs=N * rp)
    return out, rp


def linear_t(w, x, bias=None, *, out=None, pad_cols=None):
    """Operand-swapped projection: out[n, m] = sum_k w[n, k] * x[m, k] (+ bias[n]) -> [N, M]: the transposed layout the
    attention kernel wants for V. `pad_cols`: allocate zero-filled columns up to this count (16-byte row alignment)."""
    N, K = w.shape[0], kdim(w, x)
    M = x.shape[0]
    if out is None:
        cols = pad_cols or M
        odt = _out_dtype(x, None)
        out = torch.zeros((N, cols), device=x.device, dtype=odt) if cols != M else torch.empty((N, M), device=x.device, dtype=odt)
    return conv_gemm(w, x, out, M=N, N=M, K=K, Cin=K, lda=_ld(w), ldw=_ld(x), ldo=_ld(out), bias=bias, bias_per_row=True)


def temporal_attention(q, k, v, *, B, T, HW, H, scale, out=None, split_out=False):
    lib = _lib.load()
    _dev(q, "q")
    if out is None:
        out = new_split(B * T * HW, H * 64, q.device) if split_out else torch.empty((B * T * HW, H * 64), device=q.device, dtype=q.dtype)
    split_out = isinstance(out, SplitAct)
    _dev(k, "k"); _dev(v, "v")
    if split_out:
        _split_out_ok(out, B * T * HW)
    _lib.check(lib.geo4d_temporal_attention2(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), out.data_ptr(),
                                             _ld(out) // 2 if split_out else _ld(out), B, T, HW, H, 64, scale, dt_code(q.dtype),
                                             int(split_out), _stream()), "geo4d_temporal_attention")
    return out


def tokens_from_ncthw(src0, src1, cpad, dtype):
    """[B,C0,T,H,W] (+[B,C1,T,H,W]) fp32 -> tokens [(b t) h w, cpad] of `dtype`, zero padded channels."""
    lib = _lib.load()
    _dev(src0, "src0")
    assert src0.dtype == torch.float32 and src0.is_contiguous()
    B, C0, T, H, W = src0.shape
    C1 = 0
    if src1 is not None:
        assert src1.dtype == torch.float32 and src1.is_contiguous() and src1.shape[0] == B and src1.shape[2:] == src0.shape[2:]
        C1 = src1.shape[1]
    out = torch.empty((B * T * H * W, cpad), device=src0.device, dtype=dtype)
    _lib.check(lib.geo4d_tokens_from_ncthw(src0.data_ptr(), C0, _ptr(src1), C1, out.data_ptr(), cpad, B, T, H * W,
                                           dt_code(dtype), _stream()), "geo4d_tokens_from_ncthw")
    return out


def cast_f16(x, out=None):
    """f32 rows [M, C] -> plain f16 rows (clamped, NaN kept): the two-pass GEMM's A operand made from a tensor without a normalising producer
    (bf16x3m class "vaeup": the VAE decoder's stream in front of its upsampling convolutions)."""
    lib = _lib.load()
    _dev(x, "x")
    assert x.dtype == torch.float32 and x.dim() == 2
    M, Cc = x.shape
    if out is None:
        out = torch.empty((M, Cc), device=x.device, dtype=torch.float16)
    _lib.check(lib.geo4d_cast_rows_f16(x.data_ptr(), _ld(x), out.data_ptr(), _ld(out), M, Cc, _ptr(SAT_COUNTER), _stream()), "geo4d_cast_rows_f16")
    return out


def presplit(x):
    """f32 rows [M, C] -> SplitAct (the bf16x3 pre-split operand format): conv_gemm then skips its in-register split of the A fragments (12-29 %
    of a launch, paid per K slab and wave). Worth its own pass only where every input element is used many times: the 3x3 Upsample convolutions."""
    lib = _lib.load()
    _dev(x, "x")
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] % 8 == 0
    M, Cc = x.shape
    out = new_split(M, Cc, x.device)
    _lib.check(lib.geo4d_split_rows_bf16(x.data_ptr(), _ld(x), out.data_ptr(), _ld(out) // 2, M, Cc, _stream()), "geo4d_split_rows_bf16")
    return out


def concat_channels(a, b):
    lib = _lib.load()
    _dev(a, "a"); _dev(b, "b")
    M, Ca = a.shape
    Cb = b.shape[1]
    assert b.shape[0] == M and a.dtype == b.dtype
    out = torch.empty((M, Ca + Cb), device=a.device, dtype=a.dtype)
    _lib.check(lib.geo4d_concat_channels(a.data_ptr(), _ld(a), Ca, b.data_ptr(), _ld(b), Cb, out.data_ptr(), _ld(out), M,
                                         dt_code(a.dtype), _stream()), "geo4d_concat_channels")
    return out


def timestep_embedding(t, freqs):
    """t int64 [B] on device, freqs fp32 [dim/2] -> fp32 [B, dim] = [cos | sin]."""
    lib = _lib.load()
    _dev(t, "t")
    assert t.dtype == torch.int64 and freqs.dtype == torch.float32
    B, half = t.shape[0], freqs.shape[0]
    out = torch.empty((B, 2 * half), device=t.device, dtype=torch.float32)
    _lib.check(lib.geo4d_timestep_embedding(t.data_ptr(), freqs.data_ptr(), out.data_ptr(), B, 2 * half, _stream()),
               "geo4d_timestep_embedding")
    return out


def embed_tokens(tokens, table, pos, dtype):
    """tokens int64 [B, n_ctx] (device), table fp32 [vocab, W], pos fp32 [n_ctx, W] -> [B * n_ctx, W] of `dtype`."""
    lib = _lib.load()
    _dev(tokens, "tokens")
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and table.dtype == torch.float32 and pos.dtype == torch.float32
    B, n = tokens.shape
    out = torch.empty((B * n, table.shape[1]), device=tokens.device, dtype=dtype)
    _lib.check(lib.geo4d_embed_tokens(tokens.data_ptr(), table.data_ptr(), pos.data_ptr(), out.data_ptr(), _ld(out), B * n, n,
                                      table.shape[1], table.shape[0], dt_code(dtype), _stream()), "geo4d_embed_tokens")
    return out


def linear_small(x, w, bias=None, *, add=None, act_in=False, act_out=False, out=None):
    """fp32 [M,K] x fp32 [N,K]^T for M = batch-sized rows (time / fps / ResBlock embedding MLPs)."""
    lib = _lib.load()
    _dev(x, "x")
    assert x.dtype == torch.float32 and w.dtype == torch.float32
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    _lib.check(lib.geo4d_linear_small(x.data_ptr(), _ld(x), w.data_ptr(), _ld(w), _ptr(bias), _ptr(add),
                                      _ld(add) if add is not None else 0, out.data_ptr(), _ld(out), M, N, K, int(act_in),
                                      int(act_out), _stream()), "geo4d_linear_small")
    return out


def ddim_step(x, v, coef, step_index, noise=None, pred_x0=None):
    lib = _lib.load()
    _dev(x, "x")
    assert x.dtype == torch.float32 and v.dtype == torch.float32 and x.is_contiguous() and v.is_contiguous()
    assert coef.dtype == torch.float32 and step_index.dtype == torch.int32
    _lib.check(lib.geo4d_ddim_step(x.data_ptr(), v.data_ptr(), _ptr(noise), _ptr(pred_x0), coef.data_ptr(),
                                   step_index.data_ptr(), x.numel(), _stream()), "geo4d_ddim_step")
    return x


NOISE_STREAM_XT, NOISE_STREAM_STEP = 0, 1      # Philox counter word 2 (geo4d_amd/noise.py): initial noise x_T / DDIM step noise


def _seeds(seeds, B, dev):
    assert seeds.dtype == torch.int64 and seeds.is_contiguous() and seeds.numel() == B and seeds.device == dev, \
        f"seeds: int64 [{B}] on {dev} expected"


def philox_fill(out, seeds, *, step, stream_id, draw=0, scale=1.0, raw=False):
    """out [B, ...] (fp32: normals * scale; ``raw``: int32, the 32-bit words) <- the counter-based noise of geo4d_amd/noise.py, row b keyed by
    seeds[b] (int64 [B] on the device). ``step``: an int, or an int32 [1] device tensor read by the kernel (capturable)."""
    lib = _lib.load()
    _dev(out, "out")
    assert out.is_contiguous() and out.dtype == (torch.int32 if raw else torch.float32)
    B = out.shape[0]
    _seeds(seeds, B, out.device)
    on_dev = isinstance(step, torch.Tensor)
    assert not on_dev or (step.dtype == torch.int32 and step.device == out.device)
    _lib.check(lib.geo4d_philox_fill(out.data_ptr(), int(raw), seeds.data_ptr(), B, out.numel() // B, step.data_ptr() if on_dev else None,
                                     0 if on_dev else int(step), int(stream_id), int(draw), float(scale), _stream()), "geo4d_philox_fill")
    return out


def ddim_step_rng(x, v, coef, step_index, seeds, *, draw=0, noise_scale=1.0, pred_x0=None):
    """ddim_step with the noise of row b made in the kernel: the stream-1 normals of (seeds[b], *step_index, element, draw) * noise_scale."""
    lib = _lib.load()
    _dev(x, "x")
    assert x.dtype == torch.float32 and v.dtype == torch.float32 and x.is_contiguous() and v.is_contiguous() and v.shape == x.shape
    assert coef.dtype == torch.float32 and step_index.dtype == torch.int32
    assert pred_x0 is None or (pred_x0.dtype == torch.float32 and pred_x0.is_contiguous() and pred_x0.shape == x.shape)
    B = x.shape[0]
    _seeds(seeds, B, x.device)
    _lib.check(lib.geo4d_ddim_step_rng(x.data_ptr(), v.data_ptr(), _ptr(pred_x0), coef.data_ptr(), step_index.data_ptr(), seeds.data_ptr(),
                                       B, x.numel() // B, int(draw), float(noise_scale), _stream()), "geo4d_ddim_step_rng")
    return x


def cfg_combine(e_c, e_u, e_i=None, *, scale, cfg_img=None, guidance_rescale=0.0):
    """Classifier-free guidance on fp32 U-Net outputs [B, ...]: 2-way, or 3-way with e_i (image yes / text ""), + rescale_noise_cfg."""
    lib = _lib.load()
    _dev(e_c, "e_c")
    ts = [t for t in (e_c, e_u, e_i) if t is not None]
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.shape == e_c.shape for t in ts)
    B = e_c.shape[0]
    n = e_c.numel() // B
    out = torch.empty_like(e_c)
    need = lib.geo4d_cfg_combine_workspace(B)
    ws = torch.empty(need // 8, device=e_c.device, dtype=torch.float64)
    _lib.check(lib.geo4d_cfg_combine(e_c.data_ptr(), e_u.data_ptr(), _ptr(e_i), out.data_ptr(), B, n, float(scale),
                                     float(scale if cfg_img is None else cfg_img), float(guidance_rescale), ws.data_ptr(), need,
                                     _stream()), "geo4d_cfg_combine")
    return out


def advance_index(idx, delta):
    lib = _lib.load()
    _lib.check(lib.geo4d_advance_index(idx.data_ptr(), delta, _stream()), "geo4d_advance_index")


def gather_timestep(idx, table, ts):
    """ts[:] = table[idx] on the device (idx int32[1], table int64[S], ts int64[B])."""
    lib = _lib.load()
    assert idx.dtype == torch.int32 and table.dtype == torch.int64 and ts.dtype == torch.int64
    _lib.check(lib.geo4d_gather_timestep(idx.data_ptr(), table.data_ptr(), ts.data_ptr(), ts.numel(), _stream()),
               "geo4d_gather_timestep")
    return ts


def plucker_cameras(raymap, crossmap):
    """raymap, crossmap: fp32 [1, 3, T, H, W] (may be channel views of the decoded [B, 11, T, H, W] tensor) -> P_c2w [T, 4, 4]."""
    lib = _lib.load()
    _dev(raymap, "raymap"); _dev(crossmap, "crossmap")
    assert raymap.dtype == torch.float32 and crossmap.dtype == torch.float32 and raymap.shape == crossmap.shape
    B, Cc, T, H, W = raymap.shape
    assert B == 1 and Cc == 3, raymap.shape
    for m in (raymap, crossmap):
        assert m.stride(4) == 1 and m.stride(3) == W, "pixel planes must be contiguous"
    assert raymap.stride(1) == crossmap.stride(1) and raymap.stride(2) == crossmap.stride(2)
    need = lib.geo4d_plucker_cameras_workspace(T, H, W)
    ws = torch.empty(need // 8, device=raymap.device, dtype=torch.float64)
    out = torch.empty((T, 4, 4), device=raymap.device, dtype=torch.float32)
    _lib.check(lib.geo4d_plucker_cameras(raymap.data_ptr(), crossmap.data_ptr(), raymap.stride(1), raymap.stride(2), T, H, W,
                                         ws.data_ptr(), need, out.data_ptr(), _stream()), "geo4d_plucker_cameras")
    return out


def bicubic_resize(x, size, out=None):
    """x fp32 [T, h, w] -> [T, OH, OW] = F.interpolate(x[None], size, mode="bicubic", align_corners=False)[0] (torchvision Resize(BICUBIC)
    on a float tensor under the reference's pinned torch 2.0 stack: no antialias, no output clamp)."""
    lib = _lib.load()
    _dev(x, "x")
    assert x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous(), (x.dtype, x.shape)
    T, h, w = x.shape
    OH, OW = int(size[0]), int(size[1])
    out = torch.empty((T, OH, OW), device=x.device, dtype=torch.float32) if out is None else out
    assert out.shape == (T, OH, OW) and out.dtype == torch.float32 and out.is_contiguous()
    _lib.check(lib.geo4d_bicubic_resize(x.data_ptr(), out.data_ptr(), T, h, w, OH, OW, _stream()), "geo4d_bicubic_resize")
    return out


def _mask_ptr(mask, n, device):
    if mask is None:
        return None, None
    assert mask.numel() == n and mask.device == device, "mask must match the depth maps"
    m = mask.reshape(-1).to(torch.bool).contiguous()
    return m, m.data_ptr()


def masked_select(pred, gt, *, max_depth=None, mask=None, pre_clip_min=None, pre_clip_max=None):
    """(clamp(pred, pre_clip_min, pre_clip_max)[v], gt[v], count) with v = (gt > 0) & (gt < max_depth) & mask in index order
    (= torch boolean indexing). The two outputs are n-element buffers of which the first `count` (a device int64 [1]) are written."""
    lib = _lib.load()
    _dev(pred, "pred"); _dev(gt, "gt")
    assert pred.dtype == torch.float32 and gt.dtype == torch.float32 and pred.is_contiguous() and gt.is_contiguous()
    n = gt.numel()
    assert pred.numel() == n and n > 0
    m, mp = _mask_ptr(mask, n, gt.device)
    pv, gv = torch.empty(n, device=gt.device, dtype=torch.float32), torch.empty(n, device=gt.device, dtype=torch.float32)
    count = torch.empty(1, device=gt.device, dtype=torch.int64)
    need = lib.geo4d_masked_select_workspace(n)
    ws = torch.empty((need + 3) // 4, device=gt.device, dtype=torch.int32)
    inf = float("inf")
    _lib.check(lib.geo4d_masked_select(pred.data_ptr(), gt.data_ptr(), n, inf if max_depth is None else float(max_depth), mp,
                                       -inf if pre_clip_min is None else float(pre_clip_min), inf if pre_clip_max is None else float(pre_clip_max),
                                       pv.data_ptr(), gv.data_ptr(), count.data_ptr(), ws.data_ptr(), need, _stream()), "geo4d_masked_select")
    return pv, gv, count


def depth_metrics(pred, gt, st, *, max_depth=None, custom_mask=None, pre_clip_min=None, pre_clip_max=None, post_clip_min=None,
                  post_clip_max=None, aligned=False):
    """One pass of depth_evaluation's metrics (depth_eval.py:283-335) with (s, t) = st (fp32 device [2]): returns (sums fp64 [8] = sum |a-g|/g,
    sum (a-g)^2/g, sum (a-g)^2, sum (log a' - log g)^2, #delta < 1.25, < 1.25^2, < 1.25^3, #pixels; error map [n]; s * pred + t [n] or None)."""
    lib = _lib.load()
    _dev(pred, "pred"); _dev(gt, "gt"); _dev(st, "st")
    assert pred.dtype == torch.float32 and gt.dtype == torch.float32 and pred.is_contiguous() and gt.is_contiguous()
    assert st.dtype == torch.float32 and st.numel() == 2 and st.is_contiguous()
    n = gt.numel()
    assert pred.numel() == n and n > 0
    m, mp = _mask_ptr(custom_mask, n, gt.device)
    sums = torch.empty(8, device=gt.device, dtype=torch.float64)
    err = torch.empty(n, device=gt.device, dtype=torch.float32)
    al = torch.empty(n, device=gt.device, dtype=torch.float32) if aligned else None
    need = lib.geo4d_depth_metrics_workspace(n)
    ws = torch.empty((need + 7) // 8, device=gt.device, dtype=torch.float64)
    inf = float("inf")
    clip = lambda v, d: d if v is None else float(v)
    _lib.check(lib.geo4d_depth_metrics(pred.data_ptr(), gt.data_ptr(), n, clip(max_depth, inf), mp, st.data_ptr(), clip(pre_clip_min, -inf),
                                       clip(pre_clip_max, inf), clip(post_clip_min, -inf), clip(post_clip_max, inf), sums.data_ptr(),
                                       err.data_ptr(), _ptr(al), ws.data_ptr(), need, _stream()), "geo4d_depth_metrics")
    return sums, err, al


def _want(t, what, dtype, shape):
    """`t`, which must be on the HIP device (_dev), of `dtype`, contiguous and of `shape`, where None stands for any extent. The
    AssertionError says what was found."""
    _dev(t, what)
    assert t.dtype == dtype and t.dim() == len(shape) and all(s is None or s == d for s, d in zip(shape, t.shape)) and t.is_contiguous(), \
        (what, t.dtype, tuple(t.shape))
    return t


def _no_rows(dev, rgba, *more):
    """The result of an op that found nothing: (points fp32 [0, 3], rgba uint8 [0, 4] or None as `rgba` is, weight fp32 [0], *more)."""
    return (torch.empty((0, 3), device=dev, dtype=torch.float32), None if rgba is None else torch.empty((0, 4), device=dev, dtype=torch.uint8),
            torch.empty(0, device=dev, dtype=torch.float32), *more)


def scene_clean(conf, pts3d, depth, mats, tol=0.001, bad_conf=0.0):
    """clean_pointcloud (base_opt_group.py:630-665) in place on conf fp32 [n, H, W]: pts3d [n, H, W, 3] world points, depth [n, H, W],
    mats [n, 21] = rows 0..2 of each world-to-camera matrix then its intrinsics, row-major. Returns conf."""
    lib = _lib.load()
    n, H, W = _want(conf, "conf", torch.float32, (None, None, None)).shape
    _want(pts3d, "pts3d", torch.float32, (n, H, W, 3)), _want(depth, "depth", torch.float32, (n, H, W)), _want(mats, "mats", torch.float32, (n, 21))
    _lib.check(lib.geo4d_scene_clean(conf.data_ptr(), pts3d.data_ptr(), depth.data_ptr(), mats.data_ptr(), n, H, W, float(tol), float(bad_conf),
                                     _stream()), "geo4d_scene_clean")
    return conf


def _scene_mask(mask, shape, device):
    if mask is None:
        return None
    assert tuple(mask.shape) == tuple(shape) and mask.device == device, (mask.shape, shape)
    return mask.to(torch.bool).contiguous()


def scene_points(pts3d, rgb=None, mask=None):
    """(pts [n H W, 3] fp32, rgba [n H W, 4] uint8 or None, count device int64 [1]): pts3d[mask] and the matching colours of rgb
    [n, H, W, 3] in [0, 1], image-major raster order (= torch boolean indexing); the first `count` rows are written. mask None = all."""
    lib = _lib.load()
    n, H, W, _ = _want(pts3d, "pts3d", torch.float32, (None, None, None, 3)).shape
    if rgb is not None:
        _want(rgb, "rgb", torch.float32, (n, H, W, 3))
    m = _scene_mask(mask, (n, H, W), pts3d.device)
    pts = torch.empty((n * H * W, 3), device=pts3d.device, dtype=torch.float32)
    rgba = None if rgb is None else torch.empty((n * H * W, 4), device=pts3d.device, dtype=torch.uint8)
    count = torch.empty(1, device=pts3d.device, dtype=torch.int64)
    need = lib.geo4d_scene_points_workspace(n, H, W)
    ws = torch.empty((need + 3) // 4, device=pts3d.device, dtype=torch.int32)
    _lib.check(lib.geo4d_scene_points(pts3d.data_ptr(), _ptr(rgb), _ptr(m), n, H, W, pts.data_ptr(), _ptr(rgba), count.data_ptr(),
                                      ws.data_ptr(), need, _stream()), "geo4d_scene_points")
    return pts, rgba, count


def scene_mesh_faces(mask, n, H, W, device):
    """(faces [4 n (H-1)(W-1), 3] int32, count device int64 [1]): pts3d_to_trimesh + cat_meshes's faces (dust3r/viz.py:40-90) for a
    valid-vertex mask [n, H, W] (None = every vertex valid); the first `count` rows are written."""
    lib = _lib.load()
    if mask is not None:
        _dev(mask, "mask")
    m = _scene_mask(mask, (n, H, W), device)
    faces = torch.empty((4 * n * max(H - 1, 0) * max(W - 1, 0), 3), device=device, dtype=torch.int32)
    count = torch.zeros(1, device=device, dtype=torch.int64)
    if H < 2 or W < 2:                                      # no quads
        return faces, count
    need = lib.geo4d_scene_mesh_faces_workspace(n, H, W)
    ws = torch.empty((need + 3) // 4, device=device, dtype=torch.int32)
    _lib.check(lib.geo4d_scene_mesh_faces(_ptr(m), n, H, W, faces.data_ptr(), count.data_ptr(), ws.data_ptr(), need, _stream()),
               "geo4d_scene_mesh_faces")
    return faces, count


def render_workspace(V, H, W, n_entries, device):
    """The renderer's workspace (two uint64 key buffers [V, H, W] and the device copy of the source lists) as an int64 tensor."""
    need = _lib.load().geo4d_render_workspace(V, H, W, n_entries)
    if need == 0:
        raise _lib.Geo4DNativeError(f"geo4d_render_workspace: need V, H, W > 0 and V * H * W < 2^31, got {(V, H, W)}")
    return torch.empty((need + 7) // 8, device=device, dtype=torch.int64)


def render_splat(points, views, view_src_ptr, view_src, size, ws, mask=None, radius=None, pts_per_image=None, near=1e-3, max_size=9):
    """Splat points fp32 [N, 3] into the key buffers of `ws` (render_workspace) for views fp32 [V, 16] (world-to-camera rows 0..2, then
    fx, fy, cx, cy). view_src_ptr / view_src: host int lists, the CSR of source images per view, an image being `pts_per_image`
    consecutive points (None: all N are one image). mask [N] bool, radius [N] fp32 world radii (None: one pixel per point)."""
    lib = _lib.load()
    H, W = size
    _dev(ws, "ws")
    N, V = _want(points, "points", torch.float32, (None, 3)).shape[0], _want(views, "views", torch.float32, (None, 16)).shape[0]
    if mask is not None:
        assert tuple(_dev(mask, "mask").shape) == (N,), mask.shape
        mask = mask.to(torch.bool).contiguous()
    if radius is not None:
        _want(radius, "radius", torch.float32, (N,))
    assert len(view_src_ptr) == V + 1 and len(view_src) == view_src_ptr[-1], (len(view_src_ptr), len(view_src), V)
    ptr = (C.c_int * (V + 1))(*view_src_ptr)
    src = (C.c_int * max(len(view_src), 1))(*view_src)
    _lib.check(lib.geo4d_render_splat(points.data_ptr(), _ptr(mask), _ptr(radius), N, N if pts_per_image is None else pts_per_image,
                                      views.data_ptr(), ptr, src, V, H, W, float(near), int(max_size), ws.data_ptr(), ws.numel() * 8,
                                      _stream()), "geo4d_render_splat")
    return ws


def render_fill(ws, V, size, passes):
    """`passes` hole-filling passes on the key buffers of `ws`: an empty pixel takes the minimum key of its 3 x 3 neighbours."""
    _dev(ws, "ws")
    _lib.check(_lib.load().geo4d_render_fill(V, size[0], size[1], int(passes), ws.data_ptr(), ws.numel() * 8, _stream()), "geo4d_render_fill")
    return ws


def render_resolve(ws, colors, V, size, background=(1.0, 1.0, 1.0)):
    """(rgb uint8 [V, H, W, 3], depth fp32 [V, H, W], index int32 [V, H, W]) of the key buffers of `ws`: the winning point's colour
    (colors fp32 [N, 3] in [0, 1], scene_points' rounding), camera depth and id; background / 0 / -1 where no point landed."""
    lib = _lib.load()
    H, W = size
    _dev(ws, "ws"), _want(colors, "colors", torch.float32, (None, 3))
    rgb = torch.empty((V, H, W, 3), device=ws.device, dtype=torch.uint8)
    depth = torch.empty((V, H, W), device=ws.device, dtype=torch.float32)
    index = torch.empty((V, H, W), device=ws.device, dtype=torch.int32)
    bg = (C.c_float * 3)(*[float(c) for c in background])
    _lib.check(lib.geo4d_render_resolve(colors.data_ptr(), colors.shape[0], bg, V, H, W, rgb.data_ptr(), depth.data_ptr(), index.data_ptr(),
                                        ws.data_ptr(), ws.numel() * 8, _stream()), "geo4d_render_resolve")
    return rgb, depth, index


RASTER_LARGE_AREA = 16           # from tools/render_mesh_bench.py's sweep (profiles/render_mesh.md)
RASTER_LIST_CAPACITY = 1 << 16


def _mesh(vertices, faces):
    """(Nv, T) of vertices fp32 [Nv, 3] and faces int32 [T, 3] on the HIP device."""
    return (_want(vertices, "vertices", torch.float32, (None, 3)).shape[0], _want(faces, "faces", torch.int32, (None, 3)).shape[0])


def render_raster(vertices, faces, views, size, ws, face_mask=None, near=1e-3, cull_back=False, id_base=0, clear=True, *,
                  large_area=None, capacity=None):
    """Rasterise the mesh (vertices fp32 [Nv, 3] world, faces int32 [T, 3], face_mask [T] bool or None) into the key buffer of `ws`
    (render_workspace) for views fp32 [V, 16]: per covered pixel the minimum of float_bits(zc) << 32 | (id_base + t). `clear=False` draws
    into what render_splat / render_fill left. A triangle whose clipped bounding box holds more than `large_area` pixels goes through a
    list of `capacity` entries that one wave per entry draws (a full list: the thread draws it itself); the image depends on neither."""
    lib = _lib.load()
    H, W = size
    _dev(ws, "ws")
    Nv, T = _mesh(vertices, faces)
    V = _want(views, "views", torch.float32, (None, 16)).shape[0]
    if face_mask is not None:
        assert tuple(_dev(face_mask, "face_mask").shape) == (T,), face_mask.shape
        face_mask = face_mask.to(torch.bool).contiguous()
    capacity = RASTER_LIST_CAPACITY if capacity is None else int(capacity)
    need = lib.geo4d_render_raster_workspace(capacity)
    if need == 0:
        raise _lib.Geo4DNativeError(f"geo4d_render_raster_workspace: need 0 <= capacity <= 2^28, got {capacity}")
    lst = torch.empty((need + 7) // 8, device=ws.device, dtype=torch.int64)
    _lib.check(lib.geo4d_render_raster(_ptr(vertices) if Nv else 0, Nv, _ptr(faces) if T else 0, T, _ptr(face_mask), views.data_ptr(), V, H, W,
                                       float(near), int(bool(cull_back)), int(id_base), int(bool(clear)),
                                       RASTER_LARGE_AREA if large_area is None else int(large_area), ws.data_ptr(), ws.numel() * 8,
                                       lst.data_ptr(), need, _stream()), "geo4d_render_raster")
    return ws


def render_resolve_mesh(ws, colors, vertices, faces, views, size, vertex_colors=None, mesh_color=(0.7, 0.7, 0.7), shade=0.0, near=1e-3,
                        background=(1.0, 1.0, 1.0)):
    """(rgb uint8 [V, H, W, 3], depth fp32 [V, H, W], index int32 [V, H, W], face int32 [V, H, W]) of the key buffer of `ws` after
    render_raster with id_base = N: colors fp32 [N, 3] of the points (None: no points, N = 0), the mesh and the views as render_raster
    took them, vertex_colors uint8 rgba [Nv, 4] or fp32 [Nv, 3] (None: `mesh_color`), flat headlight shading of strength `shade`."""
    lib = _lib.load()
    H, W = size
    _dev(ws, "ws")
    N = 0 if colors is None else _want(colors, "colors", torch.float32, (None, 3)).shape[0]
    Nv, T = _mesh(vertices, faces)
    V = _want(views, "views", torch.float32, (None, 16)).shape[0]
    rgba = rgbf = None
    if vertex_colors is not None and vertex_colors.dtype == torch.uint8:
        rgba = _want(vertex_colors, "vertex_colors", torch.uint8, (Nv, 4))
    elif vertex_colors is not None:
        rgbf = _want(vertex_colors, "vertex_colors", torch.float32, (Nv, 3))
    rgb = torch.empty((V, H, W, 3), device=ws.device, dtype=torch.uint8)
    depth = torch.empty((V, H, W), device=ws.device, dtype=torch.float32)
    index = torch.empty((V, H, W), device=ws.device, dtype=torch.int32)
    face = torch.empty((V, H, W), device=ws.device, dtype=torch.int32)
    bg = (C.c_float * 3)(*[float(c) for c in background])
    mc = (C.c_float * 3)(*[float(c) for c in mesh_color])
    _lib.check(lib.geo4d_render_resolve_mesh(_ptr(colors) if N else 0, N, _ptr(vertices) if Nv else 0, Nv, _ptr(faces) if T else 0, T,
                                             _ptr(rgba) if Nv else 0, _ptr(rgbf) if Nv else 0, mc, views.data_ptr(), float(near),
                                             float(shade), bg, V, H, W, rgb.data_ptr(), depth.data_ptr(), index.data_ptr(),
                                             face.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()), "geo4d_render_resolve_mesh")
    return rgb, depth, index, face


def motion_range(depth, valid=None):
    """The motion rule's workspace for depth fp32 [n, H, W] and valid bool [n, H, W] (None: every pixel): per pixel the (dmin, dmax) of
    the valid depths in its 3 x 3 neighbourhood, dmin = NaN on invalid pixels; fp32 [n, H, W, 2]."""
    lib = _lib.load()
    n, H, W = _want(depth, "depth", torch.float32, (None, None, None)).shape
    if valid is not None:
        _dev(valid, "valid")
    valid = _scene_mask(valid, (n, H, W), depth.device)
    need = lib.geo4d_motion_workspace(n, H, W)
    if need == 0:
        raise _lib.Geo4DNativeError(f"geo4d_motion_workspace: need n, H, W > 0 and n * H * W < 2^31, got {(n, H, W)}")
    ws = torch.empty((n, H, W, 2), device=depth.device, dtype=torch.float32)
    _lib.check(lib.geo4d_motion_range(depth.data_ptr(), _ptr(valid), n, H, W, ws.data_ptr(), need, _stream()), "geo4d_motion_range")
    return ws


def motion_votes(pts3d, depth, valid, views, radius=8, tol=0.05, near=1e-3, ws=None):
    """votes uint8 [n, H, W, 3] = (consistent, free, occluded) counts of every pixel over the images 0 < |j - i| <= radius (the rule of
    include/geo4d_hip.h): pts3d fp32 [n, H, W, 3] world points, depth fp32 [n, H, W], valid bool [n, H, W] or None, views fp32 [n, 16]
    (world-to-camera rows 0..2, then fx, fy, cx, cy). `ws`: a motion_range result to reuse instead of computing the depth ranges."""
    lib = _lib.load()
    n, H, W, _ = _want(pts3d, "pts3d", torch.float32, (None, None, None, 3)).shape
    _want(views, "views", torch.float32, (n, 16))
    if ws is None:
        assert tuple(depth.shape) == (n, H, W), (depth.shape, pts3d.shape)
        ws = motion_range(depth, valid)
    _want(ws, "ws", torch.float32, (n, H, W, 2))
    votes = torch.empty((n, H, W, 3), device=pts3d.device, dtype=torch.uint8)
    _lib.check(lib.geo4d_motion_votes(pts3d.data_ptr(), views.data_ptr(), n, H, W, int(radius), float(tol), float(near), votes.data_ptr(),
                                      ws.data_ptr(), ws.numel() * 4, _stream()), "geo4d_motion_votes")
    return votes


FUSE_REDUCE = {"mean": 0, "best": 1}


class FuseTable:
    """The voxel table of one fuse_insert: the workspace, its sizes, the inputs the later launches read, and `dropped` (device int64 [1])."""

    def __init__(self, ws, need, capacity, reduce, voxel, points, rgba, weight, dropped):
        self.ws, self.need, self.capacity, self.reduce, self.voxel = ws, need, capacity, reduce, voxel
        self.points, self.rgba, self.weight, self.dropped = points, rgba, weight, dropped


def fuse_capacity(N):
    """The default table size: the power of two >= 2 N."""
    return 1 << max(2 * N - 1, 0).bit_length()


def fuse_insert(points, rgba=None, weight=None, mask=None, *, voxel, reduce="mean", capacity=None):
    """Insert points fp32 [N, 3] into a fresh voxel table (the rule of include/geo4d_hip.h): rgba uint8 [N, 4], weight fp32 [N] and mask
    bool [N] are optional. Returns the FuseTable for fuse_compact / fuse_finalize."""
    lib = _lib.load()
    N = _want(points, "points", torch.float32, (None, 3)).shape[0]
    if rgba is not None:
        _want(rgba, "rgba", torch.uint8, (N, 4))
    if weight is not None:
        _want(weight, "weight", torch.float32, (N,))
    if mask is not None:
        assert tuple(_dev(mask, "mask").shape) == (N,), mask.shape
        mask = mask.to(torch.bool).contiguous()
    if reduce not in FUSE_REDUCE:
        raise ValueError(f"fuse_insert: reduce must be one of {tuple(FUSE_REDUCE)}, got {reduce!r}")
    capacity = fuse_capacity(N) if capacity is None else int(capacity)
    need = lib.geo4d_fuse_workspace(capacity, FUSE_REDUCE[reduce])
    if need == 0:
        raise _lib.Geo4DNativeError(f"geo4d_fuse_workspace: capacity must be a power of two in 1 .. 2^32, got {capacity}")
    ws = torch.empty(need // 8, device=points.device, dtype=torch.int64)
    dropped = torch.empty(1, device=points.device, dtype=torch.int64)
    _lib.check(lib.geo4d_fuse_insert(points.data_ptr(), _ptr(rgba), _ptr(weight), _ptr(mask), N, float(voxel), FUSE_REDUCE[reduce], capacity,
                                     dropped.data_ptr(), ws.data_ptr(), need, _stream()), "geo4d_fuse_insert")
    return FuseTable(ws, need, capacity, FUSE_REDUCE[reduce], float(voxel), points, rgba, weight, dropped)


def fuse_compact(table):
    """(keys int64 [N], slots int64 [N], count device int64 [1]) of a FuseTable: the occupied slots in arrival order; the first `count`
    rows are written."""
    N = table.points.shape[0]
    dev = table.ws.device
    keys, slots = torch.empty(N, device=dev, dtype=torch.int64), torch.empty(N, device=dev, dtype=torch.int64)
    count = torch.empty(1, device=dev, dtype=torch.int64)
    _lib.check(_lib.load().geo4d_fuse_compact(table.capacity, table.reduce, keys.data_ptr(), slots.data_ptr(), N, count.data_ptr(),
                                              table.ws.data_ptr(), table.need, _stream()), "geo4d_fuse_compact")
    return keys, slots, count


def fuse_finalize(table, order):
    """(points fp32 [M, 3], rgba uint8 [M, 4] or None, weight fp32 [M], count int32 [M]): the voxels in the slots `order` int64 [M]."""
    M, dev = _want(order, "order", torch.int64, (None,)).shape[0], order.device
    pts = torch.empty((M, 3), device=dev, dtype=torch.float32)
    rgba = None if table.rgba is None else torch.empty((M, 4), device=dev, dtype=torch.uint8)
    weight = torch.empty(M, device=dev, dtype=torch.float32)
    count = torch.empty(M, device=dev, dtype=torch.int32)
    if M == 0:                                                      # no voxel: nothing to launch (an empty tensor has no address)
        return pts, rgba, weight, count
    _lib.check(_lib.load().geo4d_fuse_finalize(order.data_ptr(), M, table.points.data_ptr(), _ptr(table.rgba), _ptr(table.weight),
                                               table.points.shape[0], table.voxel, table.reduce, table.capacity, pts.data_ptr(), _ptr(rgba),
                                               weight.data_ptr(), count.data_ptr(), table.ws.data_ptr(), table.need, _stream()),
               "geo4d_fuse_finalize")
    return pts, rgba, weight, count


def fuse_points(points, rgba=None, weight=None, mask=None, *, voxel, reduce="mean", capacity=None):
    """One point per occupied voxel of side `voxel` (the rule of include/geo4d_hip.h), in key order = lexicographic (cx, cy, cz):
    (points fp32 [M, 3], rgba uint8 [M, 4] or None, weight fp32 [M], count int32 [M], dropped int). points fp32 [N, 3], rgba uint8
    [N, 4], weight fp32 [N], mask bool [N] on the HIP device. `capacity`: the table's size, a power of two >= N (default: >= 2 N).
    Insert, compact and finalize are HIP launches; between them the (key, slot) pairs are sorted by key with torch.sort, because a
    slot's position depends on the order the points arrived in. Reads two counts back (one synchronisation)."""
    if _dev(points, "points").shape[0] == 0:                        # no point: no table
        return (points.new_empty((0, 3)), None if rgba is None else rgba.new_empty((0, 4)), points.new_empty(0),
                torch.empty(0, device=points.device, dtype=torch.int32), 0)
    table = fuse_insert(points, rgba, weight, mask, voxel=voxel, reduce=reduce, capacity=capacity)
    keys, slots, count = fuse_compact(table)
    M, dropped = torch.cat([count, table.dropped]).tolist()
    order = slots[:M][torch.sort(keys[:M]).indices]                 # keys < 2^63: signed order is unsigned order
    return (*fuse_finalize(table, order.contiguous()), dropped)


class TsdfTableFull(RuntimeError):
    """The TSDF's voxel table was too small for the scene: nothing was computed; pass the capacity the message names."""


def tsdf_capacity(taking_part):
    """The default table size: the power of two >= 4 x the taking-part pixels."""
    return 1 << max(4 * int(taking_part) - 1, 0).bit_length()


def _tsdf_images(depth, valid, rgba, weight):
    """The checked per-pixel inputs every tsdf op takes: (n, H, W, valid as bool or None) of depth fp32 [n, H, W]."""
    n, H, W = _want(depth, "depth", torch.float32, (None, None, None)).shape
    if valid is not None:
        _dev(valid, "valid")
    if rgba is not None:
        _want(rgba, "rgba", torch.uint8, (n, H, W, 4))
    if weight is not None:
        _want(weight, "weight", torch.float32, (n, H, W))
    return n, H, W, _scene_mask(valid, (n, H, W), depth.device)


def _tsdf_maps(pts3d, depth, valid, rgba, weight):
    """_tsdf_images, with the point maps pts3d fp32 [n, H, W, 3] checked first."""
    _want(depth, "depth", torch.float32, _want(pts3d, "pts3d", torch.float32, (None, None, None, 3)).shape[:3])
    return _tsdf_images(depth, valid, rgba, weight)


def tsdf_mark(pts3d, depth, valid, centres, *, voxel, trunc=4, near=1e-3, capacity):
    """Mark the voxels within `trunc` voxels of every taking-part pixel's point along its ray (the rule of include/geo4d_hip.h) in a
    fresh table of `capacity` keys: (table int64 [capacity], counters device int64 [2] = dropped, overflow)."""
    lib = _lib.load()
    n, H, W, valid = _tsdf_maps(pts3d, depth, valid, None, None)
    _want(centres, "centres", torch.float32, (n, 3))
    need = lib.geo4d_tsdf_workspace(int(capacity))
    if need == 0:
        raise _lib.Geo4DNativeError(f"geo4d_tsdf_workspace: capacity must be a power of two in 1 .. 2^32, got {capacity}")
    table = torch.empty(need // 8, device=pts3d.device, dtype=torch.int64)
    counters = torch.empty(2, device=pts3d.device, dtype=torch.int64)
    _lib.check(lib.geo4d_tsdf_mark(pts3d.data_ptr(), depth.data_ptr(), _ptr(valid), centres.data_ptr(), n, H, W, float(voxel), int(trunc),
                                   float(near), int(capacity), counters.data_ptr(), table.data_ptr(), need, _stream()), "geo4d_tsdf_mark")
    return table, counters


def tsdf_compact(table, max_keys=None):
    """(keys int64 [max_keys], count device int64 [1]) of a tsdf_mark table: the marked keys in arrival order; the first `count` rows
    are written (max_keys None: room for a full table)."""
    capacity = _want(table, "table", torch.int64, (None,)).numel()
    assert capacity >= 1, (table.dtype, table.shape)
    max_keys = capacity if max_keys is None else max(int(max_keys), 1)
    keys = torch.empty(max_keys, device=table.device, dtype=torch.int64)
    count = torch.empty(1, device=table.device, dtype=torch.int64)
    _lib.check(_lib.load().geo4d_tsdf_compact(capacity, keys.data_ptr(), max_keys, count.data_ptr(), table.data_ptr(), capacity * 8,
                                              _stream()), "geo4d_tsdf_compact")
    return keys, count


def _tsdf_voxels(keys, f, wt, rgba):
    """M of a field as tsdf_integrate leaves it: keys int64 [M], f and wt fp32 [M], rgba uint8 [M, 4] or None."""
    M = _want(keys, "keys", torch.int64, (None,)).shape[0]
    _want(f, "f", torch.float32, (M,)), _want(wt, "wt", torch.float32, (M,))
    if rgba is not None:
        _want(rgba, "rgba", torch.uint8, (M, 4))
    return M


def tsdf_integrate(keys, depth, valid, views, rgba=None, weight=None, *, voxel, trunc=4, near=1e-3):
    """(f fp32 [M], Wt fp32 [M], rgba uint8 [M, 4] or None) of the voxels `keys` int64 [M]: the truncated signed distance averaged over
    the images in the order 0 .. n-1, its weight and the averaged colour (the rule of include/geo4d_hip.h)."""
    lib = _lib.load()
    M, dev = _want(keys, "keys", torch.int64, (None,)).shape[0], keys.device
    n, H, W, valid = _tsdf_images(depth, valid, rgba, weight)
    _want(views, "views", torch.float32, (n, 16))
    f = torch.empty(M, device=dev, dtype=torch.float32)
    wt = torch.empty(M, device=dev, dtype=torch.float32)
    col = None if rgba is None else torch.empty((M, 4), device=dev, dtype=torch.uint8)
    if M == 0:                                                      # no voxel: nothing to launch (an empty tensor has no address)
        return f, wt, col
    _lib.check(lib.geo4d_tsdf_integrate(keys.data_ptr(), M, depth.data_ptr(), _ptr(valid), _ptr(weight), _ptr(rgba), views.data_ptr(), n, H, W,
                                        float(voxel), int(trunc), float(near), f.data_ptr(), wt.data_ptr(), _ptr(col), _stream()),
               "geo4d_tsdf_integrate")
    return f, wt, col


def tsdf_extract(keys, f, wt, rgba=None, *, voxel, min_weight=4.0):
    """(points fp32 [P, 3], rgba uint8 [P, 4] or None, weight fp32 [P]): one point per sign change of f between two live voxels that are
    neighbours along an axis, in (voxel, axis) order. keys int64 [M] sorted, f / wt / rgba as tsdf_integrate returns them. A count
    launch, torch.cumsum, a write launch; reads P back (one synchronisation)."""
    lib = _lib.load()
    M, dev = _tsdf_voxels(keys, f, wt, rgba), keys.device
    if M == 0:
        return _no_rows(dev, rgba)
    counts = torch.empty(M, device=dev, dtype=torch.int32)
    _lib.check(lib.geo4d_tsdf_count(keys.data_ptr(), M, f.data_ptr(), wt.data_ptr(), float(min_weight), counts.data_ptr(), _stream()),
               "geo4d_tsdf_count")
    last = torch.cumsum(counts, 0, dtype=torch.int64)
    P = int(last[-1])
    if P == 0:
        return _no_rows(dev, rgba)
    first = (last - counts).contiguous()
    pts = torch.empty((P, 3), device=dev, dtype=torch.float32)
    col = None if rgba is None else torch.empty((P, 4), device=dev, dtype=torch.uint8)
    w = torch.empty(P, device=dev, dtype=torch.float32)
    _lib.check(lib.geo4d_tsdf_write(keys.data_ptr(), M, f.data_ptr(), wt.data_ptr(), _ptr(rgba), first.data_ptr(), P, float(voxel),
                                    float(min_weight), pts.data_ptr(), _ptr(col), w.data_ptr(), _stream()), "geo4d_tsdf_write")
    return pts, col, w


def tsdf_mesh_extract(keys, f, wt, rgba=None, *, voxel, min_weight=4.0):
    """(vertices fp32 [V, 3], rgba uint8 [V, 4] or None, weight fp32 [V], faces int32 [T, 3]): the surface of the field as one indexed
    triangle mesh by naive surface nets (the rule of include/geo4d_hip.h): one vertex per used cell in key order, two triangles per
    sign-changing pair of live neighbours whose four surrounding cells are complete, in (voxel, axis) order, front faces toward positive
    f. keys int64 [M] sorted, f / wt / rgba as tsdf_integrate returns them. A cells and a count launch, two torch.cumsum, a vertices
    and a faces launch; reads (Q, V) back (one synchronisation)."""
    lib = _lib.load()
    M, dev = _tsdf_voxels(keys, f, wt, rgba), keys.device
    no_faces = torch.empty((0, 3), device=dev, dtype=torch.int32)
    if M == 0:
        return _no_rows(dev, rgba, no_faces)
    complete = torch.empty(M, device=dev, dtype=torch.uint8)
    used = torch.empty(M, device=dev, dtype=torch.uint8)
    counts = torch.empty(M, device=dev, dtype=torch.int32)
    _lib.check(lib.geo4d_tsdf_mesh_cells(keys.data_ptr(), M, f.data_ptr(), wt.data_ptr(), float(min_weight), complete.data_ptr(), _stream()),
               "geo4d_tsdf_mesh_cells")
    _lib.check(lib.geo4d_tsdf_mesh_count(keys.data_ptr(), M, complete.data_ptr(), counts.data_ptr(), used.data_ptr(), _stream()),
               "geo4d_tsdf_mesh_count")
    last_quad = torch.cumsum(counts, 0, dtype=torch.int64)
    last_vertex = torch.cumsum(used, 0, dtype=torch.int64)
    Q, V = torch.stack([last_quad[-1], last_vertex[-1]]).tolist()
    if Q == 0:
        return _no_rows(dev, rgba, no_faces)
    first_quad, first_vertex = (last_quad - counts).contiguous(), (last_vertex - used).contiguous()
    vertices = torch.empty((V, 3), device=dev, dtype=torch.float32)
    col = None if rgba is None else torch.empty((V, 4), device=dev, dtype=torch.uint8)
    w = torch.empty(V, device=dev, dtype=torch.float32)
    faces = torch.empty((2 * Q, 3), device=dev, dtype=torch.int32)
    _lib.check(lib.geo4d_tsdf_mesh_vertices(keys.data_ptr(), M, f.data_ptr(), wt.data_ptr(), _ptr(rgba), used.data_ptr(), first_vertex.data_ptr(),
                                            V, float(voxel), vertices.data_ptr(), _ptr(col), w.data_ptr(), _stream()), "geo4d_tsdf_mesh_vertices")
    _lib.check(lib.geo4d_tsdf_mesh_faces(keys.data_ptr(), M, f.data_ptr(), complete.data_ptr(), counts.data_ptr(), first_quad.data_ptr(),
                                         first_vertex.data_ptr(), Q, V, faces.data_ptr(), _stream()), "geo4d_tsdf_mesh_faces")
    return vertices, col, w, faces


def _mesh_faces(faces, mask, what):
    """(T, mask as contiguous uint8 or None) of faces int32 [T, 3] and a per-face mask [T] (bool or uint8) on the HIP device."""
    T = _want(faces, "faces", torch.int32, (None, 3)).shape[0]
    if mask is not None:
        assert tuple(_dev(mask, what).shape) == (T,) and mask.dtype in (torch.bool, torch.uint8), (what, mask.dtype, tuple(mask.shape))
        mask = mask.contiguous().view(torch.uint8)                  # a bool's byte is 0 or 1
    return T, mask


def mesh_components(faces, n_vertices, face_mask=None):
    """(vertex_component int32 [Nv], face_component int32 [T], component_vertices int32 [C], component_faces int32 [C]): the connected
    pieces of the mesh faces int32 [T, 3] over `n_vertices` vertices (the rule of include/geo4d_hip.h): a face is valid iff `face_mask`
    ([T] bool or uint8; None: every face) lets it through and its indices lie in [0, Nv); vertices joined by a chain of valid faces
    sharing a vertex are one component, numbered in ascending order of their smallest vertex; -1 marks a vertex no valid face names and
    a face that is not valid. A hook (lock-free union-find), a flatten and a count launch with one torch.cumsum between; reads C back
    (one synchronisation)."""
    lib = _lib.load()
    Nv = int(n_vertices)
    assert 0 <= Nv < 1 << 31, n_vertices
    T, mask = _mesh_faces(faces, face_mask, "face_mask")
    dev = faces.device
    none = torch.empty(0, device=dev, dtype=torch.int32)
    vertex_component = torch.full((Nv,), -1, device=dev, dtype=torch.int32)
    face_component = torch.full((T,), -1, device=dev, dtype=torch.int32)
    if T == 0 or Nv == 0:
        return vertex_component, face_component, none, none.clone()
    parent, root = torch.empty(Nv, device=dev, dtype=torch.int32), torch.empty(Nv, device=dev, dtype=torch.int32)
    touched, is_root = torch.empty(Nv, device=dev, dtype=torch.uint8), torch.empty(Nv, device=dev, dtype=torch.uint8)
    _lib.check(lib.geo4d_mesh_components_hook(faces.data_ptr(), T, Nv, _ptr(mask), parent.data_ptr(), touched.data_ptr(), _stream()),
               "geo4d_mesh_components_hook")
    _lib.check(lib.geo4d_mesh_components_flatten(parent.data_ptr(), touched.data_ptr(), Nv, root.data_ptr(), is_root.data_ptr(), _stream()),
               "geo4d_mesh_components_flatten")
    last = torch.cumsum(is_root, 0, dtype=torch.int64)
    C = int(last[-1])
    if C == 0:
        return vertex_component, face_component, none, none.clone()
    first = (last - is_root).contiguous()
    component_vertices, component_faces = torch.empty(C, device=dev, dtype=torch.int32), torch.empty(C, device=dev, dtype=torch.int32)
    _lib.check(lib.geo4d_mesh_components_count(faces.data_ptr(), T, Nv, _ptr(mask), root.data_ptr(), first.data_ptr(), C,
                                               vertex_component.data_ptr(), face_component.data_ptr(), component_vertices.data_ptr(),
                                               component_faces.data_ptr(), _stream()), "geo4d_mesh_components_count")
    return vertex_component, face_component, component_vertices, component_faces


def mesh_select(vertices, faces, keep_face, rgba=None, weight=None):
    """(vertices fp32 [V', 3], rgba uint8 [V', 4] or None, weight fp32 [V'] or None, faces int32 [T', 3], vertex_index int32 [V']): the
    mesh of the kept faces (the rule of include/geo4d_hip.h): face t is kept iff keep_face[t] ([T] bool or uint8) is set and its indices
    lie in [0, Nv); a vertex is kept iff a kept face names it; both keep their relative order, faces are rewritten to the new vertex rows
    and vertex_index is the old row of every new one. A mark launch, two torch.cumsum, a gather launch; reads (V', T') back (one
    synchronisation)."""
    lib = _lib.load()
    Nv = _want(vertices, "vertices", torch.float32, (None, 3)).shape[0]
    T, keep = _mesh_faces(faces, keep_face, "keep_face")
    assert keep is not None, "keep_face is required"
    if rgba is not None:
        _want(rgba, "rgba", torch.uint8, (Nv, 4))
    if weight is not None:
        _want(weight, "weight", torch.float32, (Nv,))
    dev = vertices.device

    def nothing():
        return (torch.empty((0, 3), device=dev, dtype=torch.float32), None if rgba is None else torch.empty((0, 4), device=dev, dtype=torch.uint8),
                None if weight is None else torch.empty(0, device=dev, dtype=torch.float32),
                torch.empty((0, 3), device=dev, dtype=torch.int32), torch.empty(0, device=dev, dtype=torch.int32))
    if T == 0 or Nv == 0:
        return nothing()
    keep_vertex, kept = torch.empty(Nv, device=dev, dtype=torch.uint8), torch.empty(T, device=dev, dtype=torch.uint8)
    _lib.check(lib.geo4d_mesh_select_mark(faces.data_ptr(), T, Nv, keep.data_ptr(), keep_vertex.data_ptr(), kept.data_ptr(), _stream()),
               "geo4d_mesh_select_mark")
    last_vertex, last_face = torch.cumsum(keep_vertex, 0, dtype=torch.int64), torch.cumsum(kept, 0, dtype=torch.int64)
    V, F = torch.stack([last_vertex[-1], last_face[-1]]).tolist()
    if F == 0:
        return nothing()
    first_vertex, first_face = (last_vertex - keep_vertex).contiguous(), (last_face - kept).contiguous()
    out = torch.empty((V, 3), device=dev, dtype=torch.float32)
    col = None if rgba is None else torch.empty((V, 4), device=dev, dtype=torch.uint8)
    w = None if weight is None else torch.empty(V, device=dev, dtype=torch.float32)
    new_faces, vertex_index = torch.empty((F, 3), device=dev, dtype=torch.int32), torch.empty(V, device=dev, dtype=torch.int32)
    _lib.check(lib.geo4d_mesh_select_gather(vertices.data_ptr(), _ptr(rgba), _ptr(weight), faces.data_ptr(), T, Nv, keep_vertex.data_ptr(),
                                            kept.data_ptr(), first_vertex.data_ptr(), first_face.data_ptr(), V, F, out.data_ptr(), _ptr(col),
                                            _ptr(w), new_faces.data_ptr(), vertex_index.data_ptr(), _stream()), "geo4d_mesh_select_gather")
    return out, col, w, new_faces, vertex_index


# Rows of the corner table longer than this are sorted, and searched for boundary neighbours, by a whole wave instead of one thread
# (csrc/mesh_smooth.hip). Both paths give the same table; the value only decides the time. tools/mesh_smooth_bench.py sweeps it: on the
# TSDF bench mesh (rows of 6 on average, 18 at most) the table takes 0.44 / 0.42 / 0.30 / 0.28 / 0.32 ms at 0 / 4 / 8 / 16 / 32 and above,
# and with a row of 4000 entries added 119 ms at every value up to 128 against 559 ms by one thread (profiles/mesh_smooth.md).
MESH_LONG_ROW = 16


def _mesh_table(faces, offsets, corners, Nv):
    """(T, E) of faces int32 [T, 3] with the corner table offsets int32 [Nv + 1], corners int32 [E] on the HIP device."""
    T = _want(faces, "faces", torch.int32, (None, 3)).shape[0]
    _want(offsets, "offsets", torch.int32, (Nv + 1,))
    E = _want(corners, "corners", torch.int32, (None,)).shape[0]
    assert E <= 3 * T, (E, T)
    return T, E


def mesh_adjacency(faces, n_vertices, face_mask=None, *, long_row=None):
    """(offsets int32 [Nv + 1], corners int32 [E], boundary uint8 [Nv]): the corner table of the mesh faces int32 [T, 3] over
    `n_vertices` vertices and its boundary vertices (the rule of include/geo4d_hip.h). An entry e = 3 t + k stands for corner k of the
    valid face t (`face_mask` [T] bool or uint8 lets it through, indices in [0, Nv)) and lies in the row of vertex faces[t][k]; row v is
    corners[offsets[v]:offsets[v + 1]], ascending. boundary[v] = 1 iff some neighbour stands exactly once in v's neighbour list. Rows
    longer than `long_row` (None: MESH_LONG_ROW) are handled by a wave instead of a thread; the result is the same. A count launch, one
    torch.cumsum, a fill, a sort and a boundary launch; reads E back (one synchronisation)."""
    lib = _lib.load()
    Nv = int(n_vertices)
    assert 0 <= Nv < 1 << 31, n_vertices
    long_row = MESH_LONG_ROW if long_row is None else int(long_row)
    assert 0 <= long_row < 1 << 31, long_row
    T, mask = _mesh_faces(faces, face_mask, "face_mask")
    dev = faces.device
    offsets = torch.zeros(Nv + 1, device=dev, dtype=torch.int32)
    boundary = torch.zeros(Nv, device=dev, dtype=torch.uint8)
    none = torch.empty(0, device=dev, dtype=torch.int32)
    if T == 0 or Nv == 0:
        return offsets, none, boundary
    degree = torch.zeros(Nv, device=dev, dtype=torch.int32)
    _lib.check(lib.geo4d_mesh_adjacency_count(faces.data_ptr(), T, Nv, _ptr(mask), degree.data_ptr(), _stream()), "geo4d_mesh_adjacency_count")
    torch.cumsum(degree, 0, dtype=torch.int32, out=offsets[1:])
    E = int(offsets[-1])
    if E == 0:
        return offsets, none, boundary
    cursor = degree.zero_()
    unsorted, corners = torch.empty(E, device=dev, dtype=torch.int32), torch.empty(E, device=dev, dtype=torch.int32)
    _lib.check(lib.geo4d_mesh_adjacency_fill(faces.data_ptr(), T, Nv, _ptr(mask), offsets.data_ptr(), E, cursor.data_ptr(),
                                             unsorted.data_ptr(), _stream()), "geo4d_mesh_adjacency_fill")
    _lib.check(lib.geo4d_mesh_adjacency_sort(offsets.data_ptr(), T, Nv, E, unsorted.data_ptr(), corners.data_ptr(), long_row, _stream()),
               "geo4d_mesh_adjacency_sort")
    _lib.check(lib.geo4d_mesh_boundary(faces.data_ptr(), T, Nv, offsets.data_ptr(), corners.data_ptr(), E, long_row, boundary.data_ptr(),
                                       _stream()), "geo4d_mesh_boundary")
    return offsets, corners, boundary


def mesh_smooth_step(vertices, faces, offsets, corners, s, pinned=None, *, out=None):
    """fp32 [Nv, 3]: one Jacobi smoothing step with factor `s` (the rule of include/geo4d_hip.h): every vertex moves by s times the way
    to the mean of its neighbour list (mesh_adjacency's table; a neighbour seen from two faces counts twice); a vertex without
    neighbours, or with pinned[v] != 0 (`pinned` [Nv] bool or uint8), keeps its bits. One launch into `out` (None: a new tensor),
    which is never `vertices`."""
    lib = _lib.load()
    Nv = _want(vertices, "vertices", torch.float32, (None, 3)).shape[0]
    T, E = _mesh_table(faces, offsets, corners, Nv)
    if pinned is not None:
        assert tuple(_dev(pinned, "pinned").shape) == (Nv,) and pinned.dtype in (torch.bool, torch.uint8), (pinned.dtype, tuple(pinned.shape))
        pinned = pinned.contiguous().view(torch.uint8)
    if out is None:
        out = torch.empty_like(vertices)
    assert _want(out, "out", torch.float32, (Nv, 3)).data_ptr() != vertices.data_ptr() or Nv == 0, "a step is never in place"
    if T == 0 or Nv == 0:
        return out.copy_(vertices)
    _lib.check(lib.geo4d_mesh_smooth_step(vertices.data_ptr(), faces.data_ptr(), T, Nv, offsets.data_ptr(), corners.data_ptr(), E,
                                          _ptr(pinned), float(s), out.data_ptr(), _stream()), "geo4d_mesh_smooth_step")
    return out


def mesh_vertex_normals(vertices, faces, offsets, corners):
    """fp32 [Nv, 3]: area-weighted unit vertex normals (the rule of include/geo4d_hip.h): the sum of the cross products (p1 - p0) x
    (p2 - p0) of the faces in the vertex's row of mesh_adjacency's table, in the row's order, divided by its length; (0, 0, 0) where
    that length is not positive and finite (a vertex no valid face names among them). One launch."""
    lib = _lib.load()
    Nv = _want(vertices, "vertices", torch.float32, (None, 3)).shape[0]
    T, E = _mesh_table(faces, offsets, corners, Nv)
    if T == 0 or Nv == 0:
        return torch.zeros_like(vertices)
    out = torch.empty_like(vertices)
    _lib.check(lib.geo4d_mesh_vertex_normals(vertices.data_ptr(), faces.data_ptr(), T, Nv, offsets.data_ptr(), corners.data_ptr(), E,
                                             out.data_ptr(), _stream()), "geo4d_mesh_vertex_normals")
    return out


class NNGrid:
    """The cell grid of one reference set (the rule of include/geo4d_hip.h): `radius` (the cell side), cell_keys int64 [M] sorted and
    unique, cell_start int32 [M + 1], ref_sorted fp32 [Nt, 3] and ref_row int32 [Nt] (the taking-part points in (key, row) order and
    their original rows), n_reference = Nr, n_taking = Nt, and `dropped`, the reference points outside the grid (an int)."""

    def __init__(self, radius, cell_keys, cell_start, ref_sorted, ref_row, n_reference, n_taking, dropped, device):
        self.radius, self.cell_keys, self.cell_start, self.ref_sorted, self.ref_row = radius, cell_keys, cell_start, ref_sorted, ref_row
        self.n_reference, self.n_taking, self.dropped, self.device = n_reference, n_taking, dropped, device


def check_nn_radius(radius, who="nearest_points", what="radius"):
    """The fp32 radius; ValueError unless it is finite and > 0 in fp32 and so is its square."""
    try:
        r = torch.tensor(float(radius), dtype=torch.float32)
        r, r2 = r.item(), (r * r).item()
    except (TypeError, ValueError):
        r = r2 = float("nan")
    if not (r > 0 and r2 < float("inf")):
        raise ValueError(f"{who}: {what} must be finite and > 0 in fp32, and so must its square, got {radius!r}")
    return r


def check_min_neighbours(min_neighbours, who="radius_outliers"):
    if isinstance(min_neighbours, bool) or not isinstance(min_neighbours, int) or min_neighbours < 0:
        raise ValueError(f"{who}: min_neighbours must be an integer >= 0, got {min_neighbours!r}")
    return min_neighbours


def _nn_mask(mask, N):
    if mask is None:
        return None
    assert tuple(_dev(mask, "mask").shape) == (N,), mask.shape
    return mask.to(torch.bool).contiguous()


def _nn_sorted_rows(points, mask, radius):
    """(order int64 [N], taking, dropped, sorted keys int64 [taking]): the rows of points fp32 [N, 3] (N > 0), the `taking` taking-part
    ones first in (key, row) order. One launch (geo4d_nn_keys), one stable torch.sort, and one synchronisation for the two counts. A
    point that takes no part has the key -1 (all ones), which the signed sort puts first: the order is rolled so that they come last."""
    N, dev = points.shape[0], points.device
    keys, dropped = torch.empty(N, device=dev, dtype=torch.int64), torch.empty(1, device=dev, dtype=torch.int64)
    _lib.check(_lib.load().geo4d_nn_keys(points.data_ptr(), _ptr(mask), N, radius, keys.data_ptr(), dropped.data_ptr(), _stream()),
               "geo4d_nn_keys")
    skeys, order = torch.sort(keys, stable=True)
    taking, n_dropped = torch.cat([(keys >= 0).sum().reshape(1), dropped]).tolist()
    out = N - taking
    return torch.cat([order[out:], order[:out]]).contiguous(), taking, n_dropped, skeys[out:]


def nn_grid(reference, *, radius, mask=None):
    """The NNGrid of reference fp32 [Nr, 3] (mask bool [Nr] or None) for cells of side `radius`, on the HIP device. geo4d_nn_keys and
    geo4d_nn_gather are HIP launches; between them torch.sort (stable) orders the keys, torch.unique_consecutive and torch.cumsum make
    cell_keys and cell_start. Reads Nt and the dropped count back in one synchronisation. Reusable for any number of nn_query calls."""
    Nr, dev = _want(reference, "reference", torch.float32, (None, 3)).shape[0], reference.device
    mask = _nn_mask(mask, Nr)
    radius = float(radius)
    empty = lambda dt, *shape: torch.empty(shape, device=dev, dtype=dt)
    if Nr == 0:
        return NNGrid(radius, empty(torch.int64, 0), torch.zeros(1, device=dev, dtype=torch.int32), empty(torch.float32, 0, 3),
                      empty(torch.int32, 0), 0, 0, 0, dev)
    assert Nr < 1 << 31, Nr
    order, Nt, dropped, skeys = _nn_sorted_rows(reference, mask, radius)
    cell_keys, counts = torch.unique_consecutive(skeys, return_counts=True)
    cell_start = torch.zeros(cell_keys.shape[0] + 1, device=dev, dtype=torch.int32)
    torch.cumsum(counts, 0, dtype=torch.int32, out=cell_start[1:])
    ref_sorted, ref_row = empty(torch.float32, Nt, 3), empty(torch.int32, Nt)
    if Nt:
        _lib.check(_lib.load().geo4d_nn_gather(reference.data_ptr(), order.data_ptr(), Nt, Nr, ref_sorted.data_ptr(), ref_row.data_ptr(),
                                               _stream()), "geo4d_nn_gather")
    return NNGrid(radius, cell_keys.contiguous(), cell_start, ref_sorted, ref_row, Nr, Nt, dropped, dev)


def nn_query(grid, query, *, mask=None, exclude_same_row=False):
    """(index int32 [Nq], dist2 fp32 [Nq], count int32 [Nq], dropped int) of query fp32 [Nq, 3] (mask bool [Nq] or None) against an
    NNGrid (the rule of include/geo4d_hip.h): the nearest reference row within grid.radius (-1: none), its squared distance (+inf) and
    the number of reference points within; `dropped` counts the queries outside the grid, which get (-1, +inf, 0) like every query
    that takes no part. geo4d_nn_keys, a stable torch.sort of the queries' keys, then geo4d_nn_query; one synchronisation. No query, or
    a grid without points, launches nothing."""
    Nq, dev = _want(query, "query", torch.float32, (None, 3)).shape[0], query.device
    assert grid.device == dev, (grid.device, dev)
    mask = _nn_mask(mask, Nq)
    index = torch.full((Nq,), -1, device=dev, dtype=torch.int32)
    dist2 = torch.full((Nq,), float("inf"), device=dev, dtype=torch.float32)
    count = torch.zeros(Nq, device=dev, dtype=torch.int32)
    if Nq == 0:
        return index, dist2, count, 0
    assert Nq < 1 << 31, Nq
    order, taking, dropped, _ = _nn_sorted_rows(query, mask, grid.radius)
    if grid.n_taking == 0 or taking == 0:
        return index, dist2, count, dropped
    _lib.check(_lib.load().geo4d_nn_query(query.data_ptr(), order.data_ptr(), taking, Nq, grid.cell_keys.data_ptr(), grid.cell_start.data_ptr(),
                                          grid.cell_keys.shape[0], grid.ref_sorted.data_ptr(), grid.ref_row.data_ptr(), grid.n_taking,
                                          grid.n_reference, grid.radius, int(bool(exclude_same_row)), index.data_ptr(), dist2.data_ptr(),
                                          count.data_ptr(), _stream()), "geo4d_nn_query")
    return index, dist2, count, dropped


def tsdf_field(pts3d, depth, valid, views, centres, rgba=None, weight=None, *, voxel, trunc=4, near=1e-3, capacity=None):
    """The TSDF field of a scene (the rule of include/geo4d_hip.h): (K int64 [M] sorted keys, f fp32 [M], wt fp32 [M], col uint8 [M, 4]
    or None, M, dropped); K, f, wt and col are None when no voxel was marked. Inputs as tsdf_points takes them. Mark, compact and
    integrate are HIP launches; the marked keys are sorted with torch.sort. Raises TsdfTableFull when the table overflowed."""
    n, H, W, valid = _tsdf_maps(pts3d, depth, valid, rgba, weight)
    dev = pts3d.device
    if capacity is None:
        part = torch.isfinite(pts3d).all(-1) & torch.isfinite(depth) & (depth > torch.tensor(float(near), dtype=torch.float32, device=dev))
        taking = int((part if valid is None else part & valid).sum())
        if taking == 0:                                             # no pixel: no table
            return None, None, None, None, 0, 0
        capacity = tsdf_capacity(taking)
    table, counters = tsdf_mark(pts3d, depth, valid, centres, voxel=voxel, trunc=trunc, near=near, capacity=capacity)
    keys, count = tsdf_compact(table)
    M, dropped, overflow = torch.cat([count, counters]).tolist()
    if overflow:
        raise TsdfTableFull(f"tsdf_points: overflow = {overflow} > 0: that many samples found no free slot among the table's capacity = "
                            f"{capacity}; pass capacity >= {1 << (int(capacity) + overflow - 1).bit_length()}")
    if M == 0:
        return None, None, None, None, 0, dropped
    K = torch.sort(keys[:M]).values.contiguous()                    # keys < 2^63: signed order is unsigned order
    return (K, *tsdf_integrate(K, depth, valid, views, rgba, weight, voxel=voxel, trunc=trunc, near=near), M, dropped)


def tsdf_points(pts3d, depth, valid, views, centres, rgba=None, weight=None, *, voxel, trunc=4, min_weight=4.0, near=1e-3, capacity=None):
    """The surface points of the TSDF of a scene (the rule of include/geo4d_hip.h): (points fp32 [P, 3], rgba uint8 [P, 4] or None,
    weight fp32 [P], voxels, dropped). pts3d fp32 [n, H, W, 3], depth fp32 [n, H, W], valid bool [n, H, W] or None, views fp32 [n, 16],
    centres fp32 [n, 3], rgba uint8 [n, H, W, 4], weight fp32 [n, H, W] on the HIP device. `capacity`: the table's size, a power of two
    (default: >= 4 x the taking-part pixels, which are counted with torch). Mark, compact, integrate (tsdf_field), count and write are
    HIP launches; the marked keys are sorted with torch.sort. Raises TsdfTableFull when the table overflowed."""
    K, f, wt, col, M, dropped = tsdf_field(pts3d, depth, valid, views, centres, rgba, weight, voxel=voxel, trunc=trunc, near=near,
                                           capacity=capacity)
    if M == 0:
        return _no_rows(pts3d.device, rgba, 0, dropped)
    return (*tsdf_extract(K, f, wt, col, voxel=voxel, min_weight=min_weight), M, dropped)


def focal_shift(points, weight=None, thr=0.5, downsample_size=None, z_offset=None, iters=40):
    """(shift [B], focal [B] fp32, status [B] int32) of point maps `points` fp32 [B, H, W, 3] (any map stride: `pred[:, 0]` is used in
    place): the z-shift and normalised focal that minimise sum |focal * xy / (z + shift) - uv|^2 over the pixels with `weight` [B, H, W]
    > `thr` (None: all) - utils.geometry.solve_optimal_shift_focal(..., ransac_iters=None) for every map in one enqueue, nothing read back.
    `downsample_size` (h, w): solve on F.interpolate(mode="nearest")'s sample of the maps (None: every pixel); `z_offset`: device fp32
    scalar added to every z; `iters`: solver iterations enqueued (converged maps skip theirs). status: 0 ok, 1 fewer than 3 selected
    pixels, 2 non-finite / non-positive result."""
    lib = _lib.load()
    _dev(points, "points")
    if points.dtype != torch.float32 or points.dim() != 4 or points.shape[-1] != 3 or 0 in points.shape:
        raise ValueError(f"focal_shift: points must be a non-empty fp32 [B, H, W, 3] tensor, got {points.dtype} {tuple(points.shape)}")
    B, H, W, _ = points.shape
    if points.stride()[1:] != (3 * W, 3, 1) or (B > 1 and points.stride(0) < 0):
        points = points.contiguous()
    wp, wstride = None, 0
    if weight is not None:
        _dev(weight, "weight")
        if tuple(weight.shape) != (B, H, W) or weight.device != points.device:
            raise ValueError(f"focal_shift: weight must be [B, H, W] = {(B, H, W)} on {points.device}, got {tuple(weight.shape)} on {weight.device}")
        if weight.dtype != torch.float32:
            weight = weight.float()
        if weight.stride()[1:] != (W, 1) or (B > 1 and weight.stride(0) < 0):
            weight = weight.contiguous()
        wp, wstride = weight.data_ptr(), weight.stride(0)
    if z_offset is not None:
        _dev(z_offset, "z_offset")
        if z_offset.dtype != torch.float32 or z_offset.numel() != 1 or z_offset.device != points.device:
            raise ValueError("focal_shift: z_offset must be ONE fp32 value on the points' device")
    h_lr, w_lr = (H, W) if downsample_size is None else (int(downsample_size[0]), int(downsample_size[1]))
    if h_lr <= 0 or w_lr <= 0 or int(iters) <= 0:
        raise ValueError(f"focal_shift: downsample_size {downsample_size} and iters {iters} must be positive")
    shift = torch.empty(B, device=points.device, dtype=torch.float32)
    focal = torch.empty(B, device=points.device, dtype=torch.float32)
    status = torch.empty(B, device=points.device, dtype=torch.int32)
    need = lib.geo4d_focal_shift_workspace(B, h_lr, w_lr)
    ws = torch.empty(need // 8, device=points.device, dtype=torch.float64)
    _lib.check(lib.geo4d_focal_shift(points.data_ptr(), points.stride(0), wp, wstride, float(thr), _ptr(z_offset), B, H, W, h_lr, w_lr, int(iters),
                                     shift.data_ptr(), focal.data_ptr(), status.data_ptr(), ws.data_ptr(), need, _stream()), "geo4d_focal_shift")
    return shift, focal, status


PNP_FEW, PNP_NO_CONSENSUS, PNP_BAD_FOCAL, PNP_BAD_TABLES = 1, 2, 4, 8       # status bits of pnp_ransac


class PnpTables:
    """pnp.sample_tables of B images on the device, in the layout geo4d_pnp_ransac reads: n [B], m [B], sub [B, max_points],
    draws [B, iterations, 6], all int32 (rows padded with zeros). Built once per set of masked-pixel counts and reused."""

    def __init__(self, tables, n, iterations, device):
        import numpy as np
        B = len(tables)
        if B == 0 or len(n) != B:
            raise ValueError("pnp tables: one (sub, draws) pair and one masked-pixel count per image")
        self.iterations = int(iterations)
        self.max_points = max(6, max(len(t[0]) for t in tables))
        sub = np.zeros((B, self.max_points), np.int32)
        draws = np.zeros((B, self.iterations, 6), np.int32)
        m = np.zeros(B, np.int32)
        for b, (s, d) in enumerate(tables):
            s, d = np.asarray(s), np.asarray(d)
            if d.size and (d.shape[0] < self.iterations or d.shape[1] != 6):
                raise ValueError(f"pnp tables: draws of image {b} are {d.shape}, need at least [{self.iterations}, 6]")
            m[b] = len(s)
            sub[b, :len(s)] = s
            if d.size:
                draws[b] = d[:self.iterations]
        host = torch.from_numpy(np.concatenate([np.asarray(n, np.int32).reshape(B), m, sub.reshape(-1), draws.reshape(-1)]))
        flat = host.to(device)                                  # one upload
        self.B = B
        self.n, self.m = flat[:B], flat[B:2 * B]
        self.sub = flat[2 * B:2 * B + B * self.max_points].view(B, self.max_points)
        self.draws = flat[2 * B + B * self.max_points:].view(B, self.iterations * 6)

    def rows(self, which):
        """The tables of the images `which` (a list of indices) as another PnpTables: views for a contiguous run, else a device gather."""
        which = [int(w) for w in which]
        t = object.__new__(PnpTables)
        t.B, t.iterations, t.max_points = len(which), self.iterations, self.max_points
        if which == list(range(which[0], which[0] + len(which))):
            sl = slice(which[0], which[0] + len(which))
            t.n, t.m, t.sub, t.draws = self.n[sl], self.m[sl], self.sub[sl], self.draws[sl]
        else:
            ix = torch.as_tensor(which, device=self.n.device)
            t.n, t.m, t.sub, t.draws = self.n[ix], self.m[ix], self.sub[ix], self.draws[ix]
        return t


def pnp_ransac(points, conf, cand_focals, tables, *, thr=0.5, reproj=5.0, iterations, pp=None, out=None):
    """Batched RANSAC-PnP of geo4d_amd/pnp.py on the device (csrc/pnp.hip): B images x C candidate focals in one enqueue, nothing read
    back. points fp32 [B, H, W, 3] world points (any image stride), conf [B, H, W] (pixels with conf > thr take part), cand_focals fp64
    [B, C] ON THE DEVICE (C <= 64); `tables`: a PnpTables, or a list of B `(sub, draws, n)` triples / `(sub, draws)` pairs of
    pnp.sample_tables (n = the image's masked-pixel count; with a pair, len(sub) when that is below the sampler's max_points);
    pp = (x, y), default (W / 2, H / 2). Returns (focal [B] fp64, c2w [B, 4, 4] fp64, status [B] int32, info [B, C, 4] int32): focal and
    pose are written only where status == 0 - pass `out=(focal, c2w)` to keep earlier values on failure (fresh outputs start at NaN).
    status bits: PNP_FEW, PNP_NO_CONSENSUS, PNP_BAD_FOCAL, PNP_BAD_TABLES; info = iterations run, chosen hypothesis, sub-sample inliers
    after the refit, inliers over all masked pixels."""
    lib = _lib.load()
    _dev(points, "points"); _dev(conf, "conf"); _dev(cand_focals, "cand_focals")
    if points.dtype != torch.float32 or points.dim() != 4 or points.shape[-1] != 3 or 0 in points.shape:
        raise ValueError(f"pnp_ransac: points must be a non-empty fp32 [B, H, W, 3] tensor, got {points.dtype} {tuple(points.shape)}")
    B, H, W, _ = points.shape
    if points.stride()[1:] != (3 * W, 3, 1) or (B > 1 and points.stride(0) < 0):
        points = points.contiguous()
    if tuple(conf.shape) != (B, H, W) or conf.device != points.device:
        raise ValueError(f"pnp_ransac: conf must be [B, H, W] = {(B, H, W)} on {points.device}, got {tuple(conf.shape)} on {conf.device}")
    if conf.dtype != torch.float32:
        conf = conf.float()
    if conf.stride()[1:] != (W, 1) or (B > 1 and conf.stride(0) < 0):
        conf = conf.contiguous()
    if cand_focals.dtype != torch.float64 or cand_focals.dim() != 2 or cand_focals.shape[0] != B or not 1 <= cand_focals.shape[1] <= 64:
        raise ValueError(f"pnp_ransac: cand_focals must be fp64 [B, C] with 1 <= C <= 64, got {cand_focals.dtype} {tuple(cand_focals.shape)}")
    cand_focals = cand_focals.contiguous()
    C = cand_focals.shape[1]
    iterations = int(iterations)
    if iterations <= 0:
        raise ValueError(f"pnp_ransac: iterations {iterations} must be positive")
    if not isinstance(tables, PnpTables):
        tables = list(tables)
        tables = PnpTables([t[:2] for t in tables], [t[2] if len(t) > 2 else len(t[0]) for t in tables], iterations, points.device)
    if tables.B != B or tables.iterations != iterations or tables.n.device != points.device:
        raise ValueError(f"pnp_ransac: tables are for {tables.B} images x {tables.iterations} iterations on {tables.n.device}")
    px, py = (W / 2, H / 2) if pp is None else (float(v) for v in torch.as_tensor(pp).reshape(-1).tolist())
    if out is None:
        focal = torch.full((B,), float("nan"), device=points.device, dtype=torch.float64)
        c2w = torch.full((B, 4, 4), float("nan"), device=points.device, dtype=torch.float64)
    else:
        focal, c2w = out
        _dev(focal, "out focal"); _dev(c2w, "out c2w")
        if focal.dtype != torch.float64 or c2w.dtype != torch.float64 or tuple(focal.shape) != (B,) or tuple(c2w.shape) != (B, 4, 4) or \
                not focal.is_contiguous() or not c2w.is_contiguous():
            raise ValueError("pnp_ransac: out = (focal [B], c2w [B, 4, 4]), contiguous fp64")
    status = torch.empty(B, device=points.device, dtype=torch.int32)
    info = torch.empty((B, C, 4), device=points.device, dtype=torch.int32)
    need = lib.geo4d_pnp_ransac_workspace(B, C, H, W, iterations, tables.max_points)
    ws = torch.empty(need // 8, device=points.device, dtype=torch.float64)
    _lib.check(lib.geo4d_pnp_ransac(points.data_ptr(), points.stride(0), conf.data_ptr(), conf.stride(0), float(thr), cand_focals.data_ptr(), px, py,
                                    float(reproj), iterations, 6, tables.n.data_ptr(), tables.m.data_ptr(), tables.sub.data_ptr(),
                                    tables.draws.data_ptr(), tables.max_points, B, C, H, W, focal.data_ptr(), c2w.data_ptr(), status.data_ptr(),
                                    info.data_ptr(), ws.data_ptr(), need, _stream()), "geo4d_pnp_ransac")
    return focal, c2w, status, info
