// geo4d_amd/csrc/gemm_plan.h — the host-side planner of geo4d_conv_gemm: ONE tile table, validate() with the descriptor checks and ONE
// function, resolve(), that turns a (validated) launch descriptor into the kernel variant that runs it. geo4d_conv_gemm launches what the
// plan says, geo4d_conv_gemm_plan and geo4d_conv_gemm_colsum_rows answer from the same plan, so they cannot disagree. Host code only: no
// HIP call, no allocation, no device code. Include after common.h (dtype and return codes).
#pragma once
#include <cstddef>
#include <cstdint>
#include "geo4d_hip.h"

namespace geo4d_gemm {

constexpr int KSLAB_BYTES = 128;      // K bytes per operand row and pipeline stage (8 x 16-byte chunks) in every generation
constexpr int MAX_TAPS = 9;           // KT x KH x KW at most: a row of the kernels' gather tables (their MAXTAP; gemm.hip asserts the two agree)

// The hint number space: first generation (gemm_kernel.h) below 21, second (gemm_kernel_v2.h) 21..70, third (gemm_kernel_v3.h) from 71.
constexpr int generation(int hint) { return hint >= 71 ? 3 : hint >= 21 ? 2 : 1; }

// One row per tile hint: workgroup tile BM x BN on WM x WN waves, and the second-generation tile that takes the launch when this one
// cannot (`alt`; `alt_geglu` where the launch is a GEGLU, which needs wave tiles a multiple of 64 columns wide):
//   first generation  - a pre-split output (o_split), which only the register epilogue of the later generations writes;
//   third generation  - a launch the phased stream cannot take (v3_native); every tile sums in the same order, so the bits are the same;
//   22                - the two-pass f16 type, which has no 256x256 instantiation (that tile spills around its K loop there).
struct Tile {
    int hint, bm, bn, wm, wn, alt, alt_geglu;
    constexpr bool geglu() const { return (bn / wn) % 64 == 0; }
    // rows of the output one gn_colsum entry covers: 32 from the first generation's LDS epilogue, the wave tile's rows from the register epilogue
    constexpr int colsum_rows() const { return generation(hint) == 1 ? 32 : bm / wm; }
};
constexpr Tile TILES[] = {
    {1, 128, 128, 2, 2, 25, 25},  {2, 128, 64, 4, 1, 25, 25},   {3, 64, 128, 2, 2, 27, 27},   {4, 64, 64, 2, 2, 28, 27},    {5, 128, 32, 4, 1, 25, 25},
    {11, 256, 128, 4, 2, 22, 22}, {13, 256, 256, 4, 2, 22, 22}, {16, 160, 320, 5, 2, 23, 22}, {17, 160, 160, 5, 1, 25, 25},
    {22, 256, 256, 4, 2, 23, 25}, {23, 160, 320, 2, 4, 0, 0},   {25, 128, 128, 2, 2, 0, 0},   {27, 64, 128, 2, 2, 0, 0},    {28, 64, 64, 2, 2, 0, 0},
    {71, 192, 256, 2, 4, 22, 22}, {72, 160, 320, 2, 4, 23, 23}, {73, 256, 128, 2, 4, 25, 25}, {74, 128, 256, 2, 4, 25, 25},
};
constexpr int N_SCORED = 5;                      // hints 1..5 = TILES[0..4]: the tiles the library scores itself when the hint is 0
constexpr float SCORED_EFF[N_SCORED] = {1.00f, 0.85f, 0.80f, 0.62f, 0.50f};      // their MFMA efficiency relative to 128x128
constexpr int V2_DEFAULT = 25;                   // where a pre-split output goes from a hint without a row
// two-pass f16 (dtype 4) without a hint: small problems, large ones, large GEGLUs
constexpr int TWO_PASS_SMALL = 25, TWO_PASS_LARGE = 72, TWO_PASS_LARGE_GEGLU = 71;

inline const Tile* find_tile(int hint) {
    for (const Tile& t : TILES)
        if (t.hint == hint) return &t;
    return nullptr;
}

struct Plan {
    int hint = 0;               // the tile that runs (a row of TILES) after defaults, redirects and fall-backs
    int splits = 1;             // gridDim.z / K slices; > 1 is followed by the reduce launch
    int hot = 0;                // operand layout fixed at compile time (4-byte types): 0 generic, 1 raw A x split W, 2 split A x split W
    bool osplit = false;        // the epilogue writes the producers' pre-split format (o_split = 1) / plain f16 rows (o_split = 2)
    int colsum_rows = 0;        // rows per gn_colsum entry this launch emits (would emit, where gn_colsum is null); 0 = it cannot
    int up_w = 0, up_phase = 0; // resolve_up2 only: source width (> 0 = the sub-pixel Upsample kernels) and phase 2 py + px (-1 = the batch index)
    const char* error = nullptr;
};

inline bool aligned(const void* ptr, int bytes) { return ((uintptr_t)ptr % bytes) == 0; }

// gn_colsum of the first generation: one entry per 32 rows from the vectorised LDS epilogue
inline bool colsum_gen1_ok(const geo4d_conv_gemm_t& p, int split_k) {
    const int oesz = p.out_dtype == GEO4D_F32 ? 4 : 2;
    return !(p.M % 32) && !(p.N % 8) && !p.out_nchw && p.act != 2 && p.batch == 1 && split_k == 1 && !((p.ldo * oesz) % 16) && aligned(p.O, 16) &&
           (!p.R || (!((p.ldr * oesz) % 16) && aligned(p.R, 16)));
}
// gn_colsum from the register epilogue's fast path: where the plain f32-row path runs (no activation, no split-K, no pre-split output)
inline bool colsum_fast_ok(const geo4d_conv_gemm_t& p, int sp) {
    return sp == 1 && p.act == 0 && !p.o_split && !p.out_nchw && p.batch == 1 && p.out_dtype == GEO4D_F32 && (p.N & 3) == 0 && (p.ldo & 3) == 0 &&
           aligned(p.O, 16) && (!p.R || ((p.ldr & 3) == 0 && aligned(p.R, 16)));
}
// rows per gn_colsum entry a split-K launch of the second / third generation emits through splitk_reduce_colsum_kernel (0 = it cannot): 32, or 8
// where a frame's rows are a multiple of 8 but not of 32 (the 5 x 8 level: per-frame GroupNorms need blocks that do not straddle frames)
inline int splitk_colsum_rows(const geo4d_conv_gemm_t& p, int sp) {
    if (sp <= 1 || p.batch != 1 || p.act != 0 || p.o_split || p.out_nchw || p.out_dtype != GEO4D_F32 || p.bias_per_row || (p.ldo & 3) || !aligned(p.O, 16) ||
        (p.R && !aligned(p.R, 4))) return 0;
    const int hw = p.Hout * p.Wout;
    if (hw % 32 == 0 && p.M % 32 == 0 && p.N % 64 == 0) return 32;
    if (hw % 8 == 0 && p.M % 8 == 0 && p.N % 256 == 0) return 8;
    return 0;
}

// o_split = 1 (bf16x3, pre-split x pre-split operands only): the output in the producers' pre-split format - needs whole 8-column groups
// and 32-byte aligned rows, has no split-K (the reduce kernel writes plain f32)
inline bool o_split_ok(const geo4d_conv_gemm_t& p, int splits) {
    const long nout = p.act == 2 ? (p.N >> 1) : p.N;
    return splits == 1 && p.w_split && p.a_split && (nout & 7) == 0 && (p.ldo & 7) == 0 && aligned(p.O, 32) &&
           (p.batch == 1 || (p.o_bs & 7) == 0) && (!p.R || ((p.ldr & 3) == 0 && aligned(p.R, 16) && (p.batch == 1 || (p.r_bs & 3) == 0)));
}
// o_split = 2 (the two-pass f16 type): plain f16 rows out - column bias + alpha (+ GEGLU) only, whole 8-column groups, 16-byte aligned rows
inline bool o_f16_ok(const geo4d_conv_gemm_t& p, int splits) {
    const long nout = p.act == 2 ? (p.N >> 1) : p.N;
    return splits == 1 && p.w_split && p.a_split == 2 && (p.act == 0 || p.act == 2) && !p.R && !p.rowbias && !p.bias_per_row && (nout & 7) == 0 && (p.ldo & 7) == 0 &&
           aligned(p.O, 16) && (p.batch == 1 || (p.o_bs & 7) == 0);
}

// Does the third generation's phased stream take this launch? Not an odd number or fewer than 4 K slabs per tile, an uneven split-K,
// outputs that are not 4-element aligned, nearest-upsampling gathers, operands beyond the 2 GB buffer window, a geometry whose rows do not
// walk forward through the input (padding wider than the kernel's reach).
inline bool v3_native(const geo4d_conv_gemm_t& p, int sp, int nslab, long esz, long esz_a) {
    // the phased kernel carries the vector-store epilogue only (its scalar fallback costs ~900 spilled registers there)
    const bool geglu = sp == 1 && p.act == 2;
    const long nout = geglu ? (p.N >> 1) : p.N;
    const long oesz = (sp > 1 || p.out_dtype == GEO4D_F32) ? 4 : 2;
    bool vec_ok = (nout & 3) == 0;
    if (sp > 1) {
        vec_ok = vec_ok && aligned(p.workspace, 16);
    } else {
        vec_ok = vec_ok && (p.ldo & 3) == 0 && aligned(p.O, 4 * oesz) && (p.batch == 1 || (p.o_bs & 3) == 0);
        if (p.R) vec_ok = vec_ok && (p.ldr & 3) == 0 && aligned(p.R, 4 * oesz) && (p.batch == 1 || (p.r_bs & 3) == 0);
    }
    // the staging side addresses each operand through a 2 GB buffer window per tile (see the kernel): nearest-upsampling gathers have
    // no uniform tap offsets, and a tile's rows plus its taps must stay inside the window
    const long frames = 256 / ((long)p.Hout * p.Wout) + 2 + p.KT;
    const bool window_ok = p.ups == 1 && frames * p.Hin * p.Win * p.lda * esz_a < (1L << 31) && (320L * p.ldw + p.K) * esz < (1L << 31);
    // a lane's offset is UNSIGNED and relative to the tap-0 pixel of the tile's first row: that pixel must be the smallest of the tile, i.e.
    // tap-0 pixel(row m) = (f - pt) Hin Win + (oy stride - ph) Win + ox stride - pw must not decrease from the end of one output row to the
    // start of the next, nor from the last row of a frame to the first of the next (a smaller one wraps beyond the window and the row's
    // in-image taps are staged as zeros). The networks' convolutions (pad <= (K - 1) / 2, a 3x3 with pad_end) pass; the first condition
    // is stricter than needed where Hout == 1 and a 1x1 with pad_end fails it - such a launch only runs the tile's alt. The second also
    // bounds a frame's rows by a frame of pixels, which `frames` above assumes.
    const bool forward = (long)p.Wout - 1 <= p.Win && ((long)(p.Hout - 1) * p.Win + (p.Wout - 1)) * p.stride <= (long)p.Hin * p.Win;
    return !(nslab % sp || ((nslab / sp) & 1) || nslab / sp < 4 || !vec_ok || !window_ok || !forward);
}

// Tile choice without a hint (first generation): score = MFMA efficiency of the tile shape x useful fraction x how full the last wave of
// workgroups is (2 workgroups fit per CU by LDS => 512 slots on 256 CUs). Split-K multiplies the workgroup count
// when M x N alone cannot fill the chip and K is deep enough to amortise the extra fp32 slab traffic.
// `hint` 0 scores all of TILES[0..4], 1..5 only that tile; false = nothing applies.
inline bool score_tiles(const geo4d_conv_gemm_t& p, int nslab, int& hint, int& splits) {
    const bool can_split = p.workspace && p.act != 2 && !p.out_nchw && (p.N % 8) == 0 && p.split_k != 1;
    int best = -1, best_split = 1;
    float best_score = -1.f;
    for (int i = 0; i < N_SCORED; ++i) {
        const Tile& c = TILES[i];
        if (p.act == 2 && !c.geglu()) continue;
        if (hint && c.hint != hint) continue;
        const double tm = (p.M + c.bm - 1) / c.bm, tn = (p.N + c.bn - 1) / c.bn;
        const double tiles = tm * tn * p.batch;
        const double useful = ((double)p.M * p.N * p.batch) / (tiles * c.bm * c.bn);
        for (int s = 1; s <= 16; s *= 2) {
            if (s > 1 && (!can_split || nslab / s < 8)) break;
            if (p.split_k > 1 && s != p.split_k) continue;
            if (s > 1 && (size_t)s * p.batch * p.M * p.N * 4 > p.workspace_bytes) break;
            const double wgs = tiles * s;
            const double waves = (double)(long)((wgs + 511) / 512);
            const double fill = wgs / (waves * 512);
            const double split_cost = s > 1 ? 0.92 : 1.0;      // slab write + reduce kernel
            const float score = (float)(SCORED_EFF[i] * useful * (0.30 + 0.70 * fill) * split_cost);
            if (score > best_score) { best_score = score; best = i; best_split = s; }
        }
    }
    if (best < 0) return false;
    hint = TILES[best].hint;
    splits = best_split;
    return true;
}

// The descriptor checks of geo4d_conv_gemm, in the order they have always been made (callers match on the messages): the message of the
// first one that fails, or nullptr. Every refusal, here and in resolve(), returns GEO4D_EINVAL.
inline const char* validate(const geo4d_conv_gemm_t& p) {
    const int esz = (p.dtype == GEO4D_F32 || p.dtype == GEO4D_BF16X3 || p.dtype == GEO4D_F16X2) ? 4 : 2;
    const int bk = KSLAB_BYTES / esz;
    if (p.dtype < 0 || p.dtype > 4 || p.out_dtype < 0 || p.out_dtype > 2) return "conv_gemm: bad dtype";
    if (p.dtype != GEO4D_BF16X3 && p.dtype != GEO4D_F16X2 && (p.a_split || p.w_split)) return "conv_gemm: a_split / w_split are bf16x3 / f16x2 (dtype 3 / 4) options";
    // two-pass f16: plain f16 activation rows x a pre-split f16 weight, f32 rows (or, o_split = 2, plain f16 rows) out, second / third
    // generation tiles (0 = a default per shape)
    if (p.dtype == GEO4D_F16X2 && (p.a_split != 2 || !p.w_split || (p.o_split != 0 && p.o_split != 2) || p.out_nchw || p.out_dtype != GEO4D_F32 || (p.tile_hint != 0 && generation(p.tile_hint) == 1)))
        return "conv_gemm: f16x2 (dtype 4) needs a_split = 2 (plain f16 activation rows) and w_split, a row-major output (f32 rows, or o_split = 2: plain f16 rows), and tile hint 0 or >= 22";
    if (p.o_split) {
        const int nst = p.act == 2 ? p.N / 2 : p.N;
        if ((p.dtype != GEO4D_BF16X3 && p.dtype != GEO4D_F16X2) || (p.dtype == GEO4D_BF16X3 && p.o_split != 1) || p.out_dtype != GEO4D_F32 || !p.a_split || !p.w_split || p.split_k > 1 || p.out_nchw || p.gn_colsum ||
            (nst % 8) || (p.ldo % 8) || (p.o_bs % 8) || ((uintptr_t)p.O % (p.o_split == 2 ? 16 : 32)))
            return "conv_gemm: o_split needs a pre-split x pre-split bf16x3 launch, f32 row-major output, stored columns % 8 == 0, 32-byte aligned rows, no split-K";
    }
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.batch <= 0) return "conv_gemm: empty problem";
    if (p.KT <= 0 || p.KH <= 0 || p.KW <= 0 || p.KT * p.KH * p.KW > MAX_TAPS) return "conv_gemm: at most 9 taps";
    if (p.Cin % bk || p.K != p.Cin * p.KT * p.KH * p.KW) return "conv_gemm: Cin must be a multiple of the 128-byte K slab and K = taps*Cin";
    const int esz_a = p.dtype == GEO4D_F16X2 ? 2 : esz;      // (dtype 4: the activation is plain f16 rows)
    if ((p.lda * esz_a) % 16 || (p.ldw * esz) % 16 || ((uintptr_t)p.A % 16) || ((uintptr_t)p.W % 16) || (p.a_bs * esz_a) % 16 || (p.w_bs * esz) % 16)
        return "conv_gemm: operands must be 16-byte aligned";
    if (p.T <= 0 || p.Hout <= 0 || p.Wout <= 0 || p.Hin <= 0 || p.Win <= 0 || p.M % (p.Hout * p.Wout)) return "conv_gemm: bad geometry";
    if ((p.M / (p.Hout * p.Wout)) % p.T) return "conv_gemm: frames not a multiple of T";
    if ((long)(p.M / (p.Hout * p.Wout)) * p.Hin * p.Win > 2147483647L) return "conv_gemm: more than 2^31 input pixels";
    if (p.ups != 1 && p.ups != 2) return "conv_gemm: ups must be 1 or 2";
    if (p.act == 2 && (p.N % 64 || p.out_nchw || p.R)) return "conv_gemm: GEGLU needs N % 64 == 0, row-major output, no residual";
    if (p.act < 0 || p.act > 3) return "conv_gemm: act must be 0 (none), 1 (SiLU), 2 (GEGLU) or 3 (GELU)";
    if (p.act == 3) {   // GELU lives in the vectorised epilogue only (the scalar NCTHW / odd-shape path stays small enough to unroll)
        const int oesz = p.out_dtype == GEO4D_F32 ? 4 : 2;
        if (p.out_nchw || p.R || (p.N % 8) || ((p.ldo * oesz) % 16) || ((uintptr_t)p.O % 16) || ((p.o_bs * oesz) % 16))
            return "conv_gemm: GELU needs a row-major output with N % 8 == 0, 16-byte aligned rows and no residual";
    }
    if (p.rowbias && p.rowbias_div <= 0) return "conv_gemm: rowbias_div";
    if (p.batch > 65535) return "conv_gemm: batch too large";
    if (!p.zeros || ((uintptr_t)p.zeros % 16)) return "conv_gemm: `zeros` must point at 16 zero bytes (16-byte aligned) in device memory";
    if (p.workspace && ((uintptr_t)p.workspace % 16)) return "conv_gemm: workspace alignment";
    return nullptr;
}

// The kernel variant the (validated) descriptor `p` becomes, or why it cannot run. The gn_colsum pointer only decides whether a launch
// that cannot emit the sums is an error; colsum_rows is filled either way.
inline Plan resolve(const geo4d_conv_gemm_t& p) {
    Plan pl;
    auto refuse = [&pl](const char* why) { pl.error = why; pl.colsum_rows = 0; return pl; };
    const bool two_pass = p.dtype == GEO4D_F16X2, wide = two_pass || p.dtype == GEO4D_BF16X3;
    const long esz = (wide || p.dtype == GEO4D_F32) ? 4 : 2, esz_a = two_pass ? 2 : esz;
    const int nslab = p.K / (KSLAB_BYTES / (int)esz);
    int hint = p.tile_hint, split_k = p.split_k;
    if (two_pass) {      // second / third generation only, never split by default
        if (hint == 0) hint = p.M < 4096 ? TWO_PASS_SMALL : p.act == 2 ? TWO_PASS_LARGE_GEGLU : TWO_PASS_LARGE;
        if (split_k == 0) split_k = 1;
    }
    const Tile* t = find_tile(hint);
    if (generation(hint) == 1 && p.o_split) {
        hint = !t ? V2_DEFAULT : p.act == 2 ? t->alt_geglu : t->alt;
        t = find_tile(hint);
    }
    int gen = generation(hint);
    if (gen > 1 && !wide && p.dtype != GEO4D_BF16)
        return refuse("conv_gemm: tile hints 22..28 and 71..74 serve bf16 / bf16x3 / f16x2 (the exact-f32 and the f16 modes stay on hints 0..17)");
    if (gen > 1 && p.out_nchw) return refuse("conv_gemm: tile hints 22..28 and 71..74 have no NCTHW epilogue");
    if (gen == 1 && hint <= N_SCORED) {
        if (!score_tiles(p, nslab, hint, pl.splits)) return refuse("conv_gemm: no tile configuration (split_k / tile_hint not applicable to this problem?)");
        t = find_tile(hint);
    } else if (split_k > 1) {
        if (!p.workspace || p.act == 2 || (gen == 1 && p.out_nchw) || (p.N % 8) || (size_t)split_k * p.batch * p.M * p.N * 4 > p.workspace_bytes || nslab / split_k < 1)
            return refuse("conv_gemm: split_k not applicable (workspace too small / epilogue not splittable)");
        pl.splits = split_k;
    }
    if (!t) return refuse("conv_gemm: unknown tile_hint");
    if (gen == 3 && !v3_native(p, pl.splits, nslab, esz, esz_a)) {
        t = find_tile(t->alt);
        gen = 2;
    }
    if (gen == 2 && two_pass && t->alt) t = find_tile(p.act == 2 ? t->alt_geglu : t->alt);
    pl.hint = t->hint;
    if (p.act == 2 && !t->geglu()) return refuse("conv_gemm: GEGLU needs wave tiles that are a multiple of 64 columns wide");
    if (p.o_split) {
        if (!wide) return refuse("conv_gemm: o_split is a bf16x3 / f16x2 option");
        if (two_pass ? !o_f16_ok(p, pl.splits) : !o_split_ok(p, pl.splits))
            return refuse(two_pass ? "conv_gemm: o_split = 2 (plain f16 rows out) needs no split-K / residual / row biases / SiLU / GELU, stored columns % 8 == 0 and 16-byte aligned output rows"
                                   : "conv_gemm: o_split needs pre-split x pre-split operands, no split-K, N % 8 == 0 and 32-byte aligned output rows");
        pl.hot = 2;
        pl.osplit = true;
    } else if (two_pass) {
        pl.hot = 2;
    } else if (wide && p.w_split) {
        pl.hot = p.a_split ? 2 : 1;
    }
    if (gen == 1) pl.colsum_rows = colsum_gen1_ok(p, split_k) ? t->colsum_rows() : 0;
    else if (pl.splits > 1) pl.colsum_rows = splitk_colsum_rows(p, pl.splits);      // from the reduce launch
    else pl.colsum_rows = (colsum_fast_ok(p, 1) && p.M % t->colsum_rows() == 0) ? t->colsum_rows() : 0;
    if (p.gn_colsum && (!pl.colsum_rows || (pl.splits == 1 && !aligned(p.gn_colsum, 16))))
        return refuse("conv_gemm: this launch cannot emit gn_colsum (geo4d_conv_gemm_colsum_rows): it needs a row-major 16-byte aligned output, batch 1, no GEGLU, "
                      "M a multiple of the rows per entry; first generation: no split-K; later generations: f32 rows, no activation");
    return pl;
}

// geo4d_conv_gemm_up2: the (validated) descriptor `p` is a 2x2 convolution on the source grid whose rows land on phase 2 py + px of the
// nearest-2x grid (`phase` 0..3: one launch per phase with ph = 1 - py, pw = 1 - px; -1: the four phases are the batch index, which then
// steps through the weights only). The launch runs the plan resolve() gives the same descriptor, on the kernels that carry the row
// mapping: bf16x3 against a pre-split weight, tile hints 22, 23, 25, 71, 72, plain f32 rows with a column bias. gn_colsum entries of the
// four phases interleave ([M / rows][4][N][2]), so a frame's entries stay contiguous where its source rows are a multiple of `rows`.
inline Plan resolve_up2(const geo4d_conv_gemm_t& p, int src_w, int phase) {
    Plan pl;
    auto refuse = [&pl](const char* why) { pl.error = why; pl.colsum_rows = 0; return pl; };
    if (p.dtype != GEO4D_BF16X3 || !p.w_split)
        return refuse("conv_gemm_up2: the sub-pixel form serves bf16x3 (dtype 3) against a pre-split weight; the other modes keep the ups = 2 gather");
    if (p.ups != 1 || p.KT != 1 || p.KH != 2 || p.KW != 2 || p.stride != 1 || p.pt != 0 || src_w <= 0 || p.Win != src_w || p.Wout != src_w || p.Hout != p.Hin)
        return refuse("conv_gemm_up2: the descriptor must be the 2x2 stride-1 convolution on the source grid (ups = 1, Hout = Hin, Wout = Win = src_w)");
    if (phase < -1 || phase > 3) return refuse("conv_gemm_up2: phase must be 2 py + px (0..3), or -1 for the four phases in the batch index");
    if (phase >= 0 ? (p.batch != 1 || p.ph != 1 - (phase >> 1) || p.pw != 1 - (phase & 1)) : (p.batch != 4 || p.a_bs != 0 || p.o_bs != 0))
        return refuse("conv_gemm_up2: a phase launch has batch 1, ph = 1 - py, pw = 1 - px; the batch form has batch 4 with a_bs = o_bs = 0");
    if (p.split_k > 1) return refuse("conv_gemm_up2: no split-K (the reduce kernel writes unmapped rows)");
    if (p.act != 0 || p.R || p.rowbias || p.bias_per_row || p.out_nchw || p.o_split || p.out_dtype != GEO4D_F32 || (p.N & 3) || (p.ldo & 3) || !aligned(p.O, 16))
        return refuse("conv_gemm_up2: the mapped epilogue writes plain f32 rows with a column bias only (N % 4 == 0, 16-byte aligned rows)");
    // a wave tile's (at most 128) rows land within 4 (128 + W) + 2 W rows of the output: their byte offsets must stay inside the buffer window
    if ((4L * (128 + src_w) + 2L * src_w) * p.ldo * 4 >= (1L << 31)) return refuse("conv_gemm_up2: a wave tile's output rows span more than the 2 GB buffer window");
    geo4d_conv_gemm_t q = p;      // the phases of the batch form share everything a plan depends on
    q.batch = 1;
    q.gn_colsum = nullptr;
    q.split_k = 1;
    pl = resolve(q);
    if (pl.error) return pl;
    if (pl.hint != 22 && pl.hint != 23 && pl.hint != 25 && pl.hint != 71 && pl.hint != 72)
        return refuse("conv_gemm_up2: the mapped epilogue lives on tile hints 22, 23, 25, 71 and 72");
    if ((p.Hin * p.Win) % (pl.colsum_rows ? pl.colsum_rows : 1)) pl.colsum_rows = 0;      // an entry's rows must not straddle frames
    if (p.gn_colsum && (!pl.colsum_rows || !aligned(p.gn_colsum, 16)))
        return refuse("conv_gemm_up2: this launch cannot emit gn_colsum: it needs a frame's source rows and M to be multiples of the wave tile's rows");
    pl.up_w = src_w;
    pl.up_phase = phase;
    return pl;
}

}  // namespace geo4d_gemm
