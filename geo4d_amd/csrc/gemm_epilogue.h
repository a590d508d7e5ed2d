// geo4d_amd/csrc/gemm_epilogue.h — the epilogue pieces every conv_gemm generation shares (device code only; included by gemm_kernel.h):
//   * EpiDest: where a launch stores - the output tensor, or the raw fp32 slab of split kz when the epilogue runs in the reduce kernel;
//   * the value math: epi_value (alpha, per-row bias, column bias, row-bias table, SiLU / GELU) and geglu_value, in ONE floating-point
//     order that every call site had before it was factored out (sites that differ by even a `+ 0.f` keep their own line);
//   * store policies (element size + pack + store of one lane's 4 consecutive columns) and the register epilogue's fast paths written
//     once over them: geglu_fast, plain_fast16 (8-byte stores of 16-bit rows) and their 16-byte forms geglu_wide16, plain_wide16; the wide
//     f32 plain path (the one that carries gn_colsum and the row biases) is its own.
#pragma once
#include "common.h"
#include "geo4d_hip.h"

namespace geo4d_gemm {

__device__ __forceinline__ void store_out(void* O, long idx, float v, int dt) {
    if (dt == GEO4D_F32) ((float*)O)[idx] = v;
    else if (dt == GEO4D_BF16) ((unsigned short*)O)[idx] = f32_to_bf16_bits(v);
    else ((unsigned short*)O)[idx] = f32_to_f16_bits(v);
}
__device__ __forceinline__ float load_res(const void* R, long idx, int dt) {
    if (dt == GEO4D_F32) return ((const float*)R)[idx];
    if (dt == GEO4D_BF16) return bf16_bits_to_f32(((const unsigned short*)R)[idx]);
    return f16_bits_to_f32(((const unsigned short*)R)[idx]);
}

// ---- destination ---------------------------------------------------------------------------------------------------------------------
// `partial` (split-K): the raw fp32 slab of split kz goes to the workspace and the epilogue runs in the reduce kernel
struct EpiDest { void* O; long ldo, obase; int odt, oesz, nout; bool geglu; };
__device__ __forceinline__ EpiDest epi_dest(const geo4d_conv_gemm_t& p, const bool partial, const int kz, const long bz) {
    const int odt = partial ? GEO4D_F32 : p.out_dtype;
    void* O = partial ? (void*)((float*)p.workspace + ((long)kz * p.batch + bz) * (long)p.M * p.N) : p.O;
    const bool geglu = !partial && p.act == 2;
    return EpiDest{O, partial ? (long)p.N : p.ldo, partial ? 0 : bz * p.o_bs, odt, odt == GEO4D_F32 ? 4 : 2, geglu ? (p.N >> 1) : p.N, geglu};
}

// ---- sub-pixel Upsample: strided output rows ---------------------------------------------------------------------------------------------
// A nearest-2x + 3x3 convolution is, per output parity (py, px), a 2x2 convolution on the source grid (geo4d_conv_gemm_up2). Row
// m = (f, y, x) of phase 2 py + px lands on token row (f, 2y + py, 2x + px) of the [F, 2H, 2W] grid; frames fold into m div W.
struct Up2Map {
    int w, phase;        // source width W; 2 py + px
    __device__ __forceinline__ long row(const int m) const {
        const int q = m / w;
        return 4L * w * q + 2 * (m - q * w) + (phase >> 1) * 2 * w + (phase & 1);
    }
};

// the kernel argument the sub-pixel Upsample instantiations take after `splits` and `tiles_mn` (the other instantiations take none)
struct Up2Args { int w, phase; };      // source width; 2 py + px, or -1: the batch index
__host__ __device__ __forceinline__ Up2Args up2_args() { return Up2Args{0, 0}; }
__host__ __device__ __forceinline__ Up2Args up2_args(const Up2Args& a) { return a; }

// ---- value ---------------------------------------------------------------------------------------------------------------------------
// out[m][n] before the residual: ((acc * alpha + brow) + bias[n]) + rowbias[rboff + n], then SiLU / GELU. `brow`: the per-row bias of row
// m (0.f without one), `rboff`: the row's offset into the row-bias table; `inb`: n < N (a lane past the last column adds no biases).
// GELU = false: the first generation's direct path, which the host never gives act == 3.
template <bool GELU = true>
__device__ __forceinline__ float epi_value(const geo4d_conv_gemm_t& p, const float acc, const float brow, const long rboff, const int n, const bool inb = true) {
    float v = acc * p.alpha + brow;
    if (inb) {
        if (p.bias && !p.bias_per_row) v += p.bias[n];
        if (p.rowbias) v += p.rowbias[rboff + n];
    }
    if (p.act == 1) v = silu_f(v);
    else if (GELU && p.act == 3) v = gelu_erf_f(v);
    return v;
}
// GEGLU: value x gelu(gate); the gate's accumulator and bias sit 32 columns after the value's (pack.pack_geglu)
__device__ __forceinline__ float geglu_value(const float alpha, const float xacc, const float gacc, const float xbias, const float gbias) {
    const float xv = xacc * alpha + xbias;
    const float gv = gacc * alpha + gbias;
    return xv * gelu_erf_f(gv);
}

// ---- 4 consecutive 16-bit elements <-> f32 ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u32x2 pack4_16(const float (&e)[4], const bool isbf) {
    return isbf ? u32x2{f32x2_to_bf16x2(e[0], e[1]), f32x2_to_bf16x2(e[2], e[3])} : u32x2{f32x2_to_f16x2(e[0], e[1]), f32x2_to_f16x2(e[2], e[3])};
}
__device__ __forceinline__ void unpack4_16(const u32x2 r, const bool isbf, float (&f)[4]) {
    if (isbf) {
        f[0] = __uint_as_float(r[0] << 16); f[1] = __uint_as_float(r[0] & 0xffff0000u);
        f[2] = __uint_as_float(r[1] << 16); f[3] = __uint_as_float(r[1] & 0xffff0000u);
    } else {
        f[0] = f16_bits_to_f32((unsigned short)(r[0] & 0xffffu)); f[1] = f16_bits_to_f32((unsigned short)(r[0] >> 16));
        f[2] = f16_bits_to_f32((unsigned short)(r[1] & 0xffffu)); f[3] = f16_bits_to_f32((unsigned short)(r[1] >> 16));
    }
}

// ---- buffer resources of the register epilogue's fast paths ----------------------------------------------------------------------------
// Every access goes through a raw buffer resource whose base is this wave's tile corner (wave-uniform, SGPRs): a lane outside M x N
// offers an offset beyond the 2 GB window (stores dropped, loads return 0 - no exec-masked branches, so hipcc's waits stay COUNTED), an
// absent bias / residual is a resource with zero records (its loads return 0 without touching memory).
constexpr unsigned EPI_OOB = 0x80000000u;
// debug_ablate bit 6 (A/B runs and the bit tests, ops.EPI_WIDE = 0): 16-bit rows keep the 8-byte epilogue (geglu_fast / plain_fast16);
// the low six bits keep their meanings (2 = three persistent workgroups, 16 + g = tile order)
constexpr int EPI_ABLATE_NARROW = 64, EPI_ABLATE_LOW = 63;
__device__ __forceinline__ bool epi_wide_on(const geo4d_conv_gemm_t& p) { return (p.debug_ablate & EPI_ABLATE_NARROW) == 0; }
constexpr int EPI_RSRC_FLAGS = 0x00020000;
__device__ __forceinline__ void* uniform_ptr(const void* q) {
    const unsigned long long v = (unsigned long long)q;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (void*)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* corner, const bool present = true) {
    return __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(corner), 0, present ? EPI_OOB : 0u, EPI_RSRC_FLAGS);
}
// the column bias from column n_w0 on (`has`: the launch has one): records end at N
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bias_rsrc(const geo4d_conv_gemm_t& p, const bool has, const int n_w0) {
    const int nleft = p.N - n_w0;
    return __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(has ? (const void*)(p.bias + n_w0) : p.zeros), 0, (has && nleft > 0) ? (unsigned)nleft * 4u : 0u, EPI_RSRC_FLAGS);
}

// ---- store policies: one lane's 4 consecutive output columns -----------------------------------------------------------------------------
// ES = bytes per stored element; pack(p, e) = the lane's vector; store(v, rsrc, byte offset). All static. (Rows16 keeps
// bf16 / f16 a run-time test, as the code always had: one loop in the binary instead of two.)
struct StoreF32 {                  // f32 rows: this lane's 16-byte chunk `lq` of a block's 64 output bytes
    static constexpr unsigned ES = 4;
    static __device__ __forceinline__ u32x4 pack(const geo4d_conv_gemm_t&, const float (&e)[4]) {
        return u32x4{__float_as_uint(e[0]), __float_as_uint(e[1]), __float_as_uint(e[2]), __float_as_uint(e[3])};
    }
    static __device__ __forceinline__ void store(const u32x4 v, const __amdgpu_buffer_rsrc_t rs, const unsigned off) { __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 0); }
};
struct StoreSplit {                // the producers' pre-split format: whole 16-byte bf16 hi | lo chunks
    static constexpr unsigned ES = 4;
    static __device__ __forceinline__ u32x4 pack(const geo4d_conv_gemm_t&, const float (&e)[4]) {
        unsigned int h0, h1, l0, l1;
        h0 = f32x2_to_bf16x2(e[0], e[1]); h1 = f32x2_to_bf16x2(e[2], e[3]);
        l0 = f32x2_to_bf16x2(e[0] - __uint_as_float(h0 << 16), e[1] - __uint_as_float(h0 & 0xffff0000u));
        l1 = f32x2_to_bf16x2(e[2] - __uint_as_float(h1 << 16), e[3] - __uint_as_float(h1 & 0xffff0000u));
        // rows of 16 lanes = lq: odd rows of (h) <-> even rows of (l): even lq ends with [h own | h of lq + 1] = the group's hi chunk,
        // odd lq with [l of lq - 1 | l own] = its lo chunk (every lane of the wave takes part: no divergence before this point)
        const u32x2 s0 = __builtin_amdgcn_permlane16_swap(h0, l0, false, false);
        const u32x2 s1 = __builtin_amdgcn_permlane16_swap(h1, l1, false, false);
        return u32x4{s0[0], s1[0], s0[1], s1[1]};
    }
    static __device__ __forceinline__ void store(const u32x4 v, const __amdgpu_buffer_rsrc_t rs, const unsigned off) { __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 0); }
};
struct StoreRows16 {               // bf16 / f16 rows of an un-split launch (a split one stores f32 slabs): the format is the launch's out_dtype
    static constexpr unsigned ES = 2;
    static __device__ __forceinline__ bool isbf(const geo4d_conv_gemm_t& p) { return p.out_dtype == GEO4D_BF16; }
    static __device__ __forceinline__ u32x2 pack(const geo4d_conv_gemm_t& p, const float (&e)[4]) { return pack4_16(e, isbf(p)); }
    static __device__ __forceinline__ void store(const u32x2 v, const __amdgpu_buffer_rsrc_t rs, const unsigned off) { __builtin_amdgcn_raw_buffer_store_b64(v, rs, off, 0, 0); }
    // the 16-byte forms' halves (nothing to count)
    static __device__ __forceinline__ bool counts(const geo4d_conv_gemm_t&) { return false; }
    static __device__ __forceinline__ void count(const geo4d_conv_gemm_t&, const float (&)[4]) {}
    static __device__ __forceinline__ u32x2 pack_half(const geo4d_conv_gemm_t& p, const float (&e)[4]) { return pack4_16(e, isbf(p)); }
};
struct StoreF16Sat {               // plain f16 rows clamped to the finite range, NaN kept (common.h pack4_f16_sat); p.sat_count (debug) counts the clamped lanes
    static constexpr unsigned ES = 2;
    static __device__ __forceinline__ u32x2 pack(const geo4d_conv_gemm_t& p, const float (&e)[4]) {
        count_f16_saturation(p.sat_count, e);
        return pack4_f16_sat(e);
    }
    static __device__ __forceinline__ void store(const u32x2 v, const __amdgpu_buffer_rsrc_t rs, const unsigned off) { __builtin_amdgcn_raw_buffer_store_b64(v, rs, off, 0, 0); }
    // the 16-byte forms' halves: the counter's test is made once per wave tile (counts), not per store, and the clamp works on the
    // packed pair (common.h f32x2_to_f16x2_sat: the same bits)
    static __device__ __forceinline__ bool counts(const geo4d_conv_gemm_t& p) { return p.sat_count != nullptr; }
    static __device__ __forceinline__ void count(const geo4d_conv_gemm_t& p, const float (&e)[4]) { count_f16_saturation(p.sat_count, e); }
    static __device__ __forceinline__ u32x2 pack_half(const geo4d_conv_gemm_t&, const float (&e)[4]) {
        return u32x2{f32x2_to_f16x2_sat(e[0], e[1]), f32x2_to_f16x2_sat(e[2], e[3])};
    }
};

// ---- 16-byte stores of 16-bit rows: two horizontally adjacent 16-column blocks b, b + 1 ---------------------------------------------------
// A lane holds 8 bytes of each block (its columns 4 lq .. 4 lq + 3). v_permlane16_swap trades the odd 16-lane rows of the first operand for
// the even rows of the second (as StoreSplit::pack does for hi | lo): an even lq ends with [own x | x of lq + 1] = columns 4 lq .. 4 lq + 7
// of block b, an odd lq with [y of lq - 1 | own y] = columns 4 (lq - 1) .. 4 lq + 3 of block b + 1 - 12 columns after its own 4 lq of
// block b (pair_shift16). One 16-byte store where two 8-byte ones stood, a row's run 64 contiguous bytes; every lane of the wave takes part.
// The exchange is its own inverse: unpair_rows16 turns a 16-byte load at the same offset into the two blocks' halves (the residual).
__device__ __forceinline__ unsigned pair_shift16(const int lq) { return (lq & 1) ? 24u : 0u; }      // bytes
__device__ __forceinline__ u32x4 pair_rows16(const u32x2 x, const u32x2 y) {
    const u32x2 s0 = __builtin_amdgcn_permlane16_swap(x[0], y[0], false, false);
    const u32x2 s1 = __builtin_amdgcn_permlane16_swap(x[1], y[1], false, false);
    return u32x4{s0[0], s1[0], s0[1], s1[1]};
}
__device__ __forceinline__ void unpair_rows16(const u32x4 r, u32x2& x, u32x2& y) {
    const u32x2 s0 = __builtin_amdgcn_permlane16_swap(r[0], r[2], false, false);
    const u32x2 s1 = __builtin_amdgcn_permlane16_swap(r[1], r[3], false, false);
    x = u32x2{s0[0], s1[0]};
    y = u32x2{s0[1], s1[1]};
}
// whether a wave tile takes the 16-byte forms: the switch, and every one of its NB blocks whole inside N (wave-uniform, in SGPRs: a
// scalar branch around the whole epilogue, no exec masks; a wave tile cut by N keeps the 8-byte code, which folds the cut into its offsets)
template <int NB>
__device__ __forceinline__ bool wide16_tile(const geo4d_conv_gemm_t& p, const int n_w0) {
    return NB >= 2 && epi_wide_on(p) && __builtin_amdgcn_readfirstlane(n_w0) + 16 * NB <= p.N;
}

// ---- fast paths of the register epilogue: acc[a][b][j] is out[m_w0 + 16a + lr][n_w0 + 16b + 4lq + j] --------------------------------------
// `corner`: the element of the output at the wave tile's corner (row m_w0, first stored column), `ldo`: the row pitch in elements.
// GEGLU: the bias (value | gate columns) once per block, outside the row loop; only stores inside. Packed GEGLU weights interleave value /
// gate in 32-column blocks: 16-blocks 4j, 4j + 1 = value, 4j + 2, 4j + 3 = gate.
template <int MB, int NB, typename Store>
__device__ __forceinline__ void geglu_fast(const geo4d_conv_gemm_t& p, const f32x4 (&acc)[MB][NB], const void* corner, const long ldo,
                                           const int m_w0, const int n_w0, const int lr, const int lq) {
    if constexpr (NB % 4 == 0) {
        const __amdgpu_buffer_rsrc_t rsO = tile_rsrc(corner);
        const __amdgpu_buffer_rsrc_t rsB = bias_rsrc(p, p.bias != nullptr, n_w0);
        const unsigned offO = (unsigned)(lr * (int)ldo + 4 * lq) * Store::ES, rowO = (unsigned)ldo * (16u * Store::ES);      // bytes per 16-row block
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if ((b & 3) >= 2) continue;
            // whole 64-column value | gate groups only (N % 64 == 0): wave-uniform, folded into the store offset
            const bool grp = n_w0 + 16 * (b & ~3) + 64 <= p.N;
            const u32x4 bv = __builtin_amdgcn_raw_buffer_load_b128(rsB, (unsigned)(4 * lq) * 4u + 64u * b, 0, 0);
            const u32x4 bg = __builtin_amdgcn_raw_buffer_load_b128(rsB, (unsigned)(4 * lq) * 4u + 64u * b + 128u, 0, 0);
#pragma unroll
            for (int a = 0; a < MB; ++a) {
                const bool ok = grp && m_w0 + a * 16 + lr < p.M;
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    e[j] = geglu_value(p.alpha, acc[a][b][j], acc[a][b + 2 < NB ? b + 2 : b][j], __uint_as_float(bv[j]), __uint_as_float(bg[j]));
                Store::store(Store::pack(p, e), rsO, (ok ? offO + a * rowO : EPI_OOB) + (unsigned)(32 * (b >> 2) + 16 * (b & 1)) * Store::ES);
            }
        }
    }
}

// 16-bit rows, alpha + column bias (+ residual: RES, read through `rcorner` / `ldr` a row block AHEAD of the stores so that its wait
// stays counted): 8-byte vectors
// (B0: the first block - the 16-byte form leaves the last block of an odd NB to this code)
template <int MB, int NB, bool RES, typename Store, int B0 = 0>
__device__ __forceinline__ void plain_fast16(const geo4d_conv_gemm_t& p, const f32x4 (&acc)[MB][NB], const void* corner, const long ldo,
                                             const void* rcorner, const bool has_res, const int m_w0, const int n_w0, const int lr, const int lq) {
    const __amdgpu_buffer_rsrc_t rsO = tile_rsrc(corner);
    const __amdgpu_buffer_rsrc_t rsB = bias_rsrc(p, p.bias != nullptr, n_w0);
    const unsigned offO = (unsigned)(lr * (int)ldo + 4 * lq) * 2u, rowO = (unsigned)ldo * 32u;       // bytes per 16-row block
    __amdgpu_buffer_rsrc_t rsR = rsO;
    unsigned offR = 0, rowR = 0;
    if constexpr (RES) {
        rsR = tile_rsrc(has_res ? rcorner : p.zeros, has_res);
        offR = (unsigned)(lr * (int)p.ldr + 4 * lq) * 2u;
        rowR = (unsigned)p.ldr * 32u;
    }
#pragma unroll
    for (int b = B0; b < NB; ++b) {
        const bool colok = n_w0 + 16 * b + 4 * lq < p.N;
        const u32x4 bcu = __builtin_amdgcn_raw_buffer_load_b128(rsB, (unsigned)(4 * lq) * 4u + 64u * b, 0, 0);
        u32x2 ru = {0u, 0u};
        if constexpr (RES) ru = __builtin_amdgcn_raw_buffer_load_b64(rsR, ((colok && m_w0 + lr < p.M) ? offR : EPI_OOB) + 32u * b, 0, 0);
#pragma unroll
        for (int a = 0; a < MB; ++a) {
            const bool ok = colok && m_w0 + a * 16 + lr < p.M;
            float e[4], rf[4];
            if constexpr (RES) unpack4_16(ru, Store::isbf(p), rf);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                e[j] = acc[a][b][j] * p.alpha + __uint_as_float(bcu[j]);
                if constexpr (RES) e[j] += rf[j];
            }
            const u32x2 c = Store::pack(p, e);
            if constexpr (RES) {
                if (a + 1 < MB)
                    ru = __builtin_amdgcn_raw_buffer_load_b64(rsR, ((colok && m_w0 + (a + 1) * 16 + lr < p.M) ? offR : EPI_OOB) + 32u * b, (a + 1) * rowR, 0);
            }
            Store::store(c, rsO, (ok ? offO + a * rowO : EPI_OOB) + 32u * b);
        }
    }
}

// ---- the 16-byte forms (wide16_tile: every block of the wave tile inside N, so only rows are cut). The same IEEE operations in the same
// order as the 8-byte forms and the same bytes stored; COUNT: p.sat_count is set (debug) - tested once, by the callers below.
template <int MB, int NB, typename Store, bool COUNT>
__device__ __forceinline__ void geglu_wide16_rows(const geo4d_conv_gemm_t& p, const f32x4 (&acc)[MB][NB], const void* corner, const long ldo,
                                                  const int m_w0, const int n_w0, const int lr, const int lq) {
    if constexpr (NB % 4 == 0) {
        const __amdgpu_buffer_rsrc_t rsO = tile_rsrc(corner);
        const __amdgpu_buffer_rsrc_t rsB = bias_rsrc(p, p.bias != nullptr, n_w0);
        const unsigned offO = (unsigned)(lr * (int)ldo + 4 * lq) * 2u + pair_shift16(lq), rowO = (unsigned)ldo * 32u;      // bytes per 16-row block
#pragma unroll
        for (int b = 0; b < NB; b += 4) {                  // value blocks b, b + 1 (adjacent in the output), gate blocks b + 2, b + 3
            u32x4 bu[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bu[i] = __builtin_amdgcn_raw_buffer_load_b128(rsB, (unsigned)(4 * lq) * 4u + 64u * (b + i), 0, 0);
#pragma unroll
            for (int a = 0; a < MB; ++a) {
                const bool ok = m_w0 + a * 16 + lr < p.M;
                float e0[4], e1[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    e0[j] = geglu_value(p.alpha, acc[a][b][j], acc[a][b + 2][j], __uint_as_float(bu[0][j]), __uint_as_float(bu[2][j]));
                    e1[j] = geglu_value(p.alpha, acc[a][b + 1][j], acc[a][b + 3][j], __uint_as_float(bu[1][j]), __uint_as_float(bu[3][j]));
                }
                if constexpr (COUNT) { Store::count(p, e0); Store::count(p, e1); }
                const u32x4 c = pair_rows16(Store::pack_half(p, e0), Store::pack_half(p, e1));
                __builtin_amdgcn_raw_buffer_store_b128(c, rsO, (ok ? offO + a * rowO : EPI_OOB) + 16u * b, 0, 0);      // 32 output columns per group
            }
        }
    }
}
template <int MB, int NB, typename Store>
__device__ __forceinline__ void geglu_wide16(const geo4d_conv_gemm_t& p, const f32x4 (&acc)[MB][NB], const void* corner, const long ldo,
                                             const int m_w0, const int n_w0, const int lr, const int lq) {
    if (Store::counts(p)) geglu_wide16_rows<MB, NB, Store, true>(p, acc, corner, ldo, m_w0, n_w0, lr, lq);
    else geglu_wide16_rows<MB, NB, Store, false>(p, acc, corner, ldo, m_w0, n_w0, lr, lq);
}

// alpha + column bias (+ residual: one 16-byte load per block pair, at the stores' own offsets and a row block AHEAD of them)
template <int MB, int NB, bool RES, typename Store, bool COUNT>
__device__ __forceinline__ void plain_wide16_rows(const geo4d_conv_gemm_t& p, const f32x4 (&acc)[MB][NB], const void* corner, const long ldo,
                                                  const void* rcorner, const bool has_res, const int m_w0, const int n_w0, const int lr, const int lq) {
    const __amdgpu_buffer_rsrc_t rsO = tile_rsrc(corner);
    const __amdgpu_buffer_rsrc_t rsB = bias_rsrc(p, p.bias != nullptr, n_w0);
    const unsigned offO = (unsigned)(lr * (int)ldo + 4 * lq) * 2u + pair_shift16(lq), rowO = (unsigned)ldo * 32u;       // bytes per 16-row block
    __amdgpu_buffer_rsrc_t rsR = rsO;
    unsigned offR = 0, rowR = 0;
    if constexpr (RES) {
        rsR = tile_rsrc(has_res ? rcorner : p.zeros, has_res);
        offR = (unsigned)(lr * (int)p.ldr + 4 * lq) * 2u + pair_shift16(lq);
        rowR = (unsigned)p.ldr * 32u;
    }
#pragma unroll
    for (int b = 0; b + 1 < NB; b += 2) {
        const u32x4 bc0 = __builtin_amdgcn_raw_buffer_load_b128(rsB, (unsigned)(4 * lq) * 4u + 64u * b, 0, 0);
        const u32x4 bc1 = __builtin_amdgcn_raw_buffer_load_b128(rsB, (unsigned)(4 * lq) * 4u + 64u * (b + 1), 0, 0);
        u32x4 ru = {0u, 0u, 0u, 0u};
        if constexpr (RES) ru = __builtin_amdgcn_raw_buffer_load_b128(rsR, (m_w0 + lr < p.M ? offR : EPI_OOB) + 32u * b, 0, 0);
#pragma unroll
        for (int a = 0; a < MB; ++a) {
            const bool ok = m_w0 + a * 16 + lr < p.M;
            float e0[4], e1[4], rf0[4], rf1[4];
            if constexpr (RES) {
                u32x2 r0, r1;
                unpair_rows16(ru, r0, r1);
                unpack4_16(r0, Store::isbf(p), rf0);
                unpack4_16(r1, Store::isbf(p), rf1);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                e0[j] = acc[a][b][j] * p.alpha + __uint_as_float(bc0[j]);
                e1[j] = acc[a][b + 1][j] * p.alpha + __uint_as_float(bc1[j]);
                if constexpr (RES) { e0[j] += rf0[j]; e1[j] += rf1[j]; }
            }
            if constexpr (COUNT) { Store::count(p, e0); Store::count(p, e1); }
            const u32x4 c = pair_rows16(Store::pack_half(p, e0), Store::pack_half(p, e1));
            if constexpr (RES) {
                if (a + 1 < MB)
                    ru = __builtin_amdgcn_raw_buffer_load_b128(rsR, (m_w0 + (a + 1) * 16 + lr < p.M ? offR : EPI_OOB) + 32u * b, (a + 1) * rowR, 0);
            }
            __builtin_amdgcn_raw_buffer_store_b128(c, rsO, (ok ? offO + a * rowO : EPI_OOB) + 32u * b, 0, 0);
        }
    }
}
template <int MB, int NB, bool RES, typename Store>
__device__ __forceinline__ void plain_wide16(const geo4d_conv_gemm_t& p, const f32x4 (&acc)[MB][NB], const void* corner, const long ldo,
                                             const void* rcorner, const bool has_res, const int m_w0, const int n_w0, const int lr, const int lq) {
    if (Store::counts(p)) plain_wide16_rows<MB, NB, RES, Store, true>(p, acc, corner, ldo, rcorner, has_res, m_w0, n_w0, lr, lq);
    else plain_wide16_rows<MB, NB, RES, Store, false>(p, acc, corner, ldo, rcorner, has_res, m_w0, n_w0, lr, lq);
    if constexpr (NB & 1) plain_fast16<MB, NB, RES, Store, NB - 1>(p, acc, corner, ldo, rcorner, has_res, m_w0, n_w0, lr, lq);      // the odd last block
}

}  // namespace geo4d_gemm
