// geo4d_amd/csrc/gemm_epilogue.h — the epilogue pieces every conv_gemm generation shares (device code only; included by gemm_kernel.h):
//   * EpiDest: where a launch stores - the output tensor, or the raw fp32 slab of split kz when the epilogue runs in the reduce kernel;
//   * the value math: epi_value (alpha, per-row bias, column bias, row-bias table, SiLU / GELU) and geglu_value, in ONE floating-point
//     order that every call site had before it was factored out (sites that differ by even a `+ 0.f` keep their own line);
//   * store policies (element size + pack + store of one lane's 4 consecutive columns) and the register epilogue's fast paths written
//     once over them: geglu_fast, plain_fast16; the wide f32 plain path (the one that carries gn_colsum and the row biases) is its own.
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
};
struct StoreF16Sat {               // plain f16 rows clamped to the finite range, NaN kept (common.h pack4_f16_sat); p.sat_count (debug) counts the clamped lanes
    static constexpr unsigned ES = 2;
    static __device__ __forceinline__ u32x2 pack(const geo4d_conv_gemm_t& p, const float (&e)[4]) {
        count_f16_saturation(p.sat_count, e);
        return pack4_f16_sat(e);
    }
    static __device__ __forceinline__ void store(const u32x2 v, const __amdgpu_buffer_rsrc_t rs, const unsigned off) { __builtin_amdgcn_raw_buffer_store_b64(v, rs, off, 0, 0); }
};

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
template <int MB, int NB, bool RES, typename Store>
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
    for (int b = 0; b < NB; ++b) {
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

}  // namespace geo4d_gemm
