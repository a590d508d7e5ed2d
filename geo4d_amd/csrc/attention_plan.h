// geo4d_amd/csrc/attention_plan.h — the host-side planner of geo4d_attention: validate() holds the descriptor checks and ONE function,
// resolve(), turns a (validated) descriptor into the kernel instantiation and grid that run it. geo4d_attention launches what the plan
// says, geo4d_attention_plan answers from the same plan, so the two cannot disagree. Host code only: no HIP call, no allocation, no
// device code. Include after common.h (dtype and return codes).
#pragma once
#include <cstdint>
#include "geo4d_hip.h"

namespace geo4d_attn {

// What runs: `kernel` 1 = flash_attn_kernel<T, nseg, qb, occ, ps>, 2 = flash_attn2_kernel<T, ps, occ> (always nseg 1, qb 2), on
// grid {ceil(Nq / rows_per_wg), H, B} x 256 threads; or why nothing runs (`error` and its return code `rc`).
struct AttnPlan : geo4d_attention_plan_t {
    int rc = GEO4D_OK;
    const char* error = nullptr;
};

inline AttnPlan refuse(int rc, const char* why) {
    AttnPlan pl{};
    pl.rc = rc;
    pl.error = why;
    return pl;
}

inline bool is16(int dtype) { return dtype == GEO4D_BF16 || dtype == GEO4D_F16; }
inline bool aligned(const void* ptr, int bytes) { return ((uintptr_t)ptr % bytes) == 0; }

// The descriptor checks of geo4d_attention, in the order they have always been made (callers match on the messages).
inline AttnPlan validate(const geo4d_attention_t& p) {
    const int esz = is16(p.dtype) ? 2 : 4, epc = 16 / esz;
    if (p.dtype < 0 || p.dtype > 3 || p.B <= 0 || p.H <= 0 || p.Nq <= 0 || p.nseg < 1 || p.nseg > 2) return refuse(GEO4D_EINVAL, "attention: bad arguments");
    if (p.head_dim != 64) return refuse(GEO4D_ENOTSUP, "attention: only d_head = 64 is built (yaml num_head_channels: 64)");
    if ((p.ldq * esz) % 16 || (p.ldo * esz) % 16 || !aligned(p.q, 16) || !aligned(p.o, 16)) return refuse(GEO4D_EINVAL, "attention: q/o alignment");
    for (int s = 0; s < p.nseg; ++s) {
        if (p.Nk[s] <= 0 || p.kv_div[s] <= 0 || !p.k[s] || !p.vt[s] || (p.ldk[s] * esz) % 16 || (p.ldvt[s] * esz) % 16 || (p.vt_bs[s] * esz) % 16 ||
            !aligned(p.k[s], 16) || !aligned(p.vt[s], 16) || p.ldvt[s] * epc < 0 || ((p.Nk[s] + epc - 1) / epc) * epc > p.ldvt[s])
            return refuse(GEO4D_EINVAL, "attention: bad key/value segment");
    }
    if (!p.zeros || !aligned(p.zeros, 16)) return refuse(GEO4D_EINVAL, "attention: `zeros` must point at 16 zero bytes");
    if (p.H > 65535 || p.B > 65535) return refuse(GEO4D_EINVAL, "attention: grid too large");
    if (p.split_out && esz != 4) return refuse(GEO4D_EINVAL, "attention: split_out is the producer format of the 4-byte storage modes (f32 / bf16x3)");
    if (p.qkv_split && (p.dtype != GEO4D_BF16X3 || p.nseg != 1 || (p.Nk[0] % 8) || (p.ldq % 8) || (p.ldk[0] % 8) || (p.ldvt[0] % 8) || (p.vt_bs[0] % 8) ||
                        !aligned(p.q, 32) || !aligned(p.k[0], 32) || !aligned(p.vt[0], 32)))
        return refuse(GEO4D_EINVAL, "attention: qkv_split needs dtype bf16x3, one key/value set, Nk % 8 == 0, leading dimensions % 8 == 0 and 32-byte aligned bases");
    return AttnPlan{};
}

// flash_attn2_kernel stages K / V^T through 2 GB buffer windows with 32-bit offsets: one (batch, head)'s keys and V^T rows must fit
// one - they do by orders of magnitude at every size of BASELINE.json; otherwise the pointer-staged flash_attn_kernel serves the call.
inline bool window_ok(const geo4d_attention_t& p) {
    const long esz = is16(p.dtype) ? 2 : 4;
    return p.nseg == 1 && ((long)(p.Nk[0] + 64) * p.ldk[0] + 64) * esz < (1L << 31) && (64L * p.ldvt[0] + p.Nk[0] + 64) * esz < (1L << 31);
}

// The launch of the (validated) descriptor `p`, or why it cannot run. p.variant: 0 = host default; A/B builds of the same math:
// 1 = flash_attn_kernel, 128 rows / workgroup at 3 waves per SIMD (round-1 kernel), 2 = the same at 4 waves per SIMD (128-VGPR budget),
// 3 = 256 rows / workgroup, two query blocks per wave (self-attention only); 4 / 5 = flash_attn2_kernel (round 4: skewed query blocks,
// matrix work beside every softmax): one key/value set, 16-bit types (4) and bf16x3 on pre-split inputs (4 = one wave per SIMD with the
// whole register file, 5 = two waves per SIMD).
inline AttnPlan resolve(const geo4d_attention_t& p) {
    if (p.variant < 0 || p.variant > 5) return refuse(GEO4D_EINVAL, "attention: unknown variant");
    const bool b16 = is16(p.dtype), x3 = p.dtype == GEO4D_BF16X3, x3ps = x3 && p.qkv_split, win = window_ok(p);
    AttnPlan pl{};
    // flash_attn2_kernel is the default since round 4 wherever it applies and a 256-row workgroup is not mostly empty (measured,
    // profiles/r04_attention.md: bf16 N = 2560 199.9 -> 189.9 us, N = 640 33.6 -> 31.4; pre-split bf16x3 N = 2560 524 -> 443 us,
    // N = 640 76.3 -> 67.8). bf16x3: the two-waves-per-SIMD build wins on the long level-0 sequences once the workgroups of a
    // (frame, head) share an XCD: N = 2560 467 us (variant 4) vs 443 us (variant 5); N = 640 67.8 vs 70.3 us.
    const bool second_default = p.variant == 0 && p.nseg == 1 && p.Nq >= 256 && win && (b16 || x3ps);
    const int asked = !second_default ? p.variant : (x3 && p.Nq >= 1024) ? 5 : 4;
    if (asked >= 4) {
        if (p.nseg != 1 || !((b16 && asked == 4) || x3ps))
            return refuse(GEO4D_EINVAL, "attention: variants 4 / 5 take one key/value set in bf16 / f16 (4) or pre-split bf16x3");
        if (!win) return refuse(GEO4D_EINVAL, "attention: variants 4 / 5 need one (batch, head)'s keys and V^T rows inside a 2 GB window");
        pl.kernel = 2;
        pl.variant = asked;
        pl.nseg = 1;
        pl.qb = 2;
        pl.occ = (b16 || asked == 5) ? 2 : 1;
        pl.ps = x3;
    } else {
        // default (measured, profiles/r02_attention_variants.md): two query blocks per wave for 16-bit self-attention (bf16 N = 2560:
        // 245 -> 199 us), one for the 4-byte storage modes (their two-block build spills: bf16x3 523 -> 563 us). Dual-KV cross
        // attention has one query block per wave only; the 4-waves-per-SIMD build needs <= 128 VGPRs, which 4-byte storage exceeds.
        const int v = asked == 0 ? (p.nseg == 1 && b16 ? 3 : 1) : (asked == 3 && p.nseg == 2) ? 1 : (asked == 2 && !b16) ? 1 : asked;
        pl.kernel = 1;
        pl.variant = v;
        pl.nseg = p.nseg;
        pl.qb = v == 3 ? 2 : 1;
        pl.occ = p.nseg == 2 ? 1 : v == 3 ? 2 : (b16 && v == 2) ? 4 : 1;
        pl.ps = x3ps;
    }
    pl.rows_per_wg = 128 * pl.qb;
    pl.grid[0] = (p.Nq + pl.rows_per_wg - 1) / pl.rows_per_wg;
    pl.grid[1] = p.H;
    pl.grid[2] = p.B;
    return pl;
}

}  // namespace geo4d_attn
