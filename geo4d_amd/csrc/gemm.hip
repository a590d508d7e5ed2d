// geo4d_amd/csrc/gemm.hip — the workhorse: implicit-GEMM convolution / linear / batched GEMM on MFMA.
//
// One kernel covers every dense contraction of the Geo4D hot path:
//   nn.Linear                         (1 tap, Hin=Win=Hout=Wout=1, F = M rows)
//   nn.Conv2d 3x3 / 1x1, stride 1|2   (openaimodel3d.py:154,179 ResBlock; :51-78 Downsample)
//   nearest-2x upsample + Conv2d 3x3  (openaimodel3d.py:80-106, ae_modules.py:111-127) — the upsample is
//                                      folded into the gather (src = dst >> 1), nothing is materialised
//   nn.Conv3d (3,1,1), pad (1,0,0)    (openaimodel3d.py:257-266 TemporalConvBlock) — 3 temporal taps
//   batched Q.K^T / P.V GEMMs         (ae_modules.py:53-78 VAE AttnBlock, d = 512)
// Element types: bf16 / f16 (one MFMA 32x32x16 per 16 k), f32 (exact, v_mfma_f32_32x32x2_f32) and bf16x3 — f32 in memory,
// split into bf16 hi + lo in registers (weights pre-split at pack time) and multiplied with three bf16 MFMAs per 16 k: the
// precision of ~16-bit mantissas (point-map parity 1e-3 needs more than any single 16-bit pass gives, tests/precision_sim.py)
// at 3/16 of the f32-MFMA cost.
// Activations are channels-last tokens [F, H*W, C]; weights are packed [N][taps*Cin] (K-major, tap-major).
// out[m][n] = epilogue(alpha * sum_k A_gather[m][k] * W[n][k])
//
// Host side: gemm_plan.h validates the descriptor and resolves it - ONE tile table (every hint of the three kernel generations:
// gemm_kernel.h, gemm_kernel_v2.h, gemm_kernel_v3.h), validate() and ONE function, resolve(), that applies defaults, redirects, fall-backs,
// split-K, the operand-layout variant and the gn_colsum granularity - and the generation's translation unit launches the plan's tile.
// geo4d_conv_gemm_plan, geo4d_conv_gemm_tiles and geo4d_conv_gemm_colsum_rows answer from the same plan and table.
//
// Structure of the first-generation kernel (template in gemm_kernel.h; 4, 5, 8 or 10 waves, tile BM x BN x 128 B of K per stage; tiles
// 128x128, 128x64, 64x128, 64x64, 128x32, 256x128, 256x256, 160x320, 160x160 picked per problem by the host's measured table):
//   * gather table: the source pixel of every (tile row, tap) is resolved ONCE per workgroup into LDS
//     (-1 = zero padding), so the K loop does one ds_read + one 64-bit mad per 16-byte chunk instead of
//     re-deriving (frame, y, x), bounds and upsample/stride arithmetic every stage;
//   * global->LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction, no VGPR round trip and no
//     ds_write: the ds_write_b128 path tops out at ~79 B/clk/CU and was the limiter of the register-staged version),
//     2-deep LDS ring, one EXPLICIT `s_waitcnt vmcnt(0)` + barrier per stage (hipcc does not track LDS-DMA and drops the
//     wait inside loops). K is walked channel-slab major / tap minor so a conv's re-reads of its input hit the XCD's L2.
//     The DMA image is lane-linear (8 lanes = one 128-byte row),
//     so bank conflicts are removed by an XOR swizzle applied on the SOURCE address (slot = chunk ^ ((row>>1)&7))
//     and mirrored on the fragment ds_read_b128 (conflict-free for all four 16-lane service groups);
//     zero padding = lanes whose tap falls outside the image fetch from a 16-byte zero block;
//   * swapped MFMA operands: the weight fragment is the MFMA "A" side, the activation fragment the "B" side,
//     so a lane owns ONE output row m and 4 consecutive output columns n per register quad;
//   * epilogue through LDS (fp32): bias / row-bias / SiLU / GEGLU applied in registers, each wave transposes its tile through
//     a private 32 x 64 (or 32 x 32) block of the idle stage buffers, then residual add + rounding + coalesced 16-byte stores;
//   * optional split-K (gridDim.z) into fp32 partial slabs + a deterministic fixed-order reduce kernel
//     carrying the epilogue — for the 5x8 / 10x16 levels whose M x N tile count cannot fill 256 CUs;
//   * workgroup ids remapped so each XCD (private 4 MiB L2) walks a contiguous range of tiles with the
//     N-tile index fastest: neighbours share the gathered A panel.
#include "gemm_kernel.h"

namespace geo4d_gemm {
// one translation unit per generation and element type (parallel build): gemm_*.hip, gemm_v2_*.hip, gemm_v3_*.hip
extern template int launch_typed<float>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_typed<bf16_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_typed<f16_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_typed<bf16x3_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_v2_typed<bf16_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_v2_typed<bf16x3_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_v2_typed<f16x2p_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_v3_typed<bf16_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_v3_typed<bf16x3_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_v3_typed<f16x2p_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_v2_up2<bf16x3_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
extern template int launch_v3_up2<bf16x3_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);

// the second / third generation's launcher of the plan's tile (resolve() refuses those hints for the other element types)
template <typename T>
static int launch_v23(const geo4d_conv_gemm_t& p, const Plan& plan, hipStream_t s) {
    return generation(plan.hint) == 2 ? launch_v2_typed<T>(p, plan, s) : launch_v3_typed<T>(p, plan, s);
}
}  // namespace geo4d_gemm
using namespace geo4d_gemm;

static_assert(MAX_TAPS == MAXTAP, "gemm_plan.h validates the tap count the kernels' gather tables hold");

// validate + resolve: the one path to a plan, for the query and for the launch
static int conv_gemm_plan(const geo4d_conv_gemm_t* p, Plan& plan) {
    if (!p) return GEO4D_EINVAL;
    const char* error = validate(*p);
    if (!error) {
        plan = resolve(*p);
        error = plan.error;
    }
    if (error) geo4d_set_error(error);
    return error ? GEO4D_EINVAL : GEO4D_OK;
}

extern "C" int geo4d_conv_gemm(const geo4d_conv_gemm_t* pp, void* stream) {
    Plan plan;
    const int rc = conv_gemm_plan(pp, plan);
    if (rc != GEO4D_OK) return rc;
    const geo4d_conv_gemm_t& p = *pp;
    hipStream_t s = (hipStream_t)stream;
    const bool gen1 = generation(plan.hint) == 1;
    switch (p.dtype) {
        case GEO4D_F32: return launch_typed<float>(p, plan, s);
        case GEO4D_BF16: return gen1 ? launch_typed<bf16_t>(p, plan, s) : launch_v23<bf16_t>(p, plan, s);
        case GEO4D_BF16X3: return gen1 ? launch_typed<bf16x3_t>(p, plan, s) : launch_v23<bf16x3_t>(p, plan, s);
        case GEO4D_F16X2: return launch_v23<f16x2p_t>(p, plan, s);
        default: return launch_typed<f16_t>(p, plan, s);
    }
}

extern "C" int geo4d_conv_gemm_plan(const geo4d_conv_gemm_t* pp, geo4d_conv_gemm_plan_t* out) {
    Plan plan;
    if (!out) return GEO4D_EINVAL;
    const int rc = conv_gemm_plan(pp, plan);
    if (rc != GEO4D_OK) return rc;
    const Tile& t = *find_tile(plan.hint);
    *out = {t.hint, generation(t.hint), t.bm, t.bn, t.wm, t.wn, plan.splits, plan.hot, plan.osplit, plan.colsum_rows};
    return GEO4D_OK;
}

// the same path for the sub-pixel Upsample launch: the descriptor checks, then resolve_up2
static int conv_gemm_up2_plan(const geo4d_conv_gemm_t* p, int src_w, int phase, Plan& plan) {
    if (!p) return GEO4D_EINVAL;
    const char* error = validate(*p);
    if (!error) {
        plan = resolve_up2(*p, src_w, phase);
        error = plan.error;
    }
    if (error) geo4d_set_error(error);
    return error ? GEO4D_EINVAL : GEO4D_OK;
}

extern "C" int geo4d_conv_gemm_up2(const geo4d_conv_gemm_t* pp, int src_w, int phase, void* stream) {
    Plan plan;
    const int rc = conv_gemm_up2_plan(pp, src_w, phase, plan);
    if (rc != GEO4D_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    return generation(plan.hint) == 2 ? launch_v2_up2<bf16x3_t>(*pp, plan, s) : launch_v3_up2<bf16x3_t>(*pp, plan, s);
}

extern "C" int geo4d_conv_gemm_up2_plan(const geo4d_conv_gemm_t* pp, int src_w, int phase, geo4d_conv_gemm_plan_t* out) {
    Plan plan;
    if (!out) return GEO4D_EINVAL;
    const int rc = conv_gemm_up2_plan(pp, src_w, phase, plan);
    if (rc != GEO4D_OK) return rc;
    const Tile& t = *find_tile(plan.hint);
    *out = {t.hint, generation(t.hint), t.bm, t.bn, t.wm, t.wn, plan.splits, plan.hot, plan.osplit, plan.colsum_rows};
    return GEO4D_OK;
}

extern "C" int geo4d_conv_gemm_tiles(geo4d_conv_gemm_tile_t* out, int cap) {
    int n = 0;
    for (const Tile& t : TILES) {
        if (out && n < cap) out[n] = {t.hint, generation(t.hint), t.bm, t.bn, t.wm, t.wn, t.geglu()};
        ++n;
    }
    return n;
}

// The colsum_rows of the launch's own plan WITHOUT the descriptor checks (see geo4d_hip.h): 0 = this launch cannot emit the sums or
// resolve() refuses it (the caller then leaves gn_colsum null and the GroupNorm runs its own statistics pass).
extern "C" int geo4d_conv_gemm_colsum_rows(const geo4d_conv_gemm_t* pp) {
    if (!pp || pp->Hout <= 0 || pp->Wout <= 0) return 0;      // (the plan divides by a frame's rows)
    return resolve(*pp).colsum_rows;
}
