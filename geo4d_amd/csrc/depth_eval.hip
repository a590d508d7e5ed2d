// geo4d_amd/csrc/depth_eval.hip — video-depth evaluation against ground truth (dust3r/depth_eval.py depth_evaluation :147-355 as
// scripts/evaluation/infer_geo4d.py:514-545 calls it).
//
// The reference resizes the predicted depth to the ground-truth size (torchvision Resize, bicubic), selects the valid pixels of the
// flattened sequence by boolean indexing, fits (s, t) with a median start and 5000 Adam steps of torch ops, then computes seven metrics
// and an error map with a dozen more full-size torch ops. Here: one resize kernel; one order-preserving compaction (per-block counts,
// one scan, one scatter) whose dense output feeds the existing radix-select median and LAD fit of align.hip unchanged; one fused pass
// for the metrics (fp64 partial sums, fixed-order reduction) and the error map, reading (s, t) from the device so the fit and the
// metrics need no host round trip between them.
//
// Every arithmetic step below mirrors the reference's float32 torch op sequence (s * x then + t, (a - g)^2 then / g, ...): contraction
// into FMAs is switched off for this file so each product and sum rounds where torch's does.
#include <cmath>
#include "common.h"
#include "compact.h"
#include "geo4d_hip.h"

#pragma clang fp contract(off)

namespace {

// ---- bicubic resize = torch.nn.functional.interpolate(mode="bicubic", align_corners=False, antialias=False) on float input -------
// (aten/src/ATen/native/cpu/UpSampleKernel.cpp: source index scale * (i + 0.5) - 0.5 with scale = in / out in float, A = -0.75, taps
// clamped to the border, weighted sum over x inside the sum over y, no output clamp)
__device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
    const float A = -0.75f;
    auto cc1 = [&](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };
    auto cc2 = [&](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };
    c[0] = cc2(t + 1.f);
    c[1] = cc1(t);
    const float x2 = 1.f - t;
    c[2] = cc1(x2);
    c[3] = cc2(x2 + 1.f);
}

__device__ __forceinline__ void cubic_taps(int i, float scale, int in, int idx[4], float c[4]) {
    const float real = scale * ((float)i + 0.5f) - 0.5f;
    const int i0 = min((int)floorf(real), in - 1);
    const float t = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
    cubic_coeffs(t, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = max(min(i0 - 1 + k, in - 1), 0);
}

__global__ __launch_bounds__(256) void bicubic_resize_kernel(const float* __restrict__ x, float* __restrict__ y, int h, int w, int OH, int OW,
                                                             float sy, float sx) {
    const int f = blockIdx.y;
    const float* xf = x + (long)f * h * w;
    float* yf = y + (long)f * OH * OW;
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < (long)OH * OW; o += (long)gridDim.x * 256) {
        const int oy = (int)(o / OW), ox = (int)(o % OW);
        int iy[4], ix[4];
        float wy[4], wx[4];
        cubic_taps(oy, sy, h, iy, wy);
        cubic_taps(ox, sx, w, ix, wx);
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float* row = xf + (long)iy[a] * w;
            float r = row[ix[0]] * wx[0];
#pragma unroll
            for (int b = 1; b < 4; ++b) r += row[ix[b]] * wx[b];
            acc = a ? acc + r * wy[a] : r * wy[a];
        }
        yf[o] = acc;
    }
}

// ---- masked, order-preserving compaction -------------------------------------------------------------------------------------------
// valid(e) = gt > 0 && (max_depth infinite || gt < max_depth) && (!mask || mask[e]); tile = SEL_ROUNDS rounds of 256 consecutive
// elements per workgroup, so every load is a coalesced 256-element row and the in-tile rank of an element is a ballot popcount.
constexpr int SEL_ROUNDS = 16;
constexpr long SEL_TILE = 256L * SEL_ROUNDS;

__device__ __forceinline__ bool depth_valid(float g, float max_depth, bool bounded) { return g > 0.f && (!bounded || g < max_depth); }

__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) {     // torch.clamp(min) then torch.clamp(max); NaN stays NaN
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

__global__ __launch_bounds__(256) void select_count_kernel(const float* __restrict__ gt, const unsigned char* __restrict__ mask, long n,
                                                           float max_depth, int bounded, unsigned* __restrict__ block_count) {
    __shared__ unsigned red[4];
    const long base = (long)blockIdx.x * SEL_TILE;
    unsigned c = 0;
#pragma unroll 4
    for (int r = 0; r < SEL_ROUNDS; ++r) {
        const long e = base + r * 256 + threadIdx.x;
        if (e < n && depth_valid(gt[e], max_depth, bounded) && (!mask || mask[e])) ++c;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void select_scatter_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                             const unsigned char* __restrict__ mask, long n, float max_depth, int bounded,
                                                             float pre_min, float pre_max, const unsigned* __restrict__ block_offset,
                                                             float* __restrict__ pred_out, float* __restrict__ gt_out) {
    __shared__ unsigned wcount[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * SEL_TILE;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned off = block_offset[blockIdx.x];
    for (int r = 0; r < SEL_ROUNDS; ++r) {
        const long e = base + r * 256 + threadIdx.x;
        float g = 0.f;
        bool v = false;
        if (e < n) {
            g = gt[e];
            v = depth_valid(g, max_depth, bounded) && (!mask || mask[e]);
        }
        const unsigned long long bal = __ballot(v);
        if (lane == 0) wcount[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned pos = off + (unsigned)__popcll(bal & below);
        for (int k = 0; k < wave; ++k) pos += wcount[k];
        if (v) {
            pred_out[pos] = clamp_nan(pred[e], pre_min, pre_max);
            gt_out[pos] = g;
        }
        off += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
}

// ---- fused metrics + error map --------------------------------------------------------------------------------------------------
// sums: 0 sum |a-g|/g, 1 sum (a-g)^2/g, 2 sum (a-g)^2, 3 sum (log max(a,1e-5) - log g)^2, 4..6 #(delta < 1.25^k), 7 #metric pixels
constexpr int MET_SUMS = 8;
constexpr int MET_BLOCKS = 1024;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void depth_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt, long n, float max_depth,
                                                            int bounded, const unsigned char* __restrict__ custom_mask, const float* __restrict__ st,
                                                            float pre_min, float pre_max, float post_min, float post_max,
                                                            float* __restrict__ err_map, float* __restrict__ aligned, double* __restrict__ part) {
    __shared__ double red[4][MET_SUMS];
    const float s = st[0], t = st[1];
    double acc[MET_SUMS];
#pragma unroll
    for (int k = 0; k < MET_SUMS; ++k) acc[k] = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const float p = pred[e], g = gt[e];
        const bool valid = depth_valid(g, max_depth, bounded);
        const float full = s * p + t;                                  // un-clipped aligned prediction (:320-335)
        if (aligned) aligned[e] = full;
        err_map[e] = valid ? fabsf(full - g) / g : 0.f;
        if (valid && (!custom_mask || custom_mask[e])) {
            const float a = clamp_nan(s * clamp_nan(p, pre_min, pre_max) + t, post_min, post_max);
            const float d = a - g;
            acc[0] += (double)(fabsf(d) / g);
            acc[1] += (double)((d * d) / g);
            acc[2] += (double)(d * d);
            const float ac = a < 1e-5f ? 1e-5f : a;
            const float l = logf(ac) - logf(g);
            acc[3] += (double)(l * l);
            const float q1 = ac / g, q2 = g / ac;
            const float r = (q1 != q1 || q2 != q2) ? NAN : fmaxf(q1, q2);  // torch.maximum propagates NaN
            acc[4] += r < 1.25f ? 1.0 : 0.0;
            acc[5] += r < 1.5625f ? 1.0 : 0.0;
            acc[6] += r < 1.953125f ? 1.0 : 0.0;
            acc[7] += 1.0;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < MET_SUMS; ++k) {
        const double v = wave_sum_d(acc[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < MET_SUMS)
        part[(long)blockIdx.x * MET_SUMS + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void depth_metrics_reduce_kernel(const double* __restrict__ part, int nblocks, double* __restrict__ sums) {
    __shared__ double red[4][MET_SUMS];
    double acc[MET_SUMS];
#pragma unroll
    for (int k = 0; k < MET_SUMS; ++k) acc[k] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256)
#pragma unroll
        for (int k = 0; k < MET_SUMS; ++k) acc[k] += part[(long)b * MET_SUMS + k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < MET_SUMS; ++k) {
        const double v = wave_sum_d(acc[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < MET_SUMS) sums[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

int met_blocks(long n) { return (int)std::min((n + 255) / 256, (long)MET_BLOCKS); }

}  // namespace

extern "C" int geo4d_bicubic_resize(const float* x, float* y, int T, int h, int w, int OH, int OW, void* stream) {
    if (!x || !y || T <= 0 || h <= 0 || w <= 0 || OH <= 0 || OW <= 0 || T > 65535) {
        geo4d_set_error("bicubic_resize: bad arguments");
        return GEO4D_EINVAL;
    }
    const long per = (long)OH * OW;
    const int gx = (int)std::min((per + 255) / 256, 4096L);
    hipLaunchKernelGGL(bicubic_resize_kernel, dim3(gx, T), dim3(256), 0, (hipStream_t)stream, x, y, h, w, OH, OW, (float)h / (float)OH,
                       (float)w / (float)OW);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" size_t geo4d_masked_select_workspace(long n) {
    if (n <= 0) return 0;
    return (size_t)((n + SEL_TILE - 1) / SEL_TILE) * sizeof(unsigned);
}

extern "C" int geo4d_masked_select(const float* pred, const float* gt, long n, float max_depth, const unsigned char* mask, float pre_min,
                                   float pre_max, float* pred_out, float* gt_out, long* count, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (!pred || !gt || !pred_out || !gt_out || !count || n <= 0 || n >= (1L << 32) || !workspace ||
        workspace_bytes < geo4d_masked_select_workspace(n) || std::isnan(max_depth)) {
        geo4d_set_error("masked_select: bad arguments / workspace too small");
        return GEO4D_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const long nblocks = (n + SEL_TILE - 1) / SEL_TILE;
    const int bounded = std::isinf(max_depth) ? 0 : 1;
    unsigned* blk = (unsigned*)workspace;
    hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, gt, mask, n, max_depth, bounded, blk);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, s, blk, nblocks, count);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_scatter_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, pred, gt, mask, n, max_depth, bounded, pre_min, pre_max, blk,
                       pred_out, gt_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" size_t geo4d_depth_metrics_workspace(long n) {
    if (n <= 0) return 0;
    return (size_t)met_blocks(n) * MET_SUMS * sizeof(double);
}

extern "C" int geo4d_depth_metrics(const float* pred, const float* gt, long n, float max_depth, const unsigned char* custom_mask, const float* st,
                                   float pre_min, float pre_max, float post_min, float post_max, double* sums, float* err_map, float* aligned,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!pred || !gt || !st || !sums || !err_map || n <= 0 || !workspace || workspace_bytes < geo4d_depth_metrics_workspace(n) ||
        std::isnan(max_depth)) {
        geo4d_set_error("depth_metrics: bad arguments / workspace too small");
        return GEO4D_EINVAL;
    }
    if ((size_t)workspace % 8) { geo4d_set_error("depth_metrics: workspace must be 8-byte aligned"); return GEO4D_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const int nb = met_blocks(n);
    double* part = (double*)workspace;
    hipLaunchKernelGGL(depth_metrics_kernel, dim3(nb), dim3(256), 0, s, pred, gt, n, max_depth, std::isinf(max_depth) ? 0 : 1, custom_mask, st,
                       pre_min, pre_max, post_min, post_max, err_map, aligned, part);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(depth_metrics_reduce_kernel, dim3(1), dim3(256), 0, s, part, nb, sums);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
