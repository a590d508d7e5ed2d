// geo4d_amd/csrc/motion.hip — which pixels of the aligned scene moved: geometric votes between the images (geo4d_amd/motion.py).
//
// The reference's results folder has dynamic_mask_{i}.png, filled there from optical flow and SAM2; nothing of that is ported. This
// rule is the project's own and is stated here, in include/geo4d_hip.h and, in numpy, in tests/motion_restatement.py.
//
// range: one thread per (image j, pixel q): dmin / dmax = minimum / maximum of depth[j] over the valid pixels of q's 3 x 3
//        neighbourhood inside the image, so that a depth edge one pixel off does not read as motion. Written once per image as a
//        float2; every image is then read by up to 2 radius others, and a vote gathers those 8 bytes and nothing else: an invalid
//        pixel q carries dmin = NaN, which no range of a valid pixel can be (its own depth, when NaN, never wins a comparison and the
//        range stays (+inf, -inf)), so the mask byte is folded into the gather.
// votes: one thread per (image i, pixel p), blocks image-uniform, so voter j's 16 view floats are wave-uniform (scalar loads). For
//        every j with 0 < |j - i| <= radius the world point goes to j's camera and pixel with the project's pixel rule (scene_view.h:
//        pixel k sits at coordinate k, inside / outside decided in float before any cast) and counts as
//          free       zc < dmin lo   j sees past the place where the point was: it is not there at time j
//          occluded   zc > dmax hi   something is in front: no evidence either way
//          consistent otherwise
//        with lo = 1 - tol, hi = 1 + tol formed in fp32 on the host. Every output byte has one writer; no atomics.
//
// Products and sums are written in the documented order with contraction into FMAs switched off, as in render.hip, so the float32
// numpy restatement rounds where the kernel does.
#include <cmath>
#include "common.h"
#include "geo4d_hip.h"
#include "scene_view.h"                                                              // the view, to_camera, project, pixel_of, dims_ok, refuse

#pragma clang fp contract(off)

namespace {

constexpr int MAX_RADIUS = 127;      // counts <= 2 radius <= 254 fit a byte

__global__ __launch_bounds__(256) void motion_range_kernel(float2* __restrict__ range, const float* __restrict__ depth,
                                                           const unsigned char* __restrict__ valid, long total, int H, int W) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float lo = INFINITY, hi = -INFINITY;
    if (valid && !valid[i]) {
        lo = __builtin_nanf("");
    } else {
        const unsigned hw = (unsigned)H * (unsigned)W, r = (unsigned)i % hw;         // total < 2^31: 32-bit division
        const int y = (int)(r / (unsigned)W), x = (int)(r - (unsigned)y * (unsigned)W);
        const long img = i - r;
        for (int yy = max(y - 1, 0); yy <= min(y + 1, H - 1); ++yy)
            for (int xx = max(x - 1, 0); xx <= min(x + 1, W - 1); ++xx) {
                const long q = img + (long)yy * W + xx;
                if (valid && !valid[q]) continue;
                const float d = depth[q];
                lo = d < lo ? d : lo;                                               // a NaN depth never wins
                hi = d > hi ? d : hi;
            }
    }
    range[i] = make_float2(lo, hi);
}

__global__ __launch_bounds__(256) void motion_votes_kernel(unsigned char* __restrict__ votes, const float* __restrict__ pts3d,
                                                           const float* __restrict__ views, const float2* __restrict__ range, int n,
                                                           long pts_per_image, unsigned blocks_per_image, int H, int W, int radius,
                                                           float lo, float hi, float near) {
    const int i = (int)(blockIdx.x / blocks_per_image);
    const long p = (long)(blockIdx.x - (unsigned)i * blocks_per_image) * 256 + threadIdx.x;
    if (p >= pts_per_image) return;
    const long id = (long)i * pts_per_image + p;
    unsigned consistent = 0, free_ = 0, occluded = 0;
    const float own = range[id].x;
    const float X = pts3d[id * 3], Y = pts3d[id * 3 + 1], Z = pts3d[id * 3 + 2];
    if (own == own && finite3(X, Y, Z)) {
        const int j0 = max(i - radius, 0), j1 = min(i + radius, n - 1);
        const float fW = (float)W, fH = (float)H;
        for (int j = j0; j <= j1; ++j) {
            if (j == i) continue;
            const float* M = views + (long)j * VIEW_FLOATS;
            float xc, yc, zc, u, v, col, row;
            to_camera(M, X, Y, Z, xc, yc, zc);
            if (!project(M, xc, yc, zc, near, u, v)) continue;
            if (!pixel_of(u, v, fW, fH, col, row)) continue;
            const float2 r = range[(long)j * pts_per_image + (long)(int)row * W + (int)col];
            if (r.x != r.x) continue;                                               // j's pixel there is invalid
            if (zc < r.x * lo) ++free_;
            else if (zc > r.y * hi) ++occluded;
            else ++consistent;
        }
    }
    votes[id * 3] = (unsigned char)consistent;
    votes[id * 3 + 1] = (unsigned char)free_;
    votes[id * 3 + 2] = (unsigned char)occluded;
}

}  // namespace

// the depth ranges: one float2 (dmin, dmax) per pixel of every image
extern "C" size_t geo4d_motion_workspace(int n, int H, int W) {
    if (!dims_ok(n, H, W)) return 0;
    return (size_t)n * H * W * sizeof(float2);
}

extern "C" int geo4d_motion_range(const float* depth, const unsigned char* valid, int n, int H, int W, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const char* who = "motion_range";
    if (!depth || !workspace || (size_t)workspace % 8) return refuse(who, "depth and an 8-byte aligned workspace are required");
    if (!dims_ok(n, H, W)) return refuse(who, "need n, H, W > 0 and n * H * W < 2^31");
    if (workspace_bytes < geo4d_motion_workspace(n, H, W)) return refuse(who, "workspace too small (geo4d_motion_workspace bytes)");
    const long total = (long)n * H * W;
    hipLaunchKernelGGL(motion_range_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (float2*)workspace,
                       depth, valid, total, H, W);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_motion_votes(const float* pts3d, const float* views, int n, int H, int W, int radius, float tol, float near,
                                  unsigned char* votes, const void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "motion_votes";
    if (!pts3d || !views || !votes || !workspace || (size_t)workspace % 8)
        return refuse(who, "pts3d, views, votes and the 8-byte aligned workspace geo4d_motion_range wrote are required");
    if (!dims_ok(n, H, W)) return refuse(who, "need n, H, W > 0 and n * H * W < 2^31");
    if (radius < 1 || radius > MAX_RADIUS) return refuse(who, "need 1 <= radius <= 127 (the counts are bytes)");
    if (!(tol > 0.f && tol < 1.f) || !(near >= 0.f)) return refuse(who, "need 0 < tol < 1 and near >= 0");
    if (workspace_bytes < geo4d_motion_workspace(n, H, W)) return refuse(who, "workspace too small (geo4d_motion_workspace bytes)");
    const long hw = (long)H * W, bpi = (hw + 255) / 256;                            // n * bpi <= n * H * W < 2^31
    const float lo = 1.f - tol, hi = 1.f + tol;
    hipLaunchKernelGGL(motion_votes_kernel, dim3((unsigned)(n * bpi)), dim3(256), 0, (hipStream_t)stream, votes, pts3d, views,
                       (const float2*)workspace, n, hw, (unsigned)bpi, H, W, radius, lo, hi, near);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
