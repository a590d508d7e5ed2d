// geo4d_amd/csrc/render.hip — frames of the aligned scene: z-buffered point splats (geo4d_amd/render.py).
//
// The reference shows a reconstruction in a browser (viser, WebGL); nothing of that is ported. This is the project's own renderer and
// every rule is stated here, in include/geo4d_hip.h and, in numpy, in tests/render_restatement.py.
//
// splat:   one thread per (view, source image, point of that image). The point goes to camera space (scene_view.h), is dropped when masked
//          out, non-finite or not beyond `near`, and is projected with the project's pixel rule (pixel i sits at coordinate i). Its square
//          footprint of side s (1, or from a world radius) is clipped to the image and every covered pixel gets one 64-bit atomicMin of
//          key = float_bits(zc) << 32 | point id. Positive floats order as unsigned integers, so the minimum key is the nearest point and
//          at equal depth the lower id: the buffer does not depend on the order the atomics arrive in, and is bitwise reproducible.
// fill:    an empty pixel takes the minimum key of its 3 x 3 neighbours, k passes between two buffers.
// resolve: key -> colour (ops.scene_points' quantisation), depth and point id.
//
// Products and sums are written in the documented order with contraction into FMAs switched off, as in depth_eval.hip, so the float32
// numpy restatement rounds where the kernel does.
#include <cmath>
#include <vector>
#include "common.h"
#include "geo4d_hip.h"
#include "scene_view.h"                                                              // u64, the view, to_camera, dims_ok, refuse

#pragma clang fp contract(off)

namespace {

constexpr u64 EMPTY = ~0ull;         // a pixel no point has landed on
constexpr int MAX_FOOTPRINT = 64;

// first covered pixel and count along one axis: c0 = floor(u - 0.5 (s - 1) + 0.5), pixels c0 .. c0 + s - 1 clipped to [0, size).
// Decided in float before any cast, so a far-away projection cannot overflow the int.
__device__ __forceinline__ bool footprint(float u, int s, int size, int& lo, int& hi) {
    const float c0 = floorf(u - 0.5f * (float)(s - 1) + 0.5f);
    if (!(c0 < (float)size && c0 + (float)s > 0.f)) return false;                   // outside, or NaN
    const int i0 = (int)c0;
    lo = max(i0, 0);
    hi = min(i0 + s, size);
    return true;
}

// entries [E][2] = (view, source image) of every item of the views' source lists; blocks_per_image blocks of 256 points per entry
__global__ __launch_bounds__(256) void render_splat_kernel(u64* __restrict__ zbuf, const float* __restrict__ points,
                                                           const unsigned char* __restrict__ mask, const float* __restrict__ radius,
                                                           const float* __restrict__ views, const int* __restrict__ entries,
                                                           long pts_per_image, unsigned blocks_per_image, int H, int W, float near,
                                                           int max_size) {
    const unsigned e = blockIdx.x / blocks_per_image;
    const long p = (long)(blockIdx.x - e * blocks_per_image) * 256 + threadIdx.x;
    if (p >= pts_per_image) return;
    const int view = entries[2 * e], src = entries[2 * e + 1];
    const long id = (long)src * pts_per_image + p;
    if (mask && !mask[id]) return;
    const float X = points[id * 3], Y = points[id * 3 + 1], Z = points[id * 3 + 2];
    if (!finite3(X, Y, Z)) return;
    const float* M = views + (long)view * VIEW_FLOATS;
    float xc, yc, zc;
    to_camera(M, X, Y, Z, xc, yc, zc);
    // scene_view.h's project(), written out: through the helper this kernel compiles to other code than it had (same registers, one
    // timed row 0.03 % over its margin, profiles/scene_shared.md), and so the lines stay here
    if (!finite3(xc, yc, zc) || zc <= near) return;
    const float fx = M[12], fy = M[13];
    const float u = fx * (xc / zc) + M[14];
    const float v = fy * (yc / zc) + M[15];
    int s = 1;
    if (radius) {
        const float sf = ceilf(2.f * radius[id] * fx / zc);
        s = sf >= (float)max_size ? max_size : (sf >= 1.f ? (int)sf : 1);           // NaN -> 1
    }
    int x0, x1, y0, y1;
    if (!footprint(u, s, W, x0, x1) || !footprint(v, s, H, y0, y1)) return;
    const u64 key = ((u64)__float_as_uint(zc) << 32) | (u64)(unsigned)id;
    u64* img = zbuf + (long)view * H * W;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) atomicMin(img + (long)y * W + x, key);
}

__global__ __launch_bounds__(256) void render_fill_kernel(u64* __restrict__ out, const u64* __restrict__ in, long total, int H, int W) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    u64 k = in[i];
    if (k == EMPTY) {
        const long hw = (long)H * W, r = i % hw;
        const int y = (int)(r / W), x = (int)(r - (long)y * W);
        const u64* img = in + (i - r);
        for (int yy = max(y - 1, 0); yy <= min(y + 1, H - 1); ++yy)
            for (int xx = max(x - 1, 0); xx <= min(x + 1, W - 1); ++xx) {
                const u64 q = img[(long)yy * W + xx];
                k = q < k ? q : k;
            }
    }
    out[i] = k;
}

__global__ __launch_bounds__(256) void render_resolve_kernel(const u64* __restrict__ zbuf, const float* __restrict__ colors, long N, long total,
                                                             float bg_r, float bg_g, float bg_b, unsigned char* __restrict__ rgb,
                                                             float* __restrict__ depth, int* __restrict__ index) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const u64 k = zbuf[i];
    float r = bg_r, g = bg_g, b = bg_b, d = 0.f;
    int id = -1;
    const unsigned pid = (unsigned)k;
    if (k != EMPTY && (long)pid < N) {                                              // an id beyond colors reads nothing
        id = (int)pid;
        d = __uint_as_float((unsigned)(k >> 32));
        const float* c = colors + (long)pid * 3;
        r = c[0]; g = c[1]; b = c[2];
    }
    if (rgb) {                                                                      // quant_u8: the glb's vertex colours
        rgb[i * 3] = (unsigned char)quant_u8(r); rgb[i * 3 + 1] = (unsigned char)quant_u8(g); rgb[i * 3 + 2] = (unsigned char)quant_u8(b);
    }
    if (depth) depth[i] = d;
    if (index) index[i] = id;
}

size_t zbuf_bytes(int V, int H, int W) { return (size_t)V * H * W * sizeof(u64); }

}  // namespace

// two z-buffers (fill's ping-pong; the first is THE buffer every call reads and leaves its result in), then the (view, source) entries
extern "C" size_t geo4d_render_workspace(int V, int H, int W, long n_entries) {
    if (!dims_ok(V, H, W) || n_entries < 0 || n_entries >= (1L << 31)) return 0;
    return 2 * zbuf_bytes(V, H, W) + (size_t)n_entries * 2 * sizeof(int);
}

extern "C" int geo4d_render_splat(const float* points, const unsigned char* mask, const float* radius, long N, long pts_per_image,
                                  const float* views, const int* view_src_ptr, const int* view_src, int V, int H, int W, float near,
                                  int max_size, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "render_splat";
    if (!points || !views || !view_src_ptr || !workspace || (size_t)workspace % 8)
        return refuse(who, "points, views, view_src_ptr and an 8-byte aligned workspace are required");
    if (!dims_ok(V, H, W)) return refuse(who, "need V, H, W > 0 and V * H * W < 2^31");
    if (N <= 0 || N >= (1L << 32) - 1 || pts_per_image <= 0 || N % pts_per_image)
        return refuse(who, "need 0 < N < 2^32 - 1 points in whole images of pts_per_image points");
    if (!(near >= 0.f) || max_size < 1 || max_size > MAX_FOOTPRINT) return refuse(who, "need near >= 0 and 1 <= max_size <= 64");
    const long n_img = N / pts_per_image, E = view_src_ptr[V];
    bool ok = view_src_ptr[0] == 0 && E >= 0 && (E == 0 || view_src);
    for (int v = 0; ok && v < V; ++v) ok = view_src_ptr[v] <= view_src_ptr[v + 1];
    for (long k = 0; ok && k < E; ++k) ok = view_src[k] >= 0 && view_src[k] < n_img;
    if (!ok) return refuse(who, "view_src_ptr must rise from 0 and every source index must name one of the N / pts_per_image images");
    const long bpi = (pts_per_image + 255) / 256;
    if (E * bpi >= (1L << 31)) return refuse(who, "too many (view, source image) blocks for one launch; render fewer views per call");
    if (workspace_bytes < geo4d_render_workspace(V, H, W, E)) return refuse(who, "workspace too small (geo4d_render_workspace bytes)");
    hipStream_t s = (hipStream_t)stream;
    u64* zbuf = (u64*)workspace;
    if (hipMemsetAsync(zbuf, 0xff, zbuf_bytes(V, H, W), s) != hipSuccess) {
        geo4d_set_error("render_splat: hipMemsetAsync failed");
        return GEO4D_EIO;
    }
    if (E == 0) return GEO4D_OK;
    // the host array outlives the call: the copy from pageable memory is staged or complete when hipMemcpyAsync returns, and the next
    // call on this thread is the first that rewrites it
    static thread_local std::vector<int> entries;
    entries.resize((size_t)E * 2);
    for (int v = 0; v < V; ++v)
        for (long k = view_src_ptr[v]; k < view_src_ptr[v + 1]; ++k) {
            entries[2 * k] = v;
            entries[2 * k + 1] = view_src[k];
        }
    int* dev_entries = (int*)((char*)workspace + 2 * zbuf_bytes(V, H, W));
    if (hipMemcpyAsync(dev_entries, entries.data(), entries.size() * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) {
        geo4d_set_error("render_splat: copying the source lists to the device failed");
        return GEO4D_EIO;
    }
    hipLaunchKernelGGL(render_splat_kernel, dim3((unsigned)(E * bpi)), dim3(256), 0, s, zbuf, points, mask, radius, views, dev_entries,
                       pts_per_image, (unsigned)bpi, H, W, near, max_size);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_render_fill(int V, int H, int W, int passes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!workspace || (size_t)workspace % 8 || !dims_ok(V, H, W) || passes < 0 || workspace_bytes < 2 * zbuf_bytes(V, H, W))
        return refuse("render_fill", "need an 8-byte aligned workspace of geo4d_render_workspace bytes, V, H, W > 0, V * H * W < 2^31, "
                                     "passes >= 0");
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)V * H * W;
    u64 *a = (u64*)workspace, *b = a + total;
    for (int k = 0; k < passes; ++k) {
        hipLaunchKernelGGL(render_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, b, a, total, H, W);
        GEO4D_CHECK_LAUNCH();
        u64* t = a; a = b; b = t;
    }
    if (passes & 1 && hipMemcpyAsync(workspace, a, zbuf_bytes(V, H, W), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        geo4d_set_error("render_fill: copying the filled buffer back failed");
        return GEO4D_EIO;
    }
    return GEO4D_OK;
}

extern "C" int geo4d_render_resolve(const float* colors, long N, const float* background, int V, int H, int W, unsigned char* rgb,
                                    float* depth, int* index, const void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "render_resolve";
    if (!workspace || (size_t)workspace % 8 || !dims_ok(V, H, W) || workspace_bytes < zbuf_bytes(V, H, W))
        return refuse(who, "need the 8-byte aligned workspace geo4d_render_splat wrote, V, H, W > 0, V * H * W < 2^31");
    if (!colors || !background || N <= 0 || N >= (1L << 31) || (!rgb && !depth && !index))
        return refuse(who, "need colors [N][3], a host background [3], 0 < N < 2^31 (index is int32) and at least one output");
    const long total = (long)V * H * W;
    hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)workspace, colors, N, total, background[0], background[1], background[2], rgb, depth, index);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
