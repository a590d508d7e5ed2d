// geo4d_amd/csrc/render_mesh.hip — triangle meshes in the renderer: an exact raster into render.hip's 64-bit z-buffer, and the
// resolve that shades what won (geo4d_amd/render.py: render_mesh, render_scene(static_mesh=...)).
//
// Nothing is ported; every rule is stated here, in include/geo4d_hip.h and, in numpy, in tests/render_mesh_restatement.py.
//
// set-up:  a triangle's three vertices go to camera space and through project() of scene_view.h. The triangle is dropped when masked
//          out, when an index is outside [0, Nv), when a vertex is not finite or not beyond `near` (no clipping), or when a projection
//          leaves the guard band |u|, |v| < 65536 (decided in float, so NaN drops). Image coordinates are snapped to 1/256 pixel:
//          X = floor(u * 256 + 0.5). Everything that decides coverage from here on is int64: edge(A, B, S) = (Bx - Ax)(Sy - Ay) -
//          (By - Ay)(Sx - Ax), below 2^51 in magnitude; area A = edge(P0, P1, P2), 0 drops, > 0 is a back face (y points down).
// raster:  pixel (x, y), sampled at (256 x, 256 y), is covered iff E0, E1, E2 >= 0 after the sign of a front face has been flipped:
//          every edge inclusive, no top-left rule; two triangles that share an edge both claim its pixels and the depth test decides.
//          w_k = (float)((double)E_k / (double)A), q = ((w0 iz0) + (w1 iz1)) + (w2 iz2) with iz_k = 1 / zc_k, zc = 1 / q: one atomicMin
//          of float_bits(zc) << 32 | (id_base + t), the same vector atomic as the splat. One thread per (view, triangle) walks the
//          clipped bounding box when it holds at most large_area pixels; larger ones are appended to a list that a second launch walks
//          one wave per entry, the lanes striding over the box. A full list makes the appending thread draw the triangle itself.
// resolve: a point key as render.hip resolves it; a triangle key repeats the set-up and the pixel's weights (the same integers, hence
//          the same floats), interpolates the vertex colours perspective-correctly and applies flat headlight shading.
//
// Products and sums are written in the documented order with contraction into FMAs switched off; the divisions and the square root
// are the correctly rounded ones (hipcc's default for fp32, IEEE for fp64), so the numpy restatement rounds where the kernels do.
#include <cmath>
#include "common.h"
#include "geo4d_hip.h"
#include "scene_view.h"                                                              // u64, the view, to_camera, project, dims_ok, refuse

#pragma clang fp contract(off)

namespace {

constexpr u64 EMPTY = ~0ull;
constexpr int MAX_FRAME = 16384;          // H, W cap: with the guard band every edge function stays below 2^51
constexpr float GUARD = 65536.f;
constexpr int WALK_BLOCKS = 1024;         // blocks of the list walk (4 waves each, one entry per wave and step)
constexpr size_t LIST_HEADER = 8;         // the list's count (unsigned, device memory), then (view, triangle) int pairs

struct Tri {
    int X0, Y0, X1, Y1, X2, Y2;           // snapped image coordinates, |.| <= 2^24
    float iz0, iz1, iz2;
    long A;                               // > 0 once `neg` has been applied
    bool neg;                             // a front face: A and every E_k change sign
    int x0, x1, y0, y1;                   // the clipped bounding box, inclusive; empty when x0 > x1 or y0 > y1
};

__device__ __forceinline__ long edge(int ax, int ay, int bx, int by, long sx, long sy) {
    return (long)(bx - ax) * (sy - ay) - (long)(by - ay) * (sx - ax);
}

// one vertex: camera coordinates (for the shading), 1 / zc and the snapped projection; false when the rule drops the triangle
__device__ __forceinline__ bool tri_vertex(const float* M, const float* __restrict__ vertices, int i, float near, float& xc, float& yc,
                                           float& zc, float& iz, int& X, int& Y) {
    const float* p = vertices + (long)i * 3;
    to_camera(M, p[0], p[1], p[2], xc, yc, zc);
    float u, v;
    const bool ok = project(M, xc, yc, zc, near, u, v);
    if (!ok || !(fabsf(u) < GUARD && fabsf(v) < GUARD)) return false;
    iz = 1.f / zc;
    X = (int)floorf(u * 256.f + 0.5f);
    Y = (int)floorf(v * 256.f + 0.5f);
    return true;
}

// steps 1 to 6 of the rule for triangle t in the view M; cam[9] receives the camera coordinates when asked for
__device__ __forceinline__ bool tri_setup(Tri& T, const float* M, const float* __restrict__ vertices, long Nv, const int* __restrict__ faces,
                                          const unsigned char* __restrict__ face_mask, long t, int H, int W, float near, int cull_back,
                                          float* cam = nullptr) {
    if (face_mask && !face_mask[t]) return false;
    const int i0 = faces[t * 3], i1 = faces[t * 3 + 1], i2 = faces[t * 3 + 2];
    if (i0 < 0 || i0 >= Nv || i1 < 0 || i1 >= Nv || i2 < 0 || i2 >= Nv) return false;
    float x, y, z;
    if (!tri_vertex(M, vertices, i0, near, x, y, z, T.iz0, T.X0, T.Y0)) return false;
    if (cam) { cam[0] = x; cam[1] = y; cam[2] = z; }
    if (!tri_vertex(M, vertices, i1, near, x, y, z, T.iz1, T.X1, T.Y1)) return false;
    if (cam) { cam[3] = x; cam[4] = y; cam[5] = z; }
    if (!tri_vertex(M, vertices, i2, near, x, y, z, T.iz2, T.X2, T.Y2)) return false;
    if (cam) { cam[6] = x; cam[7] = y; cam[8] = z; }
    const long A = edge(T.X0, T.Y0, T.X1, T.Y1, T.X2, T.Y2);
    if (A == 0 || (cull_back && A > 0)) return false;
    T.neg = A < 0;
    T.A = T.neg ? -A : A;
    const int minX = min(T.X0, min(T.X1, T.X2)), maxX = max(T.X0, max(T.X1, T.X2));
    const int minY = min(T.Y0, min(T.Y1, T.Y2)), maxY = max(T.Y0, max(T.Y1, T.Y2));
    T.x0 = max(0, (minX + 255) >> 8);
    T.x1 = min(W - 1, maxX >> 8);
    T.y0 = max(0, (minY + 255) >> 8);
    T.y1 = min(H - 1, maxY >> 8);
    return true;
}

// step 6's test and step 7's weights and depth at pixel (x, y); false when the pixel is not covered or zc is not > 0
__device__ __forceinline__ bool tri_pixel(const Tri& T, int x, int y, float& w0, float& w1, float& w2, float& zc) {
    const long sx = (long)x * 256, sy = (long)y * 256;
    long E0 = edge(T.X1, T.Y1, T.X2, T.Y2, sx, sy);
    long E1 = edge(T.X2, T.Y2, T.X0, T.Y0, sx, sy);
    long E2 = edge(T.X0, T.Y0, T.X1, T.Y1, sx, sy);
    if (T.neg) { E0 = -E0; E1 = -E1; E2 = -E2; }
    if (E0 < 0 || E1 < 0 || E2 < 0) return false;
    const double A = (double)T.A;
    w0 = (float)((double)E0 / A);
    w1 = (float)((double)E1 / A);
    w2 = (float)((double)E2 / A);
    const float q = ((w0 * T.iz0) + (w1 * T.iz1)) + (w2 * T.iz2);
    zc = 1.f / q;
    return zc > 0.f;
}

__device__ __forceinline__ void tri_write(const Tri& T, u64* __restrict__ img, int W, int x, int y, unsigned id) {
    float w0, w1, w2, zc;
    if (tri_pixel(T, x, y, w0, w1, w2, zc)) atomicMin(img + (long)y * W + x, ((u64)__float_as_uint(zc) << 32) | (u64)id);
}

// blocks_per_view blocks of 256 triangles per view: the view is block-uniform, its 16 floats are scalar loads
__global__ __launch_bounds__(256) void render_raster_kernel(u64* __restrict__ zbuf, const float* __restrict__ vertices, long Nv,
                                                            const int* __restrict__ faces, long T, const unsigned char* __restrict__ face_mask,
                                                            const float* __restrict__ views, unsigned blocks_per_view, int H, int W, float near,
                                                            int cull_back, unsigned id_base, int large_area, unsigned* __restrict__ count,
                                                            int* __restrict__ list, unsigned capacity) {
    const unsigned view = blockIdx.x / blocks_per_view;
    const long t = (long)(blockIdx.x - view * blocks_per_view) * 256 + threadIdx.x;
    if (t >= T) return;
    const float* M = views + (long)view * VIEW_FLOATS;
    Tri tri;
    if (!tri_setup(tri, M, vertices, Nv, faces, face_mask, t, H, W, near, cull_back)) return;
    if (tri.x0 > tri.x1 || tri.y0 > tri.y1) return;
    if ((long)(tri.x1 - tri.x0 + 1) * (tri.y1 - tri.y0 + 1) > large_area) {
        const unsigned slot = atomicAdd(count, 1u);
        if (slot < capacity) {
            list[2 * (long)slot] = (int)view;
            list[2 * (long)slot + 1] = (int)t;
            return;
        }                                                                           // a full list: this thread draws it, slowly
    }
    u64* img = zbuf + (long)view * H * W;
    const unsigned id = id_base + (unsigned)t;
    for (int y = tri.y0; y <= tri.y1; ++y)
        for (int x = tri.x0; x <= tri.x1; ++x) tri_write(tri, img, W, x, y, id);
}

// the listed (view, triangle) pairs, one wave per entry, grid-stride; the 64 lanes stride over the entry's bounding box
__global__ __launch_bounds__(256) void render_raster_walk_kernel(u64* __restrict__ zbuf, const float* __restrict__ vertices, long Nv,
                                                                 const int* __restrict__ faces, long T, const float* __restrict__ views,
                                                                 int V, int H, int W, float near, unsigned id_base,
                                                                 const unsigned* __restrict__ count, const int* __restrict__ list,
                                                                 unsigned capacity) {
    const unsigned n = min(*count, capacity);
    const unsigned lane = threadIdx.x & 63;
    for (unsigned e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += gridDim.x * 4) {
        // e is the same in all 64 lanes: say so, and the view, the indices and the vertices come through scalar loads
        const int view = __builtin_amdgcn_readfirstlane(list[2 * (long)e]), t = __builtin_amdgcn_readfirstlane(list[2 * (long)e + 1]);
        if (view < 0 || view >= V || t < 0 || t >= T) continue;                      // only what the first kernel wrote is ever here
        Tri tri;
        // mask and culling were decided when the entry was appended
        if (!tri_setup(tri, views + (long)view * VIEW_FLOATS, vertices, Nv, faces, nullptr, t, H, W, near, 0)) continue;
        if (tri.x0 > tri.x1 || tri.y0 > tri.y1) continue;
        u64* img = zbuf + (long)view * H * W;
        const unsigned id = id_base + (unsigned)t;
        const unsigned bw = (unsigned)(tri.x1 - tri.x0 + 1), area = bw * (unsigned)(tri.y1 - tri.y0 + 1);
        for (unsigned i = lane; i < area; i += 64) {
            const unsigned r = i / bw;
            tri_write(tri, img, W, tri.x0 + (int)(i - r * bw), tri.y0 + (int)r, id);
        }
    }
}

// vertex k's colour: u8 rgba (alpha ignored) as c / 255, or float [Nv][3] as given, or the uniform colour
__device__ __forceinline__ void vertex_color(const unsigned char* __restrict__ rgba, const float* __restrict__ rgbf, int i, float mr, float mg,
                                             float mb, float& r, float& g, float& b) {
    if (rgba) {
        const unsigned char* c = rgba + (long)i * 4;
        r = (float)c[0] / 255.f; g = (float)c[1] / 255.f; b = (float)c[2] / 255.f;
    } else if (rgbf) {
        const float* c = rgbf + (long)i * 3;
        r = c[0]; g = c[1]; b = c[2];
    } else {
        r = mr; g = mg; b = mb;
    }
}

__global__ __launch_bounds__(256) void render_resolve_mesh_kernel(const u64* __restrict__ zbuf, const float* __restrict__ colors, long N,
                                                                  const float* __restrict__ vertices, long Nv, const int* __restrict__ faces,
                                                                  long T, const unsigned char* __restrict__ vertex_rgba,
                                                                  const float* __restrict__ vertex_rgb, float mr, float mg, float mb,
                                                                  const float* __restrict__ views, int H, int W, float near, float shade,
                                                                  long total, float bg_r, float bg_g, float bg_b,
                                                                  unsigned char* __restrict__ rgb, float* __restrict__ depth,
                                                                  int* __restrict__ index, int* __restrict__ face) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const u64 k = zbuf[i];
    float r = bg_r, g = bg_g, b = bg_b, d = 0.f;
    int id = -1, fid = -1;
    const long kid = (long)(unsigned)k;
    if (k != EMPTY && kid < N) {                                                    // a point, as render_resolve_kernel has it
        id = (int)kid;
        d = __uint_as_float((unsigned)(k >> 32));
        const float* c = colors + kid * 3;
        r = c[0]; g = c[1]; b = c[2];
    } else if (k != EMPTY && kid - N < T) {                                         // a triangle; anything beyond reads nothing
        const long t = kid - N;
        const long hw = (long)H * W, view = i / hw, px = i - view * hw;
        const int y = (int)(px / W), x = (int)(px - (long)y * W);
        Tri tri;
        float cam[9], w0, w1, w2, zr;
        if (tri_setup(tri, views + view * VIEW_FLOATS, vertices, Nv, faces, nullptr, t, H, W, near, 0, cam) &&
            tri_pixel(tri, x, y, w0, w1, w2, zr)) {                                 // always true for a key the raster wrote
            fid = (int)t;
            d = __uint_as_float((unsigned)(k >> 32));
            const float b0 = (w0 * tri.iz0) * d, b1 = (w1 * tri.iz1) * d, b2 = (w2 * tri.iz2) * d;
            float r0, g0, c0, r1, g1, c1, r2, g2, c2;
            vertex_color(vertex_rgba, vertex_rgb, faces[t * 3], mr, mg, mb, r0, g0, c0);
            vertex_color(vertex_rgba, vertex_rgb, faces[t * 3 + 1], mr, mg, mb, r1, g1, c1);
            vertex_color(vertex_rgba, vertex_rgb, faces[t * 3 + 2], mr, mg, mb, r2, g2, c2);
            r = (b0 * r0 + b1 * r1) + b2 * r2;
            g = (b0 * g0 + b1 * g1) + b2 * g2;
            b = (b0 * c0 + b1 * c1) + b2 * c2;
            if (shade > 0.f) {                                                      // flat headlight: |n_z| / |n| of the camera-space normal
                const float e1x = cam[3] - cam[0], e1y = cam[4] - cam[1], e1z = cam[5] - cam[2];
                const float e2x = cam[6] - cam[0], e2y = cam[7] - cam[1], e2z = cam[8] - cam[2];
                const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
                const float len2 = (nx * nx + ny * ny) + nz * nz;
                const float lam = len2 > 0.f ? fabsf(nz) / sqrtf(len2) : 0.f;
                const float s = (1.f - shade) + shade * lam;
                r = r * s; g = g * s; b = b * s;
            }
        }
    }
    if (rgb) {
        rgb[i * 3] = (unsigned char)quant_u8(r); rgb[i * 3 + 1] = (unsigned char)quant_u8(g); rgb[i * 3 + 2] = (unsigned char)quant_u8(b);
    }
    if (depth) depth[i] = d;
    if (index) index[i] = id;
    if (face) face[i] = fid;
}

size_t zbuf_bytes(int V, int H, int W) { return (size_t)V * H * W * sizeof(u64); }

bool mesh_ok(const float* vertices, long Nv, const int* faces, long T) {
    return Nv >= 0 && Nv < (1L << 31) && T >= 0 && (Nv == 0 || vertices) && (T == 0 || faces);
}

}  // namespace

// the list of large (view, triangle) pairs: an 8-byte count, then `capacity` pairs of int
extern "C" size_t geo4d_render_raster_workspace(long capacity) {
    if (capacity < 0 || capacity > (1L << 28)) return 0;
    return LIST_HEADER + (size_t)capacity * 2 * sizeof(int);
}

extern "C" int geo4d_render_raster(const float* vertices, long Nv, const int* faces, long T, const unsigned char* face_mask,
                                   const float* views, int V, int H, int W, float near, int cull_back, long id_base, int clear,
                                   int large_area, void* workspace, size_t workspace_bytes, void* list, size_t list_bytes, void* stream) {
    const char* who = "render_raster";
    if (!views || !workspace || (size_t)workspace % 8 || !list || (size_t)list % 8)
        return refuse(who, "views, an 8-byte aligned workspace and an 8-byte aligned list are required");
    if (!dims_ok(V, H, W) || H > MAX_FRAME || W > MAX_FRAME) return refuse(who, "need V, H, W > 0, H, W <= 16384 and V * H * W < 2^31");
    if (!mesh_ok(vertices, Nv, faces, T)) return refuse(who, "need vertices [Nv][3] and faces [T][3] with 0 <= Nv < 2^31 and T >= 0");
    if (id_base < 0 || id_base + T >= (1L << 32) - 1) return refuse(who, "need id_base >= 0 and id_base + T < 2^32 - 1");
    if (!(near >= 0.f) || large_area < 0) return refuse(who, "need near >= 0 and large_area >= 0");
    if (workspace_bytes < zbuf_bytes(V, H, W)) return refuse(who, "workspace too small (geo4d_render_workspace bytes)");
    if (list_bytes < LIST_HEADER) return refuse(who, "list too small (geo4d_render_raster_workspace bytes)");
    const long bpv = (T + 255) / 256;
    if (V * bpv >= (1L << 31)) return refuse(who, "too many (view, triangle) blocks for one launch; render fewer views per call");
    hipStream_t s = (hipStream_t)stream;
    u64* zbuf = (u64*)workspace;
    if (clear && hipMemsetAsync(zbuf, 0xff, zbuf_bytes(V, H, W), s) != hipSuccess) {
        geo4d_set_error("render_raster: hipMemsetAsync failed");
        return GEO4D_EIO;
    }
    if (T == 0) return GEO4D_OK;
    size_t cap = (list_bytes - LIST_HEADER) / (2 * sizeof(int));
    if (cap > (1u << 28)) cap = 1u << 28;
    unsigned* count = (unsigned*)list;
    int* entries = (int*)((char*)list + LIST_HEADER);
    if (hipMemsetAsync(count, 0, LIST_HEADER, s) != hipSuccess) {
        geo4d_set_error("render_raster: hipMemsetAsync of the list count failed");
        return GEO4D_EIO;
    }
    hipLaunchKernelGGL(render_raster_kernel, dim3((unsigned)(V * bpv)), dim3(256), 0, s, zbuf, vertices, Nv, faces, T, face_mask, views,
                       (unsigned)bpv, H, W, near, cull_back, (unsigned)id_base, large_area, count, entries, (unsigned)cap);
    GEO4D_CHECK_LAUNCH();
    if (cap) {
        hipLaunchKernelGGL(render_raster_walk_kernel, dim3(WALK_BLOCKS), dim3(256), 0, s, zbuf, vertices, Nv, faces, T, views, V, H, W, near,
                           (unsigned)id_base, count, entries, (unsigned)cap);
        GEO4D_CHECK_LAUNCH();
    }
    return GEO4D_OK;
}

extern "C" int geo4d_render_resolve_mesh(const float* colors, long N, const float* vertices, long Nv, const int* faces, long T,
                                         const unsigned char* vertex_rgba, const float* vertex_rgb, const float* mesh_color,
                                         const float* views, float near, float shade, const float* background, int V, int H, int W,
                                         unsigned char* rgb, float* depth, int* index, int* face, const void* workspace,
                                         size_t workspace_bytes, void* stream) {
    const char* who = "render_resolve_mesh";
    if (!workspace || (size_t)workspace % 8 || !dims_ok(V, H, W) || H > MAX_FRAME || W > MAX_FRAME || workspace_bytes < zbuf_bytes(V, H, W))
        return refuse(who, "need the 8-byte aligned workspace geo4d_render_raster wrote, V, H, W > 0, H, W <= 16384, V * H * W < 2^31");
    if (!views || !background || !mesh_color || (!rgb && !depth && !index && !face))
        return refuse(who, "need views, host arrays background [3] and mesh_color [3], and at least one output");
    if (N < 0 || N >= (1L << 31) || (N > 0 && !colors)) return refuse(who, "need 0 <= N < 2^31 points (index is int32) and colors [N][3]");
    if (!mesh_ok(vertices, Nv, faces, T) || T >= (1L << 31))                        // so N + T < 2^32 - 1, the raster's bound
        return refuse(who, "need vertices [Nv][3] and faces [T][3] with 0 <= Nv, T < 2^31 (face is int32)");
    if (vertex_rgba && vertex_rgb) return refuse(who, "vertex colours are rgba u8 or rgb fp32, not both");
    if (!(near >= 0.f) || !(shade >= 0.f && shade <= 1.f)) return refuse(who, "need near >= 0 and 0 <= shade <= 1");
    const long total = (long)V * H * W;
    hipLaunchKernelGGL(render_resolve_mesh_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)workspace, colors, N, vertices, Nv, faces, T, vertex_rgba, vertex_rgb, mesh_color[0], mesh_color[1],
                       mesh_color[2], views, H, W, near, shade, total, background[0], background[1], background[2], rgb, depth, index, face);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
