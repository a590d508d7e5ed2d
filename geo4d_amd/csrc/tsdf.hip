// geo4d_amd/csrc/tsdf.hip — the static scene denoised: a truncated signed distance function over the voxels near a surface, fused from
// every image that sees them, and the surface points where it crosses zero (geo4d_amd/tsdf.py).
//
// The reference has no such step; nothing is ported. The rule is the project's own and is stated here, in include/geo4d_hip.h and, in
// numpy, in tests/tsdf_restatement.py. All float arithmetic is fp32 in the written order with contraction into FMAs switched off, as in
// render.hip, motion.hip and fuse.hip; only division is used, no sqrt.
//
// Inputs: pts3d [n][H][W][3], depth [n][H][W], valid [n][H][W] bytes (NULL: all), views [n][16] (world-to-camera rows 0..2, then fx, fy,
//   cx, cy, as geo4d_motion_votes takes them), camera centres [n][3], rgba [n][H][W][4] u8 (NULL: no colours), weight [n][H][W] (NULL:
//   every weight is 1), voxel v > 0, truncation T in 1..8 voxels with trunc = (float)T * v, near >= 0, min_weight > 0.
// mark:      pixel (i, p) takes part iff it is valid, its point P and depth are finite and depth > near. d = P - C_i,
//            s = (v * 0.5f) / depth; for k = -2T .. 2T the sample is P_a + ((float)k * s) * d_a, a step of v / 2 in camera z, and its
//            cell floorf(sample_a / v). Keys are voxel_table.h's: (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20) with |c| < 2^20,
//            all ones = empty; a sample whose cell is out of range is counted in `dropped`. One thread per pixel, blocks image-uniform
//            (C_i through scalar loads). The table (voxel_table.h) holds keys only: open addressing, linear probing from a 64-bit mix of
//            the key, a relaxed read, a 64-bit CAS only on an empty slot, forward probing, no lane waits for another. A sample that has
//            probed `capacity` slots without a home is counted in `overflow` and gives up; once the count is not zero the table is known
//            to be full and every lane that looks (each 256 probes) gives up as well, so a full table ends in the host's refusal and not
//            in samples x capacity probes. A sample in the cell of the lane's previous sample is already there and does not probe.
// compact:   voxel_table.h's: 16 slots per thread, one atomicAdd per workgroup; keys only, no slots (nothing hangs on a slot here). The
//            caller sorts the keys: K[0..M).
// integrate: one thread per voxel m, centre X_a = ((float)c_a + 0.5f) * v. For j = 0 .. n-1 in that order (the sums are a function of
//            the inputs alone; j is uniform, so the view floats are scalar loads): xc = ((r00 X + r01 Y) + r02 Z) + t0, likewise yc,
//            zc; skip unless all are finite and zc > near; u = fx (xc / zc) + cx, likewise v; column = floorf(u + 0.5f), row =
//            floorf(v + 0.5f), inside / outside in float before any cast; skip unless j's pixel is valid, its depth finite, its weight
//            w finite and > 0; sd = depth - zc; skip if sd < -trunc; t = fminf(1.f, sd / trunc); D += w * t; Wt += w; if sd <= trunc
//            also C_k += w * (float)rgba_k and Wc += w. Out: f = D / Wt, Wt, colour (u8)clamp(floorf(C_k / Wc + 0.5f), 0, 255) (0 when
//            Wc == 0), alpha 255.
// extract:   voxel m is live iff Wt >= min_weight and |f| < 1. For live m and axis a = 0, 1, 2: the neighbour m' with key K[m] +
//            (1 << 42, 1 << 21, 1)[a] by binary search in K (a carry out of a field gives a key no cell has); if it exists, is live and
//            (f >= 0) != (f' >= 0): one point at X_a + (f / (f - f')) * v on axis a, the centre's coordinates on the others, the colour
//            of the voxel of smaller |f| (m on ties), weight fminf(Wt, Wt'). A count launch, the caller's cumsum, a write launch: rows
//            in (m, a) order, one writer each.
#include <cmath>
#include "common.h"
#include "geo4d_hip.h"
#include "tsdf_field.h"                                                              // centre_of, live, find_key; the view and the table

#pragma clang fp contract(off)

namespace {

constexpr int MAX_TRUNC = 8;

__global__ __launch_bounds__(256) void tsdf_mark_kernel(u64* __restrict__ keys, u64* __restrict__ counters, const float* __restrict__ pts3d,
                                                        const float* __restrict__ depth, const unsigned char* __restrict__ valid,
                                                        const float* __restrict__ centres, long pts_per_image, unsigned blocks_per_image,
                                                        float v, int T, float near, u64 capacity) {
    const int i = (int)(blockIdx.x / blocks_per_image);
    const long p = (long)(blockIdx.x - (unsigned)i * blocks_per_image) * 256 + threadIdx.x;
    if (p >= pts_per_image) return;
    const long id = (long)i * pts_per_image + p;
    if (valid && !valid[id]) return;
    const float X = pts3d[id * 3], Y = pts3d[id * 3 + 1], Z = pts3d[id * 3 + 2], dep = depth[id];
    if (!finite3(X, Y, Z) || !finite1(dep) || !(dep > near)) return;
    const float* C = centres + (long)i * 3;
    const float dx = X - C[0], dy = Y - C[1], dz = Z - C[2];
    const float s = (v * 0.5f) / dep;
    u64 last = EMPTY;
    unsigned dropped = 0;
    for (int k = -2 * T; k <= 2 * T; ++k) {
        const float ks = (float)k * s;
        const float sx = X + ks * dx, sy = Y + ks * dy, sz = Z + ks * dz;
        const float cx = floorf(sx / v), cy = floorf(sy / v), cz = floorf(sz / v);
        if (!cell_ok(cx, cy, cz)) {
            ++dropped;
            continue;
        }
        const u64 key = key_of(cx, cy, cz);
        if (key == last) continue;                                                   // this lane has put it there already
        if (claim_slot(keys, capacity, key, counters + 1) != EMPTY) last = key;
        else atomicAdd(counters + 1, 1ull);                                          // at once: the others look at it
    }
    if (dropped) atomicAdd(counters, (u64)dropped);
}

__device__ __forceinline__ unsigned colour_byte(float c, float wc) {
    if (!(wc > 0.f)) return 0u;
    float t = floorf(c / wc + 0.5f);
    t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
    return (unsigned)(int)t;
}

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const long* __restrict__ keys, long M, const float* __restrict__ depth,
                                                             const unsigned char* __restrict__ valid, const float* __restrict__ weight,
                                                             const unsigned char* __restrict__ rgba, const float* __restrict__ views, int n,
                                                             int H, int W, long pts_per_image, float v, float trunc, float near,
                                                             float* __restrict__ f_out, float* __restrict__ wt_out,
                                                             unsigned char* __restrict__ rgba_out) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float X, Y, Z;
    centre_of((u64)keys[m], v, X, Y, Z);
    const float fW = (float)W, fH = (float)H;
    float D = 0.f, Wt = 0.f, Wc = 0.f, C0 = 0.f, C1 = 0.f, C2 = 0.f;
    for (int j = 0; j < n; ++j) {
        const float* V = views + (long)j * VIEW_FLOATS;
        float xc, yc, zc, u, w_, col, row;
        to_camera(V, X, Y, Z, xc, yc, zc);
        if (!project(V, xc, yc, zc, near, u, w_)) continue;
        if (!pixel_of(u, w_, fW, fH, col, row)) continue;
        const long q = (long)j * pts_per_image + (long)(int)row * W + (int)col;
        if (valid && !valid[q]) continue;
        const float dj = depth[q];
        if (!finite1(dj)) continue;
        const float w = weight ? weight[q] : 1.f;
        if (!(w > 0.f && w < INFINITY)) continue;
        const float sd = dj - zc;
        if (sd < -trunc) continue;                                                  // far behind the surface j sees: no evidence
        const float t = fminf(1.f, sd / trunc);
        D += w * t;
        Wt += w;
        if (rgba && sd <= trunc) {
            const unsigned c = *(const unsigned*)(rgba + q * 4);
            C0 += w * (float)(c & 255u);
            C1 += w * (float)((c >> 8) & 255u);
            C2 += w * (float)((c >> 16) & 255u);
            Wc += w;
        }
    }
    f_out[m] = D / Wt;                                                               // NaN for a voxel nobody saw: not live
    wt_out[m] = Wt;
    if (rgba_out)
        *(unsigned*)(rgba_out + m * 4) = colour_byte(C0, Wc) | (colour_byte(C1, Wc) << 8) | (colour_byte(C2, Wc) << 16) | (255u << 24);
}

// the live neighbours of live voxel m across which f changes sign: nb[a] = the row, or -1
__device__ __forceinline__ int crossings(const long* __restrict__ K, long M, const float* __restrict__ f, const float* __restrict__ wt,
                                         float min_weight, long m, long nb[3]) {
    int count = 0;
    nb[0] = nb[1] = nb[2] = -1;
    const float fm = f[m];
    if (!live(fm, wt[m], min_weight)) return 0;
    const u64 key = (u64)K[m];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long m2 = find_key(K, m + 1, M, key + axis_step(a));
        if (m2 < 0) continue;
        const float f2 = f[m2];
        if (!live(f2, wt[m2], min_weight) || (fm >= 0.f) == (f2 >= 0.f)) continue;
        nb[a] = m2;
        ++count;
    }
    return count;
}

__global__ __launch_bounds__(256) void tsdf_count_kernel(const long* __restrict__ K, long M, const float* __restrict__ f,
                                                         const float* __restrict__ wt, float min_weight, int* __restrict__ counts) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    long nb[3];
    counts[m] = crossings(K, M, f, wt, min_weight, m, nb);
}

__global__ __launch_bounds__(256) void tsdf_write_kernel(const long* __restrict__ K, long M, const float* __restrict__ f,
                                                         const float* __restrict__ wt, const unsigned char* __restrict__ rgba_vox,
                                                         const long* __restrict__ first_row, long P, float v, float min_weight,
                                                         float* __restrict__ pts_out, unsigned char* __restrict__ rgba_out,
                                                         float* __restrict__ weight_out) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    long nb[3];
    if (!crossings(K, M, f, wt, min_weight, m, nb)) return;
    float X[3];
    centre_of((u64)K[m], v, X[0], X[1], X[2]);
    const float fm = f[m], wm = wt[m];
    long row = first_row[m];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long m2 = nb[a];
        if (m2 < 0) continue;
        if (row < 0 || row >= P) return;                                            // not this table's offsets: nothing is written
        const float f2 = f[m2];
        const float at = X[a] + (fm / (fm - f2)) * v;
        pts_out[row * 3] = a == 0 ? at : X[0];
        pts_out[row * 3 + 1] = a == 1 ? at : X[1];
        pts_out[row * 3 + 2] = a == 2 ? at : X[2];
        if (rgba_out) *(unsigned*)(rgba_out + row * 4) = *(const unsigned*)(rgba_vox + (fabsf(f2) < fabsf(fm) ? m2 : m) * 4);
        weight_out[row] = fminf(wm, wt[m2]);
        ++row;
    }
}

bool trunc_ok(int T) { return T >= 1 && T <= MAX_TRUNC; }

int tsdf_table_ok(const char* who, const void* workspace, size_t workspace_bytes, long capacity) {
    return table_ok(who, workspace, workspace_bytes, capacity, geo4d_tsdf_workspace(capacity), "workspace too small (geo4d_tsdf_workspace bytes)");
}

}  // namespace

// the table: capacity 64-bit keys
extern "C" size_t geo4d_tsdf_workspace(long capacity) { return capacity_ok(capacity) ? (size_t)capacity * 8 : 0; }

extern "C" int geo4d_tsdf_mark(const float* pts3d, const float* depth, const unsigned char* valid, const float* centres, int n, int H, int W,
                               float voxel, int trunc, float near, long capacity, long* counters, void* workspace, size_t workspace_bytes,
                               void* stream) {
    const char* who = "tsdf_mark";
    if (!pts3d || !depth || !centres || !counters) return refuse(who, "pts3d, depth, centres and counters [2] are required");
    if (!dims_ok(n, H, W)) return refuse(who, "need n, H, W > 0 and n * H * W < 2^31");
    if (!voxel_ok(voxel)) return refuse(who, "voxel must be finite and > 0");
    if (!trunc_ok(trunc)) return refuse(who, "the truncation must be 1 .. 8 voxels");
    if (!(near >= 0.f)) return refuse(who, "need near >= 0");
    if (int rc = tsdf_table_ok(who, workspace, workspace_bytes, capacity)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(workspace, 0xff, (size_t)capacity * 8, s) != hipSuccess || hipMemsetAsync(counters, 0, 2 * sizeof(long), s) != hipSuccess) {
        geo4d_set_error("tsdf_mark: hipMemsetAsync failed");
        return GEO4D_EIO;
    }
    const long hw = (long)H * W, bpi = (hw + 255) / 256;                            // n * bpi <= n * H * W < 2^31
    hipLaunchKernelGGL(tsdf_mark_kernel, dim3((unsigned)(n * bpi)), dim3(256), 0, s, (u64*)workspace, (u64*)counters, pts3d, depth, valid,
                       centres, hw, (unsigned)bpi, voxel, trunc, near, (u64)capacity);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_tsdf_compact(long capacity, long* keys_out, long max_keys, long* count, const void* workspace, size_t workspace_bytes,
                                  void* stream) {
    const char* who = "tsdf_compact";
    if (!keys_out || !count || max_keys < 0) return refuse(who, "keys_out [max_keys >= 0] and count are required");
    if (int rc = tsdf_table_ok(who, workspace, workspace_bytes, capacity)) return rc;
    return table_compact<false>(who, workspace, capacity, keys_out, nullptr, max_keys, count, (hipStream_t)stream);
}

extern "C" int geo4d_tsdf_integrate(const long* keys, long M, const float* depth, const unsigned char* valid, const float* weight,
                                    const unsigned char* rgba, const float* views, int n, int H, int W, float voxel, int trunc, float near,
                                    float* f_out, float* weight_out, unsigned char* rgba_out, void* stream) {
    const char* who = "tsdf_integrate";
    if (!keys || !depth || !views || !f_out || !weight_out || (rgba_out && !rgba))
        return refuse(who, "keys, depth, views, f_out and weight_out are required, and rgba with rgba_out");
    if (M < 0 || M >= (1L << 31)) return refuse(who, "need 0 <= M < 2^31");
    if (!dims_ok(n, H, W)) return refuse(who, "need n, H, W > 0 and n * H * W < 2^31");
    if (!voxel_ok(voxel)) return refuse(who, "voxel must be finite and > 0");
    if (!trunc_ok(trunc)) return refuse(who, "the truncation must be 1 .. 8 voxels");
    if (!(near >= 0.f)) return refuse(who, "need near >= 0");
    if (M == 0) return GEO4D_OK;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keys, M, depth, valid,
                       weight, rgba_out ? rgba : nullptr, views, n, H, W, (long)H * W, voxel, (float)trunc * voxel, near, f_out, weight_out,
                       rgba_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_tsdf_count(const long* keys, long M, const float* f, const float* weight, float min_weight, int* counts, void* stream) {
    const char* who = "tsdf_count";
    if (!keys || !f || !weight || !counts) return refuse(who, "keys, f, weight and counts are required");
    if (M < 0 || M >= (1L << 31)) return refuse(who, "need 0 <= M < 2^31");
    if (!(min_weight > 0.f)) return refuse(who, "need min_weight > 0");
    if (M == 0) return GEO4D_OK;
    hipLaunchKernelGGL(tsdf_count_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keys, M, f, weight, min_weight,
                       counts);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_tsdf_write(const long* keys, long M, const float* f, const float* weight, const unsigned char* rgba, const long* first_row,
                                long P, float voxel, float min_weight, float* points_out, unsigned char* rgba_out, float* weight_out,
                                void* stream) {
    const char* who = "tsdf_write";
    if (!keys || !f || !weight || !first_row || !points_out || !weight_out || (rgba_out && !rgba))
        return refuse(who, "keys, f, weight, first_row, points_out and weight_out are required, and rgba with rgba_out");
    if (M < 0 || M >= (1L << 31) || P < 0 || P > 3 * M) return refuse(who, "need 0 <= M < 2^31 and 0 <= P <= 3 M");
    if (!voxel_ok(voxel)) return refuse(who, "voxel must be finite and > 0");
    if (!(min_weight > 0.f)) return refuse(who, "need min_weight > 0");
    if (M == 0 || P == 0) return GEO4D_OK;
    hipLaunchKernelGGL(tsdf_write_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keys, M, f, weight, rgba,
                       first_row, P, voxel, min_weight, points_out, rgba_out, weight_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
