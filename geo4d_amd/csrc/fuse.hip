// geo4d_amd/csrc/fuse.hip — the aligned scene's points merged into one cloud, one point per occupied voxel (geo4d_amd/fusion.py).
//
// The reference has no such step; nothing is ported. The rule is the project's own and is stated here, in include/geo4d_hip.h and, in
// numpy, in tests/fusion_restatement.py. All float arithmetic is fp32 in the written order with contraction into FMAs switched off,
// as in render.hip; only the final position is fp64.
//
// Which points take part: point i takes part iff mask[i] (when given), X, Y, Z are finite, its weight w (when given; else 1) is finite
//   and > 0, and per axis the cell c = floorf(X / v) satisfies fabsf(c) < 2^20. A point that fails only the last condition is counted
//   in `dropped`; the others are skipped silently, as the renderer skips them.
// Voxel key (voxel_table.h): (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20), below 2^63; all ones marks an empty slot. Unsigned
//   key order is lexicographic (cx, cy, cz) order, the order of the output.
// Per point: offset q_a = (int)clamp(floorf((X_a - c_a v) / v * 65536.f + 0.5f), 0.f, 65535.f) (clamped as a float, then cast),
//   weight wq = (int)clamp(floorf(w * 128.f + 0.5f), 1.f, 32767.f).
// Per voxel, integer sums: count, sw = sum wq, sq_a = sum wq q_a, sc_k = sum wq rgba_k (k = 0..2), u64 each. N < 2^31, wq < 2^15 and
//   q < 2^16, so no sum can overflow; integer addition is associative, so the sums do not depend on the order the points arrive in.
//   That is why the accumulators are fixed point and not float atomics.
// reduce = mean: pos_a = (float)(((double)c_a + (double)sq_a / ((double)sw * 65536.0)) * (double)v); colour (sc_k + sw / 2) / sw in
//   integers, alpha 255; weight (float)((double)sw / (128.0 * count)).
// reduce = best: the voxel's point is the input point of highest weight, the lowest row on ties: the unsigned 64-bit maximum of
//   float_bits(w) << 32 | (0xffffffff - i), the way the splat takes a minimum. Position, colour and weight are copied bit for bit;
//   count is still the voxel's count.
//
// insert:   keys := all ones, accumulators := 0 (hipMemsetAsync), then one thread per point. The table is voxel_table.h's: open
//           addressing with linear probing from a 64-bit mix of the key, a 64-bit atomicCAS only on an empty slot, forward probing, no
//           lane waits for another; its capacity is a power of two >= N. There are never more voxels than taking-part points, so a slot
//           is always found. The sums are integer atomicAdd (atomicMax for best) whose results are not used; all eight of a voxel share
//           one 64-byte line, and for mean a wave issues them line by line (see the kernel).
// compact:  voxel_table.h's: 16 slots per thread; the occupied ones go out as (key, slot) pairs behind a device count, one atomicAdd
//           per workgroup; pairs beyond the caller's max_pairs are counted and not written. Slot positions depend on arrival order, so
//           the caller sorts the pairs by key before
// finalize: one thread per output row, in the caller's order of slots.
#include <cmath>
#include "common.h"
#include "geo4d_hip.h"
#include "voxel_table.h"                                                             // u64, the key, the table and its checks, refuse

#pragma clang fp contract(off)

namespace {

constexpr int MEAN = 0, BEST = 1;
constexpr int MEAN_WORDS = 8;       // sw, sq[3], sc[3], count
constexpr int BEST_WORDS = 2;       // winner, count

__device__ __forceinline__ u64 offset_q(float X, float c, float v) {
    float t = (X - c * v) / v * 65536.f + 0.5f;
    t = floorf(t);
    t = t < 0.f ? 0.f : (t > 65535.f ? 65535.f : t);
    return (u64)(int)t;
}

// WORDS = the slot's accumulator words (MEAN_WORDS / BEST_WORDS). GROUPED (mean): the lanes of a wave hand their words over through LDS,
// so that one atomic instruction covers 8 points with the 8 consecutive words of each (whole 64-byte lines) instead of one word of 64
// scattered slots; the adds and their operands are the same, only the lane that issues each differs. Measured on the 64-image scene
// (profiles/fusion.md): insert 4.15 -> 0.92 ms for mean; for best (16-byte runs) it made no difference and is not used.
template <int WORDS>
__global__ __launch_bounds__(256) void fuse_insert_kernel(u64* __restrict__ keys, u64* __restrict__ acc, u64* __restrict__ dropped,
                                                          const float* __restrict__ points, const unsigned char* __restrict__ rgba,
                                                          const float* __restrict__ weight, const unsigned char* __restrict__ mask,
                                                          long N, float v, u64 capacity) {
    constexpr bool GROUPED = WORDS == MEAN_WORDS;
    __shared__ u64 word_s[GROUPED ? 256 * WORDS : 1];
    __shared__ u64 slot_s[GROUPED ? 256 : 1];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    u64 slot = EMPTY;                                                                // EMPTY: this lane has nothing to add
    u64 val[WORDS] = {};
    if (i < N && (!mask || mask[i])) {
        const float X = points[i * 3], Y = points[i * 3 + 1], Z = points[i * 3 + 2];
        const float w = weight ? weight[i] : 1.f;
        if (finite3(X, Y, Z) && w > 0.f && w < INFINITY) {
            const float cx = floorf(X / v), cy = floorf(Y / v), cz = floorf(Z / v);
            if (!cell_ok(cx, cy, cz)) {
                atomicAdd(dropped, 1ull);
            } else {
                slot = claim_slot(keys, capacity, key_of(cx, cy, cz), nullptr);      // always found (see above)
                if (WORDS == MEAN_WORDS) {
                    float t = floorf(w * 128.f + 0.5f);
                    t = t < 1.f ? 1.f : (t > 32767.f ? 32767.f : t);
                    const u64 wq = (u64)(int)t;
                    const unsigned c = rgba ? *(const unsigned*)(rgba + i * 4) : 0u;
                    val[0] = wq;
                    val[1] = wq * offset_q(X, cx, v);
                    val[2] = wq * offset_q(Y, cy, v);
                    val[3] = wq * offset_q(Z, cz, v);
                    val[4 % WORDS] = wq * (u64)(c & 255u);
                    val[5 % WORDS] = wq * (u64)((c >> 8) & 255u);
                    val[6 % WORDS] = wq * (u64)((c >> 16) & 255u);
                    val[7 % WORDS] = 1ull;
                } else {
                    val[0] = ((u64)__float_as_uint(w) << 32) | (u64)(0xffffffffu - (unsigned)i);
                    val[1] = 1ull;
                }
            }
        }
    }
    // word 0 of BEST is a maximum, every other word a sum; adding 0 changes nothing and is left out
    if (GROUPED) {
        const int first = threadIdx.x & ~63, lane = threadIdx.x & 63;                // this wave's part of the two arrays
#pragma unroll
        for (int k = 0; k < WORDS; ++k) word_s[threadIdx.x * WORDS + k] = val[k];
        slot_s[threadIdx.x] = slot;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < WORDS; ++r) {
            const int idx = 64 * r + lane, src = idx / WORDS, k = idx % WORDS;
            const u64 to = slot_s[first + src], x = word_s[first * WORDS + idx];
            if (to == EMPTY || x == 0) continue;
            atomicAdd(acc + to * WORDS + k, x);
        }
    } else if (slot != EMPTY) {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) {
            if (val[k] == 0) continue;
            if (WORDS == BEST_WORDS && k == 0) atomicMax(acc + slot * WORDS, val[k]);
            else atomicAdd(acc + slot * WORDS + k, val[k]);
        }
    }
}

__global__ __launch_bounds__(256) void fuse_finalize_kernel(const u64* __restrict__ keys, const u64* __restrict__ acc,
                                                            const long* __restrict__ order, long M, u64 capacity,
                                                            const float* __restrict__ points, const unsigned char* __restrict__ rgba,
                                                            const float* __restrict__ weight, long N, float v, int reduce,
                                                            float* __restrict__ pts_out, unsigned char* __restrict__ rgba_out,
                                                            float* __restrict__ weight_out, int* __restrict__ count_out) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const u64 slot = (u64)order[m];
    if (slot >= capacity) return;                                                    // not a slot of this table: the row is left as it is
    if (reduce == MEAN) {
        const u64 key = keys[slot];
        const u64* a = acc + slot * MEAN_WORDS;
        const u64 sw = a[0], n = a[7];
        if (key == EMPTY || sw == 0) return;                                         // an empty slot: likewise
        const double dv = (double)v, den = (double)sw * 65536.0;
        int c[3];
        cell_of(key, c);
        for (int k = 0; k < 3; ++k) pts_out[m * 3 + k] = (float)(((double)c[k] + (double)a[1 + k] / den) * dv);
        if (rgba_out)
            *(unsigned*)(rgba_out + m * 4) = (unsigned)((a[4] + sw / 2) / sw) | ((unsigned)((a[5] + sw / 2) / sw) << 8) |
                                             ((unsigned)((a[6] + sw / 2) / sw) << 16) | (255u << 24);
        weight_out[m] = (float)((double)sw / (128.0 * (double)n));
        count_out[m] = (int)n;
    } else {
        const u64* a = acc + slot * BEST_WORDS;
        const long i = (long)(0xffffffffu - (unsigned)a[0]);
        if (a[1] == 0 || i >= N) return;
        for (int k = 0; k < 3; ++k) pts_out[m * 3 + k] = points[i * 3 + k];
        if (rgba_out) *(unsigned*)(rgba_out + m * 4) = *(const unsigned*)(rgba + i * 4);
        weight_out[m] = weight ? weight[i] : 1.f;
        count_out[m] = (int)a[1];
    }
}

bool reduce_ok(int reduce) { return reduce == MEAN || reduce == BEST; }
size_t acc_words(int reduce) { return reduce == MEAN ? MEAN_WORDS : BEST_WORDS; }

// the checks the three launches share. An unknown reduce makes geo4d_fuse_workspace 0, so it passes the table's last check and is
// refused right after it: the refusals come in the order workspace, capacity, reduce, bytes.
int fuse_table_ok(const char* who, const void* workspace, size_t workspace_bytes, long capacity, int reduce) {
    if (int rc = table_ok(who, workspace, workspace_bytes, capacity, geo4d_fuse_workspace(capacity, reduce),
                          "workspace too small (geo4d_fuse_workspace bytes)"))
        return rc;
    return reduce_ok(reduce) ? GEO4D_OK : refuse(who, "unknown reduce (0 mean, 1 best)");
}

}  // namespace

// the table: capacity keys, then capacity x (8 words for mean, 2 for best) of accumulators
extern "C" size_t geo4d_fuse_workspace(long capacity, int reduce) {
    if (!capacity_ok(capacity) || !reduce_ok(reduce)) return 0;
    return (size_t)capacity * 8 * (1 + acc_words(reduce));
}

extern "C" int geo4d_fuse_insert(const float* points, const unsigned char* rgba, const float* weight, const unsigned char* mask, long N,
                                 float voxel, int reduce, long capacity, long* dropped, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    const char* who = "fuse_insert";
    if (!points || !dropped) return refuse(who, "points and dropped are required");
    if (N < 0 || N >= (1L << 31)) return refuse(who, "need 0 <= N < 2^31");
    if (!voxel_ok(voxel)) return refuse(who, "voxel must be finite and > 0");
    if (int rc = fuse_table_ok(who, workspace, workspace_bytes, capacity, reduce)) return rc;
    if (capacity < N) return refuse(who, "capacity must be >= N (there can be as many voxels as points)");
    hipStream_t s = (hipStream_t)stream;
    u64* keys = (u64*)workspace;
    if (hipMemsetAsync(keys, 0xff, (size_t)capacity * 8, s) != hipSuccess ||
        hipMemsetAsync(keys + capacity, 0, (size_t)capacity * 8 * acc_words(reduce), s) != hipSuccess ||
        hipMemsetAsync(dropped, 0, sizeof(long), s) != hipSuccess) {
        geo4d_set_error("fuse_insert: hipMemsetAsync failed");
        return GEO4D_EIO;
    }
    if (N == 0) return GEO4D_OK;
    const dim3 grid((unsigned)((N + 255) / 256));
    if (reduce == MEAN)
        hipLaunchKernelGGL(fuse_insert_kernel<MEAN_WORDS>, grid, dim3(256), 0, s, keys, keys + capacity, (u64*)dropped, points, rgba, weight,
                           mask, N, voxel, (u64)capacity);
    else
        hipLaunchKernelGGL(fuse_insert_kernel<BEST_WORDS>, grid, dim3(256), 0, s, keys, keys + capacity, (u64*)dropped, points, rgba, weight,
                           mask, N, voxel, (u64)capacity);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_fuse_compact(long capacity, int reduce, long* keys_out, long* slots_out, long max_pairs, long* count, const void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const char* who = "fuse_compact";
    if (!keys_out || !slots_out || !count || max_pairs < 0) return refuse(who, "keys_out, slots_out [max_pairs >= 0] and count are required");
    if (int rc = fuse_table_ok(who, workspace, workspace_bytes, capacity, reduce)) return rc;
    return table_compact<true>(who, workspace, capacity, keys_out, slots_out, max_pairs, count, (hipStream_t)stream);
}

extern "C" int geo4d_fuse_finalize(const long* order, long M, const float* points, const unsigned char* rgba, const float* weight, long N,
                                   float voxel, int reduce, long capacity, float* points_out, unsigned char* rgba_out, float* weight_out,
                                   int* count_out, const void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "fuse_finalize";
    if (!order || !points || !points_out || !weight_out || !count_out || (rgba_out && !rgba))
        return refuse(who, "order, points, points_out, weight_out and count_out are required, and rgba with rgba_out");
    if (N < 0 || N >= (1L << 31) || M < 0 || M > N) return refuse(who, "need 0 <= M <= N < 2^31");
    if (!voxel_ok(voxel)) return refuse(who, "voxel must be finite and > 0");
    if (int rc = fuse_table_ok(who, workspace, workspace_bytes, capacity, reduce)) return rc;
    if (capacity < N) return refuse(who, "capacity must be >= N (there can be as many voxels as points)");
    if (M == 0) return GEO4D_OK;
    const u64* keys = (const u64*)workspace;
    hipLaunchKernelGGL(fuse_finalize_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keys, keys + capacity,
                       order, M, (u64)capacity, points, rgba, weight, N, voxel, reduce, points_out, rgba_out, weight_out, count_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
