// geo4d_amd/csrc/fuse.hip — the aligned scene's points merged into one cloud, one point per occupied voxel (geo4d_amd/fusion.py).
//
// The reference has no such step; nothing is ported. The rule is the project's own and is stated here, in include/geo4d_hip.h and, in
// numpy, in tests/fusion_restatement.py. All float arithmetic is fp32 in the written order with contraction into FMAs switched off,
// as in render.hip; only the final position is fp64.
//
// Which points take part: point i takes part iff mask[i] (when given), X, Y, Z are finite, its weight w (when given; else 1) is finite
//   and > 0, and per axis the cell c = floorf(X / v) satisfies fabsf(c) < 2^20. A point that fails only the last condition is counted
//   in `dropped`; the others are skipped silently, as the renderer skips them.
// Voxel key: (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20), below 2^63; all ones marks an empty slot. Unsigned key order is
//   lexicographic (cx, cy, cz) order, the order of the output.
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
// insert:   keys := all ones, accumulators := 0 (hipMemsetAsync), then one thread per point. The table is open addressing with linear
//           probing from a 64-bit mix of the key, its capacity a power of two >= N. A lane reads the slot's key; on its own key it
//           has found its slot, on an empty slot it tries a 64-bit atomicCAS (which succeeds or shows who won), otherwise it moves on.
//           A lane only ever probes forward and waits for nobody; keys change once, from empty to their value, so a stale read can only
//           cost a CAS. There are never more voxels than taking-part points, so a slot is always found. The sums are integer atomicAdd
//           (atomicMax for best) whose results are not used; all eight of a voxel share one 64-byte line, and for mean a wave issues
//           them line by line (see the kernel).
// compact:  16 slots per thread; the occupied ones go out as (key, slot) pairs behind a device count, one atomicAdd per workgroup
//           (one per wave serialised on the counter: 5.1 ms against 0.11 ms for 2^25 slots); pairs beyond the caller's max_pairs are
//           counted and not written. Slot positions depend on arrival order, so the caller sorts the pairs by key before
// finalize: one thread per output row, in the caller's order of slots.
#include <cmath>
#include "common.h"
#include "geo4d_hip.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr u64 EMPTY = ~0ull;
constexpr int MEAN = 0, BEST = 1;
constexpr int MEAN_WORDS = 8;       // sw, sq[3], sc[3], count
constexpr int BEST_WORDS = 2;       // winner, count
constexpr float CELL_LIMIT = 1048576.f;   // 2^20

__device__ __forceinline__ bool finite3(float a, float b, float c) {
    return fabsf(a) < INFINITY && fabsf(b) < INFINITY && fabsf(c) < INFINITY;      // NaN fails the comparison
}

__device__ __forceinline__ u64 mix64(u64 h) {
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

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
            if (!(fabsf(cx) < CELL_LIMIT && fabsf(cy) < CELL_LIMIT && fabsf(cz) < CELL_LIMIT)) {
                atomicAdd(dropped, 1ull);
            } else {
                const u64 key = ((u64)((int)cx + (1 << 20)) << 42) | ((u64)((int)cy + (1 << 20)) << 21) | (u64)((int)cz + (1 << 20));
                u64 at = mix64(key) & (capacity - 1);
                // a slot is always found within `capacity` steps (see above); the bound only keeps a lane from spinning on a table it
                // did not set up
                for (u64 step = 0; step < capacity; ++step) {
                    u64 seen = __atomic_load_n(keys + at, __ATOMIC_RELAXED);
                    if (seen == EMPTY) {
                        seen = atomicCAS(keys + at, EMPTY, key);
                        if (seen == EMPTY) seen = key;
                    }
                    if (seen == key) {
                        slot = at;
                        break;
                    }
                    at = (at + 1) & (capacity - 1);
                }
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

constexpr int COMPACT_ROUNDS = 16;                                                   // slots per thread: one atomicAdd per 4 096 slots

__global__ __launch_bounds__(256) void fuse_compact_kernel(const u64* __restrict__ keys, u64 capacity, long* __restrict__ key_out,
                                                           long* __restrict__ slot_out, u64 max_pairs, u64* __restrict__ count) {
    __shared__ unsigned wave_sum[4];
    __shared__ u64 base_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 s0 = (u64)blockIdx.x * (256 * COMPACT_ROUNDS) + threadIdx.x;           // round r looks at slot s0 + 256 r
    u64 key[COMPACT_ROUNDS];
    unsigned mine = 0;
#pragma unroll
    for (int r = 0; r < COMPACT_ROUNDS; ++r) {
        const u64 s = s0 + 256 * r;
        key[r] = s < capacity ? keys[s] : EMPTY;
        mine += key[r] != EMPTY;
    }
    unsigned incl = mine;                                                            // inclusive scan inside the wave
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        base_s = total ? atomicAdd(count, (u64)total) : 0;
    }
    __syncthreads();
    u64 pos = base_s + incl - mine;
    for (int k = 0; k < wave; ++k) pos += wave_sum[k];
#pragma unroll
    for (int r = 0; r < COMPACT_ROUNDS; ++r) {
        if (key[r] == EMPTY) continue;
        if (pos < max_pairs) {                                                       // the count still says how many there were
            key_out[pos] = (long)key[r];
            slot_out[pos] = (long)(s0 + 256 * r);
        }
        ++pos;
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
        const int c[3] = {(int)(key >> 42) - (1 << 20), (int)((key >> 21) & 0x1fffffu) - (1 << 20), (int)(key & 0x1fffffu) - (1 << 20)};
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
bool capacity_ok(long capacity) { return capacity >= 1 && capacity <= (1L << 32) && (capacity & (capacity - 1)) == 0; }
size_t acc_words(int reduce) { return reduce == MEAN ? MEAN_WORDS : BEST_WORDS; }

// the checks the three launches share; `who` prefixes the message
int table_ok(const char* who, const void* workspace, size_t workspace_bytes, long capacity, int reduce) {
    char msg[160];
    const char* what = nullptr;
    if (!workspace || (size_t)workspace % 8) what = "an 8-byte aligned workspace is required";
    else if (!capacity_ok(capacity)) what = "capacity must be a power of two, 1 <= capacity <= 2^32";
    else if (!reduce_ok(reduce)) what = "unknown reduce (0 mean, 1 best)";
    else if (workspace_bytes < geo4d_fuse_workspace(capacity, reduce)) what = "workspace too small (geo4d_fuse_workspace bytes)";
    if (!what) return GEO4D_OK;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    geo4d_set_error(msg);
    return GEO4D_EINVAL;
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
    if (!points || !dropped) {
        geo4d_set_error("fuse_insert: points and dropped are required");
        return GEO4D_EINVAL;
    }
    if (N < 0 || N >= (1L << 31)) {
        geo4d_set_error("fuse_insert: need 0 <= N < 2^31");
        return GEO4D_EINVAL;
    }
    if (!(voxel > 0.f && voxel < INFINITY)) {
        geo4d_set_error("fuse_insert: voxel must be finite and > 0");
        return GEO4D_EINVAL;
    }
    if (int rc = table_ok("fuse_insert", workspace, workspace_bytes, capacity, reduce)) return rc;
    if (capacity < N) {
        geo4d_set_error("fuse_insert: capacity must be >= N (there can be as many voxels as points)");
        return GEO4D_EINVAL;
    }
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
    if (!keys_out || !slots_out || !count || max_pairs < 0) {
        geo4d_set_error("fuse_compact: keys_out, slots_out [max_pairs >= 0] and count are required");
        return GEO4D_EINVAL;
    }
    if (int rc = table_ok("fuse_compact", workspace, workspace_bytes, capacity, reduce)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, sizeof(long), s) != hipSuccess) {
        geo4d_set_error("fuse_compact: hipMemsetAsync failed");
        return GEO4D_EIO;
    }
    hipLaunchKernelGGL(fuse_compact_kernel, dim3((unsigned)((capacity + 256 * COMPACT_ROUNDS - 1) / (256 * COMPACT_ROUNDS))), dim3(256), 0, s,
                       (const u64*)workspace, (u64)capacity, keys_out, slots_out, (u64)max_pairs, (u64*)count);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_fuse_finalize(const long* order, long M, const float* points, const unsigned char* rgba, const float* weight, long N,
                                   float voxel, int reduce, long capacity, float* points_out, unsigned char* rgba_out, float* weight_out,
                                   int* count_out, const void* workspace, size_t workspace_bytes, void* stream) {
    if (!order || !points || !points_out || !weight_out || !count_out || (rgba_out && !rgba)) {
        geo4d_set_error("fuse_finalize: order, points, points_out, weight_out and count_out are required, and rgba with rgba_out");
        return GEO4D_EINVAL;
    }
    if (N < 0 || N >= (1L << 31) || M < 0 || M > N) {
        geo4d_set_error("fuse_finalize: need 0 <= M <= N < 2^31");
        return GEO4D_EINVAL;
    }
    if (!(voxel > 0.f && voxel < INFINITY)) {
        geo4d_set_error("fuse_finalize: voxel must be finite and > 0");
        return GEO4D_EINVAL;
    }
    if (int rc = table_ok("fuse_finalize", workspace, workspace_bytes, capacity, reduce)) return rc;
    if (capacity < N) {
        geo4d_set_error("fuse_finalize: capacity must be >= N (there can be as many voxels as points)");
        return GEO4D_EINVAL;
    }
    if (M == 0) return GEO4D_OK;
    const u64* keys = (const u64*)workspace;
    hipLaunchKernelGGL(fuse_finalize_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keys, keys + capacity,
                       order, M, (u64)capacity, points, rgba, weight, N, voxel, reduce, points_out, rgba_out, weight_out, count_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
