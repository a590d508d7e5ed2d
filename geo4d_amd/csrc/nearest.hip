// geo4d_amd/csrc/nearest.hip — for every query point, the nearest reference point within a radius and the number of reference points
// within it, on a grid of cells of side radius (geo4d_amd/nearest.py): what the cloud metrics of geo4d_amd/evaluation.py and the radius
// outlier removal of geo4d_amd/fusion.py stand on.
//
// The reference has no such step; nothing is ported. The rule is the project's own and is stated here, in include/geo4d_hip.h and, in
// numpy, in tests/nearest_restatement.py. All float arithmetic is fp32 in the written order with contraction into FMAs switched off,
// only + - * / and floorf, each correctly rounded: numpy float32 rounds where the kernels do, and no comparison has a tolerance.
//
// Inputs: reference fp32 [Nr][3] with reference_mask u8 [Nr] (NULL: every row), query fp32 [Nq][3] with query_mask likewise, the radius
//   r > 0 with r2 = r * r finite in fp32, exclude_same_row (0 / 1); Nr, Nq < 2^31.
// 1. Cells: the cell side is r; a point's cell is c_a = floorf(X_a / r); cell_ok and the key are voxel_table.h's: fabsf(c_a) < 2^20 on
//    every axis, key = (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20), unsigned key order = lexicographic (cx, cy, cz) order.
// 2. Who takes part: a point (reference or query) takes part iff its mask is set, its coordinates are finite and cell_ok holds. A point
//    that fails only cell_ok is counted in `dropped`; the others are skipped silently. A query that takes no part gets index = -1,
//    dist2 = +inf, count = 0.
// 3. Candidates of query i: the taking-part reference rows j whose integer cell differs from the query's by at most 1 on every axis,
//    without j = i when exclude_same_row. Cells outside the grid (|c| >= 2^20) do not exist and are skipped: the neighbour cells are
//    formed as integers and tested against the limit before a key is made of them, never by adding to a key, so no carry between the
//    key's fields can reach a cell at the other end of the grid.
// 4. Distance: dx = Qx - Rx, likewise dy, dz; d2 = (dx dx + dy dy) + dz dz; j is within iff d2 <= r2.
// 5. Per query: count int32 = the number of candidates within; index int32 = the within candidate with the smallest (d2, j) in
//    lexicographic order (the lowest original row wins on ties), or -1; dist2 fp32 = its d2, or +inf.
// 6. Every output is a minimum or an integer count over a set: it depends neither on the order the candidates are visited in, nor on
//    how the queries are spread over lanes, nor on the run. Permuting the reference rows leaves dist2 and count unchanged.
// 7. Against the cell-free definition ("every taking-part reference with d2 <= r2"): a point within r lies at most one cell away on
//    every axis in exact arithmetic; floorf(X / r) rounds, so the two can differ only where some reference is within rounding of r
//    from the query. tests/test_nearest_cpu.py measures it (0 of 3 000 queries in six runs).
//
// keys:    one thread per point: the key of a taking-part point, all ones for any other. All ones is after every real key in the
//          unsigned order the keys are defined in (a real key is below 2^63); the caller's sort is signed, there it comes first, and
//          the caller takes the other end. `dropped` := 0 (hipMemsetAsync), then one integer atomicAdd per workgroup that has any.
// grid:    the caller's plumbing between launches (a stable sort of the keys, the unique keys and the prefix sum of their counts) gives
//          cell_keys int64 [M] sorted and unique and cell_start int32 [M + 1]; gather: one thread per taking-part point k in (key, row)
//          order writes ref_sorted[k] = reference[order[k]] and ref_row[k] = order[k]. An order entry outside [0, Nr) gives the row -1
//          and NaN coordinates, which no query can match.
// query:   the queries are sorted by their own key (the caller's plumbing), so the lanes of a wave look at the same cells and their
//          loads hit the same lines. One thread per sorted query. The cells (cz - 1, cz, cz + 1) of a column (cx + i, cy + j) are
//          consecutive in key order, so one lower-bound search per column (nine in all) finds the first of them, and the points of the
//          at most three cells that exist are one contiguous range of ref_sorted. Results go to the query's original row; the sorted
//          positions from Nq_taking on get index -1, dist2 +inf, count 0. The consumer trusts nothing it is handed: a cell_start outside
//          [0, Nt] or a ref_row outside [0, Nr) is skipped and never dereferenced, a query_order entry outside [0, Nq) writes nothing.
// Termination: every loop is counted. The column loops run 3 x 3 times; the lower bound halves hi - lo <= M < 2^31 and ends within 32
//   turns; the scan for the end of the column looks at no more than 3 cells; the walk runs over p in [first, last) with 0 <= first <=
//   last <= Nt. No thread waits for another, and the only atomic is the integer add on `dropped`.
#include <cmath>
#include <initializer_list>
#include "common.h"
#include "geo4d_hip.h"
#include "tsdf_field.h"                                                              // u64, EMPTY, key_of, cell_ok, finite3, refuse

#pragma clang fp contract(off)

namespace {

constexpr int CELL_MAX = (1 << 20) - 1;                                              // the outermost cell on an axis

// `dropped` gets one add per workgroup, as table_compact_kernel's count does
__global__ __launch_bounds__(256) void nn_keys_kernel(const float* __restrict__ points, const unsigned char* __restrict__ mask, long N, float r,
                                                      u64* __restrict__ keys_out, u64* __restrict__ dropped) {
    __shared__ unsigned wave_sum[4];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned out = 0;
    if (i < N) {
        u64 key = EMPTY;
        if (!mask || mask[i]) {
            const float X = points[i * 3], Y = points[i * 3 + 1], Z = points[i * 3 + 2];
            if (finite3(X, Y, Z)) {
                const float cx = floorf(X / r), cy = floorf(Y / r), cz = floorf(Z / r);
                if (cell_ok(cx, cy, cz)) key = key_of(cx, cy, cz);
                else out = 1;
            }
        }
        keys_out[i] = key;
    }
    for (int o = 32; o > 0; o >>= 1) out += __shfl_down(out, o);                     // 6 turns: the wave's sum in lane 0
    if (lane == 0) wave_sum[wave] = out;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        if (total) atomicAdd(dropped, (u64)total);
    }
}

__global__ __launch_bounds__(256) void nn_gather_kernel(const float* __restrict__ points, const long* __restrict__ order, long Nt, long N,
                                                        float* __restrict__ sorted_out, int* __restrict__ row_out) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= Nt) return;
    const long i = order[k];
    const bool ok = i >= 0 && i < N;
    sorted_out[k * 3] = ok ? points[i * 3] : NAN;
    sorted_out[k * 3 + 1] = ok ? points[i * 3 + 1] : NAN;
    sorted_out[k * 3 + 2] = ok ? points[i * 3 + 2] : NAN;
    row_out[k] = ok ? (int)i : -1;
}

// the first row of K[0..M) whose key is not below `target` (M when there is none); unsigned order, as find_key's
__device__ __forceinline__ long lower_bound(const long* __restrict__ K, long M, u64 target) {
    long lo = 0, hi = M;
    while (lo < hi) {                                                                // hi - lo at least halves: within 32 turns for M < 2^31
        const long mid = lo + ((hi - lo) >> 1);
        if ((u64)K[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ u64 key_of_cell(int cx, int cy, int cz) {
    return ((u64)(cx + (1 << 20)) << 42) | ((u64)(cy + (1 << 20)) << 21) | (u64)(cz + (1 << 20));
}

__global__ __launch_bounds__(256) void nn_query_kernel(const float* __restrict__ query, const long* __restrict__ query_order, long Nq_taking,
                                                       long Nq, const long* __restrict__ cell_keys, const int* __restrict__ cell_start, long M,
                                                       const float* __restrict__ ref_sorted, const int* __restrict__ ref_row, long Nt, long Nr,
                                                       float r, int exclude_same_row, int* __restrict__ index_out,
                                                       float* __restrict__ dist2_out, int* __restrict__ count_out) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= Nq) return;
    const long row = query_order[k];
    if (row < 0 || row >= Nq) return;                                                // not a row of the outputs: nothing is written
    int best = -1, count = 0;
    float best_d2 = INFINITY;
    const float Qx = query[row * 3], Qy = query[row * 3 + 1], Qz = query[row * 3 + 2];
    const float fx = floorf(Qx / r), fy = floorf(Qy / r), fz = floorf(Qz / r);
    if (k < Nq_taking && finite3(Qx, Qy, Qz) && cell_ok(fx, fy, fz)) {
        const float r2 = r * r;
        const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
        const int z0 = cz - 1 < -CELL_MAX ? -CELL_MAX : cz - 1, z1 = cz + 1 > CELL_MAX ? CELL_MAX : cz + 1;   // the cells of the column that exist
        for (int a = -1; a <= 1; ++a) {                                              // 3 x 3 columns
            for (int b = -1; b <= 1; ++b) {
                const int X = cx + a, Y = cy + b;
                if (X < -CELL_MAX || X > CELL_MAX || Y < -CELL_MAX || Y > CELL_MAX) continue;   // no such column
                const u64 last_key = key_of_cell(X, Y, z1);
                const long c0 = lower_bound(cell_keys, M, key_of_cell(X, Y, z0));
                long c1 = c0;                                                        // at most three cells lie in [key(z0), key(z1)]
                for (int t = 0; t < 3 && c1 < M && (u64)cell_keys[c1] <= last_key; ++t) ++c1;
                if (c1 == c0) continue;
                const long first = cell_start[c0], last = cell_start[c1];
                if (first < 0 || last > Nt || first > last) continue;               // not a range of ref_sorted: skipped
                for (long p = first; p < last; ++p) {                                // last - first <= Nt turns
                    const int j = ref_row[p];
                    if (j < 0 || (long)j >= Nr || (exclude_same_row && (long)j == row)) continue;
                    const float dx = Qx - ref_sorted[p * 3], dy = Qy - ref_sorted[p * 3 + 1], dz = Qz - ref_sorted[p * 3 + 2];
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(d2 <= r2)) continue;                                       // NaN is not within
                    ++count;
                    if (d2 < best_d2 || (d2 == best_d2 && j < best)) {
                        best_d2 = d2;
                        best = j;
                    }
                }
            }
        }
    }
    index_out[row] = best;
    dist2_out[row] = best_d2;
    count_out[row] = count;
}

bool size_ok(long n) { return n >= 0 && n < (1L << 31); }
// finite, > 0 and with a finite square in fp32
bool radius_ok(float r) {
    const float r2 = r * r;
    return r > 0.f && r < INFINITY && r2 < INFINITY;
}
const char* const RADIUS = "radius must be finite and > 0, and so must its square in fp32";
unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }
// p is one of `others` (a null pointer is no buffer and aliases nothing)
bool among(const void* p, std::initializer_list<const void*> others) {
    for (const void* o : others)
        if (p && p == o) return true;
    return false;
}

}  // namespace

extern "C" int geo4d_nn_keys(const float* points, const unsigned char* mask, long N, float radius, long* keys_out, long* dropped,
                             void* stream) {
    const char* who = "nn_keys";
    if (!size_ok(N)) return refuse(who, "need 0 <= N < 2^31");
    if (!radius_ok(radius)) return refuse(who, RADIUS);
    if (!dropped || (N > 0 && (!points || !keys_out))) return refuse(who, "points, keys_out (unless N = 0) and dropped are required");
    if (among(keys_out, {points, mask, dropped}) || among(dropped, {points, mask}))
        return refuse(who, "keys_out and dropped must be buffers of their own");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(dropped, 0, sizeof(long), s) != hipSuccess) {
        geo4d_set_error("nn_keys: hipMemsetAsync failed");
        return GEO4D_EIO;
    }
    if (N == 0) return GEO4D_OK;
    hipLaunchKernelGGL(nn_keys_kernel, dim3(blocks_of(N)), dim3(256), 0, s, points, mask, N, radius, (u64*)keys_out, (u64*)dropped);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_nn_gather(const float* points, const long* order, long Nt, long N, float* sorted_out, int* row_out, void* stream) {
    const char* who = "nn_gather";
    if (!size_ok(N) || Nt < 0 || Nt > N) return refuse(who, "need 0 <= Nt <= N < 2^31");
    if (Nt > 0 && (!points || !order || !sorted_out || !row_out)) return refuse(who, "points, order, sorted_out and row_out are required");
    if (Nt > 0 && (among(sorted_out, {points, order, row_out}) || among(row_out, {points, order})))
        return refuse(who, "sorted_out and row_out must be buffers of their own");
    if (Nt == 0) return GEO4D_OK;
    hipLaunchKernelGGL(nn_gather_kernel, dim3(blocks_of(Nt)), dim3(256), 0, (hipStream_t)stream, points, order, Nt, N, sorted_out, row_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_nn_query(const float* query, const long* query_order, long Nq_taking, long Nq, const long* cell_keys,
                              const int* cell_start, long M, const float* ref_sorted, const int* ref_row, long Nt, long Nr, float radius,
                              int exclude_same_row, int* index_out, float* dist2_out, int* count_out, void* stream) {
    const char* who = "nn_query";
    if (!size_ok(Nq) || Nq_taking < 0 || Nq_taking > Nq) return refuse(who, "need 0 <= Nq_taking <= Nq < 2^31");
    if (!size_ok(Nr) || M < 0 || M > Nt || Nt > Nr) return refuse(who, "need 0 <= M <= Nt <= Nr < 2^31");
    if (!radius_ok(radius)) return refuse(who, RADIUS);
    if (exclude_same_row != 0 && exclude_same_row != 1) return refuse(who, "exclude_same_row must be 0 or 1");
    if (Nq > 0 && (!query || !query_order || !index_out || !dist2_out || !count_out))
        return refuse(who, "query, query_order, index_out, dist2_out and count_out are required");
    if (!cell_start || (M > 0 && !cell_keys) || (Nt > 0 && (!ref_sorted || !ref_row)))
        return refuse(who, "cell_start, cell_keys (unless M = 0), ref_sorted and ref_row (unless Nt = 0) are required");
    if (Nq > 0) {
        for (const void* o : {(const void*)index_out, (const void*)dist2_out, (const void*)count_out})
            if (among(o, {query, query_order, cell_keys, cell_start, ref_sorted, ref_row})) return refuse(who, "an output must not be an input");
        if (among(index_out, {dist2_out, count_out}) || among(dist2_out, {count_out})) return refuse(who, "the three outputs must be three buffers");
    }
    if (Nq == 0) return GEO4D_OK;
    hipLaunchKernelGGL(nn_query_kernel, dim3(blocks_of(Nq)), dim3(256), 0, (hipStream_t)stream, query, query_order, Nq_taking, Nq, cell_keys,
                       cell_start, M, ref_sorted, ref_row, Nt, Nr, radius, exclude_same_row, index_out, dist2_out, count_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
