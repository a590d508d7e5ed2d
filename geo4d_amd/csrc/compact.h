// geo4d_amd/csrc/compact.h — the scan step of the order-preserving compactions (depth_eval.hip masked_select, scene_export.hip points /
// mesh faces). A compaction is three launches: per-tile counts of the kept elements, this exclusive scan of the counts (the start of
// every tile's output range), a scatter in which each element's rank inside its tile is a ballot popcount. No atomics: the output
// order is the input order, whatever the schedule.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// exclusive scan of block_count in place (one workgroup of 1024 lanes walking the array), total -> *count
__global__ __launch_bounds__(1024) void compact_scan_kernel(unsigned* __restrict__ block_count, long nblocks, long* __restrict__ count) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned long long carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (long b0 = 0; b0 < nblocks; b0 += 1024) {
        const long b = b0 + tid;
        const unsigned v = b < nblocks ? block_count[b] : 0u;
        unsigned incl = v;                                          // inclusive scan inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_up(incl, o);
            if (lane >= o) incl += u;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned before = 0;
        for (int k = 0; k < wave; ++k) before += wsum[k];
        const unsigned long long carry = carry_s;
        if (b < nblocks) block_count[b] = (unsigned)(carry + before + incl - v);
        __syncthreads();
        if (tid == 1023) carry_s = carry + before + incl;
        __syncthreads();
    }
    if (tid == 0) *count = (long)carry_s;
}

// Generic form of the count and scatter steps for a kept-element rule `op.keep(e)` and a writer `op.emit(e, pos)`: a tile is
// COMPACT_ROUNDS rounds of 256 consecutive elements per workgroup, so an element's rank inside its tile is a ballot popcount.
constexpr int COMPACT_ROUNDS = 16;
constexpr long COMPACT_TILE = 256L * COMPACT_ROUNDS;

inline long compact_tiles(long n) { return (n + COMPACT_TILE - 1) / COMPACT_TILE; }

template <class Op>
__global__ __launch_bounds__(256) void compact_count_kernel(Op op, long n, unsigned* __restrict__ block_count) {
    __shared__ unsigned red[4];
    const long base = (long)blockIdx.x * COMPACT_TILE;
    unsigned c = 0;
    for (int r = 0; r < COMPACT_ROUNDS; ++r) {
        const long e = base + r * 256 + threadIdx.x;
        if (e < n && op.keep(e)) ++c;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

template <class Op>
__global__ __launch_bounds__(256) void compact_scatter_kernel(Op op, long n, const unsigned* __restrict__ block_offset) {
    __shared__ unsigned wcount[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * COMPACT_TILE;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned off = block_offset[blockIdx.x];
    for (int r = 0; r < COMPACT_ROUNDS; ++r) {
        const long e = base + r * 256 + threadIdx.x;
        const bool v = e < n && op.keep(e);
        const unsigned long long bal = __ballot(v);
        if (lane == 0) wcount[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned pos = off + (unsigned)__popcll(bal & below);
        for (int k = 0; k < wave; ++k) pos += wcount[k];
        if (v) op.emit(e, pos);
        off += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
}

}  // namespace
