// geo4d_amd/csrc/voxel_table.h — the voxel key and the hash table of keys that fuse.hip and tsdf.hip fill, and that tsdf_field.h's
// readers take apart again.
//
// Voxel key: the cell c_a = floorf(X_a / v) takes part iff fabsf(c_a) < 2^20 on every axis; its key is (cx + 2^20) << 42 |
//   (cy + 2^20) << 21 | (cz + 2^20), below 2^63. A field of a real cell holds 1 .. 2^21 - 1, unsigned key order is lexicographic
//   (cx, cy, cz) order, and all ones marks an empty slot.
// Table: `capacity` 64-bit keys, a power of two, set to all ones by the host. Open addressing with linear probing from a 64-bit mix of
//   the key. A lane reads the slot's key; on its own key it has found its slot, on an empty slot it tries a 64-bit atomicCAS (which
//   succeeds or shows who won), otherwise it moves on. A lane only ever probes forward and waits for nobody; keys change once, from
//   empty to their value, so a stale read can only cost a CAS.
// Compaction: 16 slots per thread; the occupied ones go out as keys, or (key, slot) pairs, behind a device count, one atomicAdd per
//   workgroup (one per wave serialised on the counter: 5.1 ms against 0.11 ms for 2^25 slots); rows beyond the caller's limit are
//   counted and not written. Positions depend on arrival order, so the caller sorts by key.
#pragma once
#include "scene_view.h"                                                              // u64, refuse

#pragma clang fp contract(off)

namespace {

constexpr u64 EMPTY = ~0ull;
constexpr float CELL_LIMIT = 1048576.f;   // 2^20
constexpr int GIVE_UP_EVERY = 256;        // probes between two looks at the overflow count
constexpr int TABLE_ROUNDS = 16;          // slots per thread of the compaction: one atomicAdd per 4 096 slots

__device__ __forceinline__ u64 mix64(u64 h) {
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

__device__ __forceinline__ bool cell_ok(float cx, float cy, float cz) {
    return fabsf(cx) < CELL_LIMIT && fabsf(cy) < CELL_LIMIT && fabsf(cz) < CELL_LIMIT;
}

__device__ __forceinline__ u64 key_of(float cx, float cy, float cz) {
    return ((u64)((int)cx + (1 << 20)) << 42) | ((u64)((int)cy + (1 << 20)) << 21) | (u64)((int)cz + (1 << 20));
}

__device__ __forceinline__ void cell_of(u64 key, int c[3]) {
    c[0] = (int)(key >> 42) - (1 << 20);
    c[1] = (int)((key >> 21) & 0x1fffffu) - (1 << 20);
    c[2] = (int)(key & 0x1fffffu) - (1 << 20);
}

// key + axis_step(a) is the key of the next cell along axis a; a carry out of a field gives a key no cell has
__device__ __forceinline__ u64 axis_step(int a) { return 1ull << (42 - 21 * a); }

// The slot of `key`, claimed if nobody had. `overflow` == nullptr: the caller's table has room for every key, so a slot is always found
// within `capacity` steps; the bound only keeps a lane from spinning on a table it did not set up. Else *overflow counts the keys that
// found no home: keys never leave, so once one key has seen `capacity` full slots the table stays full, every lane that looks (each
// GIVE_UP_EVERY probes) gives up as well, and EMPTY comes back.
__device__ __forceinline__ u64 claim_slot(u64* __restrict__ keys, u64 capacity, u64 key, const u64* overflow) {
    u64 at = mix64(key) & (capacity - 1), slot = EMPTY;
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
        if (overflow && (step & (GIVE_UP_EVERY - 1)) == GIVE_UP_EVERY - 1 && __atomic_load_n(overflow, __ATOMIC_RELAXED) != 0) break;
        at = (at + 1) & (capacity - 1);
    }
    return slot;
}

// SLOTS: (key, slot) pairs go out; else keys only and slot_out is not looked at
template <bool SLOTS>
__global__ __launch_bounds__(256) void table_compact_kernel(const u64* __restrict__ keys, u64 capacity, long* __restrict__ key_out,
                                                            long* __restrict__ slot_out, u64 max_rows, u64* __restrict__ count) {
    __shared__ unsigned wave_sum[4];
    __shared__ u64 base_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 s0 = (u64)blockIdx.x * (256 * TABLE_ROUNDS) + threadIdx.x;             // round r looks at slot s0 + 256 r
    u64 key[TABLE_ROUNDS];
    unsigned mine = 0;
#pragma unroll
    for (int r = 0; r < TABLE_ROUNDS; ++r) {
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
    for (int r = 0; r < TABLE_ROUNDS; ++r) {
        if (key[r] == EMPTY) continue;
        if (pos < max_rows) {                                                        // the count still says how many there were
            key_out[pos] = (long)key[r];
            if (SLOTS) slot_out[pos] = (long)(s0 + 256 * r);
        }
        ++pos;
    }
}

bool capacity_ok(long capacity) { return capacity >= 1 && capacity <= (1L << 32) && (capacity & (capacity - 1)) == 0; }
bool voxel_ok(float voxel) { return voxel > 0.f && voxel < INFINITY; }

// the checks every launch on a table shares, in this order; `need` = the table's bytes at this capacity, `too_small` the refusal that
// names the function which says so
int table_ok(const char* who, const void* workspace, size_t workspace_bytes, long capacity, size_t need, const char* too_small) {
    if (!workspace || (size_t)workspace % 8) return refuse(who, "an 8-byte aligned workspace is required");
    if (!capacity_ok(capacity)) return refuse(who, "capacity must be a power of two, 1 <= capacity <= 2^32");
    if (workspace_bytes < need) return refuse(who, too_small);
    return GEO4D_OK;
}

// count := 0, then the compaction of the table's keys; the caller has checked the table and the outputs
template <bool SLOTS>
int table_compact(const char* who, const void* workspace, long capacity, long* keys_out, long* slots_out, long max_rows, long* count,
                  hipStream_t s) {
    if (hipMemsetAsync(count, 0, sizeof(long), s) != hipSuccess) {
        char msg[64];
        snprintf(msg, sizeof msg, "%s: hipMemsetAsync failed", who);
        geo4d_set_error(msg);
        return GEO4D_EIO;
    }
    hipLaunchKernelGGL(table_compact_kernel<SLOTS>, dim3((unsigned)((capacity + 256 * TABLE_ROUNDS - 1) / (256 * TABLE_ROUNDS))), dim3(256), 0, s,
                       (const u64*)workspace, (u64)capacity, keys_out, slots_out, (u64)max_rows, (u64*)count);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

}  // namespace
