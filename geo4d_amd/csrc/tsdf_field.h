// geo4d_amd/csrc/tsdf_field.h — what the readers of a TSDF field (sorted keys K[0..M), f, Wt) share: tsdf.hip's surface points and
// tsdf_mesh.hip's surface nets. Keys are voxel_table.h's, so unsigned key order is (cx, cy, cz) order.
#pragma once
#include "voxel_table.h"                                                             // u64, cell_of, axis_step, voxel_ok, refuse

#pragma clang fp contract(off)

namespace {

// the centre of the voxel with this key
__device__ __forceinline__ void centre_of(u64 key, float v, float& X, float& Y, float& Z) {
    int c[3];
    cell_of(key, c);
    X = ((float)c[0] + 0.5f) * v;
    Y = ((float)c[1] + 0.5f) * v;
    Z = ((float)c[2] + 0.5f) * v;
}

__device__ __forceinline__ bool live(float f, float wt, float min_weight) { return wt >= min_weight && fabsf(f) < 1.f; }

// the row of `target` in K[lo..M), or -1; unsigned order, so a key with bit 63 set (a carry out of the x field) is beyond every row
__device__ __forceinline__ long find_key(const long* __restrict__ K, long lo, long M, u64 target) {
    long hi = M;
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if ((u64)K[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo < M && (u64)K[lo] == target ? lo : -1;
}

}  // namespace
