// geo4d_amd/csrc/tsdf_field.h — what the readers of a TSDF field (sorted keys K[0..M), f, Wt) share: tsdf.hip's surface points and
// tsdf_mesh.hip's surface nets. Keys are (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20) with |c| < 2^20, so a field of a real cell
// holds 1 .. 2^21 - 1 and unsigned key order is (cx, cy, cz) order.
#pragma once
#include <cmath>
#include <cstdio>
#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

// the centre of the voxel with this key
__device__ __forceinline__ void centre_of(u64 key, float v, float& X, float& Y, float& Z) {
    const int cx = (int)(key >> 42) - (1 << 20), cy = (int)((key >> 21) & 0x1fffffu) - (1 << 20), cz = (int)(key & 0x1fffffu) - (1 << 20);
    X = ((float)cx + 0.5f) * v;
    Y = ((float)cy + 0.5f) * v;
    Z = ((float)cz + 0.5f) * v;
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

bool voxel_ok(float voxel) { return voxel > 0.f && voxel < INFINITY; }

int refuse(const char* who, const char* what) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    geo4d_set_error(msg);
    return GEO4D_EINVAL;
}

}  // namespace
