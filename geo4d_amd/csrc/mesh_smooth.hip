// geo4d_amd/csrc/mesh_smooth.hip — the corner table of an indexed triangle mesh (for each vertex, the corners of the faces around it)
// and its three consumers: boundary vertices, the Taubin smoothing step and area-weighted vertex normals (geo4d_amd/mesh.py,
// ops.mesh_adjacency, ops.mesh_smooth_step, ops.mesh_vertex_normals).
//
// The reference has no such step; nothing is ported. The rule is the project's own and is stated here, in include/geo4d_hip.h and, in
// numpy, in tests/mesh_smooth_restatement.py. The table is integer arithmetic and sorted, so it is a function of the mesh alone,
// whatever the order of the faces' threads. The float outputs are gathered per vertex by one thread in the table's order: fp32 in the
// written order with contraction into FMAs switched off, only + - * / and sqrtf, each correctly rounded; no float atomics.
//
// Inputs: vertices fp32 [Nv][3], faces int32 [T][3], face_mask u8 [T] (NULL: every face).
// valid:  face t is valid iff face_mask[t] != 0 (or there is no mask) and its three indices lie in [0, Nv): decided before anything is
//   read or written through them. A valid face may repeat an index.
// table:  an entry is e = 3 t + k for a valid face t and corner k and belongs to vertex faces[t][k]. offsets int32 [Nv + 1] is the
//   exclusive prefix sum of the entries per vertex, corners int32 [E] holds each vertex's entries ascending in e. A face that names v
//   twice appears twice in v's row.
// neighbours of v: walk v's row in order; of each entry (t, k) take a = faces[t][(k + 1) % 3], then b = faces[t][(k + 2) % 3]; skip
//   those equal to v; m is the list's length. A neighbour seen from two faces stands twice.
// boundary: boundary[v] = 1 iff some id occurs exactly once in v's list, else 0 (an empty list: 0). A neighbour across an edge that
//   three or four triangles share occurs three or four times and makes no boundary.
// step(s): S = 0; for each w of the list in order S_c = S_c + p[w]_c; then p'[v]_c = p[v]_c + s * (S_c / (float) m - p[v]_c). v keeps
//   its bits if m = 0 or it is pinned. Jacobi: p' is another buffer, never p.
// normals: n(t) = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x) with e1 = p1 - p0, e2 = p2 - p0 in the face's own order
//   (its length is twice the area: the weighting is by area); N = 0, then N_c = N_c + n(t)_c over v's row in order;
//   len2 = (Nx Nx + Ny Ny) + Nz Nz; the result is N_c / sqrtf(len2) if len2 > 0 and finite, else (0, 0, 0).
//
// Launches. count: one thread per face, degree[v] += 1 per corner of a valid face (integer atomics into the caller's zeroed buffer);
//   the caller's cumsum gives offsets and E. fill: one thread per face, slot = offsets[v] + atomicAdd(cursor + v, 1) (cursor zeroed by
//   the caller), corners[slot] = 3 t + k: a row's order is arbitrary here. sort: every row ascending into a second buffer; a row of at
//   most long_row entries by its vertex's thread (insertion), a longer one by that thread's whole wave (each entry's rank by counting
//   the smaller ones; a row's entries are distinct). boundary: the same split, counting occurrences. step, normals: one thread per
//   vertex walks its row; face normals are recomputed per corner, the bits are those of a stored one.
// Every loop is bounded by a row length or by the 64 lanes of a wave, and says so where it stands; no thread waits on another.
// Whatever offsets and corners hold, nothing is read or written outside the buffers: a row outside [0, E], an entry outside [0, 3 T)
// and an index outside [0, Nv) are skipped (a table built by count, fill and sort holds none).
// limits: 3 T < 2^31, Nv < 2^31; time is linear in the largest valence (step, normals) and quadratic in it over 64 lanes (sort,
//   boundary); no LDS, no scratch.
#include "common.h"
#include "geo4d_hip.h"
#include "scene_view.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ bool index_ok(int i, long Nv) { return i >= 0 && (long)i < Nv; }

// the three indices of face t if it is valid
__device__ __forceinline__ bool valid_face(const int* __restrict__ faces, long t, long Nv, const unsigned char* __restrict__ mask, int& i0,
                                           int& i1, int& i2) {
    if (mask && !mask[t]) return false;
    i0 = faces[t * 3];
    i1 = faces[t * 3 + 1];
    i2 = faces[t * 3 + 2];
    return index_ok(i0, Nv) && index_ok(i1, Nv) && index_ok(i2, Nv);
}

// v's row [first, first + n) of the table; n = 0 where offsets do not describe a row inside [0, E]
__device__ __forceinline__ void row_of(const int* __restrict__ offsets, long v, long E, int& first, int& n) {
    const int b = offsets[v], e = offsets[v + 1];
    first = b;
    n = (b >= 0 && e >= b && (long)e <= E) ? e - b : 0;
}

// the i-th candidate of v's neighbour list (i = 2 * place in the row + 0 for a, 1 for b), -1 where it is skipped: equal to v, or an
// entry or index that no table of this mesh holds
__device__ __forceinline__ int candidate(const int* __restrict__ faces, long T3, long Nv, const int* __restrict__ corners, int first, int i,
                                         int v) {
    const int e = corners[first + (i >> 1)];
    if (e < 0 || (long)e >= T3) return -1;
    const int t = e / 3, k = e - 3 * t;
    int c = k + 1 + (i & 1);
    c = c >= 3 ? c - 3 : c;
    const int w = faces[(long)t * 3 + c];
    return (w != v && index_ok(w, Nv)) ? w : -1;
}

__global__ __launch_bounds__(256) void adjacency_count_kernel(const int* __restrict__ faces, long T, long Nv,
                                                              const unsigned char* __restrict__ mask, int* __restrict__ degree) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int i0, i1, i2;
    if (!valid_face(faces, t, Nv, mask, i0, i1, i2)) return;
    atomicAdd(degree + i0, 1);
    atomicAdd(degree + i1, 1);
    atomicAdd(degree + i2, 1);
}

__global__ __launch_bounds__(256) void adjacency_fill_kernel(const int* __restrict__ faces, long T, long Nv,
                                                             const unsigned char* __restrict__ mask, const int* __restrict__ offsets, long E,
                                                             int* __restrict__ cursor, int* __restrict__ corners) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int i[3];
    if (!valid_face(faces, t, Nv, mask, i[0], i[1], i[2])) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                                    // three corners
        int first, n;
        row_of(offsets, i[k], E, first, n);
        const int place = atomicAdd(cursor + i[k], 1);
        if (place >= 0 && place < n) corners[first + place] = (int)(3 * t + k);      // else not this mesh's offsets: nothing is written
    }
}

// Row (first, n) of `in`, ascending, into the same row of `out`, by the calling thread alone: insertion. The outer loop runs n times,
// the inner one at most i times: it moves j down by one each turn and stops at 0.
__device__ __forceinline__ void sort_row_thread(const int* __restrict__ in, int* __restrict__ out, int first, int n) {
    for (int i = 0; i < n; ++i) {
        const int x = in[first + i];
        int j = i;
        for (; j > 0; --j) {
            const int y = out[first + j - 1];
            if (y <= x) break;
            out[first + j] = y;
        }
        out[first + j] = x;
    }
}

// Row (first, n) of `in`, ascending, into the same row of `out`, by the 64 lanes of the calling wave: lane l places entries l, l + 64,
// ... each at its rank, the number of smaller entries, ties broken by the place so that equal entries (which no table of the rule
// holds) still get distinct ranks. Both loops are bounded by n.
__device__ __forceinline__ void sort_row_wave(const int* __restrict__ in, int* __restrict__ out, int first, int n, int lane) {
    for (int i = lane; i < n; i += 64) {
        const int x = in[first + i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const int y = in[first + j];
            rank += (y < x || (y == x && j < i)) ? 1 : 0;
        }
        out[first + rank] = x;
    }
}

__global__ __launch_bounds__(256) void adjacency_sort_kernel(const int* __restrict__ offsets, long Nv, long E, const int* __restrict__ in,
                                                             int* __restrict__ out, int long_row) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;                             // no early return: the wave's lanes vote below
    int first = 0, n = 0;
    if (v < Nv) row_of(offsets, v, E, first, n);
    const bool is_long = n > long_row;
    if (!is_long) sort_row_thread(in, out, first, n);
    const int lane = threadIdx.x & 63;
    // the long rows of this wave's 64 vertices, one after the other, each by all 64 lanes: every turn clears one bit of `todo`
    for (unsigned long long todo = __ballot(is_long); todo; todo &= todo - 1) {
        const int owner = __ffsll((long long)todo) - 1;
        sort_row_wave(in, out, __shfl(first, owner), __shfl(n, owner), lane);
    }
}

// Does candidate i of v's list (2 n candidates) stand exactly once in it? Bounded by 2 n; stops early at the second occurrence.
__device__ __forceinline__ bool stands_once(const int* __restrict__ faces, long T3, long Nv, const int* __restrict__ corners, int first, int n,
                                            int v, int i) {
    const int w = candidate(faces, T3, Nv, corners, first, i, v);
    if (w < 0) return false;
    int seen = 0;
    for (int j = 0; j < 2 * n && seen < 2; ++j) seen += candidate(faces, T3, Nv, corners, first, j, v) == w ? 1 : 0;
    return seen == 1;
}

__global__ __launch_bounds__(256) void boundary_kernel(const int* __restrict__ faces, long T3, long Nv, const int* __restrict__ offsets,
                                                       const int* __restrict__ corners, long E, int long_row,
                                                       unsigned char* __restrict__ boundary) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;                             // no early return: the wave's lanes vote below
    int first = 0, n = 0;
    if (v < Nv) row_of(offsets, v, E, first, n);
    const bool is_long = n > long_row;
    if (v < Nv && !is_long) {
        bool open = false;
        for (int i = 0; i < 2 * n && !open; ++i) open = stands_once(faces, T3, Nv, corners, first, n, (int)v, i);   // at most 2 n turns
        boundary[v] = open ? 1 : 0;
    }
    const int lane = threadIdx.x & 63;
    // the long rows of this wave's 64 vertices, one after the other: every turn clears one bit of `todo`
    for (unsigned long long todo = __ballot(is_long); todo; todo &= todo - 1) {
        const int owner = __ffsll((long long)todo) - 1;
        const int f = __shfl(first, owner), rows = __shfl(n, owner);
        const int u = __shfl((int)v, owner);                                         // the owner's vertex (below Nv < 2^31: its row is not empty)
        bool open = false;
        for (int i = lane; i < 2 * rows; i += 64) open = open || stands_once(faces, T3, Nv, corners, f, rows, u, i);   // bounded by 2 n
        const bool any = __ballot(open) != 0;
        if (lane == owner) boundary[v] = any ? 1 : 0;                                // one writer: the row's own thread
    }
}

__global__ __launch_bounds__(256) void smooth_step_kernel(const float* __restrict__ p, const int* __restrict__ faces, long T3, long Nv,
                                                          const int* __restrict__ offsets, const int* __restrict__ corners, long E,
                                                          const unsigned char* __restrict__ pinned, float s, float* __restrict__ out) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= Nv) return;
    const float x = p[v * 3], y = p[v * 3 + 1], z = p[v * 3 + 2];
    float Sx = 0.f, Sy = 0.f, Sz = 0.f;
    int m = 0;
    if (!(pinned && pinned[v])) {
        int first, n;
        row_of(offsets, v, E, first, n);
        for (int i = 0; i < 2 * n; ++i) {                                            // the row's candidates in order: 2 n turns
            const int w = candidate(faces, T3, Nv, corners, first, i, (int)v);
            if (w < 0) continue;
            Sx = Sx + p[(long)w * 3];
            Sy = Sy + p[(long)w * 3 + 1];
            Sz = Sz + p[(long)w * 3 + 2];
            ++m;
        }
    }
    if (m == 0) {                                                                    // no neighbour, or pinned: the same bits
        out[v * 3] = x;
        out[v * 3 + 1] = y;
        out[v * 3 + 2] = z;
        return;
    }
    const float fm = (float)m;
    out[v * 3] = x + s * (Sx / fm - x);
    out[v * 3 + 1] = y + s * (Sy / fm - y);
    out[v * 3 + 2] = z + s * (Sz / fm - z);
}

__global__ __launch_bounds__(256) void vertex_normals_kernel(const float* __restrict__ p, const int* __restrict__ faces, long T3, long Nv,
                                                             const int* __restrict__ offsets, const int* __restrict__ corners, long E,
                                                             float* __restrict__ out) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= Nv) return;
    int first, n;
    row_of(offsets, v, E, first, n);
    float Nx = 0.f, Ny = 0.f, Nz = 0.f;
    for (int i = 0; i < n; ++i) {                                                    // the row's entries in order: n turns
        const int e = corners[first + i];
        if (e < 0 || (long)e >= T3) continue;
        int i0, i1, i2;
        if (!valid_face(faces, e / 3, Nv, nullptr, i0, i1, i2)) continue;
        const float x0 = p[(long)i0 * 3], y0 = p[(long)i0 * 3 + 1], z0 = p[(long)i0 * 3 + 2];
        const float e1x = p[(long)i1 * 3] - x0, e1y = p[(long)i1 * 3 + 1] - y0, e1z = p[(long)i1 * 3 + 2] - z0;
        const float e2x = p[(long)i2 * 3] - x0, e2y = p[(long)i2 * 3 + 1] - y0, e2z = p[(long)i2 * 3 + 2] - z0;
        Nx = Nx + (e1y * e2z - e1z * e2y);
        Ny = Ny + (e1z * e2x - e1x * e2z);
        Nz = Nz + (e1x * e2y - e1y * e2x);
    }
    const float len2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (len2 > 0.f && finite1(len2)) {
        const float len = sqrtf(len2);
        ox = Nx / len;
        oy = Ny / len;
        oz = Nz / len;
    }
    out[v * 3] = ox;
    out[v * 3 + 1] = oy;
    out[v * 3 + 2] = oz;
}

// 0 <= T, 3 T < 2^31, 0 <= Nv < 2^31
bool mesh_ok(long T, long Nv) { return T >= 0 && T < (1L << 31) && 3 * T < (1L << 31) && Nv >= 0 && Nv < (1L << 31); }
const char* const MESH_DIMS = "need 0 <= T, 3 T < 2^31 and 0 <= Nv < 2^31";
unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int geo4d_mesh_adjacency_count(const int* faces, long T, long Nv, const unsigned char* face_mask, int* degree, void* stream) {
    const char* who = "mesh_adjacency_count";
    if (!mesh_ok(T, Nv)) return refuse(who, MESH_DIMS);
    if (!faces || !degree) return refuse(who, "faces and degree are required");
    if (T == 0 || Nv == 0) return GEO4D_OK;
    hipLaunchKernelGGL(adjacency_count_kernel, dim3(blocks_of(T)), dim3(256), 0, (hipStream_t)stream, faces, T, Nv, face_mask, degree);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_mesh_adjacency_fill(const int* faces, long T, long Nv, const unsigned char* face_mask, const int* offsets, long E,
                                         int* cursor, int* corners, void* stream) {
    const char* who = "mesh_adjacency_fill";
    if (!mesh_ok(T, Nv)) return refuse(who, MESH_DIMS);
    if (E < 0 || E > 3 * T) return refuse(who, "need 0 <= E <= 3 T");
    if (!faces || !offsets || !cursor || !corners) return refuse(who, "faces, offsets, cursor and corners are required");
    if (T == 0 || Nv == 0 || E == 0) return GEO4D_OK;
    hipLaunchKernelGGL(adjacency_fill_kernel, dim3(blocks_of(T)), dim3(256), 0, (hipStream_t)stream, faces, T, Nv, face_mask, offsets, E, cursor,
                       corners);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_mesh_adjacency_sort(const int* offsets, long T, long Nv, long E, const int* corners_in, int* corners_out, int long_row,
                                         void* stream) {
    const char* who = "mesh_adjacency_sort";
    if (!mesh_ok(T, Nv)) return refuse(who, MESH_DIMS);
    if (E < 0 || E > 3 * T) return refuse(who, "need 0 <= E <= 3 T");
    if (long_row < 0) return refuse(who, "need long_row >= 0");
    if (!offsets || !corners_in || !corners_out || corners_in == corners_out)
        return refuse(who, "offsets, corners_in and another buffer corners_out are required");
    if (T == 0 || Nv == 0 || E == 0) return GEO4D_OK;
    hipLaunchKernelGGL(adjacency_sort_kernel, dim3(blocks_of(Nv)), dim3(256), 0, (hipStream_t)stream, offsets, Nv, E, corners_in, corners_out,
                       long_row);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_mesh_boundary(const int* faces, long T, long Nv, const int* offsets, const int* corners, long E, int long_row,
                                   unsigned char* boundary, void* stream) {
    const char* who = "mesh_boundary";
    if (!mesh_ok(T, Nv)) return refuse(who, MESH_DIMS);
    if (E < 0 || E > 3 * T) return refuse(who, "need 0 <= E <= 3 T");
    if (long_row < 0) return refuse(who, "need long_row >= 0");
    if (!faces || !offsets || (!corners && E > 0) || !boundary) return refuse(who, "faces, offsets, corners (unless E = 0) and boundary are required");
    if (T == 0 || Nv == 0) return GEO4D_OK;
    hipLaunchKernelGGL(boundary_kernel, dim3(blocks_of(Nv)), dim3(256), 0, (hipStream_t)stream, faces, 3 * T, Nv, offsets, corners, E, long_row,
                       boundary);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_mesh_smooth_step(const float* vertices, const int* faces, long T, long Nv, const int* offsets, const int* corners, long E,
                                      const unsigned char* pinned, float s, float* vertices_out, void* stream) {
    const char* who = "mesh_smooth_step";
    if (!mesh_ok(T, Nv)) return refuse(who, MESH_DIMS);
    if (E < 0 || E > 3 * T) return refuse(who, "need 0 <= E <= 3 T");
    if (!std::isfinite(s)) return refuse(who, "the factor s must be finite");
    if (!vertices || !faces || !offsets || (!corners && E > 0) || !vertices_out || vertices == vertices_out)
        return refuse(who, "vertices, faces, offsets, corners (unless E = 0) and another buffer vertices_out are required (a step is never in place)");
    if (T == 0 || Nv == 0) return GEO4D_OK;
    hipLaunchKernelGGL(smooth_step_kernel, dim3(blocks_of(Nv)), dim3(256), 0, (hipStream_t)stream, vertices, faces, 3 * T, Nv, offsets, corners,
                       E, pinned, s, vertices_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_mesh_vertex_normals(const float* vertices, const int* faces, long T, long Nv, const int* offsets, const int* corners,
                                         long E, float* normals_out, void* stream) {
    const char* who = "mesh_vertex_normals";
    if (!mesh_ok(T, Nv)) return refuse(who, MESH_DIMS);
    if (E < 0 || E > 3 * T) return refuse(who, "need 0 <= E <= 3 T");
    if (!vertices || !faces || !offsets || (!corners && E > 0) || !normals_out)
        return refuse(who, "vertices, faces, offsets, corners (unless E = 0) and normals_out are required");
    if (T == 0 || Nv == 0) return GEO4D_OK;
    hipLaunchKernelGGL(vertex_normals_kernel, dim3(blocks_of(Nv)), dim3(256), 0, (hipStream_t)stream, vertices, faces, 3 * T, Nv, offsets,
                       corners, E, normals_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
