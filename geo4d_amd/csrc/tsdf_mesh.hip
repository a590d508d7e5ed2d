// geo4d_amd/csrc/tsdf_mesh.hip — the denoised static scene as one triangle mesh: naive surface nets (the dual method) on the TSDF field
// that tsdf.hip integrates (geo4d_amd/tsdf.py tsdf_mesh, ops.tsdf_mesh_extract).
//
// The reference has no such step; nothing is ported. The rule is the project's own and is stated here, in include/geo4d_hip.h and, in
// numpy, in tests/tsdf_mesh_restatement.py. All float arithmetic is fp32 in the written order with contraction into FMAs switched off,
// as in tsdf.hip; only + - * / are used. No table of cases, no atomics: every output row has one writer and its place is a function of
// the inputs alone.
//
// Inputs: exactly what geo4d_tsdf_integrate leaves: K int64 [M] sorted keys ((c + 2^20) in three 21-bit fields, voxel_table.h), f fp32
//   [M], Wt fp32 [M], rgba u8 [M][4] (NULL: no colours), plus the voxel v and min_weight.
// live, s, E: live is tsdf_field.h's live(f, Wt, min_weight); s(m) = f[m] >= 0; the step along axis a is E_a = (1 << 42, 1 << 21, 1)[a]. A
//   key field holds 1 .. 2^21 - 1 for a real cell: + E_a out of a full field carries into a field of value 0 and - E_a from 1 gives 0,
//   and no cell has either key, so no edge-of-grid test is needed in either direction.
// cell:   cell m is the cube whose eight corners are the voxel centres with keys K[m] + ox E_0 + oy E_1 + oz E_2, o in {0, 1}^3, corner
//   index 4 ox + 2 oy + oz. It is complete iff all eight keys are in K and all eight voxels are live. (cells: one thread per m, seven
//   searches, each above the row of the corner before it, since the corner keys ascend with the corner index; the + z corners are the
//   next rows and need no search. The byte it leaves is 0 for a cell that is not complete, else 1 | 2 x0 | 4 x1 | 8 x2 with x_a =
//   s(m) != s(m + E_a), which the cell's own corners say: count and faces search only for the rings of those pairs.)
// face:   for voxel m and axis a let m' = the row of K[m] + E_a. The pair qualifies if m and m' are live and s(m) != s(m'). With
//   b = (a + 1) % 3 and c = (a + 2) % 3 the four cells sharing that grid edge are r0 = m, r1 = m - E_b, r2 = m - E_b - E_c, r3 = m - E_c;
//   one quad is emitted iff all four exist in K and are complete (r0 complete implies that the pair is live). If f[m] < 0 the ring is
//   (r0, r1, r2, r3): positive f is the free space in front of the surface, which is then on the + a side, and this ring is counter-
//   clockwise seen from + a; otherwise the ring is (r0, r3, r2, r1). The two triangles are (q0, q1, q2) and (q0, q2, q3) of the ring, so
//   front faces look toward the cameras. Quads are ordered by (m, a); triangle rows are 2 quad and 2 quad + 1. (count: quads per m and
//   used[r] = 1 for the ring cells of every quad, plain byte stores of one value; the caller's cumsum; faces: one writer per (m, a).)
// vertex: a cell is used iff an emitted quad names it; used cells get the ids 0 .. V - 1 in order of m (the caller's cumsum over used).
//   A complete cell with a sign change but no emitted quad gets no vertex. Position: for a = 0, 1, 2 and, within a, the four edges with
//   the other two axes' offsets (0, 0), (1, 0), (0, 1), (1, 1) (lower axis first): p = the corner with o_a = 0, q = the corner with
//   o_a = 1; if s(p) != s(q): t = f_p / (f_p - f_q), o with o_a replaced by t is added to S componentwise (S starts at 0), cnt += 1.
//   The vertex is X0_k + (S_k / (float)cnt) * v with X0 = ((float)cell + 0.5f) * v, the centre of voxel m. Colour: that of the corner
//   with the smallest |f|, the lowest corner index on ties. Weight: the minimum Wt of the eight corners by fminf in corner order.
// limits: M < 2^31; vertex ids and face indices are int32; T = 2 Q. A grid face with four sign changes gives a mesh edge shared by four
//   triangles: a property of the method.
#include <cmath>
#include "common.h"
#include "geo4d_hip.h"
#include "tsdf_field.h"

#pragma clang fp contract(off)

namespace {

// find_key in K[lo..M) after a look at row lo, and in K[0..hi) after a look at row hi - 1: z is the lowest key field, so the + z
// neighbour of a voxel is the next row and its - z neighbour the row before, if they exist at all; half the searches end there
__device__ __forceinline__ long find_from(const long* __restrict__ K, long lo, long M, u64 target) {
    if (lo < M && (u64)K[lo] == target) return lo;
    return find_key(K, lo, M, target);
}
__device__ __forceinline__ long find_below(const long* __restrict__ K, long hi, u64 target) {
    if (hi > 0 && (u64)K[hi - 1] == target) return hi - 1;
    return find_key(K, 0, hi, target);
}

// rows of the corners 1 .. 7 of cell m (corner 0 is m itself); false as soon as one is missing
__device__ __forceinline__ bool corners_of(const long* __restrict__ K, long M, long m, long c[8]) {
    const u64 key = (u64)K[m];
    c[0] = m;
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        c[i] = find_from(K, c[i - 1] + 1, M, key + (u64)(i >> 2) * axis_step(0) + (u64)((i >> 1) & 1) * axis_step(1) + (u64)(i & 1));
        if (c[i] < 0) return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void tsdf_mesh_cells_kernel(const long* __restrict__ K, long M, const float* __restrict__ f,
                                                              const float* __restrict__ wt, float min_weight,
                                                              unsigned char* __restrict__ complete) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    bool ok = live(f[m], wt[m], min_weight);
    long c[8];
    ok = ok && corners_of(K, M, m, c);
    unsigned cell = 0;
    if (ok) {
        float fc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) fc[i] = f[c[i]];
#pragma unroll
        for (int i = 1; i < 8; ++i) ok = ok && live(fc[i], wt[c[i]], min_weight);
        const bool sm = fc[0] >= 0.f;
        if (ok) cell = 1u | (sm != (fc[4] >= 0.f) ? 2u : 0u) | (sm != (fc[2] >= 0.f) ? 4u : 0u) | (sm != (fc[1] >= 0.f) ? 8u : 0u);
    }
    complete[m] = (unsigned char)cell;
}

// the quads of voxel m: ring[a] = the rows r1, r2, r3 of quad (m, a), ring[a][0] = -1 where there is none; returns how many there are
__device__ __forceinline__ int quads_of(const long* __restrict__ K, const unsigned char* __restrict__ complete, long m, long ring[3][3]) {
    ring[0][0] = ring[1][0] = ring[2][0] = -1;
    const unsigned cell = complete[m];
    if (cell < 2u) return 0;                                                         // not complete, or no sign change along an axis
    int count = 0;
    const u64 key = (u64)K[m];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(cell & (2u << a))) continue;                                           // m' is a corner of the complete cell m: it is live
        const u64 eb = axis_step((a + 1) % 3), ec = axis_step((a + 2) % 3);
        const long r1 = find_below(K, m, key - eb);
        if (r1 < 0 || !complete[r1]) continue;
        const long r3 = find_below(K, m, key - ec);
        if (r3 < 0 || !complete[r3]) continue;
        const long r2 = find_below(K, r1 < r3 ? r1 : r3, key - eb - ec);
        if (r2 < 0 || !complete[r2]) continue;
        ring[a][0] = r1;
        ring[a][1] = r2;
        ring[a][2] = r3;
        ++count;
    }
    return count;
}

__global__ __launch_bounds__(256) void tsdf_mesh_count_kernel(const long* __restrict__ K, long M, const unsigned char* __restrict__ complete,
                                                              int* __restrict__ counts, unsigned char* __restrict__ used) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    long ring[3][3];
    const int count = quads_of(K, complete, m, ring);
    counts[m] = count;
    if (!count) return;
    used[m] = 1;                                                                     // every writer of a byte stores the same value
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (ring[a][0] < 0) continue;
        used[ring[a][0]] = 1;
        used[ring[a][1]] = 1;
        used[ring[a][2]] = 1;
    }
}

__global__ __launch_bounds__(256) void tsdf_mesh_vertices_kernel(const long* __restrict__ K, long M, const float* __restrict__ f,
                                                                 const float* __restrict__ wt, const unsigned char* __restrict__ rgba_vox,
                                                                 const unsigned char* __restrict__ used,
                                                                 const long* __restrict__ first_vertex, long V, float v,
                                                                 float* __restrict__ vertices_out, unsigned char* __restrict__ rgba_out,
                                                                 float* __restrict__ weight_out) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M || !used[m]) return;
    const long id = first_vertex[m];
    if (id < 0 || id >= V) return;                                                   // not this field's offsets: nothing is written
    long c[8];
    if (!corners_of(K, M, m, c)) return;                                             // a used cell is complete
    float fc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) fc[i] = f[c[i]];
    float S[3] = {0.f, 0.f, 0.f};
    int cnt = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int lo = a == 0 ? 1 : 0, hi = a == 2 ? 1 : 2;                          // the other two axes, lower first
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int o[3] = {0, 0, 0};
            o[lo] = e & 1;
            o[hi] = e >> 1;
            const int p = 4 * o[0] + 2 * o[1] + o[2], q = p + (4 >> a);
            if ((fc[p] >= 0.f) == (fc[q] >= 0.f)) continue;
            const float t = fc[p] / (fc[p] - fc[q]);
            S[0] += a == 0 ? t : (float)o[0];
            S[1] += a == 1 ? t : (float)o[1];
            S[2] += a == 2 ? t : (float)o[2];
            ++cnt;
        }
    }
    float X[3];
    centre_of((u64)K[m], v, X[0], X[1], X[2]);
    const float n = (float)cnt;
    vertices_out[id * 3] = X[0] + (S[0] / n) * v;
    vertices_out[id * 3 + 1] = X[1] + (S[1] / n) * v;
    vertices_out[id * 3 + 2] = X[2] + (S[2] / n) * v;
    long pick = c[0];
    float least = fabsf(fc[0]), w = wt[c[0]];
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        if (fabsf(fc[i]) < least) {
            least = fabsf(fc[i]);
            pick = c[i];
        }
        w = fminf(w, wt[c[i]]);
    }
    if (rgba_out) *(unsigned*)(rgba_out + id * 4) = *(const unsigned*)(rgba_vox + pick * 4);
    weight_out[id] = w;
}

__global__ __launch_bounds__(256) void tsdf_mesh_faces_kernel(const long* __restrict__ K, long M, const float* __restrict__ f,
                                                              const unsigned char* __restrict__ complete, const int* __restrict__ counts,
                                                              const long* __restrict__ first_quad, const long* __restrict__ first_vertex,
                                                              long Q, long V, int* __restrict__ faces_out) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M || !counts[m]) return;
    long ring[3][3];
    if (!quads_of(K, complete, m, ring)) return;
    const bool inside = f[m] < 0.f;
    const long q0 = first_vertex[m];
    long row = first_quad[m];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (ring[a][0] < 0) continue;
        if (row < 0 || row >= Q) return;                                            // not this field's offsets: nothing is written
        const long r1 = first_vertex[ring[a][0]], q2 = first_vertex[ring[a][1]], r3 = first_vertex[ring[a][2]];
        const long q1 = inside ? r1 : r3, q3 = inside ? r3 : r1;
        if (q0 < 0 || q0 >= V || q1 < 0 || q1 >= V || q2 < 0 || q2 >= V || q3 < 0 || q3 >= V) return;
        int* out = faces_out + row * 6;
        out[0] = (int)q0;
        out[1] = (int)q1;
        out[2] = (int)q2;
        out[3] = (int)q0;
        out[4] = (int)q2;
        out[5] = (int)q3;
        ++row;
    }
}

bool rows_ok(long M) { return M >= 0 && M < (1L << 31); }
unsigned blocks_of(long M) { return (unsigned)((M + 255) / 256); }

}  // namespace

extern "C" int geo4d_tsdf_mesh_cells(const long* keys, long M, const float* f, const float* weight, float min_weight, unsigned char* complete,
                                     void* stream) {
    const char* who = "tsdf_mesh_cells";
    if (!keys || !f || !weight || !complete) return refuse(who, "keys, f, weight and complete are required");
    if (!rows_ok(M)) return refuse(who, "need 0 <= M < 2^31");
    if (!(min_weight > 0.f)) return refuse(who, "need min_weight > 0");
    if (M == 0) return GEO4D_OK;
    hipLaunchKernelGGL(tsdf_mesh_cells_kernel, dim3(blocks_of(M)), dim3(256), 0, (hipStream_t)stream, keys, M, f, weight, min_weight, complete);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_tsdf_mesh_count(const long* keys, long M, const unsigned char* complete, int* counts, unsigned char* used, void* stream) {
    const char* who = "tsdf_mesh_count";
    if (!keys || !complete || !counts || !used) return refuse(who, "keys, complete, counts and used are required");
    if (!rows_ok(M)) return refuse(who, "need 0 <= M < 2^31");
    if (M == 0) return GEO4D_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(used, 0, (size_t)M, s) != hipSuccess) {
        geo4d_set_error("tsdf_mesh_count: hipMemsetAsync failed");
        return GEO4D_EIO;
    }
    hipLaunchKernelGGL(tsdf_mesh_count_kernel, dim3(blocks_of(M)), dim3(256), 0, s, keys, M, complete, counts, used);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_tsdf_mesh_vertices(const long* keys, long M, const float* f, const float* weight, const unsigned char* rgba,
                                        const unsigned char* used, const long* first_vertex, long V, float voxel, float* vertices_out,
                                        unsigned char* rgba_out, float* weight_out, void* stream) {
    const char* who = "tsdf_mesh_vertices";
    if (!keys || !f || !weight || !used || !first_vertex || !vertices_out || !weight_out || (rgba_out && !rgba))
        return refuse(who, "keys, f, weight, used, first_vertex, vertices_out and weight_out are required, and rgba with rgba_out");
    if (!rows_ok(M) || V < 0 || V > M) return refuse(who, "need 0 <= M < 2^31 and 0 <= V <= M");
    if (!voxel_ok(voxel)) return refuse(who, "voxel must be finite and > 0");
    if (M == 0 || V == 0) return GEO4D_OK;
    hipLaunchKernelGGL(tsdf_mesh_vertices_kernel, dim3(blocks_of(M)), dim3(256), 0, (hipStream_t)stream, keys, M, f, weight, rgba, used,
                       first_vertex, V, voxel, vertices_out, rgba_out, weight_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_tsdf_mesh_faces(const long* keys, long M, const float* f, const unsigned char* complete, const int* counts,
                                     const long* first_quad, const long* first_vertex, long Q, long V, int* faces_out, void* stream) {
    const char* who = "tsdf_mesh_faces";
    if (!keys || !f || !complete || !counts || !first_quad || !first_vertex || !faces_out)
        return refuse(who, "keys, f, complete, counts, first_quad, first_vertex and faces_out are required");
    if (!rows_ok(M) || Q < 0 || Q > 3 * M || V < 0 || V > M) return refuse(who, "need 0 <= M < 2^31, 0 <= Q <= 3 M and 0 <= V <= M");
    if (M == 0 || Q == 0) return GEO4D_OK;
    hipLaunchKernelGGL(tsdf_mesh_faces_kernel, dim3(blocks_of(M)), dim3(256), 0, (hipStream_t)stream, keys, M, f, complete, counts, first_quad,
                       first_vertex, Q, V, faces_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
