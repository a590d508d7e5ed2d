// geo4d_amd/csrc/mesh_components.hip — the connected pieces of an indexed triangle mesh, and the mesh of a chosen set of faces
// (geo4d_amd/mesh.py, ops.mesh_components, ops.mesh_select): what removes the detached debris a TSDF of noisy depth leaves.
//
// The reference has no such step; nothing is ported. The rule is the project's own and is stated here, in include/geo4d_hip.h and, in
// numpy, in tests/mesh_components_restatement.py. Everything is integer arithmetic: every output is a function of the inputs alone,
// whatever the order of the faces' threads.
//
// Inputs: faces int32 [T][3], the vertex count Nv, face_mask u8 [T] (NULL: every face).
// valid:  face t is valid iff face_mask[t] != 0 (or there is no mask) and its three indices lie in [0, Nv): decided before anything is
//   read or written through them. A valid face may repeat an index: (a, a, b) connects a and b, (a, a, a) touches a alone.
// joined: two vertices are connected iff a chain of valid faces links them, consecutive faces sharing at least one vertex (vertex
//   connectivity, not edge connectivity).
// labels: a vertex no valid face names is untouched: vertex_component = -1. Every other vertex is in exactly one component; a
//   component's root is its smallest vertex index; components are numbered 0 .. C - 1 in ascending order of root. face_component[t] is
//   the component of the face's vertices, -1 for a face that is not valid. component_vertices [C] and component_faces [C] count the
//   touched vertices and the valid faces.
// select: given keep_face u8 [T], face t is kept iff keep_face[t] != 0 and its indices lie in [0, Nv); a vertex is kept iff a kept face
//   names it. Kept vertices and kept faces keep their relative order; faces are rewritten to the new vertex rows; vertex_index [V'] is
//   the old row of every new one.
//
// Launches. hook: touched := 0, parent := identity, then one thread per face unions (i0, i1) and (i1, i2) in a lock-free union-find
//   (union_find.h, where the termination argument is) and stores touched = 1 for its vertices (plain byte stores of one value).
//   flatten (after hook has finished; parent is only read): root[v] = the root of v's chain, -1 for an untouched v, and
//   is_root[v] = (root[v] == v). The caller's cumsum over is_root gives first_component and C. count: component_* := 0, then
//   vertex_component and face_component by one writer per row, and the two counts by integer atomic adds, one add per wave where the
//   wave's lanes share a component. mark: keep_vertex := 0, then keep_vertex = 1 for the vertices of kept faces and kept[t] per
//   face; the caller's cumsum over both. gather: one writer per kept vertex and per kept face.
// limits: T < 2^31, Nv < 2^31; no LDS, no scratch.
#include "common.h"
#include "geo4d_hip.h"
#include "scene_view.h"
#include "union_find.h"

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

__global__ __launch_bounds__(256) void mesh_identity_kernel(int* __restrict__ parent, long Nv) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v < Nv) parent[v] = (int)v;
}

// no loop of this kernel waits for another thread: union_min and find_root (union_find.h) either finish or go on from a strictly
// smaller index, whatever the other threads do
__global__ __launch_bounds__(256) void mesh_hook_kernel(const int* __restrict__ faces, long T, long Nv, const unsigned char* __restrict__ mask,
                                                        int* parent, unsigned char* __restrict__ touched) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int i0, i1, i2;
    if (!valid_face(faces, t, Nv, mask, i0, i1, i2)) return;
    touched[i0] = 1;                                                                 // every writer of a byte stores the same value
    touched[i1] = 1;
    touched[i2] = 1;
    const int r = i0 != i1 ? union_min(parent, i0, i1) : i1;                         // i1's root, or i1: the next find starts there
    if (i1 != i2) union_min(parent, r, i2);
}

// hook has finished: parent is read only, with plain loads. The chain strictly descends (parent[x] < x for a non-root), so the walk
// ends after at most v steps.
__global__ __launch_bounds__(256) void mesh_flatten_kernel(const int* __restrict__ parent, const unsigned char* __restrict__ touched, long Nv,
                                                           int* __restrict__ root_out, unsigned char* __restrict__ is_root_out) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= Nv) return;
    int x = -1;
    if (touched[v]) {
        x = (int)v;
        for (int p = parent[x]; p < x; p = parent[x]) x = p;                         // p == x at a root; p > x never happens, and would end it
    }
    root_out[v] = x;
    is_root_out[v] = x == (int)v ? 1 : 0;
}

// counts[c] += 1 for every lane with c >= 0. Called by whole waves. Where the lanes that add share one component (the usual case: one
// piece holds almost every face) one lane adds their number; integer sums do not depend on the order, so both forms give the same counts.
// (One add per lane instead: the count launch 3.66 ms for 0.144 ms on the TSDF bench mesh and 268 ms for 4.2 ms on the 64-image sheets,
// profiles/mesh_components.md: every lane of the chip queues on a handful of words.)
__device__ __forceinline__ void count_into(int* __restrict__ counts, int c) {
    const unsigned long long adding = __ballot(c >= 0);
    if (!adding) return;
    const int leader = __ffsll((long long)adding) - 1;
    const int c0 = __shfl(c, leader);
    if (__ballot(c >= 0 && c != c0)) {
        if (c >= 0) atomicAdd(counts + c, 1);
    } else if ((int)(threadIdx.x & 63) == leader) {
        atomicAdd(counts + c0, (int)__popcll(adding));
    }
}

// the dense id of the component rooted at r (>= 0), -1 where first_component does not belong to this root array
__device__ __forceinline__ int dense_id(const long* __restrict__ first_component, int r, long C) {
    const long c = first_component[r];
    return c >= 0 && c < C ? (int)c : -1;
}

__global__ __launch_bounds__(256) void mesh_count_kernel(const int* __restrict__ faces, long T, long Nv, const unsigned char* __restrict__ mask,
                                                         const int* __restrict__ root, const long* __restrict__ first_component, long C,
                                                         int* __restrict__ vertex_component, int* __restrict__ face_component,
                                                         int* __restrict__ component_vertices, int* __restrict__ component_faces) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;                             // no early return: count_into is called by whole waves
    int cv = -1, cf = -1;
    if (i < Nv) {
        const int r = root[i];
        if (index_ok(r, Nv)) cv = dense_id(first_component, r, C);
        vertex_component[i] = cv;
    }
    if (i < T) {
        int i0, i1, i2;
        if (valid_face(faces, i, Nv, mask, i0, i1, i2)) {
            const int r = root[i0];
            if (index_ok(r, Nv)) cf = dense_id(first_component, r, C);
        }
        face_component[i] = cf;
    }
    count_into(component_vertices, cv);
    count_into(component_faces, cf);
}

__global__ __launch_bounds__(256) void mesh_mark_kernel(const int* __restrict__ faces, long T, long Nv, const unsigned char* __restrict__ keep_face,
                                                        unsigned char* __restrict__ keep_vertex, unsigned char* __restrict__ kept) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int i0, i1, i2;
    const bool ok = valid_face(faces, t, Nv, keep_face, i0, i1, i2);
    kept[t] = ok ? 1 : 0;
    if (!ok) return;
    keep_vertex[i0] = 1;                                                             // every writer of a byte stores the same value
    keep_vertex[i1] = 1;
    keep_vertex[i2] = 1;
}

__global__ __launch_bounds__(256) void mesh_gather_kernel(const float* __restrict__ vertices, const unsigned char* __restrict__ rgba,
                                                          const float* __restrict__ weight, const int* __restrict__ faces, long T, long Nv,
                                                          const unsigned char* __restrict__ keep_vertex, const unsigned char* __restrict__ kept,
                                                          const long* __restrict__ first_vertex, const long* __restrict__ first_face, long V,
                                                          long F, float* __restrict__ vertices_out, unsigned char* __restrict__ rgba_out,
                                                          float* __restrict__ weight_out, int* __restrict__ faces_out,
                                                          int* __restrict__ vertex_index) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < Nv && keep_vertex[i]) {
        const long row = first_vertex[i];
        if (row >= 0 && row < V) {                                                   // else not this mesh's offsets: nothing is written
            vertices_out[row * 3] = vertices[i * 3];
            vertices_out[row * 3 + 1] = vertices[i * 3 + 1];
            vertices_out[row * 3 + 2] = vertices[i * 3 + 2];
            if (rgba_out) *(unsigned*)(rgba_out + row * 4) = *(const unsigned*)(rgba + i * 4);
            if (weight_out) weight_out[row] = weight[i];
            vertex_index[row] = (int)i;
        }
    }
    if (i < T && kept[i]) {
        const long row = first_face[i];
        int i0, i1, i2;
        if (row < 0 || row >= F || !valid_face(faces, i, Nv, nullptr, i0, i1, i2)) return;
        const long n0 = first_vertex[i0], n1 = first_vertex[i1], n2 = first_vertex[i2];
        if (n0 < 0 || n0 >= V || n1 < 0 || n1 >= V || n2 < 0 || n2 >= V) return;
        faces_out[row * 3] = (int)n0;
        faces_out[row * 3 + 1] = (int)n1;
        faces_out[row * 3 + 2] = (int)n2;
    }
}

bool rows_ok(long n) { return n >= 0 && n < (1L << 31); }
unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

int zero(void* p, size_t bytes, hipStream_t s, const char* who) {
    if (hipMemsetAsync(p, 0, bytes, s) == hipSuccess) return GEO4D_OK;
    char msg[96];
    snprintf(msg, sizeof msg, "%s: hipMemsetAsync failed", who);
    geo4d_set_error(msg);
    return GEO4D_EIO;
}

}  // namespace

extern "C" int geo4d_mesh_components_hook(const int* faces, long T, long Nv, const unsigned char* face_mask, int* parent, unsigned char* touched,
                                          void* stream) {
    const char* who = "mesh_components_hook";
    if (!rows_ok(T) || !rows_ok(Nv)) return refuse(who, "need 0 <= T < 2^31 and 0 <= Nv < 2^31");
    if (!faces || !parent || !touched) return refuse(who, "faces, parent and touched are required");
    if (T == 0 || Nv == 0) return GEO4D_OK;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = zero(touched, (size_t)Nv, s, who)) return rc;
    hipLaunchKernelGGL(mesh_identity_kernel, dim3(blocks_of(Nv)), dim3(256), 0, s, parent, Nv);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_hook_kernel, dim3(blocks_of(T)), dim3(256), 0, s, faces, T, Nv, face_mask, parent, touched);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_mesh_components_flatten(const int* parent, const unsigned char* touched, long Nv, int* root_out,
                                             unsigned char* is_root_out, void* stream) {
    const char* who = "mesh_components_flatten";
    if (!rows_ok(Nv)) return refuse(who, "need 0 <= Nv < 2^31");
    if (!parent || !touched || !root_out || !is_root_out) return refuse(who, "parent, touched, root_out and is_root_out are required");
    if (Nv == 0) return GEO4D_OK;
    hipLaunchKernelGGL(mesh_flatten_kernel, dim3(blocks_of(Nv)), dim3(256), 0, (hipStream_t)stream, parent, touched, Nv, root_out, is_root_out);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_mesh_components_count(const int* faces, long T, long Nv, const unsigned char* face_mask, const int* root,
                                           const long* first_component, long C, int* vertex_component, int* face_component,
                                           int* component_vertices, int* component_faces, void* stream) {
    const char* who = "mesh_components_count";
    if (!rows_ok(T) || !rows_ok(Nv) || C < 0 || C > Nv) return refuse(who, "need 0 <= T < 2^31, 0 <= Nv < 2^31 and 0 <= C <= Nv");
    if (!faces || !root || !first_component || !vertex_component || !face_component || !component_vertices || !component_faces)
        return refuse(who, "faces, root, first_component and the four outputs are required");
    if (T == 0 || Nv == 0 || C == 0) return GEO4D_OK;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = zero(component_vertices, (size_t)C * sizeof(int), s, who)) return rc;
    if (int rc = zero(component_faces, (size_t)C * sizeof(int), s, who)) return rc;
    hipLaunchKernelGGL(mesh_count_kernel, dim3(blocks_of(T > Nv ? T : Nv)), dim3(256), 0, s, faces, T, Nv, face_mask, root, first_component, C,
                       vertex_component, face_component, component_vertices, component_faces);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_mesh_select_mark(const int* faces, long T, long Nv, const unsigned char* keep_face, unsigned char* keep_vertex,
                                      unsigned char* kept_face, void* stream) {
    const char* who = "mesh_select_mark";
    if (!rows_ok(T) || !rows_ok(Nv)) return refuse(who, "need 0 <= T < 2^31 and 0 <= Nv < 2^31");
    if (!faces || !keep_face || !keep_vertex || !kept_face) return refuse(who, "faces, keep_face, keep_vertex and kept_face are required");
    if (T == 0 || Nv == 0) return GEO4D_OK;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = zero(keep_vertex, (size_t)Nv, s, who)) return rc;
    hipLaunchKernelGGL(mesh_mark_kernel, dim3(blocks_of(T)), dim3(256), 0, s, faces, T, Nv, keep_face, keep_vertex, kept_face);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

extern "C" int geo4d_mesh_select_gather(const float* vertices, const unsigned char* rgba, const float* weight, const int* faces, long T, long Nv,
                                        const unsigned char* keep_vertex, const unsigned char* kept_face, const long* first_vertex,
                                        const long* first_face, long V, long F, float* vertices_out, unsigned char* rgba_out, float* weight_out,
                                        int* faces_out, int* vertex_index, void* stream) {
    const char* who = "mesh_select_gather";
    if (!rows_ok(T) || !rows_ok(Nv) || V < 0 || V > Nv || F < 0 || F > T)
        return refuse(who, "need 0 <= T < 2^31, 0 <= Nv < 2^31, 0 <= V' <= Nv and 0 <= T' <= T");
    if (!vertices || !faces || !keep_vertex || !kept_face || !first_vertex || !first_face || !vertices_out || !faces_out || !vertex_index ||
        (rgba_out && !rgba) || (weight_out && !weight))
        return refuse(who, "vertices, faces, the two masks, the two prefix sums and the outputs are required, and rgba / weight with their outputs");
    if (V == 0 || F == 0) return GEO4D_OK;                                           // a kept face names kept vertices, and the other way round
    hipLaunchKernelGGL(mesh_gather_kernel, dim3(blocks_of(T > Nv ? T : Nv)), dim3(256), 0, (hipStream_t)stream, vertices, rgba, weight, faces,
                       T, Nv, keep_vertex, kept_face, first_vertex, first_face, V, F, vertices_out, rgba_out, weight_out, faces_out,
                       vertex_index);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
