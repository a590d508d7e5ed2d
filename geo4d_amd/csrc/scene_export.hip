// geo4d_amd/csrc/scene_export.hip — turning an aligned scene into what a user opens (dust3r/demo.py get_3D_model_from_scene :56-86).
//
// geo4d_scene_clean is clean_pointcloud (dust3r/cloud_opt/base_opt_group.py:630-665, the clean_depth option): for every ordered pair of
// images (i, j) project every pixel of i into camera j, round to a pixel, and clip i's confidence where i lies in front of j's depth
// and is less confident. The reference runs it as a dozen small torch launches per pair, updating res[i] in loop order: for j < i it
// compares against rows already cleaned, for j > i against rows not yet touched, and inside one i against the running res[i]. The
// form here keeps exactly that order: one launch per source image i (stream order), one thread per pixel of i looping j = 0 .. n-1,
// its confidence in a register and written once at the end. While launch i runs, rows j < i are final and rows j > i untouched, and
// row i itself is read by nobody, so the update is in place.
//
// geo4d_scene_points / geo4d_scene_mesh_faces are the two geometry branches of convert_scene_output_to_glb
// (dust3r/utils/viz_demo.py:25-34): pts3d[mask] with its colours, and the pts3d_to_trimesh + cat_meshes faces (dust3r/viz.py:40-90),
// both as order-preserving compactions (compact.h) so only the kept points / faces leave the device.
//
// Products and sums are written in the reference's order with contraction into FMAs switched off, as in depth_eval.hip.
#include <cmath>
#include "common.h"
#include "compact.h"
#include "geo4d_hip.h"
#include "scene_view.h"                                                              // dims_ok

#pragma clang fp contract(off)

namespace {

constexpr int MAT_FLOATS = 21;     // world-to-camera rows 0..2 (12) + intrinsics (9), row-major
constexpr int CLEAN_MATS = 256;    // matrices per LDS chunk: 21.5 KB

__global__ __launch_bounds__(256) void scene_clean_kernel(float* __restrict__ conf, const float* __restrict__ pts3d,
                                                          const float* __restrict__ depth, const float* __restrict__ mats, int n, int H,
                                                          int W, int i, float keep, float bad_conf) {
    __shared__ float sm[CLEAN_MATS * MAT_FLOATS];
    const long HW = (long)H * W;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = p < HW;
    float x = 0.f, y = 0.f, z = 0.f, c = 0.f;
    if (live) {
        const float* q = pts3d + ((long)i * HW + p) * 3;
        x = q[0]; y = q[1]; z = q[2];
        c = conf[(long)i * HW + p];
    }
    const float fW = (float)W, fH = (float)H;
    for (int j0 = 0; j0 < n; j0 += CLEAN_MATS) {
        const int m = min(CLEAN_MATS, n - j0);
        __syncthreads();
        for (int k = threadIdx.x; k < m * MAT_FLOATS; k += 256) sm[k] = mats[(long)j0 * MAT_FLOATS + k];
        __syncthreads();
        if (!live) continue;
        for (int jj = 0; jj < m; ++jj) {
            const int j = j0 + jj;
            if (j == i) continue;
            const float* M = sm + jj * MAT_FLOATS;
            // geotrf(cams[j], pts3d): pts @ cam[:3, :3]^T + cam[:3, 3]
            const float cx = x * M[0] + y * M[1] + z * M[2] + M[3];
            const float cy = x * M[4] + y * M[5] + z * M[6] + M[7];
            const float cz = x * M[8] + y * M[9] + z * M[10] + M[11];
            // geotrf(K[j], proj, norm=1, ncol=2): (proj @ K^T)[:2] / (proj @ K^T)[2], then torch.round (half to even)
            const float* K = M + 12;
            const float kx = cx * K[0] + cy * K[1] + cz * K[2];
            const float ky = cx * K[3] + cy * K[4] + cz * K[5];
            const float kz = cx * K[6] + cy * K[7] + cz * K[8];
            const float u = rintf(kx / kz), v = rintf(ky / kz);
            if (cz > 0.f && u >= 0.f && u < fW && v >= 0.f && v < fH) {      // NaN fails every test, as .long() of NaN does
                const long t = (long)j * HW + (long)v * W + (long)u;
                if (cz < keep * depth[t] && c < conf[t]) c = fminf(c, bad_conf);
            }
        }
    }
    if (live) conf[(long)i * HW + p] = c;
}

// pts3d[mask] and the matching colours, image-major raster order; RGBA u8 = io.save_glb's clip(c * 255 + 0.5, 0, 255) then truncation
struct PointsOp {
    const float* pts;
    const float* rgb;
    const unsigned char* mask;
    float* pts_out;
    unsigned* rgba_out;

    __device__ bool keep(long e) const { return !mask || mask[e]; }

    __device__ void emit(long e, unsigned pos) const {
        const float* q = pts + e * 3;
        float* o = pts_out + (long)pos * 3;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
        if (rgba_out) {
            const float* r = rgb + e * 3;
            rgba_out[pos] = quant_u8(r[0]) | (quant_u8(r[1]) << 8) | (quant_u8(r[2]) << 16) | (255u << 24);
        }
    }
};

// pts3d_to_trimesh's faces for every image, image-major: per image the blocks (tl, tr, bl), (bl, tr, tl), (tr, bl, br), (br, bl, tr),
// each over the (H-1) x (W-1) quads in raster order; a face is kept when its three vertices are valid; + i * H * W (cat_meshes)
struct FacesOp {
    const unsigned char* mask;
    int H, W;
    long Q;                 // quads per image
    int* faces;

    __device__ void corners(long e, long& base, long& a, long& b, long& c) const {
        const long img = e / (4 * Q), r = e - img * 4 * Q;
        const int blk = (int)(r / Q);
        const long q = r - blk * Q;
        const long qy = q / (W - 1), qx = q - qy * (W - 1);
        const long tl = qy * W + qx, tr = tl + 1, bl = tl + W, br = bl + 1;
        base = img * (long)H * W;
        switch (blk) {
            case 0: a = tl; b = tr; c = bl; break;
            case 1: a = bl; b = tr; c = tl; break;
            case 2: a = tr; b = bl; c = br; break;
            default: a = br; b = bl; c = tr; break;
        }
    }

    __device__ bool keep(long e) const {
        if (!mask) return true;
        long base, a, b, c;
        corners(e, base, a, b, c);
        return mask[base + a] && mask[base + b] && mask[base + c];
    }

    __device__ void emit(long e, unsigned pos) const {
        long base, a, b, c;
        corners(e, base, a, b, c);
        int* o = faces + (long)pos * 3;
        o[0] = (int)(base + a); o[1] = (int)(base + b); o[2] = (int)(base + c);
    }
};

template <class Op>
int run_compaction(const Op& op, long n, long* count, void* workspace, hipStream_t s) {
    const long nb = compact_tiles(n);
    unsigned* blk = (unsigned*)workspace;
    hipLaunchKernelGGL(compact_count_kernel<Op>, dim3((unsigned)nb), dim3(256), 0, s, op, n, blk);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, s, blk, nb, count);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(compact_scatter_kernel<Op>, dim3((unsigned)nb), dim3(256), 0, s, op, n, blk);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}

long n_faces_max(int n, int H, int W) { return 4L * n * (H - 1) * (W - 1); }

}  // namespace

extern "C" int geo4d_scene_clean(float* conf, const float* pts3d, const float* depth, const float* mats, int n, int H, int W, double tol,
                                 float bad_conf, void* stream) {
    if (!conf || !pts3d || !depth || !mats || !dims_ok(n, H, W) || !(tol >= 0.0 && tol < 1.0)) {
        geo4d_set_error("scene_clean: bad arguments (need device pointers, n, H, W > 0, n * H * W < 2^31, 0 <= tol < 1)");
        return GEO4D_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const float keep = (float)(1.0 - tol);                  // torch: the Python scalar (1 - tol) is cast to the tensor's fp32
    const int nb = (int)(((long)H * W + 255) / 256);
    for (int i = 0; i < n; ++i) {
        hipLaunchKernelGGL(scene_clean_kernel, dim3(nb), dim3(256), 0, s, conf, pts3d, depth, mats, n, H, W, i, keep, bad_conf);
        GEO4D_CHECK_LAUNCH();
    }
    return GEO4D_OK;
}

extern "C" size_t geo4d_scene_points_workspace(int n, int H, int W) {
    if (!dims_ok(n, H, W)) return 0;
    return (size_t)compact_tiles((long)n * H * W) * sizeof(unsigned);
}

extern "C" int geo4d_scene_points(const float* pts3d, const float* rgb, const unsigned char* mask, int n, int H, int W, float* pts_out,
                                  unsigned char* rgba_out, long* count, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pts3d || !pts_out || !count || !dims_ok(n, H, W) || (!rgb) != (!rgba_out) || !workspace ||
        workspace_bytes < geo4d_scene_points_workspace(n, H, W)) {
        geo4d_set_error("scene_points: bad arguments / workspace too small (rgb and rgba_out are both set or both NULL)");
        return GEO4D_EINVAL;
    }
    if ((size_t)rgba_out % 4 || (size_t)workspace % 4) {
        geo4d_set_error("scene_points: rgba_out and workspace must be 4-byte aligned");
        return GEO4D_EINVAL;
    }
    const PointsOp op{pts3d, rgb, mask, pts_out, (unsigned*)rgba_out};
    return run_compaction(op, (long)n * H * W, count, workspace, (hipStream_t)stream);
}

extern "C" size_t geo4d_scene_mesh_faces_workspace(int n, int H, int W) {
    if (!dims_ok(n, H, W) || H < 2 || W < 2) return 0;
    return (size_t)compact_tiles(n_faces_max(n, H, W)) * sizeof(unsigned);
}

extern "C" int geo4d_scene_mesh_faces(const unsigned char* mask, int n, int H, int W, int* faces, long* count, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    if (!faces || !count || !dims_ok(n, H, W) || H < 2 || W < 2 || n_faces_max(n, H, W) >= (1L << 32) || !workspace ||
        workspace_bytes < geo4d_scene_mesh_faces_workspace(n, H, W) || (size_t)workspace % 4) {
        geo4d_set_error("scene_mesh_faces: bad arguments / workspace too small (need H, W >= 2 and 4 n (H-1)(W-1) < 2^32)");
        return GEO4D_EINVAL;
    }
    const FacesOp op{mask, H, W, (long)(H - 1) * (W - 1), faces};
    return run_compaction(op, n_faces_max(n, H, W), count, workspace, (hipStream_t)stream);
}
