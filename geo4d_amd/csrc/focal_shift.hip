// geo4d_amd/csrc/focal_shift.hip — z-shift and focal of a point map from the map alone, batched over maps.
//
// Replaces utils.geometry.point_map_to_depth -> solve_optimal_shift_focal(..., ransac_iters=None) (utils/geometry.py:162-270), which the
// reference's shipped initialisation (init_im_poses.align_group_prefix :244-271) runs on the host: G x H x W x 3 floats copied off the
// device, then scipy.optimize.least_squares(method="lm", x0 = 0) per window. For map b, over the selected pixels i:
//     E(s) = sum_i | f p_i - uv_i |^2,   p_i = xy_i / (z_i + s),   f = A / B,   A = sum p.uv,   B = sum p.p       (f eliminated)
//          = U - A^2 / B,                U = sum |uv|^2
// With w = 1 / (z + s): p' = -w p, p'' = 2 w^2 p, so A' = -sum w p.uv, B' = -2 sum w p.p, A'' = 2 sum w^2 p.uv, B'' = 6 sum w^2 p.p:
// ONE pass over the pixels at a trial shift gives E and its first and second derivative there (and the Gauss-Newton curvature
// J.J = f'^2 B + f f' B' + f^2 sum w^2 p.p of the residual vector, used where E'' <= 0).
//
// One solver iteration = two launches: focal_shift_sums_kernel (grid = chunks x maps; 9 running sums per lane in fp64 -> wave shuffle ->
// LDS -> one partial row per block in the workspace) and focal_shift_step_kernel (one block per map: fixed-order combine of the partial
// rows, then one thread takes the decision). The decision is a safeguarded Newton step from shift 0: the trial is ACCEPTED only if E
// decreased (otherwise the step from the last accepted point is quartered), and a trial never leaves z_i + s > 0 for the selected pixel of
// smallest z - so the iteration walks downhill inside the basin that contains its start, like the reference's Levenberg-Marquardt, and
// ends on that basin's minimiser (the reference stops at ftol = 1e-3). All state lives in the workspace; the iteration count is fixed by
// the caller; a converged map is frozen (its blocks skip the pixel loop), nothing is read by the host in between.
// HBM/L2-bound: 12 (+4 with a weight) bytes per selected-or-not pixel per pass; uv is recomputed from the pixel index.
#include <cmath>
#include "common.h"
#include "geo4d_hip.h"

namespace {

// sums of one pass: 0 A = sum p.uv | 1 B = sum p.p | 2 sum w p.uv | 3 sum w p.p | 4 sum w^2 p.p | 5 sum w^2 p.uv | 6 U = sum |uv|^2 |
// 7 number of selected pixels | 8 min z over them (a min, not a sum)
constexpr int NS = 9;
constexpr int K_ZMIN = 8;
// per-map state (doubles) at the head of the workspace
enum { S_SHIFT = 0, S_E, S_FOCAL, S_GH, S_H, S_GSCALE, S_ALPHA, S_TRIAL, S_PHASE, S_STATUS, S_STATE };
constexpr double PH_FIRST = 0.0, PH_RUN = 1.0, PH_FROZEN = 2.0;
constexpr long CHUNK = 4096;       // pixels per block and pass (16 per thread)
constexpr int MAX_CHUNKS = 64;

__host__ __device__ inline int fs_chunks(long n) {
    const long c = (n + CHUNK - 1) / CHUNK;
    return c < 1 ? 1 : (c > MAX_CHUNKS ? MAX_CHUNKS : (int)c);
}

// source index of F.interpolate(mode="nearest"): min(floor(dst * (float)in / out), in - 1), the scale held in float like ATen's
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) { return min((int)floorf((float)dst * scale), in - 1); }

__global__ __launch_bounds__(64) void focal_shift_init_kernel(double* __restrict__ state, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double* st = state + (long)b * S_STATE;
    st[S_SHIFT] = 0.0; st[S_E] = 0.0; st[S_FOCAL] = 1.0; st[S_GH] = 0.0; st[S_H] = 1.0; st[S_GSCALE] = 0.0; st[S_ALPHA] = 1.0;
    st[S_TRIAL] = 0.0; st[S_PHASE] = PH_FIRST; st[S_STATUS] = 0.0;
}

__global__ __launch_bounds__(256) void focal_shift_sums_kernel(const float* __restrict__ pts, long map_stride, const float* __restrict__ weight,
                                                               long weight_stride, float thr, const float* __restrict__ z_offset, int H, int W,
                                                               int h_lr, int w_lr, int nchunk, const double* __restrict__ state,
                                                               double* __restrict__ part) {
    __shared__ double red[4][NS];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const double* st = state + (long)b * S_STATE;
    const bool live = st[S_PHASE] != PH_FROZEN;            // block-uniform: a frozen map skips the loop, not the barrier
    const double shift = st[S_TRIAL];
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    acc[K_ZMIN] = INFINITY;
    if (live) {
        const long n = (long)h_lr * w_lr;
        const long per = (n + nchunk - 1) / nchunk;
        const long i0 = chunk * per, i1 = min(n, i0 + per);
        const float sy = (float)H / (float)h_lr, sx = (float)W / (float)w_lr;
        const float zoff = z_offset ? z_offset[0] : 0.f;
        // image_plane_uv: u_x = span_x (2 x - (W - 1)) / W with span_x = W / diagonal, i.e. (2 x - (W - 1)) / diagonal; v alike
        const double inv_diag = 1.0 / sqrt((double)H * H + (double)W * W);
        const float* pb = pts + (long)b * map_stride;
        const float* wb = weight ? weight + (long)b * weight_stride : nullptr;
        for (long i = i0 + tid; i < i1; i += 256) {
            const int yl = (int)(i / w_lr), xl = (int)(i - (long)yl * w_lr);
            const int y = nearest_src(yl, sy, H), x = nearest_src(xl, sx, W);
            const long off = (long)y * W + x;
            if (wb && !(wb[off] > thr)) continue;
            const float* p3 = pb + off * 3;
            const double px = p3[0], py = p3[1], z = (double)(p3[2] + zoff);
            const double u = (double)(2 * x - (W - 1)) * inv_diag, v = (double)(2 * y - (H - 1)) * inv_diag;
            const double w = 1.0 / (z + shift);
            const double qx = px * w, qy = py * w;
            const double puv = qx * u + qy * v, pp = qx * qx + qy * qy;
            acc[0] += puv; acc[1] += pp;
            acc[2] += w * puv; acc[3] += w * pp;
            acc[4] += w * w * pp; acc[5] += w * w * puv;
            acc[6] += u * u + v * v; acc[7] += 1.0;
            acc[K_ZMIN] = fmin(acc[K_ZMIN], z);
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_down(v, o);
            v = k == K_ZMIN ? fmin(v, other) : v + other;
        }
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (live && tid < NS) {
        const double r0 = red[0][tid], r1 = red[1][tid], r2 = red[2][tid], r3 = red[3][tid];
        part[((long)b * nchunk + chunk) * NS + tid] = tid == K_ZMIN ? fmin(fmin(r0, r1), fmin(r2, r3)) : ((r0 + r1) + r2) + r3;
    }
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.79e308; }           // false for NaN and +-inf

__global__ __launch_bounds__(64) void focal_shift_step_kernel(const double* __restrict__ part, int nchunk, double* __restrict__ state,
                                                              float* __restrict__ shift_out, float* __restrict__ focal_out,
                                                              int* __restrict__ status_out) {
    __shared__ double sum[NS];
    const int b = blockIdx.x, tid = threadIdx.x;
    double* st = state + (long)b * S_STATE;
    const bool live = st[S_PHASE] != PH_FROZEN;
    if (live && tid < NS) {
        double v = tid == K_ZMIN ? INFINITY : 0.0;
        for (int c = 0; c < nchunk; ++c) {                                                      // fixed order
            const double x = part[((long)b * nchunk + c) * NS + tid];
            v = tid == K_ZMIN ? fmin(v, x) : v + x;
        }
        sum[tid] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    if (live) {
        const double trial = st[S_TRIAL], zmin = sum[K_ZMIN];
        const bool first = st[S_PHASE] == PH_FIRST;
        bool done = false, evaluated = true;
        if (!(sum[7] >= 3.0)) {                                            // two unknowns: fewer than 3 pixels do not determine them
            st[S_STATUS] = 1.0; st[S_SHIFT] = 0.0; st[S_FOCAL] = 1.0;
            done = true; evaluated = false;
        } else if (first && !(zmin + trial > 0.0)) {
            // shift 0 leaves a selected pixel at or behind the camera plane (or z is not finite): restart from the smallest feasible
            // offset, zmin + s = 1 (the start the reference keeps commented out, geometry.py:243)
            if (finite_d(zmin) && trial == 0.0) st[S_TRIAL] = 1.0 - zmin;
            else { st[S_STATUS] = 2.0; done = true; }
            evaluated = false;
        }
        if (evaluated) {
            const double A = sum[0], Bs = sum[1];
            const double f = A / Bs;
            const double E = sum[6] - A * f;
            const double Ap = -sum[2], Bp = -2.0 * sum[3], App = 2.0 * sum[5], Bpp = 6.0 * sum[4];
            const double fp = (Ap - f * Bp) / Bs;
            const double gh = -(f * Ap) + 0.5 * f * f * Bp;                                             // E' / 2
            const double h_newton = -(fp * Ap + f * App - f * fp * Bp - 0.5 * f * f * Bpp);           // E'' / 2
            const double h_gn = fp * fp * Bs + f * fp * Bp + f * f * sum[4];                          // J.J
            const bool ok = Bs > 0.0 && finite_d(E) && finite_d(f) && finite_d(gh) && finite_d(h_newton) && finite_d(h_gn);
            bool accept;
            if (first) {
                accept = ok;
                if (!ok) { st[S_STATUS] = 2.0; done = true; }
            } else {
                accept = ok && E < st[S_E];
            }
            if (accept) {
                st[S_SHIFT] = trial; st[S_E] = E; st[S_FOCAL] = f; st[S_GH] = gh; st[S_H] = h_newton > 0.0 ? h_newton : h_gn;
                st[S_GSCALE] = fabs(f * Ap) + 0.5 * f * f * fabs(Bp);
                st[S_ALPHA] = 1.0; st[S_PHASE] = PH_RUN;
            } else if (!done) {
                st[S_ALPHA] *= 0.25;
            }
            if (!done) {
                // propose the next trial from the last accepted point
                const double s = st[S_SHIFT], g = st[S_GH], Hc = st[S_H], alpha = st[S_ALPHA];
                if (!(Hc > 0.0) || fabs(g) <= 1e-14 * st[S_GSCALE] || alpha < 1e-12) {
                    done = true;                                        // flat (shift unobservable) / gradient at rounding level / no descent left
                } else {
                    double t = s - g / Hc * alpha;
                    if (!(zmin + t > 0.0)) t = s - 0.5 * (zmin + s);    // stay in front of the nearest selected pixel: halve its depth at most
                    if (!(fabs(t - s) > 1e-11 * (zmin + s))) done = true;
                    else st[S_TRIAL] = t;
                }
            }
        }
        if (done) {
            st[S_PHASE] = PH_FROZEN;
            const double f = st[S_FOCAL];
            if (st[S_STATUS] == 0.0 && !(f > 0.0 && finite_d(f))) st[S_STATUS] = 2.0;
        }
    }
    // outputs are rewritten after every iteration, so the last launch leaves the answer whatever the iteration count was
    const double s = st[S_SHIFT], f = st[S_FOCAL];
    int status = (int)st[S_STATUS];
    const bool s_ok = fabs(s) < 3.0e38, f_ok = fabs(f) < 3.0e38;           // representable as fp32 (false for NaN)
    if (status == 0 && !(f > 0.0 && f_ok && s_ok)) status = 2;
    if (status == 0 && st[S_PHASE] == PH_FIRST) status = 2;              // never evaluated (iteration count too small)
    shift_out[b] = s_ok ? (float)s : 0.f;
    focal_out[b] = f_ok ? (float)f : 1.f;
    status_out[b] = status;
}

}  // namespace

extern "C" size_t geo4d_focal_shift_workspace(int B, int h_lr, int w_lr) {
    if (B <= 0 || h_lr <= 0 || w_lr <= 0) return 0;
    return ((size_t)B * S_STATE + (size_t)B * fs_chunks((long)h_lr * w_lr) * NS) * sizeof(double);
}

extern "C" int geo4d_focal_shift(const float* points, long map_stride, const float* weight, long weight_stride, float thr, const float* z_offset,
                                 int B, int H, int W, int h_lr, int w_lr, int iters, float* shift, float* focal, int* status, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!points || !shift || !focal || !status || !workspace || B <= 0 || B > 65535 || H <= 0 || W <= 0 || h_lr <= 0 || w_lr <= 0 || iters <= 0 ||
        std::isnan(thr)) {
        geo4d_set_error("focal_shift: bad arguments");
        return GEO4D_EINVAL;
    }
    if ((long)H * W > (1L << 30)) { geo4d_set_error("focal_shift: map too large"); return GEO4D_EINVAL; }
    if (workspace_bytes < geo4d_focal_shift_workspace(B, h_lr, w_lr) || ((uintptr_t)workspace & 7)) {
        geo4d_set_error("focal_shift: workspace too small / unaligned");
        return GEO4D_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = fs_chunks((long)h_lr * w_lr);
    double* state = (double*)workspace;
    double* part = state + (size_t)B * S_STATE;
    hipLaunchKernelGGL(focal_shift_init_kernel, dim3((B + 63) / 64), dim3(64), 0, s, state, B);
    GEO4D_CHECK_LAUNCH();
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(focal_shift_sums_kernel, dim3(nchunk, B), dim3(256), 0, s, points, map_stride, weight, weight_stride, thr, z_offset, H, W,
                           h_lr, w_lr, nchunk, (const double*)state, part);
        GEO4D_CHECK_LAUNCH();
        hipLaunchKernelGGL(focal_shift_step_kernel, dim3(B), dim3(64), 0, s, (const double*)part, nchunk, state, shift, focal, status);
        GEO4D_CHECK_LAUNCH();
    }
    return GEO4D_OK;
}
