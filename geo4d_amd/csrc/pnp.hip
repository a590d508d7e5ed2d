// geo4d_amd/csrc/pnp.hip — batched RANSAC-PnP: B images x C candidate focals per call, mirroring geo4d_amd/pnp.py hypothesis for hypothesis.
//
// The host solver (fast_pnp -> solve_pnp_ransac -> pnp_orthogonal_iteration) runs once per image of every window at clip start-up: a full
// [H, W, 3] map copied off the device, then up to `iterations` 6-point solves and 2 x 500 refit steps per candidate focal in numpy. Here
// the same arithmetic runs in six launches per call, nothing read back; the sampler's index tables (numpy PCG64, pnp.sample_tables)
// are drawn on the host once per (n, iterations, seed) and uploaded.
//   1 pnp_compact_kernel     one workgroup per image: pixel indices with conf > thr in raster order (ballot ranks, no atomics), their
//                            number checked against the caller's n (the tables were drawn for THAT n), candidate focals checked
//   2 pnp_gather_kernel      the m <= max_points sub-sampled points (fp64) and their pixel index; a bearing is recomputed from the pixel
//                            index and the candidate's focal where it is used, so nothing is stored per candidate
//   3 pnp_hypothesis_kernel  one wave per (image, candidate, hypothesis): direct linear transform on the 6 samples (12 x 12 one-sided
//                            Jacobi SVD held in LDS, 6 disjoint column pairs per round), 15 orthogonal-iteration steps (every lane
//                            computes them redundantly: no broadcasts), then all 64 lanes score the m points -> inlier count
//   4 pnp_refit_kernel       one workgroup per (image, candidate): thread 0 walks the counts exactly as the host loop does (strictly
//                            greater = new best, adaptive stop), then two rounds of up to 500 orthogonal-iteration steps on the consensus
//                            set. The step is linear in (R, t) once the projectors V_i are fixed, so a round accumulates 60 moment sums
//                            of the CENTRED points once (sum V_i (x) X_i X_i^T, sum V_i (x) X_i, sum V_i) and iterates on those.
//   5 pnp_full_count_kernel  inliers over ALL masked pixels per candidate (chunk partials, integer)
//   6 pnp_final_kernel       one thread per image: first candidate with strictly the most inliers, camera-to-world, status, info.
// All solver arithmetic is fp64 and every reduction has a fixed order: two runs give identical bits. No kernel uses scratch: the small
// matrices live in registers behind fully unrolled loops, the 12 x 12 one in LDS.
#include <cmath>
#include "common.h"
#include "geo4d_hip.h"
#include "pnp_math.h"

namespace {

constexpr int SAMPLE = PNP_SAMPLE;
constexpr int MAX_CAND = 64;
constexpr int NMOM = PNP_NMOM;
enum { ST_FEW = 1, ST_NOCONS = 2, ST_FOCAL = 4, ST_TABLE = 8 };
constexpr long FC_CHUNK = 4096;
constexpr int FC_MAX_CHUNKS = 64;

inline int fc_chunks(long hw) {
    const long c = (hw + FC_CHUNK - 1) / FC_CHUNK;
    return c < 1 ? 1 : (c > FC_MAX_CHUNKS ? FC_MAX_CHUNKS : (int)c);
}

// workspace layout (byte offsets, every array 8-byte aligned)
struct Layout {
    size_t hyp, fit, xs, idx, pix, cnt, state, ok, part, total;
};
inline size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }
inline Layout make_layout(int B, int C, int H, int W, int I, int maxp) {
    Layout L;
    const size_t bc = (size_t)B * C, hw = (size_t)H * W;
    size_t o = 0;
    L.hyp = o;   o += bc * I * 12 * sizeof(double);                 // R (9) and t (3) of every hypothesis
    L.fit = o;   o += bc * 12 * sizeof(double);                     // refitted R, t
    L.xs = o;    o += (size_t)B * maxp * 3 * sizeof(double);        // sub-sampled points
    L.idx = o;   o += up8((size_t)B * hw * sizeof(int));            // masked pixel indices, raster order
    L.pix = o;   o += up8((size_t)B * maxp * sizeof(int));          // pixel index of every sub-sampled point
    L.cnt = o;   o += up8(bc * I * sizeof(int));                    // inlier count of every hypothesis
    L.state = o; o += up8((size_t)B * 2 * sizeof(int));             // per image: masked pixels found, m (0: skip)
    L.ok = o;    o += up8(bc * sizeof(int));                        // per (image, candidate): consensus found
    L.part = o;  o += up8(bc * fc_chunks((long)hw) * sizeof(int));  // full-count partials
    L.total = o;
    return L;
}

// ---- 1 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void pnp_compact_kernel(const float* __restrict__ conf, long conf_stride, float thr, int HW,
                                                           const int* __restrict__ n_in, const int* __restrict__ m_in, int maxp,
                                                           const double* __restrict__ cand, int C, int* __restrict__ idx, int* __restrict__ state,
                                                           int* __restrict__ status) {
    __shared__ unsigned wsum[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* cb = conf + (long)b * conf_stride;
    int* ib = idx + (long)b * HW;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned off = 0;
    for (int base = 0; base < HW; base += 1024) {
        const int e = base + tid;
        const bool keep = e < HW && cb[e] > thr;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wsum[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned pos = off + (unsigned)__popcll(bal & below), total = 0;
        for (int k = 0; k < 16; ++k) {
            if (k < wave) pos += wsum[k];
            total += wsum[k];
        }
        if (keep) ib[pos] = e;
        off += total;
        __syncthreads();
    }
    if (tid != 0) return;
    const int n = (int)off, m = m_in[b];
    int flags = 0;
    if (n < 4 || n < SAMPLE) flags |= ST_FEW;
    else if (n_in[b] != n || m < SAMPLE || m > n || m > maxp) flags |= ST_TABLE;        // the tables were drawn for another count
    for (int c = 0; c < C; ++c) {
        const double f = cand[(long)b * C + c];
        if (!(f > 0.0 && finite_d(f))) flags |= ST_FOCAL;
    }
    state[2 * b] = n;
    state[2 * b + 1] = flags ? 0 : m;
    status[b] = flags;
}

// ---- 2 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pnp_gather_kernel(const float* __restrict__ points, long image_stride, int HW, const int* __restrict__ sub,
                                                         int maxp, const int* __restrict__ idx, const int* __restrict__ state, double* __restrict__ xs,
                                                         int* __restrict__ pix, int* __restrict__ status) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int n = state[2 * b], m = state[2 * b + 1];
    if (j >= m) return;
    int r = sub[(long)b * maxp + j];
    if ((unsigned)r >= (unsigned)n) { atomicOr(&status[b], ST_TABLE); r = 0; }              // never index past the masked pixels
    const int p = idx[(long)b * HW + r];
    const float* p3 = points + (long)b * image_stride + 3 * (long)p;
    double* o = xs + ((long)b * maxp + j) * 3;
    o[0] = (double)p3[0]; o[1] = (double)p3[1]; o[2] = (double)p3[2];
    pix[(long)b * maxp + j] = p;
}

// ---- 3 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pnp_hypothesis_kernel(const double* __restrict__ cand, int C, int I, int W, double cx, double cy, double reproj,
                                                            const int* __restrict__ draws, int maxp, const double* __restrict__ xs_all,
                                                            const int* __restrict__ pix_all, const int* __restrict__ state, double* __restrict__ hyp,
                                                            int* __restrict__ cnt, int* __restrict__ status) {
    __shared__ double M[24][PNP_LD];                // rows 0..11: A of the DLT, rows 12..23: the accumulated right rotations
    __shared__ double sig[12];
    __shared__ double rcs[6][2];
    __shared__ int rpq[6][2];
    const int gid = blockIdx.x, lane = threadIdx.x;
    const int h = gid % I, bc = gid / I, b = bc / C;
    if (status[b] & ~ST_TABLE) return;                            // block-uniform
    const int m = state[2 * b + 1];
    if (m < SAMPLE) return;
    const double f = cand[bc];
    const double* xs = xs_all + (long)b * maxp * 3;
    const int* pix = pix_all + (long)b * maxp;
    const int* dr = draws + ((long)b * I + h) * SAMPLE;
    double X[6][3], bb[6][3];                                     // every lane holds all six samples: the solve is computed redundantly
    bool bad = false;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        int j = dr[s];
        if ((unsigned)j >= (unsigned)m) { bad = true; j = 0; }    // never index past the sub-sample
        load_point(xs, pix, j, W, f, cx, cy, X[s], bb[s]);
    }
    if (bad && lane == 0) atomicOr(&status[b], ST_TABLE);
    if (lane < 12) {
        int j = dr[lane >> 1];
        if ((unsigned)j >= (unsigned)m) j = 0;
        double Xi[3], bi[3];
        load_point(xs, pix, j, W, f, cx, cy, Xi, bi);
        dlt_row(lane, Xi, bi, M[lane]);
    } else if (lane < 24) {
        for (int k = 0; k < 12; ++k) M[lane][k] = k == lane - 12 ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int sweep = 0; sweep < 30; ++sweep) {
        int any_rot = 0;
        for (int r = 0; r < 11; ++r) {
            bool rot = false;
            if (lane < 6) {
                int p, q;
                double c, s;
                dlt_pair(r, lane, &p, &q);
                rot = dlt_pair_rotation(M, p, q, &c, &s);
                rcs[lane][0] = c; rcs[lane][1] = s; rpq[lane][0] = p; rpq[lane][1] = q;
            }
            any_rot |= __any(rot);
            __syncthreads();
            for (int e = lane; e < 144; e += 64) {                   // 6 pairs x 24 rows
                const int k = e / 24, row = e - 24 * k;
                dlt_rotate_row(M[row], rpq[k][0], rpq[k][1], rcs[k][0], rcs[k][1]);
            }
            __syncthreads();
        }
        if (!any_rot) break;
    }
    if (lane < 12) sig[lane] = dlt_column_norm(M, lane);
    __syncthreads();
    double R[3][3], t[3];
    dlt_start_rotation(M, sig, R);
    oi6(X, bb, R, t);
    // ---- consensus: every lane scores its share of the m points ---------------------------------------------------------------------
    int count = 0;
    for (int j = lane; j < m; j += 64)
        count += is_inlier(R, t, xs[3 * (long)j], xs[3 * (long)j + 1], xs[3 * (long)j + 2], pix[j], W, f, cx, cy, reproj) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
    if (lane == 0) {
        double* o = hyp + (long)gid * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int k = 0; k < 3; ++k) o[3 * r + k] = R[r][k];
            o[9 + r] = t[r];
        }
        cnt[gid] = count;
    }
}

// ---- 4 ---------------------------------------------------------------------------------------------------------------------------

// sums of K doubles over the 256 threads of a workgroup in a fixed order -> out[K] (LDS), visible to every thread on return
template <int K>
__device__ __forceinline__ void block_sum(double (&acc)[K], double (*red)[NMOM], double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) out[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    __syncthreads();
}

__global__ __launch_bounds__(256) void pnp_refit_kernel(const double* __restrict__ cand, int C, int I, int W, double cx, double cy, double reproj, int maxp,
                                                        const double* __restrict__ xs_all, const int* __restrict__ pix_all, const int* __restrict__ state,
                                                        const double* __restrict__ hyp, const int* __restrict__ cnt, const int* __restrict__ status,
                                                        double* __restrict__ fit, int* __restrict__ okf, int* __restrict__ info) {
    __shared__ double red[4][NMOM];
    __shared__ double mom[NMOM];
    __shared__ int sel[3];
    const int bc = blockIdx.x, b = bc / C, tid = threadIdx.x;
    int* inf = info + (long)bc * 4;
    const int m = state[2 * b + 1];
    if ((status[b] & ~ST_TABLE) || m < SAMPLE) {                     // block-uniform
        if (tid == 0) { okf[bc] = 0; inf[0] = 0; inf[1] = -1; inf[2] = 0; inf[3] = 0; }
        return;
    }
    if (tid == 0) {
        int it, besti, best;
        ransac_walk(cnt + (long)bc * I, I, m, &it, &besti, &best);
        sel[0] = it; sel[1] = besti; sel[2] = best;
    }
    __syncthreads();
    const int besti = sel[1];
    int cur_cnt = sel[2];
    if (cur_cnt < SAMPLE) {
        if (tid == 0) { okf[bc] = 0; inf[0] = sel[0]; inf[1] = besti; inf[2] = 0; inf[3] = 0; }
        return;
    }
    const double f = cand[bc];
    const double* xs = xs_all + (long)b * maxp * 3;
    const int* pix = pix_all + (long)b * maxp;
    double R[3][3], t[3];
    {
        const double* hp = hyp + ((long)bc * I + besti) * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int k = 0; k < 3; ++k) R[r][k] = hp[3 * r + k];
            t[r] = hp[9 + r];
        }
    }
    for (int round = 0; round < 2; ++round) {
        // the consensus set is re-derived from the current (R, t) wherever it is needed instead of being stored. The compiler may contract
        // multiply-adds differently in each inlined copy of is_inlier, so a point within rounding of the threshold could fall on the other
        // side here than where it was counted: the refit then runs on a set one such point larger or smaller (it is re-scored below either
        // way), which is why ninl is taken from THIS pass and not from the count.
        double a4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = tid; j < m; j += 256) {
            const double x = xs[3 * (long)j], y = xs[3 * (long)j + 1], z = xs[3 * (long)j + 2];
            if (is_inlier(R, t, x, y, z, pix[j], W, f, cx, cy, reproj)) { a4[0] += x; a4[1] += y; a4[2] += z; a4[3] += 1.0; }
        }
        block_sum<4>(a4, red, mom);
        const double ninl = mom[3], wn = 1.0 / ninl;
        const double xm[3] = {mom[0] * wn, mom[1] * wn, mom[2] * wn};
        __syncthreads();                                               // mom is rewritten below
        double acc[NMOM];
#pragma unroll
        for (int k = 0; k < NMOM; ++k) acc[k] = 0.0;
        for (int j = tid; j < m; j += 256) {
            const double x = xs[3 * (long)j], y = xs[3 * (long)j + 1], z = xs[3 * (long)j + 2];
            const int p = pix[j];
            if (!is_inlier(R, t, x, y, z, p, W, f, cx, cy, reproj)) continue;
            moments_add(acc, x, y, z, xm, p, W, f, cx, cy);
        }
        block_sum<NMOM>(acc, red, mom);
        // ---- up to 500 steps on the moments, every thread on the same numbers
        double R2[3][3], t2[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) R2[r][c] = R[r][c];
        refit_iterate(mom, ninl, xm, R2, t2);
        // ---- re-score on the sub-sample; keep only if no fewer inliers
        double c1[1] = {0.0};
        for (int j = tid; j < m; j += 256)
            c1[0] += is_inlier(R2, t2, xs[3 * (long)j], xs[3 * (long)j + 1], xs[3 * (long)j + 2], pix[j], W, f, cx, cy, reproj) ? 1.0 : 0.0;
        __syncthreads();                                               // every thread is done reading mom
        block_sum<1>(c1, red, mom);
        const int cnt2 = (int)mom[0];
        __syncthreads();
        if (cnt2 < cur_cnt) break;
        cur_cnt = cnt2;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) R[r][c] = R2[r][c];
            t[r] = t2[r];
        }
    }
    if (tid == 0) {
        bool fin = true;
        double* o = fit + (long)bc * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { o[3 * r + k] = R[r][k]; fin = fin && finite_d(R[r][k]); }
            o[9 + r] = t[r]; fin = fin && finite_d(t[r]);
        }
        okf[bc] = fin ? 1 : 0;
        inf[0] = sel[0]; inf[1] = besti; inf[2] = fin ? cur_cnt : 0; inf[3] = 0;
    }
}

// ---- 5 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pnp_full_count_kernel(const float* __restrict__ points, long image_stride, const float* __restrict__ conf,
                                                             long conf_stride, float thr, int HW, int W, const double* __restrict__ cand, int C, double cx,
                                                             double cy, double reproj, const double* __restrict__ fit, const int* __restrict__ okf,
                                                             int nchunk, int* __restrict__ part) {
    __shared__ int red[4];
    const int bc = blockIdx.y, b = bc / C, chunk = blockIdx.x, tid = threadIdx.x;
    int count = 0;
    if (okf[bc]) {                                                     // block-uniform
        double R[3][3], t[3];
        const double* fp = fit + (long)bc * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int k = 0; k < 3; ++k) R[r][k] = fp[3 * r + k];
            t[r] = fp[9 + r];
        }
        const double f = cand[bc];
        const int per = (HW + nchunk - 1) / nchunk;
        const int i0 = chunk * per, i1 = min(HW, i0 + per);
        const float* cb = conf + (long)b * conf_stride;
        const float* pb = points + (long)b * image_stride;
        for (int i = i0 + tid; i < i1; i += 256) {
            if (!(cb[i] > thr)) continue;
            const float* p3 = pb + 3 * (long)i;
            count += is_inlier(R, t, (double)p3[0], (double)p3[1], (double)p3[2], i, W, f, cx, cy, reproj) ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
    if ((tid & 63) == 0) red[tid >> 6] = count;
    __syncthreads();
    if (tid == 0) part[(long)bc * nchunk + chunk] = red[0] + red[1] + red[2] + red[3];
}

// ---- 6 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pnp_final_kernel(int B, int C, const double* __restrict__ cand, const double* __restrict__ fit,
                                                       const int* __restrict__ okf, int nchunk, const int* __restrict__ part, double* __restrict__ focal,
                                                       double* __restrict__ c2w, int* __restrict__ status, int* __restrict__ info) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int best = 0, bestc = -1;
    for (int c = 0; c < C; ++c) {
        const long bc = (long)b * C + c;
        int full = 0;
        for (int k = 0; k < nchunk; ++k) full += part[bc * nchunk + k];
        info[bc * 4 + 3] = full;
        if (okf[bc] && full > best) { best = full; bestc = c; }        // strictly more: ties go to the first candidate
    }
    int st = status[b];
    if (st == 0 && bestc < 0) st = ST_NOCONS;
    status[b] = st;
    if (st != 0) return;                                                // the caller's focal and pose survive a failure
    const double* fp = fit + ((long)b * C + bestc) * 12;
    double* M = c2w + (long)b * 16;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) M[4 * i + j] = fp[3 * j + i];      // inverse of the world->camera rigid transform: R^T, -R^T t
        M[4 * i + 3] = -(fp[i] * fp[9] + fp[3 + i] * fp[10] + fp[6 + i] * fp[11]);
    }
    M[12] = 0.0; M[13] = 0.0; M[14] = 0.0; M[15] = 1.0;
    focal[b] = cand[(long)b * C + bestc];
}

}  // namespace

extern "C" size_t geo4d_pnp_ransac_workspace(int B, int C, int H, int W, int iterations, int max_points) {
    if (B <= 0 || C <= 0 || C > MAX_CAND || H <= 0 || W <= 0 || iterations <= 0 || max_points < SAMPLE) return 0;
    return make_layout(B, C, H, W, iterations, max_points).total;
}

extern "C" int geo4d_pnp_ransac(const float* points, long image_stride, const float* conf, long conf_stride, float thr, const double* cand_focals,
                                double ppx, double ppy, double reproj, int iterations, int sample, const int* n, const int* m, const int* sub,
                                const int* draws, int max_points, int B, int C, int H, int W, double* focal, double* c2w, int* status, int* info,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (!points || !conf || !cand_focals || !n || !m || !sub || !draws || !focal || !c2w || !status || !info || !workspace || B <= 0 || B > 65535 ||
        C <= 0 || C > MAX_CAND || H <= 0 || W <= 0 || iterations <= 0 || sample != SAMPLE || max_points < SAMPLE || std::isnan(thr) ||
        std::isnan(reproj) || std::isnan(ppx) || std::isnan(ppy)) {
        geo4d_set_error("pnp_ransac: bad arguments (1 <= C <= 64, sample = 6, max_points >= 6)");
        return GEO4D_EINVAL;
    }
    if ((long)H * W > (1L << 30) || (long)B * C > 65535 || (long)B * C * iterations > (1L << 30) || max_points > (1 << 24)) {   // B C is a grid.y
        geo4d_set_error("pnp_ransac: problem too large");
        return GEO4D_EINVAL;
    }
    if (workspace_bytes < geo4d_pnp_ransac_workspace(B, C, H, W, iterations, max_points) || ((uintptr_t)workspace & 7)) {
        geo4d_set_error("pnp_ransac: workspace too small / unaligned");
        return GEO4D_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const Layout L = make_layout(B, C, H, W, iterations, max_points);
    char* ws = (char*)workspace;
    double *hyp = (double*)(ws + L.hyp), *fit = (double*)(ws + L.fit), *xs = (double*)(ws + L.xs);
    int *idx = (int*)(ws + L.idx), *pix = (int*)(ws + L.pix), *cnt = (int*)(ws + L.cnt), *state = (int*)(ws + L.state), *okf = (int*)(ws + L.ok),
        *part = (int*)(ws + L.part);
    const int HW = H * W, nchunk = fc_chunks(HW);
    hipLaunchKernelGGL(pnp_compact_kernel, dim3(B), dim3(1024), 0, s, conf, conf_stride, thr, HW, n, m, max_points, cand_focals, C, idx, state, status);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(pnp_gather_kernel, dim3((max_points + 255) / 256, B), dim3(256), 0, s, points, image_stride, HW, sub, max_points, (const int*)idx,
                       (const int*)state, xs, pix, status);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(pnp_hypothesis_kernel, dim3(B * C * iterations), dim3(64), 0, s, cand_focals, C, iterations, W, ppx, ppy, reproj, draws, max_points,
                       (const double*)xs, (const int*)pix, (const int*)state, hyp, cnt, status);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(pnp_refit_kernel, dim3(B * C), dim3(256), 0, s, cand_focals, C, iterations, W, ppx, ppy, reproj, max_points, (const double*)xs,
                       (const int*)pix, (const int*)state, (const double*)hyp, (const int*)cnt, (const int*)status, fit, okf, info);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(pnp_full_count_kernel, dim3(nchunk, B * C), dim3(256), 0, s, points, image_stride, conf, conf_stride, thr, HW, W, cand_focals, C,
                       ppx, ppy, reproj, (const double*)fit, (const int*)okf, nchunk, part);
    GEO4D_CHECK_LAUNCH();
    hipLaunchKernelGGL(pnp_final_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, C, cand_focals, (const double*)fit, (const int*)okf, nchunk,
                       (const int*)part, focal, c2w, status, info);
    GEO4D_CHECK_LAUNCH();
    return GEO4D_OK;
}
