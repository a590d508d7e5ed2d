// geo4d_amd/csrc/pnp_math.h — the arithmetic of the batched RANSAC-PnP (csrc/pnp.hip) as plain functions of their arguments: no thread
// index, no shared memory, no intrinsic. The kernels call them; a host build of the same header (tests/pnp_math_host.cpp) runs the whole
// solve serially, so the maths is checked against geo4d_amd/pnp.py without a GPU. Every small matrix is indexed by constants behind fully
// unrolled loops (registers on the device, no scratch).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PNP_HD __host__ __device__ __forceinline__
#else
#define PNP_HD inline
#endif

namespace {

constexpr int PNP_SAMPLE = 6;
constexpr int PNP_HYP_ITERS = 15, PNP_REFIT_ITERS = 500;
constexpr double PNP_CONFIDENCE = 0.99;
constexpr int PNP_LD = 13;       // row stride of the 24 x 12 DLT work matrix (rows 0..11: A, rows 12..23: the accumulated right rotations)
constexpr int PNP_NMOM = 60;     // refit moments: 36 sum V_ab Xc_c Xc_d (symmetric in ab and in cd) | 18 sum V_ab Xc_c | 6 sum V_ab

PNP_HD bool finite_d(double v) { return fabs(v) <= 1.79e308; }           // false for NaN and +-inf

PNP_HD double det3(const double M[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

PNP_HD void inv3(const double A[3][3], double O[3][3]) {
    const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2], c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    const double id = 1.0 / (A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02);
    O[0][0] = c00 * id; O[1][0] = c01 * id; O[2][0] = c02 * id;
    O[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * id; O[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * id; O[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * id;
    O[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * id; O[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * id; O[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * id;
}

// Jacobi rotation that makes two columns with squared norms alpha, beta and inner product gamma orthogonal; false: already are
PNP_HD bool jacobi_cs(double alpha, double beta, double gamma, double* c, double* s) {
    *c = 1.0; *s = 0.0;
    if (!(fabs(gamma) > 2.3e-16 * sqrt(alpha * beta))) return false;          // (also false for NaN)
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    *c = 1.0 / sqrt(1.0 + tt * tt);
    *s = *c * tt;
    return true;
}

PNP_HD void swap_col(double M[3][3], int a, int b) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double x = M[k][a]; M[k][a] = M[k][b]; M[k][b] = x; }
}

// Rotation of a 3x3 H = U S V^T by a one-sided Jacobi SVD on H itself (singular vectors to full relative accuracy, planar point sets
// included). kabsch: R = U diag(1, 1, sign det(U V^T)) V^T (pnp._absolute_orientation). Otherwise R = U V^T, *neg = det(R) < 0 and
// *smean the mean singular value (the 3x3 block of pnp._dlt_pose). The third left vector is u0 x u1 with its sign restored from H v2.
PNP_HD void svd3_rotation(const double H[3][3], bool kabsch, double R[3][3], double* smean, bool* neg) {
    double G[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { G[i][j] = H[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rot = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double alpha = G[0][p] * G[0][p] + G[1][p] * G[1][p] + G[2][p] * G[2][p];
            const double beta = G[0][q] * G[0][q] + G[1][q] * G[1][q] + G[2][q] * G[2][q];
            const double gamma = G[0][p] * G[0][q] + G[1][p] * G[1][q] + G[2][p] * G[2][q];
            double c, s;
            if (jacobi_cs(alpha, beta, gamma, &c, &s)) {
                rot = true;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double gp = G[k][p], gq = G[k][q], vp = V[k][p], vq = V[k][q];
                    G[k][p] = c * gp - s * gq; G[k][q] = s * gp + c * gq;
                    V[k][p] = c * vp - s * vq; V[k][q] = s * vp + c * vq;
                }
            }
        }
        if (!rot) break;
    }
    double sg[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) sg[j] = sqrt(G[0][j] * G[0][j] + G[1][j] * G[1][j] + G[2][j] * G[2][j]);
    // singular values descending (three compare-and-swaps on the columns themselves: every index stays a constant)
    if (sg[0] < sg[1]) { swap_col(G, 0, 1); swap_col(V, 0, 1); const double x = sg[0]; sg[0] = sg[1]; sg[1] = x; }
    if (sg[0] < sg[2]) { swap_col(G, 0, 2); swap_col(V, 0, 2); const double x = sg[0]; sg[0] = sg[2]; sg[2] = x; }
    if (sg[1] < sg[2]) { swap_col(G, 1, 2); swap_col(V, 1, 2); const double x = sg[1]; sg[1] = sg[2]; sg[2] = x; }
    double u0[3], u1[3], u2[3];
    const double i0 = sg[0] > 0.0 ? 1.0 / sg[0] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) u0[k] = sg[0] > 0.0 ? G[k][0] * i0 : (k == 0 ? 1.0 : 0.0);
    const double pr = u0[0] * G[0][1] + u0[1] * G[1][1] + u0[2] * G[2][1];
#pragma unroll
    for (int k = 0; k < 3; ++k) u1[k] = G[k][1] - pr * u0[k];
    double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    if (!(n1 > 1e-300)) {                                      // rank <= 1: any unit vector orthogonal to u0 (the host's is arbitrary too)
        const double ax = fabs(u0[0]), ay = fabs(u0[1]), az = fabs(u0[2]);
        const double e0 = ax <= ay && ax <= az ? 1.0 : 0.0, e1 = e0 == 0.0 && ay <= az ? 1.0 : 0.0, e2 = 1.0 - e0 - e1;
        u1[0] = u0[1] * e2 - u0[2] * e1; u1[1] = u0[2] * e0 - u0[0] * e2; u1[2] = u0[0] * e1 - u0[1] * e0;
        n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) u1[k] /= n1;
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    const double detV = det3(V);
    double s3;
    if (kabsch) {
        s3 = detV >= 0.0 ? 1.0 : -1.0;                         // det [u0 u1 u2] = +1, so det(R) = s3 det(V) = +1
        *neg = false;
    } else {
        s3 = (G[0][2] * u2[0] + G[1][2] * u2[1] + G[2][2] * u2[2]) >= 0.0 ? 1.0 : -1.0;        // the SVD's own third left vector
        *neg = s3 * detV < 0.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = u0[i] * V[j][0] + u1[i] * V[j][1] + s3 * u2[i] * V[j][2];
    *smean = (sg[0] + sg[1] + sg[2]) / 3.0;
}

PNP_HD void load_point(const double* __restrict__ xs, const int* __restrict__ pix, int j, int W, double f, double cx, double cy,
                                           double X[3], double b[3]) {
    X[0] = xs[3 * (long)j]; X[1] = xs[3 * (long)j + 1]; X[2] = xs[3 * (long)j + 2];
    const int p = pix[j], v = p / W, u = p - v * W;                 // pnp.pixel_grid: x = column, y = row
    b[0] = ((double)u - cx) / f; b[1] = ((double)v - cy) / f; b[2] = 1.0;
}

// pnp.reprojection_error(...) < reproj for one point; points at or behind the camera are never inliers
PNP_HD bool is_inlier(const double R[3][3], const double t[3], double x, double y, double z, int p, int W, double f, double cx,
                                          double cy, double reproj) {
    const double xc = R[0][0] * x + R[0][1] * y + R[0][2] * z + t[0];
    const double yc = R[1][0] * x + R[1][1] * y + R[1][2] * z + t[1];
    const double zc = R[2][0] * x + R[2][1] * y + R[2][2] * z + t[2];
    const double zz = fabs(zc) < 1e-12 ? 1e-12 : zc;
    const int v = p / W, u = p - v * W;
    const double du = f * xc / zz + cx - (double)u, dv = f * yc / zz + cy - (double)v;
    return zc > 0.0 && sqrt(du * du + dv * dv) < reproj;
}


// pnp.pnp_orthogonal_iteration on six points, R given (the DLT's or the identity), t = None: every lane runs it on the same registers
PNP_HD void oi6(const double X[6][3], const double b[6][3], double R[3][3], double t[3]) {
    double bn[6][3], Xc[6][3], xm[3] = {0.0, 0.0, 0.0}, Vbar[3][3], A[3][3], Tfac[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Vbar[i][j] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double inv = 1.0 / sqrt(b[i][0] * b[i][0] + b[i][1] * b[i][1] + b[i][2] * b[i][2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) { bn[i][k] = b[i][k] * inv; xm[k] += X[i][k]; }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Vbar[r][c] += bn[i][r] * bn[i][c];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) xm[k] *= 1.0 / 6.0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) Xc[i][k] = X[i][k] - xm[k];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r][c] = (r == c ? 1.0 : 0.0) - Vbar[r][c] * (1.0 / 6.0);
    inv3(A, Tfac);
    auto t_of = [&](const double Rm[3][3], double to[3]) {
        double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double rx[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) rx[k] = Rm[k][0] * X[i][0] + Rm[k][1] * X[i][1] + Rm[k][2] * X[i][2];
            const double d = bn[i][0] * rx[0] + bn[i][1] * rx[1] + bn[i][2] * rx[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] += bn[i][k] * d - rx[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) to[k] = (Tfac[k][0] * s[0] + Tfac[k][1] * s[1] + Tfac[k][2] * s[2]) * (1.0 / 6.0);
    };
    t_of(R, t);
    for (int pass = 0; pass < 2; ++pass) {
        for (int it = 0; it < PNP_HYP_ITERS; ++it) {
            double Q[6][3], qm[3] = {0.0, 0.0, 0.0}, Hm[3][3], Rn[3][3], sm;
            bool ng;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double y[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) y[k] = R[k][0] * X[i][0] + R[k][1] * X[i][1] + R[k][2] * X[i][2] + t[k];
                const double d = bn[i][0] * y[0] + bn[i][1] * y[1] + bn[i][2] * y[2];
#pragma unroll
                for (int k = 0; k < 3; ++k) { Q[i][k] = bn[i][k] * d; qm[k] += Q[i][k]; }       // the point projected on its line of sight
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double s = 0.0;
#pragma unroll
                    for (int i = 0; i < 6; ++i) s += (Q[i][r] - qm[r] * (1.0 / 6.0)) * Xc[i][c];
                    Hm[r][c] = s * (1.0 / 6.0);
                }
            svd3_rotation(Hm, true, Rn, &sm, &ng);
            double dmax = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) { dmax = fmax(dmax, fabs(Rn[r][c] - R[r][c])); R[r][c] = Rn[r][c]; }
            t_of(R, t);
            if (dmax < 1e-13) break;
        }
        double zs = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) zs += R[2][0] * X[i][0] + R[2][1] * X[i][1] + R[2][2] * X[i][2] + t[2];
        if (pass == 1 || !(zs < 0.0)) break;
        // converged to the mirrored solution behind the camera: restart from its flip
#pragma unroll
        for (int c = 0; c < 3; ++c) { R[0][c] = -R[0][c]; R[1][c] = -R[1][c]; }
        t_of(R, t);
    }
}


// ---- pnp._dlt_pose: null vector of the 12 x 12 A by a one-sided Jacobi SVD on A itself (singular values to full relative accuracy, which
// the S[-2] < 1e-9 S[0] refusal needs), round-robin ordering: 11 rounds of 6 disjoint column pairs ------------------------------------
PNP_HD void dlt_row(int row, const double X[3], const double b[3], double* Mrow) {
    const bool odd = row & 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double xh = k < 3 ? X[k < 3 ? k : 0] : 1.0;
        Mrow[odd ? 4 + k : k] = xh * b[2];
        Mrow[odd ? k : 4 + k] = 0.0;
        Mrow[8 + k] = -xh * (odd ? b[1] : b[0]);
    }
}

PNP_HD void dlt_pair(int round, int k, int* p, int* q) {
    const int a = k == 0 ? 11 : (round + k) % 11, c = k == 0 ? round : (round + 11 - k) % 11;
    *p = a < c ? a : c;
    *q = a < c ? c : a;
}

PNP_HD bool dlt_pair_rotation(const double (*M)[PNP_LD], int p, int q, double* c, double* s) {
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
    for (int k = 0; k < 12; ++k) {
        const double x = M[k][p], y = M[k][q];
        alpha += x * x; beta += y * y; gamma += x * y;
    }
    return jacobi_cs(alpha, beta, gamma, c, s);
}

PNP_HD void dlt_rotate_row(double* Mrow, int p, int q, double c, double s) {
    const double x = Mrow[p], y = Mrow[q];
    Mrow[p] = c * x - s * y;
    Mrow[q] = s * x + c * y;
}

PNP_HD double dlt_column_norm(const double (*M)[PNP_LD], int j) {
    double s = 0.0;
    for (int k = 0; k < 12; ++k) s += M[k][j] * M[k][j];
    return sqrt(s);
}

// the rotation the orthogonal iteration starts from: the DLT's when it is well conditioned and proper, else the identity
PNP_HD void dlt_start_rotation(const double (*M)[PNP_LD], const double* sig, double R[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) R[r][k] = r == k ? 1.0 : 0.0;
    double smax = 0.0, smin = INFINITY, smin2 = INFINITY;
    int jmin = 0;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const double s = sig[j];
        smax = fmax(smax, s);
        if (s < smin) { smin2 = smin; smin = s; jmin = j; }
        else if (s < smin2) smin2 = s;
    }
    if (!(smin2 >= 1e-9 * smax)) return;                              // (also for NaN)
    double P3[3][3], Rd[3][3], sm;
    bool ng;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) P3[r][k] = M[12 + 4 * r + k][jmin];
    if (det3(P3) < 0.0) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) P3[r][k] = -P3[r][k];
    }
    svd3_rotation(P3, false, Rd, &sm, &ng);
    if (ng || !finite_d(sm)) return;                                  // (the DLT's translation is not used: the iteration starts at t = None)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) R[r][k] = Rd[r][k];
}

// ---- the host loop of solve_pnp_ransac over the hypothesis counts: strictly greater = new best, `needed` recomputed from the inlier
// ratio, stop at min(iterations, needed); hypotheses past the stop were computed but do not count ---------------------------------------
PNP_HD void ransac_walk(const int* cnt, int iterations, int m, int* it_out, int* besti_out, int* best_out) {
    int best = 0, besti = -1, it = 0;
    double needed = (double)iterations;
    while (it < iterations && (double)it < needed) {
        const int c = cnt[it];
        ++it;
        if (c > best) {
            best = c; besti = it - 1;
            const double ratio = (double)c / (double)m;
            const double p_all = pow(ratio, (double)PNP_SAMPLE);
            needed = p_all < 1e-9 ? INFINITY : (p_all >= 1.0 ? 0.0 : log(1.0 - PNP_CONFIDENCE) / log(1.0 - p_all));
        }
    }
    *it_out = it; *besti_out = besti; *best_out = best;
}

// ---- refit on the consensus set through moments of the CENTRED points. With V_i the projector on the i-th line of sight, Xc_i = X_i - mean,
// and t' = t + R mean: Q_i = V_i (R Xc_i + t'), H = mean Q_i Xc_i^T, t' = (I - mean V)^-1 mean V_i R Xc_i: all linear in (R, t') -----------
PNP_HD constexpr int sidx(int a, int b) { return a == b ? (a == 0 ? 0 : (a == 1 ? 3 : 5)) : (a + b == 1 ? 1 : (a + b == 2 ? 2 : 4)); }

PNP_HD void moments_add(double acc[PNP_NMOM], double x, double y, double z, const double xm[3], int p, int W, double f, double cx, double cy) {
    const int v = p / W, u = p - v * W;
    double bv[3] = {((double)u - cx) / f, ((double)v - cy) / f, 1.0};
    const double inv = 1.0 / sqrt(bv[0] * bv[0] + bv[1] * bv[1] + 1.0);
    bv[0] *= inv; bv[1] *= inv; bv[2] *= inv;
    const double xc[3] = {x - xm[0], y - xm[1], z - xm[2]};
    const double Vs[6] = {bv[0] * bv[0], bv[0] * bv[1], bv[0] * bv[2], bv[1] * bv[1], bv[1] * bv[2], bv[2] * bv[2]};
    const double XX[6] = {xc[0] * xc[0], xc[0] * xc[1], xc[0] * xc[2], xc[1] * xc[1], xc[1] * xc[2], xc[2] * xc[2]};
#pragma unroll
    for (int vi = 0; vi < 6; ++vi) {
#pragma unroll
        for (int xi = 0; xi < 6; ++xi) acc[6 * vi + xi] += Vs[vi] * XX[xi];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[36 + 3 * vi + c] += Vs[vi] * xc[c];
        acc[54 + vi] += Vs[vi];
    }
}

PNP_HD void moments_t(const double* mom, double wn, const double Tfac[3][3], const double Rm[3][3], double to[3]) {
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int c = 0; c < 3; ++c) s[a] += mom[36 + 3 * sidx(a, b) + c] * Rm[b][c];
#pragma unroll
    for (int k = 0; k < 3; ++k) to[k] = (Tfac[k][0] * s[0] + Tfac[k][1] * s[1] + Tfac[k][2] * s[2]) * wn;
}

// pnp_orthogonal_iteration(X[inl], b[inl], R = R, t = None, iters = 500) on the summed moments `mom` of ninl points with mean xm:
// R (in: start, out: result), t (out)
PNP_HD void refit_iterate(const double* mom, double ninl, const double xm[3], double R[3][3], double t[3]) {
    const double wn = 1.0 / ninl;
    double Tfac[3][3], A[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r][c] = (r == c ? 1.0 : 0.0) - mom[54 + sidx(r, c)] * wn;
    inv3(A, Tfac);
    moments_t(mom, wn, Tfac, R, t);
    for (int pass = 0; pass < 2; ++pass) {
        for (int it = 0; it < PNP_REFIT_ITERS; ++it) {
            double Hm[3][3], Rn[3][3], sm;
            bool ng;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    double s = 0.0;
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) s += R[b][c] * mom[6 * sidx(a, b) + sidx(c, d)];
                        s += t[b] * mom[36 + 3 * sidx(a, b) + d];
                    }
                    Hm[a][d] = s * wn;
                }
            svd3_rotation(Hm, true, Rn, &sm, &ng);
            double dmax = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) { dmax = fmax(dmax, fabs(Rn[r][c] - R[r][c])); R[r][c] = Rn[r][c]; }
            moments_t(mom, wn, Tfac, R, t);
            if (dmax < 1e-13) break;
        }
        if (pass == 1 || !(t[2] < 0.0)) break;                       // mean z of the transformed set = z of the centred translation
#pragma unroll
        for (int c = 0; c < 3; ++c) { R[0][c] = -R[0][c]; R[1][c] = -R[1][c]; }
        moments_t(mom, wn, Tfac, R, t);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] -= R[k][0] * xm[0] + R[k][1] * xm[1] + R[k][2] * xm[2];
}

}  // namespace
