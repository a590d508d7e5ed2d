// Host build of geo4d_amd/csrc/pnp_math.h: the device RANSAC-PnP's arithmetic run serially for ONE image and ONE candidate focal, in the
// order the kernels of csrc/pnp.hip apply it (the six column pairs of a Jacobi round are all computed before any is applied, as the six
// lanes do). tests/test_pnp_device_cpu.py compiles this with the host compiler and compares it with geo4d_amd/pnp.py.
//   usage: pnp_math_host <input> ; input = int32 m, W, I | double f, cx, cy, reproj | double xs[m][3] | int32 pix[m] | int32 draws[I][6]
//   prints: ok it besti sub_inliers | R (9) t (3) | the I hypothesis counts
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pnp_math.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) return 2;
    int hdr[3];
    double par[4];
    if (std::fread(hdr, 4, 3, fp) != 3 || std::fread(par, 8, 4, fp) != 4) return 2;
    const int m = hdr[0], W = hdr[1], I = hdr[2];
    const double f = par[0], cx = par[1], cy = par[2], reproj = par[3];
    if (m < PNP_SAMPLE || m > (1 << 24) || W <= 0 || I <= 0 || I > (1 << 20)) return 2;
    std::vector<double> xs(3 * (size_t)m);
    std::vector<int> pix(m), draws(6 * (size_t)I), cnt(I);
    if (std::fread(xs.data(), 8, xs.size(), fp) != xs.size() || std::fread(pix.data(), 4, pix.size(), fp) != pix.size() ||
        std::fread(draws.data(), 4, draws.size(), fp) != draws.size())
        return 2;
    std::fclose(fp);
    std::vector<double> hyp(12 * (size_t)I);
    for (int h = 0; h < I; ++h) {
        double X[6][3], bb[6][3], M[24][PNP_LD], sig[12];
        for (int s = 0; s < 6; ++s) {
            const int j = draws[6 * h + s];
            if (j < 0 || j >= m) return 3;
            load_point(xs.data(), pix.data(), j, W, f, cx, cy, X[s], bb[s]);
        }
        for (int row = 0; row < 12; ++row) dlt_row(row, X[row >> 1], bb[row >> 1], M[row]);
        for (int row = 12; row < 24; ++row)
            for (int k = 0; k < 12; ++k) M[row][k] = k == row - 12 ? 1.0 : 0.0;
        for (int sweep = 0; sweep < 30; ++sweep) {
            bool any_rot = false;
            for (int r = 0; r < 11; ++r) {
                int p[6], q[6];
                double c[6], s[6];
                for (int k = 0; k < 6; ++k) {
                    dlt_pair(r, k, &p[k], &q[k]);
                    any_rot |= dlt_pair_rotation(M, p[k], q[k], &c[k], &s[k]);
                }
                for (int k = 0; k < 6; ++k)
                    for (int row = 0; row < 24; ++row) dlt_rotate_row(M[row], p[k], q[k], c[k], s[k]);
            }
            if (!any_rot) break;
        }
        for (int j = 0; j < 12; ++j) sig[j] = dlt_column_norm(M, j);
        double R[3][3], t[3];
        dlt_start_rotation(M, sig, R);
        oi6(X, bb, R, t);
        int count = 0;
        for (int j = 0; j < m; ++j) count += is_inlier(R, t, xs[3 * j], xs[3 * j + 1], xs[3 * j + 2], pix[j], W, f, cx, cy, reproj) ? 1 : 0;
        cnt[h] = count;
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) hyp[12 * h + 3 * r + k] = R[r][k];
            hyp[12 * h + 9 + r] = t[r];
        }
    }
    int it, besti, best;
    ransac_walk(cnt.data(), I, m, &it, &besti, &best);
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, t[3] = {0, 0, 0};
    int cur = 0;
    const bool ok = best >= PNP_SAMPLE;
    if (ok) {
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) R[r][k] = hyp[12 * besti + 3 * r + k];
            t[r] = hyp[12 * besti + 9 + r];
        }
        cur = best;
        for (int round = 0; round < 2; ++round) {
            double xm[3] = {0, 0, 0}, ninl = 0, acc[PNP_NMOM] = {0};
            for (int j = 0; j < m; ++j)
                if (is_inlier(R, t, xs[3 * j], xs[3 * j + 1], xs[3 * j + 2], pix[j], W, f, cx, cy, reproj)) {
                    xm[0] += xs[3 * j]; xm[1] += xs[3 * j + 1]; xm[2] += xs[3 * j + 2]; ninl += 1.0;
                }
            for (int k = 0; k < 3; ++k) xm[k] *= 1.0 / ninl;
            for (int j = 0; j < m; ++j)
                if (is_inlier(R, t, xs[3 * j], xs[3 * j + 1], xs[3 * j + 2], pix[j], W, f, cx, cy, reproj))
                    moments_add(acc, xs[3 * j], xs[3 * j + 1], xs[3 * j + 2], xm, pix[j], W, f, cx, cy);
            double R2[3][3], t2[3];
            for (int r = 0; r < 3; ++r)
                for (int k = 0; k < 3; ++k) R2[r][k] = R[r][k];
            refit_iterate(acc, ninl, xm, R2, t2);
            int c2 = 0;
            for (int j = 0; j < m; ++j) c2 += is_inlier(R2, t2, xs[3 * j], xs[3 * j + 1], xs[3 * j + 2], pix[j], W, f, cx, cy, reproj) ? 1 : 0;
            if (c2 < cur) break;
            cur = c2;
            for (int r = 0; r < 3; ++r) {
                for (int k = 0; k < 3; ++k) R[r][k] = R2[r][k];
                t[r] = t2[r];
            }
        }
    }
    std::printf("%d %d %d %d\n", ok ? 1 : 0, it, besti, cur);
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) std::printf("%.17g ", R[r][k]);
    for (int r = 0; r < 3; ++r) std::printf("%.17g ", t[r]);
    std::printf("\n");
    for (int h = 0; h < I; ++h) std::printf("%d ", cnt[h]);
    std::printf("\n");
    return 0;
}
