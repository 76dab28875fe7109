// The host side of one point-to-point ICP alignment (pcl::IterativeClosestPoint::computeTransformation as icp.hip restates it):
// the rigid increment from the 17 correspondence sums, F = T * F, PCL's DefaultConvergenceCriteria.  One implementation for the
// single alignment (icp.hip) and the batched multiview refine (refine.hip), so that both walk the same ladder on the same numbers.
// The point-to-plane alignment (scal_icp_align_plane) takes its increment from the 6x6 normal equations instead and shares the rest.
#pragma once
#include <cmath>
#include <cstring>
#include <limits>

namespace scal {

// largest eigenpair of a symmetric 4x4 by cyclic Jacobi -> unit quaternion (w, x, y, z)
inline void eig4_max(double a[4][4], double q[4]) {
    double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0, diag = 0;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) (i == j ? diag : off) += a[i][j] * a[i][j];
        if (off <= 1e-40 * diag || off == 0.0) break;
        for (int p = 0; p < 3; ++p)
            for (int r = p + 1; r < 4; ++r) {
                if (a[p][r] == 0.0) continue;
                const double theta = (a[r][r] - a[p][p]) / (2.0 * a[p][r]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double akp = a[k][p], akr = a[k][r];
                    a[k][p] = c * akp - s * akr, a[k][r] = s * akp + c * akr;
                }
                for (int k = 0; k < 4; ++k) {
                    const double apk = a[p][k], ark = a[r][k];
                    a[p][k] = c * apk - s * ark, a[r][k] = s * apk + c * ark;
                }
                for (int k = 0; k < 4; ++k) {
                    const double vkp = v[k][p], vkr = v[k][r];
                    v[k][p] = c * vkp - s * vkr, v[k][r] = s * vkp + c * vkr;
                }
            }
    }
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (a[i][i] > a[best][best]) best = i;
    double nrm = 0;
    for (int k = 0; k < 4; ++k) nrm += v[k][best] * v[k][best];
    nrm = std::sqrt(nrm);
    for (int k = 0; k < 4; ++k) q[k] = v[k][best] / nrm;
}

// rigid increment (as the Matrix4f PCL keeps) from the correspondence sums: Horn's quaternion form of the Umeyama problem
inline void transform_from_sums(const double* sums, float* T) {
    const double n = sums[0];
    double mp[3], mq[3], S[3][3];
    for (int k = 0; k < 3; ++k) mp[k] = sums[1 + k] / n, mq[k] = sums[4 + k] / n;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) S[c][r] = sums[7 + 3 * r + c] / n - mq[r] * mp[c];
    double N[4][4] = {{S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
                      {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
                      {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
                      {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
    double q[4];
    eig4_max(N, q);
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    for (int r = 0; r < 3; ++r) {
        double t = mq[r];
        for (int c = 0; c < 3; ++c) {
            T[4 * r + c] = static_cast<float>(R[r][c]);
            t -= R[r][c] * mp[c];
        }
        T[4 * r + 3] = static_cast<float>(t);
    }
    T[12] = T[13] = T[14] = 0.f, T[15] = 1.f;
}

struct IcpIterState {
    float F[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // the accumulated transformation
    int it = 0, st = 0, n_corr = 0;
    bool converged = false;
    double prev_mse = std::numeric_limits<double>::max();
};
enum { ICP_STEP_STOP = 0, ICP_STEP_CONTINUE = 1, ICP_STEP_CONVERGED = 2 };

// The half of an iteration every metric shares: F takes the increment T up, then PCL's DefaultConvergenceCriteria on T and on the
// sweep's mean squared correspondence distance.  ICP_STEP_CONVERGED when one of the criteria fired (s.st tells which).
inline int icp_host_accumulate(IcpIterState& s, const float* T, double mse, int max_iterations, double te, double fe) {
    float* F = s.F;
    float G[16];
    for (int r = 0; r < 4; ++r)
        for (int cc = 0; cc < 4; ++cc) G[4 * r + cc] = ((T[4 * r] * F[cc] + T[4 * r + 1] * F[4 + cc]) + T[4 * r + 2] * F[8 + cc]) + T[4 * r + 3] * F[12 + cc];
    std::memcpy(F, G, sizeof G);
    ++s.it;
    // DefaultConvergenceCriteria::hasConverged (PCL 1.8)
    if (s.it >= max_iterations) {
        s.st = 1, s.converged = true;
        return ICP_STEP_CONVERGED;
    }
    const double cos_angle = 0.5 * (static_cast<double>(T[0]) + T[5] + T[10] - 1.0);
    const double tr2 = static_cast<double>(T[3]) * T[3] + static_cast<double>(T[7]) * T[7] + static_cast<double>(T[11]) * T[11];
    if (cos_angle >= 1.0 - te && tr2 <= te) {
        s.st = 2, s.converged = true;
        return ICP_STEP_CONVERGED;
    }
    if (std::fabs(mse - s.prev_mse) < 1e-12) {
        s.st = 3, s.converged = true;
        return ICP_STEP_CONVERGED;
    }
    if (std::fabs(mse - s.prev_mse) / s.prev_mse < fe) {
        s.st = 4, s.converged = true;
        return ICP_STEP_CONVERGED;
    }
    s.prev_mse = mse;
    return ICP_STEP_CONTINUE;
}

// One iteration's host work on the sums of a correspondence sweep (n, sum p, sum q, sum q p^T, sum d^2).  ICP_STEP_STOP: too few
// correspondences, state 5, no increment.  Otherwise T is the increment to apply to the source cloud and F has taken it up.
inline int icp_host_step(IcpIterState& s, const double* sums, int max_iterations, double te, double fe, float* T) {
    s.n_corr = static_cast<int>(sums[0]);
    if (sums[0] < 3) {  // icp.hpp: "Not enough correspondences found"
        s.st = 5;
        return ICP_STEP_STOP;
    }
    transform_from_sums(sums, T);
    return icp_host_accumulate(s, T, sums[16] / sums[0], max_iterations, te, fe);
}

// ---- point-to-plane (scal_icp_align_plane): the increment comes from the 6x6 normal equations instead -------------------------------
constexpr double ICP_PLANE_PIVOT_MIN = 1e-10;  // SCAL_ICP_PLANE_PIVOT_MIN

// A x = b by LDL^T without pivoting, in the order include/scaloam_hip.h writes out; A's upper triangle row-major in tri[21].
// false: a pivot d_j is not > ICP_PLANE_PIVOT_MIN * A_jj, the system is degenerate and x is not written.
inline bool icp_plane_solve(const double* tri, const double* b, double* x) {
    double A[6][6], L[6][6], D[6], v[6], y[6];
    for (int i = 0, k = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++k) A[i][j] = A[j][i] = tri[k];
    for (int j = 0; j < 6; ++j) {
        for (int k = 0; k < j; ++k) v[k] = L[j][k] * D[k];
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d = d - L[j][k] * v[k];
        if (!(d > ICP_PLANE_PIVOT_MIN * A[j][j])) return false;
        D[j] = d;
        for (int i = j + 1; i < 6; ++i) {
            double s = A[i][j];
            for (int k = 0; k < j; ++k) s = s - L[i][k] * v[k];
            L[i][j] = s / d;
        }
    }
    for (int i = 0; i < 6; ++i) {
        y[i] = b[i];
        for (int k = 0; k < i; ++k) y[i] = y[i] - L[i][k] * y[k];
    }
    for (int i = 0; i < 6; ++i) x[i] = y[i] / D[i];
    for (int i = 5; i >= 0; --i)
        for (int k = i + 1; k < 6; ++k) x[i] = x[i] - L[k][i] * x[k];
    return true;
}

// the increment of x = (alpha, beta, gamma, tx, ty, tz): the unit quaternion (1, alpha / 2, beta / 2, gamma / 2) / norm through
// transform_from_sums' matrix formula, no trigonometric function, so that a numpy restatement agrees to the bit
inline void transform_from_plane_solution(const double* x6, float* T) {
    const double hx = x6[0] / 2.0, hy = x6[1] / 2.0, hz = x6[2] / 2.0;
    const double m = std::sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
    const double w = 1.0 / m, x = hx / m, y = hy / m, z = hz / m;
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = static_cast<float>(R[r][c]);
        T[4 * r + 3] = static_cast<float>(x6[3 + r]);
    }
    T[12] = T[13] = T[14] = 0.f, T[15] = 1.f;
}

// icp_host_step for the 32 sums of a point-to-plane sweep.  ICP_STEP_STOP with state 5 (fewer than 6 rows) or 6 (degenerate normal
// equations), no increment; everything after the increment is icp_host_accumulate, with mse the rows' mean squared distance.
inline int icp_plane_host_step(IcpIterState& s, const double* sums, int max_iterations, double te, double fe, float* T) {
    s.n_corr = static_cast<int>(sums[0]);
    if (sums[0] < 6) {
        s.st = 5;
        return ICP_STEP_STOP;
    }
    double x[6];
    if (!icp_plane_solve(sums + 1, sums + 22, x)) {
        s.st = 6;
        return ICP_STEP_STOP;
    }
    transform_from_plane_solution(x, T);
    return icp_host_accumulate(s, T, sums[29] / sums[0], max_iterations, te, fe);
}

}  // namespace scal
