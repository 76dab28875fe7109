// scal_posegraph: batch pose-graph optimisation on the device (include/scaloam_hip.h).  What the pose-graph node
// asks of GTSAM (laserPosegraphOptimization.cpp :284-310, :644-690, :761-768, :399-406), restated from the published algorithms; the
// CPU restatement it is held to is scaloam/pgo.py (optimize_pose_graph), and both take the same series branches.
//
// One Gauss-Newton iteration, everything f64 in HBM:
//   k_pg_linearize   one thread per edge (edge 0 is the prior): r = Log(Z^-1 Ti^-1 Tj), Jr^-1(r), Ad, whitening, Cauchy weight ->
//                    the edge's two 6x6 blocks, its 6-vector, cost term and weight
//   k_pg_assemble    one thread per (node, element): the node's diagonal block of H = J^T J, its block towards node + 1 and g = J^T b,
//                    summed over the node's incident edges in edge order (CSR built once per graph) - no atomics
//   k_pg_offdiag     one thread per (edge, element): the edge's off-diagonal block of H
//   k_pg_pcr_*       the block-tridiagonal part M of H (diagonal blocks + the blocks between neighbours: prior and odometry chain, plus
//                    what loops add to the diagonal) is factored by parallel cyclic reduction: ceil(log2 n) levels, every row active in each,
//                    the two 6x6 multipliers of every row and level are kept, 36 threads per row
//   conjugate gradients on H d = -g preconditioned by M: H p from the blocks (CSR gather), M^-1 r = one launch per level; alpha, beta and
//                    the stop flag live on the device, dot products are per-workgroup partials summed by one workgroup in a fixed order.
//                    The host queues iterations in growing batches and reads the flag after each batch, never per iteration.
//   k_pg_retract     T <- T Exp(d), quaternion renormalised; k_pg_linearize<false> gives the new cost; the host accepts or rejects.
// Launch boundaries only: no workgroup ever waits for another one.  Every loop is bounded by max_iterations / max_linear_iterations.
#include "common.hpp"
#include <algorithm>
#include <cmath>

namespace scal {

constexpr double PG_SERIES_THETA2 = 0.1 * 0.1;   // pgo.py SERIES_THETA
constexpr double PG_SERIES_SINE2 = 1e-4 * 1e-4;  // pgo.py SERIES_SINE
constexpr int PG_ROWS = 7;                       // rows per workgroup of the 36-thread-per-row kernels
constexpr int PG_RT = PG_ROWS * 36;
constexpr int PG_VB = 192;                       // vector kernels: 32 nodes x 6

struct PgState {  // the scalars of one linear solve and one step, on the device
    double rz, rz0, pq, alpha, beta;
    double cost, step_max;
    int iters, done, status, pad;
};

struct V3 {
    double x, y, z;
};
struct M3 {
    double a[3][3];
};
__device__ inline V3 cross3(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline M3 hat3(V3 w) {
    M3 m;
    m.a[0][0] = 0, m.a[0][1] = -w.z, m.a[0][2] = w.y;
    m.a[1][0] = w.z, m.a[1][1] = 0, m.a[1][2] = -w.x;
    m.a[2][0] = -w.y, m.a[2][1] = w.x, m.a[2][2] = 0;
    return m;
}
__device__ inline M3 mul3(const M3& p, const M3& q) {
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.a[i][j] = (p.a[i][0] * q.a[0][j] + p.a[i][1] * q.a[1][j]) + p.a[i][2] * q.a[2][j];
    return r;
}
__device__ inline M3 lin3(double s, const M3& p, double t, const M3& q) {  // s p + t q
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.a[i][j] = s * p.a[i][j] + t * q.a[i][j];
    return r;
}
__device__ inline M3 neg3(const M3& p) {
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.a[i][j] = -p.a[i][j];
    return r;
}
__device__ inline M3 transpose3(const M3& p) {
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.a[i][j] = p.a[j][i];
    return r;
}
__device__ inline V3 mv3(const M3& m, V3 v) {
    return {(m.a[0][0] * v.x + m.a[0][1] * v.y) + m.a[0][2] * v.z, (m.a[1][0] * v.x + m.a[1][1] * v.y) + m.a[1][2] * v.z,
            (m.a[2][0] * v.x + m.a[2][1] * v.y) + m.a[2][2] * v.z};
}
struct Q4 {
    double x, y, z, w;
};
__device__ inline Q4 qmul(Q4 a, Q4 b) {
    return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
            a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
__device__ inline Q4 qconj(Q4 q) { return {-q.x, -q.y, -q.z, q.w}; }
__device__ inline M3 qmat(Q4 q) {
    M3 R;
    R.a[0][0] = 1 - 2 * (q.y * q.y + q.z * q.z), R.a[0][1] = 2 * (q.x * q.y - q.w * q.z), R.a[0][2] = 2 * (q.x * q.z + q.w * q.y);
    R.a[1][0] = 2 * (q.x * q.y + q.w * q.z), R.a[1][1] = 1 - 2 * (q.x * q.x + q.z * q.z), R.a[1][2] = 2 * (q.y * q.z - q.w * q.x);
    R.a[2][0] = 2 * (q.x * q.z - q.w * q.y), R.a[2][1] = 2 * (q.y * q.z + q.w * q.x), R.a[2][2] = 1 - 2 * (q.x * q.x + q.y * q.y);
    return R;
}

// pgo.py _coeffs: a = (1 - cos)/t^2, b = (t - sin)/t^3, c = (1 - (t/2) cot(t/2))/t^2, c2 = (t^2 + 2 cos - 2)/(2 t^4),
// c3 = (2 t - 3 sin + t cos)/(2 t^5); four series terms below 0.1 rad
__device__ inline void pg_coeffs(double th2, double& a, double& b, double& c, double& c2, double& c3) {
    if (th2 < PG_SERIES_THETA2) {
        const double x = th2;
        a = 1.0 / 2 + x * (-1.0 / 24 + x * (1.0 / 720 - x / 40320));
        b = 1.0 / 6 + x * (-1.0 / 120 + x * (1.0 / 5040 - x / 362880));
        c = 1.0 / 12 + x * (1.0 / 720 + x * (1.0 / 30240 + x / 1209600));
        c2 = 1.0 / 24 + x * (-1.0 / 720 + x * (1.0 / 40320 - x / 3628800));
        c3 = 1.0 / 120 + x * (-1.0 / 2520 + x * (1.0 / 120960 - x / 9979200));
        return;
    }
    const double t = sqrt(th2), s = sin(t), co = cos(t);
    a = (1 - co) / th2;
    b = (t - s) / (th2 * t);
    c = (1 - 0.5 * t * cos(0.5 * t) / sin(0.5 * t)) / th2;
    c2 = (th2 + 2 * co - 2) / (2 * th2 * th2);
    c3 = (2 * t - 3 * s + t * co) / (2 * th2 * th2 * t);
}

struct Pose {
    Q4 q;
    V3 t;
};
__device__ inline Pose load_pose(const double* p) { return {{p[0], p[1], p[2], p[3]}, {p[4], p[5], p[6]}}; }
// a^-1 b
__device__ inline Pose pose_between(const Pose& a, const Pose& b) {
    const M3 Rt = transpose3(qmat(a.q));
    return {qmul(qconj(a.q), b.q), mv3(Rt, V3{b.t.x - a.t.x, b.t.y - a.t.y, b.t.z - a.t.z})};
}
__device__ inline V3 rot_log(Q4 q) {
    if (q.w < 0) q = {-q.x, -q.y, -q.z, -q.w};
    const double s2 = q.x * q.x + q.y * q.y + q.z * q.z;
    double k;
    if (s2 < PG_SERIES_SINE2) {
        const double x = s2 / (q.w * q.w);
        k = 2 / q.w * (1 + x * (-1.0 / 3 + x / 5));
    } else {
        const double s = sqrt(s2);
        k = 2 * atan2(s, q.w) / s;
    }
    return {k * q.x, k * q.y, k * q.z};
}

// One edge: residual, cost and weight; JAC: the whitened, weighted blocks A_i, A_j (row-major 6x6 each) and b.
// Edge 0 is the prior (ej < 0): r = Log(P^-1 T), A_i = Jr^-1(r), A_j = 0.
template <bool JAC>
__global__ void __launch_bounds__(64) k_pg_linearize(int n_e, const double* __restrict__ x, const int* __restrict__ ei, const int* __restrict__ ej,
                                                      const double* __restrict__ ez, const double* __restrict__ esi, const double* __restrict__ ek,
                                                      double* __restrict__ A, double* __restrict__ bvec, double* __restrict__ cost_e,
                                                      double* __restrict__ w_e) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_e) return;
    const int i = ei[e], j = ej[e];
    const Pose Z = load_pose(ez + 7 * (size_t)e);
    Pose rel;
    if (j < 0) {
        rel = load_pose(x + 7 * (size_t)i);
    } else {
        rel = pose_between(load_pose(x + 7 * (size_t)i), load_pose(x + 7 * (size_t)j));
    }
    const Pose D = pose_between(Z, rel);
    const V3 w = rot_log(D.q);
    double ca, cb, cc, c2, c3;
    pg_coeffs(w.x * w.x + w.y * w.y + w.z * w.z, ca, cb, cc, c2, c3);
    const V3 wt = cross3(w, D.t), wwt = cross3(w, wt);
    const V3 v = {D.t.x - 0.5 * wt.x + cc * wwt.x, D.t.y - 0.5 * wt.y + cc * wwt.y, D.t.z - 0.5 * wt.z + cc * wwt.z};
    const double r[6] = {w.x, w.y, w.z, v.x, v.y, v.z};
    double si[6], e6[6], e2 = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        si[k] = esi[6 * (size_t)e + k];
        e6[k] = r[k] * si[k];
        e2 += e6[k] * e6[k];
    }
    const double kc = ek[e], k2 = kc * kc;
    const bool robust = k2 > 0;
    const double wgt = robust ? k2 / (k2 + e2) : 1.0;
    cost_e[e] = robust ? 0.5 * k2 * log1p(e2 / k2) : 0.5 * e2;
    w_e[e] = wgt;
    if (!JAC) return;
    const double sw = sqrt(wgt);
    // Jr^-1(r) = Jl^-1(-r) = [[J, 0], [B, J]]: J = I - W/2 + c W^2, B = -J Q J with W = hat(-omega), V = hat(-v) (Barfoot eq. 7.86)
    const M3 W = hat3(V3{-w.x, -w.y, -w.z}), Vh = hat3(V3{-v.x, -v.y, -v.z});
    const M3 WW = mul3(W, W);
    M3 J = lin3(-0.5, W, cc, WW);
    J.a[0][0] += 1, J.a[1][1] += 1, J.a[2][2] += 1;
    const M3 WV = mul3(W, Vh), VW = mul3(Vh, W), WVW = mul3(WV, W);
    M3 Q;
    {
        const M3 t2a = mul3(W, WV), t2b = mul3(VW, W), t3a = mul3(WVW, W), t3b = mul3(W, WVW);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
                Q.a[a][b] = 0.5 * Vh.a[a][b] + cb * (WV.a[a][b] + VW.a[a][b] + WVW.a[a][b]) + c2 * (t2a.a[a][b] + t2b.a[a][b] - 3 * WVW.a[a][b]) +
                            c3 * (t3a.a[a][b] + t3b.a[a][b]);
    }
    const M3 JQJ = mul3(mul3(J, Q), J);
    const M3 zero = {};
    const M3 B = neg3(JQJ);
    double* Ai = A + 72 * (size_t)e;
    double* Aj = Ai + 36;
    // row block scale: sqrt(w) / sigma
    auto store = [&](double* dst, const M3& tl, const M3& bl, const M3& d) {  // [[tl, 0], [bl, d]]
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                dst[6 * a + b] = tl.a[a][b] * (si[a] * sw);
                dst[6 * a + 3 + b] = 0.0;
                dst[6 * (a + 3) + b] = bl.a[a][b] * (si[a + 3] * sw);
                dst[6 * (a + 3) + 3 + b] = d.a[a][b] * (si[a + 3] * sw);
            }
    };
#pragma unroll
    for (int k = 0; k < 6; ++k) bvec[6 * (size_t)e + k] = e6[k] * sw;
    if (j < 0) {
        store(Ai, J, B, J);
        store(Aj, zero, zero, zero);
        return;
    }
    store(Aj, J, B, J);
    // dr/dd_i = -Jr^-1(r) Ad(rel^-1), Ad(rel^-1) = [[R', 0], [hat(t') R', R']] with R' = R_rel^T, t' = -R' t_rel
    const M3 Rp = transpose3(qmat(rel.q));
    const V3 tp0 = mv3(Rp, rel.t);
    const M3 Cp = mul3(hat3(V3{-tp0.x, -tp0.y, -tp0.z}), Rp);
    const M3 JR = mul3(J, Rp);
    const M3 low = lin3(1, mul3(B, Rp), 1, mul3(J, Cp));
    store(Ai, neg3(JR), neg3(low), neg3(JR));
}

// element `el` of node `nd`: el < 36 the diagonal block D (with Levenberg damping on its diagonal) and the block U towards nd + 1,
// el 36..41 the gradient
__global__ void __launch_bounds__(256) k_pg_assemble(int n, const int* __restrict__ rowptr, const int* __restrict__ inc, const int* __restrict__ ei,
                                                      const int* __restrict__ ej, const double* __restrict__ A, const double* __restrict__ bvec,
                                                      double lambda, double* __restrict__ Dg, double* __restrict__ Ug, double* __restrict__ g) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int nd = tid / 42, el = tid % 42;
    if (nd >= n) return;
    const int r = el < 36 ? el / 6 : el - 36, c = el < 36 ? el % 6 : 0;
    double d = 0, u = 0;
    for (int q = rowptr[nd]; q < rowptr[nd + 1]; ++q) {
        const int e = inc[q];
        const bool first = ei[e] == nd;
        const double* As = A + 72 * (size_t)e + (first ? 0 : 36);
        const double* Ao = A + 72 * (size_t)e + (first ? 36 : 0);
        if (el < 36) {
            double s = 0;
            for (int k = 0; k < 6; ++k) s += As[6 * k + r] * As[6 * k + c];
            d += s;
            const int other = first ? ej[e] : ei[e];
            if (other == nd + 1) {
                double t = 0;
                for (int k = 0; k < 6; ++k) t += As[6 * k + r] * Ao[6 * k + c];
                u += t;
            }
        } else {
            double s = 0;
            for (int k = 0; k < 6; ++k) s += As[6 * k + r] * bvec[6 * (size_t)e + k];
            d += s;
        }
    }
    if (el < 36) {
        if (r == c) d += lambda * d;
        Dg[36 * (size_t)nd + el] = d;
        Ug[36 * (size_t)nd + el] = u;
    } else {
        g[6 * (size_t)nd + r] = d;
    }
}

__global__ void __launch_bounds__(256) k_pg_offdiag(int n_e, const double* __restrict__ A, double* __restrict__ O) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = tid / 36, el = tid % 36;
    if (e >= n_e) return;
    const int r = el / 6, c = el % 6;
    const double* Ai = A + 72 * (size_t)e;
    double s = 0;
    for (int k = 0; k < 6; ++k) s += Ai[6 * k + r] * Ai[36 + 6 * k + c];
    O[36 * (size_t)e + el] = s;
}

// ---- parallel cyclic reduction of M (rows L_i, D_i, U_i; L_i = U_{i-1}^T): 36 threads per row, PG_ROWS rows per workgroup
// in-place Gauss-Jordan inverse of the PG_ROWS 6x6 matrices in `m` (no pivoting: they are symmetric positive definite); all threads call
__device__ inline void pg_inv6(double (*m)[36], int row, int r, int c) {
    for (int k = 0; k < 6; ++k) {
        __syncthreads();
        const double p = 1.0 / m[row][6 * k + k];
        const double ark = m[row][6 * r + k], akc = m[row][6 * k + c], arc = m[row][6 * r + c];
        __syncthreads();
        double v;
        if (r == k)
            v = c == k ? p : akc * p;
        else
            v = c == k ? -ark * p : arc - ark * akc * p;
        m[row][6 * r + c] = v;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(PG_RT) k_pg_pcr_init(int n, const double* __restrict__ Dg, const double* __restrict__ Ug, double* __restrict__ L,
                                                        double* __restrict__ D, double* __restrict__ U, double* __restrict__ Di) {
    __shared__ double m[PG_ROWS][36];
    const int row = threadIdx.x / 36, el = threadIdx.x % 36, r = el / 6, c = el % 6;
    const int i = blockIdx.x * PG_ROWS + row;
    const bool on = i < n;
    const double d = on ? Dg[36 * (size_t)i + el] : (r == c ? 1.0 : 0.0);
    m[row][el] = d;
    pg_inv6(m, row, r, c);
    if (!on) return;
    D[36 * (size_t)i + el] = d;
    Di[36 * (size_t)i + el] = m[row][el];
    U[36 * (size_t)i + el] = i + 1 < n ? Ug[36 * (size_t)i + el] : 0.0;
    L[36 * (size_t)i + el] = i > 0 ? Ug[36 * (size_t)(i - 1) + 6 * c + r] : 0.0;
}

// one level at stride s: alpha = L_i Dinv_{i-s}, gamma = U_i Dinv_{i+s} (kept for the solves), D' = D_i - alpha U_{i-s} - gamma L_{i+s},
// L' = -alpha L_{i-s}, U' = -gamma U_{i+s}, Dinv' = D'^-1
__global__ void __launch_bounds__(PG_RT) k_pg_pcr_level(int n, int s, const double* __restrict__ L, const double* __restrict__ D,
                                                         const double* __restrict__ U, const double* __restrict__ Di, double* __restrict__ Ln,
                                                         double* __restrict__ Dn, double* __restrict__ Un, double* __restrict__ Din,
                                                         double* __restrict__ alpha, double* __restrict__ gamma) {
    __shared__ double sa[PG_ROWS][36], sg[PG_ROWS][36], m[PG_ROWS][36];
    const int row = threadIdx.x / 36, el = threadIdx.x % 36, r = el / 6, c = el % 6;
    const int i = blockIdx.x * PG_ROWS + row;
    const bool on = i < n, lo = on && i - s >= 0, hi = on && i + s < n;
    const size_t me = 36 * (size_t)(on ? i : 0), dn = 36 * (size_t)(lo ? i - s : 0), up = 36 * (size_t)(hi ? i + s : 0);
    double a = 0, g = 0;
    if (lo)
        for (int k = 0; k < 6; ++k) a += L[me + 6 * r + k] * Di[dn + 6 * k + c];
    if (hi)
        for (int k = 0; k < 6; ++k) g += U[me + 6 * r + k] * Di[up + 6 * k + c];
    sa[row][el] = a, sg[row][el] = g;
    __syncthreads();
    double d = on ? D[me + el] : (r == c ? 1.0 : 0.0), l = 0, u = 0;
    if (lo)
        for (int k = 0; k < 6; ++k) {
            d -= sa[row][6 * r + k] * U[dn + 6 * k + c];
            l -= sa[row][6 * r + k] * L[dn + 6 * k + c];
        }
    if (hi)
        for (int k = 0; k < 6; ++k) {
            d -= sg[row][6 * r + k] * L[up + 6 * k + c];
            u -= sg[row][6 * r + k] * U[up + 6 * k + c];
        }
    m[row][el] = d;
    pg_inv6(m, row, r, c);
    if (!on) return;
    alpha[me + el] = a, gamma[me + el] = g;
    Ln[me + el] = l, Dn[me + el] = d, Un[me + el] = u, Din[me + el] = m[row][el];
}

// solve, one level: out_i = in_i - alpha_i in_{i-s} - gamma_i in_{i+s}; one thread per (node, row)
__global__ void __launch_bounds__(PG_VB) k_pg_pcr_apply(int n, int s, const double* __restrict__ alpha, const double* __restrict__ gamma,
                                                         const double* __restrict__ in, double* __restrict__ out, const PgState* __restrict__ st) {
    if (st->done) return;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = tid / 6, r = tid % 6;
    if (i >= n) return;
    double v = in[tid];
    if (i - s >= 0)
        for (int k = 0; k < 6; ++k) v -= alpha[36 * (size_t)i + 6 * r + k] * in[6 * (size_t)(i - s) + k];
    if (i + s < n)
        for (int k = 0; k < 6; ++k) v -= gamma[36 * (size_t)i + 6 * r + k] * in[6 * (size_t)(i + s) + k];
    out[tid] = v;
}

// fixed-order sum of a workgroup's values (PG_VB threads, power-of-two tree over 256 slots)
__device__ inline double pg_block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    if (threadIdx.x < 256 - PG_VB) sh[PG_VB + threadIdx.x] = 0.0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// last step of M^-1: z_i = Dinv_i in_i, and this workgroup's part of r . z
__global__ void __launch_bounds__(PG_VB) k_pg_pcr_final(int n, const double* __restrict__ Di, const double* __restrict__ in, const double* __restrict__ rvec,
                                                         double* __restrict__ z, double* __restrict__ part, const PgState* __restrict__ st) {
    __shared__ double sh[256];
    if (st->done) return;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = tid / 6, r = tid % 6;
    double v = 0, rz = 0;
    if (i < n) {
        for (int k = 0; k < 6; ++k) v += Di[36 * (size_t)i + 6 * r + k] * in[6 * (size_t)i + k];
        z[tid] = v;
        rz = rvec[tid] * v;
    }
    const double s = pg_block_sum(rz, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// q = H p from the blocks, and this workgroup's part of p . q
__global__ void __launch_bounds__(PG_VB) k_pg_hp(int n, const int* __restrict__ rowptr, const int* __restrict__ inc, const int* __restrict__ ei,
                                                  const int* __restrict__ ej, const double* __restrict__ Dg, const double* __restrict__ O,
                                                  const double* __restrict__ p, double* __restrict__ q, double* __restrict__ part,
                                                  const PgState* __restrict__ st) {
    __shared__ double sh[256];
    if (st->done) return;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = tid / 6, r = tid % 6;
    double v = 0, pq = 0;
    if (i < n) {
        for (int k = 0; k < 6; ++k) v += Dg[36 * (size_t)i + 6 * r + k] * p[6 * (size_t)i + k];
        for (int t = rowptr[i]; t < rowptr[i + 1]; ++t) {
            const int e = inc[t];
            const int a = ei[e], b = ej[e];
            if (b < 0) continue;  // the prior
            const double* Oe = O + 36 * (size_t)e;
            double s = 0;
            if (a == i)
                for (int k = 0; k < 6; ++k) s += Oe[6 * r + k] * p[6 * (size_t)b + k];
            else
                for (int k = 0; k < 6; ++k) s += Oe[6 * k + r] * p[6 * (size_t)a + k];
            v += s;
        }
        q[tid] = v;
        pq = p[tid] * v;
    }
    const double s = pg_block_sum(pq, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one workgroup: the partials in a fixed order (every thread a strided share, then the tree)
__device__ inline double pg_sum_parts(const double* part, int np, double* sh) {
    double v = 0;
    for (int k = threadIdx.x; k < np; k += 256) v += part[k];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// start of a solve: rz0 = r . M^-1 r; nothing to do when it is zero, breakdown when it is negative or not finite
__global__ void __launch_bounds__(256) k_pg_cg_start(const double* __restrict__ part, int np, PgState* st) {
    __shared__ double sh[256];
    const double rz = pg_sum_parts(part, np, sh);
    if (threadIdx.x) return;
    st->rz = st->rz0 = rz;
    st->alpha = st->beta = 0;
    st->iters = 0;
    st->done = !(rz > 0);
    st->status = rz == 0 ? 0 : (rz > 0 ? 1 : 2);  // 1 until the tolerance is met
}
__global__ void __launch_bounds__(256) k_pg_cg_alpha(const double* __restrict__ part, int np, PgState* st) {
    __shared__ double sh[256];
    if (st->done) return;
    const double pq = pg_sum_parts(part, np, sh);
    if (threadIdx.x) return;
    st->pq = pq;
    if (!(pq > 0) || !isfinite(pq)) {
        st->done = 1, st->status = 2, st->alpha = 0;
        return;
    }
    st->alpha = st->rz / pq;
}
__global__ void __launch_bounds__(PG_VB) k_pg_cg_axpy(int n6, const PgState* __restrict__ st, double* __restrict__ xs, double* __restrict__ r,
                                                       const double* __restrict__ p, const double* __restrict__ q) {
    if (st->done) return;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n6) return;
    const double a = st->alpha;
    xs[tid] += a * p[tid];
    r[tid] -= a * q[tid];
}
__global__ void __launch_bounds__(256) k_pg_cg_beta(const double* __restrict__ part, int np, PgState* st, double rtol2, int max_iters) {
    __shared__ double sh[256];
    if (st->done) return;
    const double rz = pg_sum_parts(part, np, sh);
    if (threadIdx.x) return;
    st->iters += 1;
    if (!isfinite(rz) || rz < 0) {
        st->done = 1, st->status = 2, st->beta = 0;
        return;
    }
    st->beta = rz / st->rz;
    st->rz = rz;
    if (rz <= rtol2 * st->rz0)
        st->done = 1, st->status = 0;
    else if (st->iters >= max_iters)
        st->done = 1, st->status = 1;
}
__global__ void __launch_bounds__(PG_VB) k_pg_cg_p(int n6, const PgState* __restrict__ st, const double* __restrict__ z, double* __restrict__ p) {
    if (st->done) return;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n6) return;
    p[tid] = z[tid] + st->beta * p[tid];
}
// xs = 0, r = -g
__global__ void __launch_bounds__(PG_VB) k_pg_cg_init(int n6, const double* __restrict__ g, double* __restrict__ xs, double* __restrict__ r, PgState* st) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid == 0) st->done = 0;
    if (tid >= n6) return;
    xs[tid] = 0.0;
    r[tid] = -g[tid];
}

// T <- T Exp(d), quaternion renormalised; this workgroup's max |d|
__global__ void __launch_bounds__(256) k_pg_retract(int n, const double* __restrict__ x, const double* __restrict__ d, double* __restrict__ xn,
                                                     double* __restrict__ part) {
    __shared__ double sh[256];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double mx = 0;
    if (i < n) {
        const V3 w = {d[6 * (size_t)i], d[6 * (size_t)i + 1], d[6 * (size_t)i + 2]}, v = {d[6 * (size_t)i + 3], d[6 * (size_t)i + 4], d[6 * (size_t)i + 5]};
        mx = fmax(fmax(fmax(fabs(w.x), fabs(w.y)), fabs(w.z)), fmax(fmax(fabs(v.x), fabs(v.y)), fabs(v.z)));
        if (!(mx == mx)) mx = INFINITY;
        const double th2 = w.x * w.x + w.y * w.y + w.z * w.z;
        double ca, cb, cc, c2, c3, sh2, ch2;
        pg_coeffs(th2, ca, cb, cc, c2, c3);
        if (th2 < PG_SERIES_THETA2) {
            sh2 = 1.0 / 2 + th2 * (-1.0 / 48 + th2 * (1.0 / 3840 - th2 / 645120));
            ch2 = 1 + th2 * (-1.0 / 8 + th2 * (1.0 / 384 - th2 / 46080));
        } else {
            const double t = sqrt(th2);
            sh2 = sin(0.5 * t) / t, ch2 = cos(0.5 * t);
        }
        const V3 wv = cross3(w, v), wwv = cross3(w, wv);
        const V3 tr = {v.x + ca * wv.x + cb * wwv.x, v.y + ca * wv.y + cb * wwv.y, v.z + ca * wv.z + cb * wwv.z};
        const Pose T = load_pose(x + 7 * (size_t)i);
        Q4 q = qmul(T.q, Q4{sh2 * w.x, sh2 * w.y, sh2 * w.z, ch2});
        const V3 rt = mv3(qmat(T.q), tr);
        const double nq = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
        double* o = xn + 7 * (size_t)i;
        o[0] = q.x / nq, o[1] = q.y / nq, o[2] = q.z / nq, o[3] = q.w / nq;
        o[4] = T.t.x + rt.x, o[5] = T.t.y + rt.y, o[6] = T.t.z + rt.z;
    }
    sh[threadIdx.x] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// one workgroup: cost = sum of the edge costs in a fixed order; np > 0: step_max = max of the retract's partials
__global__ void __launch_bounds__(256) k_pg_reduce(const double* __restrict__ cost_e, int n_e, const double* __restrict__ part, int np, PgState* st) {
    __shared__ double sh[256];
    const double c = pg_sum_parts(cost_e, n_e, sh);
    __syncthreads();
    double mx = 0;
    for (int k = threadIdx.x; k < np; k += 256) mx = fmax(mx, part[k]);
    sh[threadIdx.x] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st->cost = c;
        if (np > 0) st->step_max = sh[0];
    }
}

}  // namespace scal

using namespace scal;

struct scal_posegraph {
    scal_posegraph_config cfg{};
    LaneStream stream;
    int levels_cap = 0;
    // host side of the graph
    int n = 0;
    bool have_prior = false, graph_dirty = true, weights_valid = false;
    std::vector<double> h_x;                 // [n][7]
    std::vector<int> h_ei, h_ej;             // edge 0 = the prior (ej = -1)
    std::vector<double> h_ez, h_esi, h_ek;   // measurement, 1 / sigma, Cauchy k
    // device
    DevBuf<double> x, xn, ez, esi, ek, A, bvec, cost_e, w_e, Dg, Ug, O, g;
    DevBuf<int> ei, ej, rowptr, inc;
    DevBuf<double> wL[2], wD[2], wU[2], wDi[2], alpha, gamma;
    DevBuf<double> xs, r, z, p, q, t0, t1, part;
    DevBuf<PgState> st;
    PinBuf<PgState> h_st;
    PinBuf<double> h_io;
};

namespace {

constexpr int PG_DEF_MAX_IT = 50, PG_DEF_MAX_LIN = 2000;
constexpr double PG_DEF_STEP_TOL = 1e-8, PG_DEF_RTOL = 1e-12;
constexpr double PG_LAMBDA_FIRST = 1e-4, PG_LAMBDA_FACTOR = 10.0, PG_LAMBDA_MAX = 1e8;  // pgo.py PG_DEFAULTS

int levels_for(int n) {
    int l = 0;
    for (long long s = 1; s < n; s *= 2) ++l;
    return l;
}

bool finite7(const double* p) {
    for (int k = 0; k < 7; ++k)
        if (!std::isfinite(p[k])) return false;
    return (p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]) > 0;
}
void put_pose(std::vector<double>& v, size_t at, const double* p) {
    const double nq = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]);
    for (int k = 0; k < 4; ++k) v[at + k] = p[k] / nq;
    for (int k = 4; k < 7; ++k) v[at + k] = p[k];
}
bool variances_ok(const double* v) {
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(v[k]) || !(v[k] > 0)) return false;
    return true;
}

// edges and CSR to the device (once per graph)
int upload_graph(scal_posegraph* c) {
    hipStream_t s = c->stream;
    const int ne = static_cast<int>(c->h_ei.size());
    std::vector<int> rowptr(static_cast<size_t>(c->n) + 1, 0), inc;
    for (int e = 0; e < ne; ++e) {
        rowptr[static_cast<size_t>(c->h_ei[e]) + 1]++;
        if (c->h_ej[e] >= 0) rowptr[static_cast<size_t>(c->h_ej[e]) + 1]++;
    }
    for (int i = 0; i < c->n; ++i) rowptr[static_cast<size_t>(i) + 1] += rowptr[static_cast<size_t>(i)];
    inc.resize(static_cast<size_t>(rowptr[static_cast<size_t>(c->n)]));
    std::vector<int> fill(rowptr.begin(), rowptr.end() - 1);
    for (int e = 0; e < ne; ++e) {  // edge order within every node
        inc[static_cast<size_t>(fill[static_cast<size_t>(c->h_ei[e])]++)] = e;
        if (c->h_ej[e] >= 0) inc[static_cast<size_t>(fill[static_cast<size_t>(c->h_ej[e])]++)] = e;
    }
    SCAL_HIP(hipMemcpyAsync(c->ei.p, c->h_ei.data(), sizeof(int) * ne, hipMemcpyHostToDevice, s));
    SCAL_HIP(hipMemcpyAsync(c->ej.p, c->h_ej.data(), sizeof(int) * ne, hipMemcpyHostToDevice, s));
    SCAL_HIP(hipMemcpyAsync(c->ez.p, c->h_ez.data(), sizeof(double) * 7 * ne, hipMemcpyHostToDevice, s));
    SCAL_HIP(hipMemcpyAsync(c->esi.p, c->h_esi.data(), sizeof(double) * 6 * ne, hipMemcpyHostToDevice, s));
    SCAL_HIP(hipMemcpyAsync(c->ek.p, c->h_ek.data(), sizeof(double) * ne, hipMemcpyHostToDevice, s));
    SCAL_HIP(hipMemcpyAsync(c->rowptr.p, rowptr.data(), sizeof(int) * rowptr.size(), hipMemcpyHostToDevice, s));
    if (!inc.empty()) SCAL_HIP(hipMemcpyAsync(c->inc.p, inc.data(), sizeof(int) * inc.size(), hipMemcpyHostToDevice, s));
    SCAL_HIP(hipStreamSynchronize(s));  // the host vectors above go away
    c->graph_dirty = false;
    return SCAL_OK;
}

int read_state(scal_posegraph* c) {
    SCAL_HIP(hipMemcpyAsync(c->h_st.p, c->st.p, sizeof(PgState), hipMemcpyDeviceToHost, c->stream));
    SCAL_HIP(hipStreamSynchronize(c->stream));
    return SCAL_OK;
}

// cost (and weights) at `poses` -> st->cost; np > 0 also reduces the retract's step partials
int eval_cost(scal_posegraph* c, const double* poses, int np) {
    const int ne = static_cast<int>(c->h_ei.size());
    SCAL_LAUNCH_PROF("k_pg_linearize<0>", k_pg_linearize<false>, dim3(div_up(ne, 64)), dim3(64), 0, c->stream, ne, poses, c->ei.p, c->ej.p, c->ez.p, c->esi.p,
                     c->ek.p, c->A.p, c->bvec.p, c->cost_e.p, c->w_e.p);
    SCAL_LAUNCH_PROF("k_pg_reduce", k_pg_reduce, dim3(1), dim3(256), 0, c->stream, c->cost_e.p, ne, c->part.p, np, c->st.p);
    SCAL_HIP(hipGetLastError());
    return SCAL_OK;
}

// z = M^-1 src and the partials of rvec . z
void precondition(scal_posegraph* c, const double* src, int levels, int nvb) {
    hipStream_t s = c->stream;
    const double* in = src;
    double* tmp[2] = {c->t0.p, c->t1.p};
    int step = 1;
    for (int l = 0; l < levels; ++l, step *= 2) {
        double* out = tmp[l & 1];
        SCAL_LAUNCH_PROF("k_pg_pcr_apply", k_pg_pcr_apply, dim3(nvb), dim3(PG_VB), 0, s, c->n, step, c->alpha.p + 36 * static_cast<size_t>(l) * c->n,
                         c->gamma.p + 36 * static_cast<size_t>(l) * c->n, in, out, c->st.p);
        in = out;
    }
    SCAL_LAUNCH_PROF("k_pg_pcr_final", k_pg_pcr_final, dim3(nvb), dim3(PG_VB), 0, s, c->n, c->wDi[levels & 1].p, in, c->r.p, c->z.p, c->part.p, c->st.p);
}

// H d = -g -> c->xs; h_st holds the solve's state afterwards
int solve(scal_posegraph* c, double lambda, int max_lin, double rtol, int* guess) {
    hipStream_t s = c->stream;
    const int n = c->n, n6 = 6 * n;
    const int nvb = div_up(n6, PG_VB), levels = levels_for(n), nrb = div_up(n, PG_ROWS);
    SCAL_LAUNCH_PROF("k_pg_assemble", k_pg_assemble, dim3(div_up(42 * n, 256)), dim3(256), 0, s, n, c->rowptr.p, c->inc.p, c->ei.p, c->ej.p, c->A.p, c->bvec.p,
                     lambda, c->Dg.p, c->Ug.p, c->g.p);
    SCAL_LAUNCH_PROF("k_pg_pcr_init", k_pg_pcr_init, dim3(nrb), dim3(PG_RT), 0, s, n, c->Dg.p, c->Ug.p, c->wL[0].p, c->wD[0].p, c->wU[0].p, c->wDi[0].p);
    int step = 1;
    for (int l = 0; l < levels; ++l, step *= 2) {
        const int a = l & 1, b = a ^ 1;
        SCAL_LAUNCH_PROF("k_pg_pcr_level", k_pg_pcr_level, dim3(nrb), dim3(PG_RT), 0, s, n, step, c->wL[a].p, c->wD[a].p, c->wU[a].p, c->wDi[a].p, c->wL[b].p,
                         c->wD[b].p, c->wU[b].p, c->wDi[b].p, c->alpha.p + 36 * static_cast<size_t>(l) * n, c->gamma.p + 36 * static_cast<size_t>(l) * n);
    }
    SCAL_LAUNCH_PROF("k_pg_cg_init", k_pg_cg_init, dim3(nvb), dim3(PG_VB), 0, s, n6, c->g.p, c->xs.p, c->r.p, c->st.p);
    precondition(c, c->r.p, levels, nvb);
    SCAL_LAUNCH_PROF("k_pg_cg_start", k_pg_cg_start, dim3(1), dim3(256), 0, s, c->part.p, nvb, c->st.p);
    SCAL_HIP(hipMemcpyAsync(c->p.p, c->z.p, sizeof(double) * n6, hipMemcpyDeviceToDevice, s));
    SCAL_HIP(hipGetLastError());
    // iterations are queued in batches (the last solve's count plus a margin, then doubling); the flag is read once per batch
    int queued = 0, batch = std::max(8, *guess + 4);
    for (;;) {
        batch = std::min(batch, max_lin - queued);
        for (int k = 0; k < batch; ++k) {
            SCAL_LAUNCH_PROF("k_pg_hp", k_pg_hp, dim3(nvb), dim3(PG_VB), 0, s, n, c->rowptr.p, c->inc.p, c->ei.p, c->ej.p, c->Dg.p, c->O.p, c->p.p, c->q.p,
                             c->part.p, c->st.p);
            SCAL_LAUNCH_PROF("k_pg_cg_alpha", k_pg_cg_alpha, dim3(1), dim3(256), 0, s, c->part.p, nvb, c->st.p);
            SCAL_LAUNCH_PROF("k_pg_cg_axpy", k_pg_cg_axpy, dim3(nvb), dim3(PG_VB), 0, s, n6, c->st.p, c->xs.p, c->r.p, c->p.p, c->q.p);
            precondition(c, c->r.p, levels, nvb);
            SCAL_LAUNCH_PROF("k_pg_cg_beta", k_pg_cg_beta, dim3(1), dim3(256), 0, s, c->part.p, nvb, c->st.p, rtol * rtol, max_lin);
            SCAL_LAUNCH_PROF("k_pg_cg_p", k_pg_cg_p, dim3(nvb), dim3(PG_VB), 0, s, n6, c->st.p, c->z.p, c->p.p);
        }
        SCAL_HIP(hipGetLastError());
        queued += batch;
        SCAL_TRY(read_state(c));
        if (c->h_st.p->done || queued >= max_lin) break;
        batch *= 2;
    }
    if (!c->h_st.p->done) c->h_st.p->status = 1;  // cannot happen: k_pg_cg_beta stops at max_lin
    *guess = c->h_st.p->iters;
    return SCAL_OK;
}

}  // namespace

int scal::posegraph_create_on_lane(const scal_posegraph_config* cfg, int lane, scal_posegraph_t** out) {
    if (!cfg || !out || cfg->max_nodes < 1 || cfg->max_edges < 0) {
        set_error("scal_posegraph_create: bad argument (max_nodes >= 1, max_edges >= 0)");
        return SCAL_E_ARG;
    }
    *out = nullptr;
    SCAL_TRY(select_device(cfg->device));
    auto* c = new scal_posegraph();
    c->cfg = *cfg;
    const size_t N = static_cast<size_t>(cfg->max_nodes), E = static_cast<size_t>(cfg->max_edges) + 1;
    c->levels_cap = levels_for(cfg->max_nodes);
    int rc = SCAL_OK;
    auto A = [&](int r) { if (rc == SCAL_OK) rc = r; };
    A(c->x.alloc(7 * N)); A(c->xn.alloc(7 * N));
    A(c->ei.alloc(E)); A(c->ej.alloc(E)); A(c->ez.alloc(7 * E)); A(c->esi.alloc(6 * E)); A(c->ek.alloc(E));
    A(c->rowptr.alloc(N + 1)); A(c->inc.alloc(2 * E));
    A(c->A.alloc(72 * E)); A(c->bvec.alloc(6 * E)); A(c->cost_e.alloc(E)); A(c->w_e.alloc(E));
    A(c->Dg.alloc(36 * N)); A(c->Ug.alloc(36 * N)); A(c->O.alloc(36 * E)); A(c->g.alloc(6 * N));
    for (int k = 0; k < 2; ++k) { A(c->wL[k].alloc(36 * N)); A(c->wD[k].alloc(36 * N)); A(c->wU[k].alloc(36 * N)); A(c->wDi[k].alloc(36 * N)); }
    A(c->alpha.alloc(36 * N * static_cast<size_t>(std::max(1, c->levels_cap)))); A(c->gamma.alloc(36 * N * static_cast<size_t>(std::max(1, c->levels_cap))));
    for (DevBuf<double>* b : {&c->xs, &c->r, &c->z, &c->p, &c->q, &c->t0, &c->t1}) A(b->alloc(6 * N));
    A(c->part.alloc(std::max<size_t>(div_up(static_cast<int>(6 * N), PG_VB), div_up(static_cast<int>(N), 256)) + 1));
    A(c->st.alloc(1)); A(c->h_st.alloc(1)); A(c->h_io.alloc(std::max(7 * N, E)));
    if (rc == SCAL_OK) rc = c->stream.acquire(cfg->device, lane);
    if (rc == SCAL_OK && (hipMemsetAsync(c->st.p, 0, sizeof(PgState), c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)) {
        set_error("scal_posegraph_create: initialisation failed");
        rc = SCAL_E_HIP;
    }
    if (rc != SCAL_OK) {
        delete c;
        return rc;
    }
    // edge 0: the prior's slot
    c->h_ei.assign(1, 0), c->h_ej.assign(1, -1), c->h_ez.assign(7, 0.0), c->h_esi.assign(6, 1.0), c->h_ek.assign(1, 0.0);
    *out = c;
    return SCAL_OK;
}

extern "C" int scal_posegraph_create(const scal_posegraph_config* cfg, scal_posegraph_t** out) { return posegraph_create_on_lane(cfg, 0, out); }

extern "C" void scal_posegraph_destroy(scal_posegraph_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

extern "C" int scal_posegraph_set_nodes(scal_posegraph_t* c, const double* pose7, int n) {
    if (!c || !pose7 || n < 1) {
        set_error("scal_posegraph_set_nodes: bad argument");
        return SCAL_E_ARG;
    }
    if (n > c->cfg.max_nodes) {
        set_error("scal_posegraph_set_nodes: %d nodes, capacity is %d", n, c->cfg.max_nodes);
        return SCAL_E_CAPACITY;
    }
    for (int i = 0; i < n; ++i)
        if (!finite7(pose7 + 7 * static_cast<size_t>(i))) {
            set_error("scal_posegraph_set_nodes: pose %d is not finite or has a zero quaternion", i);
            return SCAL_E_ARG;
        }
    if (n != c->n) c->graph_dirty = true;
    c->n = n;
    c->h_x.resize(7 * static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) put_pose(c->h_x, 7 * static_cast<size_t>(i), pose7 + 7 * static_cast<size_t>(i));
    c->weights_valid = false;
    return SCAL_OK;
}

extern "C" int scal_posegraph_set_prior(scal_posegraph_t* c, int node, const double* pose7, const double* variances6) {
    if (!c || !pose7 || !variances6 || node < 0 || node >= c->n || !finite7(pose7) || !variances_ok(variances6)) {
        set_error("scal_posegraph_set_prior: bad argument (node within the nodes set so far, finite pose, variances finite and > 0)");
        return SCAL_E_ARG;
    }
    c->h_ei[0] = node;
    put_pose(c->h_ez, 0, pose7);
    for (int k = 0; k < 6; ++k) c->h_esi[static_cast<size_t>(k)] = 1.0 / std::sqrt(variances6[k]);
    c->have_prior = true, c->graph_dirty = true, c->weights_valid = false;
    return SCAL_OK;
}

extern "C" int scal_posegraph_add_between(scal_posegraph_t* c, int n, const int* i, const int* j, const double* pose7_rel, const double* variances6,
                                          const double* cauchy_k) {
    if (!c || n < 0 || (n > 0 && (!i || !j || !pose7_rel || !variances6))) {
        set_error("scal_posegraph_add_between: bad argument");
        return SCAL_E_ARG;
    }
    const size_t have = c->h_ei.size() - 1;
    if (have + static_cast<size_t>(n) > static_cast<size_t>(c->cfg.max_edges)) {
        set_error("scal_posegraph_add_between: %zu + %d edges, capacity is %d", have, n, c->cfg.max_edges);
        return SCAL_E_CAPACITY;
    }
    for (int e = 0; e < n; ++e) {
        if (i[e] < 0 || i[e] >= c->n || j[e] < 0 || j[e] >= c->n || i[e] == j[e]) {
            set_error("scal_posegraph_add_between: edge %d joins nodes %d and %d (%d nodes set)", e, i[e], j[e], c->n);
            return SCAL_E_ARG;
        }
        if (!finite7(pose7_rel + 7 * static_cast<size_t>(e)) || !variances_ok(variances6 + 6 * static_cast<size_t>(e)) ||
            (cauchy_k && (!std::isfinite(cauchy_k[e]) || cauchy_k[e] < 0))) {
            set_error("scal_posegraph_add_between: edge %d: pose not finite, a variance not finite and > 0, or cauchy_k negative", e);
            return SCAL_E_ARG;
        }
    }
    for (int e = 0; e < n; ++e) {
        c->h_ei.push_back(i[e]), c->h_ej.push_back(j[e]);
        const size_t at = c->h_ez.size();
        c->h_ez.resize(at + 7);
        put_pose(c->h_ez, at, pose7_rel + 7 * static_cast<size_t>(e));
        for (int k = 0; k < 6; ++k) c->h_esi.push_back(1.0 / std::sqrt(variances6[6 * static_cast<size_t>(e) + k]));
        c->h_ek.push_back(cauchy_k ? cauchy_k[e] : 0.0);
    }
    if (n > 0) c->graph_dirty = true, c->weights_valid = false;
    return SCAL_OK;
}

extern "C" int scal_posegraph_clear_edges(scal_posegraph_t* c) {
    if (!c) {
        set_error("scal_posegraph_clear_edges: null argument");
        return SCAL_E_ARG;
    }
    c->h_ei.resize(1), c->h_ej.resize(1), c->h_ez.resize(7), c->h_esi.resize(6), c->h_ek.resize(1);
    c->graph_dirty = true, c->weights_valid = false;
    return SCAL_OK;
}

extern "C" int scal_posegraph_optimize(scal_posegraph_t* c, const scal_posegraph_params* params, scal_posegraph_stats* stats) {
    if (!c) {
        set_error("scal_posegraph_optimize: null argument");
        return SCAL_E_ARG;
    }
    scal_posegraph_params P{};
    if (params) P = *params;
    if (P.max_iterations < 0 || P.max_linear_iterations < 0 || !(P.step_tol >= 0) || !(P.linear_rtol >= 0) || !std::isfinite(P.step_tol) ||
        !std::isfinite(P.linear_rtol)) {
        set_error("scal_posegraph_optimize: parameters must be finite and >= 0 (0 = default)");
        return SCAL_E_ARG;
    }
    const int max_it = P.max_iterations ? P.max_iterations : PG_DEF_MAX_IT, max_lin = P.max_linear_iterations ? P.max_linear_iterations : PG_DEF_MAX_LIN;
    const double step_tol = P.step_tol > 0 ? P.step_tol : PG_DEF_STEP_TOL, rtol = P.linear_rtol > 0 ? P.linear_rtol : PG_DEF_RTOL;
    if (c->n < 1 || !c->have_prior) {
        set_error("scal_posegraph_optimize: needs nodes and a prior");
        return SCAL_E_STATE;
    }
    const int ne = static_cast<int>(c->h_ei.size());
    for (int e = 0; e < ne; ++e)
        if (c->h_ei[e] >= c->n || c->h_ej[e] >= c->n) {
            set_error("scal_posegraph_optimize: %s names node %d, there are %d nodes", e ? "an edge" : "the prior", std::max(c->h_ei[e], c->h_ej[e]), c->n);
            return SCAL_E_STATE;
        }
    SCAL_HIP(hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    if (c->graph_dirty) SCAL_TRY(upload_graph(c));
    std::memcpy(c->h_io.p, c->h_x.data(), sizeof(double) * 7 * c->n);
    SCAL_HIP(hipMemcpyAsync(c->x.p, c->h_io.p, sizeof(double) * 7 * c->n, hipMemcpyHostToDevice, s));
    double* x = c->x.p;
    double* xn = c->xn.p;
    SCAL_TRY(eval_cost(c, x, 0));
    SCAL_TRY(read_state(c));
    double cost = c->h_st.p->cost;
    scal_posegraph_stats S{};
    S.initial_cost = cost;
    double lambda = 0;
    int it = 0, guess = 24;
    bool stop = !std::isfinite(cost);
    while (!stop && it < max_it) {
        SCAL_LAUNCH_PROF("k_pg_linearize<1>", k_pg_linearize<true>, dim3(div_up(ne, 64)), dim3(64), 0, s, ne, x, c->ei.p, c->ej.p, c->ez.p, c->esi.p, c->ek.p,
                         c->A.p, c->bvec.p, c->cost_e.p, c->w_e.p);
        SCAL_LAUNCH_PROF("k_pg_offdiag", k_pg_offdiag, dim3(div_up(36 * ne, 256)), dim3(256), 0, s, ne, c->A.p, c->O.p);
        for (;;) {
            ++it;
            SCAL_TRY(solve(c, lambda, max_lin, rtol, &guess));
            S.linear_iterations += c->h_st.p->iters;
            S.linear_status = c->h_st.p->status;
            if (S.linear_status != 0) {  // bound hit or breakdown: the last accepted poses stand
                stop = true;
                break;
            }
            SCAL_LAUNCH_PROF("k_pg_retract", k_pg_retract, dim3(div_up(c->n, 256)), dim3(256), 0, s, c->n, x, c->xs.p, xn, c->part.p);
            SCAL_TRY(eval_cost(c, xn, div_up(c->n, 256)));
            SCAL_TRY(read_state(c));
            const double cn = c->h_st.p->cost, step = c->h_st.p->step_max;
            S.last_step_max = step;
            const bool ok = std::isfinite(cn) && cn <= cost;
            if (ok) {
                std::swap(x, xn);
                cost = cn, lambda = 0;
            } else {
                lambda = lambda == 0 ? PG_LAMBDA_FIRST : lambda * PG_LAMBDA_FACTOR;
            }
            if (step < step_tol) S.converged = 1;
            if (ok || S.converged || it >= max_it || lambda > PG_LAMBDA_MAX) break;
        }
        if (S.converged || lambda > PG_LAMBDA_MAX) break;
    }
    // cost and weights at the returned estimate
    SCAL_TRY(eval_cost(c, x, 0));
    SCAL_HIP(hipMemcpyAsync(c->h_io.p, x, sizeof(double) * 7 * c->n, hipMemcpyDeviceToHost, s));
    SCAL_TRY(read_state(c));
    std::memcpy(c->h_x.data(), c->h_io.p, sizeof(double) * 7 * c->n);
    S.iterations = it;
    S.final_cost = c->h_st.p->cost;
    c->weights_valid = true;
    if (stats) *stats = S;
    return SCAL_OK;
}

extern "C" int scal_posegraph_get_nodes(scal_posegraph_t* c, double* pose7, int n) {
    if (!c || !pose7 || n != c->n || n < 1) {
        set_error("scal_posegraph_get_nodes: bad argument (n must be the number of nodes)");
        return SCAL_E_ARG;
    }
    std::memcpy(pose7, c->h_x.data(), sizeof(double) * 7 * static_cast<size_t>(n));
    return SCAL_OK;
}

extern "C" int scal_posegraph_get_edge_weights(scal_posegraph_t* c, double* w, int n) {
    if (!c || n != static_cast<int>(c->h_ei.size()) - 1 || (n > 0 && !w)) {
        set_error("scal_posegraph_get_edge_weights: bad argument (n must be the number of edges)");
        return SCAL_E_ARG;
    }
    if (!c->weights_valid) {
        set_error("scal_posegraph_get_edge_weights: no optimize has run on these edges");
        return SCAL_E_STATE;
    }
    if (n == 0) return SCAL_OK;
    SCAL_HIP(hipSetDevice(c->cfg.device));
    SCAL_HIP(hipMemcpyAsync(c->h_io.p, c->w_e.p + 1, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    SCAL_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(w, c->h_io.p, sizeof(double) * static_cast<size_t>(n));
    return SCAL_OK;
}
