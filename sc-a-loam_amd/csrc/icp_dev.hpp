// The device half of the ICP correspondence step, shared by the single alignment (icp.hip) and the multiview refine (refine.hip),
// which is held to it bit for bit: the same nearest neighbour, the same key, the same order of every f32 and f64 operation.  What
// differs between the two - where a cell's points are found, which candidates are admissible, which point a thread owns - comes in
// as an argument; the arithmetic is written here once.  The host half is icp_host.hpp.
#pragma once
#include "device_utils.hpp"

namespace scal {

constexpr int ICP_NSUM = 17;           // n, sum p[3], sum q[3], sum q p^T[9], sum d^2
constexpr int ICP_PLANE_NSUM = 32;     // point-to-plane: n, 21 of a a^T, a r[6], r r, sum d, n any, sum d any (SCAL_ICP_PLANE_NSUM)
constexpr int ICP_RINGS = 3;          // rings of cells the grid search examines before it gives a query up
constexpr int ICP_QPT = 4;             // dense sweep: queries per thread
constexpr int ICP_QT = 256 * ICP_QPT;  //              queries per workgroup
constexpr int ICP_TC = 2048;           //              targets per workgroup

// (f32 squared distance, target index): the smallest key is the nearest point, the lowest index among equal distances
__device__ __forceinline__ unsigned long long icp_key(float d, unsigned idx) {
    return (static_cast<unsigned long long>(__float_as_uint(d)) << 32) | idx;
}

// ---- ring search: one wave, one query ---------------------------------------------------------------------------------------------
// The target's points lie bucketed into cubic cells of width `cell`, in cell order in sorted[] with their original index in .w.
// The wave examines the cube of cells around the query's cell (cx, cy, cz) ring by ring.  After ring k every unexamined point lies
// more than k cell widths away, so the search stops as soon as the best squared distance is below ((k - 0.05) cell)^2 (the margin
// covers the f32 cell assignment of either point); keys are those of the dense sweep, so equal distances still resolve to the
// lowest index.  Returns whether the query was settled within ICP_RINGS rings; bk is then the nearest point's key.
//   lookup(x, y, z, s0, cnt)  the points of cell (x, y, z) are sorted[s0 .. s0 + cnt); leaves both alone where there is no such cell
//   admit(idx)                whether the target point with original index idx is a candidate at all
template <class Lookup, class Admit>
__device__ __forceinline__ bool icp_ring_search(const float4& q, int cx, int cy, int cz, float cell, const float4* __restrict__ sorted, Lookup lookup,
                                                Admit admit, unsigned long long& bk) {
    const int lane = lane_id();
    bk = ~0ull;
    bool done = false;
    for (int k = 1; k <= ICP_RINGS && !done; ++k) {
        const int w = 2 * k + 1, ncube = w * w * w;
        for (int j0 = 0; j0 < ncube; j0 += 64) {  // 64 cells at a time, one per lane
            const int j = j0 + lane;
            int s0 = 0, cnt = 0;
            if (j < ncube) {
                const int jz = j / (w * w), rem = j - jz * w * w, jy = rem / w, jx = rem - jy * w;
                const int ax = jx - k, ay = jy - k, az = jz - k;
                const bool fresh = k == 1 || max(max(abs(ax), abs(ay)), abs(az)) == k;  // inner cells were examined in an earlier ring
                if (fresh) lookup(cx + ax, cy + ay, cz + az, s0, cnt);
            }
            // the points of these cells as one list spread over the lanes: candidate t belongs to the lane whose running count
            // first exceeds t (six-step search over the inclusive scan), so a crowded cell costs no lane more than an empty one
            const int incl = wave_inclusive_scan(cnt);
            const int total = __shfl(incl, 63, 64);
            const int excl = incl - cnt;
            for (int base = 0; base < total; base += 64) {
                const int t = base + lane;
                int owner = 0;
#pragma unroll
                for (int step = 32; step > 0; step >>= 1) {
                    const int v = __shfl(incl, owner + step - 1, 64);
                    if (v <= t) owner += step;
                }
                owner = min(owner, 63);
                const int idx = __shfl(s0, owner, 64) + (t - __shfl(excl, owner, 64));
                if (t < total) {
                    const float4 p = sorted[idx];
                    const int ti = __float_as_int(p.w);
                    if (admit(ti)) {
                        const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
                        float d = dx * dx;  // the dense sweep's arithmetic
                        d += dy * dy;
                        d += dz * dz;
                        if (d < 3.4e38f) {
                            const unsigned long long key = icp_key(d, static_cast<unsigned>(ti));
                            bk = key < bk ? key : bk;
                        }
                    }
                }
            }
        }
        bk = wave_min_u64(bk);
        const float bound = (static_cast<float>(k) - 0.05f) * cell;
        done = bk != ~0ull && __uint_as_float(static_cast<unsigned>(bk >> 32)) < bound * bound;
    }
    return done;
}

// ---- dense sweep: one workgroup, one (query tile, target chunk) pair -----------------------------------------------------------------
// Queries q0 .. q0 + ICP_QT of the caller's numbering - query(qi) is the point of cur[] behind number qi, -1 beyond the last -
// against targets [t0, t0 + ICP_TC): the chunk staged in LDS and read as wave-wide broadcasts, every thread owns ICP_QPT queries
// and walks the whole chunk (one LDS read feeds ICP_QPT distance evaluations), the chunks' results merged with a 64-bit atomicMin
// on the key.  OWN: the targets of the query's own frame, the index range goff[f] .. goff[f + 1) for f = frame_of[query], are no
// candidates.  A caller that runs several pairs puts a __syncthreads() between them.
template <bool OWN, class Query>
__device__ __forceinline__ void icp_dense_tile(const float4* __restrict__ cur, const float4* __restrict__ tgt, int n_tgt, int t0, int q0, Query query,
                                               const int* __restrict__ frame_of, const int* __restrict__ goff,
                                               unsigned long long* __restrict__ best) {
    __shared__ float4 st[ICP_TC];
    const int tn = min(ICP_TC, n_tgt - t0);
    for (int i = threadIdx.x; i < tn; i += 256) st[i] = tgt[t0 + i];
    __syncthreads();
    float qx[ICP_QPT], qy[ICP_QPT], qz[ICP_QPT], bd[ICP_QPT];
    int bi[ICP_QPT], qid[ICP_QPT], own0[ICP_QPT];
    unsigned own_n[ICP_QPT];
#pragma unroll
    for (int u = 0; u < ICP_QPT; ++u) {
        qid[u] = query(q0 + u * 256 + static_cast<int>(threadIdx.x));
        const float4 q = qid[u] >= 0 ? cur[qid[u]] : make_float4(0.f, 0.f, 0.f, 0.f);
        own0[u] = 0, own_n[u] = 0u;
        if (OWN) {
            const int f = qid[u] >= 0 ? frame_of[qid[u]] : 0;
            own0[u] = goff[f] - t0, own_n[u] = qid[u] >= 0 ? static_cast<unsigned>(goff[f + 1] - goff[f]) : 0u;
        }
        qx[u] = q.x, qy[u] = q.y, qz[u] = q.z, bd[u] = 3.4e38f, bi[u] = -1;
    }
#pragma unroll 2
    for (int t = 0; t < tn; ++t) {
        const float4 p = st[t];
#pragma unroll
        for (int u = 0; u < ICP_QPT; ++u) {
            const float dx = qx[u] - p.x, dy = qy[u] - p.y, dz = qz[u] - p.z;
            float d = dx * dx;  // FLANN L2_Simple<float>, the metric of pcl::KdTreeFLANN
            d += dy * dy;
            d += dz * dz;
            // ascending t: the lowest index of equal distances is kept
            if (d < bd[u] && (!OWN || static_cast<unsigned>(t - own0[u]) >= own_n[u])) bd[u] = d, bi[u] = t;
        }
    }
#pragma unroll
    for (int u = 0; u < ICP_QPT; ++u) {
        if (qid[u] >= 0 && bi[u] >= 0) atomicMin(&best[qid[u]], icp_key(bd[u], static_cast<unsigned>(t0 + bi[u])));
    }
}

// ---- the tail of both sums below: a workgroup of 256 threads, NS f64 terms a thread ----------------------------------------------------
// Every sum: wave_sum, then the four waves as ((r0 + r1) + r2) + r3 -> partials[0 .. NS).  The kernels and their CPU restatements
// are held to this order of additions bit for bit.
template <int NS>
__device__ __forceinline__ void icp_block_sums(const double (&v)[NS], double* __restrict__ partials) {
    __shared__ double red[4][NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double s = wave_sum(v[k]);
        if (lane_id() == 0) red[wave_id()][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NS) partials[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- the 17 correspondence sums of one workgroup of 256 source points ----------------------------------------------------------------
// Thread t owns source point i (has == false: none).  Reads its key and resets it for the next sweep; a correspondence within the
// cap (max2, squared) adds 1, p, q, q p^T and d^2 in f64; icp_block_sums -> partials[0 .. 17).
__device__ __forceinline__ void icp_corr_sums(const float4* __restrict__ cur, const float4* __restrict__ tgt, unsigned long long* __restrict__ best,
                                              float max2, int i, bool has, double* __restrict__ partials) {
    double v[ICP_NSUM];
#pragma unroll
    for (int k = 0; k < ICP_NSUM; ++k) v[k] = 0.0;
    if (has) {
        const unsigned long long key = best[i];
        best[i] = ~0ull;
        const float d = __uint_as_float(static_cast<unsigned>(key >> 32));
        if (key != ~0ull && !(d > max2)) {
            const float4 p = cur[i];
            const float4 q = tgt[static_cast<unsigned>(key & 0xffffffffu)];
            v[0] = 1.0;
            v[1] = p.x, v[2] = p.y, v[3] = p.z;
            v[4] = q.x, v[5] = q.y, v[6] = q.z;
            const double qq[3] = {q.x, q.y, q.z}, pp[3] = {p.x, p.y, p.z};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[7 + 3 * r + c] = qq[r] * pp[c];
            v[16] = d;
        }
    }
    icp_block_sums(v, partials);
}

// ---- the 32 point-to-plane sums of one workgroup of 256 source points (scal_icp_align_plane; the header has the definition) -----------
// The arguments of icp_corr_sums and the target's normals nc[] (normal, curvature; scal_nbr_normals' layout).  Reads the key and
// resets it; gathers tgt[idx] and nc[idx]; a correspondence within the cap whose normal is finite makes the row a = (p x n, n),
// r = (q - p).n in f64 and adds 1, a a^T's upper triangle, a r, r r and d; every query with a neighbour adds 1 and d to [30], [31]
// whatever the cap and the normal.  icp_block_sums -> partials[0 .. 32).
__device__ __forceinline__ void icp_plane_sums(const float4* __restrict__ cur, const float4* __restrict__ tgt, const float4* __restrict__ nc,
                                               unsigned long long* __restrict__ best, float max2, int i, bool has, double* __restrict__ partials) {
    double v[ICP_PLANE_NSUM];
#pragma unroll
    for (int k = 0; k < ICP_PLANE_NSUM; ++k) v[k] = 0.0;
    if (has) {
        const unsigned long long key = best[i];
        best[i] = ~0ull;
        if (key != ~0ull) {
            const float d = __uint_as_float(static_cast<unsigned>(key >> 32));
            v[30] = 1.0, v[31] = d;
            if (!(d > max2)) {
                const unsigned idx = static_cast<unsigned>(key & 0xffffffffu);
                const float4 nf = nc[idx];
                if (fabsf(nf.x) <= 3.4028235e38f && fabsf(nf.y) <= 3.4028235e38f && fabsf(nf.z) <= 3.4028235e38f) {  // finite: false for NaN
                    const float4 pf = cur[i], qf = tgt[idx];
                    const double px = pf.x, py = pf.y, pz = pf.z, nx = nf.x, ny = nf.y, nz = nf.z;
                    const double a[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
                    const double ex = static_cast<double>(qf.x) - px, ey = static_cast<double>(qf.y) - py, ez = static_cast<double>(qf.z) - pz;
                    const double r = (ex * nx + ey * ny) + ez * nz;
                    v[0] = 1.0;
                    int k = 1;
#pragma unroll
                    for (int r0 = 0; r0 < 6; ++r0)
#pragma unroll
                        for (int c0 = r0; c0 < 6; ++c0) v[k++] = a[r0] * a[c0];
#pragma unroll
                    for (int r0 = 0; r0 < 6; ++r0) v[22 + r0] = a[r0] * r;
                    v[28] = r * r;
                    v[29] = d;
                }
            }
        }
    }
    icp_block_sums(v, partials);
}

// ---- the rigid increment applied to a point, f32 as PCL does: rows of the 3x4 matrix m, .w kept ---------------------------------------
__device__ __forceinline__ float4 icp_transform(const float* __restrict__ m, const float4& p) {
    float4 o;
    o.x = ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3];
    o.y = ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7];
    o.z = ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11];
    o.w = p.w;
    return o;
}

}  // namespace scal
