// Radius neighbour index (scal_nbr_*, include/scaloam_hip.h has the semantics; python/scaloam/nbr.py is the CPU restatement the device
// equals bit for bit): per query the number of index records within r (saturating u16) and the smallest f32 d^2 among them.  The
// primitive behind the session map diff and the radius outlier filter.
//
// One context, one stream (lane 0).  set_index:
//   SparseCells::build (cell_index.hpp, the index refine.hip uses as well): records in cell order with their input position in .w,
//   the cells' [start, end) ranges behind an open-addressing hash table; its two launches are timed as k_nb_keys and k_nb_index.
// query: the queries are sorted by the same key (SparseCells::sort, k_nb_gather; a self query reuses the index's own order), then
//   k_nb_query: one wave per 64 consecutive sorted queries, a query per lane.  The wave takes the runs of equal cells among its 64
//   queries one after the other (a run that crosses a multiple of 64 is cut there): such a piece is a work item - up to 64 queries of
//   ONE cell, so the 27 cell ranges around it are wave-uniform.  Lanes 0 .. 26 look one range up each; the wave then streams the
//   ranges' records 64 at a time, one 16-byte load per lane, and hands them round by v_readlane_b32 with a uniform lane index: the
//   record's x, y, z arrive as scalar operands of the subtractions, every lane tests the record against its own query.  Count and
//   minimum stay in registers and are written once, through the permutation, into the caller's order: no atomics on the outputs.
//   An LDS stage for the broadcast was not built: it would add a ds_write / s_waitcnt / ds_read round trip per 64 records to save
//   three VALU issues per record; see DESIGN.md for the instruction count of the inner loop as built.
//   The traversal - work items, ranges, batches, statistics - is one function, nb_visit, with what happens to a record passed in.
// knn (scal_nbr_knn*): the same sorted queries and the same index, then k_nb_knn<KC>: the same traversal
//   (written out once more in nb_knn_lists, see there) with a sorted k-best list of 64-bit keys (d2 bits, input position) per lane in LDS (nb_knn_lists); the rows go out padded with -1 / +inf,
//   into staging that exists only once a host k-NN entry point has been called.
// normals (scal_nbr_normals*): k_nb_normals<KC> builds the same lists, then fits the plane where the list
//   is - centroid, covariance and a cyclic Jacobi in f64 per lane - and writes 20 bytes per query.  It finds a neighbour's record
//   through a position -> place table (k_nb_slots), which exists only once a normals entry point has been called.
// Host side: every entry point is the argument check (nb_check), the queries in cell order (nb_queries), where the kernel writes
//   (nb_out), the launch with the statistics read back (nb_run) and, for a host caller, the download (nb_download).
//
// Cell width.  w = the smallest power of two GREATER than r (never below 2^-62; one cell for everything when r r overflows), cell
// coordinate floor(v * (1 / w)) in f32.  1 / w is a power of two, so the product is exact and so is the floor: the coordinate is
// floor(v / w) of the real numbers (f32 denormals are on for gfx9; a product that overflows gives +-inf, which the clamp takes; one
// that is lost below the denormals belongs to a |v| so far below w that no float lies between it and the cell's edge).
// Claim: a pair that passes d2 <= r2 has |qv - pv| < w on every axis, so its cell coordinates differ by at most 1.  Every term of d2
// is >= 0 and rounding is monotone, so fl(dv'^2) <= d2 <= r2 for dv' = fl(qv - pv).  r < w are floats, so r <= w (1 - 2^-24) and
// r2 = fl(r r) <= w^2 (1 - 2^-23); fl(dv'^2) <= that forces dv' < w, i.e. dv' <= w (1 - 2^-24), and the true difference is within
// half an ulp of dv': |qv - pv| <= w (1 - 2^-24) + w 2^-25 < w.  (With w = r for a power of two r the claim fails: q = 0.5,
// p = -2^-30, r = 0.5 has fl(q - p) = 0.5 and passes, and the cells are 1 and -1.)  Where the squares fall below the normal range
// (r2 or dv'^2 < 2^-126) dv' < 2^-63 < w by the lower bound on w.  Clamping the coordinate to the key range is monotone and keeps
// the difference <= 1.  So the 27 cells around a query's cell hold every record within r: an argument, no slack factor; the cost is
// a cell up to twice r wide.
#include "common.hpp"
#include "cell_index.hpp"
#include <algorithm>
#include <cmath>
#include <limits>
#include <type_traits>

namespace scal {

constexpr unsigned NB_INF = 0x7f800000u;

__device__ __forceinline__ bool nb_finite(const float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// sorted position i: the record with its input position in .w (the queries of a set, in cell order)
__global__ void __launch_bounds__(256) k_nb_gather(const int* __restrict__ vals, int n, const float4* __restrict__ pts, float4* __restrict__ sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int idx = vals[i];
    float4 p = pts[idx];
    p.w = __int_as_float(idx);
    sorted[i] = p;
}

__device__ __forceinline__ float nb_lane_f(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// The traversal of the query kernels, for one wave with a query per lane (fin: the lane holds a finite one).  The wave takes
// the runs of equal cells among its queries one after the other: the lowest lane still waiting leads, `mine` are the lanes of its
// cell - a work item.  Lanes 0 .. 26 look the 27 ranges around that cell up, the wave streams their records 64 at a time and hands
// them round by v_readlane_b32.  What a kernel does with a record is its own:
//   begin()                at the start of a work item,
//   visit(mine, d2, p, j)  per record: p is the batch (a record per lane), j the uniform lane the record sits in, d2 the f32 distance
//                          of the lane's own query to it - on every lane, `mine` or not,
//   end(mine)              at the end of a work item.
// stats: [0] (query, record) pairs tested, [1] work items - the same for every kernel, since they depend on nothing a callable does.
template <class Begin, class Visit, class End>
__device__ __forceinline__ void nb_visit(const float4 q, const bool fin, const int lane, const CellView ix,
                                         unsigned long long* __restrict__ stats, Begin begin, Visit visit, End end) {
    const int cx = ix.cx(q.x), cy = ix.cx(q.y), cz = ix.cz(q.z);
    unsigned long long waiting = __ballot(fin), pairs = 0;
    int items = 0;
    while (waiting) {
        const int leader = __ffsll(static_cast<long long>(waiting)) - 1;
        const int lx = __builtin_amdgcn_readlane(cx, leader), ly = __builtin_amdgcn_readlane(cy, leader), lz = __builtin_amdgcn_readlane(cz, leader);
        const bool mine = fin && cx == lx && cy == ly && cz == lz;
        const unsigned long long peers = __ballot(mine);  // holds the leader's bit: every round takes lanes out of `waiting`
        int s0 = 0, e0 = 0;
        if (lane < 27) {
            const int az = lane / 9, ay = (lane - 9 * az) / 3, ax = lane - 9 * az - 3 * ay;
            int2 r;
            if (ix.find(lx + ax - 1, ly + ay - 1, lz + az - 1, r)) s0 = r.x, e0 = r.y;
        }
        begin();
        int seen = 0;
        for (int c = 0; c < 27; ++c) {
            const int s = __builtin_amdgcn_readlane(s0, c), e = __builtin_amdgcn_readlane(e0, c);
            seen += e - s;
            for (int b = s; b < e; b += 64) {
                const int m = __builtin_amdgcn_readfirstlane(min(64, e - b));  // keeps the loop counter on the scalar side
                const float4 p = lane < m ? ix.sorted[b + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
                for (int j = 0; j < m; ++j) {
                    const float dx = q.x - nb_lane_f(p.x, j), dy = q.y - nb_lane_f(p.y, j), dz = q.z - nb_lane_f(p.z, j);
                    visit(mine, (dx * dx + dy * dy) + dz * dz, p, j);
                }
            }
        }
        end(mine);
        pairs += static_cast<unsigned long long>(seen) * __popcll(peers);
        ++items;
        waiting &= ~peers;
    }
    if (lane == 0 && items) {
        atomicAdd(stats, pairs);
        atomicAdd(stats + 1, static_cast<unsigned long long>(items));
    }
}

// qs: nq queries in cell order with their output position in .w; a wave per 64 of them (four waves per block, independent).
// cnt_out / d2_out may be null.
__global__ void __launch_bounds__(256) k_nb_query(const float4* __restrict__ qs, int nq, float r2, const CellView ix,
                                                  unsigned short* __restrict__ cnt_out, float* __restrict__ d2_out, unsigned long long* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int i = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + lane;
    const bool have = i < nq;
    const float4 q = have ? qs[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool fin = have && nb_finite(q);
    const int out = __float_as_int(q.w);
    if (have && !fin) {  // a query that is not finite: count 0, +inf
        if (cnt_out) cnt_out[out] = 0;
        if (d2_out) d2_out[out] = __uint_as_float(NB_INF);
    }
    int count = 0;
    float best = __uint_as_float(NB_INF);
    nb_visit(
        q, fin, lane, ix, stats, [&] { count = 0, best = __uint_as_float(NB_INF); },
        [&](bool, float d2, const float4&, int) {  // every lane counts, its own work item or not: a predicate here is an issue per record
            if (d2 <= r2) {
                ++count;
                best = d2 < best ? d2 : best;  // no NaN can arrive here: both records are finite
            }
        },
        [&](bool mine) {
            if (mine) {
                if (cnt_out) cnt_out[out] = static_cast<unsigned short>(min(count, 65535));
                if (d2_out) d2_out[out] = best;
            }
        });
}

constexpr unsigned long long NB_NO_KEY = ~0ull;  // above every key: d2 bits are at most +inf's, positions below 2^30

// The k nearest candidates of every query (d2 <= r2), ordered by (d2, input position): nb_visit's traversal with a k-best list per lane
// in place of count and minimum.  A list entry is the 64-bit key (d2 bits << 32) | input position: d2 is >= +0 and not NaN, so its bits
// order as its value does, and the whole key orders as (d2, position) however the records arrive from the cells.  The lists are in
// LDS as list[slot][lane], so one slot of the wave's 64 lanes is 512 contiguous bytes: ds_read_b64 takes it in two conflict-free
// halves.  A lane's list is kept sorted; its length and its current k-th key (NB_NO_KEY until the list is full) are in registers, so a
// record that does not enter costs the distance, one 64-bit compare and no LDS access.  One wave per block: the waves share nothing,
// and the block's LDS is KC * 512 bytes for the class KC >= k the host picks (8, 16, 32, 64), which is what sets the waves per CU.
// Only a lane that holds a finite query touches its column, and only in the work item it belongs to.
// nb_knn_lists fills the lane's column (slot s at mylist[64 * s]) and returns its length; k_nb_knn and k_nb_normals start with it.
// It is NOT a use of nb_visit: the traversal is written out here a second time, statement for statement, and has to be kept equal to
// nb_visit by hand (the tests pin equal statistics across the calls).  With the insertion passed to nb_visit as a callable - or
// to any other function - the record and insertion loops compile to the same instructions in other registers, and k_nb_knn and
// k_nb_normals then run between 4 % faster and 2 % slower, which is outside what identical builds show.
__device__ __forceinline__ int nb_knn_lists(const float4 q, const bool fin, const int lane, const int k, const float r2, const CellView ix,
                                            unsigned long long* const mylist, unsigned long long* __restrict__ stats) {
    const int cx = ix.cx(q.x), cy = ix.cx(q.y), cz = ix.cz(q.z);
    int len = 0;
    unsigned long long kth = NB_NO_KEY;
    unsigned long long waiting = __ballot(fin), pairs = 0;
    int items = 0;
    while (waiting) {
        const int leader = __ffsll(static_cast<long long>(waiting)) - 1;
        const int lx = __builtin_amdgcn_readlane(cx, leader), ly = __builtin_amdgcn_readlane(cy, leader), lz = __builtin_amdgcn_readlane(cz, leader);
        const bool mine = fin && cx == lx && cy == ly && cz == lz;
        const unsigned long long peers = __ballot(mine);
        int s0 = 0, e0 = 0;
        if (lane < 27) {
            const int az = lane / 9, ay = (lane - 9 * az) / 3, ax = lane - 9 * az - 3 * ay;
            int2 r;
            if (ix.find(lx + ax - 1, ly + ay - 1, lz + az - 1, r)) s0 = r.x, e0 = r.y;
        }
        int seen = 0;
        for (int c = 0; c < 27; ++c) {
            const int s = __builtin_amdgcn_readlane(s0, c), e = __builtin_amdgcn_readlane(e0, c);
            seen += e - s;
            for (int b = s; b < e; b += 64) {
                const int m = __builtin_amdgcn_readfirstlane(min(64, e - b));
                const float4 p = lane < m ? ix.sorted[b + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
                for (int j = 0; j < m; ++j) {
                    const float dx = q.x - nb_lane_f(p.x, j), dy = q.y - nb_lane_f(p.y, j), dz = q.z - nb_lane_f(p.z, j);
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const unsigned pos = static_cast<unsigned>(__builtin_amdgcn_readlane(__float_as_int(p.w), j));
                    const unsigned long long key = (static_cast<unsigned long long>(__float_as_uint(d2)) << 32) | pos;
                    if (mine && d2 <= r2 && key < kth) {
                        // the list is sorted in slots [0, len); a full list drops its last entry
                        int t = len < k ? len : k - 1;
                        while (t > 0) {
                            const unsigned long long prev = mylist[64 * (t - 1)];
                            if (prev < key) break;
                            mylist[64 * t] = prev;
                            --t;
                        }
                        mylist[64 * t] = key;
                        len += len < k;
                        if (len == k) kth = mylist[64 * (k - 1)];
                    }
                }
            }
        }
        pairs += static_cast<unsigned long long>(seen) * __popcll(peers);
        ++items;
        waiting &= ~peers;
    }
    if (lane == 0 && items) {
        atomicAdd(stats, pairs);
        atomicAdd(stats + 1, static_cast<unsigned long long>(items));
    }
    return len;
}

// idx_out / d2_out [nq][k] may be null.
template <int KC>
__global__ void __launch_bounds__(64) k_nb_knn(const float4* __restrict__ qs, int nq, int k, float r2, const CellView ix,
                                               int* __restrict__ idx_out, float* __restrict__ d2_out, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long list[KC * 64];
    const int lane = threadIdx.x;
    const long long i = static_cast<long long>(blockIdx.x) * 64 + lane;
    const bool have = i < nq;
    const float4 q = have ? qs[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool fin = have && nb_finite(q);
    const size_t row = static_cast<size_t>(__float_as_int(q.w)) * static_cast<size_t>(k);
    unsigned long long* const mylist = list + lane;  // slot s at mylist[64 * s]
    const int len = nb_knn_lists(q, fin, lane, k, r2, ix, mylist, stats);
    if (have) {  // a query that is not finite has len 0: a fully padded row
        for (int s = 0; s < k; ++s) {
            const bool in = s < len;
            const unsigned long long key = in ? mylist[64 * s] : 0ull;
            if (idx_out) idx_out[row + s] = in ? static_cast<int>(static_cast<unsigned>(key)) : -1;
            if (d2_out) d2_out[row + s] = __uint_as_float(in ? static_cast<unsigned>(key >> 32) : NB_INF);
        }
    }
}

constexpr unsigned NB_QNAN = 0x7fc00000u;  // SCAL_NBR_NAN_BITS

// position -> slot: sorted[] is in cell order and a list entry names its record by input position
__global__ void __launch_bounds__(256) k_nb_slots(const float4* __restrict__ sorted, int n, int* __restrict__ slot_of) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    slot_of[__float_as_int(sorted[i].w)] = i;
}

// One Jacobi rotation of the symmetric 3x3 A (pair p, q; r the third index) and of V's columns p and q, in the header's operation order.
// a_pq == 0 leaves everything untouched.  All operands are named scalars: A and V stay in registers.
__device__ __forceinline__ void nb_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p,
                                          double& v1q, double& v2p, double& v2q) {
    if (apq != 0.0) {
        const double theta = (aqq - app) / (2.0 * apq);
        const double ta = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double t = theta < 0.0 ? -ta : ta;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, h = t * apq;
        app -= h, aqq += h, apq = 0.0;
        const double rp = c * arp - s * arq, rq = s * arp + c * arq;
        arp = rp, arq = rq;
        const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q, a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
        const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
        v0p = a0, v0q = b0, v1p = a1, v1q = b1, v2p = a2, v2q = b2;
    }
}

// Normal, curvature and point-to-plane distance per query (scal_nbr_normals*): nb_knn_lists, then the fit
// where the list is.  The lane walks its column in slot order twice - centroid, then covariance about it - fetching each
// neighbour's record from sorted[] through slot_of (the first walk leaves the slot in the entry for the second), runs the cyclic Jacobi
// of the header in f64 on 15 named scalars and writes one float4 and one float through .w: no [n][k] buffer exists on this path.
// Lanes without a fit (fewer than 3 neighbours, no query) carry A = 0 through the sweeps, which is a no-op, so the wave leaves the
// sweep loop together on a ballot once every lane's off-diagonals are exactly 0.  nc_out / dist_out may be null.
// The index comes as loose arguments, not as a CellView like k_nb_query's and k_nb_knn's: with the view as the argument this kernel
// ran 9 % slower at k = 21 (profiles/cell_index_ab.txt), with the view put together in here it runs as before.
template <int KC>
__global__ void __launch_bounds__(64) k_nb_normals(const float4* __restrict__ qs, int nq, int k, float inv, float r2, const unsigned long long* __restrict__ hkeys,
                                                   const int2* __restrict__ hrange, unsigned mask, const float4* __restrict__ sorted,
                                                   const int* __restrict__ slot_of, int use_vp, double vpx, double vpy, double vpz,
                                                   float4* __restrict__ nc_out, float* __restrict__ dist_out, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long list[KC * 64];
    const int lane = threadIdx.x;
    const long long i = static_cast<long long>(blockIdx.x) * 64 + lane;
    const bool have = i < nq;
    const float4 q = have ? qs[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool fin = have && nb_finite(q);
    const int out = __float_as_int(q.w);
    unsigned long long* const mylist = list + lane;
    const CellView ix{hkeys, hrange, sorted, mask, inv};
    const int len = nb_knn_lists(q, fin, lane, k, r2, ix, mylist, stats);
    const int m = len >= 3 ? len : 0;
    const double dm = static_cast<double>(m);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int s = 0; s < m; ++s) {
        const int slot = slot_of[static_cast<unsigned>(mylist[64 * s])];
        mylist[64 * s] = static_cast<unsigned long long>(slot);
        const float4 p = sorted[slot];
        sx += static_cast<double>(p.x), sy += static_cast<double>(p.y), sz += static_cast<double>(p.z);
    }
    const double cx = sx / dm, cy = sy / dm, cz = sz / dm;  // NaN where m is 0: never used
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (int s = 0; s < m; ++s) {
        const float4 p = sorted[static_cast<int>(mylist[64 * s])];
        const double dx = static_cast<double>(p.x) - cx, dy = static_cast<double>(p.y) - cy, dz = static_cast<double>(p.z) - cz;
        a00 += dx * dx, a01 += dx * dy, a02 += dx * dz, a11 += dy * dy, a12 += dy * dz, a22 += dz * dz;
    }
    if (m) a00 /= dm, a01 /= dm, a02 /= dm, a11 /= dm, a12 /= dm, a22 /= dm;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < 8; ++sweep) {
        if (!__ballot(a01 != 0.0 || a02 != 0.0 || a12 != 0.0)) break;
        nb_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        nb_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        nb_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    if (!have) return;
    float4 nc = make_float4(__uint_as_float(NB_QNAN), __uint_as_float(NB_QNAN), __uint_as_float(NB_QNAN), __uint_as_float(NB_QNAN));
    float dist = __uint_as_float(NB_QNAN);
    if (m) {
        int j = 0;
        double lmin = a00;
        if (a11 < lmin) lmin = a11, j = 1;
        if (a22 < lmin) lmin = a22, j = 2;
        double nx = j == 0 ? v00 : j == 1 ? v01 : v02, ny = j == 0 ? v10 : j == 1 ? v11 : v12, nz = j == 0 ? v20 : j == 1 ? v21 : v22;
        const double tr = (a00 + a11) + a22;
        const double curv = tr > 0.0 ? (lmin > 0.0 ? lmin : 0.0) / tr : 0.0;
        const double qx = static_cast<double>(q.x), qy = static_cast<double>(q.y), qz = static_cast<double>(q.z);
        if (use_vp) {
            const double wx = vpx - qx, wy = vpy - qy, wz = vpz - qz;
            if ((nx * wx + ny * wy) + nz * wz < 0.0) nx = -nx, ny = -ny, nz = -nz;
        }
        const double ex = qx - cx, ey = qy - cy, ez = qz - cz;
        nc = make_float4(static_cast<float>(nx), static_cast<float>(ny), static_cast<float>(nz), static_cast<float>(curv));
        dist = static_cast<float>((nx * ex + ny * ey) + nz * ez);
    }
    if (nc_out) nc_out[out] = nc;
    if (dist_out) dist_out[out] = dist;
}

}  // namespace scal

using namespace scal;

struct scal_nbr {
    scal_nbr_config cfg;
    LaneStream stream;
    int cap = 0;  // max(max_index_points, max_query_points): a self query has as many queries as the index has records
    SparseCells ix;  // the index; its sort takes the query sets as well
    DevBuf<float4> stage, qsorted;  // stage: host records staged in (index or queries), allocated on first use
    DevBuf<unsigned long long> d_stats;
    DevBuf<unsigned short> d_cnt;
    DevBuf<float> d_d2;
    DevBuf<int> d_kidx;   // k-NN rows staged for the host: allocated at the first k-NN call, grown to the largest n * k so far
    DevBuf<float> d_kd2;
    DevBuf<int> slot_of;  // input position -> place in sorted: allocated at the first normals call, refilled there after a new index
    bool slots_ok = false;
    DevBuf<float4> d_nc;  // normals staged for the host, cap entries each, allocated when first asked for
    DevBuf<float> d_dist;
    int n = -1;  // -1: no index set
    float r2 = 0.f;
    long long pairs = 0;
    int work_items = 0;
};

extern "C" int scal_nbr_create(const scal_nbr_config* cfg, scal_nbr_t** out) {
    if (!cfg || !out || cfg->max_index_points < 1 || cfg->max_index_points > (1 << 30) || cfg->max_query_points < 1 || cfg->max_query_points > (1 << 30)) {
        set_error("scal_nbr_create: bad argument");
        return SCAL_E_ARG;
    }
    *out = nullptr;
    SCAL_TRY(select_device(cfg->device));
    auto* c = new scal_nbr();
    c->cfg = *cfg;
    c->cap = std::max(cfg->max_index_points, cfg->max_query_points);
    const size_t nq = static_cast<size_t>(cfg->max_query_points), nc = static_cast<size_t>(c->cap);
    c->ix.set_names("k_nb_keys", "k_nb_index");
    int rc = SCAL_OK;
    auto A = [&](int r) { if (rc == SCAL_OK) rc = r; };
    A(c->stream.acquire(cfg->device, 0));
    A(c->ix.init(cfg->max_index_points, cfg->max_query_points)); A(c->qsorted.alloc(nq));
    A(c->d_stats.alloc(2)); A(c->d_cnt.alloc(nc)); A(c->d_d2.alloc(nc));
    if (rc != SCAL_OK) {
        scal_nbr_destroy(c);
        return rc;
    }
    *out = c;
    return SCAL_OK;
}

extern "C" void scal_nbr_destroy(scal_nbr_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

static int nb_check_index(scal_nbr* c, const char* who, const float* xyzi, int n, double radius) {
    const float r = static_cast<float>(radius);
    if (!c || n < 0 || (n > 0 && !xyzi) || !(radius > 0) || !std::isfinite(radius) || !(r > 0.f) || !std::isfinite(r)) {
        set_error("%s: bad argument (the radius must be finite and > 0 as a float)", who);
        return SCAL_E_ARG;
    }
    if (n > c->cfg.max_index_points) {
        set_error("%s: %d records, max_index_points is %d", who, n, c->cfg.max_index_points);
        return SCAL_E_CAPACITY;
    }
    return SCAL_OK;
}

static int nb_build(scal_nbr* c, const float4* pts, int n, double radius) {
    hipStream_t s = c->stream;
    c->n = -1, c->pairs = 0, c->work_items = 0, c->slots_ok = false;
    const float r = static_cast<float>(radius);
    c->r2 = r * r;
    // 1 / w for w = the smallest power of two > r: r = mant 2^e with mant in [0.5, 1), so w = 2^e
    int e = 0;
    (void)std::frexp(r, &e);
    const float inv = std::isinf(c->r2) ? 0.f : std::ldexp(1.f, -std::max(e, -62));
    SCAL_TRY(c->ix.build(s, pts, n, inv, std::numeric_limits<float>::infinity()));  // every finite record is in a cell
    SCAL_HIP(hipStreamSynchronize(s));  // the caller's records have been read
    c->n = n;
    return SCAL_OK;
}

extern "C" int scal_nbr_set_index(scal_nbr_t* c, const float* xyzi, int n, double radius) {
    SCAL_TRY(nb_check_index(c, "scal_nbr_set_index", xyzi, n, radius));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    c->n = -1;
    if (!c->stage.p) SCAL_TRY(c->stage.alloc(static_cast<size_t>(c->cap)));  // a context fed from the device never needs it
    if (n > 0) SCAL_HIP(hipMemcpyAsync(c->stage.p, xyzi, sizeof(float4) * static_cast<size_t>(n), hipMemcpyHostToDevice, c->stream));
    return nb_build(c, c->stage.p, n, radius);
}

extern "C" int scal_nbr_set_index_device(scal_nbr_t* c, const float* d_xyzi, int n, double radius) {
    SCAL_TRY(nb_check_index(c, "scal_nbr_set_index_device", d_xyzi, n, radius));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    return nb_build(c, reinterpret_cast<const float4*>(d_xyzi), n, radius);
}

enum NbSource { NB_HOST, NB_DEVICE, NB_SELF };  // where a call's queries are: the caller's host or device memory, or the index itself

// kmin: the smallest k the call takes (1: k-NN, 3: normals), 0 for a call without a k.  Refuses in the order ARG, STATE, CAPACITY.
static int nb_check(scal_nbr* c, const char* who, NbSource src, const float* xyzi, int n, int kmin, int k) {
    const bool self = src == NB_SELF;
    if (!c || (!self && (n < 0 || (n > 0 && !xyzi))) || (kmin && (k < kmin || k > SCAL_NBR_MAX_K))) {
        if (kmin) set_error("%s: bad argument (k is %d .. %d)", who, kmin, SCAL_NBR_MAX_K);
        else set_error("%s: bad argument", who);
        return SCAL_E_ARG;
    }
    if (c->n < 0) {
        set_error("%s: no index set", who);
        return SCAL_E_STATE;
    }
    if (!self && n > c->cfg.max_query_points) {
        set_error("%s: %d queries, max_query_points is %d", who, n, c->cfg.max_query_points);
        return SCAL_E_CAPACITY;
    }
    return SCAL_OK;
}

// sorts the n queries at pts into qsorted
static int nb_sort_queries(scal_nbr* c, const float4* pts, int n) {
    if (n == 0) return SCAL_OK;
    SortedPairs sp;
    SCAL_TRY(c->ix.sort(c->stream, pts, n, &sp));
    SCAL_LAUNCH_PROF("k_nb_gather", k_nb_gather, dim3(div_up(n, 256)), dim3(256), 0, c->stream, sp.vals[sp.fixed_sel], n, pts, c->qsorted.p);
    SCAL_HIP(hipGetLastError());
    return SCAL_OK;
}

// a checked call's queries in cell order, output position in .w: *qs, *nq.  A self query runs on the index's own order.
static int nb_queries(scal_nbr* c, NbSource src, const float* xyzi, int n, const float4** qs, int* nq) {
    if (src == NB_SELF) {
        *qs = c->ix.sorted.p, *nq = c->n;
        return SCAL_OK;
    }
    const float4* pts = reinterpret_cast<const float4*>(xyzi);
    if (src == NB_HOST) {
        if (!c->stage.p) SCAL_TRY(c->stage.alloc(static_cast<size_t>(c->cap)));
        if (n > 0) SCAL_HIP(hipMemcpyAsync(c->stage.p, xyzi, sizeof(float4) * static_cast<size_t>(n), hipMemcpyHostToDevice, c->stream));
        pts = c->stage.p;
    }
    SCAL_TRY(nb_sort_queries(c, pts, n));
    *qs = c->qsorted.p, *nq = n;
    return SCAL_OK;
}

// *d: where the kernel writes an output.  A device call's is the caller's buffer; a host caller's is staging of at least m entries,
// allocated or grown when asked for (a failed allocation leaves the buffer empty and the context as it was); null stays null.
template <class T>
static int nb_out(DevBuf<T>& stage, NbSource src, T* user, size_t m, T** d) {
    *d = user;
    if (src == NB_DEVICE || !user) return SCAL_OK;
    if (m && !(stage.p && stage.n >= m)) SCAL_TRY(stage.alloc(m));
    *d = stage.p;
    return SCAL_OK;
}

// launch(stream) runs one query kernel over nq queries; waits, reads the counters
template <class Launch>
static int nb_run(scal_nbr* c, int nq, Launch launch) {
    hipStream_t s = c->stream;
    c->pairs = 0, c->work_items = 0;
    if (nq == 0) return SCAL_OK;
    SCAL_HIP(hipMemsetAsync(c->d_stats.p, 0, 2 * sizeof(unsigned long long), s));
    SCAL_TRY(launch(s));
    SCAL_HIP(hipGetLastError());
    unsigned long long st[2] = {0, 0};
    SCAL_HIP(hipMemcpyAsync(st, c->d_stats.p, sizeof st, hipMemcpyDeviceToHost, s));
    SCAL_HIP(hipStreamSynchronize(s));
    c->pairs = static_cast<long long>(st[0]), c->work_items = static_cast<int>(std::min<unsigned long long>(st[1], 0x7fffffffull));
    return SCAL_OK;
}

// f(the list class KC >= k as a std::integral_constant): the kernels with a k-best list are instantiated for 8, 16, 32, 64
template <class F>
static void nb_list_class(int k, F f) {
    if (k <= 8) f(std::integral_constant<int, 8>{});
    else if (k <= 16) f(std::integral_constant<int, 16>{});
    else if (k <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

// a host caller's outputs, m entries each, out of the staging the kernel wrote them to (either may be null)
template <class A, class B>
static int nb_download(scal_nbr* c, NbSource src, size_t m, A* a, const A* d_a, B* b, const B* d_b) {
    if (src == NB_DEVICE || m == 0) return SCAL_OK;
    hipStream_t s = c->stream;
    if (a) SCAL_HIP(hipMemcpyAsync(a, d_a, sizeof(A) * m, hipMemcpyDeviceToHost, s));
    if (b) SCAL_HIP(hipMemcpyAsync(b, d_b, sizeof(B) * m, hipMemcpyDeviceToHost, s));
    SCAL_HIP(hipStreamSynchronize(s));
    return SCAL_OK;
}

// Each family below is one sequence for its three entry points: check, output staging (before `stage`, so that a failed allocation
// leaves the context as it was), queries in cell order, kernel, download.
static int nb_query(scal_nbr* c, const char* who, NbSource src, const float* xyzi, int n, unsigned short* cnt, float* d2) {
    SCAL_TRY(nb_check(c, who, src, xyzi, n, 0, 0));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    const size_t m = static_cast<size_t>(src == NB_SELF ? c->n : n);
    unsigned short* d_cnt;
    float* d_d2;
    SCAL_TRY(nb_out(c->d_cnt, src, cnt, m, &d_cnt));
    SCAL_TRY(nb_out(c->d_d2, src, d2, m, &d_d2));
    const float4* qs;
    int nq;
    SCAL_TRY(nb_queries(c, src, xyzi, n, &qs, &nq));
    SCAL_TRY(nb_run(c, nq, [&](hipStream_t s) -> int {
        SCAL_LAUNCH_PROF("k_nb_query", k_nb_query, dim3(div_up(nq, 256)), dim3(256), 0, s, qs, nq, c->r2, c->ix.view(), d_cnt, d_d2, c->d_stats.p);
        return SCAL_OK;
    }));
    return nb_download(c, src, m, cnt, d_cnt, d2, d_d2);
}

extern "C" int scal_nbr_query(scal_nbr_t* c, const float* xyzi, int n, unsigned short* count_u16, float* min_d2) {
    return nb_query(c, "scal_nbr_query", NB_HOST, xyzi, n, count_u16, min_d2);
}

extern "C" int scal_nbr_query_device(scal_nbr_t* c, const float* d_xyzi, int n, unsigned short* d_count_u16, float* d_min_d2) {
    return nb_query(c, "scal_nbr_query_device", NB_DEVICE, d_xyzi, n, d_count_u16, d_min_d2);
}

extern "C" int scal_nbr_query_self(scal_nbr_t* c, unsigned short* count_u16, float* min_d2) {
    return nb_query(c, "scal_nbr_query_self", NB_SELF, nullptr, 0, count_u16, min_d2);
}

// the rows are staged in n * k entries, allocated at the first host k-NN call and grown to the largest so far
static int nb_knn(scal_nbr* c, const char* who, NbSource src, const float* xyzi, int n, int k, int* idx, float* d2) {
    SCAL_TRY(nb_check(c, who, src, xyzi, n, 1, k));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    const size_t m = static_cast<size_t>(src == NB_SELF ? c->n : n) * static_cast<size_t>(k);
    int* d_idx;
    float* d_d2;
    SCAL_TRY(nb_out(c->d_kidx, src, idx, m, &d_idx));
    SCAL_TRY(nb_out(c->d_kd2, src, d2, m, &d_d2));
    const float4* qs;
    int nq;
    SCAL_TRY(nb_queries(c, src, xyzi, n, &qs, &nq));
    SCAL_TRY(nb_run(c, nq, [&](hipStream_t s) -> int {
        nb_list_class(k, [&](auto kc) {
            SCAL_LAUNCH_PROF("k_nb_knn", k_nb_knn<decltype(kc)::value>, dim3(div_up(nq, 64)), dim3(64), 0, s, qs, nq, k, c->r2, c->ix.view(),
                             d_idx, d_d2, c->d_stats.p);
        });
        return SCAL_OK;
    }));
    return nb_download(c, src, m, idx, d_idx, d2, d_d2);
}

extern "C" int scal_nbr_knn(scal_nbr_t* c, const float* xyzi, int n, int k, int* idx, float* d2) {
    return nb_knn(c, "scal_nbr_knn", NB_HOST, xyzi, n, k, idx, d2);
}

extern "C" int scal_nbr_knn_device(scal_nbr_t* c, const float* d_xyzi, int n, int k, int* d_idx, float* d_d2) {
    return nb_knn(c, "scal_nbr_knn_device", NB_DEVICE, d_xyzi, n, k, d_idx, d_d2);
}

extern "C" int scal_nbr_knn_self(scal_nbr_t* c, int k, int* idx, float* d2) {
    return nb_knn(c, "scal_nbr_knn_self", NB_SELF, nullptr, 0, k, idx, d2);
}

// nc and dist are staged in cap entries each, allocated when first asked for.  The position table's allocation and fill are part of
// the launcher, so a call without queries allocates nothing; they come after nb_run has queued the counters' memset, which is
// harmless: the same stream, and a failed allocation leaves only zeroed counters behind.
static int nb_normals(scal_nbr* c, const char* who, NbSource src, const float* xyzi, int n, int k, const double* vp, float* nc, float* dist) {
    SCAL_TRY(nb_check(c, who, src, xyzi, n, 3, k));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    float4* const nc4 = reinterpret_cast<float4*>(nc);
    float4* d_nc;
    float* d_dist;
    SCAL_TRY(nb_out(c->d_nc, src, nc4, static_cast<size_t>(c->cap), &d_nc));
    SCAL_TRY(nb_out(c->d_dist, src, dist, static_cast<size_t>(c->cap), &d_dist));
    const float4* qs;
    int nq;
    SCAL_TRY(nb_queries(c, src, xyzi, n, &qs, &nq));
    SCAL_TRY(nb_run(c, nq, [&](hipStream_t s) -> int {
        if (!c->slot_of.p) SCAL_TRY(c->slot_of.alloc(static_cast<size_t>(c->cfg.max_index_points)));
        if (!c->slots_ok && c->n > 0) {  // from the index's own copy of the records: the caller's are not needed
            SCAL_LAUNCH_PROF("k_nb_slots", k_nb_slots, dim3(div_up(c->n, 256)), dim3(256), 0, s, c->ix.sorted.p, c->n, c->slot_of.p);
            SCAL_HIP(hipGetLastError());
        }
        c->slots_ok = true;
        const int use_vp = vp != nullptr;
        const double vx = vp ? vp[0] : 0.0, vy = vp ? vp[1] : 0.0, vz = vp ? vp[2] : 0.0;
        nb_list_class(k, [&](auto kc) {
            SCAL_LAUNCH_PROF("k_nb_normals", k_nb_normals<decltype(kc)::value>, dim3(div_up(nq, 64)), dim3(64), 0, s, qs, nq, k, c->ix.inv, c->r2,
                             c->ix.hkeys.p, c->ix.hrange.p, c->ix.mask, c->ix.sorted.p, c->slot_of.p, use_vp, vx, vy, vz, d_nc, d_dist, c->d_stats.p);
        });
        return SCAL_OK;
    }));
    return nb_download(c, src, static_cast<size_t>(nq), nc4, d_nc, dist, d_dist);
}

extern "C" int scal_nbr_normals(scal_nbr_t* c, const float* xyzi, int n, int k, const double* viewpoint3, float* nc, float* dist) {
    return nb_normals(c, "scal_nbr_normals", NB_HOST, xyzi, n, k, viewpoint3, nc, dist);
}

extern "C" int scal_nbr_normals_device(scal_nbr_t* c, const float* d_xyzi, int n, int k, const double* viewpoint3, float* d_nc, float* d_dist) {
    return nb_normals(c, "scal_nbr_normals_device", NB_DEVICE, d_xyzi, n, k, viewpoint3, d_nc, d_dist);
}

extern "C" int scal_nbr_normals_self(scal_nbr_t* c, int k, const double* viewpoint3, float* nc, float* dist) {
    return nb_normals(c, "scal_nbr_normals_self", NB_SELF, nullptr, 0, k, viewpoint3, nc, dist);
}

extern "C" int scal_nbr_stats(scal_nbr_t* c, long long* pairs, int* work_items) {
    if (!c || !pairs || !work_items) {
        set_error("scal_nbr_stats: bad argument");
        return SCAL_E_ARG;
    }
    *pairs = c->pairs, *work_items = c->work_items;
    return SCAL_OK;
}
