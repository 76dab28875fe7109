// Loop-closure verification ICP on gfx950.  Replaces the pcl::IterativeClosestPoint call of
// doICPVirtualRelative, /root/reference/src/laserPosegraphOptimization.cpp:518-535 (setMaxCorrespondenceDistance(150),
// setMaximumIterations(100), setTransformationEpsilon(1e-6), setEuclideanFitnessEpsilon(1e-6), setRANSACIterations(0),
// hasConverged(), getFitnessScore()).  The submaps that feed it (:472-494: keyframes moved by ONE root pose, concatenated,
// VoxelGrid 0.4) are scal_mapmerge_* + scal_voxel_*.
//
// Per iteration (PCL icp.hpp computeTransformation, restated in oracle/icp.cpp):
//   k_icp_nn      exact nearest target point of every current source point: 1024 queries x 2048 targets per workgroup (4 queries
//                 per thread), targets staged in LDS and read as wave-wide broadcasts, (f32 squared distance, target index) keys merged across
//                 target chunks with 64-bit atomicMin (= smallest distance, lowest index on ties)
//   k_icp_reduce  correspondences within max distance -> n, sum p, sum q, sum q p^T, sum d^2 in f64: fixed-order workgroup
//                 partials, summed in workgroup order by the last kernel and written to pinned host memory
//   host          Horn's closed form of the rigid least-squares fit (what TransformationEstimationSVD / Eigen::umeyama solve),
//                 PCL's DefaultConvergenceCriteria
//   k_icp_apply   the increment applied to the source cloud in place, f32 as PCL does
// The reference pays a kd-tree query per point and iteration on the CPU.  Here the target is bucketed into a cell grid once per
// alignment and a wave per query searches it ring by ring (k_icp_grid_nn, exact); queries the grid cannot settle within three
// rings fall back to the dense sweep of k_icp_nn, which is also the whole search when scal_icp_set_search(ctx, 0) asks for it.
// The ring search, the dense tile, the 17 sums and the point transform are icp_dev.hpp's, shared with the multiview refine
// (refine.hip), which is held to this file bit for bit; the kernels here say where a cell's points are and which point a thread owns.
//
// scal_icp_align_plane* (an extension, include/scaloam_hip.h and DESIGN.md section 8.14) is the same alignment with a point-to-plane
// metric on the target's normals: the search is untouched, k_icp_plane_reduce (icp_plane_sums: one f64 row per correspondence, 32
// sums) stands in for k_icp_reduce and icp_plane_host_step (LDL^T of the 6x6 normal equations) for icp_host_step.
#include "common.hpp"
#include "device_utils.hpp"
#include "icp_dev.hpp"
#include "icp_host.hpp"
#include <cmath>
#include <cstring>
#include <limits>

namespace scal {

// qlist == nullptr: queries are cur[0 .. n_src); else the *d_nq queries qlist[] (the cell grid's unresolved ones; surplus
// workgroups leave at once)
__global__ void __launch_bounds__(256) k_icp_nn(const float4* __restrict__ cur, int n_src, const float4* __restrict__ tgt, int n_tgt,
                                                unsigned long long* __restrict__ best, const int* __restrict__ qlist,
                                                const int* __restrict__ d_nq) {
    if (qlist) {
        n_src = *d_nq;
        if (static_cast<int>(blockIdx.x) * ICP_QT >= n_src) return;
    }
    icp_dense_tile<false>(
        cur, tgt, n_tgt, blockIdx.y * ICP_TC, blockIdx.x * ICP_QT, [&](int qi) { return qi < n_src ? (qlist ? qlist[qi] : qi) : -1; }, nullptr, nullptr,
        best);
}

// ---- cell grid over the target (built once per alignment) ---------------------------------------------------------------------
// Exact nearest neighbour without the dense sweep: target points bucketed into <= 2^18 cubic cells (counting sort, original
// index kept beside each point); a wave per query examines the cube of cells around the query ring by ring (icp_ring_search has the
// stop rule and the keys).  Queries with nothing close enough within ICP_RINGS rings (far outliers, a poor initial guess) go to the
// dense sweep as a list - the result is the same either way.  The grid is a counting sort of six launches and not the refine's sparse
// index (cell_index.hpp), whose four-pass radix sort is 20 launches and about 0.3 ms at 1.15 M points: the refine pays that once per
// round of about 100 sweeps, an alignment of 1.0-1.5 ms would pay it every time.
constexpr int ICP_NCELL = 1 << 18;
struct IcpGrid {
    float ox, oy, oz, cell, inv;
    int dx, dy, dz;
};

__global__ void __launch_bounds__(256) k_icp_bbox(const float4* __restrict__ tgt, int n, unsigned* __restrict__ mm) {
    float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float4 p = tgt[i];
        if (!(fabsf(p.x) < 3.4e38f && fabsf(p.y) < 3.4e38f && fabsf(p.z) < 3.4e38f)) continue;  // never a neighbour either
        lo[0] = fminf(lo[0], p.x), lo[1] = fminf(lo[1], p.y), lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x), hi[1] = fmaxf(hi[1], p.y), hi[2] = fmaxf(hi[2], p.z);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = wave_min_i(static_cast<int>(float_to_ordered(lo[k]) ^ 0x80000000u));
        const int b = wave_max_i(static_cast<int>(float_to_ordered(hi[k]) ^ 0x80000000u));
        if (lane_id() == 0) {
            atomicMin(&mm[k], static_cast<unsigned>(a) ^ 0x80000000u);
            atomicMax(&mm[3 + k], static_cast<unsigned>(b) ^ 0x80000000u);
        }
    }
}

// one thread: origin, cell width (>= min_cell, grown until the grid fits ICP_NCELL cells), dimensions; resets the box for the next call
__global__ void k_icp_grid_setup(unsigned* __restrict__ mm, IcpGrid* __restrict__ g, float min_cell) {
    float lo[3], ext[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        lo[k] = ordered_to_float(mm[k]);
        const float hi = ordered_to_float(mm[3 + k]);
        ext[k] = hi - lo[k];
        ok = ok && hi >= lo[k];
        mm[k] = 0xffffffffu, mm[3 + k] = 0u;
    }
    IcpGrid r;
    r.ox = lo[0], r.oy = lo[1], r.oz = lo[2], r.cell = min_cell, r.inv = 1.f / min_cell, r.dx = r.dy = r.dz = 0;
    if (ok) {
        float c = min_cell;
        for (int it = 0; it < 200; ++it) {
            const long long dx = static_cast<long long>(ext[0] / c) + 2, dy = static_cast<long long>(ext[1] / c) + 2,
                            dz = static_cast<long long>(ext[2] / c) + 2;
            if (dx * dy * dz <= ICP_NCELL) {
                r.cell = c, r.inv = 1.f / c, r.dx = static_cast<int>(dx), r.dy = static_cast<int>(dy), r.dz = static_cast<int>(dz);
                break;
            }
            c *= 1.1f;
        }
    }
    *g = r;
}

__device__ __forceinline__ int icp_cell_coord(float v, float o, float inv) {
    const float f = floorf((v - o) * inv);
    return static_cast<int>(fminf(fmaxf(f, -1048576.f), 1048576.f));  // NaN -> -2^20: outside every grid
}

__global__ void __launch_bounds__(256) k_icp_cell_count(const float4* __restrict__ tgt, int n, const IcpGrid* __restrict__ gp,
                                                        int* __restrict__ count, int* __restrict__ cell_of) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const IcpGrid g = *gp;
    const float4 p = tgt[i];
    const int x = icp_cell_coord(p.x, g.ox, g.inv), y = icp_cell_coord(p.y, g.oy, g.inv), z = icp_cell_coord(p.z, g.oz, g.inv);
    int cell = -1;  // non-finite points are in no cell: they can never be a nearest neighbour (d < bd fails for NaN)
    if (static_cast<unsigned>(x) < static_cast<unsigned>(g.dx) && static_cast<unsigned>(y) < static_cast<unsigned>(g.dy) &&
        static_cast<unsigned>(z) < static_cast<unsigned>(g.dz)) {
        cell = (z * g.dy + y) * g.dx + x;
        atomicAdd(&count[cell], 1);
    }
    cell_of[i] = cell;
}

// exclusive scan of count[ICP_NCELL] in two launches: workgroup sums, then every workgroup adds the sums in front of it
__global__ void __launch_bounds__(256) k_icp_scan_sums(const int* __restrict__ count, int* __restrict__ bsum) {
    const int4 v = reinterpret_cast<const int4*>(count)[blockIdx.x * 256 + threadIdx.x];
    __shared__ int red[4];
    const int s = wave_sum((v.x + v.y) + (v.z + v.w));
    if (lane_id() == 0) red[wave_id()] = s;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void __launch_bounds__(256) k_icp_scan_apply(int* __restrict__ count, const int* __restrict__ bsum, int* __restrict__ start,
                                                        int* __restrict__ total) {
    __shared__ int smem[17];
    __shared__ int red[4];
    // sum of the workgroup sums in front of this one (gridDim.x = ICP_NCELL / 1024 = 256 = blockDim.x)
    const int mine = static_cast<int>(threadIdx.x) < static_cast<int>(blockIdx.x) ? bsum[threadIdx.x] : 0;
    const int ws = wave_sum(mine);
    if (lane_id() == 0) red[wave_id()] = ws;
    __syncthreads();
    const int base = (red[0] + red[1]) + (red[2] + red[3]);
    int4 v = reinterpret_cast<const int4*>(count)[blockIdx.x * 256 + threadIdx.x];
    int tot;
    const int ex = block_exclusive_scan((v.x + v.y) + (v.z + v.w), smem, &tot) + base;
    int4 o;
    o.x = ex, o.y = ex + v.x, o.z = o.y + v.y, o.w = o.z + v.z;
    reinterpret_cast<int4*>(start)[blockIdx.x * 256 + threadIdx.x] = o;
    reinterpret_cast<int4*>(count)[blockIdx.x * 256 + threadIdx.x] = make_int4(0, 0, 0, 0);  // becomes the fill cursor, zero again after
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) start[ICP_NCELL] = base + tot, *total = base + tot;
}

__global__ void __launch_bounds__(256) k_icp_cell_fill(const float4* __restrict__ tgt, int n, const int* __restrict__ cell_of,
                                                       const int* __restrict__ start, int* __restrict__ cursor, float4* __restrict__ sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int cell = cell_of[i];
    if (cell < 0) return;
    float4 p = tgt[i];
    p.w = __int_as_float(i);
    sorted[start[cell] + atomicAdd(&cursor[cell], 1)] = p;
}

// one wave per query
__global__ void __launch_bounds__(256) k_icp_grid_nn(const float4* __restrict__ cur, int n_src, const IcpGrid* __restrict__ gp,
                                                     const int* __restrict__ start, const float4* __restrict__ sorted,
                                                     unsigned long long* __restrict__ best, int* __restrict__ un_list, int* __restrict__ d_nun) {
    const int qi = blockIdx.x * 4 + wave_id();
    if (qi >= n_src) return;
    const IcpGrid g = *gp;
    const float4 q = cur[qi];
    const int cx = icp_cell_coord(q.x, g.ox, g.inv), cy = icp_cell_coord(q.y, g.oy, g.inv), cz = icp_cell_coord(q.z, g.oz, g.inv);
    unsigned long long bk;
    const bool done = icp_ring_search(
        q, cx, cy, cz, g.cell, sorted,
        [&](int x, int y, int z, int& s0, int& cnt) {
            if (static_cast<unsigned>(x) < static_cast<unsigned>(g.dx) && static_cast<unsigned>(y) < static_cast<unsigned>(g.dy) &&
                static_cast<unsigned>(z) < static_cast<unsigned>(g.dz)) {
                const int cell = (z * g.dy + y) * g.dx + x;
                s0 = start[cell];
                cnt = start[cell + 1] - s0;
            }
        },
        [](int) { return true; }, bk);
    if (lane_id() == 0) {
        if (done)
            best[qi] = bk;
        else
            un_list[atomicAdd(d_nun, 1)] = qi;
    }
}

// partial sums of one workgroup of 256 source points; resets the keys for the next sweep
__global__ void __launch_bounds__(256) k_icp_reduce(const float4* __restrict__ cur, int n_src, const float4* __restrict__ tgt,
                                                    unsigned long long* __restrict__ best, float max2, double* __restrict__ partials,
                                                    int* __restrict__ d_nun) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *d_nun = 0;  // the cell grid's unresolved-query list is consumed by now
    icp_corr_sums(cur, tgt, best, max2, i, i < n_src, partials + static_cast<size_t>(blockIdx.x) * ICP_NSUM);
}

// the same for the 32 point-to-plane sums (scal_icp_align_plane); nc: the target's normals
__global__ void __launch_bounds__(256) k_icp_plane_reduce(const float4* __restrict__ cur, int n_src, const float4* __restrict__ tgt,
                                                          const float4* __restrict__ nc, unsigned long long* __restrict__ best, float max2,
                                                          double* __restrict__ partials, int* __restrict__ d_nun) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *d_nun = 0;
    icp_plane_sums(cur, tgt, nc, best, max2, i, i < n_src, partials + static_cast<size_t>(blockIdx.x) * ICP_PLANE_NSUM);
}

// sums the workgroup partials (NS to a workgroup) in workgroup order and hands them to the host (pinned, device-visible memory)
template <int NS>
__global__ void __launch_bounds__(64) k_icp_final(const double* __restrict__ partials, int nb, double* __restrict__ host_out) {
    if (threadIdx.x < NS) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += partials[b * NS + threadIdx.x];
        host_out[threadIdx.x] = s;
    }
}

struct Mat34f {
    float m[12];
};
// in and out may be the same array (the working copy moved in place): neither is __restrict__
__global__ void __launch_bounds__(256) k_icp_apply(const float4* in, float4* out, int n, Mat34f T) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = icp_transform(T.m, in[i]);
}

__global__ void k_icp_fill(unsigned long long* __restrict__ best, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) best[i] = ~0ull;
}

}  // namespace scal

using namespace scal;

struct scal_icp {
    scal_icp_config cfg;
    LaneStream stream;  // released by `delete c`, after scal_icp_destroy has synchronised it
    DevBuf<float4> src, cur, tgt;
    const float4* tgt_cur = nullptr;  // the target of the alignment in flight: tgt, or the caller's device cloud
    DevBuf<unsigned long long> best;
    DevBuf<double> partials;
    PinBuf<double> h_sums;
    // cell grid over the target
    int search = 1;  // 0: dense sweep, 1: cell grid with the dense sweep for unresolved queries
    bool grid_built = false;
    DevBuf<IcpGrid> grid;
    DevBuf<unsigned> mm;
    DevBuf<int> count, start, bsum, cell_of, un_list, d_nun;
    DevBuf<float4> sorted;
    // point-to-plane: allocated by the first scal_icp_align_plane* call (the normals staging by the first with host arrays)
    DevBuf<float4> nc;
    DevBuf<double> plane_partials;
    PinBuf<double> h_plane;
};

extern "C" int scal_icp_create(const scal_icp_config* cfg, scal_icp_t** out) { return icp_create_on_lane(cfg, 0, out); }

int scal::icp_create_on_lane(const scal_icp_config* cfg, int lane, scal_icp_t** out) {
    if (!cfg || !out || cfg->max_source <= 0 || cfg->max_target <= 0 || cfg->max_iterations <= 0 || !(cfg->max_corr_dist > 0)) {
        set_error("scal_icp_create: bad argument");
        return SCAL_E_ARG;
    }
    *out = nullptr;
    SCAL_TRY(select_device(cfg->device));
    auto* c = new scal_icp();
    c->cfg = *cfg;
    int rc = SCAL_OK;
    auto A = [&](int r) { if (rc == SCAL_OK) rc = r; };
    A(c->src.alloc(cfg->max_source)); A(c->cur.alloc(cfg->max_source)); A(c->tgt.alloc(cfg->max_target));
    A(c->best.alloc(cfg->max_source));
    A(c->partials.alloc(static_cast<size_t>(ICP_NSUM) * (div_up(cfg->max_source, 256) + 1)));
    A(c->h_sums.alloc(ICP_NSUM));
    A(c->grid.alloc(1)); A(c->mm.alloc(6)); A(c->count.alloc(ICP_NCELL)); A(c->start.alloc(ICP_NCELL + 4)); A(c->bsum.alloc(256));
    A(c->cell_of.alloc(cfg->max_target)); A(c->sorted.alloc(cfg->max_target)); A(c->un_list.alloc(cfg->max_source)); A(c->d_nun.alloc(2));
    if (rc == SCAL_OK) rc = c->stream.acquire(cfg->device, lane);
    if (rc == SCAL_OK) {  // initialised on the context's own stream (the legacy null stream is not ordered against it)
        const unsigned init[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
        if (hipMemcpyAsync(c->mm.p, init, sizeof init, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemsetAsync(c->d_nun.p, 0, 2 * sizeof(int), c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            rc = SCAL_E_HIP;
    }
    if (rc != SCAL_OK) {
        delete c;
        return rc;
    }
    *out = c;
    return SCAL_OK;
}

extern "C" int scal_icp_set_search(scal_icp_t* c, int mode) {
    if (!c || (mode != 0 && mode != 1)) {
        set_error("scal_icp_set_search: bad argument");
        return SCAL_E_ARG;
    }
    c->search = mode;
    return SCAL_OK;
}

extern "C" void scal_icp_destroy(scal_icp_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

// one correspondence sweep of `pts` against the target: sums -> c->h_sums (waits); nc != nullptr: the target's normals, the 32
// point-to-plane sums -> c->h_plane instead
static int icp_sweep(scal_icp* c, const float4* pts, int n_src, int n_tgt, float max2, const float4* nc = nullptr) {
    hipStream_t s = c->stream;
    const int nb = div_up(n_src, 256);
    const int* no_list = nullptr;
    if (c->grid_built) {
        SCAL_LAUNCH_PROF("k_icp_grid_nn", k_icp_grid_nn, dim3(div_up(n_src, 4)), dim3(256), 0, s, pts, n_src, c->grid.p, c->start.p, c->sorted.p,
                         c->best.p, c->un_list.p, c->d_nun.p);
        SCAL_LAUNCH_PROF("k_icp_nn", k_icp_nn, dim3(div_up(n_src, ICP_QT), div_up(n_tgt, ICP_TC)), dim3(256), 0, s, pts, n_src, c->tgt_cur, n_tgt,
                         c->best.p, c->un_list.p, c->d_nun.p);
    } else {
        SCAL_LAUNCH_PROF("k_icp_nn", k_icp_nn, dim3(div_up(n_src, ICP_QT), div_up(n_tgt, ICP_TC)), dim3(256), 0, s, pts, n_src, c->tgt_cur, n_tgt,
                         c->best.p, no_list, no_list);
    }
    if (nc) {
        SCAL_LAUNCH_PROF("k_icp_plane_reduce", k_icp_plane_reduce, dim3(nb), dim3(256), 0, s, pts, n_src, c->tgt_cur, nc, c->best.p, max2,
                         c->plane_partials.p, c->d_nun.p);
        hipLaunchKernelGGL(k_icp_final<ICP_PLANE_NSUM>, dim3(1), dim3(64), 0, s, c->plane_partials.p, nb, c->h_plane.p);
    } else {
        hipLaunchKernelGGL(k_icp_reduce, dim3(nb), dim3(256), 0, s, pts, n_src, c->tgt_cur, c->best.p, max2, c->partials.p, c->d_nun.p);
        hipLaunchKernelGGL(k_icp_final<ICP_NSUM>, dim3(1), dim3(64), 0, s, c->partials.p, nb, c->h_sums.p);
    }
    SCAL_HIP(hipGetLastError());
    SCAL_HIP(hipStreamSynchronize(s));
    return SCAL_OK;
}

// what only the point-to-plane calls need, allocated by the first of them and released with the context
static int icp_plane_prepare(scal_icp* c, bool staging) {
    if (!c->plane_partials.p) SCAL_TRY(c->plane_partials.alloc(static_cast<size_t>(ICP_PLANE_NSUM) * (div_up(c->cfg.max_source, 256) + 1)));
    if (!c->h_plane.p) SCAL_TRY(c->h_plane.alloc(ICP_PLANE_NSUM));
    if (staging && !c->nc.p) SCAL_TRY(c->nc.alloc(c->cfg.max_target));
    return SCAL_OK;
}

// clouds in host memory (on_device = false: staged into the context) or already in HBM (the target is then used in place).
// guess != nullptr: pcl::Registration::align(output, guess) - the working copy of the source is moved by the guess once and the
// accumulated transformation starts from it; nullptr is align(output), today's path launch for launch.
// pres != nullptr: point-to-plane on the target's normals tgt_nc (where the clouds are), the result in *pres and res unused; the
// two metrics differ in the reduction of a sweep, in the host's increment and in the final sweep's cap, and in nothing else.
static int icp_align(scal_icp* c, const float* src_xyzi, int n_src, const float* tgt_xyzi, int n_tgt, bool on_device, const float* guess,
                     scal_icp_result* res, const float* tgt_nc = nullptr, scal_icp_plane_result* pres = nullptr) {
    const bool plane = pres != nullptr;
    if (!c || !(res || pres) || n_src < 0 || n_tgt < 0 || (n_src && !src_xyzi) || (n_tgt && !tgt_xyzi) || (plane && n_tgt && !tgt_nc)) {
        set_error("%s: bad argument", plane ? "scal_icp_align_plane" : "scal_icp_align");
        return SCAL_E_ARG;
    }
    if (n_src > c->cfg.max_source || n_tgt > c->cfg.max_target) {
        set_error("%s: cloud larger than the context capacity (source %d, target %d)", plane ? "scal_icp_align_plane" : "scal_icp_align",
                  c->cfg.max_source, c->cfg.max_target);
        return SCAL_E_TOO_MANY;
    }
    float F[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (plane) {
        std::memset(pres, 0, sizeof *pres);
        for (int k = 0; k < 16; ++k) pres->T[k] = F[k];
        pres->fitness = pres->plane_fitness = std::numeric_limits<double>::max();
    } else {
        std::memset(res, 0, sizeof *res);
        for (int k = 0; k < 16; ++k) res->T[k] = F[k];
        res->fitness = std::numeric_limits<double>::max();
    }
    if (n_src == 0 || n_tgt == 0) {  // pcl::Registration::align refuses empty clouds: not converged
        (plane ? pres->state : res->state) = 5;
        return SCAL_OK;
    }
    SCAL_HIP(hipSetDevice(c->cfg.device));
    if (plane) SCAL_TRY(icp_plane_prepare(c, !on_device));
    hipStream_t s = c->stream;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    SCAL_HIP(hipMemcpyAsync(c->src.p, src_xyzi, sizeof(float) * 4 * n_src, kind, s));
    SCAL_HIP(hipMemcpyAsync(c->cur.p, src_xyzi, sizeof(float) * 4 * n_src, kind, s));
    const float4* tgt = c->tgt.p;
    const float4* nc = nullptr;
    if (on_device)
        tgt = reinterpret_cast<const float4*>(tgt_xyzi);
    else
        SCAL_HIP(hipMemcpyAsync(c->tgt.p, tgt_xyzi, sizeof(float) * 4 * n_tgt, hipMemcpyHostToDevice, s));
    if (plane) {
        nc = on_device ? reinterpret_cast<const float4*>(tgt_nc) : c->nc.p;
        if (!on_device) SCAL_HIP(hipMemcpyAsync(c->nc.p, tgt_nc, sizeof(float) * 4 * n_tgt, hipMemcpyHostToDevice, s));
    }
    c->tgt_cur = tgt;
    if (guess) {
        Mat34f G;
        std::memcpy(G.m, guess, sizeof G.m);
        hipLaunchKernelGGL(k_icp_apply, dim3(div_up(n_src, 256)), dim3(256), 0, s, c->cur.p, c->cur.p, n_src, G);
    }
    hipLaunchKernelGGL(k_icp_fill, dim3(div_up(n_src, 256)), dim3(256), 0, s, c->best.p, n_src);
    c->grid_built = false;
    if (c->search == 1 && n_tgt >= 4 * ICP_TC) {  // small targets: the dense sweep is a handful of workgroups anyway
        SCAL_HIP(hipMemsetAsync(c->count.p, 0, sizeof(int) * ICP_NCELL, s));
        hipLaunchKernelGGL(k_icp_bbox, dim3(std::min(div_up(n_tgt, 256), 1024)), dim3(256), 0, s, tgt, n_tgt, c->mm.p);
        hipLaunchKernelGGL(k_icp_grid_setup, dim3(1), dim3(1), 0, s, c->mm.p, c->grid.p, 1.0f);
        hipLaunchKernelGGL(k_icp_cell_count, dim3(div_up(n_tgt, 256)), dim3(256), 0, s, tgt, n_tgt, c->grid.p, c->count.p, c->cell_of.p);
        hipLaunchKernelGGL(k_icp_scan_sums, dim3(ICP_NCELL / 1024), dim3(256), 0, s, c->count.p, c->bsum.p);
        hipLaunchKernelGGL(k_icp_scan_apply, dim3(ICP_NCELL / 1024), dim3(256), 0, s, c->count.p, c->bsum.p, c->start.p, c->d_nun.p + 1);
        SCAL_LAUNCH_PROF("k_icp_cell_fill", k_icp_cell_fill, dim3(div_up(n_tgt, 256)), dim3(256), 0, s, tgt, n_tgt, c->cell_of.p, c->start.p,
                         c->count.p, c->sorted.p);
        SCAL_HIP(hipGetLastError());
        c->grid_built = true;
    }
    const float max2 = static_cast<float>(c->cfg.max_corr_dist * c->cfg.max_corr_dist);
    const double te = c->cfg.transformation_epsilon, fe = c->cfg.fitness_epsilon;
    IcpIterState is;  // the iteration itself is icp_host.hpp's, shared with the multiview refine
    if (guess) std::memcpy(is.F, guess, sizeof is.F);
    for (;;) {
        SCAL_TRY(icp_sweep(c, c->cur.p, n_src, n_tgt, max2, nc));
        float T[16];
        int step;
        if (plane) {
            if (is.it == 0) std::memcpy(pres->first_eq, c->h_plane.p + 1, sizeof pres->first_eq);
            step = icp_plane_host_step(is, c->h_plane.p, c->cfg.max_iterations, te, fe, T);
            pres->n_correspondences = is.n_corr;
        } else {
            step = icp_host_step(is, c->h_sums.p, c->cfg.max_iterations, te, fe, T);
            res->n_correspondences = is.n_corr;
        }
        if (step == ICP_STEP_STOP) break;
        Mat34f M;
        std::memcpy(M.m, T, sizeof M.m);
        hipLaunchKernelGGL(k_icp_apply, dim3(div_up(n_src, 256)), dim3(256), 0, s, c->cur.p, c->cur.p, n_src, M);
        if (step == ICP_STEP_CONVERGED) break;
    }
    std::memcpy(F, is.F, sizeof F);
    const int it = is.it, st = is.st;
    const bool converged = is.converged;
    // getFitnessScore(): the original source moved by the final transform, no distance cap (point-to-plane: the cap stays for the
    // rows, and the uncapped pair of sums rides along)
    Mat34f M;
    std::memcpy(M.m, F, sizeof M.m);
    hipLaunchKernelGGL(k_icp_apply, dim3(div_up(n_src, 256)), dim3(256), 0, s, c->src.p, c->cur.p, n_src, M);
    SCAL_TRY(icp_sweep(c, c->cur.p, n_src, n_tgt, plane ? max2 : 3.4e38f, nc));
    if (plane) {
        const double* h = c->h_plane.p;
        pres->converged = converged ? 1 : 0;
        pres->iterations = it;
        pres->state = st;
        pres->fitness = h[30] > 0 ? h[31] / h[30] : std::numeric_limits<double>::max();
        pres->plane_fitness = h[0] > 0 ? h[28] / h[0] : std::numeric_limits<double>::max();
        std::memcpy(pres->normal_eq, h + 1, sizeof pres->normal_eq);
        for (int k = 0; k < 16; ++k) pres->T[k] = F[k];
        return SCAL_OK;
    }
    res->converged = converged ? 1 : 0;
    res->iterations = it;
    res->state = st;
    res->fitness = c->h_sums.p[0] > 0 ? c->h_sums.p[16] / c->h_sums.p[0] : std::numeric_limits<double>::max();
    for (int k = 0; k < 16; ++k) res->T[k] = F[k];
    return SCAL_OK;
}

extern "C" int scal_icp_align(scal_icp_t* c, const float* src_xyzi, int n_src, const float* tgt_xyzi, int n_tgt, scal_icp_result* res) {
    return icp_align(c, src_xyzi, n_src, tgt_xyzi, n_tgt, false, nullptr, res);
}

extern "C" int scal_icp_align_device(scal_icp_t* c, const float* d_src_xyzi, int n_src, const float* d_tgt_xyzi, int n_tgt, scal_icp_result* res) {
    return icp_align(c, d_src_xyzi, n_src, d_tgt_xyzi, n_tgt, true, nullptr, res);
}

// the guess as icp_align takes it: nullptr for none or the identity (both are align(output)), the 16 f32 values otherwise
static int icp_check_guess(const float guess[16], const float** use) {
    *use = nullptr;
    if (!guess) return SCAL_OK;
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(guess[k])) {
            set_error("scal_icp_align_guess: the guess is not finite");
            return SCAL_E_ARG;
        }
    if (!(guess[12] == 0.f && guess[13] == 0.f && guess[14] == 0.f && guess[15] == 1.f)) {
        set_error("scal_icp_align_guess: the last row of the guess must be 0 0 0 1");
        return SCAL_E_ARG;
    }
    bool identity = true;
    for (int k = 0; k < 12; ++k) identity = identity && guess[k] == (k % 5 == 0 ? 1.f : 0.f);
    if (!identity) *use = guess;
    return SCAL_OK;
}

extern "C" int scal_icp_align_guess(scal_icp_t* c, const float* src_xyzi, int n_src, const float* tgt_xyzi, int n_tgt, const float guess[16],
                                    scal_icp_result* res) {
    const float* g;
    SCAL_TRY(icp_check_guess(guess, &g));
    return icp_align(c, src_xyzi, n_src, tgt_xyzi, n_tgt, false, g, res);
}

extern "C" int scal_icp_align_guess_device(scal_icp_t* c, const float* d_src_xyzi, int n_src, const float* d_tgt_xyzi, int n_tgt,
                                           const float guess[16], scal_icp_result* res) {
    const float* g;
    SCAL_TRY(icp_check_guess(guess, &g));
    return icp_align(c, d_src_xyzi, n_src, d_tgt_xyzi, n_tgt, true, g, res);
}

extern "C" int scal_icp_align_plane(scal_icp_t* c, const float* src_xyzi, int n_src, const float* tgt_xyzi, const float* tgt_nc, int n_tgt,
                                    const float guess[16], scal_icp_plane_result* res) {
    const float* g;
    SCAL_TRY(icp_check_guess(guess, &g));
    if (!res) {
        set_error("scal_icp_align_plane: bad argument");
        return SCAL_E_ARG;
    }
    return icp_align(c, src_xyzi, n_src, tgt_xyzi, n_tgt, false, g, nullptr, tgt_nc, res);
}

extern "C" int scal_icp_align_plane_device(scal_icp_t* c, const float* d_src_xyzi, int n_src, const float* d_tgt_xyzi, const float* d_tgt_nc,
                                           int n_tgt, const float guess[16], scal_icp_plane_result* res) {
    const float* g;
    SCAL_TRY(icp_check_guess(guess, &g));
    if (!res) {
        set_error("scal_icp_align_plane: bad argument");
        return SCAL_E_ARG;
    }
    return icp_align(c, d_src_xyzi, n_src, d_tgt_xyzi, n_tgt, true, g, nullptr, d_tgt_nc, res);
}
