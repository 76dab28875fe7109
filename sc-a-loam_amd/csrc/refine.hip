// Multiview refine on gfx950 (BASELINE.json config #5, "global ICP refine"; include/scaloam_hip.h has the semantics): all K keyframes
// of a session aligned at once by point-to-point ICP, each against the points of all the others, in Jacobi rounds.  An extension -
// the reference has no counterpart; the single alignment it is held to is scal_icp_align (icp.hip), bit for bit.
//
// Per round:
//   k_rf_count / k_rf_write   every frame moved by its pose with the map merge's own passes (mapmerge_dev.hpp) -> G, the round's
//                             target, frames in order, every point with its frame beside it; the sources start as a copy of G
//   SparseCells::build        sparse neighbour index over G (cell_index.hpp, the index nbr.hip uses as well) with a 1 m cell: sorted
//                             by cell (stable, so a cell's points stay in index order), the cells' [start, end) ranges behind a hash
//                             table in HBM; the index launch is timed as k_rf_index.  The cell width does not depend on the map's
//                             extent, as icp.hip's dense 2^18-cell grid does.
// Per iteration, ONE launch chain for all frames still iterating and one host synchronisation:
//   k_rf_apply    last iteration's increments, one 3x4 matrix per frame (icp_transform)
//   k_rf_grid_nn  a wave per source point: icp_ring_search with the cells looked up through the index (CellView::find); a candidate of
//                 the query's own frame is dropped before the key is formed
//   k_rf_dense    only when max_corr_dist reaches beyond the last ring: the unsettled queries as a list against all of G, a fixed
//                 number of workgroups striding over (query tile, target chunk) pairs (icp_dense_tile) - none when the list is empty
//   k_rf_reduce   icp_corr_sums per workgroup of 256 source points COUNTED FROM THE FRAME'S FIRST POINT, then
//   k_rf_final    the frame's workgroup partials in workgroup order -> pinned [K][17]: the additions of k_icp_reduce / k_icp_final on
//                 that frame alone, in their order
//   host          icp_host_step (icp_host.hpp, shared with icp.hip) per frame; K 3x4 increments and the active mask go back in one copy
// scal_refine_run_plane* (an extension) is the same round with the point-to-plane metric of
// scal_icp_align_plane on the frames' own local normals: k_rf_write_nc writes the rotated normals beside the moved points, the search
// is untouched, k_rf_plane_reduce (icp_plane_sums, 32 sums) stands in for k_rf_reduce, k_rf_final<32> for k_rf_final<17> and
// icp_plane_host_step for icp_host_step.
// Frames that have finished cost an early return per workgroup.  The search, the sums and the transform are icp_dev.hpp's, the same
// code icp.hip runs: what is written here is where a cell's points are, which candidates count and which point a thread owns.
#include "common.hpp"
#include "cell_index.hpp"
#include "device_utils.hpp"
#include "icp_dev.hpp"
#include "icp_host.hpp"
#include "mapmerge_dev.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

namespace scal {

constexpr float RF_CELL = 1.0f;    // cell width in metres; cell coordinate = floor(v), exact in f32
constexpr int RF_DENSE_WG = 2048;  // workgroups of the dense sweep
// The index clamps cell coordinates beyond +-65 km in x and y and +-8 km in z.  Clamping is monotone, so a cell that the ring
// search has not examined is still at least k cells away from the query along some axis and the stop rule holds out there too.
// A point is in a cell when |v| < 3.4e38 on every axis: any other can never be a nearest neighbour (d < 3.4e38 fails).
constexpr float RF_FINITE = 3.4e38f;

struct RfBlock {
    int first, end, frame;  // 256 source points of one frame: [first, min(first + 256, end)) of G
};
struct RfCtrl {  // per frame, host -> device once per iteration
    int active;    // the frame takes part in this iteration's sweep
    float m[12];   // increment to apply first (active frames, from the second iteration on)
};

__global__ void __launch_bounds__(256) k_rf_count(const float4* __restrict__ in, const MMBlock* __restrict__ blocks, double thres,
                                                  int* __restrict__ blkcnt) {
    mm_count_body(in, blocks, thres, blkcnt);
}
__global__ void __launch_bounds__(256) k_rf_write(const float4* __restrict__ in, const MMBlock* __restrict__ blocks, const double* __restrict__ poses,
                                                  double thres, const int* __restrict__ blkoff, long long cap, float4* __restrict__ out,
                                                  int* __restrict__ frame_of) {
    mm_write_body<true>(in, blocks, poses, thres, blkoff, 0, cap, out, frame_of);
}

// scal_refine_run_plane*: the normals of the points k_rf_write keeps, rotated by the frame's pose, to the positions k_rf_write gives
// the points - the same keep rule on the same records, the same ballot ranks, so out[o] is the normal of g[o].  A kernel of its own:
// mm_write_body stays what the map merge compiles.  Rows of the pose's rotation in f64, one rounding per operation, no translation.
__global__ void __launch_bounds__(256) k_rf_write_nc(const float4* __restrict__ in, const float4* __restrict__ nc, const MMBlock* __restrict__ blocks,
                                                     const double* __restrict__ poses, double thres, const int* __restrict__ blkoff, long long cap,
                                                     float4* __restrict__ out) {
    __shared__ int s_cnt[MM_ITEMS][4];
    const MMBlock b = blocks[blockIdx.x];
    const int w = wave_id();
    bool keep[MM_ITEMS];
    int rank[MM_ITEMS];
#pragma unroll
    for (int j = 0; j < MM_ITEMS; ++j) {
        const int i = b.first + j * 256 + threadIdx.x;
        keep[j] = i < b.end && mm_keep(in[i], thres);
        const uint64_t m = __ballot(keep[j]);
        rank[j] = __popcll(m & lanemask_lt());
        if (lane_id() == 0) s_cnt[j][w] = __popcll(m);
    }
    __syncthreads();
    const double* T = poses + 12 * b.frame;
    int before = 0;  // kept points of the workgroup in front of (j, wave w)
#pragma unroll
    for (int j = 0; j < MM_ITEMS; ++j) {
        int mine = before;
        for (int q = 0; q < w; ++q) mine += s_cnt[j][q];
        before += s_cnt[j][0] + s_cnt[j][1] + s_cnt[j][2] + s_cnt[j][3];
        if (!keep[j]) continue;
        const long long o = blkoff[blockIdx.x] + mine + rank[j];
        if (o >= cap) continue;
        const float4 n = nc[b.first + j * 256 + threadIdx.x];
        const double x = n.x, y = n.y, z = n.z;
        float4 g;
        g.x = static_cast<float>((T[0] * x + T[1] * y) + T[2] * z);
        g.y = static_cast<float>((T[4] * x + T[5] * y) + T[6] * z);
        g.z = static_cast<float>((T[8] * x + T[9] * y) + T[10] * z);
        g.w = n.w;
        out[o] = g;
    }
}

// a frame's 3x4 matrix applied to its points: last iteration's increment to the sources in place (in == out), or the whole
// transformation to the moved frame itself for the fitness sweep (in = G); neither pointer is __restrict__
__global__ void __launch_bounds__(256) k_rf_apply(const float4* in, float4* out, const RfBlock* __restrict__ blocks, const RfCtrl* __restrict__ ctrl) {
    const RfBlock b = blocks[blockIdx.x];
    if (!ctrl[b.frame].active) return;
    const int i = b.first + threadIdx.x;
    if (i >= b.end) return;
    out[i] = icp_transform(ctrl[b.frame].m, in[i]);
}

// one wave per query: icp_dev.hpp's ring search with the cell looked up through the index and the query's own frame left out.
// The index comes as loose arguments and the view is put together in here: with a CellView as the argument the kernel ran 1.2 %
// slower, outside what two identical builds show (profiles/cell_index_ab.txt); this way its code is the one from before.
__global__ void __launch_bounds__(256) k_rf_grid_nn(const float4* __restrict__ cur, int n, const int* __restrict__ frame_of, const int* __restrict__ goff,
                                                    const RfCtrl* __restrict__ ctrl, const unsigned long long* __restrict__ hkeys,
                                                    const int2* __restrict__ hrange, unsigned mask, const float4* __restrict__ sorted,
                                                    unsigned long long* __restrict__ best, int* __restrict__ un_list, int* __restrict__ d_nun,
                                                    int keep_unresolved) {
    const int qi = blockIdx.x * 4 + wave_id();
    if (qi >= n) return;
    const int frame = frame_of[qi];
    if (!ctrl[frame].active) return;
    const int own0 = goff[frame], own_n = goff[frame + 1] - own0;  // the frame's points are one index range of G
    const float4 q = cur[qi];
    const CellView ix{hkeys, hrange, sorted, mask, 1.0f / RF_CELL};
    unsigned long long bk;
    const bool done = icp_ring_search(
        q, ix.cx(q.x), ix.cx(q.y), ix.cz(q.z), RF_CELL, ix.sorted,
        [&](int x, int y, int z, int& s0, int& cnt) {
            int2 r;
            if (ix.find(x, y, z, r)) s0 = r.x, cnt = r.y - r.x;
        },
        [&](int ti) { return static_cast<unsigned>(ti - own0) >= static_cast<unsigned>(own_n); }, bk);
    if (lane_id() == 0) {
        if (done)
            best[qi] = bk;
        else if (keep_unresolved)  // else: nothing within the last ring's bound, and max_corr_dist does not reach beyond it
            un_list[atomicAdd(d_nun, 1)] = qi;
    }
}

// exact nearest neighbour of the *d_nq listed queries among all of G but their own frame; the workgroups stride over the
// (query tile, target chunk) pairs, so an empty list costs RF_DENSE_WG early returns
__global__ void __launch_bounds__(256) k_rf_dense(const float4* __restrict__ cur, const float4* __restrict__ tgt, int n_tgt, const int* __restrict__ frame_of,
                                                  const int* __restrict__ goff, unsigned long long* __restrict__ best, const int* __restrict__ qlist,
                                                  const int* __restrict__ d_nq) {
    const int nq = *d_nq;
    if (nq == 0) return;
    const long long n_qt = (nq + ICP_QT - 1) / ICP_QT, n_tc = (n_tgt + ICP_TC - 1) / ICP_TC;
    for (long long w = blockIdx.x; w < n_qt * n_tc; w += gridDim.x) {
        const int q0 = static_cast<int>(w / n_tc) * ICP_QT, t0 = static_cast<int>(w % n_tc) * ICP_TC;
        __syncthreads();  // the previous pair's chunk has been read
        icp_dense_tile<true>(cur, tgt, n_tgt, t0, q0, [&](int qi) { return qi < nq ? qlist[qi] : -1; }, frame_of, goff, best);
    }
}

// partial sums of one workgroup of 256 source points of one frame; resets the keys for the next sweep
__global__ void __launch_bounds__(256) k_rf_reduce(const float4* __restrict__ cur, const float4* __restrict__ tgt, const RfBlock* __restrict__ blocks,
                                                   const RfCtrl* __restrict__ ctrl, unsigned long long* __restrict__ best, float max2,
                                                   double* __restrict__ partials) {
    const RfBlock b = blocks[blockIdx.x];
    if (!ctrl[b.frame].active) return;
    const int i = b.first + threadIdx.x;
    icp_corr_sums(cur, tgt, best, max2, i, i < b.end, partials + static_cast<size_t>(blockIdx.x) * ICP_NSUM);
}

// the same for the 32 point-to-plane sums (scal_refine_run_plane); nc: the moved normals of all of G
__global__ void __launch_bounds__(256) k_rf_plane_reduce(const float4* __restrict__ cur, const float4* __restrict__ tgt, const float4* __restrict__ nc,
                                                         const RfBlock* __restrict__ blocks, const RfCtrl* __restrict__ ctrl,
                                                         unsigned long long* __restrict__ best, float max2, double* __restrict__ partials) {
    const RfBlock b = blocks[blockIdx.x];
    if (!ctrl[b.frame].active) return;
    const int i = b.first + threadIdx.x;
    icp_plane_sums(cur, tgt, nc, best, max2, i, i < b.end, partials + static_cast<size_t>(blockIdx.x) * ICP_PLANE_NSUM);
}

// one workgroup per frame: its workgroup partials (NS to a workgroup) in workgroup order -> host_out[frame][NS] (pinned, device-visible memory)
template <int NS>
__global__ void __launch_bounds__(64) k_rf_final(const double* __restrict__ partials, const int* __restrict__ fb0, const RfCtrl* __restrict__ ctrl,
                                                 double* __restrict__ host_out, int* __restrict__ d_nun) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *d_nun = 0;  // the unresolved-query list is consumed by now
    const int f = blockIdx.x;
    if (!ctrl[f].active) return;
    if (threadIdx.x < NS) {
        double s = 0.0;
        for (int b = fb0[f]; b < fb0[f + 1]; ++b) s += partials[static_cast<size_t>(b) * NS + threadIdx.x];
        host_out[f * NS + threadIdx.x] = s;
    }
}

}  // namespace scal

using namespace scal;

struct scal_refine {
    scal_refine_config cfg;
    LaneStream stream;  // released by `delete c`, after scal_refine_destroy has synchronised it
    int nb_mm_cap = 0, nb_cap = 0;  // workgroups of the move (<= max_points / 1024 + max_frames) and of a sweep (<= max_points / 256 + max_frames)
    SparseCells ix;  // the round's neighbour index over G
    DevBuf<float4> loc, g, cur;  // loc: host records staged in (scal_refine_run), allocated on first use
    DevBuf<int> frame_of, un_list, d_nun;  // d_nun: the unresolved count
    DevBuf<unsigned long long> best;
    DevBuf<MMBlock> mm_blocks;
    DevBuf<int> blk;       // kept points per move workgroup, then their exclusive prefix
    DevBuf<double> poses, partials;
    DevBuf<RfBlock> blocks;
    DevBuf<int> goff, fb0;
    DevBuf<RfCtrl> ctrl;
    PinBuf<MMBlock> h_mm_blocks;
    PinBuf<int> h_blk, h_goff, h_fb0;
    PinBuf<double> h_poses, h_sums;
    PinBuf<RfBlock> h_blocks;
    PinBuf<RfCtrl> h_ctrl;
    // point-to-plane: allocated by the first scal_refine_run_plane* call (the normals staging by the first with host arrays)
    DevBuf<float4> nloc, gn;  // the input normals staged in; the moved normals of G
    DevBuf<double> plane_partials;
    PinBuf<double> h_plane;
};

extern "C" int scal_refine_create(const scal_refine_config* cfg, scal_refine_t** out) { return refine_create_on_lane(cfg, 0, out); }

int scal::refine_create_on_lane(const scal_refine_config* cfg, int lane, scal_refine_t** out) {
    if (!cfg || !out || cfg->max_frames <= 0 || cfg->max_points <= 0 || cfg->max_iterations <= 0 || !(cfg->max_corr_dist > 0) ||
        !(cfg->fitness_gate == cfg->fitness_gate) || cfg->max_points > (1 << 30)) {
        set_error("scal_refine_create: bad argument");
        return SCAL_E_ARG;
    }
    *out = nullptr;
    SCAL_TRY(select_device(cfg->device));
    auto* c = new scal_refine();
    c->cfg = *cfg;
    const size_t np = static_cast<size_t>(cfg->max_points), nf = static_cast<size_t>(cfg->max_frames);
    c->nb_mm_cap = static_cast<int>(np / MM_TILE + nf);
    c->nb_cap = static_cast<int>(np / 256 + nf);
    c->ix.set_names(nullptr, "k_rf_index");
    int rc = SCAL_OK;
    auto A = [&](int r) { if (rc == SCAL_OK) rc = r; };
    A(c->g.alloc(np)); A(c->cur.alloc(np)); A(c->frame_of.alloc(np)); A(c->un_list.alloc(np)); A(c->d_nun.alloc(1));
    A(c->best.alloc(np)); A(c->ix.init(cfg->max_points, cfg->max_points));
    A(c->mm_blocks.alloc(c->nb_mm_cap)); A(c->h_mm_blocks.alloc(c->nb_mm_cap)); A(c->blk.alloc(c->nb_mm_cap)); A(c->h_blk.alloc(c->nb_mm_cap));
    A(c->poses.alloc(12 * nf)); A(c->h_poses.alloc(12 * nf)); A(c->partials.alloc(static_cast<size_t>(ICP_NSUM) * c->nb_cap));
    A(c->blocks.alloc(c->nb_cap)); A(c->h_blocks.alloc(c->nb_cap));
    A(c->goff.alloc(nf + 1)); A(c->h_goff.alloc(nf + 1)); A(c->fb0.alloc(nf + 1)); A(c->h_fb0.alloc(nf + 1));
    A(c->ctrl.alloc(nf)); A(c->h_ctrl.alloc(nf)); A(c->h_sums.alloc(ICP_NSUM * nf));
    if (rc == SCAL_OK) rc = c->stream.acquire(cfg->device, lane);
    if (rc == SCAL_OK && (hipMemsetAsync(c->d_nun.p, 0, sizeof(int), c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)) rc = SCAL_E_HIP;
    if (rc != SCAL_OK) {
        delete c;
        return rc;
    }
    *out = c;
    return SCAL_OK;
}

extern "C" void scal_refine_destroy(scal_refine_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

static int refine_check_args(scal_refine* c, const float* xyzi, const int* offsets, int n_frames, double* poses12, double near_thres, int rounds,
                             const void* res, int* rounds_run) {
    if (!c || !offsets || !poses12 || !res || !rounds_run || n_frames < 0 || rounds < 1 || !(near_thres == near_thres) || std::isinf(near_thres)) {
        set_error("scal_refine_run: bad argument");
        return SCAL_E_ARG;
    }
    if (n_frames > c->cfg.max_frames) {
        set_error("scal_refine_run: %d frames exceed max_frames %d", n_frames, c->cfg.max_frames);
        return SCAL_E_TOO_MANY;
    }
    if (offsets[0] != 0) {
        set_error("scal_refine_run: offsets[0] must be 0");
        return SCAL_E_ARG;
    }
    for (int f = 0; f < n_frames; ++f)
        if (offsets[f + 1] < offsets[f]) {
            set_error("scal_refine_run: offsets must not decrease");
            return SCAL_E_ARG;
        }
    if (offsets[n_frames] > c->cfg.max_points) {
        set_error("scal_refine_run: %d points exceed max_points %d", offsets[n_frames], c->cfg.max_points);
        return SCAL_E_TOO_MANY;
    }
    if (offsets[n_frames] > 0 && !xyzi) {
        set_error("scal_refine_run: bad argument");
        return SCAL_E_ARG;
    }
    return SCAL_OK;
}

namespace {
struct RfFrame {
    IcpIterState is;
    bool runs = false;    // not fixed and not empty: takes part in this round
    bool active = false;  // still iterating
};
}  // namespace

// one sweep of the frames marked active in h_ctrl (already uploaded): sums -> c->h_sums (waits)
// plane: the 32 point-to-plane sums on the moved normals c->gn -> c->h_plane instead
static int refine_sweep(scal_refine* c, int n, int n_frames, int nb, float max2, bool dense, bool plane) {
    hipStream_t s = c->stream;
    SCAL_LAUNCH_PROF("k_rf_grid_nn", k_rf_grid_nn, dim3(div_up(n, 4)), dim3(256), 0, s, c->cur.p, n, c->frame_of.p, c->goff.p, c->ctrl.p, c->ix.hkeys.p,
                     c->ix.hrange.p, c->ix.mask, c->ix.sorted.p, c->best.p, c->un_list.p, c->d_nun.p, dense ? 1 : 0);
    if (dense)
        SCAL_LAUNCH_PROF("k_rf_dense", k_rf_dense, dim3(RF_DENSE_WG), dim3(256), 0, s, c->cur.p, c->g.p, n, c->frame_of.p, c->goff.p, c->best.p,
                         c->un_list.p, c->d_nun.p);
    if (plane) {
        SCAL_LAUNCH_PROF("k_rf_plane_reduce", k_rf_plane_reduce, dim3(nb), dim3(256), 0, s, c->cur.p, c->g.p, c->gn.p, c->blocks.p, c->ctrl.p, c->best.p,
                         max2, c->plane_partials.p);
        hipLaunchKernelGGL(k_rf_final<ICP_PLANE_NSUM>, dim3(n_frames), dim3(64), 0, s, c->plane_partials.p, c->fb0.p, c->ctrl.p, c->h_plane.p, c->d_nun.p);
    } else {
        SCAL_LAUNCH_PROF("k_rf_reduce", k_rf_reduce, dim3(nb), dim3(256), 0, s, c->cur.p, c->g.p, c->blocks.p, c->ctrl.p, c->best.p, max2, c->partials.p);
        hipLaunchKernelGGL(k_rf_final<ICP_NSUM>, dim3(n_frames), dim3(64), 0, s, c->partials.p, c->fb0.p, c->ctrl.p, c->h_sums.p, c->d_nun.p);
    }
    SCAL_HIP(hipGetLastError());
    SCAL_HIP(hipStreamSynchronize(s));
    return SCAL_OK;
}

// Res = scal_refine_plane_frame_result: the point-to-plane metric on the frames' local normals d_nc (scal_refine_run_plane*)
template <class Res>
static int refine_rounds(scal_refine* c, const float4* d_loc, const float4* d_nc, const int* offsets, int K, double* poses12, const unsigned char* fixed,
                         double near_thres, int rounds, Res* res, int* rounds_run) {
    constexpr bool plane = std::is_same<Res, scal_refine_plane_frame_result>::value;
    constexpr int NS = plane ? ICP_PLANE_NSUM : ICP_NSUM;
    const double* const h_sums = plane ? c->h_plane.p : c->h_sums.p;
    hipStream_t s = c->stream;
    *rounds_run = 0;
    const double dmax = std::numeric_limits<double>::max();
    for (int f = 0; f < K; ++f) {
        std::memset(&res[f], 0, sizeof res[f]);
        for (int k = 0; k < 4; ++k) res[f].T[5 * k] = 1.0;
        res[f].fitness = dmax;
        if constexpr (plane) res[f].plane_fitness = dmax;
    }
    if (K == 0) return SCAL_OK;
    // the move's workgroups: the same for every round
    int nb_mm = 0;
    for (int f = 0; f < K; ++f)
        for (int i = offsets[f]; i < offsets[f + 1]; i += MM_TILE) c->h_mm_blocks.p[nb_mm++] = MMBlock{i, offsets[f + 1], f};
    if (nb_mm) SCAL_HIP(hipMemcpyAsync(c->mm_blocks.p, c->h_mm_blocks.p, sizeof(MMBlock) * nb_mm, hipMemcpyHostToDevice, s));
    const float max2 = static_cast<float>(c->cfg.max_corr_dist * c->cfg.max_corr_dist);
    const float last_bound = (static_cast<float>(ICP_RINGS) - 0.05f) * RF_CELL;
    // a query the rings leave unsettled has nothing nearer than last_bound: it only needs the dense sweep when the cap reaches further
    const bool dense = !(max2 < last_bound * last_bound);
    const double te = c->cfg.transformation_epsilon, fe = c->cfg.fitness_epsilon;
    std::vector<RfFrame> fr(K);
    for (int round = 0; round < rounds; ++round) {
        // 1. G = every frame moved by its pose
        std::memcpy(c->h_poses.p, poses12, sizeof(double) * 12 * K);
        SCAL_HIP(hipMemcpyAsync(c->poses.p, c->h_poses.p, sizeof(double) * 12 * K, hipMemcpyHostToDevice, s));
        int n = 0;
        if (nb_mm) {
            hipLaunchKernelGGL(k_rf_count, dim3(nb_mm), dim3(256), 0, s, d_loc, c->mm_blocks.p, near_thres, c->blk.p);
            SCAL_HIP(hipMemcpyAsync(c->h_blk.p, c->blk.p, sizeof(int) * nb_mm, hipMemcpyDeviceToHost, s));
            SCAL_HIP(hipStreamSynchronize(s));
            for (int b = 0; b < nb_mm; ++b) {  // exclusive prefix; a frame's offset in G is that of its first workgroup
                const int cnt = c->h_blk.p[b];
                c->h_blk.p[b] = n;
                n += cnt;
            }
        }
        int b_mm = 0, nb = 0;
        for (int f = 0; f < K; ++f) {
            const int n_wg = div_up(offsets[f + 1] - offsets[f], MM_TILE);
            c->h_goff.p[f] = n_wg ? c->h_blk.p[b_mm] : (b_mm < nb_mm ? c->h_blk.p[b_mm] : n);
            b_mm += n_wg;
        }
        c->h_goff.p[K] = n;
        for (int f = 0; f < K; ++f) {  // the sweeps' workgroups: 256 points counted from the frame's own first point
            c->h_fb0.p[f] = nb;
            for (int i = c->h_goff.p[f]; i < c->h_goff.p[f + 1]; i += 256) c->h_blocks.p[nb++] = RfBlock{i, c->h_goff.p[f + 1], f};
        }
        c->h_fb0.p[K] = nb;
        bool any = false;
        for (int f = 0; f < K; ++f) {
            fr[f] = RfFrame();
            const int nf = c->h_goff.p[f + 1] - c->h_goff.p[f];
            const bool is_fixed = fixed && fixed[f];
            fr[f].runs = fr[f].active = !is_fixed && nf > 0 && n - nf > 0;
            if (!is_fixed && !fr[f].runs) fr[f].is.st = 5;  // pcl::Registration::align refuses empty clouds: not converged
            any = any || fr[f].runs;
        }
        if (any) {
            SCAL_HIP(hipMemcpyAsync(c->blk.p, c->h_blk.p, sizeof(int) * nb_mm, hipMemcpyHostToDevice, s));
            SCAL_HIP(hipMemcpyAsync(c->goff.p, c->h_goff.p, sizeof(int) * (K + 1), hipMemcpyHostToDevice, s));
            SCAL_HIP(hipMemcpyAsync(c->fb0.p, c->h_fb0.p, sizeof(int) * (K + 1), hipMemcpyHostToDevice, s));
            SCAL_HIP(hipMemcpyAsync(c->blocks.p, c->h_blocks.p, sizeof(RfBlock) * nb, hipMemcpyHostToDevice, s));
            SCAL_LAUNCH_PROF("k_rf_write", k_rf_write, dim3(nb_mm), dim3(256), 0, s, d_loc, c->mm_blocks.p, c->poses.p, near_thres, c->blk.p,
                             static_cast<long long>(n), c->g.p, c->frame_of.p);
            if constexpr (plane)
                SCAL_LAUNCH_PROF("k_rf_write_nc", k_rf_write_nc, dim3(nb_mm), dim3(256), 0, s, d_loc, d_nc, c->mm_blocks.p, c->poses.p, near_thres, c->blk.p,
                                 static_cast<long long>(n), c->gn.p);
            SCAL_HIP(hipMemcpyAsync(c->cur.p, c->g.p, sizeof(float4) * n, hipMemcpyDeviceToDevice, s));
            // 2. the neighbour index over G
            SCAL_HIP(hipMemsetAsync(c->best.p, 0xff, sizeof(unsigned long long) * n, s));
            SCAL_TRY(c->ix.build(s, c->g.p, n, 1.0f / RF_CELL, RF_FINITE));
            // 3. the iterations: one launch chain and one synchronisation each, for all frames still iterating
            bool first = true;
            for (;;) {
                bool go = false;
                for (int f = 0; f < K; ++f) {
                    c->h_ctrl.p[f].active = fr[f].active ? 1 : 0;
                    go = go || fr[f].active;
                }
                if (!go) break;
                SCAL_HIP(hipMemcpyAsync(c->ctrl.p, c->h_ctrl.p, sizeof(RfCtrl) * K, hipMemcpyHostToDevice, s));
                if (!first) hipLaunchKernelGGL(k_rf_apply, dim3(nb), dim3(256), 0, s, c->cur.p, c->cur.p, c->blocks.p, c->ctrl.p);
                first = false;
                SCAL_TRY(refine_sweep(c, n, K, nb, max2, dense, plane));
                for (int f = 0; f < K; ++f) {
                    if (!fr[f].active) continue;
                    float T[16];
                    int step;
                    if constexpr (plane) {
                        if (fr[f].is.it == 0) std::memcpy(res[f].first_eq, h_sums + NS * f + 1, sizeof res[f].first_eq);
                        step = icp_plane_host_step(fr[f].is, h_sums + NS * f, c->cfg.max_iterations, te, fe, T);
                    } else {
                        step = icp_host_step(fr[f].is, h_sums + NS * f, c->cfg.max_iterations, te, fe, T);
                    }
                    if (step == ICP_STEP_CONTINUE)
                        std::memcpy(c->h_ctrl.p[f].m, T, sizeof(float) * 12);
                    else  // finished: the fitness sweep moves the frame by the whole transformation, the last increment need not be applied
                        fr[f].active = false;
                }
            }
            // 4. fitness: the moved frame by the whole transformation, one more sweep with the same cap
            for (int f = 0; f < K; ++f) {
                c->h_ctrl.p[f].active = fr[f].runs ? 1 : 0;
                std::memcpy(c->h_ctrl.p[f].m, fr[f].is.F, sizeof(float) * 12);
            }
            SCAL_HIP(hipMemcpyAsync(c->ctrl.p, c->h_ctrl.p, sizeof(RfCtrl) * K, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_rf_apply, dim3(nb), dim3(256), 0, s, c->g.p, c->cur.p, c->blocks.p, c->ctrl.p);
            SCAL_TRY(refine_sweep(c, n, K, nb, max2, dense, plane));
        }
        // 5. results and poses
        bool moved = false;
        for (int f = 0; f < K; ++f) {
            Res& r = res[f];
            const IcpIterState& is = fr[f].is;
            r.converged = is.converged ? 1 : 0, r.iterations = is.it, r.state = is.st, r.n_correspondences = is.n_corr;
            const double* sums = h_sums + NS * f;
            r.fitness = fr[f].runs && sums[0] > 0 ? sums[plane ? 29 : 16] / sums[0] : dmax;
            if constexpr (plane) {
                r.plane_fitness = fr[f].runs && sums[0] > 0 ? sums[28] / sums[0] : dmax;
                if (fr[f].runs)
                    std::memcpy(r.normal_eq, sums + 1, sizeof r.normal_eq);
                else  // a frame that does not run has no sweep, in this round or (its first_eq) in an earlier one
                    std::memset(r.normal_eq, 0, sizeof r.normal_eq), std::memset(r.first_eq, 0, sizeof r.first_eq);
            }
            for (int k = 0; k < 16; ++k) r.T[k] = is.F[k];
            r.accepted = fr[f].runs && is.converged && r.fitness <= c->cfg.fitness_gate ? 1 : 0;
            if (!r.accepted) continue;
            double* P = poses12 + 12 * f;
            double Q[12];
            for (int rr = 0; rr < 3; ++rr)
                for (int cc = 0; cc < 4; ++cc) {
                    const double F0 = is.F[4 * rr], F1 = is.F[4 * rr + 1], F2 = is.F[4 * rr + 2];
                    double v = (F0 * P[cc] + F1 * P[4 + cc]) + F2 * P[8 + cc];
                    if (cc == 3) v += static_cast<double>(is.F[4 * rr + 3]);
                    Q[4 * rr + cc] = v;
                }
            std::memcpy(P, Q, sizeof Q);
            const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            moved = moved || std::memcmp(is.F, I, sizeof I) != 0;
        }
        *rounds_run = round + 1;
        if (!moved) break;
    }
    return SCAL_OK;
}

extern "C" int scal_refine_run_device(scal_refine_t* c, const float* d_xyzi, const int* offsets, int n_frames, double* poses12, const unsigned char* fixed,
                                      double near_thres, int rounds, scal_refine_frame_result* res, int* rounds_run) {
    SCAL_TRY(refine_check_args(c, d_xyzi, offsets, n_frames, poses12, near_thres, rounds, res, rounds_run));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    return refine_rounds(c, reinterpret_cast<const float4*>(d_xyzi), nullptr, offsets, n_frames, poses12, fixed, near_thres, rounds, res, rounds_run);
}

extern "C" int scal_refine_run(scal_refine_t* c, const float* xyzi, const int* offsets, int n_frames, double* poses12, const unsigned char* fixed,
                               double near_thres, int rounds, scal_refine_frame_result* res, int* rounds_run) {
    SCAL_TRY(refine_check_args(c, xyzi, offsets, n_frames, poses12, near_thres, rounds, res, rounds_run));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    const int n = offsets[n_frames];
    if (!c->loc.p) SCAL_TRY(c->loc.alloc(static_cast<size_t>(c->cfg.max_points)));
    if (n) SCAL_HIP(hipMemcpyAsync(c->loc.p, xyzi, sizeof(float) * 4 * n, hipMemcpyHostToDevice, c->stream));
    return refine_rounds(c, c->loc.p, nullptr, offsets, n_frames, poses12, fixed, near_thres, rounds, res, rounds_run);
}

// what only the point-to-plane calls need, allocated by the first of them and released with the context
static int refine_plane_prepare(scal_refine* c, bool staging) {
    const size_t np = static_cast<size_t>(c->cfg.max_points);
    if (!c->gn.p) SCAL_TRY(c->gn.alloc(np));
    if (!c->plane_partials.p) SCAL_TRY(c->plane_partials.alloc(static_cast<size_t>(ICP_PLANE_NSUM) * c->nb_cap));
    if (!c->h_plane.p) SCAL_TRY(c->h_plane.alloc(static_cast<size_t>(ICP_PLANE_NSUM) * c->cfg.max_frames));
    if (staging && !c->nloc.p) SCAL_TRY(c->nloc.alloc(np));
    return SCAL_OK;
}

static int refine_plane_check_args(scal_refine* c, const float* xyzi, const float* nc, const int* offsets, int n_frames, double* poses12, double near_thres,
                                   int rounds, const void* res, int* rounds_run) {
    SCAL_TRY(refine_check_args(c, xyzi, offsets, n_frames, poses12, near_thres, rounds, res, rounds_run));
    if (offsets[n_frames] > 0 && !nc) {
        set_error("scal_refine_run_plane: bad argument (no normals)");
        return SCAL_E_ARG;
    }
    return SCAL_OK;
}

extern "C" int scal_refine_run_plane_device(scal_refine_t* c, const float* d_xyzi, const float* d_nc, const int* offsets, int n_frames, double* poses12,
                                            const unsigned char* fixed, double near_thres, int rounds, scal_refine_plane_frame_result* res,
                                            int* rounds_run) {
    SCAL_TRY(refine_plane_check_args(c, d_xyzi, d_nc, offsets, n_frames, poses12, near_thres, rounds, res, rounds_run));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    SCAL_TRY(refine_plane_prepare(c, false));
    return refine_rounds(c, reinterpret_cast<const float4*>(d_xyzi), reinterpret_cast<const float4*>(d_nc), offsets, n_frames, poses12, fixed, near_thres,
                         rounds, res, rounds_run);
}

extern "C" int scal_refine_run_plane(scal_refine_t* c, const float* xyzi, const float* nc, const int* offsets, int n_frames, double* poses12,
                                     const unsigned char* fixed, double near_thres, int rounds, scal_refine_plane_frame_result* res, int* rounds_run) {
    SCAL_TRY(refine_plane_check_args(c, xyzi, nc, offsets, n_frames, poses12, near_thres, rounds, res, rounds_run));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    SCAL_TRY(refine_plane_prepare(c, true));
    const int n = offsets[n_frames];
    if (!c->loc.p) SCAL_TRY(c->loc.alloc(static_cast<size_t>(c->cfg.max_points)));
    if (n) {
        SCAL_HIP(hipMemcpyAsync(c->loc.p, xyzi, sizeof(float) * 4 * n, hipMemcpyHostToDevice, c->stream));
        SCAL_HIP(hipMemcpyAsync(c->nloc.p, nc, sizeof(float) * 4 * n, hipMemcpyHostToDevice, c->stream));
    }
    return refine_rounds(c, c->loc.p, c->nloc.p, offsets, n_frames, poses12, fixed, near_thres, rounds, res, rounds_run);
}
