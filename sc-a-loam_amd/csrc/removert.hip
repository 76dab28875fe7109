// Dynamic-point removal from a merged keyframe map (scal_removert_*, include/scaloam_hip.h): the second offline use the reference's
// README names for a saved session and ships no code for.  The semantics are python/scaloam/removert.py's, bit for bit.
//
// One context, one stream (lane 0).  set_map bins the map once:
//   k_rv_bounds -> (host: grid) -> k_rv_count -> (host: scan of the cell counts, work items) -> k_rv_scatter
// run, per chunk of keyframes that fits the device:
//   fill (empty = the bits of +inf) -> k_rv_images (u32 atomic min on the f32 bits of r: positive floats order like unsigned ints)
//   -> k_rv_test
// and once at the end k_rv_finish (hits -> mask).  compact: k_rv_sel_count -> (host: scan of the block counts) -> k_rv_compact.
//
// k_rv_test is point-centric with plain global gathers: a work item is up to 64 points of ONE cell, owned by one wave, a point per
// lane.  The wave walks the chunk's keyframes 64 at a time - every lane tests one keyframe against the cell (XY distance to the
// cell's centre <= max_range + half diagonal), a ballot makes the list - and then visits the listed keyframes one by one: the pose
// is wave-uniform, every lane projects its own point and gathers one pixel per resolution.  Images staged in LDS were not built: a
// keyframe's images (11.5 KB at 2.5 degrees, 32 KB at 1.5) would be copied to serve 64 reads each, the whole image set of a chunk is
// read by every wave that lists the keyframe and stays in L2, and the f64 atan2 pair per visit outweighs the gathers.
// Each point's hit counts are read, added to and written once per chunk by the lane that owns it: no atomics on the large output.
#include "common.hpp"
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

namespace scal {

constexpr int RV_MAX_RES = 8;
constexpr int RV_MAX_CELLS = 1 << 18;
constexpr unsigned RV_EMPTY = 0x7f800000u;  // +inf: no in-range r reaches it

struct RvParams {
    int R, n_remove, min_hits, stride;  // stride: pixels of one keyframe's images
    int H[RV_MAX_RES], W[RV_MAX_RES], poff[RV_MAX_RES];
    float min_range, max_range, diff_thres;
    double fu, fd;
};
struct RvGrid {
    double x0, y0, cell, rad2;  // rad2: the square of (max_range + half diagonal), with slack for the roundings on the way
    int nx, ny;
};
struct RvItem {
    int first, count, ix, iy;
};

struct RvView {
    double az, el;
    float r;
};

// the part of the projection that does not depend on the resolution; false: outside the range gate
__device__ __forceinline__ bool rv_view(const double* __restrict__ P, const float4 p, float min_range, float max_range, RvView& o) {
    const double d0 = static_cast<double>(p.x) - P[3], d1 = static_cast<double>(p.y) - P[7], d2 = static_cast<double>(p.z) - P[11];
    const double x = (P[0] * d0 + P[4] * d1) + P[8] * d2;
    const double y = (P[1] * d0 + P[5] * d1) + P[9] * d2;
    const double z = (P[2] * d0 + P[6] * d1) + P[10] * d2;
    const double xy = x * x + y * y;
    o.r = static_cast<float>(sqrt(xy + z * z));
    if (!(o.r >= min_range && o.r <= max_range)) return false;
    o.az = atan2(y, x);
    o.el = atan2(z, sqrt(xy));
    return true;
}

// pixel index inside resolution i's image; -1: outside the field of view
__device__ __forceinline__ int rv_pixel(const RvParams& q, int i, const RvView& w) {
    const int H = q.H[i], W = q.W[i];
    const double u = (w.az + M_PI) / (2.0 * M_PI) * W;
    const double v = (q.fu - w.el) / (q.fu - q.fd) * H;
    if (!(v >= 0.0 && v < static_cast<double>(H))) return -1;
    const int row = static_cast<int>(v);
    const int col = max(0, min(static_cast<int>(u), W - 1));  // u >= 0 as |atan2| <= pi: the lower clamp only guards the memory
    return row * W + col;
}

__device__ __forceinline__ int rv_order(float f) {  // an int that orders like the float
    const int i = __float_as_int(f);
    return i ^ ((i >> 31) & 0x7fffffff);
}
static float rv_unorder(int i) {
    i ^= (i >> 31) & 0x7fffffff;
    float f;
    std::memcpy(&f, &i, sizeof f);
    return f;
}

__device__ __forceinline__ bool rv_finite(const float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// XY bounds of the finite records: b = {min x, max x, min y, max y} as ordered ints
__global__ void __launch_bounds__(256) k_rv_bounds(const float4* __restrict__ map, int n, int* __restrict__ b) {
    int lo_x = INT_MAX, hi_x = INT_MIN, lo_y = INT_MAX, hi_y = INT_MIN;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float4 p = map[i];
        if (!rv_finite(p)) continue;
        const int x = rv_order(p.x), y = rv_order(p.y);
        lo_x = min(lo_x, x), hi_x = max(hi_x, x), lo_y = min(lo_y, y), hi_y = max(hi_y, y);
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo_x = min(lo_x, __shfl_xor(lo_x, o)), hi_x = max(hi_x, __shfl_xor(hi_x, o));
        lo_y = min(lo_y, __shfl_xor(lo_y, o)), hi_y = max(hi_y, __shfl_xor(hi_y, o));
    }
    if ((threadIdx.x & 63) == 0 && lo_x <= hi_x) {
        atomicMin(b + 0, lo_x), atomicMax(b + 1, hi_x), atomicMin(b + 2, lo_y), atomicMax(b + 3, hi_y);
    }
}

// the cell of a record; nx * ny (one past the last cell) for a record that is not finite
__device__ __forceinline__ int rv_cell(const RvGrid& g, const float4 p) {
    if (!rv_finite(p)) return g.nx * g.ny;
    const int ix = static_cast<int>(floor((static_cast<double>(p.x) - g.x0) / g.cell));
    const int iy = static_cast<int>(floor((static_cast<double>(p.y) - g.y0) / g.cell));
    // the host sized the grid from the same expressions on the bounds: the clamps only guard the memory
    return max(0, min(iy, g.ny - 1)) * g.nx + max(0, min(ix, g.nx - 1));
}

// One atomic per wave and cell instead of one per record: neighbouring records mostly share a cell (a map is keyframe after
// keyframe), and a few thousand records per cell on one counter is what the plain form spent its time on.  Returns the slot
// atomicAdd(counter + c, 1) would have given this lane, had the wave's lanes of one cell gone in lane order; -1 for !valid.
// Every lane of the wave must call it.  The loop runs once per distinct cell in the wave and is driven by the ballot of the lanes
// still waiting, which changes every round: a loop that only re-reads the first active lane's cell has no state of its own, and the
// compiler, entitled to assume that such a loop ends, drops it and counts the whole wave into the first lane's cell.
__device__ __forceinline__ int rv_wave_add(int* __restrict__ counter, int c, bool valid) {
    const int lane = threadIdx.x & 63;
    int slot = -1;
    unsigned long long waiting = __ballot(valid);
    while (waiting) {
        const int leader = __ffsll(static_cast<long long>(waiting)) - 1;
        const int c0 = __shfl(c, leader);
        const bool mine = valid && c == c0;
        const unsigned long long peers = __ballot(mine);  // holds the leader's bit: every round takes lanes out of `waiting`
        int base = 0;
        if (lane == leader) base = atomicAdd(counter + c0, __popcll(peers));
        base = __shfl(base, leader);
        if (mine) slot = base + __popcll(peers & ((1ull << lane) - 1));
        waiting &= ~peers;
    }
    return slot;
}

__global__ void __launch_bounds__(256) k_rv_count(const float4* __restrict__ map, int n, RvGrid g, int* __restrict__ count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    rv_wave_add(count, i < n ? rv_cell(g, map[i]) : 0, i < n);
}

// cursor: the cells' first slots on entry.  The order inside a cell depends on the run; no result does (every output is indexed by
// the record's own index).
__global__ void __launch_bounds__(256) k_rv_scatter(const float4* __restrict__ map, int n, RvGrid g, int* __restrict__ cursor,
                                                    int* __restrict__ perm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int c = i < n ? rv_cell(g, map[i]) : 0;
    const bool valid = i < n && c != g.nx * g.ny;
    const int slot = rv_wave_add(cursor, c, valid);
    if (valid) perm[slot] = i;
}

// off: the chunk's kc + 1 scan offsets (off[0] = 0).  img: kc images sets of q.stride pixels each, filled with RV_EMPTY.
__global__ void __launch_bounds__(256) k_rv_images(const float4* __restrict__ scans, const int* __restrict__ off, int kc, RvParams q,
                                                   unsigned* __restrict__ img) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= off[kc]) return;
    int lo = 0, hi = kc;  // the scan k with off[k] <= i < off[k + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    RvView w;
    if (!rv_view(I, scans[i], q.min_range, q.max_range, w)) return;
    unsigned* dst = img + static_cast<size_t>(lo) * q.stride;
#pragma unroll
    for (int r = 0; r < RV_MAX_RES; ++r) {
        if (r >= q.R) break;
        const int px = rv_pixel(q, r, w);
        if (px >= 0) atomicMin(dst + q.poff[r] + px, __float_as_uint(w.r));
    }
}

// one wave per work item (four items per block); hits: [R][n] u16, read - add - write by the owning lane
__global__ void __launch_bounds__(256) k_rv_test(const float4* __restrict__ map, int n, const int* __restrict__ perm,
                                                 const RvItem* __restrict__ items, int n_items, RvGrid g, const double* __restrict__ poses,
                                                 int kc, RvParams q, const unsigned* __restrict__ img, unsigned short* __restrict__ hits,
                                                 unsigned long long* __restrict__ pairs) {
    const int it = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (it >= n_items) return;
    const RvItem item = items[it];
    const bool active = lane < item.count;
    const int m = active ? perm[item.first + lane] : 0;
    const float4 p = active ? map[m] : make_float4(0.f, 0.f, 0.f, 0.f);
    const double cx = g.x0 + (item.ix + 0.5) * g.cell, cy = g.y0 + (item.iy + 0.5) * g.cell;
    int h[RV_MAX_RES];
#pragma unroll
    for (int r = 0; r < RV_MAX_RES; ++r) h[r] = 0;
    int visited = 0;
    for (int k0 = 0; k0 < kc; k0 += 64) {
        const int k = k0 + lane;
        bool listed = false;
        if (k < kc) {
            const double dx = poses[12 * static_cast<size_t>(k) + 3] - cx, dy = poses[12 * static_cast<size_t>(k) + 7] - cy;
            listed = dx * dx + dy * dy <= g.rad2;
        }
        unsigned long long list = __ballot(listed);
        while (list) {
            const int kk = k0 + __ffsll(static_cast<long long>(list)) - 1;  // the same in every lane
            list &= list - 1;
            ++visited;
            RvView w;
            if (!active || !rv_view(poses + 12 * static_cast<size_t>(kk), p, q.min_range, q.max_range, w)) continue;
            const unsigned* src = img + static_cast<size_t>(kk) * q.stride;
#pragma unroll
            for (int r = 0; r < RV_MAX_RES; ++r) {
                if (r >= q.R) break;
                const int px = rv_pixel(q, r, w);
                if (px < 0) continue;
                const unsigned bits = src[q.poff[r] + px];
                if (bits != RV_EMPTY && (__uint_as_float(bits) - w.r) > q.diff_thres) ++h[r];
            }
        }
    }
    if (active) {
#pragma unroll
        for (int r = 0; r < RV_MAX_RES; ++r) {
            if (r >= q.R) break;
            if (h[r]) {
                unsigned short* dst = hits + static_cast<size_t>(r) * n + m;
                *dst = static_cast<unsigned short>(min(static_cast<int>(*dst) + h[r], 65535));
            }
        }
    }
    if (lane == 0) atomicAdd(pairs, static_cast<unsigned long long>(visited) * item.count);
}

__global__ void __launch_bounds__(256) k_rv_finish(const unsigned short* __restrict__ hits, int n, RvParams q, unsigned char* __restrict__ mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool removed = false, kept = false;
    for (int r = 0; r < q.n_remove; ++r) removed |= hits[static_cast<size_t>(r) * n + i] >= q.min_hits;
    for (int r = q.n_remove; r < q.R; ++r) kept |= hits[static_cast<size_t>(r) * n + i] < 1;
    mask[i] = removed && !kept;
}

// records with mask == which, per block of 256
__global__ void __launch_bounds__(256) k_rv_sel_count(const unsigned char* __restrict__ mask, int n, int which, int* __restrict__ block_count) {
    __shared__ int s_wave[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long b = __ballot(i < n && mask[i] == which);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// block_first: the exclusive scan of block_count; the selected records keep their order
__global__ void __launch_bounds__(256) k_rv_compact(const float4* __restrict__ map, const unsigned char* __restrict__ mask, int n, int which,
                                                    const int* __restrict__ block_first, int cap, float4* __restrict__ out) {
    __shared__ int s_wave[4];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool sel = i < n && mask[i] == which;
    const unsigned long long b = __ballot(sel);
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int pos = block_first[blockIdx.x] + __popcll(b & ((1ull << lane) - 1));
    for (int w = 0; w < wave; ++w) pos += s_wave[w];
    if (sel && pos < cap) out[pos] = map[i];
}

}  // namespace scal

using namespace scal;

struct scal_removert {
    scal_removert_config cfg;  // zeros replaced by the defaults
    LaneStream stream;
    int pix_cap = 0;           // pixels of one image at min_res_deg: a run's images are no larger
    DevBuf<float4> own_map, scans, out;
    DevBuf<int> d_bounds, d_cells, d_perm, d_off, d_blocks;
    DevBuf<RvItem> d_items;
    DevBuf<double> d_poses;
    DevBuf<unsigned> d_img;
    DevBuf<unsigned short> d_hits;
    DevBuf<unsigned char> d_mask;
    DevBuf<unsigned long long> d_pairs;
    PinBuf<double> h_poses;
    PinBuf<int> h_off;
    const float4* map = nullptr;  // own_map or the caller's records
    int n = -1;                   // -1: no map set
    int n_items = 0;
    RvGrid grid{};
    // the last run
    bool have_run = false;
    RvParams q{};
    int res_k0 = 0, res_k1 = 0;   // keyframes whose images are resident
};

static bool rv_pos(double v) { return v > 0 && std::isfinite(v); }
static bool rv_nonneg(double v) { return v >= 0 && std::isfinite(v); }

// (H, W) at res degrees per pixel; false: no such image
static bool rv_shape(const scal_removert_config& g, double res, int* H, int* W) {
    if (!(res > 0) || !(res <= 360.0)) return false;
    const double h = (g.fov_up_deg - g.fov_down_deg) / res, w = 360.0 / res;
    if (!(h < 1e6) || !(w < 1e6)) return false;
    *H = std::max(1l, std::lround(h)), *W = static_cast<int>(std::lround(w));
    return *W >= 1;
}

extern "C" int scal_removert_create(const scal_removert_config* cfg, scal_removert_t** out) {
    if (!cfg || !out || cfg->max_points <= 0 || cfg->max_points > (1 << 30) || cfg->max_keyframes <= 0 || cfg->max_keyframes > (1 << 24) ||
        cfg->max_scan_points <= 0 || cfg->max_scan_points > (1 << 30) || cfg->max_resolutions <= 0 || cfg->max_resolutions > RV_MAX_RES ||
        cfg->min_hits < 1 || cfg->min_hits > 65535 || !std::isfinite(cfg->fov_up_deg) || !std::isfinite(cfg->fov_down_deg) ||
        !(cfg->fov_up_deg > cfg->fov_down_deg) || cfg->fov_up_deg > 90.0 || cfg->fov_down_deg < -90.0 || !rv_pos(cfg->min_range) ||
        !rv_pos(cfg->max_range) || cfg->min_range > cfg->max_range || !rv_pos(cfg->diff_thres) || !rv_nonneg(cfg->min_res_deg) ||
        cfg->min_res_deg > 360.0 || !rv_nonneg(cfg->cell_size)) {
        set_error("scal_removert_create: bad argument");
        return SCAL_E_ARG;
    }
    scal_removert_config g = *cfg;
    if (g.min_res_deg == 0) g.min_res_deg = 1.0;
    if (g.cell_size == 0) g.cell_size = g.max_range / 8;
    int H = 0, W = 0;
    if (!rv_shape(g, g.min_res_deg, &H, &W) || static_cast<double>(H) * W * g.max_resolutions * g.max_keyframes > 1e9) {
        set_error("scal_removert_create: bad argument (the images at min_res_deg = %g need more than 1e9 pixels)", g.min_res_deg);
        return SCAL_E_ARG;
    }
    *out = nullptr;
    SCAL_TRY(select_device(g.device));
    auto* c = new scal_removert();
    c->cfg = g;
    // every image of a run is at a resolution >= min_res_deg; one more row and column cover the roundings of H and W
    c->pix_cap = (H + 1) * (W + 1);
    const size_t np = static_cast<size_t>(g.max_points), nk = static_cast<size_t>(g.max_keyframes);
    int rc = SCAL_OK;
    auto A = [&](int r) { if (rc == SCAL_OK) rc = r; };
    A(c->stream.acquire(g.device, 0));
    A(c->scans.alloc(static_cast<size_t>(g.max_scan_points)));
    A(c->d_bounds.alloc(4)); A(c->d_cells.alloc(RV_MAX_CELLS + 1)); A(c->d_perm.alloc(np));
    A(c->d_items.alloc(np / 64 + RV_MAX_CELLS + 1));
    A(c->d_off.alloc(nk + 1)); A(c->d_poses.alloc(12 * nk)); A(c->h_off.alloc(nk + 1)); A(c->h_poses.alloc(12 * nk));
    A(c->d_img.alloc(nk * g.max_resolutions * c->pix_cap));
    A(c->d_hits.alloc(np * g.max_resolutions)); A(c->d_mask.alloc(np)); A(c->d_pairs.alloc(1));
    A(c->d_blocks.alloc(np / 256 + 1));
    if (rc != SCAL_OK) {
        scal_removert_destroy(c);
        return rc;
    }
    *out = c;
    return SCAL_OK;
}

extern "C" void scal_removert_destroy(scal_removert_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

// bins the n records at c->map
static int rv_bin(scal_removert* c, int n) {
    hipStream_t s = c->stream;
    c->n = -1, c->have_run = false, c->n_items = 0;
    if (n == 0) {
        c->n = 0;
        return SCAL_OK;
    }
    int b[4] = {INT_MAX, INT_MIN, INT_MAX, INT_MIN};
    SCAL_HIP(hipMemcpyAsync(c->d_bounds.p, b, sizeof b, hipMemcpyHostToDevice, s));
    SCAL_LAUNCH_PROF("k_rv_bounds", k_rv_bounds, dim3(std::min(div_up(n, 256), 2048)), dim3(256), 0, s, c->map, n, c->d_bounds.p);
    SCAL_HIP(hipGetLastError());
    SCAL_HIP(hipMemcpyAsync(b, c->d_bounds.p, sizeof b, hipMemcpyDeviceToHost, s));
    SCAL_HIP(hipStreamSynchronize(s));
    if (b[0] > b[1]) {  // no finite record: nothing is ever tested
        c->n = n;
        return SCAL_OK;
    }
    RvGrid& g = c->grid;
    g.x0 = rv_unorder(b[0]), g.y0 = rv_unorder(b[2]);
    const double x1 = rv_unorder(b[1]), y1 = rv_unorder(b[3]);
    double nx = 0, ny = 0;
    for (g.cell = c->cfg.cell_size;; g.cell *= 2) {  // a grid of more than RV_MAX_CELLS cells gets larger cells
        nx = std::floor((x1 - g.x0) / g.cell) + 1, ny = std::floor((y1 - g.y0) / g.cell) + 1;
        if (nx * ny <= RV_MAX_CELLS) break;
    }
    g.nx = static_cast<int>(nx), g.ny = static_cast<int>(ny);
    // r <= max_range is taken on the f32 rounding of r and the cell index on a rounded quotient: 1e-6 relative covers both
    const double rad = (c->cfg.max_range + g.cell * std::sqrt(0.5)) * (1.0 + 1e-6);
    g.rad2 = rad * rad;
    const int n_cells = g.nx * g.ny;
    SCAL_HIP(hipMemsetAsync(c->d_cells.p, 0, sizeof(int) * (static_cast<size_t>(n_cells) + 1), s));
    SCAL_LAUNCH_PROF("k_rv_count", k_rv_count, dim3(div_up(n, 256)), dim3(256), 0, s, c->map, n, g, c->d_cells.p);
    SCAL_HIP(hipGetLastError());
    std::vector<int> cnt(static_cast<size_t>(n_cells) + 1);
    SCAL_HIP(hipMemcpyAsync(cnt.data(), c->d_cells.p, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost, s));
    SCAL_HIP(hipStreamSynchronize(s));
    std::vector<RvItem> items;
    items.reserve(static_cast<size_t>(n) / 64 + 64);
    int first = 0;
    for (int cell = 0; cell < n_cells; ++cell) {
        const int m = cnt[cell];
        cnt[cell] = first;
        for (int o = 0; o < m; o += 64) items.push_back({first + o, std::min(64, m - o), cell % g.nx, cell / g.nx});
        first += m;
    }
    if (items.size() > c->d_items.n) {  // cannot happen: n / 64 + one partial item per cell
        set_error("scal_removert_set_map: %zu work items exceed the %zu reserved", items.size(), c->d_items.n);
        return SCAL_E_CAPACITY;
    }
    SCAL_HIP(hipMemcpyAsync(c->d_cells.p, cnt.data(), sizeof(int) * static_cast<size_t>(n_cells), hipMemcpyHostToDevice, s));
    if (!items.empty()) SCAL_HIP(hipMemcpyAsync(c->d_items.p, items.data(), sizeof(RvItem) * items.size(), hipMemcpyHostToDevice, s));
    SCAL_LAUNCH_PROF("k_rv_scatter", k_rv_scatter, dim3(div_up(n, 256)), dim3(256), 0, s, c->map, n, g, c->d_cells.p, c->d_perm.p);
    SCAL_HIP(hipGetLastError());
    SCAL_HIP(hipStreamSynchronize(s));  // cnt and items go away
    c->n_items = static_cast<int>(items.size());
    c->n = n;
    return SCAL_OK;
}

static int rv_check_map(scal_removert* c, const char* who, const float* xyzi, int n) {
    if (!c || n < 0 || (n > 0 && !xyzi)) {
        set_error("%s: bad argument", who);
        return SCAL_E_ARG;
    }
    if (n > c->cfg.max_points) {
        set_error("%s: the map has %d points, max_points is %d", who, n, c->cfg.max_points);
        return SCAL_E_TOO_MANY;
    }
    return SCAL_OK;
}

extern "C" int scal_removert_set_map(scal_removert_t* c, const float* xyzi, int n) {
    SCAL_TRY(rv_check_map(c, "scal_removert_set_map", xyzi, n));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    c->n = -1;
    if (!c->own_map.p) SCAL_TRY(c->own_map.alloc(static_cast<size_t>(c->cfg.max_points)));  // a context fed from the device never needs it
    if (n > 0) SCAL_HIP(hipMemcpyAsync(c->own_map.p, xyzi, sizeof(float4) * static_cast<size_t>(n), hipMemcpyHostToDevice, c->stream));
    c->map = c->own_map.p;
    return rv_bin(c, n);
}

extern "C" int scal_removert_set_map_device(scal_removert_t* c, const float* d_xyzi, int n) {
    SCAL_TRY(rv_check_map(c, "scal_removert_set_map_device", d_xyzi, n));
    SCAL_HIP(hipSetDevice(c->cfg.device));
    c->map = reinterpret_cast<const float4*>(d_xyzi);
    return rv_bin(c, n);
}

extern "C" int scal_removert_run(scal_removert_t* c, const float* scans_xyzi, const int* offsets, int K, const double* poses12,
                                 const double* remove_res, int n_remove, const double* revert_res, int n_revert, unsigned char* dynamic_out,
                                 unsigned short* hits_out, scal_removert_stats* stats) {
    if (!c || !offsets || K < 0 || (K > 0 && !poses12) || !remove_res || n_remove < 1 || n_revert < 0 || (n_revert > 0 && !revert_res) ||
        !stats || offsets[0] != 0) {
        set_error("scal_removert_run: bad argument");
        return SCAL_E_ARG;
    }
    if (c->n < 0) {
        set_error("scal_removert_run: no map set");
        return SCAL_E_STATE;
    }
    const int n = c->n;
    if ((n > 0 && !dynamic_out) || static_cast<long long>(n_remove) + n_revert > c->cfg.max_resolutions) {
        set_error("scal_removert_run: bad argument (%d + %d resolutions, max_resolutions is %d)", n_remove, n_revert, c->cfg.max_resolutions);
        return SCAL_E_ARG;
    }
    RvParams q{};
    q.R = n_remove + n_revert, q.n_remove = n_remove, q.min_hits = c->cfg.min_hits;
    int finest = 0;
    for (int i = 0; i < q.R; ++i) {
        const double res = i < n_remove ? remove_res[i] : revert_res[i - n_remove];
        if (!(res >= c->cfg.min_res_deg) || !rv_shape(c->cfg, res, &q.H[i], &q.W[i]) || q.H[i] * q.W[i] > c->pix_cap) {
            set_error("scal_removert_run: resolution %d is %g degrees; it must lie in [min_res_deg = %g, 360]", i, res, c->cfg.min_res_deg);
            return SCAL_E_ARG;
        }
        q.poff[i] = q.stride;
        q.stride += q.H[i] * q.W[i];
        if (i < n_remove && res < remove_res[finest]) finest = i;
    }
    for (int k = 0; k < K; ++k) {
        if (offsets[k + 1] < offsets[k]) {
            set_error("scal_removert_run: offsets must not decrease");
            return SCAL_E_ARG;
        }
        if (offsets[k + 1] - offsets[k] > c->cfg.max_scan_points) {
            set_error("scal_removert_run: scan %d has %d points, max_scan_points is %d", k, offsets[k + 1] - offsets[k], c->cfg.max_scan_points);
            return SCAL_E_TOO_MANY;
        }
        for (int j = 0; j < 12; ++j)
            if (!std::isfinite(poses12[12 * static_cast<size_t>(k) + j])) {
                set_error("scal_removert_run: pose %d is not finite", k);
                return SCAL_E_ARG;
            }
    }
    if (K > 0 && offsets[K] > 0 && !scans_xyzi) {
        set_error("scal_removert_run: bad argument");
        return SCAL_E_ARG;
    }
    q.min_range = static_cast<float>(c->cfg.min_range), q.max_range = static_cast<float>(c->cfg.max_range);
    q.diff_thres = static_cast<float>(c->cfg.diff_thres);
    q.fu = c->cfg.fov_up_deg * (M_PI / 180.0), q.fd = c->cfg.fov_down_deg * (M_PI / 180.0);
    SCAL_HIP(hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    c->have_run = false;
    std::memset(stats, 0, sizeof *stats);
    stats->points = n, stats->keyframes = K, stats->pairs_bruteforce = static_cast<long long>(n) * K;
    if (n == 0) {
        c->q = q, c->res_k0 = c->res_k1 = 0, c->have_run = true;
        return SCAL_OK;
    }
    SCAL_HIP(hipMemsetAsync(c->d_hits.p, 0, sizeof(unsigned short) * static_cast<size_t>(n) * q.R, s));
    SCAL_HIP(hipMemsetAsync(c->d_pairs.p, 0, sizeof(unsigned long long), s));
    int k0 = 0, k1 = 0;
    while (k1 < K) {
        k0 = k1;
        while (k1 < K && k1 - k0 < c->cfg.max_keyframes && offsets[k1 + 1] - offsets[k0] <= c->cfg.max_scan_points) ++k1;
        const int kc = k1 - k0, ns = offsets[k1] - offsets[k0];
        for (int k = 0; k <= kc; ++k) c->h_off.p[k] = offsets[k0 + k] - offsets[k0];
        std::memcpy(c->h_poses.p, poses12 + 12 * static_cast<size_t>(k0), sizeof(double) * 12 * static_cast<size_t>(kc));
        SCAL_HIP(hipMemcpyAsync(c->d_off.p, c->h_off.p, sizeof(int) * (static_cast<size_t>(kc) + 1), hipMemcpyHostToDevice, s));
        SCAL_HIP(hipMemcpyAsync(c->d_poses.p, c->h_poses.p, sizeof(double) * 12 * static_cast<size_t>(kc), hipMemcpyHostToDevice, s));
        SCAL_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->d_img.p), static_cast<int>(RV_EMPTY), static_cast<size_t>(kc) * q.stride, s));
        if (ns > 0) {
            SCAL_HIP(hipMemcpyAsync(c->scans.p, scans_xyzi + 4 * static_cast<size_t>(offsets[k0]), sizeof(float4) * static_cast<size_t>(ns),
                                    hipMemcpyHostToDevice, s));
            SCAL_LAUNCH_PROF("k_rv_images", k_rv_images, dim3(div_up(ns, 256)), dim3(256), 0, s, c->scans.p, c->d_off.p, kc, q, c->d_img.p);
            SCAL_HIP(hipGetLastError());
        }
        if (c->n_items > 0) {
            SCAL_LAUNCH_PROF("k_rv_test", k_rv_test, dim3(div_up(c->n_items, 4)), dim3(256), 0, s, c->map, n, c->d_perm.p, c->d_items.p, c->n_items,
                             c->grid, c->d_poses.p, kc, q, c->d_img.p, c->d_hits.p, c->d_pairs.p);
            SCAL_HIP(hipGetLastError());
        }
        SCAL_HIP(hipStreamSynchronize(s));  // the pinned offsets and poses are free for the next chunk
    }
    SCAL_LAUNCH_PROF("k_rv_finish", k_rv_finish, dim3(div_up(n, 256)), dim3(256), 0, s, c->d_hits.p, n, q, c->d_mask.p);
    SCAL_HIP(hipGetLastError());
    unsigned long long pairs = 0;
    SCAL_HIP(hipMemcpyAsync(dynamic_out, c->d_mask.p, static_cast<size_t>(n), hipMemcpyDeviceToHost, s));
    if (hits_out)
        SCAL_HIP(hipMemcpyAsync(hits_out, c->d_hits.p + static_cast<size_t>(finest) * n, sizeof(unsigned short) * static_cast<size_t>(n),
                                hipMemcpyDeviceToHost, s));
    SCAL_HIP(hipMemcpyAsync(&pairs, c->d_pairs.p, sizeof pairs, hipMemcpyDeviceToHost, s));
    SCAL_HIP(hipStreamSynchronize(s));
    long long dyn = 0;
    for (int i = 0; i < n; ++i) dyn += dynamic_out[i];
    stats->dynamic = dyn, stats->pairs_tested = static_cast<long long>(pairs);
    c->q = q, c->res_k0 = k0, c->res_k1 = k1, c->have_run = true;
    return SCAL_OK;
}

extern "C" int scal_removert_compact(scal_removert_t* c, int which, float* out_xyzi, int cap, int* n_out) {
    if (!c || (which != 0 && which != 1) || cap < 0 || (cap > 0 && !out_xyzi) || !n_out) {
        set_error("scal_removert_compact: bad argument");
        return SCAL_E_ARG;
    }
    if (!c->have_run) {
        set_error("scal_removert_compact: no run on this map yet");
        return SCAL_E_STATE;
    }
    *n_out = 0;
    const int n = c->n;
    if (n == 0) return SCAL_OK;
    SCAL_HIP(hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    const int nb = div_up(n, 256);
    SCAL_LAUNCH_PROF("k_rv_sel_count", k_rv_sel_count, dim3(nb), dim3(256), 0, s, c->d_mask.p, n, which, c->d_blocks.p);
    SCAL_HIP(hipGetLastError());
    std::vector<int> blocks(static_cast<size_t>(nb));
    SCAL_HIP(hipMemcpyAsync(blocks.data(), c->d_blocks.p, sizeof(int) * blocks.size(), hipMemcpyDeviceToHost, s));
    SCAL_HIP(hipStreamSynchronize(s));
    int total = 0;
    for (int& b : blocks) {
        const int m = b;
        b = total;
        total += m;
    }
    *n_out = total;
    const int m = std::min(total, cap);
    if (m == 0) return SCAL_OK;
    if (c->out.n < static_cast<size_t>(m) || !c->out.p) SCAL_TRY(c->out.alloc(static_cast<size_t>(m)));
    SCAL_HIP(hipMemcpyAsync(c->d_blocks.p, blocks.data(), sizeof(int) * blocks.size(), hipMemcpyHostToDevice, s));
    SCAL_LAUNCH_PROF("k_rv_compact", k_rv_compact, dim3(nb), dim3(256), 0, s, c->map, c->d_mask.p, n, which, c->d_blocks.p, m, c->out.p);
    SCAL_HIP(hipGetLastError());
    SCAL_HIP(hipMemcpyAsync(out_xyzi, c->out.p, sizeof(float4) * static_cast<size_t>(m), hipMemcpyDeviceToHost, s));
    SCAL_HIP(hipStreamSynchronize(s));
    return SCAL_OK;
}

extern "C" int scal_removert_scan_image(scal_removert_t* c, int k, int res_index, float* out, int H, int W) {
    if (!c || !out || k < 0 || res_index < 0) {
        set_error("scal_removert_scan_image: bad argument");
        return SCAL_E_ARG;
    }
    if (!c->have_run || k < c->res_k0 || k >= c->res_k1) {
        set_error("scal_removert_scan_image: keyframe %d is not resident (the last run left keyframes %d .. %d)", k, c->res_k0, c->res_k1 - 1);
        return SCAL_E_STATE;
    }
    if (res_index >= c->q.R || H != c->q.H[res_index] || W != c->q.W[res_index]) {
        set_error("scal_removert_scan_image: bad argument (no %d x %d image at resolution index %d)", H, W, res_index);
        return SCAL_E_ARG;
    }
    SCAL_HIP(hipSetDevice(c->cfg.device));
    // the pixels are the f32 bits of r, the empty ones those of +inf
    SCAL_HIP(hipMemcpyAsync(out, c->d_img.p + static_cast<size_t>(k - c->res_k0) * c->q.stride + c->q.poff[res_index],
                            sizeof(float) * static_cast<size_t>(H) * W, hipMemcpyDeviceToHost, c->stream));
    SCAL_HIP(hipStreamSynchronize(c->stream));
    return SCAL_OK;
}
