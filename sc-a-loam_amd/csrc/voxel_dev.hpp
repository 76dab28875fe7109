// pcl::VoxelGrid<PointXYZI> on the device (SoA clouds, device-resident counts).  See voxel.hip.
#pragma once
#include "common.hpp"
#include "radix_sort.hpp"

namespace scal {

struct VoxMeta {
    int error;                  // SCAL_E_CAPACITY when an axis needs more cells than the key layout holds
    int n_out;
    int guard;                  // PCL's "leaf size is too small" guard fired: output = input
    int used_bits;              // key bits in use (device-adaptive: the sort skips the passes above them)
    int b0, b1;                 // bit widths of the x and y voxel coordinates inside the key
};

struct CSoA4 {
    const float *x, *y, *z, *w;
};
struct SoA4 {
    float *x, *y, *z, *w;
    operator CSoA4() const { return CSoA4{x, y, z, w}; }
};

// Optional epilogue of a filter run, executed by its last kernel (saves one-thread launches on dependent chains):
// *slots_out = min(*other_n + n_out, slots_cap) when slots_out is set; *err_out = error code when one was raised.
struct VoxTail {
    int* err_out = nullptr;
    int* slots_out = nullptr;
    const int* other_n = nullptr;
    int slots_cap = 0;
};

struct VoxelFilter {
    int cap = 0;
    RadixSort sorter;
    DevBuf<unsigned long long> keys;
    DevBuf<int> vals;
    DevBuf<int> blockcnt;
    DevBuf<VoxMeta> meta;
    DevBuf<unsigned> box_parts;  // [128][6] per-block bounding boxes (k_vox_bbox)
    std::string n_bbox = "k_vox_bbox", n_keys = "k_vox_keys", n_heads = "k_vox_heads", n_reduce = "k_vox_reduce", n_small = "k_vox_small",
                n_small_reduce = "k_vox_small_reduce";
    void set_tag(const char* tag) {  // stage tag of the timed launches, see RadixSort::set_tag
        n_bbox = std::string("k_vox_bbox") + tag, n_keys = std::string("k_vox_keys") + tag, n_heads = std::string("k_vox_heads") + tag;
        n_reduce = std::string("k_vox_reduce") + tag, n_small = std::string("k_vox_small") + tag;
        n_small_reduce = std::string("k_vox_small_reduce") + tag;
        sorter.set_tag(tag);
    }

    int init(int capacity);
    // out must hold `cap` points.  The key packs the three voxel coordinates as tightly as the bounding box allows
    // (computed on the device); max_bits bounds the passes the host enqueues (a multiple of 9 avoids waste).
    // n_bound: host-known upper bound of *d_n; clouds of <= 8192 points take a single-workgroup LDS path.
    // d_n_out receives the number of centroids; meta.p->error is set when the box needs more than max_bits.
    // ext_parts / n_parts: per-block boxes of the cloud written by an earlier kernel (vox_bbox_block_store): the reset and
    // bounding-box launches are skipped, the key kernel reduces the parts itself.
    int run(hipStream_t s, CSoA4 in, const int* d_n, int n_bound, float leaf, int max_bits, SoA4 out, int* d_n_out, const VoxTail* tail = nullptr,
            const unsigned* ext_parts = nullptr, int n_parts = 0);
};

void launch_deinterleave(hipStream_t s, const float* aos, int n, SoA4 o);
void launch_interleave(hipStream_t s, const int* d_n, int n_cap, CSoA4 in, float* aos);

// pcl::VoxelGrid over a cloud of 16-byte xyzi records in HBM (45 key bits): the filter, its SoA planes, the device counts and the
// pinned words the host reads the result from.  A caller chains the steps it needs on its stream, `n` being the host-known bound of
// the input count throughout:
//   load (or load_counted behind a producer of the records, or a producer of the input planes) -> filter -> store -> wait
struct CloudFilter {
    struct Host {
        int n_in, n_out;
        VoxMeta meta;
    };
    VoxelFilter vf;
    DevBuf<float> plane_in[4], plane_out[4];
    DevBuf<int> d_n;  // [0] points in, [1] centroids out
    PinBuf<Host> h;

    int init(int capacity);
    bool ready() const { return h.p != nullptr; }
    void set_tag(const char* tag) { vf.set_tag(tag); }
    SoA4 in() const { return SoA4{plane_in[0].p, plane_in[1].p, plane_in[2].p, plane_in[3].p}; }      // a producer may fill these itself (and *d_n_in())
    SoA4 out() const { return SoA4{plane_out[0].p, plane_out[1].p, plane_out[2].p, plane_out[3].p}; }  // *d_n_out() centroids, valid behind filter()
    int* d_n_in() const { return d_n.p; }
    int* d_n_out() const { return d_n.p + 1; }
    // n records at d_xyzi -> the input planes; load() also uploads n, load_counted() expects a kernel to have written *d_n_in()
    int load(hipStream_t s, const float* d_xyzi, int n);
    void load_counted(hipStream_t s, const float* d_xyzi, int n) { launch_deinterleave(s, d_xyzi, n, in()); }
    int filter(hipStream_t s, int n, float leaf, const unsigned* ext_parts = nullptr, int n_parts = 0) {
        return vf.run(s, in(), d_n.p, n, leaf, 45, out(), d_n.p + 1, nullptr, ext_parts, n_parts);
    }
    void store(hipStream_t s, int n, float* d_xyzi) { launch_interleave(s, d_n.p + 1, n, out(), d_xyzi); }
    // reads the count and the filter's error word back and synchronises s: the number of centroids, or SCAL_E_CAPACITY ("<who>: ...")
    int wait(hipStream_t s, const char* who);
};

}  // namespace scal

namespace scal {
#ifdef __HIPCC__
// Bounding box without a launch of its own and without contended atomics: a kernel that reads a cloud anyway (a gather, the
// curvature pass) lets every 256-thread block store the box of ITS points (order-preserving uint images: min xyz, max xyz) in
// parts[block][6]; the filter's key kernel reduces the parts (VoxelFilter::run with ext_parts).  Every thread of the block calls
// it, also in blocks without points (they store the identity).  This form takes the box of the thread's points (lo / hi:
// order-preserving images, identity 0xffffffff / 0 for none); the one below a single point, `have` = this thread holds one.
__device__ inline void vox_bbox_block_store(unsigned* parts, int block, unsigned lo[3], unsigned hi[3]) {
    __shared__ unsigned s_box[4][6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], static_cast<unsigned>(__shfl_xor(static_cast<int>(lo[a]), o, 64)));
            hi[a] = max(hi[a], static_cast<unsigned>(__shfl_xor(static_cast<int>(hi[a]), o, 64)));
        }
        if ((threadIdx.x & 63) == 0) s_box[threadIdx.x >> 6][a] = lo[a], s_box[threadIdx.x >> 6][3 + a] = hi[a];
    }
    __syncthreads();
    if (threadIdx.x < 3)
        parts[block * 6 + threadIdx.x] = min(min(s_box[0][threadIdx.x], s_box[1][threadIdx.x]), min(s_box[2][threadIdx.x], s_box[3][threadIdx.x]));
    else if (threadIdx.x < 6)
        parts[block * 6 + threadIdx.x] = max(max(s_box[0][threadIdx.x], s_box[1][threadIdx.x]), max(s_box[2][threadIdx.x], s_box[3][threadIdx.x]));
}
__device__ __forceinline__ unsigned vox_ordered(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline void vox_bbox_block_store(unsigned* parts, int block, bool have, float x, float y, float z) {
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (have) {
        lo[0] = hi[0] = vox_ordered(x);
        lo[1] = hi[1] = vox_ordered(y);
        lo[2] = hi[2] = vox_ordered(z);
    }
    vox_bbox_block_store(parts, block, lo, hi);
}
#endif
}  // namespace scal
