// Host-side plumbing shared by every stage of libscaloam_hip.so: error reporting, RAII device/pinned buffers.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <string>
#include <vector>
#include <utility>
#include <mutex>
#include "../../include/scaloam_hip.h"
#include "batch.hpp"

namespace scal {
// Flags of events that only order streams of the same device against each other (nobody on the host reads memory behind them): no
// system-scope fence when the event completes.  Recording a default event behind a kernel writes the caches back for the host's
// sake; on the pipeline's chains that was several microseconds per record, several records per chain and scan.
constexpr unsigned EV_DEVICE_ONLY = hipEventDisableTiming | hipEventDisableSystemFence;


void set_error(const char* fmt, ...);

#define SCAL_HIP(expr)                                                                         \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            ::scal::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return SCAL_E_HIP;                                                                 \
        }                                                                                      \
    } while (0)

#define SCAL_TRY(expr)           \
    do {                         \
        int _rc = (expr);        \
        if (_rc != SCAL_OK) return _rc; \
    } while (0)

// selects the device and verifies it is a gfx950 part: the product path must fail loudly otherwise
int select_device(int device);
// Streams are shared per device and reference counted (held through LaneStream).  Lane 0 is the pipeline's in-order stream.  A stage
// context's lane follows the StreamLayout it is created with (the public scal_*_create take scal_set_stream_mode's, once, at entry):
// - Shared: stages A -> B -> C of a scan all run on lane 0, strictly dependent, no cross-stream events.  Lanes 1 and 2 carry work
//   that only depends on stage A (1: ScanContext with scal_sc_config::side_stream, 2: scal_map_prefetch_features).
// - PerStage (scal_pipeline_create): every stage gets its own stream - A: 0, D: 1, C prefetch: 2, B: 3, C: 4, folded onto four lanes
//   by stage_lane - so that consecutive scans overlap the way the reference's four ROS nodes do; every hand-over between contexts
//   is ordered by events in both directions (features_wait_done / features_note_reader).
// Lane 5 is free for a context that must not queue behind another one of its kind (scal_sc_config::side_stream = 5: the sharded
// database next to the descriptor builder, bench.py --gpus N).
enum class StreamLayout { Shared, PerStage };
enum { STAGE_FEATURES = 0, STAGE_SC = 1, STAGE_ODOM = 3, STAGE_MAP = 4, STAGE_MAP_PREFETCH = 2, STAGE_SC_FILTER = 5 };
int stage_lane(StreamLayout layout, int stage);
StreamLayout default_stream_layout();
int acquire_stream(int device, hipStream_t* out, int lane = 0);
void release_stream(int device, int lane = 0);
// scal_odom_create / scal_map_create / scal_sc_create with an explicit layout
int odom_create(const scal_odom_config* cfg, StreamLayout layout, scal_odom_t** out);
int map_create(const scal_map_config* cfg, StreamLayout layout, scal_map_t** out);
int sc_create(const scal_sc_config* cfg, StreamLayout layout, scal_sc_t** out);
// scal_icp_create on a given lane (scal_pipeline's loop verification keeps off the four busy lanes)
int icp_create_on_lane(const scal_icp_config* cfg, int lane, scal_icp_t** out);
// scal_refine_create on a given lane
int refine_create_on_lane(const scal_refine_config* cfg, int lane, scal_refine_t** out);
// scal_posegraph_create on a given lane (scal_pipeline_optimize_keyframes solves on the pose-graph map's lane)
int posegraph_create_on_lane(const scal_posegraph_config* cfg, int lane, scal_posegraph_t** out);
// scal_sc_insert_features with a hook queued on the ScanContext stream behind the descriptor and before the next keyframe filter may
// overwrite the 0.4 m filter output: after(stream, x, y, z, intensity, device count, capacity) (scal_pipeline's keyframe store)
struct ScFilterOut {
    const float *x, *y, *z, *w;
    const int* d_n;
    int cap;
};
int sc_insert_features_then(scal_sc_t* ctx, scal_features_t* feat, int (*after)(void* user, hipStream_t s, const ScFilterOut& ds), void* user);

// makeScancontext of a cloud in device memory (SoA planes, *d_n <= n_max points) into d_desc (1200 doubles, column-major, device
// memory), not inserted; queued on the ScanContext stream, nothing is waited for (scal_reloc's query descriptor)
int sc_make_cloud_device(scal_sc_t* ctx, const float* d_x, const float* d_y, const float* d_z, const int* d_n, int n_max, double* d_desc);

// Owning handles in the style of DevBuf (move-only): one reference to a shared stream, released when the handle goes away ...
struct LaneStream {
    hipStream_t s = nullptr;
    int device = 0, lane = 0;
    LaneStream() = default;
    LaneStream(LaneStream&& o) noexcept { *this = std::move(o); }
    LaneStream& operator=(LaneStream&& o) noexcept {
        release();
        std::swap(s, o.s);
        device = o.device, lane = o.lane;
        return *this;
    }
    ~LaneStream() { release(); }
    operator hipStream_t() const { return s; }
    int acquire(int dev, int ln) {
        release();
        device = dev, lane = ln;
        return acquire_stream(dev, &s, ln);
    }
    void release() {
        if (s) release_stream(device, lane);
        s = nullptr;
    }
};
// ... and an event, destroyed with its handle; ensure() creates the ones a context only needs once it is used in a particular way
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept { *this = std::move(o); }
    Event& operator=(Event&& o) noexcept {
        reset();
        std::swap(e, o.e);
        return *this;
    }
    ~Event() { reset(); }
    operator hipEvent_t() const { return e; }
    int create(unsigned flags) {
        reset();
        return ensure(flags);
    }
    int ensure(unsigned flags) {
        const hipError_t r = e ? hipSuccess : hipEventCreateWithFlags(&e, flags);
        if (r == hipSuccess) return SCAL_OK;
        set_error("hipEventCreateWithFlags failed: %s", hipGetErrorString(r));
        e = nullptr;
        return SCAL_E_HIP;
    }
    void reset() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
};

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    int alloc(size_t count) {
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
        if (e != hipSuccess) {
            set_error("hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
            p = nullptr;
            return SCAL_E_HIP;
        }
        n = count;
        return SCAL_OK;
    }
    int zero(hipStream_t s) {
        hipError_t e = op_memset_async(p, 0, n * sizeof(T), s);
        if (e != hipSuccess) {
            set_error("hipMemsetAsync failed: %s", hipGetErrorString(e));
            return SCAL_E_HIP;
        }
        return SCAL_OK;
    }
};

template <class T>
struct PinBuf {
    T* p = nullptr;
    size_t n = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() {
        if (p) (void)hipHostFree(p);
    }
    int alloc(size_t count) {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        if (count == 0) count = 1;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) {
            set_error("hipHostMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
            p = nullptr;
            return SCAL_E_HIP;
        }
        n = count;
        return SCAL_OK;
    }
};

inline int div_up(int a, int b) { return (a + b - 1) / b; }

// Host arrays of the synchronous entry points are the caller's (pageable) memory: a copy straight to or from them is staged by the
// runtime in small synchronous pieces.  This keeps one pinned area per context instead: downloads land there with ONE asynchronous
// copy each and are handed to the caller's arrays after the stream has been synchronised; uploads are copied in first.
struct HostStage {
    PinBuf<unsigned char> pin;
    size_t used = 0;
    struct Item {
        void* dst;
        size_t off, bytes;
    };
    std::vector<Item> items;
    // the staging area holds `total` bytes from now on (only grows while nothing is pending); false: no memory, callers copy directly
    bool reserve(size_t total) {
        if (pin.p && pin.n >= total) return true;
        if (used) return false;
        if (pin.alloc(total) != SCAL_OK) {
            (void)hipGetLastError();
            return false;
        }
        return true;
    }
    hipError_t d2h(void* user, const void* dev, size_t bytes, hipStream_t s) {
        if (!bytes) return hipSuccess;
        const size_t need = (bytes + 255) & ~static_cast<size_t>(255);
        if (!pin.p || used + need > pin.n) return hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, s);
        const hipError_t e = hipMemcpyAsync(pin.p + used, dev, bytes, hipMemcpyDeviceToHost, s);
        items.push_back({user, used, bytes});
        used += need;
        return e;
    }
    hipError_t h2d(void* dev, const void* user, size_t bytes, hipStream_t s) {
        if (!bytes) return hipSuccess;
        const size_t need = (bytes + 255) & ~static_cast<size_t>(255);
        if (!pin.p || used + need > pin.n) return hipMemcpyAsync(dev, user, bytes, hipMemcpyHostToDevice, s);
        std::memcpy(pin.p + used, user, bytes);
        const hipError_t e = hipMemcpyAsync(dev, pin.p + used, bytes, hipMemcpyHostToDevice, s);
        used += need;
        return e;
    }
    // the stream the copies were queued on has been synchronised: deliver the downloads, the area is free again
    void finish() {
        for (const Item& it : items) std::memcpy(it.dst, pin.p + it.off, it.bytes);
        items.clear();
        used = 0;
    }
};

// Optional per-kernel timing (bench.py's roofline leg).  The start/stop events are attached to the kernel's own dispatch
// (hipExtLaunchKernelGGL), so they read the dispatch's begin/end timestamps and put no extra packet on the stream: separate
// hipEventRecord calls cost ~5 us of stream time each, more than many of the kernels they would bracket.
// Disabled by default: SCAL_LAUNCH_PROF is then one branch + a plain launch.
bool prof_begin(const char* name, hipStream_t stream, hipEvent_t* start, hipEvent_t* stop);

#define SCAL_LAUNCH_PROF(name, kernel, grid, block, lds, stream, ...)                                   \
    do {                                                                                                \
        hipEvent_t pe0_ = nullptr, pe1_ = nullptr;                                                      \
        if (::scal::prof_begin(name, stream, &pe0_, &pe1_))                                                     \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, pe0_, pe1_, 0, __VA_ARGS__);        \
        else                                                                                            \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                          \
    } while (0)

}  // namespace scal
