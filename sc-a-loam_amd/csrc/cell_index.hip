// The host half of the sparse cell index and its two kernels (cell_index.hpp has the format and the device lookup).
// build: table clear -> keys -> RadixSort (stable, 48-bit keys) -> index, one launch chain on the caller's stream.
#include "cell_index.hpp"
#include <algorithm>

namespace scal {

// a point is in a cell when |v| < bound on every axis: +inf admits every finite point, NaN is in no cell under any bound
__global__ void __launch_bounds__(256) k_ci_keys(const float4* __restrict__ pts, int n, float inv, float bound, unsigned long long* __restrict__ keys,
                                                 int* __restrict__ vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    unsigned long long key = CH_NO_CELL;
    if (fabsf(p.x) < bound && fabsf(p.y) < bound && fabsf(p.z) < bound)
        key = ch_key(ch_clamp_coord(p.x * inv, CH_XB), ch_clamp_coord(p.y * inv, CH_XB), ch_clamp_coord(p.z * inv, CH_ZB));
    keys[i] = key;
    vals[i] = i;
}

// sorted position i is the first (head) and / or the last (tail) of cell `key`: enters that end of the cell's range (find-or-insert
// by compare-and-swap; which of the two ends arrives first does not matter)
__device__ __forceinline__ void ch_insert(unsigned long long* __restrict__ hkeys, int2* __restrict__ hrange, unsigned mask, unsigned long long key,
                                          int i, bool head, bool tail) {
    unsigned slot = ch_slot(key, mask);
    for (;;) {  // the table has at least twice as many slots as there are points
        const unsigned long long prev = atomicCAS(&hkeys[slot], CH_EMPTY, key);
        if (prev == CH_EMPTY || prev == key) break;
        slot = (slot + 1) & mask;
    }
    if (head) hrange[slot].x = i;
    if (tail) hrange[slot].y = i + 1;
}

// sorted position i: the point itself with its input position in .w; the first and the last position of a cell enter the cell's
// range into the hash table
__global__ void __launch_bounds__(256) k_ci_index(const unsigned long long* __restrict__ keys, const int* __restrict__ vals, int n,
                                                  const float4* __restrict__ pts, float4* __restrict__ sorted, unsigned long long* __restrict__ hkeys,
                                                  int2* __restrict__ hrange, unsigned mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    const int idx = vals[i];
    float4 p = pts[idx];
    p.w = __int_as_float(idx);
    sorted[i] = p;
    if (key == CH_NO_CELL) return;
    const bool head = i == 0 || keys[i - 1] != key, tail = i == n - 1 || keys[i + 1] != key;
    if (!head && !tail) return;
    ch_insert(hkeys, hrange, mask, key, i, head, tail);
}

int SparseCells::init(int max_index_points, int max_sort_points) {
    const size_t ni = static_cast<size_t>(max_index_points), ns = static_cast<size_t>(std::max(max_index_points, max_sort_points));
    size_t slots = 1024;
    while (slots < 2 * ni) slots <<= 1;
    mask = static_cast<unsigned>(slots - 1);
    SCAL_TRY(hkeys.alloc(slots));
    SCAL_TRY(hrange.alloc(slots));
    SCAL_TRY(sorted.alloc(ni));
    SCAL_TRY(keys.alloc(ns));
    SCAL_TRY(vals.alloc(ns));
    SCAL_TRY(d_n.alloc(1));
    return sorter.init(static_cast<int>(ns));
}

int SparseCells::sort(hipStream_t s, const float4* pts, int n, SortedPairs* sp) {
    SCAL_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_n.p), n, 1, s));  // no host memory behind it: nothing to keep alive, no wait
    if (n_keys.empty())
        hipLaunchKernelGGL(k_ci_keys, dim3(div_up(n, 256)), dim3(256), 0, s, pts, n, inv, bound, keys.p, vals.p);
    else
        SCAL_LAUNCH_PROF(n_keys.c_str(), k_ci_keys, dim3(div_up(n, 256)), dim3(256), 0, s, pts, n, inv, bound, keys.p, vals.p);
    SCAL_HIP(hipGetLastError());
    return sorter.sort(s, keys.p, vals.p, d_n.p, n, CH_KEY_BITS, nullptr, sp);
}

int SparseCells::build(hipStream_t s, const float4* pts, int n, float inv_cell, float finite_bound) {
    inv = inv_cell, bound = finite_bound;
    SCAL_HIP(hipMemsetAsync(hkeys.p, 0xff, sizeof(unsigned long long) * (static_cast<size_t>(mask) + 1), s));
    if (n == 0) return SCAL_OK;
    SortedPairs sp;
    SCAL_TRY(sort(s, pts, n, &sp));
    SCAL_LAUNCH_PROF(n_index.c_str(), k_ci_index, dim3(div_up(n, 256)), dim3(256), 0, s, sp.keys[sp.fixed_sel], sp.vals[sp.fixed_sel], n, pts, sorted.p,
                     hkeys.p, hrange.p, mask);
    SCAL_HIP(hipGetLastError());
    return SCAL_OK;
}

}  // namespace scal
