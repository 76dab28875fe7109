// Sparse cell index over a point array (nbr.hip's radius index, refine.hip's round target): a point's 48-bit key is made of three
// clamped cell coordinates, the points are sorted by it (stable radix sort), and the cells' [start, end) ranges of the sorted array
// sit behind an open-addressing hash table in HBM.  The format is decided here and nowhere else: the 17/17/14 bit split, the all-ones
// key of a point in no cell, a table of at least twice as many slots as points that is empty where its bytes are 0xff, and the head /
// tail insertion.  SparseCells is the host half (cell_index.hip has its two kernels), CellView what a kernel takes of it.
// A cell coordinate is floor(v * inv) in f32: inv is a power of two for nbr.hip (a cell that follows the radius) and 1 for
// refine.hip's 1 m cell, so the product is exact either way.
#pragma once
#include "common.hpp"
#include "radix_sort.hpp"
#include <string>

namespace scal {

// cell coordinates: 17 bits in x and y, 14 in z, clamped beyond.  Clamping is monotone: cells that differ by k stay within k.
constexpr int CH_XB = 17, CH_ZB = 14, CH_KEY_BITS = 2 * CH_XB + CH_ZB;
constexpr unsigned long long CH_NO_CELL = (1ull << CH_KEY_BITS) - 1;  // a point in no cell: sorted behind every cell, never in the table
constexpr unsigned long long CH_EMPTY = ~0ull;                        // a free slot (the table is filled with 0xff bytes)

// a float already in cell units -> its cell coordinate, clamped to the `bits`-bit range; NaN -> the lowest cell
__device__ __forceinline__ int ch_clamp_coord(float cells, int bits) {
    const float lim = static_cast<float>(1 << (bits - 1));
    return static_cast<int>(fminf(fmaxf(floorf(cells), -lim), lim - 2.f));
}
// key of cell (x, y, z); CH_NO_CELL outside the coordinate range (nothing is stored there)
__device__ __forceinline__ unsigned long long ch_key(int x, int y, int z) {
    const int bx = x + (1 << (CH_XB - 1)), by = y + (1 << (CH_XB - 1)), bz = z + (1 << (CH_ZB - 1));
    if (static_cast<unsigned>(bx) >= (1u << CH_XB) - 1 || static_cast<unsigned>(by) >= (1u << CH_XB) - 1 || static_cast<unsigned>(bz) >= (1u << CH_ZB) - 1)
        return CH_NO_CELL;
    return (static_cast<unsigned long long>(bz) << (2 * CH_XB)) | (static_cast<unsigned long long>(by) << CH_XB) | static_cast<unsigned long long>(bx);
}
__device__ __forceinline__ unsigned ch_slot(unsigned long long key, unsigned mask) {
    unsigned long long h = key * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    return static_cast<unsigned>(h) & mask;
}

// What a kernel takes of an index, by value: the table, the points in cell order (their input position in .w) and the cell width.
struct CellView {
    const unsigned long long* hkeys;
    const int2* hrange;
    const float4* sorted;
    unsigned mask;
    float inv;  // 1 / cell width
    __device__ __forceinline__ int cx(float v) const { return ch_clamp_coord(v * inv, CH_XB); }  // the same for y
    __device__ __forceinline__ int cz(float v) const { return ch_clamp_coord(v * inv, CH_ZB); }
    // the points of cell (x, y, z) are sorted[range.x .. range.y); false: no such cell
    __device__ __forceinline__ bool find(int x, int y, int z, int2& range) const {
        const unsigned long long key = ch_key(x, y, z);
        if (key == CH_NO_CELL) return false;
        unsigned slot = ch_slot(key, mask);
        for (;;) {
            const unsigned long long hk = hkeys[slot];
            if (hk == key) {
                range = hrange[slot];
                return true;
            }
            if (hk == CH_EMPTY) return false;
            slot = (slot + 1) & mask;
        }
    }
};

struct SparseCells {
    unsigned mask = 0;
    float inv = 0.f, bound = 0.f;  // of the last build: a point is in a cell when |v| < bound on every axis (NaN: in none)
    DevBuf<unsigned long long> hkeys, keys;
    DevBuf<int2> hrange;
    DevBuf<float4> sorted;
    DevBuf<int> vals, d_n;  // d_n: the sorter's device count
    RadixSort sorter;
    // names under which the two launches are timed (scal_prof_*), see RadixSort::set_tag; without a name for it the key kernel is not timed
    std::string n_keys, n_index = "k_ci_index";
    void set_names(const char* keys_name, const char* index_name) { n_keys = keys_name ? keys_name : "", n_index = index_name; }

    // an index of up to max_index_points; sort() takes up to max(max_index_points, max_sort_points)
    int init(int max_index_points, int max_sort_points);
    // the keys of the n points at pts (cell width and bound of the last build), sorted: the pairs are in *sp afterwards
    int sort(hipStream_t s, const float4* pts, int n, SortedPairs* sp);
    // clears the table and indexes the n points at pts, all on s and without waiting: pts is still being read when this returns
    int build(hipStream_t s, const float4* pts, int n, float inv_cell, float finite_bound);
    CellView view() const { return CellView{hkeys.p, hrange.p, sorted.p, mask, inv}; }
};

}  // namespace scal
