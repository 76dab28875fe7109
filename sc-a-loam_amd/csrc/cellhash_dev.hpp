// Sparse cell index shared by refine.hip and nbr.hip: a 48-bit key of three clamped cell coordinates, and the cells' [start, end)
// ranges of a key-sorted point array behind an open-addressing hash table in HBM (at least twice as many slots as points).  How a
// coordinate comes out of a float is the user's (refine.hip: floorf of a 1 m cell; nbr.hip: a power-of-two cell that follows the radius).
#pragma once
#include <hip/hip_runtime.h>

namespace scal {

constexpr unsigned long long CH_EMPTY = ~0ull;  // a free slot (the table is filled with 0xff bytes)

// a float already in cell units -> its cell coordinate, clamped to the `bits`-bit range (monotone); NaN -> the lowest cell
__device__ __forceinline__ int ch_clamp_coord(float cells, int bits) {
    const float lim = static_cast<float>(1 << (bits - 1));
    return static_cast<int>(fminf(fmaxf(floorf(cells), -lim), lim - 2.f));
}
// key of cell (x, y, z) with XB bits in x and y and ZB in z; all ones (in no cell: nothing is stored there) outside the range
template <int XB, int ZB>
__device__ __forceinline__ unsigned long long ch_key(int x, int y, int z) {
    const int bx = x + (1 << (XB - 1)), by = y + (1 << (XB - 1)), bz = z + (1 << (ZB - 1));
    if (static_cast<unsigned>(bx) >= (1u << XB) - 1 || static_cast<unsigned>(by) >= (1u << XB) - 1 || static_cast<unsigned>(bz) >= (1u << ZB) - 1)
        return (1ull << (2 * XB + ZB)) - 1;
    return (static_cast<unsigned long long>(bz) << (2 * XB)) | (static_cast<unsigned long long>(by) << XB) | static_cast<unsigned long long>(bx);
}
__device__ __forceinline__ unsigned ch_slot(unsigned long long key, unsigned mask) {
    unsigned long long h = key * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    return static_cast<unsigned>(h) & mask;
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
// the range of cell `key`; false: no such cell
__device__ __forceinline__ bool ch_find(const unsigned long long* __restrict__ hkeys, const int2* __restrict__ hrange, unsigned mask,
                                        unsigned long long key, int2& range) {
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

}  // namespace scal
