// dswx_grid_rule.h -- the per-byte and per-cell rule of a grid (include/dswx_hip.h "grid"), the ONE definition that the
// kernel and the host entry of dswx_grid.hip share: compiled for both sides, so the two cannot differ.
#pragma once
#include <cstdint>

#include "dswx_hip.h"

namespace {

// What one byte adds to the packed counters of a run of pixels: four 8-bit fields in one uint32, field k = count[k].  A byte
// whose category is not below n_cats adds nothing -- and "adds nothing" IS "not an observation".  A field holds at most 255:
// whoever sums increments widens (grid_field into a uint32 per category) after at most GRID_PACKED_MAX bytes.
constexpr unsigned GRID_PACKED_MAX = 255;
__host__ __device__ __forceinline__ uint32_t grid_increment(const uint8_t* cat_of_byte, int n_cats, unsigned byte) {
    const unsigned c = cat_of_byte[byte & 0xffu];
    return c < (unsigned)n_cats ? 1u << (8u * c) : 0u;
}
__host__ __device__ __forceinline__ uint32_t grid_field(uint32_t packed, int k) { return (packed >> (8 * k)) & 0xffu; }

// The derived values of a cell from its four counts (those of the categories that do not exist are zero) and the number of
// pixels it covers.  100 * count fits 32 bits because a cell has at most DSWX_GRID_MAX_CELL_PIXELS = 2^24 pixels.
__host__ __device__ __forceinline__ uint32_t grid_n_obs(const uint32_t (&count)[DSWX_GRID_MAX_CATS]) {
    return count[0] + count[1] + count[2] + count[3];
}
__host__ __device__ __forceinline__ unsigned grid_share(const uint32_t (&count)[DSWX_GRID_MAX_CATS]) {
    const uint32_t n_obs = grid_n_obs(count);
    return n_obs ? (100u * count[0]) / n_obs : (unsigned)DSWX_GRID_NO_SHARE;
}
__host__ __device__ __forceinline__ unsigned grid_coverage(const uint32_t (&count)[DSWX_GRID_MAX_CATS], uint32_t n_pix) {
    return (100u * grid_n_obs(count)) / n_pix;
}
// the smallest k whose count is the largest: a later category replaces an earlier one only when it is strictly larger
__host__ __device__ __forceinline__ unsigned grid_major(const uint32_t (&count)[DSWX_GRID_MAX_CATS]) {
    if (!grid_n_obs(count)) return (unsigned)DSWX_GRID_NONE;
    unsigned best = 0;
    uint32_t top = count[0];
#pragma unroll
    for (unsigned k = 1; k < DSWX_GRID_MAX_CATS; ++k)
        if (count[k] > top) {
            top = count[k];
            best = k;
        }
    return best;
}

}  // namespace
