// dswx_distance_rule.h -- the per-pixel rule, the summary key and the geometry of a distance transform (include/dswx_hip.h
// "distance"), the ONE definition that the kernels and the host entry of dswx_distance.hip share: compiled for both sides,
// so the two cannot differ.
#pragma once
#include <cstdint>

#include "dswx_hip.h"
#include "dswx_label_rule.h"           // the 256-bit fold of a byte table: label_member_bits / label_is_member

namespace {

// The geometry of the launches (dswx_distance.hip).  Published so that tests can build shapes around the seams;
// proteus_amd/_capi.py mirrors them.
constexpr int DSWX_DISTANCE_BAND_H = 64;                 // rows of a column-pass thread: the targets of a band are ONE 64-bit word per column
constexpr int DSWX_DISTANCE_COLS = 4;                    // adjacent columns of a column-pass thread = bytes of its load
constexpr int DSWX_DISTANCE_BLOCK_W = 64;                // columns of a block of the row pass: one wave, one minimum per block
constexpr int DSWX_DISTANCE_NEAR = 32;                   // the row pass looks this far to either side before it turns to the blocks

// ---- the working format of dist2 between the column pass and the row pass ---------------------------------------------------
// bits 0 .. 16  dy = (row of the nearest target of the column) - y as 17-bit two's complement (|dy| <= 46339), ties upward;
// bit  17       no target of the column reaches this row (none at all, or only further than max_radius);
// bits 18 .. 30 ONLY in the first row of a band: the band's own targets in this column (has, bottom-most, top-most local
//               row).  The band launch writes them, the column launch reads them from OTHER bands while it rewrites its own
//               first row -- with the same thirteen bits, so a reader sees them whichever store it meets.
constexpr uint32_t DIST_DY_MASK = 0x1FFFFu;
constexpr uint32_t DIST_DY_NONE = 1u << 17;
__host__ __device__ __forceinline__ uint32_t dist_band_bits(bool has, unsigned top, unsigned bottom) {
    return has ? (1u << 30) | (bottom << 24) | (top << 18) : 0u;
}
__host__ __device__ __forceinline__ bool dist_band_has(uint32_t e) { return (e >> 30) & 1u; }
__host__ __device__ __forceinline__ unsigned dist_band_top(uint32_t e) { return (e >> 18) & 63u; }
__host__ __device__ __forceinline__ unsigned dist_band_bottom(uint32_t e) { return (e >> 24) & 63u; }
static_assert(DSWX_DISTANCE_BAND_H == 64, "a local row is six bits and the targets of a band one uint64");

// The entry of a pixel whose nearest target at or above is `up` rows away and at or below `down` rows (DIST_FAR: none): ties
// upward, and what max_radius cannot reach is dropped here already (d2 >= dy * dy).
constexpr uint32_t DIST_FAR = 0x7FFFFFFFu;
__host__ __device__ __forceinline__ uint32_t dist_entry(uint32_t up, uint32_t down, uint32_t max_radius) {
    const bool above = up <= down;
    const uint32_t d = above ? up : down;
    if (d == DIST_FAR || (max_radius && d > max_radius)) return DIST_DY_NONE;
    return (above ? 0u - d : d) & DIST_DY_MASK;
}
constexpr int32_t DIST_NO_DY = 0x7FFFFFFF;
__host__ __device__ __forceinline__ int32_t dist_entry_dy(uint32_t e) {
    return e & DIST_DY_NONE ? DIST_NO_DY : (int32_t)(e << 15) >> 15;
}

// The row pass compares candidates by (d2, column): the smaller d2, and on a tie the smaller column.  `limit` is what no
// accepted d2 reaches: max_radius^2 + 1, or DSWX_DISTANCE_NONE.
__host__ __device__ __forceinline__ uint32_t dist_limit(uint32_t max_radius) {
    return max_radius && (uint64_t)max_radius * max_radius < 0xFFFFFFFEull ? max_radius * max_radius + 1u : DSWX_DISTANCE_NONE;
}
// d2 of a candidate column dx away whose entry is dy (never DIST_NO_DY); fits because height, width <= 46340
__host__ __device__ __forceinline__ uint32_t dist_d2(uint32_t dx, int32_t dy) { return dx * dx + (uint32_t)(dy * dy); }

// within: a non-target pixel that a target reaches becomes `mark`; every other byte is copied.  (dist2 == 0 iff target.)
__host__ __device__ __forceinline__ unsigned dist_within(unsigned byte, uint32_t d2, unsigned mark) {
    return d2 != 0u && d2 != DSWX_DISTANCE_NONE ? mark : byte;
}

// summary word 8 + b counts the reached non-target pixels with floor(log2(dist2)) == b; dist2 >= 1
__host__ __device__ __forceinline__ int dist_size_bin(uint32_t d2) { return 31 - __builtin_clz(d2); }

// The largest dist2 of a reached pixel and, on a tie, the smallest pixel index, as ONE key whose maximum is
// order-independent: words 3 and 4 of the summary are dist_key_d2 / dist_key_idx of the maximum over the reached pixels; key 0
// = no pixel reached (an index is below 2^31, so the key of a pixel is never 0).
__host__ __device__ __forceinline__ uint64_t dist_key(uint32_t d2, uint32_t idx) { return ((uint64_t)d2 << 32) | (uint64_t)(0xFFFFFFFFu - idx); }
__host__ __device__ __forceinline__ uint64_t dist_key_d2(uint64_t key) { return key >> 32; }
__host__ __device__ __forceinline__ uint64_t dist_key_idx(uint64_t key) { return key ? (uint64_t)(0xFFFFFFFFu - (uint32_t)key) : 0u; }

}  // namespace
