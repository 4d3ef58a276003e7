// dswx_outline_rule.h -- what the kernels and the host entry of dswx_outline.hip both state about an outline
// (include/dswx_hip.h "outline"): compiled for both sides, so the two cannot differ.
#pragma once
#include <cstdint>

#include "dswx_hip.h"

namespace {

// The pixels, and later the edges, of a tile that one workgroup scans (256 threads of 16) and the partials that the scan
// launches take per step: the constants of dswx_body_rule.h, repeated here so that this header stands alone (dswx_outline.hip
// asserts that they are equal).
constexpr int DSWX_OUTLINE_CHUNK = 4096;
constexpr int DSWX_OUTLINE_SCAN_STEP = 256;

// the words of a row (area2 is an int64 at words 6 - 7) and of the head
constexpr int OUTLINE_ID = 0, OUTLINE_START = 1, OUTLINE_OFFSET = 2, OUTLINE_LENGTH = 3, OUTLINE_CORNERS = 4, OUTLINE_AREA2 = 6;
constexpr int OUTLINE_HEAD_E = 0, OUTLINE_HEAD_R = 1, OUTLINE_HEAD_ROWS = 2, OUTLINE_HEAD_WRITTEN = 3, OUTLINE_HEAD_OUTER = 4,
              OUTLINE_HEAD_HOLES = 5, OUTLINE_HEAD_CORNERS = 6, OUTLINE_HEAD_OVERFLOW = 7;

// The travel T[d] of edge d and the step O[d] across it, x right and y down: d = 0 top, 1 right, 2 bottom, 3 left.
__host__ __device__ __forceinline__ int outline_tx(unsigned d) { return (d == 0u) - (d == 2u); }
__host__ __device__ __forceinline__ int outline_ty(unsigned d) { return (d == 1u) - (d == 3u); }
__host__ __device__ __forceinline__ int outline_ox(unsigned d) { return outline_ty(d); }
__host__ __device__ __forceinline__ int outline_oy(unsigned d) { return -outline_tx(d); }

// ids[y * width + x] == v, false outside the tile; `Ids` reads one element by its index (the device a plain load, the host
// entry a load from any address).
template <typename Ids>
__host__ __device__ __forceinline__ bool outline_same(const Ids& ids, int64_t x, int64_t y, int64_t width, int64_t height, uint32_t v) {
    return x >= 0 && y >= 0 && x < width && y < height && ids((uint64_t)(y * width + x)) == v;
}

// The boundary edges of pixel (x, y) with the value v != 0: bit d is set when the neighbour across d is outside the tile or
// holds another value.
template <typename Ids>
__host__ __device__ __forceinline__ unsigned outline_mask(const Ids& ids, int64_t x, int64_t y, int64_t width, int64_t height, uint32_t v) {
    unsigned m = 0;
#pragma unroll
    for (unsigned d = 0; d < 4u; ++d)
        if (!outline_same(ids, x + outline_ox(d), y + outline_oy(d), width, height, v)) m |= 1u << d;
    return m;
}

// THE SUCCESSOR of the boundary edge d of pixel (x, y) with the value v: the pixel and the direction of the edge that follows.
struct OutlineEdge {
    int64_t x, y;
    unsigned d;
};
template <typename Ids>
__host__ __device__ __forceinline__ OutlineEdge outline_succ(const Ids& ids, int64_t x, int64_t y, unsigned d, int64_t width,
                                                             int64_t height, uint32_t v, int connectivity) {
    const int64_t ax = x + outline_tx(d), ay = y + outline_ty(d);            // ahead on the region's side
    const int64_t bx = ax + outline_ox(d), by = ay + outline_oy(d);          // ahead on the other side
    const bool a = outline_same(ids, ax, ay, width, height, v), b = outline_same(ids, bx, by, width, height, v);
    const OutlineEdge right = {x, y, (d + 1u) & 3u}, straight = {ax, ay, d}, left = {bx, by, (d + 3u) & 3u};
    if (connectivity == 4) return !a ? right : !b ? straight : left;
    return b ? left : a ? straight : right;
}

// x1 * y2 - x2 * y1 of the edge d of pixel (x, y), corner 1 its start and corner 2 its end: for a unit step along an axis
// that is one coordinate, signed.
__host__ __device__ __forceinline__ int64_t outline_area2(int64_t x, int64_t y, unsigned d) {
    return d == 0u ? -y : d == 1u ? x + 1 : d == 2u ? y + 1 : -x;
}

}  // namespace
