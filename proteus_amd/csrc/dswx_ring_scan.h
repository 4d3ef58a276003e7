// dswx_ring_scan.h -- the second launch of the burn (dswx_burn.hip) and of the reach (dswx_reach.hip): a prefix along every row
// of `acc` in place -- XOR for the burn's toggles, SUM for the reach's differences --, fused with the write of `mask` and the count
// of the pixels with acc != 0.  The two kernels are this one body with another operation; the arguments of both entries are one
// struct, so that the first launches read the same fields.
//
// All rows of all tiles are numbered through; a workgroup takes a run of them, its four waves a row each in turn (so that tiles
// of a few pixels are not a launch's worth of work each).  A wave walks its row in steps of 256 pixels: 16 bytes of `acc` per
// lane from a 16-byte aligned address, a prefix in registers, one across the lanes, the running value carried from step to
// step.  A row begins wherever it begins (width 129): the slot that holds its first pixels and the one that holds its last are
// read and written pixel by pixel, so nothing outside the row is ever read.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "dswx_host.h"

namespace {

typedef u32x4 __attribute__((aligned(16))) ring_u32x4;

constexpr int RING_BLOCK = 256;
constexpr int RING_WAVES = RING_BLOCK / 64;
constexpr int RING_HEAD_WORDS = 8;                       // of both entries
constexpr int RING_HEAD_PIXELS = 6;                      // the head word that this launch counts

struct RingArgs {
    const ring_u32x4* verts;
    const long long* tile_first;
    unsigned* acc;
    unsigned char* mask;                                 // nullptr: not wanted
    const unsigned char* src;                            // nullptr: the background
    unsigned long long* head;                            // nullptr: not wanted
    long long n_tiles, height, width;
    unsigned long long n_elems;                          // height * width <= 2^30
    unsigned long long mask_stride, src_stride;
    unsigned burn, background;
    unsigned long long total_rows, rows_per_block;       // the scan launch
};

struct RingXor {                                         // join(a, b); without(join(a, b), b) == a
    static __device__ __forceinline__ unsigned join(unsigned a, unsigned b) { return a ^ b; }
    static __device__ __forceinline__ unsigned without(unsigned a, unsigned b) { return a ^ b; }
};
struct RingSum {
    static __device__ __forceinline__ unsigned join(unsigned a, unsigned b) { return a + b; }
    static __device__ __forceinline__ unsigned without(unsigned a, unsigned b) { return a - b; }
};

__device__ __forceinline__ unsigned ring_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ void ring_flush_pixels(const RingArgs& a, long long t, unsigned* pixels, unsigned lane) {
    const unsigned sum = ring_wave_sum(*pixels);
    *pixels = 0u;
    if (a.head && sum && lane == 0u) atomicAdd(a.head + (unsigned long long)t * RING_HEAD_WORDS + RING_HEAD_PIXELS, (unsigned long long)sum);
}

template <class Op>
__device__ __forceinline__ void ring_scan(const RingArgs& a) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long block_first = (unsigned long long)blockIdx.x * a.rows_per_block;
    unsigned long long block_end = block_first + a.rows_per_block;
    if (block_end > a.total_rows) block_end = a.total_rows;
    unsigned long long R = block_first + wave;           // (the same for the lanes of a wave, like everything that follows from it)
    if (R >= block_end) return;
    long long t = (long long)(R / (unsigned long long)a.height), r = (long long)(R - (unsigned long long)t * (unsigned long long)a.height);
    const unsigned burn = a.burn, burn4 = burn * 0x01010101u;
    unsigned pixels = 0;
    for (; R < block_end; R += RING_WAVES) {
        unsigned* const row = a.acc + (unsigned long long)t * a.n_elems + (unsigned long long)(r * a.width);
        unsigned char* const mrow = a.mask ? a.mask + (unsigned long long)t * a.mask_stride + (unsigned long long)(r * a.width) : nullptr;
        const unsigned char* const srow = a.src ? a.src + (unsigned long long)t * a.src_stride + (unsigned long long)(r * a.width) : nullptr;
        // slot k holds the columns 4 k - off .. 4 k - off + 3: its first pixel lies at a multiple of 16 bytes
        const long long off = (long long)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u);
        const long long slots = (a.width + off + 3) >> 2;
        // the four bytes of a whole slot in `mask` and `src` as one word: when they begin at a multiple of 4 bytes
        const bool mask_words = ((reinterpret_cast<uintptr_t>(mrow) - (uintptr_t)off) & 3u) == 0u &&
                                (!srow || ((reinterpret_cast<uintptr_t>(srow) - (uintptr_t)off) & 3u) == 0u);
        unsigned carry = 0;                              // the row's pixels before this step, joined
        for (long long s0 = 0; s0 < slots; s0 += 64) {
            const long long c0 = 4 * (s0 + lane) - off;
            const bool whole = c0 >= 0 && c0 + 4 <= a.width;                  // else: the head or the tail of the row, or behind it
            u32x4 v = {0u, 0u, 0u, 0u};
            if (whole)
                v = *reinterpret_cast<const ring_u32x4*>(row + c0);
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j >= 0 && c0 + j < a.width) v[j] = row[c0 + j];
            }
            v.y = Op::join(v.y, v.x), v.z = Op::join(v.z, v.y), v.w = Op::join(v.w, v.z);
            unsigned inc = v.w;                          // the inclusive prefix of the lanes' totals
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned u = __shfl_up(inc, o);
                if (lane >= (unsigned)o) inc = Op::join(inc, u);
            }
            const unsigned before = Op::join(carry, Op::without(inc, v.w));
            v.x = Op::join(v.x, before), v.y = Op::join(v.y, before), v.z = Op::join(v.z, before), v.w = Op::join(v.w, before);
            carry = Op::join(carry, __shfl(inc, 63));
            if (whole) {
                *reinterpret_cast<ring_u32x4*>(row + c0) = v;
                pixels += (v.x != 0u) + (v.y != 0u) + (v.z != 0u) + (v.w != 0u);
                if (mrow) {
                    if (mask_words) {
                        const unsigned other = srow ? *reinterpret_cast<const unsigned*>(srow + c0) : a.background * 0x01010101u;
                        const unsigned set = (v.x ? 0xFFu : 0u) | (v.y ? 0xFF00u : 0u) | (v.z ? 0xFF0000u : 0u) | (v.w ? 0xFF000000u : 0u);
                        *reinterpret_cast<unsigned*>(mrow + c0) = (burn4 & set) | (other & ~set);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) mrow[c0 + j] = (unsigned char)(v[j] ? burn : srow ? (unsigned)srow[c0 + j] : a.background);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j >= 0 && c0 + j < a.width) {
                        row[c0 + j] = v[j];
                        pixels += v[j] != 0u;
                        if (mrow) mrow[c0 + j] = (unsigned char)(v[j] ? burn : srow ? (unsigned)srow[c0 + j] : a.background);
                    }
            }
        }
        r += RING_WAVES;
        while (r >= a.height) {                          // (uniform) the next row of this wave lies in another tile
            ring_flush_pixels(a, t, &pixels, lane);
            r -= a.height;
            ++t;
        }
    }
    ring_flush_pixels(a, t, &pixels, lane);              // (t may be n_tiles here: nothing is left to add then)
}

}  // namespace
