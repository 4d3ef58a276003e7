// dswx_distance.hip -- the exact Euclidean distance of every pixel to the nearest target of a plane (DSWX_HAS_DISTANCE,
// additive to ABI v7): per pixel the squared distance and the index of the target that attains it, the ring of pixels within
// a radius, and a per-tile summary, without the plane crossing PCIe.  include/dswx_hip.h "distance" states the definition;
// proteus_amd/distance.py is its numpy statement and dswx_distance_host below the scalar one -- dswx_distance_rule.h is
// compiled for both sides.
//
// The first SEPARABLE SCAN here: a pixel depends on its whole column, then on its whole row.  min over targets of
// (dy^2 + dx^2) = min over columns x' of ((x - x')^2 + g(x')^2) with g(x') the vertical distance to the nearest target OF
// COLUMN x' -- so `dist2` is the working array: the column pass leaves the signed vertical offset in it (dist_entry), the row
// pass replaces it by the result, row by row, each row from its own entries only.
//
// NO WORKGROUP EVER WAITS FOR ANOTHER: no flag, no spin, no cooperative launch.  What depends on a whole phase is the next
// launch on the stream.  EVERY LOOP TERMINATES: a static trip count or a counter with a bound, stated at the loop.
//   1 ..column_k<false>      (only when the tile has more than one band.)  A thread owns 4 adjacent columns of a BAND of 64
//                             rows: one 4-byte load a row at any address, coalesced across the wave; the targets of a column of
//                             the band are the bits of ONE uint64.  It notes top-most and bottom-most target of the band in
//                             the spare bits of the band's FIRST row of dist2 (dist_band_bits) and writes nothing else.
//   2 ..column_k<true>       the same threads read the band again (it is in the Infinity Cache), find the nearest target
//                             above the band and below it by walking the NOTES of the other bands -- one word per band and
//                             column, never the plane, and no further than max_radius -- and write dist_entry for every row:
//                             nearest above from clz, nearest below from ctz of the column's word, else the carry.  The first
//                             row of a band keeps its note: the bits a neighbour may be reading hold the same value before and
//                             after the store (relaxed atomic accesses on both sides), so the order does not matter.
//   3 dswx_distance_row_k     a workgroup owns one row: its entries go to LDS (4 bytes a column), with the minimum |dy| of
//                             every BLOCK of 64 columns beside them.  A wave owns the 64 pixels of a block.  Each lane first
//                             looks outward, k = 1 .. 32 columns to either side while k^2 can still win (lane x reads
//                             ent[x - k]: consecutive banks, conflict-free); dense and noisy content ends here after a step or
//                             two.  Lanes that are still open then go through the BLOCKS that hold an entry, outward along two
//                             skip lists (so an empty row, or a row whose only entry is far away, costs nothing per empty
//                             block): a block whose (distance to the block)^2 + (its minimum)^2 cannot beat the lane's best
//                             is skipped with one broadcast read, a direction ends when distance^2 alone cannot win, and a
//                             block that may win is scanned by the wave together (every lane reads the same address:
//                             broadcast).  Exact, because only candidates that provably lose are skipped; bounded by the
//                             width per pixel whatever the content.  It writes dist2 / nearest / within in place
//                             and counts the summary: per thread, per wave, LDS, then one set of 64-bit atomics per workgroup;
//                             words 3 and 4 travel as ONE key (dist_key) under atomicMax in word 3.
//   4 dswx_distance_key_k     unpacks that key into words 3 and 4 (one thread per tile).
// DESIGN.md section 5 has the bytes per pixel of each launch and what was measured.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

#include "dswx_host.h"
#include "dswx_distance_rule.h"

namespace {

typedef uint32_t __attribute__((aligned(1))) dist_u32_b;  // 4 bytes anywhere (the plane)
typedef u32x4 __attribute__((aligned(4))) dist_u32x4_w;   // four uint32 at a 4-byte address (dist2)

constexpr int DIST_BLOCK = 256;
constexpr int BAND_H = DSWX_DISTANCE_BAND_H, COLS = DSWX_DISTANCE_COLS, BLOCK_W = DSWX_DISTANCE_BLOCK_W, NEAR = DSWX_DISTANCE_NEAR;
constexpr int DIST_WAVES = DIST_BLOCK / 64;
constexpr int64_t DIST_MAX_PIXELS = 1LL << 31;
constexpr unsigned NO_ROW = 0xFFFFFFFFu;
static_assert(COLS == 4, "a thread's load is one uint32 and its store one u32x4");
static_assert(BLOCK_W == 64, "a block of the row pass is the 64 lanes of a wave");
static_assert(NEAR < BLOCK_W, "the outward look stays inside the block and its two neighbours");

struct DistArgs {
    const unsigned char* plane;
    unsigned long long stride;                           // bytes between tiles of the plane
    unsigned long long n_elems;                          // height * width <= 2^31
    long long n_tiles;
    unsigned height, width;
    unsigned bands, cgblocks;                            // bands of rows; workgroups across the column groups
    unsigned radius, limit, mark;
    unsigned* dist2;
    unsigned* nearest;
    unsigned char* within;
    unsigned long long* summary;
    unsigned bits[8];                                    // target_of_byte as 256 bits
};

// ---- launches 1 and 2: a band of rows, four columns a thread ----------------------------------------------------------------
// The targets of rows y0 .. y0 + rows - 1 of columns x .. x + nv - 1 as bit r of m[c].  TERMINATES: rows <= 64.
__device__ __forceinline__ void band_masks(const unsigned* bits, const unsigned char* tile, unsigned width, unsigned y0,
                                           unsigned rows, unsigned x, int nv, unsigned long long (&m)[COLS]) {
#pragma unroll
    for (int c = 0; c < COLS; ++c) m[c] = 0ull;
    for (unsigned r = 0; r < rows; ++r) {
        const unsigned char* const p = tile + (unsigned long long)(y0 + r) * width + x;
        unsigned v = 0;
        if (nv == COLS) v = *reinterpret_cast<const dist_u32_b*>(p);             // (ends inside the row)
        else
#pragma unroll
            for (int c = 0; c < COLS; ++c)
                if (c < nv) v |= (unsigned)p[c] << (8 * c);
#pragma unroll
        for (int c = 0; c < COLS; ++c)
            if (c < nv && label_is_member(bits, (v >> (8 * c)) & 0xffu)) m[c] |= 1ull << r;
    }
}
__device__ __forceinline__ unsigned band_note(unsigned long long m) {
    return m ? dist_band_bits(true, (unsigned)__builtin_ctzll(m), 63u - (unsigned)__builtin_clzll(m)) : 0u;
}

template <bool FILL> __global__ __launch_bounds__(DIST_BLOCK) void dswx_distance_column_k(const DistArgs a) {
    __shared__ unsigned bits[8];
    if (threadIdx.x < 8) bits[threadIdx.x] = a.bits[threadIdx.x];
    __syncthreads();                                     // (the only barrier: a thread may leave after it)
    const unsigned band = blockIdx.x / a.cgblocks, cgb = blockIdx.x - band * a.cgblocks;
    const unsigned x = (cgb * DIST_BLOCK + threadIdx.x) * COLS;
    if (x >= a.width) return;
    const int nv = a.width - x < (unsigned)COLS ? (int)(a.width - x) : COLS;
    const unsigned y0 = band * BAND_H;
    const unsigned rows = a.height - y0 < (unsigned)BAND_H ? a.height - y0 : BAND_H;
    const unsigned long long W = a.width;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        unsigned long long m[COLS];
        band_masks(bits, a.plane + (unsigned long long)t * a.stride, a.width, y0, rows, x, nv, m);
        unsigned* const d = a.dist2 + (unsigned long long)t * a.n_elems;
        if (!FILL) {
            // launch 1: the note of the band, in its first row
#pragma unroll
            for (int c = 0; c < COLS; ++c)
                if (c < nv) d[y0 * W + x + c] = band_note(m[c]);
            continue;
        }
        // launch 2.  The row of the nearest target above the band and below it, from the notes of the other bands.
        // TERMINATES: bb runs over at most `bands` bands in each direction.
        unsigned above[COLS], below[COLS];
#pragma unroll
        for (int c = 0; c < COLS; ++c) above[c] = below[c] = NO_ROW;
        unsigned open = (1u << nv) - 1u;
        for (unsigned bb = band; bb-- > 0 && open;) {
            if (a.radius && y0 - (bb * BAND_H + BAND_H - 1) > a.radius) break;   // (nothing of that band reaches this one)
#pragma unroll
            for (int c = 0; c < COLS; ++c)
                if ((open >> c) & 1u) {
                    const unsigned e = __hip_atomic_load(d + (unsigned long long)bb * BAND_H * W + x + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (dist_band_has(e)) above[c] = bb * BAND_H + dist_band_bottom(e), open &= ~(1u << c);
                }
        }
        open = (1u << nv) - 1u;
        for (unsigned bb = band + 1; bb < a.bands && open; ++bb) {
            if (a.radius && bb * BAND_H - (y0 + rows - 1) > a.radius) break;
#pragma unroll
            for (int c = 0; c < COLS; ++c)
                if ((open >> c) & 1u) {
                    const unsigned e = __hip_atomic_load(d + (unsigned long long)bb * BAND_H * W + x + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (dist_band_has(e)) below[c] = bb * BAND_H + dist_band_top(e), open &= ~(1u << c);
                }
        }
        for (unsigned r = 0; r < rows; ++r) {
            const unsigned y = y0 + r;
            unsigned e[COLS];
#pragma unroll
            for (int c = 0; c < COLS; ++c) {
                const unsigned long long up_bits = m[c] & (~0ull >> (63u - r)), down_bits = m[c] >> r;
                const unsigned up = up_bits ? r - (63u - (unsigned)__builtin_clzll(up_bits)) : above[c] != NO_ROW ? y - above[c] : DIST_FAR;
                const unsigned down = down_bits ? (unsigned)__builtin_ctzll(down_bits) : below[c] != NO_ROW ? below[c] - y : DIST_FAR;
                e[c] = dist_entry(up, down, a.radius);
            }
            unsigned* const q = d + y * W + x;
            if (r == 0 && a.bands > 1) {
                // the note stays: another band may be reading it
#pragma unroll
                for (int c = 0; c < COLS; ++c)
                    if (c < nv) __hip_atomic_store(q + c, e[c] | band_note(m[c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (nv == COLS) {
                *reinterpret_cast<dist_u32x4_w*>(q) = u32x4{e[0], e[1], e[2], e[3]};
            } else {
#pragma unroll
                for (int c = 0; c < COLS; ++c)
                    if (c < nv) q[c] = e[c];
            }
        }
    }
}

// ---- launch 3: a row in LDS -------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned dist_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    return ((unsigned long long)hi << 32) | lo;
}
// candidate column xc with entry dy against the best so far: the smaller d2, on a tie the smaller column
__device__ __forceinline__ void dist_take(unsigned x, unsigned xc, int dy, unsigned& best, unsigned& best_x) {
    const unsigned d = dist_d2(x > xc ? x - xc : xc - x, dy);
    if (d < best || (d == best && xc < best_x)) best = d, best_x = xc;
}

__global__ __launch_bounds__(DIST_BLOCK) void dswx_distance_row_k(const DistArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dist_lds[];
    const unsigned W = a.width, nblk = (W + BLOCK_W - 1) / BLOCK_W, wpad = nblk * BLOCK_W;
    unsigned long long* const part = reinterpret_cast<unsigned long long*>(dist_lds);                   // [40]
    int* const ent = reinterpret_cast<int*>(dist_lds + DSWX_DISTANCE_SUMMARY_WORDS * 8);                  // [wpad]: dy or DIST_NO_DY
    unsigned* const bm = reinterpret_cast<unsigned*>(ent + wpad);                                        // [nblk]: min |dy|, NONE
    unsigned* const at_left = bm + nblk;                 // [nblk]: the nearest block at or left of c that is not empty, NO_BLOCK
    unsigned* const at_right = at_left + nblk;           // [nblk]: the nearest block at or right of c that is not empty, NO_BLOCK
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned y = blockIdx.x;
    constexpr unsigned NONE = DSWX_DISTANCE_NONE, NO_BLOCK = 0xFFFFFFFFu;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        __syncthreads();                                 // (ent, bm and part of the tile before)
        if (a.summary && tid < DSWX_DISTANCE_SUMMARY_WORDS) part[tid] = 0ull;
        const unsigned long long row0 = (unsigned long long)t * a.n_elems + (unsigned long long)y * W;
        unsigned* const d = a.dist2 + row0;
        // TERMINATES: xb rises by 256 up to wpad.  (Whole waves: the minimum needs every lane.)
        for (unsigned xb = wave * BLOCK_W; xb < wpad; xb += DIST_BLOCK) {
            const unsigned x = xb + lane;
            const int dy = x < W ? dist_entry_dy(d[x]) : DIST_NO_DY;
            ent[x] = dy;
            const unsigned lo = wave_min(dy == DIST_NO_DY ? NONE : (unsigned)(dy < 0 ? -dy : dy));
            if (lane == 0) bm[xb / BLOCK_W] = lo;
        }
        __syncthreads();
        // the skip lists over the blocks that hold an entry (nblk <= 128 threads).  TERMINATES: c runs to an end of the row.
        if (tid < nblk) {
            unsigned l = NO_BLOCK, r = NO_BLOCK;
            for (unsigned c = tid + 1; c-- > 0;)
                if (bm[c] != NONE) {
                    l = c;
                    break;
                }
            for (unsigned c = tid; c < nblk; ++c)
                if (bm[c] != NONE) {
                    r = c;
                    break;
                }
            at_left[tid] = l;
            at_right[tid] = r;
        }
        __syncthreads();
        unsigned n_target = 0, n_reached = 0, n_not = 0;
        unsigned long long sum = 0ull, key = 0ull;
        // TERMINATES: bi rises by 4 up to nblk.
        for (unsigned bi = wave; bi < nblk; bi += DIST_WAVES) {
            const unsigned x = bi * BLOCK_W + lane;
            const bool valid = x < W;
            unsigned best = a.limit, best_x = 0;
            if (valid) {
                const int dy = ent[x];
                if (dy != DIST_NO_DY) best = (unsigned)(dy * dy), best_x = x;
            }
            // the look to either side.  Nothing to see when the block and both neighbours are empty (wave-uniform).
            const bool near_any = bm[bi] != NONE || (bi > 0 && bm[bi - 1] != NONE) || (bi + 1 < nblk && bm[bi + 1] != NONE);
            if (near_any) {
                // TERMINATES: k <= NEAR.
                for (unsigned k = 1; k <= (unsigned)NEAR; ++k) {
                    const bool go = valid && k * k <= best;
                    if (!__any(go)) break;
                    if (go) {
                        if (x >= k) {
                            const int dy = ent[x - k];
                            if (dy != DIST_NO_DY) dist_take(x, x - k, dy, best, best_x);
                        }
                        if (x + k < W) {
                            const int dy = ent[x + k];
                            if (dy != DIST_NO_DY) dist_take(x, x + k, dy, best, best_x);
                        }
                    }
                }
            }
            // the blocks, outward, for the lanes that a column further than NEAR away may still serve
            const bool open = valid && best >= (unsigned)((NEAR + 1) * (NEAR + 1));
            if (__any(open)) {
                // only the blocks that hold an entry, the nearest first on either side
                unsigned cl = at_left[bi], cr = bi + 1 < nblk ? at_right[bi + 1] : NO_BLOCK;
                // TERMINATES: cl strictly falls and cr strictly rises from step to step, each to NO_BLOCK at the latest.
                while (cl != NO_BLOCK || cr != NO_BLOCK) {
#pragma unroll
                    for (int side = 0; side < 2; ++side) {
                        const unsigned c = side ? cr : cl;
                        if (c == NO_BLOCK) continue;
                        const unsigned x_first = c * BLOCK_W;
                        const unsigned gap = c < bi ? x - (x_first + BLOCK_W - 1) : c > bi ? x_first - x : 0u;
                        if (!__any(open && gap * gap <= best)) {         // further out the gap only grows: this side is done
                            if (side) cr = NO_BLOCK;
                            else cl = NO_BLOCK;
                            continue;
                        }
                        if (side) cr = c + 1 < nblk ? at_right[c + 1] : NO_BLOCK;
                        else cl = c > 0 ? at_left[c - 1] : NO_BLOCK;
                        const unsigned lo = bm[c];
                        // (a column of this block within NEAR has been seen: what is left is further than that)
                        const unsigned far = gap > (unsigned)NEAR ? gap : (unsigned)NEAR + 1u;
                        const unsigned bound = far * far + lo * lo;
                        const bool want = open && (bound < best || (bound == best && x_first < best_x));
                        if (!__any(want)) continue;
                        const unsigned cols = W - x_first < (unsigned)BLOCK_W ? W - x_first : BLOCK_W;
                        // TERMINATES: cols <= 64.
                        for (unsigned i = 0; i < cols; ++i) {
                            const int dy = ent[x_first + i];             // (one address for the wave: broadcast)
                            if (dy != DIST_NO_DY && want) dist_take(x, x_first + i, dy, best, best_x);
                        }
                    }
                }
            }
            const bool reached = valid && best != a.limit;
            const unsigned d2 = reached ? best : NONE;
            if (valid) {
                const unsigned idx = y * W + x;
                d[x] = d2;
                if (a.nearest) a.nearest[row0 + x] = reached ? (unsigned)(y + ent[best_x]) * W + best_x : NONE;
                if (a.within) {
                    const unsigned byte = a.plane[(unsigned long long)t * a.stride + idx];
                    a.within[row0 + x] = (unsigned char)dist_within(byte, d2, a.mark);
                }
                if (a.summary) {
                    if (!reached) ++n_not;
                    else {
                        if (d2) ++n_reached;
                        else ++n_target;
                        sum += d2;
                        const unsigned long long k = dist_key(d2, idx);
                        key = k > key ? k : key;
                    }
                }
            }
            if (a.summary) {
                // the size bins: one LDS atomic per DISTINCT bin of the wave.  TERMINATES: every round settles a lane.
                const int bin = reached && d2 ? dist_size_bin(d2) : -1;
                bool pend = bin >= 0;
                for (;;) {
                    const unsigned long long todo = __ballot(pend);
                    if (!todo) break;
                    const int leader = __ffsll((long long)todo) - 1;
                    const int b = __shfl(bin, leader);
                    const bool match = pend && bin == b;
                    const unsigned long long who = __ballot(match);
                    if (lane == (unsigned)leader) atomicAdd(&part[8 + b], (unsigned long long)__popcll(who));
                    pend = pend && !match;
                }
            }
        }
        if (a.summary) {
            n_target = dist_wave_sum(n_target);
            n_reached = dist_wave_sum(n_reached);
            n_not = dist_wave_sum(n_not);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                sum += shfl_xor_u64(sum, o);
                const unsigned long long k = shfl_xor_u64(key, o);
                key = k > key ? k : key;
            }
            if (lane == 0) {
                if (n_target) atomicAdd(&part[0], (unsigned long long)n_target);
                if (n_reached) atomicAdd(&part[1], (unsigned long long)n_reached);
                if (n_not) atomicAdd(&part[2], (unsigned long long)n_not);
                if (key) atomicMax(&part[3], key);
                if (sum) atomicAdd(&part[5], sum);
            }
            __syncthreads();
            if (tid < DSWX_DISTANCE_SUMMARY_WORDS && part[tid]) {
                unsigned long long* const w = a.summary + (unsigned long long)t * DSWX_DISTANCE_SUMMARY_WORDS + tid;
                if (tid == 3) atomicMax(w, part[3]);
                else atomicAdd(w, part[tid]);
            }
        }
    }
}

__global__ void dswx_distance_key_k(unsigned long long* summary, long long n_tiles) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const unsigned long long key = summary[t * DSWX_DISTANCE_SUMMARY_WORDS + 3];
    summary[t * DSWX_DISTANCE_SUMMARY_WORDS + 3] = dist_key_d2(key);
    summary[t * DSWX_DISTANCE_SUMMARY_WORDS + 4] = dist_key_idx(key);
}

}  // namespace

// The checks that the device and the host entry share, in the house order: the arguments before any context, nothing
// written by a refused call.  `align` = dist2 and nearest must be 4-byte and summary 8-byte aligned (the device entry).
int dswx_distance_check(const uint8_t* plane, const dswx_distance_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                        int64_t* stride, const dswx_distance_out_t* out, bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (spec->mark < 0 || spec->mark > 255) return dswx_fail(DSWX_ERR_ARG, "mark %d outside 0 .. 255", spec->mark);
    if (n_tiles < 0 || height < 0 || width < 0 || *stride < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (height > DSWX_DISTANCE_MAX_SIDE || width > DSWX_DISTANCE_MAX_SIDE)
        return dswx_fail(DSWX_ERR_ARG, "raster too large: height and width are at most %d, a squared distance would not fit 32 bits", DSWX_DISTANCE_MAX_SIDE);
    if (height * width > DIST_MAX_PIXELS) return dswx_fail(DSWX_ERR_ARG, "raster too large: height * width above 2^31");
    if (width > DSWX_DISTANCE_MAX_WIDTH)
        return dswx_fail(DSWX_ERR_ARG, "width %lld above DSWX_DISTANCE_MAX_WIDTH (%d): a row would not fit the local memory of the row pass",
                         (long long)width, DSWX_DISTANCE_MAX_WIDTH);
    const int64_t n_elems = height * width;
    if (int rc = dswx_tile_geometry_check(plane, n_tiles, n_elems, stride, true)) return rc;
    if (!out->dist2) return dswx_fail(DSWX_ERR_ARG, "dist2 is NULL: it is the working array and always required");
    if (out->within && spec->max_radius == 0)
        return dswx_fail(DSWX_ERR_ARG, "within is wanted but max_radius is 0: the ring needs a radius");
    if (align) {
        if (!aligned_to(out->dist2, 4)) return dswx_fail(DSWX_ERR_ALIGN, "dist2 not 4-byte aligned");
        if (!aligned_to(out->nearest, 4)) return dswx_fail(DSWX_ERR_ALIGN, "nearest not 4-byte aligned");
        if (!aligned_to(out->summary, 8)) return dswx_fail(DSWX_ERR_ALIGN, "summary not 8-byte aligned");
    }
    return DSWX_OK;
}

// The launches; the arguments have passed dswx_distance_check (stride resolved).
int dswx_distance_launch(dswx_ctx* ctx, const uint8_t* plane, const dswx_distance_spec_t* spec, int64_t n_tiles, int64_t height,
                         int64_t width, int64_t stride, const dswx_distance_out_t* out, hipStream_t s) {
    if (n_tiles == 0 || height == 0 || width == 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    DistArgs a = {};
    a.plane = plane;
    a.stride = (unsigned long long)stride;
    a.n_elems = (unsigned long long)(height * width);
    a.n_tiles = n_tiles;
    a.height = (unsigned)height;
    a.width = (unsigned)width;
    a.bands = (unsigned)((height + BAND_H - 1) / BAND_H);
    a.cgblocks = (unsigned)((width + COLS * DIST_BLOCK - 1) / (COLS * DIST_BLOCK));
    a.radius = spec->max_radius;
    a.limit = dist_limit(spec->max_radius);
    a.mark = (unsigned)spec->mark;
    a.dist2 = out->dist2;
    a.nearest = out->nearest;
    a.within = out->within;
    a.summary = reinterpret_cast<unsigned long long*>(out->summary);
    label_member_bits(spec->target_of_byte, a.bits);
    // (height <= 46340 and width <= 8192: at most 725 bands of 8 workgroups, and one workgroup a row -- every grid.x fits)
    const unsigned gy = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
    const unsigned nblk = (a.width + BLOCK_W - 1) / BLOCK_W;
    const size_t lds = (size_t)DSWX_DISTANCE_SUMMARY_WORDS * 8 + (size_t)nblk * BLOCK_W * 4 + (size_t)nblk * 12;
    const dim3 block(DIST_BLOCK), cgrid(a.bands * a.cgblocks, gy);
    if (out->summary) HIP_TRY(hipMemsetAsync(out->summary, 0, (size_t)n_tiles * DSWX_DISTANCE_SUMMARY_WORDS * sizeof(uint64_t), s));
    if (a.bands > 1) hipLaunchKernelGGL(dswx_distance_column_k<false>, cgrid, block, 0, s, a);
    hipLaunchKernelGGL(dswx_distance_column_k<true>, cgrid, block, 0, s, a);
    hipLaunchKernelGGL(dswx_distance_row_k, dim3(a.height, gy), block, lds, s, a);
    if (out->summary)
        hipLaunchKernelGGL(dswx_distance_key_k, dim3((unsigned)((n_tiles + DIST_BLOCK - 1) / DIST_BLOCK)), block, 0, s, a.summary,
                           (long long)n_tiles);
    HIP_TRY(hipGetLastError());
    char info[256];
    snprintf(info, sizeof info, "dswx_distance_column_k<band%s> grid=(%u,%u,1) block=%d band=%dx%d + dswx_distance_row_k grid=(%u,%u,1) lds=%zu radius=%u",
             a.bands > 1 ? ",fill" : "", a.bands * a.cgblocks, gy, DIST_BLOCK, BAND_H, COLS, a.height, gy, lds, a.radius);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_distance_host(const uint8_t* plane, const dswx_distance_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                       int64_t stride, const dswx_distance_out_t* out) {
    if (int rc = dswx_distance_check(plane, spec, n_tiles, height, width, &stride, out, false)) return rc;
    if (n_tiles == 0 || height == 0 || width == 0) return DSWX_OK;
    const int64_t n = height * width;
    const uint32_t R = spec->max_radius, limit = dist_limit(R);
    uint32_t bits[8];
    label_member_bits(spec->target_of_byte, bits);
    std::vector<int32_t> row((size_t)width);
    for (int64_t t = 0; t < n_tiles; ++t) {
        const uint8_t* tile = plane + (size_t)t * (size_t)stride;
        uint32_t* d = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(out->dist2) + (size_t)t * (size_t)n * 4);
        uint32_t* near = out->nearest ? reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(out->nearest) + (size_t)t * (size_t)n * 4) : nullptr;
        // the column pass: down with the last target seen, then up with the next one; dist2 holds the entries meanwhile
        for (int64_t x = 0; x < width; ++x) {
            int64_t last = -1;
            for (int64_t y = 0; y < height; ++y) {
                if (label_is_member(bits, tile[y * width + x])) last = y;
                dswx_store<uint32_t>(d, y * width + x, last < 0 ? DIST_FAR : (uint32_t)(y - last));
            }
            int64_t next = -1;
            for (int64_t y = height - 1; y >= 0; --y) {
                if (label_is_member(bits, tile[y * width + x])) next = y;
                dswx_store<uint32_t>(d, y * width + x, dist_entry(dswx_load<uint32_t>(d, y * width + x), next < 0 ? DIST_FAR : (uint32_t)(next - y), R));
            }
        }
        // the row pass: from every pixel outward until the step alone cannot win.  TERMINATES: k rises to the width.
        uint64_t sum[DSWX_DISTANCE_SUMMARY_WORDS] = {};
        uint64_t key = 0;
        for (int64_t y = 0; y < height; ++y) {
            bool any = false;
            for (int64_t x = 0; x < width; ++x) {
                row[(size_t)x] = dist_entry_dy(dswx_load<uint32_t>(d, y * width + x));
                any = any || row[(size_t)x] != DIST_NO_DY;
            }
            for (int64_t x = 0; x < width; ++x) {
                uint32_t best = limit, best_x = 0;
                if (any) {
                    if (row[(size_t)x] != DIST_NO_DY) best = (uint32_t)(row[(size_t)x] * row[(size_t)x]), best_x = (uint32_t)x;
                    for (int64_t k = 1; (uint64_t)(k * k) <= best && (x - k >= 0 || x + k < width); ++k) {
                        for (int side = 0; side < 2; ++side) {
                            const int64_t xc = side ? x + k : x - k;
                            if (xc < 0 || xc >= width || row[(size_t)xc] == DIST_NO_DY) continue;
                            const uint32_t c = dist_d2((uint32_t)k, row[(size_t)xc]);
                            if (c < best || (c == best && (uint32_t)xc < best_x)) best = c, best_x = (uint32_t)xc;
                        }
                    }
                }
                const int64_t p = y * width + x;
                const bool reached = best != limit;
                const uint32_t d2 = reached ? best : DSWX_DISTANCE_NONE;
                dswx_store<uint32_t>(d, p, d2);
                if (near) dswx_store<uint32_t>(near, p, reached ? (uint32_t)((y + row[best_x]) * width + best_x) : DSWX_DISTANCE_NONE);
                if (out->within) out->within[(size_t)t * (size_t)n + (size_t)p] = (uint8_t)dist_within(tile[p], d2, (unsigned)spec->mark);
                if (!reached) {
                    ++sum[2];
                    continue;
                }
                ++sum[d2 ? 1 : 0];
                sum[5] += d2;
                const uint64_t k = dist_key(d2, (uint32_t)p);
                if (k > key) key = k;
                if (d2) ++sum[8 + dist_size_bin(d2)];
            }
        }
        sum[3] = dist_key_d2(key);
        sum[4] = dist_key_idx(key);
        if (out->summary)
            for (int w = 0; w < DSWX_DISTANCE_SUMMARY_WORDS; ++w) dswx_store<uint64_t>(out->summary, t * DSWX_DISTANCE_SUMMARY_WORDS + w, sum[w]);
    }
    return DSWX_OK;
}

int dswx_distance_device(dswx_ctx_t* ctx, const uint8_t* plane, const dswx_distance_spec_t* spec, int64_t n_tiles, int64_t height,
                         int64_t width, int64_t stride, const dswx_distance_out_t* out, void* stream) {
    if (int rc = dswx_distance_check(plane, spec, n_tiles, height, width, &stride, out, true)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) { return dswx_distance_launch(ctx, plane, spec, n_tiles, height, width, stride, out, s); });
}

}  // extern "C"
