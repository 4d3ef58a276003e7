// dswx_reach.hip -- every pixel whose centre lies within a radius of a polygon edge (DSWX_HAS_REACH, additive to ABI v7): the
// exact metric buffer of the VECTOR on the raster, the twin of dswx_burn.hip.  include/dswx_hip.h "reach" states the
// definition; proteus_amd/reach.py is its numpy statement and dswx_reach_host below the scalar one -- dswx_reach_rule.h is
// compiled for both sides.
//
// The burn's shape with addition in place of XOR: the capsule of an edge is convex, so on every row it reaches ONE run of
// columns c0 .. c1.  Every edge SCATTERS +1 at (r, c0) and -1 at (r, c1 + 1) (when that is inside the row), and a per-row
// prefix SUM turns the differences into the number of edges that reach each pixel.  Integer addition commutes, so neither the
// launch geometry nor the order of the atomics shows in the result.
//
// NO WORKGROUP EVER WAITS FOR ANOTHER.  One hipMemsetAsync each of `acc` and `head`, then two launches:
//   1 dswx_reach_scatter_k blockIdx.y walks the tiles, blockIdx.x strides over the records of a tile, one thread per record: one
//                          16-byte load, the bound check of `next`, one dependent 16-byte load, K = isqrt(R^2 D) once.  An
//                          edge of at most DSWX_REACH_THREAD_ROWS rows (radii below two pixels) is finished by its thread;
//                          every other one is peeled by the wave: ballot, leader, and the 64 lanes stride its rows.  A row is
//                          reach_row: two integer square roots for the discs, the slab's ends estimated in double and moved
//                          with the exact 128-bit predicate; then two non-returning atomic adds.  The counts of the head are
//                          summed per wave and per workgroup before one set of 64-bit atomics.
//   2 dswx_reach_scan_k    the prefix sum along every row of `acc` in place, fused with the write of `mask` and the count of the
//                          pixels: dswx_ring_scan.h, the body of dswx_burn_scan_k with + for ^.
// DESIGN.md section 5 has the atomics per edge and per pixel.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dswx_host.h"
#include "dswx_reach_rule.h"
#include "dswx_ring_scan.h"

namespace {

typedef u32x4 __attribute__((aligned(16))) reach_u32x4;

constexpr int REACH_BLOCK = 256;
constexpr int REACH_WAVES = REACH_BLOCK / 64;
constexpr int REACH_COUNTS = 5;                          // head words 1 .. 5: what the scatter launch sums
constexpr unsigned REACH_SCATTER_BLOCKS = 4096;          // the scatter launch: about this many workgroups over all tiles
constexpr unsigned REACH_SCAN_BLOCKS = 4096;             // the scan launch: at most this many workgroups
static_assert(DSWX_REACH_SCAN_STEP == 64 * 4, "a wave's step: 64 lanes of four pixels");
static_assert(REACH_BLOCK == RING_BLOCK && DSWX_REACH_HEAD_WORDS == RING_HEAD_WORDS && REACH_HEAD_REACHED == RING_HEAD_PIXELS, "dswx_ring_scan.h");
static_assert(sizeof(dswx_reach_spec_t) == 32, "the spec of the header");
static_assert(DSWX_REACH_MAX_RADIUS == REACH_MAX_RADIUS, "the header and the rule");

typedef RingArgs ReachArgs;                              // (dswx_ring_scan.h: the fields of both launches)

// One row of one edge: the two differences, and what the head counts of it.  True iff the row has a pixel of the tile.
struct ReachCounts {
    unsigned intervals, cut_left, cut_right;
};
__device__ __forceinline__ bool reach_apply(unsigned* acc, long long width, long long r, const ReachEdge& e, ReachCounts* n) {
    const ReachRun run = reach_row(e, r, width);
    const long long c0 = run.lo < 0 ? 0 : run.lo, c1 = run.hi >= width ? width - 1 : run.hi;
    if (c0 > c1) return false;                           // (an empty run, or one of the two columns beside the raster alone)
    unsigned* const row = acc + (unsigned long long)(r * width);
    atomicAdd(row + c0, 1u);                             // (the results are not used: no return)
    if (c1 + 1 < width) atomicAdd(row + c1 + 1, 0xFFFFFFFFu);
    ++n->intervals;
    n->cut_left += run.lo < 0;
    n->cut_right += run.hi >= width;
    return true;
}

// ---- launch 1: the differences of every edge and row, the counts of the head ---------------------------------------------------
__global__ __launch_bounds__(REACH_BLOCK) void dswx_reach_scatter_k(const ReachArgs a, const unsigned radius) {
    __shared__ unsigned wsum[REACH_WAVES][REACH_COUNTS];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const long long first = a.tile_first[t], count = burn_count(first, a.tile_first[t + 1]);
        const reach_u32x4* const verts = a.verts + first;
        unsigned* const acc = a.acc + (unsigned long long)t * a.n_elems;
        unsigned malformed = 0, edges = 0;
        ReachCounts n = {0u, 0u, 0u};
        // (`base` is the same for the lanes of a wave: all of them take part in the ballots and the shuffles below)
        for (long long base = (long long)blockIdx.x * REACH_BLOCK + wave * 64; base < count; base += (long long)gridDim.x * REACH_BLOCK) {
            const long long i = base + lane;
            int ax = 0, ay = 0, bx = 0, by = 0;
            bool shared = false;
            if (i < count) {
                const u32x4 v = verts[i];
                if ((long long)v.w >= count)             // before the dependent load
                    ++malformed;
                else {
                    const u32x4 w = verts[v.w];
                    ax = (int)v.x, ay = (int)v.y, bx = (int)w.x, by = (int)w.y;
                    if (!burn_legal(ax) || !burn_legal(ay) || !burn_legal(bx) || !burn_legal(by))
                        ++malformed;
                    else {
                        // the rows alone, before the square root of the edge: most of a wave's edges are shared out
                        int64_t r0, r1;
                        const bool rows = reach_rows(ay, by, radius, a.height, &r0, &r1);
                        if (r1 - r0 > DSWX_REACH_THREAD_ROWS)
                            shared = true;
                        else if (rows) {
                            ReachEdge e;
                            reach_edge(ax, ay, bx, by, radius, a.height, &e);
                            bool any = false;
                            for (long long r = e.r0; r < e.r1; ++r) any |= reach_apply(acc, a.width, r, e, &n);
                            edges += any;
                        }
                    }
                }
            }
            unsigned long long todo = __ballot(shared);
            while (todo) {                               // (uniform)
                const int leader = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                ReachEdge g;
                reach_edge(__shfl(ax, leader), __shfl(ay, leader), __shfl(bx, leader), __shfl(by, leader), radius, a.height, &g);
                bool any = false;
                for (long long r = g.r0 + lane; r < g.r1; r += 64) any |= reach_apply(acc, a.width, r, g, &n);
                if (__ballot(any) && lane == (unsigned)leader) ++edges;
            }
        }
        if (!a.head) continue;                           // (uniform)
        unsigned sums[REACH_COUNTS] = {malformed, edges, n.intervals, n.cut_left, n.cut_right};
#pragma unroll
        for (int k = 0; k < REACH_COUNTS; ++k) {
            sums[k] = ring_wave_sum(sums[k]);
            if (lane == 0) wsum[wave][k] = sums[k];
        }
        __syncthreads();
        unsigned long long* const head = a.head + (unsigned long long)t * DSWX_REACH_HEAD_WORDS;
        if (threadIdx.x < REACH_COUNTS) {
            unsigned sum = 0;
#pragma unroll
            for (int w = 0; w < REACH_WAVES; ++w) sum += wsum[w][threadIdx.x];
            if (sum) atomicAdd(head + REACH_HEAD_MALFORMED + threadIdx.x, (unsigned long long)sum);
        }
        if (blockIdx.x == 0 && threadIdx.x == REACH_COUNTS) head[REACH_HEAD_RECORDS] = (unsigned long long)count;   // (behind the memset)
        __syncthreads();                                 // (wsum is written again for the next tile)
    }
}
static_assert(REACH_HEAD_MALFORMED == 1 && REACH_HEAD_EDGES == 2 && REACH_HEAD_INTERVALS == 3 && REACH_HEAD_CUT_LEFT == 4 && REACH_HEAD_CUT_RIGHT == 5,
              "the order of `sums` above");

// ---- launch 2: the prefix sum along every row, the mask, the pixels reached: dswx_ring_scan.h, which the burn shares ---------
__global__ __launch_bounds__(REACH_BLOCK) void dswx_reach_scan_k(const ReachArgs a) { ring_scan<RingSum>(a); }

const dswx_burn_spec_t* burn_part(const dswx_reach_spec_t* spec, dswx_burn_spec_t* b) {
    if (!spec) return nullptr;
    b->burn = spec->burn, b->background = spec->background;
    b->mask_tile_stride = spec->mask_tile_stride, b->src_tile_stride = spec->src_tile_stride;
    return b;
}

}  // namespace

// The checks that the entries share: the radius and the reserved word, then those of the burn entries (dswx_burn_check: the
// same records, table, planes and strides, in the house order).  Nothing is written by a refused call.
int dswx_reach_check(const void* verts, const int64_t* tile_first, const dswx_reach_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                     const uint8_t* src, const dswx_reach_out_t* out, int64_t* mask_stride, int64_t* src_stride, bool align) {
    dswx_burn_spec_t b;
    if (spec && spec->radius > DSWX_REACH_MAX_RADIUS)
        return dswx_fail(DSWX_ERR_ARG, "radius %u above DSWX_REACH_MAX_RADIUS %u (1/256 pixel)", spec->radius, (unsigned)DSWX_REACH_MAX_RADIUS);
    if (spec && spec->reserved) return dswx_fail(DSWX_ERR_ARG, "reserved %u must be 0", spec->reserved);
    return dswx_burn_check(verts, tile_first, burn_part(spec, &b), n_tiles, height, width, src, out, mask_stride, src_stride, align);
}

// The launches; the arguments have passed dswx_reach_check.
int dswx_reach_launch(dswx_ctx* ctx, const void* verts, const int64_t* tile_first, const dswx_reach_spec_t* spec, int64_t n_tiles, int64_t height,
                      int64_t width, const uint8_t* src, int64_t mask_stride, int64_t src_stride, const dswx_reach_out_t* out, hipStream_t s) {
    if (n_tiles == 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    ReachArgs a = {};
    a.verts = static_cast<const reach_u32x4*>(verts);
    a.tile_first = reinterpret_cast<const long long*>(tile_first);
    a.acc = out->acc;
    a.mask = out->mask;
    a.src = src;
    a.head = reinterpret_cast<unsigned long long*>(out->head);
    a.n_tiles = n_tiles, a.height = height, a.width = width;
    a.n_elems = (unsigned long long)(height * width);
    a.mask_stride = (unsigned long long)mask_stride, a.src_stride = (unsigned long long)src_stride;
    a.burn = (unsigned)spec->burn, a.background = (unsigned)spec->background;
    if (a.n_elems) HIP_TRY(hipMemsetAsync(a.acc, 0, (size_t)n_tiles * (size_t)a.n_elems * sizeof(uint32_t), s));
    if (a.head) HIP_TRY(hipMemsetAsync(a.head, 0, (size_t)n_tiles * DSWX_REACH_HEAD_WORDS * sizeof(uint64_t), s));
    // more than 65535 tiles: the workgroups of a row of the grid walk the tiles
    const unsigned gy = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
    const unsigned gx = REACH_SCATTER_BLOCKS / gy ? REACH_SCATTER_BLOCKS / gy : 1u;
    hipLaunchKernelGGL(dswx_reach_scatter_k, dim3(gx, gy), dim3(REACH_BLOCK), 0, s, a, spec->radius);
    unsigned scan_blocks = 0;
    if (a.n_elems) {                                     // (an empty raster has no rows or no columns)
        a.total_rows = (unsigned long long)n_tiles * (unsigned long long)height;          // <= 2^62
        a.rows_per_block = (a.total_rows + REACH_SCAN_BLOCKS - 1) / REACH_SCAN_BLOCKS;
        a.rows_per_block = (a.rows_per_block + REACH_WAVES - 1) / REACH_WAVES * REACH_WAVES;
        scan_blocks = (unsigned)((a.total_rows + a.rows_per_block - 1) / a.rows_per_block);
        hipLaunchKernelGGL(dswx_reach_scan_k, dim3(scan_blocks), dim3(REACH_BLOCK), 0, s, a);
    }
    HIP_TRY(hipGetLastError());
    char info[256];
    snprintf(info, sizeof info, "dswx_reach_scatter_k grid=(%u,%u,1) block=%d thread_rows=%d + dswx_reach_scan_k grid=(%u,1,1) block=%d rows_per_block=%llu step=%d",
             gx, gy, REACH_BLOCK, DSWX_REACH_THREAD_ROWS, scan_blocks, REACH_BLOCK, a.rows_per_block, DSWX_REACH_SCAN_STEP);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_reach_host(const dswx_burn_vertex_t* verts, const int64_t* tile_first, const dswx_reach_spec_t* spec, int64_t n_tiles, int64_t height,
                    int64_t width, const uint8_t* src, const dswx_reach_out_t* out) {
    int64_t mask_stride, src_stride;
    if (int rc = dswx_reach_check(verts, tile_first, spec, n_tiles, height, width, src, out, &mask_stride, &src_stride, false)) return rc;
    const int64_t n = height * width;
    std::vector<uint32_t> acc((size_t)n);
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t first = dswx_load<int64_t>(tile_first, (size_t)t), count = burn_count(first, dswx_load<int64_t>(tile_first, (size_t)t + 1));
        uint64_t head[DSWX_REACH_HEAD_WORDS] = {(uint64_t)count, 0, 0, 0, 0, 0, 0, 0};
        std::fill(acc.begin(), acc.end(), 0u);
        for (int64_t i = 0; i < count; ++i) {
            const dswx_burn_vertex_t v = dswx_load<dswx_burn_vertex_t>(verts, (size_t)(first + i));
            if ((int64_t)v.next >= count) {
                ++head[REACH_HEAD_MALFORMED];
                continue;
            }
            const dswx_burn_vertex_t w = dswx_load<dswx_burn_vertex_t>(verts, (size_t)(first + (int64_t)v.next));
            if (!burn_legal(v.x) || !burn_legal(v.y) || !burn_legal(w.x) || !burn_legal(w.y)) {
                ++head[REACH_HEAD_MALFORMED];
                continue;
            }
            ReachEdge e;
            if (!reach_edge(v.x, v.y, w.x, w.y, spec->radius, height, &e)) continue;
            bool any = false;
            for (int64_t r = e.r0; r < e.r1; ++r) {
                const ReachRun run = reach_row(e, r, width);
                const int64_t c0 = run.lo < 0 ? 0 : run.lo, c1 = run.hi >= width ? width - 1 : run.hi;
                if (c0 > c1) continue;
                ++acc[(size_t)(r * width + c0)];
                if (c1 + 1 < width) --acc[(size_t)(r * width + c1 + 1)];
                ++head[REACH_HEAD_INTERVALS];
                head[REACH_HEAD_CUT_LEFT] += run.lo < 0;
                head[REACH_HEAD_CUT_RIGHT] += run.hi >= width;
                any = true;
            }
            head[REACH_HEAD_EDGES] += any;
        }
        uint8_t* const mask = out->mask ? out->mask + (size_t)t * (size_t)mask_stride : nullptr;
        const uint8_t* const other = src ? src + (size_t)t * (size_t)src_stride : nullptr;
        for (int64_t r = 0; r < height; ++r) {
            uint32_t run = 0;
            for (int64_t c = 0; c < width; ++c) {
                const size_t p = (size_t)(r * width + c);
                run += acc[p];
                acc[p] = run;
                head[REACH_HEAD_REACHED] += run != 0u;
                if (mask) mask[p] = (uint8_t)(run ? spec->burn : other ? (int)other[p] : spec->background);
            }
        }
        if (n) std::memcpy(reinterpret_cast<unsigned char*>(out->acc) + (size_t)t * (size_t)n * 4, acc.data(), (size_t)n * 4);
        if (out->head)
            for (int w = 0; w < DSWX_REACH_HEAD_WORDS; ++w) dswx_store<uint64_t>(out->head, (size_t)(t * DSWX_REACH_HEAD_WORDS + w), head[w]);
    }
    return DSWX_OK;
}

int dswx_reach_device(dswx_ctx_t* ctx, const dswx_burn_vertex_t* verts, const int64_t* tile_first, const dswx_reach_spec_t* spec, int64_t n_tiles,
                      int64_t height, int64_t width, const uint8_t* src, const dswx_reach_out_t* out, void* stream) {
    int64_t mask_stride, src_stride;
    if (int rc = dswx_reach_check(verts, tile_first, spec, n_tiles, height, width, src, out, &mask_stride, &src_stride, true)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) {
        return dswx_reach_launch(ctx, verts, tile_first, spec, n_tiles, height, width, src, mask_stride, src_stride, out, s);
    });
}

}  // extern "C"
