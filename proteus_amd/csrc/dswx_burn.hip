// dswx_burn.hip -- polygon rings rasterised onto planes (DSWX_HAS_BURN, additive to ABI v7): the opposite direction of
// dswx_outline.hip.  include/dswx_hip.h "burn" states the definition; proteus_amd/burn.py is its numpy statement and
// dswx_burn_host below the scalar one -- dswx_burn_rule.h is compiled for both sides.
//
// Not a tile reduction: every edge SCATTERS the exact column of each of its row crossings as a toggle (an atomic XOR of the
// edge's word into `acc`), and a per-row XOR prefix turns the toggles into the inside of the rings.  XOR and integer addition
// commute, so neither the launch geometry nor the order of the atomics shows in the result.
//
// NO WORKGROUP EVER WAITS FOR ANOTHER.  One hipMemsetAsync each of `acc` and `head`, then two launches:
//   1 dswx_burn_toggle_k   blockIdx.y walks the tiles (so that a wave never straddles two tiles and nothing has to be searched
//                          in `tile_first`, which only the device reads), blockIdx.x strides over the records of a tile, one
//                          thread per record: one 16-byte load, the bound check of `next`, one dependent 16-byte load (in ring
//                          order the neighbouring record).  The first crossing costs ONE 64-bit division (quotient and
//                          remainder); further rows add a per-row quotient and remainder with a carry.  An edge of at most
//                          DSWX_BURN_THREAD_ROWS rows is finished by its thread; longer ones are peeled by the wave: ballot,
//                          leader, and the 64 lanes stride the rows of that edge, each with one division for its first row and
//                          the quotient and remainder of 64 rows after that -- a clip edge of 3660 rows is 58 steps of a wave.
//                          The counts of the head are summed per wave and per workgroup before one set of 64-bit atomics.
//   2 dswx_burn_scan_k     the XOR prefix along every row of `acc` in place, fused with the write of `mask` and the count of the
//                          pixels.  All rows of all tiles are numbered through; a workgroup takes a run of them, its four waves
//                          a row each in turn (so that tiles of a few pixels are not a launch's worth of work each).  A wave
//                          walks its row in steps of DSWX_BURN_SCAN_STEP pixels: 16 bytes of `acc` per lane from a 16-byte
//                          aligned address, a prefix in registers, one across the lanes, the running XOR carried from step to
//                          step.  A row begins wherever it begins (width 129): the slot that holds its first pixels and the
//                          one that holds its last are read and written pixel by pixel, so nothing outside the row is ever read.
// DESIGN.md section 5 has the bytes and atomics per pixel and per crossing.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dswx_host.h"
#include "dswx_burn_rule.h"
#include "dswx_ring_scan.h"

namespace {

typedef u32x4 __attribute__((aligned(16))) burn_u32x4;

constexpr int BURN_BLOCK = 256;
constexpr int BURN_WAVES = BURN_BLOCK / 64;
constexpr int BURN_COUNTS = 5;                           // head words 1 .. 5: what the toggle launch sums
constexpr int64_t BURN_MAX_PIXELS = 1LL << 30;
constexpr unsigned BURN_TOGGLE_BLOCKS = 4096;            // the toggle launch: about this many workgroups over all tiles
constexpr unsigned BURN_SCAN_BLOCKS = 4096;              // the scan launch: at most this many workgroups
static_assert(DSWX_BURN_SCAN_STEP == 64 * 4, "a wave's step: 64 lanes of four pixels");
static_assert(BURN_BLOCK == RING_BLOCK && DSWX_BURN_HEAD_WORDS == RING_HEAD_WORDS && BURN_HEAD_INSIDE == RING_HEAD_PIXELS, "dswx_ring_scan.h");
static_assert(sizeof(dswx_burn_vertex_t) == 16 && sizeof(dswx_burn_spec_t) == 24, "the records and the spec of the header");

typedef RingArgs BurnArgs;                               // (dswx_ring_scan.h: the fields of both launches)

__device__ __forceinline__ unsigned burn_wave_sum(unsigned v) { return ring_wave_sum(v); }

// One crossing of row r: the toggle, and what the head counts of it.
struct BurnCounts {
    unsigned toggles, dropped, clamped;
};
__device__ __forceinline__ void burn_apply(unsigned* acc, long long width, long long r, const BurnCross& c, unsigned word, BurnCounts* n) {
    long long col = burn_column(c);
    if (col < 0) col = 0, ++n->clamped;
    if (col < width) {
        atomicXor(acc + (unsigned long long)(r * width + col), word);        // (the result is not used: no return)
        ++n->toggles;
    } else
        ++n->dropped;
}

// ---- launch 1: the toggles of every edge, the counts of the head --------------------------------------------------------------
__global__ __launch_bounds__(BURN_BLOCK) void dswx_burn_toggle_k(const BurnArgs a) {
    __shared__ unsigned wsum[BURN_WAVES][BURN_COUNTS];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const long long first = a.tile_first[t], count = burn_count(first, a.tile_first[t + 1]);
        const burn_u32x4* const verts = a.verts + first;
        unsigned* const acc = a.acc + (unsigned long long)t * a.n_elems;
        unsigned malformed = 0, edges = 0;
        BurnCounts n = {0u, 0u, 0u};
        // (`base` is the same for the lanes of a wave: all of them take part in the ballot and the shuffles below)
        for (long long base = (long long)blockIdx.x * BURN_BLOCK + wave * 64; base < count; base += (long long)gridDim.x * BURN_BLOCK) {
            const long long i = base + lane;
            BurnEdge e = {0, 0, 0, 0, 0, 0};
            unsigned word = 0;
            bool shared = false;
            if (i < count) {
                const u32x4 v = verts[i];
                if ((long long)v.w >= count)             // before the dependent load
                    ++malformed;
                else {
                    const u32x4 w = verts[v.w];
                    if (!burn_legal((int)v.x) || !burn_legal((int)v.y) || !burn_legal((int)w.x) || !burn_legal((int)w.y))
                        ++malformed;
                    else if (burn_edge((int)v.x, (int)v.y, (int)w.x, (int)w.y, a.height, &e)) {
                        ++edges;
                        word = v.z;
                        if (e.r1 - e.r0 <= DSWX_BURN_THREAD_ROWS) {
                            const long long den = burn_den(e);
                            BurnCross c = burn_cross(e, e.r0);
                            burn_apply(acc, a.width, e.r0, c, word, &n);
                            if (e.r1 - e.r0 > 1) {
                                const BurnCross s = burn_step(e, 1);
                                for (long long r = e.r0 + 1; r < e.r1; ++r) {
                                    burn_advance(&c, s, den);
                                    burn_apply(acc, a.width, r, c, word, &n);
                                }
                            }
                        } else
                            shared = true;
                    }
                }
            }
            unsigned long long todo = __ballot(shared);
            while (todo) {                               // (uniform)
                const int leader = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                BurnEdge g;                              // every coordinate and row fits 32 bits
                g.x0 = __shfl((int)e.x0, leader), g.y0 = __shfl((int)e.y0, leader);
                g.x1 = __shfl((int)e.x1, leader), g.y1 = __shfl((int)e.y1, leader);
                g.r0 = __shfl((int)e.r0, leader), g.r1 = __shfl((int)e.r1, leader);
                const unsigned gw = __shfl(word, leader);
                long long r = g.r0 + lane;
                if (r < g.r1) {
                    const long long den = burn_den(g);
                    BurnCross c = burn_cross(g, r);
                    const BurnCross s = burn_step(g, 64);
                    for (;;) {
                        burn_apply(acc, a.width, r, c, gw, &n);
                        r += 64;
                        if (r >= g.r1) break;
                        burn_advance(&c, s, den);
                    }
                }
            }
        }
        if (!a.head) continue;                           // (uniform)
        unsigned sums[BURN_COUNTS] = {malformed, edges, n.toggles, n.dropped, n.clamped};
#pragma unroll
        for (int k = 0; k < BURN_COUNTS; ++k) {
            sums[k] = burn_wave_sum(sums[k]);
            if (lane == 0) wsum[wave][k] = sums[k];
        }
        __syncthreads();
        unsigned long long* const head = a.head + (unsigned long long)t * DSWX_BURN_HEAD_WORDS;
        if (threadIdx.x < BURN_COUNTS) {
            unsigned sum = 0;
#pragma unroll
            for (int w = 0; w < BURN_WAVES; ++w) sum += wsum[w][threadIdx.x];
            if (sum) atomicAdd(head + BURN_HEAD_MALFORMED + threadIdx.x, (unsigned long long)sum);
        }
        if (blockIdx.x == 0 && threadIdx.x == BURN_COUNTS) head[BURN_HEAD_RECORDS] = (unsigned long long)count;   // (behind the memset)
        __syncthreads();                                 // (wsum is written again for the next tile)
    }
}
static_assert(BURN_HEAD_MALFORMED == 1 && BURN_HEAD_EDGES == 2 && BURN_HEAD_TOGGLES == 3 && BURN_HEAD_DROPPED == 4 && BURN_HEAD_CLAMPED == 5,
              "the order of `sums` above");

// ---- launch 2: the XOR prefix along every row, the mask, the pixels inside: dswx_ring_scan.h, which the reach shares ----------
__global__ __launch_bounds__(BURN_BLOCK) void dswx_burn_scan_k(const BurnArgs a) { ring_scan<RingXor>(a); }

}  // namespace

// The checks that the entries share, in the house order: the arguments before any context, nothing written by a refused call.
// Resolves the two strides (0 = height * width).  `align`: the device's alignments.
int dswx_burn_check(const void* verts, const int64_t* tile_first, const dswx_burn_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                    const uint8_t* src, const dswx_burn_out_t* out, int64_t* mask_stride, int64_t* src_stride, bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (spec->burn < 0 || spec->burn > 255) return dswx_fail(DSWX_ERR_ARG, "burn %d outside 0 .. 255", spec->burn);
    if (spec->background < 0 || spec->background > 255) return dswx_fail(DSWX_ERR_ARG, "background %d outside 0 .. 255", spec->background);
    if (n_tiles < 0 || height < 0 || width < 0 || spec->mask_tile_stride < 0 || spec->src_tile_stride < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (height > BURN_MAX_PIXELS || width > BURN_MAX_PIXELS || height * width > BURN_MAX_PIXELS)
        return dswx_fail(DSWX_ERR_ARG, "raster too large: height * width above 2^30");
    const int64_t n = height * width;
    if (spec->mask_tile_stride && spec->mask_tile_stride < n)
        return dswx_fail(DSWX_ERR_ARG, "mask_tile_stride %lld below height * width %lld", (long long)spec->mask_tile_stride, (long long)n);
    if (spec->src_tile_stride && spec->src_tile_stride < n)
        return dswx_fail(DSWX_ERR_ARG, "src_tile_stride %lld below height * width %lld", (long long)spec->src_tile_stride, (long long)n);
    if (n_tiles > (1LL << 32)) return dswx_fail(DSWX_ERR_ARG, "plane too large: more than 2^32 tiles");
    if (!verts && n_tiles > 0) return dswx_fail(DSWX_ERR_ARG, "verts is NULL");
    if (!tile_first && n_tiles > 0) return dswx_fail(DSWX_ERR_ARG, "tile_first is NULL");
    if (!out->acc && n_tiles > 0 && n > 0) return dswx_fail(DSWX_ERR_ARG, "acc is NULL: it is the working array");
    if (src && !out->mask) return dswx_fail(DSWX_ERR_ARG, "src without mask: src is what mask holds where nothing is burnt");
    if (align) {
        if (!aligned_to(verts, 16)) return dswx_fail(DSWX_ERR_ALIGN, "verts not 16-byte aligned");
        if (!aligned_to(out->acc, 4)) return dswx_fail(DSWX_ERR_ALIGN, "acc not 4-byte aligned");
        if (!aligned_to(tile_first, 8)) return dswx_fail(DSWX_ERR_ALIGN, "tile_first not 8-byte aligned");
        if (!aligned_to(out->head, 8)) return dswx_fail(DSWX_ERR_ALIGN, "head not 8-byte aligned");
    }
    *mask_stride = spec->mask_tile_stride ? spec->mask_tile_stride : n;
    *src_stride = spec->src_tile_stride ? spec->src_tile_stride : n;
    return DSWX_OK;
}

// The launches; the arguments have passed dswx_burn_check.
int dswx_burn_launch(dswx_ctx* ctx, const void* verts, const int64_t* tile_first, const dswx_burn_spec_t* spec, int64_t n_tiles, int64_t height,
                     int64_t width, const uint8_t* src, int64_t mask_stride, int64_t src_stride, const dswx_burn_out_t* out, hipStream_t s) {
    if (n_tiles == 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    BurnArgs a = {};
    a.verts = static_cast<const burn_u32x4*>(verts);
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
    if (a.head) HIP_TRY(hipMemsetAsync(a.head, 0, (size_t)n_tiles * DSWX_BURN_HEAD_WORDS * sizeof(uint64_t), s));
    // more than 65535 tiles: the workgroups of a row of the grid walk the tiles
    const unsigned gy = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
    const unsigned gx = BURN_TOGGLE_BLOCKS / gy ? BURN_TOGGLE_BLOCKS / gy : 1u;
    hipLaunchKernelGGL(dswx_burn_toggle_k, dim3(gx, gy), dim3(BURN_BLOCK), 0, s, a);
    unsigned scan_blocks = 0;
    if (a.n_elems) {                                     // (an empty raster has no rows or no columns)
        a.total_rows = (unsigned long long)n_tiles * (unsigned long long)height;          // <= 2^62
        a.rows_per_block = (a.total_rows + BURN_SCAN_BLOCKS - 1) / BURN_SCAN_BLOCKS;
        a.rows_per_block = (a.rows_per_block + BURN_WAVES - 1) / BURN_WAVES * BURN_WAVES;
        scan_blocks = (unsigned)((a.total_rows + a.rows_per_block - 1) / a.rows_per_block);
        hipLaunchKernelGGL(dswx_burn_scan_k, dim3(scan_blocks), dim3(BURN_BLOCK), 0, s, a);
    }
    HIP_TRY(hipGetLastError());
    char info[256];
    snprintf(info, sizeof info, "dswx_burn_toggle_k grid=(%u,%u,1) block=%d thread_rows=%d + dswx_burn_scan_k grid=(%u,1,1) block=%d rows_per_block=%llu step=%d",
             gx, gy, BURN_BLOCK, DSWX_BURN_THREAD_ROWS, scan_blocks, BURN_BLOCK, a.rows_per_block, DSWX_BURN_SCAN_STEP);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_burn_host(const dswx_burn_vertex_t* verts, const int64_t* tile_first, const dswx_burn_spec_t* spec, int64_t n_tiles, int64_t height,
                   int64_t width, const uint8_t* src, const dswx_burn_out_t* out) {
    int64_t mask_stride, src_stride;
    if (int rc = dswx_burn_check(verts, tile_first, spec, n_tiles, height, width, src, out, &mask_stride, &src_stride, false)) return rc;
    const int64_t n = height * width;
    std::vector<uint32_t> acc((size_t)n);
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t first = dswx_load<int64_t>(tile_first, (size_t)t), count = burn_count(first, dswx_load<int64_t>(tile_first, (size_t)t + 1));
        uint64_t head[DSWX_BURN_HEAD_WORDS] = {(uint64_t)count, 0, 0, 0, 0, 0, 0, 0};
        std::fill(acc.begin(), acc.end(), 0u);
        for (int64_t i = 0; i < count; ++i) {
            const dswx_burn_vertex_t v = dswx_load<dswx_burn_vertex_t>(verts, (size_t)(first + i));
            if ((int64_t)v.next >= count) {
                ++head[BURN_HEAD_MALFORMED];
                continue;
            }
            const dswx_burn_vertex_t w = dswx_load<dswx_burn_vertex_t>(verts, (size_t)(first + (int64_t)v.next));
            if (!burn_legal(v.x) || !burn_legal(v.y) || !burn_legal(w.x) || !burn_legal(w.y)) {
                ++head[BURN_HEAD_MALFORMED];
                continue;
            }
            BurnEdge e;
            if (!burn_edge(v.x, v.y, w.x, w.y, height, &e)) continue;
            ++head[BURN_HEAD_EDGES];
            for (int64_t r = e.r0; r < e.r1; ++r) {      // one division per crossing: no stepping here
                int64_t col = burn_column(burn_cross(e, r));
                if (col < 0) col = 0, ++head[BURN_HEAD_CLAMPED];
                if (col < width) {
                    acc[(size_t)(r * width + col)] ^= v.word;
                    ++head[BURN_HEAD_TOGGLES];
                } else
                    ++head[BURN_HEAD_DROPPED];
            }
        }
        uint8_t* const mask = out->mask ? out->mask + (size_t)t * (size_t)mask_stride : nullptr;
        const uint8_t* const other = src ? src + (size_t)t * (size_t)src_stride : nullptr;
        for (int64_t r = 0; r < height; ++r) {
            uint32_t run = 0;
            for (int64_t c = 0; c < width; ++c) {
                const size_t p = (size_t)(r * width + c);
                run ^= acc[p];
                acc[p] = run;
                head[BURN_HEAD_INSIDE] += run != 0u;
                if (mask) mask[p] = (uint8_t)(run ? spec->burn : other ? (int)other[p] : spec->background);
            }
        }
        if (n) std::memcpy(reinterpret_cast<unsigned char*>(out->acc) + (size_t)t * (size_t)n * 4, acc.data(), (size_t)n * 4);
        if (out->head)
            for (int w = 0; w < DSWX_BURN_HEAD_WORDS; ++w) dswx_store<uint64_t>(out->head, (size_t)(t * DSWX_BURN_HEAD_WORDS + w), head[w]);
    }
    return DSWX_OK;
}

int dswx_burn_device(dswx_ctx_t* ctx, const dswx_burn_vertex_t* verts, const int64_t* tile_first, const dswx_burn_spec_t* spec, int64_t n_tiles,
                     int64_t height, int64_t width, const uint8_t* src, const dswx_burn_out_t* out, void* stream) {
    int64_t mask_stride, src_stride;
    if (int rc = dswx_burn_check(verts, tile_first, spec, n_tiles, height, width, src, out, &mask_stride, &src_stride, true)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) {
        return dswx_burn_launch(ctx, verts, tile_first, spec, n_tiles, height, width, src, mask_stride, src_stride, out, s);
    });
}

}  // extern "C"
