// dswx_grid.hip -- a plane aggregated onto a coarse grid (DSWX_HAS_GRID, additive to ABI v7): per cell of cell_h x cell_w
// pixels the per-category counts and, from them, share, coverage and majority category, without the plane crossing PCIe.
// include/dswx_hip.h "grid" states the definition; proteus_amd/grid.py is its numpy statement and dswx_grid_host below the
// scalar one -- dswx_grid_rule.h is compiled for both sides, so the host entry and the kernel cannot differ.
//
// The first analytic kernel that knows a tile is a raster.  ONE launch: grid.y walks the tiles, grid.x the JOBS of a tile.
// A job is a rectangle of whole cells, crj cell rows x cpj cell columns, and belongs to ONE workgroup: it counts the job's
// cells in LDS (four uint32 per cell, zeroed by the block), and after a barrier thread c derives share, coverage and majority
// of cell c from its four counts and writes them with plain stores -- every wanted output element is written exactly once,
// so there is no zeroing pass, no global atomic and no second pass, and an output that is not wanted costs no store.
//
// THE WALK.  A thread owns one UNIT -- up to 16 consecutive columns, one 16-byte load through the under-aligned vector type
// (gfx950 performs unaligned 16-byte global accesses in hardware: rows start at any byte address) -- and walks DOWN the rows
// of the job with GRID_U = 4 loads in flight, because down a column the cell a byte belongs to changes only every cell_h
// rows.  Where a job has fewer than 256 units in a row (narrow rasters, wide cells) the rows are dealt out in contiguous
// chunks to 256 / units groups of threads; where it has more (one cell wider than 4096 columns) a thread walks several units.
//   cell_w >= 16 (dswx_grid_k<false>).  The units of a cell belong to IT alone: they start at the multiple of 4 columns at or
// before its left edge (so that a load is dword-aligned wherever the rows are: 30-column cells start at 2 mod 4 every other
// time; DESIGN.md section 5 has what that measured) and there are ceil((cell_w + 0 .. 3) / 16) per cell.  The first
// load of a cell may begin in the cell before and the last one reads on into the cell after or the next row -- bytes of the
// same tile, never before its start or past height * width -- which are replaced before they are counted: one v_bfi per
// dword puts the spec's NEUTRAL byte (one that is not an observation, if the table has one) where the unit does not reach,
// and where every byte is an observation the known number of replaced bytes is taken off the neutral byte's field again at
// the flush.  A straddled cell boundary inside a load and a straddled row end are the same case, and both are exact.
//   cell_w < 16 (dswx_grid_k<true>).  A unit covers up to 16 cells, so units are plain runs of 16 columns from the job's left
// edge and every observed byte is one LDS atomic on its cell, as in the histogram kernel.  Bytes behind the row end are
// skipped by index.  This is the regime where the OUTPUT is as large as the input; it is recorded, not tuned.
//   The last 16-byte load of a tile would end behind height * width: a round of loads that could reach that far reads its
// valid bytes one by one instead.  No byte outside [tile, tile + height * width) is ever read.
//
// COUNTING WITHOUT A BRANCH PER CATEGORY.  As in the stack kernel the block widens cat_of_byte once into a table of INCREMENTS
// in LDS, here 256 x uint32 with four 8-bit fields: 1 << (8 * category), or 0 for a byte that is not an observation
// (grid_increment), in GRID_REPLICAS = 8 lane-indexed replicas (tab[byte][replica], lane l reads replica l & 7: the bank of
// a ds_read_b32 is then 8 (byte mod 4) + (l & 7), so only lanes with equal l & 7 can meet, and only where their bytes differ
// and agree modulo 4; class planes, a handful of byte values, read by broadcast -- dswx_stack.hip has the full argument, the
// table is half its size here).  Per byte: extract, form the LDS address, ds_read_b32, one 32-bit add.
//   FIELD WIDTHS.  A thread sums the increments of a unit and of the rows below it in ONE uint32.  An 8-bit field grows by at
// most 16 per unit (replaced bytes included), so after GRID_ROWS_PACKED = 15 units -- 240 <= 255 -- or at the last row of a
// cell the thread WIDENS: it takes the replaced bytes off (at most 15 x 15 = 225 in one field, never more than the field
// holds) and adds each non-zero field to the cell's uint32 counter in LDS (ds_add_u32).  A counter holds a whole cell, at
// most DSWX_GRID_MAX_CELL_PIXELS = 2^24, and 100 x 2^24 < 2^32 for share and coverage.  Nothing carries between fields.
//
// GEOMETRY (grid_geometry, named in dswx_last_kernel_info).  cpj = the whole cells that fit 256 units (cell_w >= 16) or 1024
// columns (cell_w < 16), at least one; crj = the cell rows that make 32 pixel rows, within GRID_MAX_CELLS = 2048 cells of LDS
// (32 KiB, dynamic: a launch asks for what its job needs, 16 bytes per cell).  30 x 30 cells on a 3660-wide tile: one job =
// 2 x 122 cells, 244 threads walk 60 rows (jobs of 5 x 122 cells, 150 rows, measured 8 % SLOWER: docs/HISTORY.md section
// 17); 128 x 128: 1 x 29 cells, 232 threads walk 128 rows.  Very large cells leave one job per cell row band -- a whole tile as one cell is ONE
// workgroup per tile: correct, not fast; dswx_batch_histogram is the entry for that.  (DESIGN.md section 5 has the rates.)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#include "dswx_host.h"
#include "dswx_grid_rule.h"

namespace {

typedef u32x4 __attribute__((aligned(1))) u32x4_b;      // 16 bytes anywhere

constexpr int GRID_BLOCK = 256;                          // threads: one table entry each at the start
constexpr int GRID_PPU = 16;                             // columns per unit = bytes per load
constexpr int GRID_U = 4;                                // loads (rows) in flight per thread
constexpr int GRID_REPLICAS = 8;                         // of the increment table: lane l reads replica l & 7
constexpr int GRID_ROWS_PACKED = 15;                     // units summed in 8-bit fields before they are widened
constexpr int GRID_MAX_CELLS = 2048;                     // of a job: 16 bytes of LDS each
constexpr int GRID_SMALL_COLS = 1024;                    // columns of a job when cell_w < 16
constexpr int GRID_TARGET_ROWS = 32;                     // pixel rows a job should have at least
constexpr int64_t GRID_MAX_SIDE = 1LL << 30;             // height, width
static_assert(GRID_BLOCK == 256, "the table has one entry per thread of a block");
static_assert(GRID_ROWS_PACKED * GRID_PPU <= (int)GRID_PACKED_MAX, "an 8-bit field holds the units summed before widening");
static_assert(100ull * DSWX_GRID_MAX_CELL_PIXELS < (1ull << 32), "100 * count in 32 bits");

struct GridArgs {
    const unsigned char* plane;
    unsigned long long stride;                           // bytes between tiles
    unsigned long long n_elems;                          // height * width
    long long n_tiles;
    int height, width;
    int cell_h, cell_w;                                  // (at most height, width)
    int gh, gw;                                          // cells of a tile
    int crj, cpj;                                        // cell rows / cell columns of a job
    int jx;                                              // jobs across; grid.x = jx * jobs down
    int upc;                                             // cell_w >= 16: units of a whole cell
    int n_cats;
    unsigned neutral;                                    // the byte put where a short unit ends
    unsigned* count[DSWX_GRID_MAX_CATS];
    unsigned char* share;
    unsigned char* coverage;
    unsigned char* major;
    unsigned char cat_of_byte[256];
};
static_assert(sizeof(GridArgs) <= 4096, "kernel arguments");

struct GridGeometry {
    int cell_h, cell_w, gh, gw, crj, cpj, jx, jy, upc;
    bool small;
};

GridGeometry grid_geometry(int64_t height, int64_t width, int64_t cell_h, int64_t cell_w) {
    GridGeometry g = {};
    g.cell_h = (int)(cell_h < height ? cell_h : height);
    g.cell_w = (int)(cell_w < width ? cell_w : width);
    g.gh = (int)((height + g.cell_h - 1) / g.cell_h);
    g.gw = (int)((width + g.cell_w - 1) / g.cell_w);
    g.small = g.cell_w < GRID_PPU;
    // the units of a cell start at the multiple of 4 columns at or before its left edge: up to 3 columns (2 for an even
    // cell_w, none for a multiple of 4) belong to the cell before
    const int head = g.cell_w % 4 == 0 ? 0 : g.cell_w % 2 == 0 ? 2 : 3;
    g.upc = (g.cell_w + head + GRID_PPU - 1) / GRID_PPU;
    int cpj = g.small ? GRID_SMALL_COLS / g.cell_w : GRID_BLOCK / g.upc;
    if (cpj < 1) cpj = 1;
    g.cpj = cpj < g.gw ? cpj : g.gw;
    int crj = (GRID_TARGET_ROWS + g.cell_h - 1) / g.cell_h;
    if (crj > GRID_MAX_CELLS / g.cpj) crj = GRID_MAX_CELLS / g.cpj;
    if (crj < 1) crj = 1;
    g.crj = crj < g.gh ? crj : g.gh;
    g.jx = (g.gw + g.cpj - 1) / g.cpj;
    g.jy = (g.gh + g.crj - 1) / g.crj;
    return g;
}

// The 16 bytes at `off` of a tile; `checked`: the load might end behind the tile, then the valid bytes lo .. hi - 1 one by one.
__device__ __forceinline__ u32x4 grid_load(const unsigned char* tile, unsigned long long off, unsigned long long n_elems, int lo,
                                           int hi, bool checked) {
    if (!checked || off + GRID_PPU <= n_elems) return ldg_u<u32x4_b, u32x4, false>(tile + off);
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < GRID_PPU; ++i)
        if (i >= lo && i < hi) v[i / 4] |= (uint32_t)tile[off + i] << (8 * (i % 4));
    return v;
}

// widen: the packed sum of a thread into the four counters of its cell; `replaced` bytes were counted as the neutral byte
__device__ __forceinline__ void grid_flush(unsigned* cell, uint32_t acc, uint32_t replaced, uint32_t inc_neutral) {
    acc -= replaced * inc_neutral;
#pragma unroll
    for (int k = 0; k < DSWX_GRID_MAX_CATS; ++k) {
        const uint32_t f = grid_field(acc, k);
        if (f) atomicAdd(cell + k, f);
    }
}

// The state of a thread walking down its unit: which cell row of the job it is in and how many rows of it are left.
struct GridWalk {
    int gyl, left;
    uint32_t acc;
    int nacc;
};

// cell_w >= 16: one unit (already masked to its cell) into the packed sum; widened when full or at the last row of a cell
__device__ __forceinline__ void grid_unit_big(const GridArgs& a, const u32x4& v, const uint32_t (&keep)[4], const uint32_t (&fillv)[4],
                                              const uint32_t* mine, unsigned* cnt, int ncc, int lc, uint32_t per_row_replaced,
                                              uint32_t inc_neutral, GridWalk& w) {
    uint32_t inc[GRID_PPU];
#pragma unroll
    for (int i = 0; i < GRID_PPU; ++i) {
        const uint32_t d = (v[i / 4] & keep[i / 4]) | fillv[i / 4];
        inc[i] = mine[((d >> (8 * (i % 4))) & 0xffu) * GRID_REPLICAS];
    }
#pragma unroll
    for (int i = 0; i < GRID_PPU; ++i) w.acc += inc[i];
    ++w.nacc;
    --w.left;
    if (w.nacc == GRID_ROWS_PACKED || w.left == 0) {
        grid_flush(cnt + (w.gyl * ncc + lc) * DSWX_GRID_MAX_CATS, w.acc, (uint32_t)w.nacc * per_row_replaced, inc_neutral);
        w.acc = 0;
        w.nacc = 0;
        if (w.left == 0) {
            ++w.gyl;
            w.left = a.cell_h;
        }
    }
}

// cell_w < 16: every observed byte of the unit is one atomic on its cell (cidx = the cell column of byte i inside the job)
__device__ __forceinline__ void grid_unit_small(const GridArgs& a, const u32x4& v, int nv, const int (&cidx)[GRID_PPU],
                                                const uint32_t* mine, unsigned* cnt, int ncc, GridWalk& w) {
    unsigned* const row = cnt + w.gyl * ncc * DSWX_GRID_MAX_CATS;
#pragma unroll
    for (int i = 0; i < GRID_PPU; ++i) {
        if (i < nv) {
            const uint32_t inc = mine[((v[i / 4] >> (8 * (i % 4))) & 0xffu) * GRID_REPLICAS];
            if (inc) atomicAdd(row + cidx[i] * DSWX_GRID_MAX_CATS + ((__ffs(inc) - 1) >> 3), 1u);
        }
    }
    if (--w.left == 0) {
        ++w.gyl;
        w.left = a.cell_h;
    }
}

// Unit u of a job down the rows ra .. rb - 1 (r0: the job's first row; c0 .. c1 - 1: its columns).
template <bool SMALL>
__device__ __forceinline__ void grid_walk(const GridArgs& a, const unsigned char* tile, const uint32_t* mine, unsigned* cnt, int u,
                                          int ra, int rb, int r0, int c0, int c1, int ncc, uint32_t inc_neutral) {
    int lc = 0, col, lo = 0, hi;                         // the unit: columns col .. col + 15, of which lo .. hi - 1 are counted
    if (SMALL) {
        col = c0 + u * GRID_PPU;
        hi = c1 - col;
    } else {
        lc = u / a.upc;
        const int left = c0 + lc * a.cell_w, right = left + a.cell_w < c1 ? left + a.cell_w : c1;
        col = (left & ~3) + (u - lc * a.upc) * GRID_PPU;   // a multiple of 4 columns: dword-aligned where the rows are
        lo = left > col ? left - col : 0;
        hi = right - col;
    }
    if (hi > GRID_PPU) hi = GRID_PPU;
    if (hi <= lo) return;                                 // (a cell does not need every one of its units)
    const int nv = hi - lo;
    uint32_t keep[4], fillv[4];
    int cidx[GRID_PPU];
    if (SMALL) {
#pragma unroll
        for (int i = 0; i < GRID_PPU; ++i) cidx[i] = (u * GRID_PPU + i) / a.cell_w;
    } else {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int n = hi - 4 * d, m = lo - 4 * d;
            keep[d] = (n >= 4 ? 0xffffffffu : n <= 0 ? 0u : (1u << (8 * n)) - 1u) & ~(m >= 4 ? 0xffffffffu : m <= 0 ? 0u : (1u << (8 * m)) - 1u);
            fillv[d] = (a.neutral * 0x01010101u) & ~keep[d];
        }
    }
    GridWalk w;
    w.gyl = (ra - r0) / a.cell_h;
    w.left = a.cell_h - ((ra - r0) - w.gyl * a.cell_h);
    w.acc = 0;
    w.nacc = 0;
    const uint32_t per_row_replaced = (uint32_t)(GRID_PPU - nv);
    unsigned long long off = (unsigned long long)ra * (unsigned long long)a.width + (unsigned long long)col;
    const unsigned long long pitch = (unsigned long long)a.width;
    for (int r = ra; r < rb; r += GRID_U, off += GRID_U * pitch) {
        u32x4 v[GRID_U];
        // a whole round whose last load ends inside the tile: the loads first, without a condition, then the counting
        const bool whole = r + GRID_U <= rb && off + (GRID_U - 1) * pitch + GRID_PPU <= a.n_elems;
        if (whole) {
#pragma unroll
            for (int j = 0; j < GRID_U; ++j) v[j] = grid_load(tile, off + j * pitch, a.n_elems, lo, hi, false);
        } else {
#pragma unroll
            for (int j = 0; j < GRID_U; ++j) {
                v[j] = u32x4{0u, 0u, 0u, 0u};
                if (r + j < rb) v[j] = grid_load(tile, off + j * pitch, a.n_elems, lo, hi, true);
            }
        }
#pragma unroll
        for (int j = 0; j < GRID_U; ++j) {
            if (whole || r + j < rb) {
                if (SMALL) grid_unit_small(a, v[j], hi, cidx, mine, cnt, ncc, w);
                else grid_unit_big(a, v[j], keep, fillv, mine, cnt, ncc, lc, per_row_replaced, inc_neutral, w);
            }
        }
    }
    if (!SMALL && w.nacc)
        grid_flush(cnt + (w.gyl * ncc + lc) * DSWX_GRID_MAX_CATS, w.acc, (uint32_t)w.nacc * per_row_replaced, inc_neutral);
}

template <bool SMALL>
__global__ __launch_bounds__(GRID_BLOCK) void dswx_grid_k(const GridArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[256 * GRID_REPLICAS];
    extern __shared__ __attribute__((aligned(16))) unsigned cnt[];           // [cell rows][cell columns][4] of this job
    {
        const uint32_t inc = grid_increment(a.cat_of_byte, a.n_cats, threadIdx.x);
#pragma unroll
        for (int r = 0; r < GRID_REPLICAS; ++r) tab[threadIdx.x * GRID_REPLICAS + r] = inc;
    }
    const uint32_t* const mine = tab + (threadIdx.x & (GRID_REPLICAS - 1));
    const uint32_t inc_neutral = grid_increment(a.cat_of_byte, a.n_cats, a.neutral);
    const int tid = (int)threadIdx.x;
    const int jyi = (int)(blockIdx.x / (unsigned)a.jx), jxi = (int)(blockIdx.x - (unsigned)jyi * (unsigned)a.jx);
    const int gy0 = jyi * a.crj, gx0 = jxi * a.cpj;
    const int ncr = a.gh - gy0 < a.crj ? a.gh - gy0 : a.crj;
    const int ncc = a.gw - gx0 < a.cpj ? a.gw - gx0 : a.cpj;
    const int ncell = ncr * ncc;
    const int r0 = gy0 * a.cell_h, c0 = gx0 * a.cell_w;
    // (cell_h <= height <= 2^30 and gh * cell_h < height + cell_h: the products fit an int)
    const int r1 = (gy0 + ncr) * a.cell_h < a.height ? (gy0 + ncr) * a.cell_h : a.height;
    const int c1 = (gx0 + ncc) * a.cell_w < a.width ? (gx0 + ncc) * a.cell_w : a.width;
    const int nu = SMALL ? (c1 - c0 + GRID_PPU - 1) / GRID_PPU : ncc * a.upc;
    // fewer units than threads: the rows in contiguous chunks to GRID_BLOCK / nu groups of threads
    const int groups = nu < GRID_BLOCK ? GRID_BLOCK / nu : 1;
    const int rs = nu < GRID_BLOCK ? tid / nu : 0;
    const int chunk = (r1 - r0 + groups - 1) / groups;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        for (int i = tid; i < ncell * DSWX_GRID_MAX_CATS; i += GRID_BLOCK) cnt[i] = 0u;
        __syncthreads();                                 // (the first time round: the table too)
        const unsigned char* const tile = a.plane + (unsigned long long)t * a.stride;
        if (nu >= GRID_BLOCK) {
            for (int u = tid; u < nu; u += GRID_BLOCK) grid_walk<SMALL>(a, tile, mine, cnt, u, r0, r1, r0, c0, c1, ncc, inc_neutral);
        } else if (rs < groups) {
            const int ra = r0 + rs * chunk;
            const int rb = ra + chunk < r1 ? ra + chunk : r1;
            if (ra < rb) grid_walk<SMALL>(a, tile, mine, cnt, tid - rs * nu, ra, rb, r0, c0, c1, ncc, inc_neutral);
        }
        __syncthreads();
        // thread c: cell c of the job, from its four counts
        for (int c = tid; c < ncell; c += GRID_BLOCK) {
            const int ly = c / ncc, gy = gy0 + ly, gx = gx0 + (c - ly * ncc);
            const u32x4 q = *reinterpret_cast<const u32x4*>(cnt + c * DSWX_GRID_MAX_CATS);
            const uint32_t count[DSWX_GRID_MAX_CATS] = {q.x, q.y, q.z, q.w};
            const int ph = a.height - gy * a.cell_h < a.cell_h ? a.height - gy * a.cell_h : a.cell_h;
            const int pw = a.width - gx * a.cell_w < a.cell_w ? a.width - gx * a.cell_w : a.cell_w;
            const unsigned long long o = ((unsigned long long)t * (unsigned long long)a.gh + (unsigned long long)gy) *
                                         (unsigned long long)a.gw + (unsigned long long)gx;
#pragma unroll
            for (int k = 0; k < DSWX_GRID_MAX_CATS; ++k)
                if (a.count[k]) a.count[k][o] = count[k];
            if (a.share) a.share[o] = (unsigned char)grid_share(count);
            if (a.coverage) a.coverage[o] = (unsigned char)grid_coverage(count, (uint32_t)ph * (uint32_t)pw);
            if (a.major) a.major[o] = (unsigned char)grid_major(count);
        }
        __syncthreads();                                 // (the counters are zeroed again for the next tile)
    }
}

}  // namespace

// The checks that the device and the host entry share, in the house order: the arguments before any context, nothing
// written by a refused call.  `align` = the uint32 outputs must be 4-byte aligned (the device entry).
int dswx_grid_check(const uint8_t* plane, const dswx_grid_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                    int64_t* stride, const dswx_grid_out_t* out, bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (spec->n_cats < 1 || spec->n_cats > DSWX_GRID_MAX_CATS)
        return dswx_fail(DSWX_ERR_ARG, "n_cats %d outside 1 .. %d", spec->n_cats, DSWX_GRID_MAX_CATS);
    if (spec->cell_h < 1 || spec->cell_w < 1) return dswx_fail(DSWX_ERR_ARG, "cell %d x %d: sizes below 1", spec->cell_h, spec->cell_w);
    if (n_tiles < 0 || height < 0 || width < 0 || *stride < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (height > GRID_MAX_SIDE || width > GRID_MAX_SIDE) return dswx_fail(DSWX_ERR_ARG, "raster too large");
    const int64_t n_elems = height * width;
    if (int rc = dswx_tile_stride_check(stride, n_elems)) return rc;
    if (int rc = dswx_tile_extent_check(*stride, n_tiles, true)) return rc;
    const int64_t ch = spec->cell_h < height ? spec->cell_h : height, cw = spec->cell_w < width ? spec->cell_w : width;
    if (ch * cw > DSWX_GRID_MAX_CELL_PIXELS)
        return dswx_fail(DSWX_ERR_ARG, "a cell of %lld x %lld pixels is above DSWX_GRID_MAX_CELL_PIXELS (%d)", (long long)ch,
                         (long long)cw, DSWX_GRID_MAX_CELL_PIXELS);
    if (int rc = dswx_tile_plane_check(plane, n_tiles, n_elems)) return rc;
    if (int rc = dswx_outputs_check(out->count, DSWX_GRID_MAX_CATS, spec->n_cats, out->share || out->coverage || out->major)) return rc;
    if (align)
        for (int k = 0; k < DSWX_GRID_MAX_CATS; ++k)
            if (!aligned_to(out->count[k], 4)) return dswx_fail(DSWX_ERR_ALIGN, "count[%d] not 4-byte aligned", k);
    return DSWX_OK;
}

// One launch; the arguments have passed dswx_grid_check (stride resolved).
int dswx_grid_launch(dswx_ctx* ctx, const uint8_t* plane, const dswx_grid_spec_t* spec, int64_t n_tiles, int64_t height,
                     int64_t width, int64_t stride, const dswx_grid_out_t* out, hipStream_t s) {
    if (n_tiles == 0 || height == 0 || width == 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    const GridGeometry g = grid_geometry(height, width, spec->cell_h, spec->cell_w);
    // (grid.x x 256 threads must stay below 2^32: the runtime refuses a larger launch)
    if ((int64_t)g.jx * g.jy * GRID_BLOCK >= (1LL << 32)) return dswx_fail(DSWX_ERR_ARG, "too many cells in a tile");
    GridArgs a = {};
    a.plane = plane;
    a.stride = (unsigned long long)stride;
    a.n_elems = (unsigned long long)(height * width);
    a.n_tiles = n_tiles;
    a.height = (int)height;
    a.width = (int)width;
    a.cell_h = g.cell_h;
    a.cell_w = g.cell_w;
    a.gh = g.gh;
    a.gw = g.gw;
    a.crj = g.crj;
    a.cpj = g.cpj;
    a.jx = g.jx;
    a.upc = g.upc;
    a.n_cats = spec->n_cats;
    a.neutral = 0;
    for (int b = 0; b < 256; ++b)
        if (spec->cat_of_byte[b] >= spec->n_cats) {
            a.neutral = (unsigned)b;
            break;
        }
    for (int k = 0; k < DSWX_GRID_MAX_CATS; ++k) a.count[k] = out->count[k];
    a.share = out->share;
    a.coverage = out->coverage;
    a.major = out->major;
    std::memcpy(a.cat_of_byte, spec->cat_of_byte, 256);
    const unsigned gy = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
    const size_t lds = (size_t)g.crj * (size_t)g.cpj * DSWX_GRID_MAX_CATS * sizeof(unsigned);
    const dim3 grid((unsigned)(g.jx * g.jy), gy), block(GRID_BLOCK);
    if (g.small) hipLaunchKernelGGL(dswx_grid_k<true>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(dswx_grid_k<false>, grid, block, lds, s, a);
    HIP_TRY(hipGetLastError());
    char info[256];
    snprintf(info, sizeof info, "dswx_grid_k grid=(%d,%u,1) block=%d cells=%dx%d job_cells=%dx%d small=%d rows_in_flight=%d replicas=%d",
             g.jx * g.jy, gy, GRID_BLOCK, g.gh, g.gw, g.crj, g.cpj, g.small ? 1 : 0, GRID_U, GRID_REPLICAS);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_grid_host(const uint8_t* plane, const dswx_grid_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                   int64_t stride, const dswx_grid_out_t* out) {
    if (int rc = dswx_grid_check(plane, spec, n_tiles, height, width, &stride, out, false)) return rc;
    if (n_tiles == 0 || height == 0 || width == 0) return DSWX_OK;
    const int64_t ch = spec->cell_h < height ? spec->cell_h : height, cw = spec->cell_w < width ? spec->cell_w : width;
    const int64_t gh = (height + ch - 1) / ch, gw = (width + cw - 1) / cw;
    uint32_t inc_of[256];
    for (int b = 0; b < 256; ++b) inc_of[b] = grid_increment(spec->cat_of_byte, spec->n_cats, (unsigned)b);
    for (int64_t t = 0; t < n_tiles; ++t) {
        const uint8_t* tile = plane + (size_t)t * (size_t)stride;
        for (int64_t gy = 0; gy < gh; ++gy) {
            const int64_t ra = gy * ch, rb = ra + ch < height ? ra + ch : height;
            for (int64_t gx = 0; gx < gw; ++gx) {
                const int64_t ca = gx * cw, cb = ca + cw < width ? ca + cw : width;
                uint32_t count[DSWX_GRID_MAX_CATS] = {0, 0, 0, 0};
                for (int64_t r = ra; r < rb; ++r) {
                    const uint8_t* p = tile + (size_t)r * (size_t)width;
                    for (int64_t c = ca; c < cb; ++c) {
                        const uint32_t inc = inc_of[p[c]];
                        for (int k = 0; k < DSWX_GRID_MAX_CATS; ++k) count[k] += grid_field(inc, k);
                    }
                }
                const int64_t o = (t * gh + gy) * gw + gx;
                for (int k = 0; k < DSWX_GRID_MAX_CATS; ++k)
                    if (out->count[k]) dswx_store<uint32_t>(out->count[k], (size_t)o, count[k]);
                if (out->share) out->share[o] = (uint8_t)grid_share(count);
                if (out->coverage) out->coverage[o] = (uint8_t)grid_coverage(count, (uint32_t)((rb - ra) * (cb - ca)));
                if (out->major) out->major[o] = (uint8_t)grid_major(count);
            }
        }
    }
    return DSWX_OK;
}

int dswx_grid_device(dswx_ctx_t* ctx, const uint8_t* plane, const dswx_grid_spec_t* spec, int64_t n_tiles, int64_t height,
                     int64_t width, int64_t stride, const dswx_grid_out_t* out, void* stream) {
    if (int rc = dswx_grid_check(plane, spec, n_tiles, height, width, &stride, out, true)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) { return dswx_grid_launch(ctx, plane, spec, n_tiles, height, width, stride, out, s); });
}

}  // extern "C"
