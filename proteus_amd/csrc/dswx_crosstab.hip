// dswx_crosstab.hip -- per-tile cross-tabulation of two planes (DSWX_HAS_CROSSTAB, additive to ABI v7): how the classes of
// plane A fall into the classes of plane B, 256 cells per tile, without either plane crossing PCIe.  include/dswx_hip.h
// "crosstab" states the definition; proteus_amd/crosstab.py is its numpy statement and dswx_crosstab_host below the scalar
// one -- hist_bin (dswx_hist_bin.h, shared with dswx_histogram.hip) and cross_cell are compiled for both sides, so the host
// entry and the kernel cannot differ, and a bin here is a bin of the histogram.
//
// The kernel is dswx_histogram_k's shape with dswx_compare_k's two read streams: one launch covers n_pairs x n_tiles through
// the pair table in its arguments (grid.z = pair, grid.y = tile, grid.x = chunks of a tile); A's kind, lo and shift, col_bits
// and the two 256-byte tables of a pair sit in its table entry and are uniform per block, so one launch mixes kinds and
// specifications.  A thread handles 16 element pairs per step: one 16-byte unit of B and one (byte planes) or two (16-bit
// planes) 16-byte units of A, read through the under-aligned vector type -- A and B have their own address and stride, so
// their residues differ; gfx950 performs unaligned 16-byte global accesses in hardware -- with CROSS_UNROLL steps' loads of
// both streams in flight before the first use.  The pairs behind the last whole step of a tile are counted by thread 0 of
// block 0 of that tile.  The records are zeroed on the stream in front of the kernel.  No scratch of the context: the
// entries own nothing, so they need no ordering against its other launches.
//
// THE TABLES.  A block turns its pair's tables into two LDS tables of 256 uint16 once: rowt[bin] = row << col_bits (the row
// premultiplied by the number of columns) and colt[byte] = col, each CROSS_OUT = 0x8000 where the definition excludes the
// entry (row >= R, col >= C).  A cell is then ONE add of two lookups, and "counted" is ONE compare: row * C + col <= 255
// for a counted pair, and a sum with an excluded side is at least 0x8000.  The lookups are ds_read_u16: equal addresses
// broadcast, different entries of one bank (a table spans 128 dwords, four per bank) serialise -- class planes, whose
// lanes mostly agree, pay nothing; a band of noise as A pays up to fourfold on the ROW lookup.  DESIGN section 5 has what
// that costs.
//
// THE ACCUMULATION is dswx_histogram_k's, LANE-INDEXED REPLICAS: a block keeps CROSS_REPLICAS = 32 sets of 256 uint32
// counters in LDS, cnt[cell][replica], and lane l adds to replica l & 31, so the bank of a counter is l & 31 WHATEVER the
// cell: the add is conflict-free for constant planes, for noise and for anything in between (dswx_histogram.hip states the
// argument and the alternatives).  ONE shortcut: a step in which the units of BOTH planes hold one value each is one add
// of 16 -- both, because a constant A over a B that changes inside the unit spreads over several cells.  Flush: thread c
// sums the 32 replicas of cell c (rotated start: 32 banks per half-wave) and adds a non-zero sum to out[pair][tile][c] with
// one 64-bit atomic.
//   COUNTER WIDTH.  A counter is a uint32.  Replica r of a block is fed by the lanes r and r + 32 of its 4 waves: 8
// threads.  A thread counts at most passes <= CROSS_MAX_PASSES = 64 steps of 16 pairs (+ 15 tail pairs for thread 0 of
// block 0): 8 x 64 x 16 + 15 = 8207 per counter at most, and the flush sums 32 of them: 262,159 -- both far below 2^32.
// The sum is widened to 64 bits only for the global add; the records are 64-bit.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#include "dswx_host.h"
#include "dswx_hist_bin.h"

namespace {

static_assert(sizeof(dswx_crosstab_spec_t) == 528 && sizeof(dswx_crosstab_pair_t) == 536, "the public structs");

typedef u32x4 __attribute__((aligned(1))) u32x4_b;      // 16 bytes anywhere

constexpr int CROSS_BLOCK = 256;                         // threads; one pass of a block = 256 steps = 4096 pairs
constexpr int CROSS_UNROLL = 4;                          // steps in flight per thread
constexpr int CROSS_MAX_PASSES = 64;                     // per block: 2^20 pairs of a tile, at most 256 atomics
constexpr int CROSS_REPLICAS = 32;                       // = the dword banks an LDS atomic sees: bank = lane & 31
constexpr int CROSS_STEP = 16;                           // pairs per step: one 16-byte unit of B
constexpr unsigned CROSS_OUT = 0x8000u;                  // table entry of an excluded bin / byte
static_assert(CROSS_BLOCK == DSWX_CROSSTAB_CELLS && DSWX_CROSSTAB_CELLS == DSWX_HIST_BINS, "the flush gives every cell one thread");
static_assert((CROSS_BLOCK / CROSS_REPLICAS) * CROSS_MAX_PASSES * (unsigned long long)CROSS_STEP + 15 < (1ull << 32) / CROSS_REPLICAS,
              "a uint32 counter, and the sum of a cell's replicas, hold the largest chunk of a block");

// the table entries of the definition: the row premultiplied by the number of columns, the column; CROSS_OUT = not counted
__host__ __device__ __forceinline__ unsigned cross_row_entry(unsigned row, int col_bits) {
    return row < (256u >> col_bits) ? row << col_bits : CROSS_OUT;
}
__host__ __device__ __forceinline__ unsigned cross_col_entry(unsigned col, int col_bits) {
    return col < (1u << col_bits) ? col : CROSS_OUT;
}
// THE CELL of a pair from its two table entries; >= DSWX_CROSSTAB_CELLS = not counted.  One function for both sides.
__host__ __device__ __forceinline__ unsigned cross_cell(unsigned row_entry, unsigned col_entry) { return row_entry + col_entry; }

struct CrossPair {
    const unsigned char* a;
    const unsigned char* b;
    unsigned long long n_elems;                          // counted pairs of every tile, from its start
    unsigned long long a_stride_bytes, b_stride_bytes;   // between tiles
    int kind;                                            // DSWX_HIST_* of plane a
    int lo, shift;                                       // U16 / I16
    int col_bits;
    unsigned char row_of_bin[256], col_of_byte[256];
};
struct CrossArgs {
    CrossPair pair[DSWX_CROSSTAB_MAX_PAIRS];
    unsigned long long* out;                             // [n_pairs][out_pitch][DSWX_CROSSTAB_CELLS]
    long long out_pitch;                                 // tiles
    int passes;                                          // per block, a multiple of CROSS_UNROLL
};
static_assert(sizeof(CrossArgs) <= 4096, "kernel arguments");

struct CrossLds {
    unsigned* mine;                                      // cnt + (lane & 31); cell c is mine[c * CROSS_REPLICAS]
    const unsigned short* rowt;
    const unsigned short* colt;
};

template <int KIND> __device__ __forceinline__ void cross_one(unsigned raw, unsigned y, const CrossLds& l, int lo, int shift,
                                                              unsigned n) {
    const int bin = hist_bin<KIND>(raw, lo, shift);
    if (bin < 0) return;
    const unsigned cell = cross_cell(l.rowt[bin], l.colt[y]);
    if (cell < (unsigned)DSWX_CROSSTAB_CELLS) atomicAdd(l.mine + cell * CROSS_REPLICAS, n);
}

__device__ __forceinline__ bool cross_one_value(const u32x4& v, int elem_bytes) {
    const unsigned turned = (v.x >> (8 * elem_bytes)) | (v.x << (32 - 8 * elem_bytes));
    return v.x == v.y && v.x == v.z && v.x == v.w && v.x == turned;
}

// the A units of one step: 16 elements
template <int KIND> struct CrossA { u32x4 v[HistElem<KIND>::BYTES]; };

// one step (16 pairs) into the thread's replica
template <int KIND> __device__ __forceinline__ void cross_step(const CrossA<KIND>& va, const u32x4& vb, const CrossLds& l, int lo,
                                                               int shift) {
    constexpr int EB = HistElem<KIND>::BYTES, EPW = 4 / EB;
    constexpr unsigned MASK = EB == 1 ? 0xffu : 0xffffu;
    bool one = cross_one_value(vb, 1) && cross_one_value(va.v[0], EB);
    if constexpr (EB == 2) one = one && cross_one_value(va.v[1], EB) && va.v[0].x == va.v[1].x;
    if (one) {                                           // one value in BOTH planes: one add
        cross_one<KIND>(va.v[0].x & MASK, vb.x & 0xffu, l, lo, shift, (unsigned)CROSS_STEP);
        return;
    }
#pragma unroll
    for (int i = 0; i < CROSS_STEP; ++i) {
        const unsigned wa = va.v[(i / EPW) / 4][(i / EPW) % 4];
        cross_one<KIND>((wa >> (8 * EB * (i % EPW))) & MASK, (vb[i / 4] >> (8 * (i % 4))) & 0xffu, l, lo, shift, 1u);
    }
}

// CROSS_UNROLL steps of one thread, CROSS_BLOCK steps apart, from step u: the loads of both streams first, then the counting
template <int KIND, bool WHOLE>
__device__ __forceinline__ void cross_round(const unsigned char* ta, const unsigned char* tb, unsigned long long u,
                                            unsigned long long steps, const CrossLds& l, int lo, int shift) {
    constexpr int EB = HistElem<KIND>::BYTES;
    CrossA<KIND> va[CROSS_UNROLL];
    u32x4 vb[CROSS_UNROLL];
#pragma unroll
    for (int j = 0; j < CROSS_UNROLL; ++j) {
        const unsigned long long uj = u + (unsigned long long)j * CROSS_BLOCK;
#pragma unroll
        for (int h = 0; h < EB; ++h) va[j].v[h] = u32x4{0u, 0u, 0u, 0u};
        vb[j] = u32x4{0u, 0u, 0u, 0u};
        if (WHOLE || uj < steps) {
#pragma unroll
            for (int h = 0; h < EB; ++h) va[j].v[h] = ldg_u<u32x4_b, u32x4, true>(ta + uj * (16 * EB) + 16 * h);
            vb[j] = ldg_u<u32x4_b, u32x4, true>(tb + uj * 16);
        }
    }
#pragma unroll
    for (int j = 0; j < CROSS_UNROLL; ++j) {
        const unsigned long long uj = u + (unsigned long long)j * CROSS_BLOCK;
        if (WHOLE || uj < steps) cross_step<KIND>(va[j], vb[j], l, lo, shift);
    }
}

template <int KIND>
__device__ __forceinline__ void cross_tile(int passes, unsigned long long n_elems, const unsigned char* ta, const unsigned char* tb,
                                           const CrossLds& l, int lo, int shift) {
    constexpr int EB = HistElem<KIND>::BYTES;
    const unsigned long long steps = n_elems / CROSS_STEP;
    unsigned long long u = (unsigned long long)blockIdx.x * (unsigned long long)passes * CROSS_BLOCK + threadIdx.x;
    for (int q = 0; q < passes && u - threadIdx.x < steps; q += CROSS_UNROLL) {
        // (wave-uniform: every round of a block but the last of a tile is whole and runs without predicates)
        if (u - threadIdx.x + CROSS_UNROLL * CROSS_BLOCK <= steps) cross_round<KIND, true>(ta, tb, u, steps, l, lo, shift);
        else cross_round<KIND, false>(ta, tb, u, steps, l, lo, shift);
        u += CROSS_UNROLL * CROSS_BLOCK;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the pairs behind the last whole step: fewer than 16, read element by element (A aligned to its element)
        for (unsigned long long e = steps * CROSS_STEP; e < n_elems; ++e) {
            const unsigned raw = EB == 1 ? (unsigned)ta[e] : (unsigned)reinterpret_cast<const unsigned short*>(ta)[e];
            cross_one<KIND>(raw, (unsigned)tb[e], l, lo, shift, 1u);
        }
    }
}

__global__ __launch_bounds__(CROSS_BLOCK) void dswx_crosstab_k(const CrossArgs a) {
    // (the entry of this block's pair is read field by field: a copy of its 568 bytes would not fit the registers)
    const CrossPair& pr = a.pair[blockIdx.z];
    const unsigned long long n_elems = pr.n_elems;
    if ((unsigned long long)blockIdx.x * (unsigned long long)a.passes * CROSS_BLOCK >= n_elems / CROSS_STEP && blockIdx.x != 0)
        return;                                          // (the whole block)
    __shared__ __attribute__((aligned(16))) unsigned cnt[DSWX_CROSSTAB_CELLS * CROSS_REPLICAS];
    __shared__ unsigned short rowt[256], colt[256];
    {
        u32x4* z = reinterpret_cast<u32x4*>(cnt);
#pragma unroll
        for (int j = 0; j < DSWX_CROSSTAB_CELLS * CROSS_REPLICAS / 4 / CROSS_BLOCK; ++j) z[j * CROSS_BLOCK + threadIdx.x] = u32x4{0u, 0u, 0u, 0u};
        const int col_bits = pr.col_bits;
        rowt[threadIdx.x] = (unsigned short)cross_row_entry(pr.row_of_bin[threadIdx.x], col_bits);
        colt[threadIdx.x] = (unsigned short)cross_col_entry(pr.col_of_byte[threadIdx.x], col_bits);
    }
    __syncthreads();
    const unsigned char* const ta = pr.a + (unsigned long long)blockIdx.y * pr.a_stride_bytes;
    const unsigned char* const tb = pr.b + (unsigned long long)blockIdx.y * pr.b_stride_bytes;
    const CrossLds l = {cnt + (threadIdx.x & (CROSS_REPLICAS - 1)), rowt, colt};
    const int lo = pr.lo, shift = pr.shift;
    switch (pr.kind) {                                   // uniform per block
        case DSWX_HIST_U8: cross_tile<DSWX_HIST_U8>(a.passes, n_elems, ta, tb, l, lo, shift); break;
        case DSWX_HIST_U16: cross_tile<DSWX_HIST_U16>(a.passes, n_elems, ta, tb, l, lo, shift); break;
        case DSWX_HIST_I16: cross_tile<DSWX_HIST_I16>(a.passes, n_elems, ta, tb, l, lo, shift); break;
        default: cross_tile<DSWX_HIST_DIAG>(a.passes, n_elems, ta, tb, l, lo, shift); break;
    }
    __syncthreads();
    // thread c sums the replicas of cell c, each lane starting at another one: 32 banks per half-wave
    const unsigned* const row = cnt + threadIdx.x * CROSS_REPLICAS;
    unsigned sum = 0;
#pragma unroll
    for (int j = 0; j < CROSS_REPLICAS; ++j) sum += row[(j + threadIdx.x) & (CROSS_REPLICAS - 1)];
    if (sum) atomicAdd(a.out + (((long long)blockIdx.z * a.out_pitch + blockIdx.y) * DSWX_CROSSTAB_CELLS + threadIdx.x), (unsigned long long)sum);
}

template <int KIND> void cross_host(const void* a, const uint8_t* b, const dswx_crosstab_spec_t& sp, int64_t n, uint64_t* cells) {
    constexpr int EB = HistElem<KIND>::BYTES;
    const unsigned char* p = static_cast<const unsigned char*>(a);
    for (int64_t i = 0; i < n; ++i) {
        unsigned raw;                                    // (memcpy: a host buffer may sit at any address)
        if (EB == 1) raw = p[i];
        else {
            uint16_t h;
            std::memcpy(&h, p + (size_t)i * 2, 2);
            raw = h;
        }
        const int bin = hist_bin<KIND>(raw, sp.a_lo, sp.a_shift);
        if (bin < 0) continue;
        const unsigned cell = cross_cell(cross_row_entry(sp.row_of_bin[bin], sp.col_bits), cross_col_entry(sp.col_of_byte[b[i]], sp.col_bits));
        if (cell < (unsigned)DSWX_CROSSTAB_CELLS) ++cells[cell];
    }
}

}  // namespace

int dswx_crosstab_check_spec(const dswx_crosstab_spec_t* spec) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (int rc = dswx_histogram_check_kind(spec->a_kind, spec->a_shift)) return rc;
    if (spec->col_bits < 0 || spec->col_bits > 8) return dswx_fail(DSWX_ERR_ARG, "col_bits %d outside 0 .. 8", spec->col_bits);
    return DSWX_OK;
}

// `n_pairs` plane pairs x `n_tiles` tiles -> out[n_pairs][n_tiles][256] (device), zeroed on `s` in front of the kernel.  One
// launch (tile counts past the 65535 of grid.y: one per 65535 tiles).
int dswx_crosstab_launch(dswx_ctx* ctx, const dswx_crosstab_item* items, int n_pairs, int64_t n_tiles, uint64_t* out, hipStream_t s) {
    if (n_pairs <= 0 || n_tiles <= 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    if (n_pairs > DSWX_CROSSTAB_MAX_PAIRS) return dswx_fail(DSWX_ERR_ARG, "%d pairs: at most %d per launch", n_pairs, DSWX_CROSSTAB_MAX_PAIRS);
    CrossArgs a = {};
    unsigned long long steps = 0;
    for (int k = 0; k < n_pairs; ++k) {
        CrossPair& pr = a.pair[k];
        const dswx_crosstab_spec_t& sp = *items[k].spec;
        pr.a = static_cast<const unsigned char*>(items[k].a);
        pr.b = static_cast<const unsigned char*>(items[k].b);
        pr.n_elems = items[k].n_elems;
        pr.a_stride_bytes = items[k].a_stride_elems * (unsigned long long)dswx_histogram_elem_bytes(sp.a_kind);
        pr.b_stride_bytes = items[k].b_stride_elems;
        pr.kind = sp.a_kind;
        pr.lo = sp.a_lo;
        pr.shift = sp.a_shift;
        pr.col_bits = sp.col_bits;
        std::memcpy(pr.row_of_bin, sp.row_of_bin, sizeof pr.row_of_bin);
        std::memcpy(pr.col_of_byte, sp.col_of_byte, sizeof pr.col_of_byte);
        if (pr.n_elems / CROSS_STEP > steps) steps = pr.n_elems / CROSS_STEP;
    }
    // the chunk of a block follows the amount of work, as the histogram's: up to 2^20 pairs (at most 256 atomics per chunk),
    // shorter while that leaves fewer than 16 K blocks for the 256 CUs (the records do not depend on the geometry)
    const unsigned long long single = (steps + CROSS_BLOCK - 1) / CROSS_BLOCK;
    int passes = CROSS_MAX_PASSES;
    while (passes > CROSS_UNROLL &&
           ((single + passes - 1) / passes) * (unsigned long long)n_tiles * (unsigned long long)n_pairs < 16384)
        passes /= 2;
    const unsigned long long gx = single ? (single + passes - 1) / passes : 1;
    if (gx > 0x7fffffffull) return dswx_fail(DSWX_ERR_ARG, "tile too large");
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_pairs * (size_t)n_tiles * DSWX_CROSSTAB_CELLS * sizeof(uint64_t), s));
    a.passes = passes;
    a.out_pitch = n_tiles;
    const int64_t max_y = 65535;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += max_y) {
        const int64_t nt = n_tiles - t0 < max_y ? n_tiles - t0 : max_y;
        CrossArgs b = a;
        for (int k = 0; k < n_pairs; ++k) {
            b.pair[k].a += (unsigned long long)t0 * b.pair[k].a_stride_bytes;
            b.pair[k].b += (unsigned long long)t0 * b.pair[k].b_stride_bytes;
        }
        b.out = reinterpret_cast<unsigned long long*>(out) + t0 * DSWX_CROSSTAB_CELLS;
        hipLaunchKernelGGL(dswx_crosstab_k, dim3((unsigned)gx, (unsigned)nt, (unsigned)n_pairs), dim3(CROSS_BLOCK), 0, s, b);
        HIP_TRY(hipGetLastError());
    }
    char info[256];
    snprintf(info, sizeof info, "dswx_crosstab_k grid=(%llu,%lld,%d) block=%d passes=%d replicas=%d", gx,
             (long long)(n_tiles < max_y ? n_tiles : max_y), n_pairs, CROSS_BLOCK, passes, CROSS_REPLICAS);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_crosstab_host(const void* a, const uint8_t* b, const dswx_crosstab_spec_t* spec, int64_t n_elems, uint64_t* out) {
    if (int rc = dswx_crosstab_check_spec(spec)) return rc;
    if (n_elems < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (!out || ((!a || !b) && n_elems)) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    if (!aligned_to(out, 8)) return dswx_fail(DSWX_ERR_ALIGN, "out not 8-byte aligned");
    std::memset(out, 0, DSWX_CROSSTAB_CELLS * sizeof(uint64_t));
    switch (spec->a_kind) {
        case DSWX_HIST_U8: cross_host<DSWX_HIST_U8>(a, b, *spec, n_elems, out); break;
        case DSWX_HIST_U16: cross_host<DSWX_HIST_U16>(a, b, *spec, n_elems, out); break;
        case DSWX_HIST_I16: cross_host<DSWX_HIST_I16>(a, b, *spec, n_elems, out); break;
        default: cross_host<DSWX_HIST_DIAG>(a, b, *spec, n_elems, out); break;
    }
    return DSWX_OK;
}

int dswx_crosstab_device(dswx_ctx_t* ctx, const void* a, const uint8_t* b, const dswx_crosstab_spec_t* spec, int64_t n_tiles,
                         int64_t n_elems, int64_t a_stride_elems, int64_t b_stride_elems, uint64_t* out, void* stream) {
    if (int rc = dswx_crosstab_check_spec(spec)) return rc;
    if (n_tiles < 0 || n_elems < 0 || a_stride_elems < 0 || b_stride_elems < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (a_stride_elems == 0) a_stride_elems = n_elems;
    if (b_stride_elems == 0) b_stride_elems = n_elems;
    if (a_stride_elems < n_elems || b_stride_elems < n_elems) return dswx_fail(DSWX_ERR_ARG, "tile_stride smaller than the tile");
    const int64_t st = a_stride_elems > b_stride_elems ? a_stride_elems : b_stride_elems;
    if (n_tiles > (1LL << 32) || st > (1LL << 46) || (n_tiles && (uint64_t)st > (1ull << 46) / (uint64_t)n_tiles))
        return dswx_fail(DSWX_ERR_ARG, "plane too large");
    if (n_tiles > 0 && (!a || !b || !out)) return dswx_fail(DSWX_ERR_ARG, "NULL pointer");
    const size_t eb = (size_t)dswx_histogram_elem_bytes(spec->a_kind);
    if (!aligned_to(a, eb)) return dswx_fail(DSWX_ERR_ALIGN, "plane a not aligned to its %d-byte elements", (int)eb);
    if (!aligned_to(out, 8)) return dswx_fail(DSWX_ERR_ALIGN, "out not 8-byte aligned");
    const dswx_crosstab_item it = {a, b, spec, (uint64_t)n_elems, (uint64_t)a_stride_elems, (uint64_t)b_stride_elems};
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) { return dswx_crosstab_launch(ctx, &it, 1, n_tiles, out, s); });
}

}  // extern "C"
