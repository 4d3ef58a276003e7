// dswx_histogram.hip -- per-tile histograms of planes (DSWX_HAS_HISTOGRAM, additive to ABI v7): how many elements of every
// tile fall into each of 256 bins, without the plane crossing PCIe.  include/dswx_hip.h "histogram" states the definition;
// proteus_amd/histogram.py is its numpy statement and dswx_histogram_host below the scalar one -- hist_bin is compiled for
// both sides, so the host entry and the kernel cannot differ.
//
// The kernel is dswx_checksum_k's shape: one launch covers n_planes x n_tiles through the plane table in its arguments
// (grid.z = plane, grid.y = tile, grid.x = chunks of a tile); kind, lo and shift sit in the table entry and are uniform per
// block, so one launch mixes kinds.  A thread reads 16 bytes per load through the under-aligned vector type (gfx950 performs
// unaligned 16-byte global accesses in hardware, so a plane at any address takes the same kernel) with HIST_UNROLL loads in
// flight before the first use; the elements behind the last whole 16-byte unit of a tile are counted by thread 0 of block 0
// of that tile.  The records are zeroed on the stream in front of the kernel.  No scratch of the context: the entries own
// nothing, so they need no ordering against its other launches.
//
// THE ACCUMULATION: LANE-INDEXED REPLICAS.  A block counts privately in LDS and flushes only its non-zero bins, each with
// one 64-bit atomic add to out[plane][tile][bin].  Class planes are skewed -- a few byte values cover almost every pixel,
// in long runs -- so with ONE set of 256 counters the 64 lanes of a ds_add would mostly name one address and the LDS would
// serialise them: 64 cycles for 64 elements where a conflict-free instruction takes 2 per half-wave.  Here a block keeps
// HIST_REPLICAS = 32 sets, laid out cnt[bin][replica], and lane l adds to replica l & 31.  A counter is one dword and the
// LDS has 32 dword banks for atomics as for stores, so the bank of cnt[bin][l & 31] is l & 31 WHATEVER the bin: the 32 lanes
// of a half-wave (the unit in which the LDS looks for conflicts) always name 32 different banks, and lanes l and l + 32,
// which share a counter, are served in different halves.  The add is conflict-free by construction -- for a constant
// plane, for noise, for anything in between -- so the rate does not depend on the content: that, not the best case, is
// what the design is chosen for.  The alternatives: counting runs in registers makes the constant plane cheap but leaves
// two alternating values, or a plane where one value holds 90 % of the pixels in short runs, on the serialised path; an
// aggregation of equal values across the wave (match-any by ballots) costs a ballot round per distinct value and per
// element -- more VALU work per byte on noise than the whole of this kernel.  On top of the replicas ONE shortcut: a
// 16-byte unit whose elements are all equal (four equal dwords, the first equal to itself rotated by one element) is one
// add of its element count instead of 16 (8) adds of one; it is wave-divergent only where a wave holds both sorts of unit
// and then costs what the plain path costs.
//   The price is 32 KiB of LDS per block (5 blocks = 20 waves per CU of the 160 KiB), zeroed at the start (8 16-byte
// stores per thread) and summed at the end: thread b sums cnt[b][(j + b) & 31], j = 0 .. 31 -- rotated, so that the 32
// lanes of a half-wave read 32 different banks -- and adds the sum to the record if it is not zero.  Zeroing and flush
// together are about a thousand LDS cycles against the 16 K ds_add cycles of a full chunk of bytes.
//   COUNTER WIDTH.  A counter is a uint32.  Replica r of a block is fed by the lanes r and r + 32 of its 4 waves: 8
// threads.  A thread counts at most passes <= HIST_MAX_PASSES = 64 units of at most 16 elements (+ 15 tail elements for
// thread 0 of block 0): 8 x 64 x 16 + 15 = 8207 per counter at most, and the flush sums 32 of them: 262,159 -- both far
// below 2^32.  The sum is widened to 64 bits only for the global add; the records are 64-bit, so a tile of 2^32 elements
// and more counts right (tests/test_gpu_histogram.py).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#include "dswx_host.h"
#include "dswx_hist_bin.h"

namespace {

typedef u32x4 __attribute__((aligned(1))) u32x4_b;      // 16 bytes anywhere

constexpr int HIST_BLOCK = 256;                          // threads; one pass of a block = 256 x 16 bytes = 4 KiB
constexpr int HIST_UNROLL = 4;                           // loads in flight per thread
constexpr int HIST_MAX_PASSES = 64;                      // per block: 256 KiB of a tile, at most 256 atomics
constexpr int HIST_REPLICAS = 32;                        // = the dword banks an LDS atomic sees: bank = lane & 31
static_assert(HIST_BLOCK == DSWX_HIST_BINS, "the flush gives every bin one thread");
static_assert((HIST_BLOCK / HIST_REPLICAS) * HIST_MAX_PASSES * 16ull + 15 < (1ull << 32) / HIST_REPLICAS,
              "a uint32 counter, and the sum of a bin's replicas, hold the largest chunk of a block");

struct HistPlane {
    const unsigned char* base;
    unsigned long long n_elems;                          // counted elements of every tile, from its start
    unsigned long long stride_bytes;                     // between tiles
    int kind;                                            // DSWX_HIST_*
    int lo, shift;                                       // U16 / I16
};
struct HistArgs {
    HistPlane plane[DSWX_BATCH_MAX_PLANES];
    unsigned long long* out;                             // [n_planes][out_pitch][DSWX_HIST_BINS]
    long long out_pitch;                                 // tiles
    int passes;                                          // per block, a multiple of HIST_UNROLL
};
static_assert(sizeof(HistArgs) <= 4096, "kernel arguments");

// one 16-byte unit into the thread's replica (`mine` = cnt + (lane & 31); bin b is mine[b * HIST_REPLICAS])
template <int KIND> __device__ __forceinline__ void hist_unit(const u32x4& v, unsigned* mine, int lo, int shift) {
    constexpr int EB = HistElem<KIND>::BYTES, EPU = 16 / EB, EPW = 4 / EB;
    constexpr unsigned MASK = EB == 1 ? 0xffu : 0xffffu;
    const unsigned turned = (v.x >> (8 * EB)) | (v.x << (32 - 8 * EB));
    if (v.x == v.y && v.x == v.z && v.x == v.w && v.x == turned) {      // one value: one add
        const int b = hist_bin<KIND>(v.x & MASK, lo, shift);
        if (b >= 0) atomicAdd(mine + b * HIST_REPLICAS, (unsigned)EPU);
        return;
    }
#pragma unroll
    for (int i = 0; i < EPU; ++i) {
        const int b = hist_bin<KIND>((v[i / EPW] >> (8 * EB * (i % EPW))) & MASK, lo, shift);
        if (b >= 0) atomicAdd(mine + b * HIST_REPLICAS, 1u);
    }
}

// HIST_UNROLL units of one thread, HIST_BLOCK units apart, from unit u: the loads first, then the counting
template <int KIND, bool WHOLE>
__device__ __forceinline__ void hist_round(const unsigned char* tile, unsigned long long u, unsigned long long units,
                                           unsigned* mine, int lo, int shift) {
    u32x4 v[HIST_UNROLL];
#pragma unroll
    for (int j = 0; j < HIST_UNROLL; ++j) {
        const unsigned long long uj = u + (unsigned long long)j * HIST_BLOCK;
        v[j] = u32x4{0u, 0u, 0u, 0u};
        if (WHOLE || uj < units) v[j] = ldg_u<u32x4_b, u32x4, true>(tile + uj * 16);
    }
#pragma unroll
    for (int j = 0; j < HIST_UNROLL; ++j) {
        const unsigned long long uj = u + (unsigned long long)j * HIST_BLOCK;
        if (WHOLE || uj < units) hist_unit<KIND>(v[j], mine, lo, shift);
    }
}

template <int KIND>
__device__ __forceinline__ void hist_tile(const HistArgs& a, const HistPlane& pl, const unsigned char* tile, unsigned* mine) {
    constexpr int EB = HistElem<KIND>::BYTES;
    const unsigned long long units = (pl.n_elems * EB) >> 4;
    unsigned long long u = (unsigned long long)blockIdx.x * (unsigned long long)a.passes * HIST_BLOCK + threadIdx.x;
    for (int q = 0; q < a.passes && u - threadIdx.x < units; q += HIST_UNROLL) {
        // (wave-uniform: every round of a block but the last of a tile is whole and runs without predicates)
        if (u - threadIdx.x + HIST_UNROLL * HIST_BLOCK <= units) hist_round<KIND, true>(tile, u, units, mine, pl.lo, pl.shift);
        else hist_round<KIND, false>(tile, u, units, mine, pl.lo, pl.shift);
        u += HIST_UNROLL * HIST_BLOCK;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the elements behind the last whole unit: fewer than 16 bytes, read element by element (aligned to the element)
        for (unsigned long long e = units * (16 / EB); e < pl.n_elems; ++e) {
            const unsigned raw = EB == 1 ? (unsigned)tile[e] : (unsigned)reinterpret_cast<const unsigned short*>(tile)[e];
            const int b = hist_bin<KIND>(raw, pl.lo, pl.shift);
            if (b >= 0) atomicAdd(mine + b * HIST_REPLICAS, 1u);
        }
    }
}

__global__ __launch_bounds__(HIST_BLOCK) void dswx_histogram_k(const HistArgs a) {
    const HistPlane pl = a.plane[blockIdx.z];
    const unsigned long long units = (pl.n_elems << (pl.kind == DSWX_HIST_U8 ? 0 : 1)) >> 4;
    if ((unsigned long long)blockIdx.x * (unsigned long long)a.passes * HIST_BLOCK >= units && blockIdx.x != 0)
        return;                                          // (the whole block: planes of one launch differ in length)
    __shared__ __attribute__((aligned(16))) unsigned cnt[DSWX_HIST_BINS * HIST_REPLICAS];
    {
        u32x4* z = reinterpret_cast<u32x4*>(cnt);
#pragma unroll
        for (int j = 0; j < DSWX_HIST_BINS * HIST_REPLICAS / 4 / HIST_BLOCK; ++j) z[j * HIST_BLOCK + threadIdx.x] = u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    const unsigned char* const tile = pl.base + (unsigned long long)blockIdx.y * pl.stride_bytes;
    unsigned* const mine = cnt + (threadIdx.x & (HIST_REPLICAS - 1));
    switch (pl.kind) {                                   // uniform per block
        case DSWX_HIST_U8: hist_tile<DSWX_HIST_U8>(a, pl, tile, mine); break;
        case DSWX_HIST_U16: hist_tile<DSWX_HIST_U16>(a, pl, tile, mine); break;
        case DSWX_HIST_I16: hist_tile<DSWX_HIST_I16>(a, pl, tile, mine); break;
        default: hist_tile<DSWX_HIST_DIAG>(a, pl, tile, mine); break;
    }
    __syncthreads();
    // thread b sums the replicas of bin b, each lane starting at another one: 32 banks per half-wave
    const unsigned* const row = cnt + threadIdx.x * HIST_REPLICAS;
    unsigned sum = 0;
#pragma unroll
    for (int j = 0; j < HIST_REPLICAS; ++j) sum += row[(j + threadIdx.x) & (HIST_REPLICAS - 1)];
    if (sum) atomicAdd(a.out + (((long long)blockIdx.z * a.out_pitch + blockIdx.y) * DSWX_HIST_BINS + threadIdx.x), (unsigned long long)sum);
}

template <int KIND> void hist_host(const void* data, int64_t n, int lo, int shift, uint64_t* bins) {
    constexpr int EB = HistElem<KIND>::BYTES;
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (int64_t i = 0; i < n; ++i) {
        unsigned raw;                                    // (memcpy: a host buffer may sit at any address)
        if (EB == 1) raw = p[i];
        else {
            uint16_t h;
            std::memcpy(&h, p + (size_t)i * 2, 2);
            raw = h;
        }
        const int b = hist_bin<KIND>(raw, lo, shift);
        if (b >= 0) ++bins[b];
    }
}

}  // namespace

int dswx_histogram_elem_bytes(int kind) { return kind == DSWX_HIST_U8 ? 1 : kind > 0 && kind < DSWX_HIST_KINDS ? 2 : 0; }

int dswx_histogram_check_kind(int kind, int shift) {
    if (kind < 0 || kind >= DSWX_HIST_KINDS) return dswx_fail(DSWX_ERR_ARG, "kind %d is not a DSWX_HIST_* value", kind);
    if (shift < 0 || shift > 8) return dswx_fail(DSWX_ERR_ARG, "shift %d outside 0 .. 8", shift);
    return DSWX_OK;
}

// `n_planes` planes x `n_tiles` tiles -> out[n_planes][n_tiles][256] (device), zeroed on `s` in front of the kernel.  One
// launch (tile counts past the 65535 of grid.y: one per 65535 tiles).
int dswx_histogram_launch(dswx_ctx* ctx, const dswx_histogram_plane* planes, int n_planes, int64_t n_tiles, uint64_t* out,
                          hipStream_t s) {
    if (n_planes <= 0 || n_tiles <= 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    HistArgs a = {};
    unsigned long long units = 0;
    for (int k = 0; k < n_planes; ++k) {
        HistPlane& pl = a.plane[k];
        const unsigned long long eb = (unsigned long long)dswx_histogram_elem_bytes(planes[k].kind);
        pl.base = static_cast<const unsigned char*>(planes[k].base);
        pl.n_elems = planes[k].n_elems;
        pl.stride_bytes = planes[k].stride_elems * eb;
        pl.kind = planes[k].kind;
        pl.lo = planes[k].lo;
        pl.shift = planes[k].shift;
        const unsigned long long un = (pl.n_elems * eb) >> 4;
        if (un > units) units = un;
    }
    // the chunk of a block follows the amount of work, as the checksum's: up to 256 KiB (at most 256 atomics per 256 KiB),
    // shorter while that leaves fewer than 16 K blocks for the 256 CUs (the records do not depend on the geometry)
    const unsigned long long single = (units + HIST_BLOCK - 1) / HIST_BLOCK;
    int passes = HIST_MAX_PASSES;
    while (passes > HIST_UNROLL &&
           ((single + passes - 1) / passes) * (unsigned long long)n_tiles * (unsigned long long)n_planes < 16384)
        passes /= 2;
    const unsigned long long gx = single ? (single + passes - 1) / passes : 1;
    if (gx > 0x7fffffffull) return dswx_fail(DSWX_ERR_ARG, "tile too large");
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_planes * (size_t)n_tiles * DSWX_HIST_BINS * sizeof(uint64_t), s));
    a.passes = passes;
    a.out_pitch = n_tiles;
    const int64_t max_y = 65535;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += max_y) {
        const int64_t nt = n_tiles - t0 < max_y ? n_tiles - t0 : max_y;
        HistArgs b = a;
        for (int k = 0; k < n_planes; ++k) b.plane[k].base += (unsigned long long)t0 * b.plane[k].stride_bytes;
        b.out = reinterpret_cast<unsigned long long*>(out) + t0 * DSWX_HIST_BINS;
        hipLaunchKernelGGL(dswx_histogram_k, dim3((unsigned)gx, (unsigned)nt, (unsigned)n_planes), dim3(HIST_BLOCK), 0, s, b);
        HIP_TRY(hipGetLastError());
    }
    char info[256];
    snprintf(info, sizeof info, "dswx_histogram_k grid=(%llu,%lld,%d) block=%d passes=%d replicas=%d", gx,
             (long long)(n_tiles < max_y ? n_tiles : max_y), n_planes, HIST_BLOCK, passes, HIST_REPLICAS);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_histogram_host(const void* data, int32_t kind, int32_t lo, int32_t shift, int64_t n_elems, uint64_t* out) {
    if (int rc = dswx_histogram_check_kind(kind, shift)) return rc;
    if (n_elems < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (!out || (!data && n_elems)) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    if (!aligned_to(out, 8)) return dswx_fail(DSWX_ERR_ALIGN, "out not 8-byte aligned");
    std::memset(out, 0, DSWX_HIST_BINS * sizeof(uint64_t));
    switch (kind) {
        case DSWX_HIST_U8: hist_host<DSWX_HIST_U8>(data, n_elems, lo, shift, out); break;
        case DSWX_HIST_U16: hist_host<DSWX_HIST_U16>(data, n_elems, lo, shift, out); break;
        case DSWX_HIST_I16: hist_host<DSWX_HIST_I16>(data, n_elems, lo, shift, out); break;
        default: hist_host<DSWX_HIST_DIAG>(data, n_elems, lo, shift, out); break;
    }
    return DSWX_OK;
}

int dswx_histogram_device(dswx_ctx_t* ctx, const void* plane, int32_t kind, int32_t lo, int32_t shift, int64_t n_tiles,
                          int64_t n_elems, int64_t tile_stride_elems, uint64_t* out, void* stream) {
    if (int rc = dswx_histogram_check_kind(kind, shift)) return rc;
    if (n_tiles < 0 || n_elems < 0 || tile_stride_elems < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (tile_stride_elems == 0) tile_stride_elems = n_elems;
    if (tile_stride_elems < n_elems) return dswx_fail(DSWX_ERR_ARG, "tile_stride smaller than the tile");
    if (n_tiles > (1LL << 32) || tile_stride_elems > (1LL << 46) ||
        (n_tiles && (uint64_t)tile_stride_elems > (1ull << 46) / (uint64_t)n_tiles))
        return dswx_fail(DSWX_ERR_ARG, "plane too large");
    if (n_tiles > 0 && (!plane || !out)) return dswx_fail(DSWX_ERR_ARG, "NULL pointer");
    const size_t eb = (size_t)dswx_histogram_elem_bytes(kind);
    if (!aligned_to(plane, eb)) return dswx_fail(DSWX_ERR_ALIGN, "plane not aligned to its %d-byte elements", (int)eb);
    if (!aligned_to(out, 8)) return dswx_fail(DSWX_ERR_ALIGN, "out not 8-byte aligned");
    const dswx_histogram_plane pl = {plane, kind, lo, shift, (uint64_t)n_elems, (uint64_t)tile_stride_elems};
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) { return dswx_histogram_launch(ctx, &pl, 1, n_tiles, out, s); });
}

}  // extern "C"
