// dswx_stack.hip -- the tiles of a plane composited per pixel (DSWX_HAS_STACK, additive to ABI v7): per-category counts, the
// latest observation and its tile index, and the share of category 0, without the plane crossing PCIe.  include/dswx_hip.h
// "stack" states the definition; proteus_amd/stack.py is its numpy statement and dswx_stack_host below the scalar one --
// dswx_stack_rule.h is compiled for both sides, so the host entry and the kernel cannot differ.
//
// The kernel is a different shape from the other analytic kernels: it reduces ACROSS tiles, so it has no atomics and no
// records, and one output element per pixel.  grid.x covers the pixels only.  A thread owns STACK_PPT = 16 consecutive
// pixels and walks the tiles: every tile costs it one 16-byte load through the under-aligned vector type (gfx950 performs
// unaligned 16-byte global accesses in hardware, so a stack at any address and any stride takes the same kernel).  The loads
// of a thread go to different tiles and do not depend on each other: STACK_U = 8 are issued before the first is used, 128
// bytes in flight per thread.  The state of a pixel stays in registers for the whole walk: 3 dwords (below), 48 for the 16
// pixels, beside the 32 of the loads.  The elements behind the last whole 16-byte unit of a tile (fewer than 16) belong to
// ONE thread, the one after the last unit, which walks them element by element with the same rule.  No scratch of the
// context, nothing zeroed in front: every wanted output element is written exactly once, by the thread that owns it.
//
// COUNTING WITHOUT A BRANCH PER CATEGORY.  The four counts of a pixel are four uint16 fields of ONE uint64 accumulator, and
// a block widens cat_of_byte once into a table of 256 uint64 INCREMENTS in LDS: 1 << (16 * category), or 0 for a byte that
// is not an observation (stack_increment).  One 64-bit add per byte advances whichever field it is; the fields cannot carry
// into each other because a field grows by at most 1 per tile and n_tiles <= 65535.  A non-zero increment also MEANS
// "observed", which is all that `last` and `last_index` need: they live together in one dword, tile << 8 | byte, replaced
// when the increment is not zero (a select, not a branch).  Per input byte that is one ds_read_b64 and, from the ISA
// (tools/isa_stats.py; DESIGN.md section 5 has the count and the budget against HBM): extract the byte, form the LDS
// address, one v_lshl_add_u64 for the 64-bit sum, and for the latest observation a compare, an or and a select -- 6.07 VALU
// instructions per byte.  A launch that wants neither `last` nor `last_index` runs the instantiation without those three,
// 3.07 per byte: that one is bound by HBM, the full one by VALU issue (measured: DESIGN.md section 5).
//
// THE TABLE: EIGHT LANE-INDEXED REPLICAS.  ds_read_b64 looks for conflicts among the 32 lanes of a half-wave, and the bank
// of a byte address a is (a / 4) mod 64.  With ONE 2-KiB table the entries e and e + 32 share their two banks.  Class planes
// do not notice: lanes that read the same entry are served by one broadcast, and the handful of byte values of a WTR-family
// plane (0 .. 4, 252 .. 255) are all different modulo 32 -- a constant plane and a plane of class noise alike cost the 2 LDS
// cycles of a conflict-free instruction.  A plane whose bytes are spread over all 256 values does: 32 lanes into 32 bank
// pairs is 3 to 4 addresses on the busiest pair, 7 LDS cycles per 64 bytes instead of 2, which is about what a CU's share
// of HBM delivers in the same time -- the kernel would tip from HBM-bound to LDS-bound on exactly the content nobody tests
// by eye.  So the table is laid out tab[byte][replica] with STACK_REPLICAS = 8 and lane l reads replica l & 7: the bank pair
// is then 8 (byte mod 4) + (l & 7), only the 4 lanes of a half-wave with equal l & 7 can meet at all, and they conflict only
// where their bytes differ and agree modulo 4 -- at most 4 addresses on a pair, 1.6 on average on uniform noise: 3 to 4 LDS
// cycles per 64 bytes, half of what HBM allows.  The replica index rides in the address add that the lookup needs anyway, so
// it costs no instruction; the price is 16 KiB of LDS per block (ten blocks per CU by LDS, fewer by registers) and 8
// ds_write_b64 per thread at the start, against at least n_tiles x 16 lookups.  The histogram's full answer, 32 replicas, is
// conflict-free by construction but 64 KiB for 8-byte entries -- two blocks per CU -- and buys 1 to 2 cycles that are
// already in the shadow of HBM.  The other kernels' all-equal-unit shortcut (one lookup for 16 equal bytes) is NOT taken:
// the accumulators are per pixel, so 16 equal bytes still are 16 adds, and with broadcast reads a constant unit costs the
// LDS nothing to begin with.  Constant planes and noise therefore run the same instructions; the rate does not depend on
// the content beyond the conflicts counted above.
//
// WHAT THE CODE DOES NOT SAY.  A block touches n_tiles pages, one per tile, a tile stride (13 MB at 3660 x 3660) apart.
// Whether address translation limits the rate at 256 tiles was a question for a measurement (tools/stack_rate.py): it does
// not -- the share-alone launch over 256 tiles reads faster than the histogram kernel reads the same bytes tile after tile
// (DESIGN.md section 5).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#include "dswx_host.h"
#include "dswx_stack_rule.h"

namespace {

typedef u32x4 __attribute__((aligned(1))) u32x4_b;      // 16 bytes anywhere

constexpr int STACK_BLOCK = 256;                         // threads: one table entry each at the start
constexpr int STACK_PPT = 16;                            // pixels per thread = bytes per load
constexpr int STACK_U = 8;                               // loads (tiles) in flight per thread
constexpr int STACK_REPLICAS = 8;                        // of the increment table: lane l reads replica l & 7
static_assert(STACK_BLOCK == 256, "the table has one entry per thread of a block");
static_assert(DSWX_STACK_MAX_CATS * 16 == 64 && DSWX_STACK_MAX_TILES < (1 << 16), "four uint16 fields that cannot carry");

struct StackArgs {
    const unsigned char* stack;
    unsigned long long n_elems;                          // pixels of a tile
    unsigned long long stride;                           // bytes between tiles
    int n_tiles, n_cats, fill;
    unsigned short* count[DSWX_STACK_MAX_CATS];
    unsigned char* last;
    unsigned short* last_index;
    unsigned char* share;
    unsigned char cat_of_byte[256];
};
static_assert(sizeof(StackArgs) <= 4096, "kernel arguments");

// one 16-byte unit of tile t into the 16 pixels of a thread (`mine` = tab + (lane & 7); the entry of byte b is mine[b * 8])
// (the callers pass t through readfirstlane: an opaque scalar, so that tile << 8 | byte is one v_or with an SGPR)
template <bool LATEST>
__device__ __forceinline__ void stack_unit(const u32x4& v, uint32_t t, const uint64_t* mine, uint64_t (&acc)[STACK_PPT],
                                           uint32_t (&latest)[STACK_PPT]) {
    // the 16 lookups first, then the 16 updates: the LDS reads of a unit are in flight together
    uint64_t inc[STACK_PPT];
#pragma unroll
    for (int i = 0; i < STACK_PPT; ++i) inc[i] = mine[((v[i / 4] >> (8 * (i % 4))) & 0xffu) * STACK_REPLICAS];
#pragma unroll
    for (int i = 0; i < STACK_PPT; ++i) {
        if (LATEST) stack_step(acc[i], latest[i], inc[i], t, (v[i / 4] >> (8 * (i % 4))) & 0xffu);
        else acc[i] += inc[i];
    }
}

// 16 values of 16 bits / of 8 bits to 16 consecutive elements at any element-aligned address
template <typename F> __device__ __forceinline__ void store16_u16(unsigned short* dst, F value) {
    u32x4 lo, hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lo[j] = value(2 * j) | (value(2 * j + 1) << 16);
        hi[j] = value(8 + 2 * j) | (value(8 + 2 * j + 1) << 16);
    }
    stg_u<u32x4_u, u32x4, false>(dst, lo);
    stg_u<u32x4_u, u32x4, false>(dst + 8, hi);
}
template <typename F> __device__ __forceinline__ void store16_u8(unsigned char* dst, F value) {
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = value(4 * j) | (value(4 * j + 1) << 8) | (value(4 * j + 2) << 16) | (value(4 * j + 3) << 24);
    stg_u<u32x4_b, u32x4, false>(dst, w);
}

template <bool LATEST>
__global__ __launch_bounds__(STACK_BLOCK) void dswx_stack_k(const StackArgs a) {
    __shared__ __attribute__((aligned(16))) uint64_t tab[256 * STACK_REPLICAS];
    {
        const uint64_t inc = stack_increment(a.cat_of_byte, a.n_cats, threadIdx.x);
#pragma unroll
        for (int r = 0; r < STACK_REPLICAS; ++r) tab[threadIdx.x * STACK_REPLICAS + r] = inc;
    }
    __syncthreads();
    const uint64_t* const mine = tab + (threadIdx.x & (STACK_REPLICAS - 1));
    const unsigned long long units = a.n_elems >> 4;
    const unsigned long long u = (unsigned long long)blockIdx.x * STACK_BLOCK + threadIdx.x;
    const uint32_t none = stack_latest_none(a.fill);
    if (u < units) {
        uint64_t acc[STACK_PPT];
        uint32_t latest[STACK_PPT];
#pragma unroll
        for (int i = 0; i < STACK_PPT; ++i) {
            acc[i] = 0;
            latest[i] = none;
        }
        const unsigned char* p = a.stack + u * STACK_PPT;            // this thread's unit of tile t
        int t = 0;
        for (; t + STACK_U <= a.n_tiles; t += STACK_U) {             // whole rounds: the loads first, then the counting
            u32x4 v[STACK_U];
#pragma unroll
            for (int j = 0; j < STACK_U; ++j) v[j] = ldg_u<u32x4_b, u32x4, true>(p + (unsigned long long)j * a.stride);
#pragma unroll
            for (int j = 0; j < STACK_U; ++j) stack_unit<LATEST>(v[j], (uint32_t)__builtin_amdgcn_readfirstlane(t + j), mine, acc, latest);
            p += (unsigned long long)STACK_U * a.stride;
        }
        if (t < a.n_tiles) {                                         // the last round, short (uniform over the grid)
            u32x4 v[STACK_U];
#pragma unroll
            for (int j = 0; j < STACK_U; ++j) {
                v[j] = u32x4{0u, 0u, 0u, 0u};
                if (t + j < a.n_tiles) v[j] = ldg_u<u32x4_b, u32x4, true>(p + (unsigned long long)j * a.stride);
            }
#pragma unroll
            for (int j = 0; j < STACK_U; ++j)
                if (t + j < a.n_tiles) stack_unit<LATEST>(v[j], (uint32_t)__builtin_amdgcn_readfirstlane(t + j), mine, acc, latest);
        }
        const unsigned long long e = u * STACK_PPT;
#pragma unroll
        for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k)
            if (a.count[k]) store16_u16(a.count[k] + e, [&](int i) { return stack_count(acc[i], k); });
        if (LATEST && a.last) store16_u8(a.last + e, [&](int i) { return stack_last(latest[i]); });
        if (LATEST && a.last_index) store16_u16(a.last_index + e, [&](int i) { return stack_last_index(latest[i]); });
        if (a.share) store16_u8(a.share + e, [&](int i) { return stack_share(acc[i]); });
    } else if (u == units) {
        // the elements behind the last whole unit: fewer than 16, one at a time, the same rule
        for (unsigned long long e = units * STACK_PPT; e < a.n_elems; ++e) {
            uint64_t acc = 0;
            uint32_t latest = none;
            const unsigned char* p = a.stack + e;
            for (int t = 0; t < a.n_tiles; ++t, p += a.stride) {
                const unsigned byte = *p;
                stack_step(acc, latest, mine[byte * STACK_REPLICAS], (uint32_t)t, byte);
            }
            for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k)
                if (a.count[k]) a.count[k][e] = (unsigned short)stack_count(acc, k);
            if (a.last) a.last[e] = (unsigned char)stack_last(latest);
            if (a.last_index) a.last_index[e] = (unsigned short)stack_last_index(latest);
            if (a.share) a.share[e] = (unsigned char)stack_share(acc);
        }
    }
}

// unaligned host stores (a host buffer may sit at any address)
inline void put_u16(uint16_t* base, int64_t i, unsigned v) {
    const uint16_t h = (uint16_t)v;
    std::memcpy(reinterpret_cast<unsigned char*>(base) + (size_t)i * 2, &h, 2);
}

}  // namespace

// The checks that the device and the host entry share, in the house order: the arguments before any context, nothing
// written by a refused call.  `align` = the uint16 outputs must be 2-byte aligned (the device entry).
int dswx_stack_check(const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems, int64_t* stride,
                     const dswx_stack_out_t* out, bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (spec->n_cats < 1 || spec->n_cats > DSWX_STACK_MAX_CATS)
        return dswx_fail(DSWX_ERR_ARG, "n_cats %d outside 1 .. %d", spec->n_cats, DSWX_STACK_MAX_CATS);
    if (spec->fill < 0 || spec->fill > 255) return dswx_fail(DSWX_ERR_ARG, "fill %d outside 0 .. 255", spec->fill);
    if (n_tiles < 0 || n_elems < 0 || *stride < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (*stride == 0) *stride = n_elems;
    if (*stride < n_elems) return dswx_fail(DSWX_ERR_ARG, "tile_stride smaller than the tile");
    if (n_tiles > DSWX_STACK_MAX_TILES)
        return dswx_fail(DSWX_ERR_ARG, "n_tiles %lld above DSWX_STACK_MAX_TILES (%d): a count would not fit its uint16",
                         (long long)n_tiles, DSWX_STACK_MAX_TILES);
    if (*stride > (1LL << 46) || (n_tiles && (uint64_t)*stride > (1ull << 46) / (uint64_t)n_tiles))
        return dswx_fail(DSWX_ERR_ARG, "plane too large");
    if (!stack && n_tiles > 0 && n_elems > 0) return dswx_fail(DSWX_ERR_ARG, "stack is NULL");
    bool any = out->last || out->last_index || out->share;
    for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k) {
        if (out->count[k] && k >= spec->n_cats)
            return dswx_fail(DSWX_ERR_ARG, "count[%d] is not NULL but n_cats is %d", k, spec->n_cats);
        any = any || out->count[k];
    }
    if (!any) return dswx_fail(DSWX_ERR_ARG, "every output is NULL");
    if (align) {
        for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k)
            if (!aligned_to(out->count[k], 2)) return dswx_fail(DSWX_ERR_ALIGN, "count[%d] not 2-byte aligned", k);
        if (!aligned_to(out->last_index, 2)) return dswx_fail(DSWX_ERR_ALIGN, "last_index not 2-byte aligned");
    }
    return DSWX_OK;
}

// One launch; the arguments have passed dswx_stack_check (stride resolved).
int dswx_stack_launch(dswx_ctx* ctx, const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems,
                      int64_t stride, const dswx_stack_out_t* out, hipStream_t s) {
    if (n_elems == 0) {
        ctx->last_kernel = "none (empty input)";
        return DSWX_OK;
    }
    const unsigned long long threads = ((unsigned long long)n_elems >> 4) + ((n_elems & 15) ? 1 : 0);
    const unsigned long long gx = (threads + STACK_BLOCK - 1) / STACK_BLOCK;
    if (gx > 0x7fffffffull) return dswx_fail(DSWX_ERR_ARG, "tile too large");
    StackArgs a = {};
    a.stack = stack;
    a.n_elems = (unsigned long long)n_elems;
    a.stride = (unsigned long long)stride;
    a.n_tiles = (int)n_tiles;
    a.n_cats = spec->n_cats;
    a.fill = spec->fill;
    for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k) a.count[k] = out->count[k];
    a.last = out->last;
    a.last_index = out->last_index;
    a.share = out->share;
    std::memcpy(a.cat_of_byte, spec->cat_of_byte, 256);
    const bool latest = out->last || out->last_index;
    if (latest) hipLaunchKernelGGL(dswx_stack_k<true>, dim3((unsigned)gx), dim3(STACK_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(dswx_stack_k<false>, dim3((unsigned)gx), dim3(STACK_BLOCK), 0, s, a);
    HIP_TRY(hipGetLastError());
    char info[256];
    snprintf(info, sizeof info, "dswx_stack_k grid=(%llu,1,1) block=%d pixels_per_thread=%d tiles_in_flight=%d replicas=%d latest=%d",
             gx, STACK_BLOCK, STACK_PPT, STACK_U, STACK_REPLICAS, latest ? 1 : 0);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_stack_host(const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems, int64_t stride,
                    const dswx_stack_out_t* out) {
    if (int rc = dswx_stack_check(stack, spec, n_tiles, n_elems, &stride, out, false)) return rc;
    uint64_t inc_of[256];
    for (int b = 0; b < 256; ++b) inc_of[b] = stack_increment(spec->cat_of_byte, spec->n_cats, (unsigned)b);
    constexpr int64_t CHUNK = 4096;                      // pixels whose state is walked through the tiles together
    uint64_t acc[CHUNK];
    uint32_t latest[CHUNK];
    for (int64_t e0 = 0; e0 < n_elems; e0 += CHUNK) {
        const int64_t n = n_elems - e0 < CHUNK ? n_elems - e0 : CHUNK;
        for (int64_t i = 0; i < n; ++i) {
            acc[i] = 0;
            latest[i] = stack_latest_none(spec->fill);
        }
        for (int64_t t = 0; t < n_tiles; ++t) {
            const uint8_t* p = stack + (size_t)t * (size_t)stride + e0;
            for (int64_t i = 0; i < n; ++i) stack_step(acc[i], latest[i], inc_of[p[i]], (uint32_t)t, p[i]);
        }
        for (int64_t i = 0; i < n; ++i) {
            for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k)
                if (out->count[k]) put_u16(out->count[k], e0 + i, stack_count(acc[i], k));
            if (out->last) out->last[e0 + i] = (uint8_t)stack_last(latest[i]);
            if (out->last_index) put_u16(out->last_index, e0 + i, stack_last_index(latest[i]));
            if (out->share) out->share[e0 + i] = (uint8_t)stack_share(acc[i]);
        }
    }
    return DSWX_OK;
}

int dswx_stack_device(dswx_ctx_t* ctx, const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems,
                      int64_t stride, const dswx_stack_out_t* out, void* stream) {
    if (int rc = dswx_stack_check(stack, spec, n_tiles, n_elems, &stride, out, true)) return rc;
    if (!ctx) return dswx_fail(DSWX_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return dswx_stack_launch(ctx, stack, spec, n_tiles, n_elems, stride, out, dswx_stream_of(ctx, stream));
}

}  // extern "C"
