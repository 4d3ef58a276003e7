// dswx_stack_core.h -- what the stack and the mosaic entries (dswx_stack.hip, dswx_mosaic.hip) share around the per-byte rule
// of dswx_stack_rule.h: on the device the table of increments, the unit of 16 pixels and their stores; on the host the checks
// of the spec and the outputs and the write-out of a pixel.  Header-only: each of the two files, alone, is a whole program
// for tests/native/stack_host_san.cpp.
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
#pragma once

#include <hip/hip_runtime.h>
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

// The outputs and the spec of a launch, inside the kernel arguments of either entry
struct StackCoreArgs {
    int n_cats, fill;
    unsigned short* count[DSWX_STACK_MAX_CATS];
    unsigned char* last;
    unsigned short* last_index;
    unsigned char* share;
    unsigned char cat_of_byte[256];
};

// The table of a block, tab[256 * STACK_REPLICAS] in LDS, filled and ready behind a barrier; returns the replica of this lane
// (the entry of byte b is mine[b * STACK_REPLICAS])
__device__ __forceinline__ const uint64_t* stack_fill_table(uint64_t* tab, const StackCoreArgs& c) {
    const uint64_t inc = stack_increment(c.cat_of_byte, c.n_cats, threadIdx.x);
#pragma unroll
    for (int r = 0; r < STACK_REPLICAS; ++r) tab[threadIdx.x * STACK_REPLICAS + r] = inc;
    __syncthreads();
    return tab + (threadIdx.x & (STACK_REPLICAS - 1));
}

// one 16-byte unit of tile t into the 16 pixels of a thread; MASKED: only the pixels whose bit of `m` is set are covered, the
// increment of the others is made zero -- which by the rule is "not an observation"
// (the callers pass t through readfirstlane: an opaque scalar, so that tile << 8 | byte is one v_or with an SGPR)
template <bool LATEST, bool MASKED>
__device__ __forceinline__ void stack_unit(const u32x4& v, unsigned m, uint32_t t, const uint64_t* mine, uint64_t (&acc)[STACK_PPT],
                                           uint32_t (&latest)[STACK_PPT]) {
    // the 16 lookups first, then the 16 updates: the LDS reads of a unit are in flight together
    uint64_t inc[STACK_PPT];
#pragma unroll
    for (int i = 0; i < STACK_PPT; ++i) inc[i] = mine[((v[i / 4] >> (8 * (i % 4))) & 0xffu) * STACK_REPLICAS];
#pragma unroll
    for (int i = 0; i < STACK_PPT; ++i) {
        if (MASKED) inc[i] = ((m >> i) & 1u) ? inc[i] : 0ull;
        if (LATEST) stack_step(acc[i], latest[i], inc[i], t, (v[i / 4] >> (8 * (i % 4))) & 0xffu);
        else acc[i] += inc[i];
    }
}

// 16 values of 16 bits / of 8 bits, or the first n of them, to consecutive elements at any element-aligned address
template <typename F> __device__ __forceinline__ void store_u16(unsigned short* dst, int n, F value) {
    if (n == STACK_PPT) {
        u32x4 lo, hi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo[j] = value(2 * j) | (value(2 * j + 1) << 16);
            hi[j] = value(8 + 2 * j) | (value(8 + 2 * j + 1) << 16);
        }
        stg_u<u32x4_u, u32x4, false>(dst, lo);
        stg_u<u32x4_u, u32x4, false>(dst + 8, hi);
    } else {
#pragma unroll
        for (int i = 0; i < STACK_PPT; ++i)
            if (i < n) dst[i] = (unsigned short)value(i);
    }
}
template <typename F> __device__ __forceinline__ void store_u8(unsigned char* dst, int n, F value) {
    if (n == STACK_PPT) {
        u32x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = value(4 * j) | (value(4 * j + 1) << 8) | (value(4 * j + 2) << 16) | (value(4 * j + 3) << 24);
        stg_u<u32x4_b, u32x4, false>(dst, w);
    } else {
#pragma unroll
        for (int i = 0; i < STACK_PPT; ++i)
            if (i < n) dst[i] = (unsigned char)value(i);
    }
}

// ---- host side.  The refusals below keep the order of the entries' checks: the spec fields, (sizes), the tiles, (plane), the
// outputs.
inline int stack_spec_check(int n_cats, int fill) {
    if (n_cats < 1 || n_cats > DSWX_STACK_MAX_CATS) return dswx_fail(DSWX_ERR_ARG, "n_cats %d outside 1 .. %d", n_cats, DSWX_STACK_MAX_CATS);
    if (fill < 0 || fill > 255) return dswx_fail(DSWX_ERR_ARG, "fill %d outside 0 .. 255", fill);
    return DSWX_OK;
}
inline int stack_tiles_check(int64_t n_tiles) {
    if (n_tiles > DSWX_STACK_MAX_TILES)
        return dswx_fail(DSWX_ERR_ARG, "n_tiles %lld above DSWX_STACK_MAX_TILES (%d): a count would not fit its uint16",
                         (long long)n_tiles, DSWX_STACK_MAX_TILES);
    return DSWX_OK;
}
// `align` = the uint16 outputs must be 2-byte aligned (the device entries)
inline int stack_out_check(const dswx_stack_out_t* out, int n_cats, bool align) {
    if (int rc = dswx_outputs_check(out->count, DSWX_STACK_MAX_CATS, n_cats, out->last || out->last_index || out->share)) return rc;
    if (align) {
        for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k)
            if (!aligned_to(out->count[k], 2)) return dswx_fail(DSWX_ERR_ALIGN, "count[%d] not 2-byte aligned", k);
        if (!aligned_to(out->last_index, 2)) return dswx_fail(DSWX_ERR_ALIGN, "last_index not 2-byte aligned");
    }
    return DSWX_OK;
}

// does a launch need the instantiation that keeps the latest observation
inline bool stack_wants_latest(const dswx_stack_out_t* out) { return out->last || out->last_index; }

inline void stack_core_args(StackCoreArgs& c, const dswx_stack_out_t* out, int n_cats, int fill, const uint8_t* cat_of_byte) {
    c.n_cats = n_cats;
    c.fill = fill;
    for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k) c.count[k] = out->count[k];
    c.last = out->last;
    c.last_index = out->last_index;
    c.share = out->share;
    std::memcpy(c.cat_of_byte, cat_of_byte, 256);
}

// the wanted outputs of pixel e of a host entry; `last` is the caller's: stack_last(latest), or the mosaic's `outside`
inline void stack_put_pixel(const dswx_stack_out_t* out, int64_t e, uint64_t acc, uint32_t latest, unsigned last) {
    for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k)
        if (out->count[k]) dswx_store<uint16_t>(out->count[k], (size_t)e, (uint16_t)stack_count(acc, k));
    if (out->last) out->last[e] = (uint8_t)last;
    if (out->last_index) dswx_store<uint16_t>(out->last_index, (size_t)e, (uint16_t)stack_last_index(latest));
    if (out->share) out->share[e] = (uint8_t)stack_share(acc);
}

}  // namespace
