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
// COUNTING WITHOUT A BRANCH PER CATEGORY, and THE TABLE of eight lane-indexed replicas that it reads: dswx_stack_core.h, which
// the mosaic kernel shares, has both and the bank arithmetic.
//
// WHAT THE CODE DOES NOT SAY.  A block touches n_tiles pages, one per tile, a tile stride (13 MB at 3660 x 3660) apart.
// Whether address translation limits the rate at 256 tiles was a question for a measurement (tools/stack_rate.py): it does
// not -- the share-alone launch over 256 tiles reads faster than the histogram kernel reads the same bytes tile after tile
// (DESIGN.md section 5).
#include <hip/hip_runtime.h>
#include <cstdio>

#include "dswx_stack_core.h"

namespace {

struct StackArgs {
    const unsigned char* stack;
    unsigned long long n_elems;                          // pixels of a tile
    unsigned long long stride;                           // bytes between tiles
    int n_tiles;
    StackCoreArgs c;                                     // outputs and spec
};
static_assert(sizeof(StackArgs) <= 4096, "kernel arguments");

template <bool LATEST>
__global__ __launch_bounds__(STACK_BLOCK) void dswx_stack_k(const StackArgs a) {
    __shared__ __attribute__((aligned(16))) uint64_t tab[256 * STACK_REPLICAS];
    const uint64_t* const mine = stack_fill_table(tab, a.c);
    const unsigned long long units = a.n_elems >> 4;
    const unsigned long long u = (unsigned long long)blockIdx.x * STACK_BLOCK + threadIdx.x;
    const uint32_t none = stack_latest_none(a.c.fill);
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
            for (int j = 0; j < STACK_U; ++j) stack_unit<LATEST, false>(v[j], 0u, (uint32_t)__builtin_amdgcn_readfirstlane(t + j), mine, acc, latest);
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
                if (t + j < a.n_tiles) stack_unit<LATEST, false>(v[j], 0u, (uint32_t)__builtin_amdgcn_readfirstlane(t + j), mine, acc, latest);
        }
        const unsigned long long e = u * STACK_PPT;
#pragma unroll
        for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k)
            if (a.c.count[k]) store_u16(a.c.count[k] + e, STACK_PPT, [&](int i) { return stack_count(acc[i], k); });
        if (LATEST && a.c.last) store_u8(a.c.last + e, STACK_PPT, [&](int i) { return stack_last(latest[i]); });
        if (LATEST && a.c.last_index) store_u16(a.c.last_index + e, STACK_PPT, [&](int i) { return stack_last_index(latest[i]); });
        if (a.c.share) store_u8(a.c.share + e, STACK_PPT, [&](int i) { return stack_share(acc[i]); });
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
                if (a.c.count[k]) a.c.count[k][e] = (unsigned short)stack_count(acc, k);
            if (a.c.last) a.c.last[e] = (unsigned char)stack_last(latest);
            if (a.c.last_index) a.c.last_index[e] = (unsigned short)stack_last_index(latest);
            if (a.c.share) a.c.share[e] = (unsigned char)stack_share(acc);
        }
    }
}

}  // namespace

// The checks that the device and the host entry share, in the house order: the arguments before any context, nothing
// written by a refused call.  `align` = the uint16 outputs must be 2-byte aligned (the device entry).
int dswx_stack_check(const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems, int64_t* stride,
                     const dswx_stack_out_t* out, bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (int rc = stack_spec_check(spec->n_cats, spec->fill)) return rc;
    if (n_tiles < 0 || n_elems < 0 || *stride < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (int rc = dswx_tile_stride_check(stride, n_elems)) return rc;
    if (int rc = stack_tiles_check(n_tiles)) return rc;
    if (int rc = dswx_tile_extent_check(*stride, n_tiles, false)) return rc;
    if (int rc = dswx_tile_plane_check(stack, n_tiles, n_elems, "stack")) return rc;
    return stack_out_check(out, spec->n_cats, align);
}

// One launch; the arguments have passed dswx_stack_check (stride resolved).
int dswx_stack_launch(dswx_ctx* ctx, const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems,
                      int64_t stride, const dswx_stack_out_t* out, hipStream_t s) {
    if (n_elems == 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
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
    stack_core_args(a.c, out, spec->n_cats, spec->fill, spec->cat_of_byte);
    const bool latest = stack_wants_latest(out);
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
        for (int64_t i = 0; i < n; ++i) stack_put_pixel(out, e0 + i, acc[i], latest[i], stack_last(latest[i]));
    }
    return DSWX_OK;
}

int dswx_stack_device(dswx_ctx_t* ctx, const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems,
                      int64_t stride, const dswx_stack_out_t* out, void* stream) {
    if (int rc = dswx_stack_check(stack, spec, n_tiles, n_elems, &stride, out, true)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) { return dswx_stack_launch(ctx, stack, spec, n_tiles, n_elems, stride, out, s); });
}

}  // extern "C"
