// dswx_checksum.hip -- per-tile checksums of planes (ABI v7): what a plane in HBM contains, as one 64-bit word per tile,
// without the plane crossing PCIe.  include/dswx_hip.h "checksums" states the definition; proteus_amd/checksum.py is its
// numpy statement and dswx_checksum_host below the scalar one.
//
// The kernel is a streaming read-only reduction.  It knows bytes only: the host turns (element size, elements, stride)
// into byte counts, so one kernel serves every element size, and one launch covers n_planes x n_tiles through the plane
// table in its arguments (grid.z = plane, grid.y = tile, grid.x = chunks of a tile).  A thread reads 16 bytes (two
// words) per load through an under-aligned vector type -- the pattern of dswx_device.h (u32x4_u, u32x2_u): gfx950
// performs unaligned 16-byte global accesses in hardware, so a plane at an odd address takes the same kernel -- keeps
// a 64-bit partial sum, the partial sums are reduced across the wave (shuffles) and the block (LDS), and ONE 64-bit
// vector atomic add per block goes to out[plane][tile].  The sum is commutative, so the order of the blocks and of
// their atomics does not show in the result.  The < 16 bytes behind the last whole 16-byte unit of a tile (at most
// two words, the last one zero-padded) and the mix(n_bytes) term are added by thread 0 of block 0 of that tile.
// The position key (g + 1) K is carried along as a running 64-bit sum: one multiply per thread, none per word.
// No scratch of the context: the entries below own nothing, so they need no ordering against its other launches.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#include "dswx_host.h"

namespace {

constexpr unsigned long long CKS_K = DSWX_CHECKSUM_K, CKS_M1 = DSWX_CHECKSUM_M1, CKS_M2 = DSWX_CHECKSUM_M2;
static_assert((CKS_K & CKS_M1 & CKS_M2 & 1) == 1, "odd constants: the position step and both multiplies are bijective");

__host__ __device__ __forceinline__ unsigned long long cks_mix(unsigned long long x) {
    x ^= x >> 30; x *= CKS_M1;
    x ^= x >> 27; x *= CKS_M2;
    x ^= x >> 31;
    return x;
}

typedef u32x4 __attribute__((aligned(1))) u32x4_b;      // 16 bytes anywhere (u32x4_u: at any int16 boundary)

constexpr int CKS_BLOCK = 256;                           // threads; one pass of a block = 256 x 16 bytes = 4 KiB
constexpr int CKS_UNROLL = 4;                            // loads in flight per thread
constexpr int CKS_MAX_PASSES = 64;                       // per block: 256 KiB of a tile, one atomic

struct CksPlane {
    const unsigned char* base;
    unsigned long long tile_bytes;                       // n_elems * elem_bytes
    unsigned long long stride_bytes;                     // tile_stride * elem_bytes
};
struct CksArgs {
    CksPlane plane[DSWX_BATCH_MAX_PLANES];
    unsigned long long* out;                             // [n_planes][out_pitch]
    long long out_pitch;
    int passes;                                          // per block, a multiple of CKS_UNROLL
};

__device__ __forceinline__ unsigned long long cks_unit(u32x4 v, unsigned long long key) {
    const unsigned long long w0 = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
    const unsigned long long w1 = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    return cks_mix(w0 + key) + cks_mix(w1 + key + CKS_K);
}

// CKS_UNROLL units of one thread, CKS_BLOCK units apart, from unit u with key (2 u + 1) K: the loads first, then the sums
template <bool WHOLE>
__device__ __forceinline__ unsigned long long cks_round(const unsigned char* tile, unsigned long long u,
                                                        unsigned long long units, unsigned long long key) {
    u32x4 v[CKS_UNROLL];
#pragma unroll
    for (int j = 0; j < CKS_UNROLL; ++j) {
        const unsigned long long uj = u + (unsigned long long)j * CKS_BLOCK;
        v[j] = u32x4{0u, 0u, 0u, 0u};
        if (WHOLE || uj < units) v[j] = ldg_u<u32x4_b, u32x4, true>(tile + uj * 16);
    }
    unsigned long long sum = 0;
#pragma unroll
    for (int j = 0; j < CKS_UNROLL; ++j) {
        const unsigned long long uj = u + (unsigned long long)j * CKS_BLOCK;
        const unsigned long long c = cks_unit(v[j], key + (unsigned long long)j * (2 * CKS_BLOCK) * CKS_K);
        sum += (WHOLE || uj < units) ? c : 0ull;
    }
    return sum;
}

__global__ __launch_bounds__(CKS_BLOCK) void dswx_checksum_k(const CksArgs a) {
    const CksPlane pl = a.plane[blockIdx.z];
    const unsigned long long nb = pl.tile_bytes, units = nb >> 4;
    unsigned long long u = (unsigned long long)blockIdx.x * (unsigned long long)a.passes * CKS_BLOCK;
    if (u >= units && blockIdx.x != 0) return;           // (the whole block: planes of one launch differ in length)
    const unsigned char* const tile = pl.base + (unsigned long long)blockIdx.y * pl.stride_bytes;
    unsigned long long sum = 0;
    u += threadIdx.x;
    unsigned long long key = (2 * u + 1) * CKS_K;        // word g = 2 u carries (g + 1) K
    for (int p = 0; p < a.passes && u - threadIdx.x < units; p += CKS_UNROLL) {
        // (wave-uniform: every round of a block but the last of a tile is whole and runs without predicates)
        if (u - threadIdx.x + CKS_UNROLL * CKS_BLOCK <= units) sum += cks_round<true>(tile, u, units, key);
        else sum += cks_round<false>(tile, u, units, key);
        u += CKS_UNROLL * CKS_BLOCK;
        key += (unsigned long long)(2 * CKS_UNROLL * CKS_BLOCK) * CKS_K;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the bytes behind the last whole unit: words 2 units and 2 units + 1, zero-padded; and the length term
        const int r = (int)(nb & 15);
        unsigned long long w[2] = {0, 0};
        for (int i = 0; i < r; ++i) w[i >> 3] |= (unsigned long long)tile[units * 16 + i] << (8 * (i & 7));
        if (r > 0) sum += cks_mix(w[0] + (2 * units + 1) * CKS_K);
        if (r > 8) sum += cks_mix(w[1] + (2 * units + 2) * CKS_K);
        sum += cks_mix(nb);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    __shared__ unsigned long long red[CKS_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < CKS_BLOCK / 64; ++w) s += red[w];
        atomicAdd(a.out + (long long)blockIdx.z * a.out_pitch + blockIdx.y, s);
    }
}

}  // namespace

// `n_planes` planes (byte counts per tile, see CksPlane) x `n_tiles` tiles -> out[n_planes][n_tiles] (device), zeroed on
// `s` in front of the kernel.  One launch (tile counts past the 65535 of grid.y: one per 65535 tiles).
int dswx_checksum_launch(dswx_ctx* ctx, const dswx_checksum_plane* planes, int n_planes, int64_t n_tiles, uint64_t* out,
                         hipStream_t s) {
    if (n_planes <= 0 || n_tiles <= 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    CksArgs a = {};
    unsigned long long units = 0;
    for (int k = 0; k < n_planes; ++k) {
        a.plane[k].base = static_cast<const unsigned char*>(planes[k].base);
        a.plane[k].tile_bytes = planes[k].tile_bytes;
        a.plane[k].stride_bytes = planes[k].stride_bytes;
        if (planes[k].tile_bytes >> 4 > units) units = planes[k].tile_bytes >> 4;
    }
    // The result does not depend on the geometry, so the chunk of a block follows the amount of work: up to 256 KiB
    // (one atomic per 256 KiB: 105,000 for the seven layers of 256 tiles), shorter while that leaves fewer than 16 K
    // blocks for the 256 CUs.
    const unsigned long long single = (units + CKS_BLOCK - 1) / CKS_BLOCK;      // passes that cover the longest tile
    int passes = CKS_MAX_PASSES;
    while (passes > CKS_UNROLL &&
           ((single + passes - 1) / passes) * (unsigned long long)n_tiles * (unsigned long long)n_planes < 16384)
        passes /= 2;
    const unsigned long long gx = single ? (single + passes - 1) / passes : 1;
    if (gx > 0x7fffffffull) return dswx_fail(DSWX_ERR_ARG, "tile too large");
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_planes * (size_t)n_tiles * sizeof(uint64_t), s));
    a.passes = passes;
    a.out_pitch = n_tiles;
    const int64_t max_y = 65535;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += max_y) {
        const int64_t nt = n_tiles - t0 < max_y ? n_tiles - t0 : max_y;
        CksArgs b = a;
        for (int k = 0; k < n_planes; ++k) b.plane[k].base += (unsigned long long)t0 * b.plane[k].stride_bytes;
        b.out = reinterpret_cast<unsigned long long*>(out) + t0;
        hipLaunchKernelGGL(dswx_checksum_k, dim3((unsigned)gx, (unsigned)nt, (unsigned)n_planes), dim3(CKS_BLOCK), 0, s, b);
        HIP_TRY(hipGetLastError());
    }
    char info[256];
    snprintf(info, sizeof info, "dswx_checksum_k grid=(%llu,%lld,%d) block=%d passes=%d", gx,
             (long long)(n_tiles < max_y ? n_tiles : max_y), n_planes, CKS_BLOCK, passes);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_checksum_host(const void* data, size_t n_bytes, uint64_t* out) {
    if (!out || (!data && n_bytes)) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    const unsigned char* p = static_cast<const unsigned char*>(data);
    unsigned long long sum = cks_mix((unsigned long long)n_bytes), key = 0;
    size_t i = 0;
    for (; i + 8 <= n_bytes; i += 8) {
        unsigned long long w = 0;
        for (int b = 0; b < 8; ++b) w |= (unsigned long long)p[i + b] << (8 * b);      // little endian on any host
        key += CKS_K;
        sum += cks_mix(w + key);
    }
    if (i < n_bytes) {
        unsigned long long w = 0;
        for (int b = 0; i + b < n_bytes; ++b) w |= (unsigned long long)p[i + b] << (8 * b);
        sum += cks_mix(w + key + CKS_K);
    }
    *out = sum;
    return DSWX_OK;
}

int dswx_checksum_device(dswx_ctx_t* ctx, const void* plane, int32_t elem_bytes, int64_t n_tiles, int64_t n_elems,
                         int64_t tile_stride_elems, uint64_t* out, void* stream) {
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)
        return dswx_fail(DSWX_ERR_ARG, "elem_bytes %d is not 1, 2, 4 or 8", elem_bytes);
    if (n_tiles < 0 || n_elems < 0 || tile_stride_elems < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (tile_stride_elems == 0) tile_stride_elems = n_elems;
    if (tile_stride_elems < n_elems) return dswx_fail(DSWX_ERR_ARG, "tile_stride smaller than the tile");
    if (n_tiles > (1LL << 32) || tile_stride_elems > (1LL << 46) ||
        (n_tiles && (uint64_t)tile_stride_elems > (1ull << 46) / (uint64_t)n_tiles))
        return dswx_fail(DSWX_ERR_ARG, "plane too large");
    if (n_tiles > 0 && (!plane || !out)) return dswx_fail(DSWX_ERR_ARG, "NULL pointer");
    if (!aligned_to(plane, (size_t)elem_bytes)) return dswx_fail(DSWX_ERR_ALIGN, "plane not aligned to its %d-byte elements", elem_bytes);
    if (!aligned_to(out, 8)) return dswx_fail(DSWX_ERR_ALIGN, "out not 8-byte aligned");
    const dswx_checksum_plane pl = {plane, (uint64_t)n_elems * (uint64_t)elem_bytes, (uint64_t)tile_stride_elems * (uint64_t)elem_bytes};
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) { return dswx_checksum_launch(ctx, &pl, 1, n_tiles, out, s); });
}

}  // extern "C"
