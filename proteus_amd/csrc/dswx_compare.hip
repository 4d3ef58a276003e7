// dswx_compare.hip -- two planes compared on the device: per tile the number of element pairs that are not close, the first
// such index and the largest difference, without either plane crossing PCIe.  include/dswx_hip.h "compare" states the
// definition (numpy's isclose, operation by operation); proteus_amd/compare.py is its numpy statement and dswx_compare_host
// below the scalar one -- cmp_close / cmp_note are compiled for both sides, so the host entry and the kernel cannot differ.
//
// The kernel is dswx_checksum_k's shape with two read streams: one launch covers n_pairs x n_tiles through the plane table
// in its arguments (grid.z = plane pair, grid.y = tile, grid.x = chunks of a tile); the element kind sits in the table
// entry and is uniform per block, so one launch mixes kinds.  A thread reads 16 bytes of EACH plane per load through the
// under-aligned vector type -- a and b have their own address and stride, so their residues differ; gfx950 performs
// unaligned 16-byte global accesses in hardware -- with CMP_UNROLL loads of each stream in flight before the first use.  A
// unit whose 16 bytes are bit-identical is close as a whole (integers always; floats when equal_nan, where NaN / NaN is
// close and anything else bit-identical is x == y) and costs four dword compares; any other unit is tested element by
// element.  Per thread: a count, the smallest index, the largest |x - y|; reduced across the wave (shuffles) and the block
// (LDS); a block that found something ends with ONE 64-bit vector atomic add, ONE atomic min and ONE atomic max into the
// tile's record (a block that found nothing would add 0, min with "none" and max with 0: it skips them).  All three are
// order-independent -- the non-negative doubles are ordered by their bit patterns -- so the records do not depend on the
// order of the blocks.  The elements behind the last whole 16-byte unit of a tile are tested by thread 0 of block 0 of that
// tile.  The records are initialised on the stream in front of the kernel.  No scratch of the context: the entries own
// nothing, so they need no ordering against its other launches.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "dswx_host.h"

namespace {

static_assert(sizeof(dswx_compare_t) == 32, "dswx_compare_t is four 64-bit words");

struct CmpTol {
    double atol, rtol;
    float atol32, rtol32;       // the tolerances rounded to float32: what numpy uses against float32 arrays
    int equal_nan;
};

struct CmpPartial {
    unsigned long long n;       // pairs that are not close
    unsigned long long first;   // smallest such index; ~0 = none
    double mx;                  // largest |double(x) - double(y)| among them, NaN pairs aside
};

template <typename T> __host__ __device__ __forceinline__ bool cmp_is_nan(T) { return false; }
__host__ __device__ __forceinline__ bool cmp_is_nan(float v) { return v != v; }
__host__ __device__ __forceinline__ bool cmp_is_nan(double v) { return v != v; }

// integer kinds: |x - y| <= atol + rtol |y| in double (both values convert exactly)
template <typename T> __host__ __device__ __forceinline__ bool cmp_close(T x, T y, const CmpTol& t) {
    if (x == y) return true;
    const double dx = (double)x, dy = (double)y;
    return fabs(dx - dy) <= t.atol + t.rtol * fabs(dy);
}
__host__ __device__ __forceinline__ bool cmp_close(double x, double y, const CmpTol& t) {
    if (x == y) return true;                                      // equal infinities, -0 against +0
    if (x != x || y != y) return t.equal_nan && x != x && y != y;
    const double d = fabs(x - y);
    const double r = t.rtol * fabs(y);
    const double tol = t.atol + r;
    return d <= tol && fabs(y) != INFINITY;
}
// float32: one subtraction, one multiply, one add, all float32 (the library is built with -ffp-contract=off)
__host__ __device__ __forceinline__ bool cmp_close(float x, float y, const CmpTol& t) {
    if (x == y) return true;
    if (x != x || y != y) return t.equal_nan && x != x && y != y;
    const float d = fabsf(x - y);
    const float r = t.rtol32 * fabsf(y);
    const float tol = t.atol32 + r;
    return d <= tol && fabsf(y) != INFINITY;
}

template <typename T> __host__ __device__ __forceinline__ void cmp_note(T x, T y, unsigned long long index, CmpPartial& p) {
    ++p.n;
    if (index < p.first) p.first = index;
    if (!cmp_is_nan(x) && !cmp_is_nan(y)) {
        const double d = fabs((double)x - (double)y);
        if (d > p.mx) p.mx = d;
    }
}

template <typename T> __host__ __device__ __forceinline__ void cmp_pair(T x, T y, unsigned long long index, const CmpTol& t,
                                                                        CmpPartial& p) {
    if (!cmp_close(x, y, t)) cmp_note(x, y, index, p);
}

typedef u32x4 __attribute__((aligned(1))) u32x4_b;      // 16 bytes anywhere

constexpr int CMP_BLOCK = 256;                           // threads; one pass of a block = 256 x 16 bytes of each plane
constexpr int CMP_UNROLL = 4;                            // loads of EACH stream in flight per thread
constexpr int CMP_MAX_PASSES = 64;                       // per block: 256 KiB of a tile of each plane, three atomics

struct CmpPlane {
    const unsigned char* a;
    const unsigned char* b;
    unsigned long long n_elems;                          // compared elements of every tile, from its start
    unsigned long long a_stride_bytes, b_stride_bytes;   // between tiles
    int kind;                                            // DSWX_CMP_*
    int elem_log2;                                       // log2 of the element size
};
struct CmpArgs {
    CmpPlane plane[DSWX_BATCH_MAX_PLANES];
    dswx_compare_t* out;                                 // [n_pairs][out_pitch]
    long long out_pitch;
    int passes;                                          // per block, a multiple of CMP_UNROLL
    CmpTol tol;
};
static_assert(sizeof(CmpArgs) <= 4096, "kernel arguments");

// element i of a 16-byte unit held in registers (i is a constant after unrolling)
template <typename T> __device__ __forceinline__ T cmp_get(const u32x4& v, int i) {
    if constexpr (sizeof(T) == 8) {
        const unsigned long long w = (unsigned long long)v[2 * i] | ((unsigned long long)v[2 * i + 1] << 32);
        if constexpr (std::is_same<T, double>::value) return __longlong_as_double((long long)w);
        else return (T)w;
    } else if constexpr (sizeof(T) == 4) {
        if constexpr (std::is_same<T, float>::value) return __uint_as_float(v[i]);
        else return (T)v[i];
    } else {
        constexpr int per = 4 / (int)sizeof(T);
        return (T)(v[i / per] >> (8 * (int)sizeof(T) * (i % per)));
    }
}

template <typename T> __device__ __forceinline__ void cmp_unit(const u32x4& va, const u32x4& vb, unsigned long long elem0,
                                                               const CmpTol& t, CmpPartial& p) {
    constexpr bool FLT = std::is_floating_point<T>::value;
    const bool same = va.x == vb.x && va.y == vb.y && va.z == vb.z && va.w == vb.w;
    if (same && (!FLT || t.equal_nan)) return;
    constexpr int EPU = 16 / (int)sizeof(T);
    constexpr int EPW = EPU / 4 > 0 ? EPU / 4 : 1;       // elements per dword (at least the loop step)
#pragma unroll
    for (int i0 = 0; i0 < EPU; i0 += EPW) {
        if constexpr (!FLT) {
            if (va[i0 / EPW] == vb[i0 / EPW]) continue;  // an identical dword of integers holds close pairs only
        }
#pragma unroll
        for (int i = i0; i < i0 + EPW; ++i) cmp_pair(cmp_get<T>(va, i), cmp_get<T>(vb, i), elem0 + (unsigned long long)i, t, p);
    }
}

// CMP_UNROLL units of one thread, CMP_BLOCK units apart, from unit u: the loads of both streams first, then the tests
template <typename T, bool WHOLE>
__device__ __forceinline__ void cmp_round(const unsigned char* ta, const unsigned char* tb, unsigned long long u,
                                          unsigned long long units, const CmpTol& t, CmpPartial& p) {
    u32x4 va[CMP_UNROLL], vb[CMP_UNROLL];
#pragma unroll
    for (int j = 0; j < CMP_UNROLL; ++j) {
        const unsigned long long uj = u + (unsigned long long)j * CMP_BLOCK;
        va[j] = u32x4{0u, 0u, 0u, 0u};
        vb[j] = u32x4{0u, 0u, 0u, 0u};
        if (WHOLE || uj < units) {
            va[j] = ldg_u<u32x4_b, u32x4, true>(ta + uj * 16);
            vb[j] = ldg_u<u32x4_b, u32x4, true>(tb + uj * 16);
        }
    }
#pragma unroll
    for (int j = 0; j < CMP_UNROLL; ++j) {
        const unsigned long long uj = u + (unsigned long long)j * CMP_BLOCK;
        if (WHOLE || uj < units) cmp_unit<T>(va[j], vb[j], uj * (16 / sizeof(T)), t, p);
    }
}

template <typename T>
__device__ __forceinline__ void cmp_tile(const CmpArgs& a, const CmpPlane& pl, const unsigned char* ta, const unsigned char* tb,
                                         CmpPartial& p) {
    const unsigned long long units = (pl.n_elems * sizeof(T)) >> 4;
    unsigned long long u = (unsigned long long)blockIdx.x * (unsigned long long)a.passes * CMP_BLOCK + threadIdx.x;
    for (int q = 0; q < a.passes && u - threadIdx.x < units; q += CMP_UNROLL) {
        // (wave-uniform: every round of a block but the last of a tile is whole and runs without predicates)
        if (u - threadIdx.x + CMP_UNROLL * CMP_BLOCK <= units) cmp_round<T, true>(ta, tb, u, units, a.tol, p);
        else cmp_round<T, false>(ta, tb, u, units, a.tol, p);
        u += CMP_UNROLL * CMP_BLOCK;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the elements behind the last whole unit: fewer than 16 bytes of each plane, read element by element
        const T* ea = reinterpret_cast<const T*>(ta);
        const T* eb = reinterpret_cast<const T*>(tb);
        for (unsigned long long e = units * (16 / sizeof(T)); e < pl.n_elems; ++e) cmp_pair(ea[e], eb[e], e, a.tol, p);
    }
}

__global__ __launch_bounds__(CMP_BLOCK) void dswx_compare_k(const CmpArgs a) {
    const CmpPlane pl = a.plane[blockIdx.z];
    const unsigned long long units = (pl.n_elems << pl.elem_log2) >> 4;
    if ((unsigned long long)blockIdx.x * (unsigned long long)a.passes * CMP_BLOCK >= units && blockIdx.x != 0)
        return;                                          // (the whole block: planes of one launch differ in length)
    const unsigned char* const ta = pl.a + (unsigned long long)blockIdx.y * pl.a_stride_bytes;
    const unsigned char* const tb = pl.b + (unsigned long long)blockIdx.y * pl.b_stride_bytes;
    CmpPartial p = {0ull, ~0ull, 0.0};
    switch (pl.kind) {                                   // uniform per block
        case DSWX_CMP_U8: cmp_tile<uint8_t>(a, pl, ta, tb, p); break;
        case DSWX_CMP_U16: cmp_tile<uint16_t>(a, pl, ta, tb, p); break;
        case DSWX_CMP_I16: cmp_tile<int16_t>(a, pl, ta, tb, p); break;
        case DSWX_CMP_F32: cmp_tile<float>(a, pl, ta, tb, p); break;
        default: cmp_tile<double>(a, pl, ta, tb, p); break;
    }
    unsigned long long n = p.n, first = p.first, mx = (unsigned long long)__double_as_longlong(p.mx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n += __shfl_xor(n, off);
        const unsigned long long f = __shfl_xor(first, off), m = __shfl_xor(mx, off);
        first = f < first ? f : first;
        mx = m > mx ? m : mx;                            // non-negative doubles: ordered as their bit patterns
    }
    __shared__ unsigned long long red[3][CMP_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = n;
        red[1][threadIdx.x >> 6] = first;
        red[2][threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        n = 0, first = ~0ull, mx = 0;
#pragma unroll
        for (int w = 0; w < CMP_BLOCK / 64; ++w) {
            n += red[0][w];
            first = red[1][w] < first ? red[1][w] : first;
            mx = red[2][w] > mx ? red[2][w] : mx;
        }
        if (n) {
            unsigned long long* rec = reinterpret_cast<unsigned long long*>(a.out + (long long)blockIdx.z * a.out_pitch + blockIdx.y);
            atomicAdd(rec + 0, n);
            atomicMin(rec + 1, first);                   // the record starts at -1 = ~0: "none" is the largest value
            atomicMax(rec + 2, mx);
        }
    }
}

__global__ __launch_bounds__(256) void dswx_compare_init_k(dswx_compare_t* out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = dswx_compare_t{0, -1, 0.0, 0ull};
}

constexpr int CMP_ELEM_LOG2[DSWX_CMP_KINDS] = {0, 1, 1, 2, 3};

template <typename T> void cmp_host(const void* a, const void* b, int64_t n, const CmpTol& t, CmpPartial& p) {
    const unsigned char* pa = static_cast<const unsigned char*>(a);
    const unsigned char* pb = static_cast<const unsigned char*>(b);
    for (int64_t i = 0; i < n; ++i) {
        T x, y;                                          // (memcpy: a host buffer may sit at any address)
        std::memcpy(&x, pa + (size_t)i * sizeof(T), sizeof(T));
        std::memcpy(&y, pb + (size_t)i * sizeof(T), sizeof(T));
        cmp_pair(x, y, (unsigned long long)i, t, p);
    }
}

}  // namespace

int dswx_compare_elem_bytes(int kind) { return kind >= 0 && kind < DSWX_CMP_KINDS ? 1 << CMP_ELEM_LOG2[kind] : 0; }

int dswx_compare_check_tol(double atol, double rtol) {
    if (!(atol >= 0.0) || !(rtol >= 0.0) || std::isinf(atol) || std::isinf(rtol))
        return dswx_fail(DSWX_ERR_ARG, "atol and rtol must be finite and not negative (atol %g, rtol %g)", atol, rtol);
    return DSWX_OK;
}

// `n_pairs` plane pairs x `n_tiles` tiles -> out[n_pairs][n_tiles] (device), initialised on `s` in front of the kernel.  One
// launch (tile counts past the 65535 of grid.y: one per 65535 tiles).
int dswx_compare_launch(dswx_ctx* ctx, const dswx_compare_pair* pairs, int n_pairs, int64_t n_tiles, double atol, double rtol,
                        int equal_nan, dswx_compare_t* out, hipStream_t s) {
    if (n_pairs <= 0 || n_tiles <= 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    CmpArgs a = {};
    unsigned long long units = 0;
    for (int k = 0; k < n_pairs; ++k) {
        CmpPlane& pl = a.plane[k];
        pl.kind = pairs[k].kind;
        pl.elem_log2 = CMP_ELEM_LOG2[pairs[k].kind];
        pl.a = static_cast<const unsigned char*>(pairs[k].a);
        pl.b = static_cast<const unsigned char*>(pairs[k].b);
        pl.n_elems = pairs[k].n_elems;
        pl.a_stride_bytes = pairs[k].a_stride_elems << pl.elem_log2;
        pl.b_stride_bytes = pairs[k].b_stride_elems << pl.elem_log2;
        const unsigned long long un = (pl.n_elems << pl.elem_log2) >> 4;
        if (un > units) units = un;
    }
    a.tol = CmpTol{atol, rtol, (float)atol, (float)rtol, equal_nan ? 1 : 0};
    // the chunk of a block follows the amount of work, as the checksum's: up to 256 KiB of each plane, shorter while that
    // leaves fewer than 16 K blocks for the 256 CUs (the records do not depend on the geometry)
    const unsigned long long single = (units + CMP_BLOCK - 1) / CMP_BLOCK;
    int passes = CMP_MAX_PASSES;
    while (passes > CMP_UNROLL &&
           ((single + passes - 1) / passes) * (unsigned long long)n_tiles * (unsigned long long)n_pairs < 16384)
        passes /= 2;
    const unsigned long long gx = single ? (single + passes - 1) / passes : 1;
    if (gx > 0x7fffffffull) return dswx_fail(DSWX_ERR_ARG, "tile too large");
    const long long n_rec = (long long)n_pairs * (long long)n_tiles;
    hipLaunchKernelGGL(dswx_compare_init_k, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, out, n_rec);
    HIP_TRY(hipGetLastError());
    a.passes = passes;
    a.out_pitch = n_tiles;
    const int64_t max_y = 65535;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += max_y) {
        const int64_t nt = n_tiles - t0 < max_y ? n_tiles - t0 : max_y;
        CmpArgs b = a;
        for (int k = 0; k < n_pairs; ++k) {
            b.plane[k].a += (unsigned long long)t0 * b.plane[k].a_stride_bytes;
            b.plane[k].b += (unsigned long long)t0 * b.plane[k].b_stride_bytes;
        }
        b.out = out + t0;
        hipLaunchKernelGGL(dswx_compare_k, dim3((unsigned)gx, (unsigned)nt, (unsigned)n_pairs), dim3(CMP_BLOCK), 0, s, b);
        HIP_TRY(hipGetLastError());
    }
    char info[256];
    snprintf(info, sizeof info, "dswx_compare_k grid=(%llu,%lld,%d) block=%d passes=%d", gx,
             (long long)(n_tiles < max_y ? n_tiles : max_y), n_pairs, CMP_BLOCK, passes);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_compare_host(const void* a, const void* b, int32_t kind, int64_t n_elems, double atol, double rtol, int32_t equal_nan,
                      dswx_compare_t* out) {
    if (kind < 0 || kind >= DSWX_CMP_KINDS) return dswx_fail(DSWX_ERR_ARG, "kind %d is not a DSWX_CMP_* value", kind);
    if (n_elems < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (!out || ((!a || !b) && n_elems)) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    if (int rc = dswx_compare_check_tol(atol, rtol)) return rc;
    const CmpTol t = {atol, rtol, (float)atol, (float)rtol, equal_nan ? 1 : 0};
    CmpPartial p = {0ull, ~0ull, 0.0};
    switch (kind) {
        case DSWX_CMP_U8: cmp_host<uint8_t>(a, b, n_elems, t, p); break;
        case DSWX_CMP_U16: cmp_host<uint16_t>(a, b, n_elems, t, p); break;
        case DSWX_CMP_I16: cmp_host<int16_t>(a, b, n_elems, t, p); break;
        case DSWX_CMP_F32: cmp_host<float>(a, b, n_elems, t, p); break;
        default: cmp_host<double>(a, b, n_elems, t, p); break;
    }
    *out = dswx_compare_t{(int64_t)p.n, p.n ? (int64_t)p.first : -1, p.mx, 0ull};
    return DSWX_OK;
}

int dswx_compare_device(dswx_ctx_t* ctx, const void* a, const void* b, int32_t kind, int64_t n_tiles, int64_t n_elems,
                        int64_t a_stride_elems, int64_t b_stride_elems, double atol, double rtol, int32_t equal_nan,
                        dswx_compare_t* out, void* stream) {
    if (kind < 0 || kind >= DSWX_CMP_KINDS) return dswx_fail(DSWX_ERR_ARG, "kind %d is not a DSWX_CMP_* value", kind);
    if (n_tiles < 0 || n_elems < 0 || a_stride_elems < 0 || b_stride_elems < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (a_stride_elems == 0) a_stride_elems = n_elems;
    if (b_stride_elems == 0) b_stride_elems = n_elems;
    if (a_stride_elems < n_elems || b_stride_elems < n_elems) return dswx_fail(DSWX_ERR_ARG, "tile_stride smaller than the tile");
    const int64_t st = a_stride_elems > b_stride_elems ? a_stride_elems : b_stride_elems;
    if (n_tiles > (1LL << 32) || st > (1LL << 46) || (n_tiles && (uint64_t)st > (1ull << 46) / (uint64_t)n_tiles))
        return dswx_fail(DSWX_ERR_ARG, "plane too large");
    if (n_tiles > 0 && (!a || !b || !out)) return dswx_fail(DSWX_ERR_ARG, "NULL pointer");
    if (int rc = dswx_compare_check_tol(atol, rtol)) return rc;
    const size_t eb = (size_t)dswx_compare_elem_bytes(kind);
    if (!aligned_to(a, eb) || !aligned_to(b, eb)) return dswx_fail(DSWX_ERR_ALIGN, "plane not aligned to its %d-byte elements", (int)eb);
    if (!aligned_to(out, 8)) return dswx_fail(DSWX_ERR_ALIGN, "out not 8-byte aligned");
    const dswx_compare_pair pr = {a, b, kind, (uint64_t)n_elems, (uint64_t)a_stride_elems, (uint64_t)b_stride_elems};
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) { return dswx_compare_launch(ctx, &pr, 1, n_tiles, atol, rtol, equal_nan, out, s); });
}

}  // extern "C"
