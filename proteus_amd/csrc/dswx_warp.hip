// dswx_warp.hip -- the tiles of a plane resampled onto another lattice through a mesh of source coordinates, nearest pixel
// (DSWX_HAS_WARP, additive to ABI v7).  include/dswx_hip.h "warp" states the definition; proteus_amd/warp.py is its numpy
// statement and dswx_warp_host below the scalar one.  The device sees integers only: the projection that made the mesh stays
// on the host (proteus_amd/warp.py), as the polygons of dswx_burn.hip do.
//
// OWNERSHIP.  A workgroup of 256 threads owns a rectangle of the destination, WARP_ROWS = 4 rows x WARP_COLS = 1024 columns,
// rectangles numbered row-major and walked along grid.x; grid.y walks the tiles (past 65535 tiles the workgroups of a row of
// the grid take several).  One wave owns each row; a thread owns WARP_PPT = 16 consecutive destination pixels of its row, a
// unit, which never straddles a destination row.  The last unit of a row (dst_w % 16 pixels) is stored element by element.
//
// POSITIONS.  dswx_mesh_rule.h states them: the definition (mesh_position: dswx_warp_host below and the resample entries) and
// the form this kernel uses, the definition's numerator within one mesh cell, num = A + fx * B in 64-bit integers
// (mesh_cell_linear); tests/native/mesh_host_san.cpp runs both on the host and holds them equal over whole cells.  With
// shift >= 4 the unit of a thread lies in ONE cell (its first column is a multiple of 16 and so is the step): the thread reads
// the four nodes once -- 32 bytes that four to sixteen neighbouring threads share through the caches -- and advances the two
// numerators by B per pixel; the rounding shift and the floor to a pixel are one 64-bit arithmetic shift by 2 * shift + 8.
// The coefficients are 32 x 32 -> 64 bit products (the weights are at most 256).  THE COMMON CASE then leaves 64 bits: when
// both slopes are below four source pixels per destination pixel and both sides of the raster below 2^23, the thread splits
// its first numerator into a pixel c0 and a fraction f < 2^(2 shift + 8) <= 2^24 and pixel k lies at c0 + ((f + k * b) >>
// (2 shift + 8)) in 32-bit arithmetic, exactly.  A floored linear function steps by m or m + 1 per pixel, so the unit is a run
// of 16 consecutive source pixels iff its LAST pixel lies 15 columns and no row from its first: two positions decide, not 16.
// Any other mesh (garbage, a scale above four, a raster side of 2^23 or more) takes the 64-bit form per pixel.
// With shift < 4 (a mesh almost as dense as the destination) a unit crosses cells and every pixel evaluates its own cell (the
// FINE instantiation): correct and slow, four cached node reads per pixel.  NOT staged in LDS, where the issue's sketch put the
// nodes of a block: at shift 6 a block of 4 x 1024 pixels touches 2 x 17 nodes, read through L1/L2 by the 256 threads as
// 8-byte loads.
//
// THE COPY.  A pixel's source element is plane[r * width + c].  Where the 16 source indices of a unit are all inside and
// CONSECUTIVE (idx[k] == idx[0] + k: the same source row, or a row's end running into the next row's start -- memory is
// contiguous there and every element is still the right one) the unit is ONE unaligned load of 16 * elem_bytes bytes (gfx950
// performs unaligned 16-byte global accesses in hardware; the classify kernel's unaligned path is the precedent) and one
// store.  All 16 indices being inside the raster is what keeps that load inside the first height * width elements of the
// tile.  Otherwise the unit is up to 16 element loads, all issued before the first is used, each behind the comparison of its
// position with the raster.  Neighbouring UTM zones are rotated against each other by a few degrees, so a destination row
// follows a source row for some 15 - 40 pixels: most units are consecutive, the rest are cut once.
//
// HEAD.  One hipMemsetAsync sets every byte of `head` to 0xFF; then ONE set of 64-bit atomics per workgroup and tile, all of
// them commuting: the sums (words 0 - 2, 7) start at 2^64 - 1 and the workgroup that owns rectangle 0 of the tile adds one
// more than its share, which wraps them to the counts; the minima (3, 5) are unsigned minima from 2^64 - 1, to which that
// workgroup also contributes `height` and `width`; the maxima (4, 6) are SIGNED maxima from -1, to which it contributes 0.
// Nothing waits, nothing is ordered, and a second call gives the same bytes.
//
// Measured: tools/warp_rate.py, DESIGN.md section 5.
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdio>
#include <cstring>

#include "dswx_host.h"

namespace {

typedef u32x4 __attribute__((aligned(1))) u32x4_b;      // 16 bytes anywhere
typedef u32x2 __attribute__((aligned(4))) u32x2_w;      // a mesh node: two int32 at a 4-byte aligned address

constexpr int WARP_BLOCK = 256;
constexpr int WARP_PPT = 16;                             // destination pixels per thread
constexpr int WARP_ROWS = WARP_BLOCK / 64;               // destination rows of a rectangle: one wave each
constexpr int WARP_COLS = 64 * WARP_PPT;                 // destination columns of a rectangle
constexpr unsigned WARP_MAX_GRID_X = 1u << 20;           // rectangles beyond that are walked
constexpr int64_t WARP_MAX_PIXELS = 1LL << 30;

struct WarpArgs {
    const unsigned char* plane;
    unsigned long long src_stride_bytes;                 // between tiles
    const int* mesh;
    unsigned long long mesh_stride_ints;                 // between the meshes of consecutive tiles, 0 = shared
    unsigned long long n_tiles, n_rects, dst_px;
    int height, width, dst_h, dst_w, shift, mesh_w;
    int thin;                                            // both sides of the raster below 2^23: r * width + c in 24-bit factors
    unsigned outside, nbx;
    unsigned char* dst;
    unsigned* src_index;
    unsigned long long* head;
};

// the coefficients of one cell and destination row: num_x = ax + fx * bx, num_y = ay + fx * by
__device__ __forceinline__ void warp_cell(const int* mesh, long long node, int mesh_w, long long step, long long fy, long long& ax,
                                          long long& bx, long long& ay, long long& by) {
    const u32x2 n00 = *reinterpret_cast<const u32x2_w*>(mesh + 2 * node);
    const u32x2 n01 = *reinterpret_cast<const u32x2_w*>(mesh + 2 * (node + 1));
    const u32x2 n10 = *reinterpret_cast<const u32x2_w*>(mesh + 2 * (node + mesh_w));
    const u32x2 n11 = *reinterpret_cast<const u32x2_w*>(mesh + 2 * (node + mesh_w + 1));
    const int gy = (int)(step - fy), hy = (int)fy, s = __builtin_ctzll((unsigned long long)step);
    mesh_cell_linear((int)n00[0], (int)n01[0], (int)n10[0], (int)n11[0], gy, hy, s, ax, bx);
    mesh_cell_linear((int)n00[1], (int)n01[1], (int)n10[1], (int)n11[1], gy, hy, s, ay, by);
}

template <int EB> __device__ __forceinline__ uint32_t warp_load(const unsigned char* src, uint32_t idx) {
    if (EB == 1) return src[idx];
    if (EB == 2) return reinterpret_cast<const unsigned short*>(src)[idx];
    return reinterpret_cast<const uint32_t*>(src)[idx];
}
template <int EB> __device__ __forceinline__ void warp_store(unsigned char* dst, int k, uint32_t v) {
    if (EB == 1) dst[k] = (unsigned char)v;
    else if (EB == 2) reinterpret_cast<unsigned short*>(dst)[k] = (unsigned short)v;
    else reinterpret_cast<uint32_t*>(dst)[k] = v;
}

// EB: bytes per element.  FINE: shift < 4, a unit crosses mesh cells and every pixel evaluates its own.
template <int EB, bool FINE>
__global__ __launch_bounds__(WARP_BLOCK) void dswx_warp_k(const WarpArgs a) {
    __shared__ int red[WARP_ROWS][5];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = a.shift;
    const long long step = 1ll << s;
    const int down = 2 * s + 8;                                          // rounding shift and floor to a pixel in one
    const long long half = s ? 1ll << (2 * s - 1) : 0;
    const uint32_t emask = EB == 4 ? 0xffffffffu : (1u << (8 * EB)) - 1u;
    const uint32_t outside = a.outside & emask;
    for (unsigned long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const unsigned char* const src = a.plane + t * a.src_stride_bytes;
        const int* const mesh = a.mesh + t * a.mesh_stride_ints;
        int n_in = 0, rmin = INT_MAX, rmax = -1, cmin = INT_MAX, cmax = -1;
        for (unsigned long long b = blockIdx.x; b < a.n_rects; b += gridDim.x) {
            const unsigned long long by = b / a.nbx, bx = b - by * a.nbx;
            const long long Y = (long long)by * WARP_ROWS + wave, X = (long long)bx * WARP_COLS + (long long)lane * WARP_PPT;
            if (Y >= a.dst_h || X >= a.dst_w) continue;
            const int nvalid = a.dst_w - X < WARP_PPT ? (int)(a.dst_w - X) : WARP_PPT;
            const long long i = Y >> s, fy = Y & (step - 1);
            int c[WARP_PPT], r[WARP_PPT];
            uint32_t idx[WARP_PPT];                                      // r * width + c < 2^30 where inside, else DSWX_WARP_OUTSIDE
            unsigned in = 0;                                             // bit k: pixel k is inside the source raster
            bool run = false;                                            // the 16 source pixels are inside and consecutive
            bool decided = false;                                        // ... and `run` says so already
            if (!FINE) {
                long long ax, bxx, ay, byy;
                warp_cell(mesh, i * a.mesh_w + (X >> s), a.mesh_w, step, fy, ax, bxx, ay, byy);
                const long long fx0 = X & (step - 1);
                long long nx = ax + fx0 * bxx + half, ny = ay + fx0 * byy + half;
                const long long lim = 1ll << (down + 2);                 // fewer than four source pixels per destination pixel
                if (a.thin && bxx > -lim && bxx < lim && byy > -lim && byy < lim) {
                    // THE COMMON CASE in 32 bits: nx = c0 * 2^down + f with 0 <= f < 2^down <= 2^24, so pixel k lies at column
                    // c0 + ((f + k * bx) >> down), and |15 * bx| < 2^30.  c0 is clamped to a range around the raster: a
                    // clamped position was outside and, moving by fewer than 60 pixels, stays outside.
                    decided = true;
                    const long long top = (1ll << 30) + 128;
                    long long c0l = nx >> down, r0l = ny >> down;
                    c0l = c0l < -128 ? -128 : (c0l > top ? top : c0l);
                    r0l = r0l < -128 ? -128 : (r0l > top ? top : r0l);
                    const int c0 = (int)c0l, r0 = (int)r0l, bx32 = (int)bxx, by32 = (int)byy;
                    int fxf = (int)(nx & ((1ll << down) - 1)), fyf = (int)(ny & ((1ll << down) - 1));
                    // a linear function floored steps by m or m + 1 per pixel: if the last pixel lies 15 columns and no row
                    // from the first, every step was one column and no row
                    const int c15 = c0 + ((fxf + 15 * bx32) >> down), r15 = r0 + ((fyf + 15 * by32) >> down);
                    run = nvalid == WARP_PPT && r15 == r0 && c15 == c0 + 15 && (unsigned)r0 < (unsigned)a.height && c0 >= 0 && c15 < a.width;
                    if (run) {
                        c[0] = c0;
                        r[0] = r0;
                        in = 0xffffu;
                        const uint32_t first = (uint32_t)__mul24(r0, a.width) + (uint32_t)c0;
#pragma unroll
                        for (int k = 0; k < WARP_PPT; ++k) idx[k] = first + (uint32_t)k;
                    } else {
#pragma unroll
                        for (int k = 0; k < WARP_PPT; ++k) {
                            const int cc = c0 + (fxf >> down), rr = r0 + (fyf >> down);
                            const bool ok = (unsigned)cc < (unsigned)a.width && (unsigned)rr < (unsigned)a.height && k < nvalid;
                            c[k] = cc;
                            r[k] = rr;
                            in |= ok ? 1u << k : 0u;
                            idx[k] = ok ? (uint32_t)__mul24(rr, a.width) + (uint32_t)cc : DSWX_WARP_OUTSIDE;      // sides below 2^23
                            fxf += bx32;
                            fyf += by32;
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < WARP_PPT; ++k) {
                        const long long cc = nx >> down, rr = ny >> down;
                        const bool ok = (unsigned long long)cc < (unsigned long long)a.width && (unsigned long long)rr < (unsigned long long)a.height && k < nvalid;
                        c[k] = (int)cc;
                        r[k] = (int)rr;
                        in |= ok ? 1u << k : 0u;
                        idx[k] = ok ? (uint32_t)rr * (uint32_t)a.width + (uint32_t)cc : DSWX_WARP_OUTSIDE;
                        nx += bxx;
                        ny += byy;
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < WARP_PPT; ++k) {
                    c[k] = r[k] = -1;
                    idx[k] = DSWX_WARP_OUTSIDE;
                    if (k < nvalid) {                                    // (a pixel past the destination's edge may have no cell)
                        long long ax, bxx, ay, byy;
                        const long long Xk = X + k, fx = Xk & (step - 1);
                        warp_cell(mesh, i * a.mesh_w + (Xk >> s), a.mesh_w, step, fy, ax, bxx, ay, byy);
                        const long long cc = (ax + fx * bxx + half) >> down, rr = (ay + fx * byy + half) >> down;
                        const bool ok = (unsigned long long)cc < (unsigned long long)a.width && (unsigned long long)rr < (unsigned long long)a.height;
                        c[k] = (int)cc;
                        r[k] = (int)rr;
                        in |= ok ? 1u << k : 0u;
                        if (ok) idx[k] = (uint32_t)rr * (uint32_t)a.width + (uint32_t)cc;
                    }
                }
            }
            if (!decided) {
                run = in == 0xffffu;
#pragma unroll
                for (int k = 1; k < WARP_PPT; ++k) run = run && idx[k] == idx[0] + (uint32_t)k;
            }
            const unsigned long long e = t * a.dst_px + (unsigned long long)Y * (unsigned long long)a.dst_w + (unsigned long long)X;
            if (a.dst) {
                unsigned char* const out = a.dst + e * EB;
                if (run) {
                    // 16 consecutive elements, all of them elements of this tile's raster: one load, one store
                    const unsigned char* const from = src + (unsigned long long)idx[0] * EB;
                    u32x4 v[EB];
#pragma unroll
                    for (int q = 0; q < EB; ++q) v[q] = ldg_u<u32x4_b, u32x4, false>(from + 16 * q);
#pragma unroll
                    for (int q = 0; q < EB; ++q) stg_u<u32x4_b, u32x4, false>(out + 16 * q, v[q]);
                } else {
                    uint32_t el[WARP_PPT];
#pragma unroll
                    for (int k = 0; k < WARP_PPT; ++k) el[k] = ((in >> k) & 1u) ? warp_load<EB>(src, idx[k]) : outside;
                    if (nvalid == WARP_PPT) {
                        u32x4 v[EB];
#pragma unroll
                        for (int q = 0; q < EB; ++q) v[q] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                        for (int k = 0; k < WARP_PPT; ++k) {
                            constexpr int bits = 8 * EB;
                            const int p = k * bits;
                            v[p / 128][(p % 128) / 32] |= el[k] << (p % 32);
                        }
#pragma unroll
                        for (int q = 0; q < EB; ++q) stg_u<u32x4_b, u32x4, false>(out + 16 * q, v[q]);
                    } else {
#pragma unroll
                        for (int k = 0; k < WARP_PPT; ++k)
                            if (k < nvalid) warp_store<EB>(out, k, el[k]);
                    }
                }
            }
            if (a.src_index) {
                unsigned* const out = a.src_index + e;
                if (nvalid == WARP_PPT) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        stg_u<u32x4_b, u32x4, false>(out + 4 * q, u32x4{idx[4 * q], idx[4 * q + 1], idx[4 * q + 2], idx[4 * q + 3]});
                } else {
#pragma unroll
                    for (int k = 0; k < WARP_PPT; ++k)
                        if (k < nvalid) out[k] = idx[k];
                }
            }
            if (a.head) {
                n_in += __popc(in);
                if (run && decided) {                                    // one source row r[0], columns c[0] .. c[0] + 15
                    rmin = r[0] < rmin ? r[0] : rmin;
                    rmax = r[0] > rmax ? r[0] : rmax;
                    cmin = c[0] < cmin ? c[0] : cmin;
                    cmax = c[0] + WARP_PPT - 1 > cmax ? c[0] + WARP_PPT - 1 : cmax;
                } else {
#pragma unroll
                    for (int k = 0; k < WARP_PPT; ++k)
                        if ((in >> k) & 1u) {
                            rmin = r[k] < rmin ? r[k] : rmin;
                            rmax = r[k] > rmax ? r[k] : rmax;
                            cmin = c[k] < cmin ? c[k] : cmin;
                            cmax = c[k] > cmax ? c[k] : cmax;
                        }
                }
            }
        }
        if (a.head) {
            // per-workgroup sums, then one set of atomics (the file comment has the arithmetic of the 0xFF start)
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                n_in += __shfl_xor(n_in, m);
                const int r0 = __shfl_xor(rmin, m), r1 = __shfl_xor(rmax, m), c0 = __shfl_xor(cmin, m), c1 = __shfl_xor(cmax, m);
                rmin = r0 < rmin ? r0 : rmin;
                rmax = r1 > rmax ? r1 : rmax;
                cmin = c0 < cmin ? c0 : cmin;
                cmax = c1 > cmax ? c1 : cmax;
            }
            __syncthreads();                                             // (the previous tile's sums have been read)
            if (lane == 0) {
                red[wave][0] = n_in;
                red[wave][1] = rmin;
                red[wave][2] = rmax;
                red[wave][3] = cmin;
                red[wave][4] = cmax;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                long long sum = 0;
#pragma unroll
                for (int w = 0; w < WARP_ROWS; ++w) {
                    sum += red[w][0];
                    rmin = red[w][1] < rmin ? red[w][1] : rmin;
                    rmax = red[w][2] > rmax ? red[w][2] : rmax;
                    cmin = red[w][3] < cmin ? red[w][3] : cmin;
                    cmax = red[w][4] > cmax ? red[w][4] : cmax;
                }
                unsigned long long* const h = a.head + t * DSWX_WARP_HEAD_WORDS;
                long long* const hs = reinterpret_cast<long long*>(h);
                if (blockIdx.x == 0) {                                   // the workgroup of rectangle 0: once per tile
                    atomicAdd(h + 0, 1ull + a.dst_px);
                    atomicAdd(h + 1, 1ull);
                    atomicAdd(h + 2, 1ull + a.dst_px);
                    atomicAdd(h + 7, 1ull);
                    atomicMin(h + 3, (unsigned long long)a.height);
                    atomicMin(h + 5, (unsigned long long)a.width);
                    atomicMax(hs + 4, 0ll);
                    atomicMax(hs + 6, 0ll);
                }
                if (sum) {
                    atomicAdd(h + 1, (unsigned long long)sum);
                    atomicAdd(h + 2, 0ull - (unsigned long long)sum);
                    atomicMin(h + 3, (unsigned long long)rmin);
                    atomicMax(hs + 4, (long long)rmax);
                    atomicMin(h + 5, (unsigned long long)cmin);
                    atomicMax(hs + 6, (long long)cmax);
                }
            }
        }
    }
}

// unaligned host accesses (a host buffer may sit at any address)
template <typename T> inline void put_at(void* base, int64_t i, T v) {
    std::memcpy(reinterpret_cast<unsigned char*>(base) + (size_t)i * sizeof(T), &v, sizeof(T));
}

}  // namespace

// What every entry that reads a plane through a mesh checks of its geometry (the warp and the resample entries), with the
// texts of the warp entries: shift, reserved, sizes, strides.  Resolves the stride of the plane (0 = height * width).
int dswx_mesh_geometry_check(int shift, int reserved, int64_t src_tile_stride, int64_t mesh_tile_stride_nodes, int64_t n_tiles,
                             int64_t height, int64_t width, int64_t dst_h, int64_t dst_w, int64_t* src_stride) {
    if (shift < 0 || shift > DSWX_WARP_MAX_SHIFT)
        return dswx_fail(DSWX_ERR_ARG, "shift %d outside 0 .. %d", shift, DSWX_WARP_MAX_SHIFT);
    if (reserved != 0) return dswx_fail(DSWX_ERR_ARG, "reserved is %d, not 0", reserved);
    if (n_tiles < 0 || height < 0 || width < 0 || dst_h < 0 || dst_w < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (src_tile_stride < 0 || mesh_tile_stride_nodes < 0) return dswx_fail(DSWX_ERR_ARG, "negative stride");
    if (height > WARP_MAX_PIXELS || width > WARP_MAX_PIXELS || (width && height > WARP_MAX_PIXELS / width))
        return dswx_fail(DSWX_ERR_ARG, "raster %lld x %lld above 2^30 pixels", (long long)height, (long long)width);
    if (dst_h > WARP_MAX_PIXELS || dst_w > WARP_MAX_PIXELS || (dst_w && dst_h > WARP_MAX_PIXELS / dst_w))
        return dswx_fail(DSWX_ERR_ARG, "destination %lld x %lld above 2^30 pixels", (long long)dst_h, (long long)dst_w);
    const int64_t n_elems = height * width;
    *src_stride = src_tile_stride ? src_tile_stride : n_elems;
    if (*src_stride < n_elems) return dswx_fail(DSWX_ERR_ARG, "src_tile_stride smaller than the tile");
    const int64_t mesh_h = mesh_dims(dst_h, shift), mesh_w = mesh_dims(dst_w, shift);
    if (mesh_tile_stride_nodes && mesh_tile_stride_nodes < mesh_h * mesh_w)
        return dswx_fail(DSWX_ERR_ARG, "mesh_tile_stride_nodes %lld smaller than the mesh (%lld x %lld nodes)",
                         (long long)mesh_tile_stride_nodes, (long long)mesh_h, (long long)mesh_w);
    if (n_tiles > (1LL << 32)) return dswx_fail(DSWX_ERR_ARG, "more than 2^32 tiles");
    if (*src_stride > (1LL << 46) || (n_tiles && (uint64_t)*src_stride > (1ull << 46) / (uint64_t)n_tiles))
        return dswx_fail(DSWX_ERR_ARG, "plane too large");
    if (mesh_tile_stride_nodes > (1LL << 46) || (n_tiles && (uint64_t)mesh_tile_stride_nodes > (1ull << 46) / (uint64_t)n_tiles))
        return dswx_fail(DSWX_ERR_ARG, "mesh too large");
    return DSWX_OK;
}

int dswx_mesh_pointer_check(bool work, const void* plane, bool plane_read, int elem_bytes, const int32_t* mesh, const void* dst,
                            const uint32_t* src_index, const uint64_t* head, bool align) {
    if (work && !mesh) return dswx_fail(DSWX_ERR_ARG, "mesh is NULL");
    if (work && !plane && plane_read) return dswx_fail(DSWX_ERR_ARG, "plane is NULL");
    if (align) {
        if (!aligned_to(mesh, 4)) return dswx_fail(DSWX_ERR_ALIGN, "mesh not 4-byte aligned");
        if (!aligned_to(src_index, 4)) return dswx_fail(DSWX_ERR_ALIGN, "src_index not 4-byte aligned");
        if (!aligned_to(head, 8)) return dswx_fail(DSWX_ERR_ALIGN, "head not 8-byte aligned");
        if (!aligned_to(plane, (size_t)elem_bytes)) return dswx_fail(DSWX_ERR_ALIGN, "plane not %d-byte aligned", elem_bytes);
        if (!aligned_to(dst, (size_t)elem_bytes)) return dswx_fail(DSWX_ERR_ALIGN, "dst not %d-byte aligned", elem_bytes);
    }
    return DSWX_OK;
}

// The checks that the device and the host entry share, in the house order: the arguments before any context, nothing written by
// a refused call.  Resolves the two strides of the spec (0 = height * width; 0 = shared mesh stays 0).  `align`: the device entry.
int dswx_warp_check(const void* plane, const dswx_warp_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                    const int32_t* mesh, int64_t dst_h, int64_t dst_w, const dswx_warp_out_t* out, int64_t* src_stride, bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (spec->elem_bytes != 1 && spec->elem_bytes != 2 && spec->elem_bytes != 4)
        return dswx_fail(DSWX_ERR_ARG, "elem_bytes %d: not 1, 2 or 4", spec->elem_bytes);
    if (int rc = dswx_mesh_geometry_check(spec->shift, spec->reserved, spec->src_tile_stride, spec->mesh_tile_stride_nodes, n_tiles, height,
                                          width, dst_h, dst_w, src_stride))
        return rc;
    const bool work = dswx_mesh_work(n_tiles, dst_h, dst_w, out->dst || out->src_index || out->head);
    return dswx_mesh_pointer_check(work, plane, height * width > 0 && out->dst, spec->elem_bytes, mesh, out->dst, out->src_index, out->head, align);
}

// One memset (of `head`, if wanted) and one launch; the arguments have passed dswx_warp_check, `src_stride` is the resolved
// stride of the plane in elements (a batch has its own).
int dswx_warp_launch(dswx_ctx* ctx, const void* plane, const dswx_warp_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                     int64_t src_stride, const int32_t* mesh, int64_t dst_h, int64_t dst_w, const dswx_warp_out_t* out, hipStream_t s) {
    if (!dswx_mesh_work(n_tiles, dst_h, dst_w, out->dst || out->src_index || out->head)) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    const int eb = spec->elem_bytes;
    WarpArgs a = {};
    unsigned gy;
    if (int rc = dswx_mesh_launch_prepare(a, plane, src_stride, eb, mesh, spec->mesh_tile_stride_nodes, spec->shift, n_tiles, height, width,
                                          dst_h, dst_w, WARP_ROWS, WARP_COLS, out->dst, out->head, s, &gy))
        return rc;
    a.outside = spec->outside;
    a.thin = height < (1 << 23) && width < (1 << 23);
    a.src_index = out->src_index;
    const unsigned gx = (unsigned)(a.n_rects < WARP_MAX_GRID_X ? a.n_rects : WARP_MAX_GRID_X);
    const dim3 grid(gx, gy), block(WARP_BLOCK);
    const bool fine = spec->shift < 4;
    if (eb == 1 && fine) hipLaunchKernelGGL((dswx_warp_k<1, true>), grid, block, 0, s, a);
    else if (eb == 1) hipLaunchKernelGGL((dswx_warp_k<1, false>), grid, block, 0, s, a);
    else if (eb == 2 && fine) hipLaunchKernelGGL((dswx_warp_k<2, true>), grid, block, 0, s, a);
    else if (eb == 2) hipLaunchKernelGGL((dswx_warp_k<2, false>), grid, block, 0, s, a);
    else if (fine) hipLaunchKernelGGL((dswx_warp_k<4, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((dswx_warp_k<4, false>), grid, block, 0, s, a);
    HIP_TRY(hipGetLastError());
    char info[256];
    snprintf(info, sizeof info, "dswx_warp_k grid=(%u,%u,1) block=%d rect=%dx%d pixels_per_thread=%d elem_bytes=%d shift=%d fine=%d head=%d",
             gx, gy, WARP_BLOCK, WARP_ROWS, WARP_COLS, WARP_PPT, eb, spec->shift, fine ? 1 : 0, out->head ? 1 : 0);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_warp_host(const void* plane, const dswx_warp_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                   const int32_t* mesh, int64_t dst_h, int64_t dst_w, const dswx_warp_out_t* out) {
    int64_t stride;
    if (int rc = dswx_warp_check(plane, spec, n_tiles, height, width, mesh, dst_h, dst_w, out, &stride, false)) return rc;
    if (!dswx_mesh_work(n_tiles, dst_h, dst_w, out->dst || out->src_index || out->head)) return DSWX_OK;
    const int s = spec->shift, eb = spec->elem_bytes;
    const int64_t mesh_w = mesh_dims(dst_w, s);
    const unsigned char* const src = static_cast<const unsigned char*>(plane);
    unsigned char* const dst = static_cast<unsigned char*>(out->dst);
    const uint32_t outside = spec->outside;              // (little endian: its low elem_bytes bytes come first)
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t m0 = 2 * t * spec->mesh_tile_stride_nodes;
        uint64_t inside = 0;
        int64_t rmin = height, rmax = 0, cmin = width, cmax = 0;
        for (int64_t Y = 0; Y < dst_h; ++Y)
            for (int64_t X = 0; X < dst_w; ++X) {
                int64_t sx, sy;
                mesh_position([&](int64_t k) { return dswx_load<int32_t>(mesh, (size_t)(m0 + k)); }, s, mesh_w, X, Y, &sx, &sy);
                const int64_t c = sx >> 8, r = sy >> 8;
                const bool in = c >= 0 && c < width && r >= 0 && r < height;
                const int64_t e = t * dst_h * dst_w + Y * dst_w + X;
                if (dst) std::memcpy(dst + (size_t)e * eb, in ? src + ((size_t)t * (size_t)stride + (size_t)(r * width + c)) * eb
                                                               : reinterpret_cast<const unsigned char*>(&outside), (size_t)eb);
                if (out->src_index) put_at<uint32_t>(out->src_index, e, in ? (uint32_t)(r * width + c) : DSWX_WARP_OUTSIDE);
                if (in) {
                    ++inside;
                    rmin = r < rmin ? r : rmin;
                    rmax = r > rmax ? r : rmax;
                    cmin = c < cmin ? c : cmin;
                    cmax = c > cmax ? c : cmax;
                }
            }
        if (out->head) {
            const uint64_t px = (uint64_t)dst_h * (uint64_t)dst_w;
            const uint64_t words[DSWX_WARP_HEAD_WORDS] = {px, inside, px - inside, (uint64_t)rmin, (uint64_t)rmax, (uint64_t)cmin, (uint64_t)cmax, 0};
            for (int k = 0; k < DSWX_WARP_HEAD_WORDS; ++k) put_at<uint64_t>(out->head, t * DSWX_WARP_HEAD_WORDS + k, words[k]);
        }
    }
    return DSWX_OK;
}

int dswx_warp_device(dswx_ctx_t* ctx, const void* plane, const dswx_warp_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                     const int32_t* mesh, int64_t dst_h, int64_t dst_w, const dswx_warp_out_t* out, void* stream) {
    int64_t stride;
    if (int rc = dswx_warp_check(plane, spec, n_tiles, height, width, mesh, dst_h, dst_w, out, &stride, true)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) {
        return dswx_warp_launch(ctx, plane, spec, n_tiles, height, width, stride, mesh, dst_h, dst_w, out, s);
    });
}

}  // extern "C"
