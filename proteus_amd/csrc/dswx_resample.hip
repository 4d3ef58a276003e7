// dswx_resample.hip -- the tiles of a float32 or int16 plane INTERPOLATED onto another lattice through a mesh of source
// coordinates, bilinear and cubic (DSWX_HAS_RESAMPLE, additive to ABI v7).  include/dswx_hip.h "resample" states the definition;
// proteus_amd/resample.py is its numpy statement and dswx_resample_host below the scalar one.  The per-pixel rule -- position,
// weights, validity, the order of the double operations, the rounding to the element -- is dswx_resample_rule.h, which the
// kernel and the host entry both execute.  ARITHMETIC: every product and every sum of the rule is one IEEE double operation
// rounded on its own.  The build passes -ffp-contract=off (proteus_amd/build.py) and must keep doing so: one fused
// multiply-add and device and host no longer agree on every bit.  The kernel runs in the default floating-point mode of a
// HIP kernel on gfx950, in which float32 and double subnormals are kept.
//
// OWNERSHIP.  A workgroup of 256 threads owns a COMPACT rectangle of the destination, RECT_H = 8 rows x RECT_W = 32 columns,
// one pixel per thread (a wave stores 128 consecutive bytes of float32 per row); rectangles are numbered row-major and walked
// along grid.x, which has at most 1024 workgroups -- a workgroup per rectangle was measured: its 55460 sets of head atomics per
// tile of 3760 x 3760 cost more than the resampling --, grid.y walks the tiles (past 65535 tiles the
// workgroups of a row of the grid take several).  Not the warp
// kernel's 4 x 1024 strip: under a few degrees of rotation the source box of a strip is tall, that of a rectangle stays small.
//
// POSITIONS.  Every thread evaluates the definition's 64-bit form for its own pixel from the four nodes of its cell (eight
// int32 loads that the threads of a rectangle share through the caches) through mesh_position of dswx_mesh_rule.h, the one
// statement of the formula, which this kernel, dswx_resample_host and dswx_warp_host execute.  The warp kernel's per-cell
// linear form (mesh_cell_linear, in the same header) is not used: a thread has one pixel, not sixteen.
//
// TAPS.  The workgroup reduces the exact bounding box of the windows of its pixels (base pixel - 1 .. + 2 for cubic, 0 .. + 1
// for bilinear), clipped to the raster; pixels whose whole window misses the raster do not count.  When the box has at most
// LDS_ELEMS = 4096 elements the workgroup loads it ONCE, row by row and coalesced, each element staged as 32 bits with its
// validity resolved at load time (resample_stage), and every tap comes from LDS: a tap outside the box is a tap outside the
// raster.  Otherwise (garbage meshes, strong decimation) every pixel gathers its taps from global memory, each behind the
// comparison of its position with the raster.  Both paths hand the same staged 32 bits to the same rule, so their bits are
// equal.  The geographic DEM case has 1.0 - 2.8 source columns and about one source row per destination pixel: a box of some
// 94 x 13 elements for 256 pixels, 5 loaded elements per pixel instead of 16 gathered ones.
//
// HEAD.  As in dswx_warp.hip: one hipMemsetAsync sets every byte of `head` to 0xFF; then one set of commuting 64-bit atomics
// per workgroup and tile.  The sums (words 0 - 4, 7) start at 2^64 - 1 and the workgroup of rectangle 0 adds one more than its
// share; the minimum (5) is an unsigned minimum to which that workgroup contributes `height`, the maximum (6) a SIGNED maximum
// from -1 to which it contributes 0.  Nothing waits, nothing is ordered, a second call gives the same bytes.
//
// Vector stores only; no inline assembly.
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdio>
#include <cstring>

#include "dswx_host.h"
#include "dswx_resample_rule.h"

namespace {

constexpr int RES_BLOCK = 256;
constexpr int RES_RECT_H = DSWX_RESAMPLE_RECT_H, RES_RECT_W = DSWX_RESAMPLE_RECT_W;
constexpr int RES_LDS = DSWX_RESAMPLE_LDS_ELEMS;
constexpr unsigned RES_MAX_GRID_X = 1024;                // rectangles beyond that are walked: the head is one set of atomics per workgroup and tile
static_assert(RES_RECT_H * RES_RECT_W == RES_BLOCK, "one pixel per thread");

struct ResArgs {
    const unsigned char* plane;
    unsigned long long src_stride_bytes;                 // between tiles
    const int* mesh;
    unsigned long long mesh_stride_ints;                 // between the meshes of consecutive tiles, 0 = shared
    unsigned long long n_tiles, n_rects, dst_px;
    int height, width, dst_h, dst_w, shift, mesh_w;
    int cubic, has_nodata;
    unsigned nodata, outside, nbx;
    unsigned char* dst;
    unsigned char* how;
    unsigned long long* head;
};

template <bool F32> __device__ __forceinline__ uint32_t res_load(const unsigned char* src, uint32_t idx) {
    if (F32) return reinterpret_cast<const uint32_t*>(src)[idx];
    return reinterpret_cast<const unsigned short*>(src)[idx];
}

template <bool F32>
__global__ __launch_bounds__(RES_BLOCK) void dswx_resample_k(const ResArgs a) {
    __shared__ uint32_t win[RES_LDS];
    __shared__ int box[RES_BLOCK / 64][4];
    __shared__ int sums[RES_BLOCK / 64][6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ly = tid / RES_RECT_W, lx = tid % RES_RECT_W;
    const int lo = a.cubic ? 1 : 0, hi = a.cubic ? 2 : 1;
    const long long H = a.height, W = a.width;
    for (unsigned long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const unsigned char* const src = a.plane + t * a.src_stride_bytes;
        const int* const mesh = a.mesh + t * a.mesh_stride_ints;
        int n_cubic = 0, n_full = 0, n_renorm = 0, n_out = 0, rmin = INT_MAX, rmax = -1;
        for (unsigned long long b = blockIdx.x; b < a.n_rects; b += gridDim.x) {
            const unsigned long long by = b / a.nbx, bx = b - by * a.nbx;
            const long long Y = (long long)by * RES_RECT_H + ly, X = (long long)bx * RES_RECT_W + lx;
            const bool live = Y < a.dst_h && X < a.dst_w;
            long long sx = 0, sy = 0;
            int cl = INT_MAX, ch = -1, rl = INT_MAX, rh = -1;
            if (live) {
                int64_t px, py;
                mesh_position([&](int64_t k) { return (int64_t)mesh[k]; }, a.shift, a.mesh_w, X, Y, &px, &py);
                sx = px, sy = py;
                const long long c0 = (sx - 128) >> 8, r0 = (sy - 128) >> 8;
                // a window that meets the raster: its clipped sides are columns and rows of the raster, so they fit an int
                if (c0 + hi >= 0 && c0 - lo < W && r0 + hi >= 0 && r0 - lo < H) {
                    cl = (int)(c0 - lo > 0 ? c0 - lo : 0);
                    ch = (int)(c0 + hi < W - 1 ? c0 + hi : W - 1);
                    rl = (int)(r0 - lo > 0 ? r0 - lo : 0);
                    rh = (int)(r0 + hi < H - 1 ? r0 + hi : H - 1);
                }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const int c0 = __shfl_xor(cl, m), c1 = __shfl_xor(ch, m), r0 = __shfl_xor(rl, m), r1 = __shfl_xor(rh, m);
                cl = c0 < cl ? c0 : cl;
                ch = c1 > ch ? c1 : ch;
                rl = r0 < rl ? r0 : rl;
                rh = r1 > rh ? r1 : rh;
            }
            if (lane == 0) {
                box[wave][0] = cl;
                box[wave][1] = ch;
                box[wave][2] = rl;
                box[wave][3] = rh;
            }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < RES_BLOCK / 64; ++w) {
                cl = box[w][0] < cl ? box[w][0] : cl;
                ch = box[w][1] > ch ? box[w][1] : ch;
                rl = box[w][2] < rl ? box[w][2] : rl;
                rh = box[w][3] > rh ? box[w][3] : rh;
            }
            // the same four numbers in every thread: the decision is uniform over the workgroup
            const int bw = ch >= cl ? ch - cl + 1 : 0, bh = rh >= rl ? rh - rl + 1 : 0;
            const bool staged = (long long)bw * bh <= RES_LDS;
            ResamplePixel px;
            px.how = RESAMPLE_OUTSIDE;
            if (staged) {
                const int n = bw * bh;                                   // <= RES_LDS; every element lies in the raster
                for (int e = tid; e < n; e += RES_BLOCK) {
                    const int rr = e / bw, cc = e - rr * bw;
                    const uint32_t idx = (uint32_t)(rl + rr) * (uint32_t)a.width + (uint32_t)(cl + cc);
                    win[e] = resample_stage<F32>(res_load<F32>(src, idx), a.has_nodata, a.nodata);
                }
                __syncthreads();
                if (live)
                    px = resample_pixel(a.cubic != 0, sx, sy, [&](int64_t c, int64_t r) {
                        if (c < cl || c > ch || r < rl || r > rh) return resample_no_tap();
                        return resample_tap_of<F32>(win[(int)(r - rl) * bw + (int)(c - cl)]);
                    });
            } else if (live) {
                px = resample_pixel(a.cubic != 0, sx, sy, [&](int64_t c, int64_t r) {
                    if (c < 0 || c >= W || r < 0 || r >= H) return resample_no_tap();
                    const uint32_t idx = (uint32_t)r * (uint32_t)a.width + (uint32_t)c;
                    return resample_tap_of<F32>(resample_stage<F32>(res_load<F32>(src, idx), a.has_nodata, a.nodata));
                });
            }
            if (live) {
                const unsigned long long e = t * a.dst_px + (unsigned long long)Y * (unsigned long long)a.dst_w + (unsigned long long)X;
                if (a.dst) {
                    const uint32_t el = px.how ? resample_element<F32>(px.v) : a.outside;
                    if (F32) reinterpret_cast<uint32_t*>(a.dst)[e] = el;
                    else reinterpret_cast<unsigned short*>(a.dst)[e] = (unsigned short)el;
                }
                if (a.how) a.how[e] = (unsigned char)px.how;
                n_cubic += px.how == RESAMPLE_CUBIC_FULL;
                n_full += px.how == RESAMPLE_BILINEAR_FULL;
                n_renorm += px.how == RESAMPLE_BILINEAR_RENORM;
                n_out += px.how == RESAMPLE_OUTSIDE;
                if (px.how) {                                            // rows of valid taps: rows of the raster
                    rmin = (int)px.rlo < rmin ? (int)px.rlo : rmin;
                    rmax = (int)px.rhi > rmax ? (int)px.rhi : rmax;
                }
            }
            __syncthreads();                                             // (`win` and `box` have been read)
        }
        if (a.head) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                n_cubic += __shfl_xor(n_cubic, m);
                n_full += __shfl_xor(n_full, m);
                n_renorm += __shfl_xor(n_renorm, m);
                n_out += __shfl_xor(n_out, m);
                const int r0 = __shfl_xor(rmin, m), r1 = __shfl_xor(rmax, m);
                rmin = r0 < rmin ? r0 : rmin;
                rmax = r1 > rmax ? r1 : rmax;
            }
            if (lane == 0) {
                sums[wave][0] = n_cubic;
                sums[wave][1] = n_full;
                sums[wave][2] = n_renorm;
                sums[wave][3] = n_out;
                sums[wave][4] = rmin;
                sums[wave][5] = rmax;
            }
            __syncthreads();
            if (tid == 0) {
                long long s[4] = {0, 0, 0, 0};
                int lo_r = INT_MAX, hi_r = -1;
#pragma unroll
                for (int w = 0; w < RES_BLOCK / 64; ++w) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[k] += sums[w][k];
                    lo_r = sums[w][4] < lo_r ? sums[w][4] : lo_r;
                    hi_r = sums[w][5] > hi_r ? sums[w][5] : hi_r;
                }
                unsigned long long* const h = a.head + t * DSWX_RESAMPLE_HEAD_WORDS;
                long long* const hs = reinterpret_cast<long long*>(h);
                if (blockIdx.x == 0) {                                   // the workgroup of rectangle 0: once per tile
                    atomicAdd(h + 0, 1ull + a.dst_px);
#pragma unroll
                    for (int k = 1; k <= 4; ++k) atomicAdd(h + k, 1ull);
                    atomicAdd(h + 7, 1ull);
                    atomicMin(h + 5, (unsigned long long)a.height);
                    atomicMax(hs + 6, 0ll);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (s[k]) atomicAdd(h + 1 + k, (unsigned long long)s[k]);
                if (hi_r >= 0) {
                    atomicMin(h + 5, (unsigned long long)lo_r);
                    atomicMax(hs + 6, (long long)hi_r);
                }
            }
            __syncthreads();                                             // (`sums` has been read before the next tile writes it)
        }
    }
}

int resample_check(const void* plane, const dswx_resample_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width, const int32_t* mesh,
                   int64_t dst_h, int64_t dst_w, const dswx_resample_out_t* out, int64_t* src_stride, bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (spec->kind != DSWX_RESAMPLE_F32 && spec->kind != DSWX_RESAMPLE_I16)
        return dswx_fail(DSWX_ERR_ARG, "kind %d: not DSWX_RESAMPLE_F32 or DSWX_RESAMPLE_I16", spec->kind);
    if (spec->method != DSWX_RESAMPLE_BILINEAR && spec->method != DSWX_RESAMPLE_CUBIC)
        return dswx_fail(DSWX_ERR_ARG, "method %d: not DSWX_RESAMPLE_BILINEAR or DSWX_RESAMPLE_CUBIC", spec->method);
    if (spec->reserved2 != 0) return dswx_fail(DSWX_ERR_ARG, "reserved2 is %d, not 0", spec->reserved2);
    if (int rc = dswx_mesh_geometry_check(spec->shift, spec->reserved, spec->src_tile_stride,
                                          spec->mesh_tile_stride_nodes, n_tiles, height, width, dst_h, dst_w, src_stride))
        return rc;
    const bool work = dswx_mesh_work(n_tiles, dst_h, dst_w, out->dst || out->how || out->head);
    return dswx_mesh_pointer_check(work, plane, height * width > 0 /* every output reads it */, spec->kind == DSWX_RESAMPLE_F32 ? 4 : 2, mesh,
                                   out->dst, nullptr, out->head, align);
}

template <bool F32>
void resample_host_tiles(const unsigned char* src, const dswx_resample_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                         int64_t stride, const int32_t* mesh, int64_t dst_h, int64_t dst_w, const dswx_resample_out_t* out) {
    const int s = spec->shift;
    const size_t eb = F32 ? 4 : 2;
    const int64_t mesh_w = mesh_dims(dst_w, s);
    unsigned char* const dst = static_cast<unsigned char*>(out->dst);
    const uint32_t outside = spec->outside;              // (little endian: its low bytes come first)
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t m0 = 2 * t * spec->mesh_tile_stride_nodes;
        const unsigned char* const tile = src + (size_t)t * (size_t)stride * eb;
        uint64_t n[4] = {0, 0, 0, 0};                    // by `how`
        int64_t rmin = height, rmax = 0;
        for (int64_t Y = 0; Y < dst_h; ++Y)
            for (int64_t X = 0; X < dst_w; ++X) {
                int64_t sx, sy;
                mesh_position([&](int64_t k) { return dswx_load<int32_t>(mesh, (size_t)(m0 + k)); }, s, mesh_w, X, Y, &sx, &sy);
                const ResamplePixel px = resample_pixel(spec->method == DSWX_RESAMPLE_CUBIC, sx, sy, [&](int64_t c, int64_t r) {
                    if (c < 0 || c >= width || r < 0 || r >= height) return resample_no_tap();
                    uint32_t raw = 0;
                    std::memcpy(&raw, tile + (size_t)(r * width + c) * eb, eb);
                    return resample_tap_of<F32>(resample_stage<F32>(raw, spec->has_nodata, spec->nodata));
                });
                const int64_t e = t * dst_h * dst_w + Y * dst_w + X;
                if (dst) {
                    const uint32_t el = px.how ? resample_element<F32>(px.v) : outside;
                    std::memcpy(dst + (size_t)e * eb, &el, eb);
                }
                if (out->how) out->how[e] = (uint8_t)px.how;
                ++n[px.how];
                if (px.how) {
                    rmin = px.rlo < rmin ? px.rlo : rmin;
                    rmax = px.rhi > rmax ? px.rhi : rmax;
                }
            }
        if (out->head) {
            const uint64_t words[DSWX_RESAMPLE_HEAD_WORDS] = {(uint64_t)dst_h * (uint64_t)dst_w, n[RESAMPLE_CUBIC_FULL], n[RESAMPLE_BILINEAR_FULL],
                                                               n[RESAMPLE_BILINEAR_RENORM], n[RESAMPLE_OUTSIDE], (uint64_t)rmin, (uint64_t)rmax, 0};
            std::memcpy(reinterpret_cast<unsigned char*>(out->head) + (size_t)t * sizeof words, words, sizeof words);
        }
    }
}

}  // namespace

extern "C" {

int dswx_resample_host(const void* plane, const dswx_resample_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                       const int32_t* mesh, int64_t dst_h, int64_t dst_w, const dswx_resample_out_t* out) {
    int64_t stride;
    if (int rc = resample_check(plane, spec, n_tiles, height, width, mesh, dst_h, dst_w, out, &stride, false)) return rc;
    if (!dswx_mesh_work(n_tiles, dst_h, dst_w, out->dst || out->how || out->head)) return DSWX_OK;
    const unsigned char* const src = static_cast<const unsigned char*>(plane);
    if (spec->kind == DSWX_RESAMPLE_F32) resample_host_tiles<true>(src, spec, n_tiles, height, width, stride, mesh, dst_h, dst_w, out);
    else resample_host_tiles<false>(src, spec, n_tiles, height, width, stride, mesh, dst_h, dst_w, out);
    return DSWX_OK;
}

int dswx_resample_device(dswx_ctx_t* ctx, const void* plane, const dswx_resample_spec_t* spec, int64_t n_tiles, int64_t height,
                         int64_t width, const int32_t* mesh, int64_t dst_h, int64_t dst_w, const dswx_resample_out_t* out, void* stream) {
    int64_t stride;
    if (int rc = resample_check(plane, spec, n_tiles, height, width, mesh, dst_h, dst_w, out, &stride, true)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) -> int {
        if (!dswx_mesh_work(n_tiles, dst_h, dst_w, out->dst || out->how || out->head)) {
            ctx->last_kernel = DSWX_NO_KERNEL;
            return DSWX_OK;
        }
        const bool f32 = spec->kind == DSWX_RESAMPLE_F32;
        ResArgs a = {};
        unsigned gy;
        if (int rc = dswx_mesh_launch_prepare(a, plane, stride, f32 ? 4 : 2, mesh, spec->mesh_tile_stride_nodes, spec->shift, n_tiles, height, width,
                                              dst_h, dst_w, RES_RECT_H, RES_RECT_W, out->dst, out->head, s, &gy))
            return rc;
        a.cubic = spec->method == DSWX_RESAMPLE_CUBIC;
        a.has_nodata = spec->has_nodata != 0;
        a.nodata = spec->nodata;
        a.outside = spec->outside;
        a.how = out->how;
        const unsigned gx = (unsigned)(a.n_rects < RES_MAX_GRID_X ? a.n_rects : RES_MAX_GRID_X);
        const dim3 grid(gx, gy), block(RES_BLOCK);
        if (f32) hipLaunchKernelGGL((dswx_resample_k<true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((dswx_resample_k<false>), grid, block, 0, s, a);
        HIP_TRY(hipGetLastError());
        char info[256];
        snprintf(info, sizeof info, "dswx_resample_k grid=(%u,%u,1) block=%d rect=%dx%d lds_elems=%d kind=%s method=%s shift=%d head=%d", gx, gy,
                 RES_BLOCK, RES_RECT_H, RES_RECT_W, RES_LDS, f32 ? "f32" : "i16", a.cubic ? "cubic" : "bilinear", spec->shift, out->head ? 1 : 0);
        ctx->last_kernel = info;
        return DSWX_OK;
    });
}

}  // extern "C"
