// dswx_land_mesh.hip -- the LAND layer of tiles whose two land-cover maps are NOT on the HLS grid: the WorldCover and the CGLS
// source windows read through two coordinate meshes, nearest pixel, and the 3 x 3 aggregation and class hierarchy of
// dswx_landcover_mask_* in the same kernel (DSWX_HAS_LAND_MESH, additive to ABI v7).  include/dswx_hip.h "land mesh" states the
// definition -- the chain dswx_warp_* x 2, dswx_landcover_mask_* --, proteus_amd/landmesh.py is its numpy statement and
// dswx_land_mesh_host below the scalar one.  The per-pixel rule is dswx_land_mesh_rule.h, which the kernel and the host entry
// both execute; the chain's [3H][3W] and [H][W] intermediates (10 bytes per HLS pixel written and read again) never exist.
//
// OWNERSHIP.  As dswx_resample.hip: a workgroup of 256 threads owns a rectangle of LM_RECT_H = 8 x LM_RECT_W = 32 HLS pixels,
// one pixel per thread; rectangles are numbered row-major and walked along grid.x, which has at most 1024 workgroups (the head
// is one set of atomics per workgroup and tile, not per rectangle); grid.y walks the tiles, past 65535 tiles the workgroups of
// a row of the grid take several.
//
// POSITIONS.  dswx_mesh_rule.h states them and nothing here does: every thread evaluates mesh_position for each of its nine
// fine pixels and for its HLS pixel (land_fine_taps / land_tap of the rule header, which the host entry executes too).  With
// shift_wc >= 2 a 3 x 3 block can straddle mesh cells: every fine pixel finds its own cell, which is the definition itself and
// so exact whatever the cells are.  MEASURED and taken out again: the header's per-cell linear form per fine row (a third of the
// 64-bit multiplications) left the time where it was, and garbage meshes that read no map cost as much as real ones -- the
// kernel was bound by the latency of a rectangle's dependent loads and barriers at the occupancy the registers allow more than
// by arithmetic.  __launch_bounds__(256, 4) (4 waves per SIMD for 2, no scratch), the CGLS gather issued first and dropping the
// LDS staging (TAPS) are what did help.  DESIGN.md section 5 has the figures; the bar against the chain is MISSED.
//
// TAPS.  Nine global gathers per HLS pixel, each behind the comparison of its position with the raster, through the 256-entry
// code table in LDS (land_code: water | urban << 4 | tree << 8), and one gather of the CGLS byte.  NOT staged in LDS, where the
// issue's sketch put the bounding box of a rectangle's WorldCover taps: that form was built (the box reduced over the workgroup,
// loaded once in aligned dwords when it fitted a budget, the taps read from LDS) and MEASURED against this one at budgets of 8,
// 16 and 32 KB -- gathering was faster at every mesh, 2.10 against 2.61 - 2.75 times the chain at 45 degrees N and 1.86 against
// 2.22 - 2.88 at 70: the box reduction and the staging cost two more workgroup barriers per rectangle, and
// the taps of neighbouring pixels share cache lines anyway.  So the budget chosen by measurement is none, and a rectangle has no
// barrier at all.
//
// HEAD.  Sums only: one hipMemsetAsync zeroes it, then one set of 64-bit additions per workgroup and tile; the workgroup of
// rectangle 0 adds the pixel count of word 0.  Nothing waits, nothing is ordered, a second call gives the same bytes.
//
// Vector stores only; no inline assembly.
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdio>
#include <cstring>

#include "dswx_host.h"
#include "dswx_land_mesh_rule.h"

namespace {

constexpr int LM_BLOCK = 256;
constexpr int LM_RECT_H = 8, LM_RECT_W = 32;
constexpr unsigned LM_MAX_GRID_X = 1024;
constexpr int64_t LM_MAX_PIXELS = 1LL << 30;
static_assert(LM_RECT_H * LM_RECT_W == LM_BLOCK, "one pixel per thread");

struct LandMeshArgs {
    const unsigned char* wc;
    const unsigned char* cg;
    unsigned long long wc_stride, cg_stride;             // bytes between tiles
    const int* mesh_wc;
    const int* mesh_cg;
    unsigned long long mesh_wc_stride_ints, mesh_cg_stride_ints;      // between the meshes of consecutive tiles, 0 = shared
    unsigned long long n_tiles, n_rects, px, land_stride;
    int wc_h, wc_w, cg_h, cg_w, height, width, shift_wc, shift_cg, mesh_wc_w, mesh_cg_w;
    unsigned outside_wc, outside_cg, nbx;
    LandRule rule;
    unsigned char* land;
    unsigned long long* head;
};

__global__ __launch_bounds__(LM_BLOCK, 4) void dswx_land_mesh_k(const LandMeshArgs a) {
    __shared__ uint16_t s_code[256];
    __shared__ uint8_t s_forest[256];
    __shared__ int sums[LM_BLOCK / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ly = tid / LM_RECT_W, lx = tid % LM_RECT_W;
    s_code[tid] = (uint16_t)land_code(tid);
    s_forest[tid] = (uint8_t)land_is_forest(a.rule, tid);
    __syncthreads();
    for (unsigned long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const unsigned char* const wc = a.wc + t * a.wc_stride;
        const unsigned char* const cg = a.cg + t * a.cg_stride;
        const int* const mesh_wc = a.mesh_wc + t * a.mesh_wc_stride_ints;
        const int* const mesh_cg = a.mesh_cg + t * a.mesh_cg_stride_ints;
        int n_live = 0, n_wc_in = 0, n_cg_in = 0, n_all_out = 0, n_255 = 0;
        for (unsigned long long b = blockIdx.x; b < a.n_rects; b += gridDim.x) {
            const unsigned long long by = b / a.nbx, bx = b - by * a.nbx;
            const long long Y = (long long)by * LM_RECT_H + ly, X = (long long)bx * LM_RECT_W + lx;
            const bool live = Y < a.height && X < a.width;
            unsigned in = 0;                                             // bit k: tap k is inside
            bool cg_in = false;
            uint32_t cls = a.outside_cg & 255u, cnt = 0;
            if (live) {
                // the CGLS tap first: its gather is in flight while the nine positions are evaluated
                int64_t cc, rr;
                land_tap([&](int64_t k) { return (int64_t)mesh_cg[k]; }, a.shift_cg, a.mesh_cg_w, X, Y, &cc, &rr);
                cg_in = land_inside(cc, rr, a.cg_h, a.cg_w);
                if (cg_in) cls = (uint32_t)cg[(uint32_t)rr * (uint32_t)a.cg_w + (uint32_t)cc];
                int64_t c64[9], r64[9];
                land_fine_taps([&](int64_t k) { return (int64_t)mesh_wc[k]; }, a.shift_wc, a.mesh_wc_w, X, Y, c64, r64);
                uint32_t el[9];                // every gather behind the comparison of its position with the raster, all issued before the first is used
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const bool ok = land_inside(c64[k], r64[k], a.wc_h, a.wc_w);
                    in |= ok ? 1u << k : 0u;
                    el[k] = ok ? (uint32_t)wc[(uint32_t)r64[k] * (uint32_t)a.wc_w + (uint32_t)c64[k]] : (a.outside_wc & 255u);
                }
#pragma unroll
                for (int k = 0; k < 9; ++k) cnt += s_code[el[k]];
            }
            if (live) {
                const int v = land_class(a.rule, (int)(cnt & 15u), (int)((cnt >> 4) & 15u), (int)(cnt >> 8), s_forest[cls] != 0);
                if (a.land) a.land[t * a.land_stride + (unsigned long long)Y * (unsigned long long)a.width + (unsigned long long)X] = (unsigned char)v;
                n_live += 1;
                n_wc_in += __popc(in);
                n_cg_in += cg_in;
                n_all_out += in == 0;
                n_255 += v == 255;
            }
        }
        if (a.head) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                n_live += __shfl_xor(n_live, m);
                n_wc_in += __shfl_xor(n_wc_in, m);
                n_cg_in += __shfl_xor(n_cg_in, m);
                n_all_out += __shfl_xor(n_all_out, m);
                n_255 += __shfl_xor(n_255, m);
            }
            if (lane == 0) {
                sums[wave][0] = n_live;
                sums[wave][1] = n_wc_in;
                sums[wave][2] = n_cg_in;
                sums[wave][3] = n_all_out;
                sums[wave][4] = n_255;
            }
            __syncthreads();
            if (tid == 0) {
                unsigned long long s[5] = {0, 0, 0, 0, 0};
#pragma unroll
                for (int w = 0; w < LM_BLOCK / 64; ++w)
#pragma unroll
                    for (int k = 0; k < 5; ++k) s[k] += (unsigned long long)sums[w][k];
                unsigned long long* const h = a.head + t * DSWX_LAND_MESH_HEAD_WORDS;
                if (blockIdx.x == 0) atomicAdd(h + 0, a.px);             // the workgroup of rectangle 0: once per tile
                if (s[0]) {
                    if (s[1]) atomicAdd(h + 1, s[1]);
                    if (9 * s[0] - s[1]) atomicAdd(h + 2, 9 * s[0] - s[1]);
                    if (s[2]) atomicAdd(h + 3, s[2]);
                    if (s[0] - s[2]) atomicAdd(h + 4, s[0] - s[2]);
                    if (s[3]) atomicAdd(h + 5, s[3]);
                    if (s[4]) atomicAdd(h + 6, s[4]);
                }
            }
            __syncthreads();                                             // (`sums` has been read before the next tile writes it)
        }
    }
}

struct LandMeshStrides {
    int64_t wc, cg;
};

// The checks that the device and the host entry share, in the house order: the arguments before any context, nothing written by
// a refused call.  Per map the geometry half of dswx_warp_check (its texts), then the LAND stride with land_check's text, then
// the pointers.  Resolves the two plane strides (0 = the raster).  `align`: the device entry.
int land_mesh_check(const uint8_t* worldcover, int64_t wc_h, int64_t wc_w, const uint8_t* copernicus, int64_t cg_h, int64_t cg_w,
                    const dswx_land_mesh_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width, const int32_t* mesh_wc,
                    const int32_t* mesh_cg, const uint8_t* land, const uint64_t* head, LandMeshStrides* strides, bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (spec->reserved2 != 0) return dswx_fail(DSWX_ERR_ARG, "reserved2 is %d, not 0", spec->reserved2);
    if (spec->outside_wc > 255u || spec->outside_cg > 255u)
        return dswx_fail(DSWX_ERR_ARG, "outside_wc %u / outside_cg %u outside 0 .. 255", spec->outside_wc, spec->outside_cg);
    if (spec->n_forest_classes < 0 || (spec->n_forest_classes > 0 && !spec->forest_classes)) return dswx_fail(DSWX_ERR_ARG, "bad size");
    if (height < 0 || width < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (height > LM_MAX_PIXELS / 9 || width > LM_MAX_PIXELS / 9 || (width && height > LM_MAX_PIXELS / 9 / width))
        return dswx_fail(DSWX_ERR_ARG, "lattice %lld x %lld above 2^30 / 9 pixels", (long long)height, (long long)width);
    if (int rc = dswx_mesh_geometry_check(spec->shift_wc, spec->reserved, spec->wc_tile_stride, spec->mesh_wc_tile_stride_nodes, n_tiles, wc_h,
                                          wc_w, 3 * height, 3 * width, &strides->wc))
        return rc;
    if (int rc = dswx_mesh_geometry_check(spec->shift_cg, spec->reserved, spec->cg_tile_stride, spec->mesh_cg_tile_stride_nodes, n_tiles, cg_h,
                                          cg_w, height, width, &strides->cg))
        return rc;
    if (spec->land_tile_stride < 0) return dswx_fail(DSWX_ERR_ARG, "negative stride");
    if (spec->land_tile_stride != 0 && spec->land_tile_stride < height * width)
        return dswx_fail(DSWX_ERR_ARG, "land_tile_stride smaller than the raster");
    if (int rc = dswx_tile_extent_check(spec->land_tile_stride, n_tiles, true)) return rc;
    const bool work = dswx_mesh_work(n_tiles, height, width, land || head);
    if (work && !mesh_wc) return dswx_fail(DSWX_ERR_ARG, "mesh_wc is NULL");
    if (work && !mesh_cg) return dswx_fail(DSWX_ERR_ARG, "mesh_cg is NULL");
    if (work && !worldcover && wc_h * wc_w > 0) return dswx_fail(DSWX_ERR_ARG, "worldcover is NULL");
    if (work && !copernicus && cg_h * cg_w > 0) return dswx_fail(DSWX_ERR_ARG, "copernicus is NULL");
    if (align) {
        if (!aligned_to(mesh_wc, 4)) return dswx_fail(DSWX_ERR_ALIGN, "mesh_wc not 4-byte aligned");
        if (!aligned_to(mesh_cg, 4)) return dswx_fail(DSWX_ERR_ALIGN, "mesh_cg not 4-byte aligned");
        if (!aligned_to(head, 8)) return dswx_fail(DSWX_ERR_ALIGN, "head not 8-byte aligned");
    }
    return DSWX_OK;
}

}  // namespace

extern "C" {

int dswx_land_mesh_host(const uint8_t* worldcover, int64_t wc_h, int64_t wc_w, const uint8_t* copernicus, int64_t cg_h, int64_t cg_w,
                        const dswx_land_mesh_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width, const int32_t* mesh_wc,
                        const int32_t* mesh_cg, uint8_t* land, uint64_t* head) {
    LandMeshStrides st;
    if (int rc = land_mesh_check(worldcover, wc_h, wc_w, copernicus, cg_h, cg_w, spec, n_tiles, height, width, mesh_wc, mesh_cg, land, head,
                                 &st, false))
        return rc;
    if (!dswx_mesh_work(n_tiles, height, width, land || head)) return DSWX_OK;
    LandRule rule;
    land_resolve(&rule, spec->forest_classes, spec->n_forest_classes, spec->thresholds, spec->year_offset);
    const int64_t mesh_wc_w = mesh_dims(3 * width, spec->shift_wc), mesh_cg_w = mesh_dims(width, spec->shift_cg);
    const int64_t land_stride = spec->land_tile_stride ? spec->land_tile_stride : height * width;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t m_wc = 2 * t * spec->mesh_wc_tile_stride_nodes, m_cg = 2 * t * spec->mesh_cg_tile_stride_nodes;
        const uint8_t* const wc = worldcover ? worldcover + (size_t)t * (size_t)st.wc : nullptr;
        const uint8_t* const cg = copernicus ? copernicus + (size_t)t * (size_t)st.cg : nullptr;
        uint64_t wc_in = 0, cg_in = 0, all_out = 0, n_255 = 0;
        for (int64_t Y = 0; Y < height; ++Y)
            for (int64_t X = 0; X < width; ++X) {
                const LandMeshPixel px = land_mesh_pixel(
                    rule, [&](int64_t k) { return (int64_t)dswx_load<int32_t>(mesh_wc, (size_t)(m_wc + k)); }, spec->shift_wc, mesh_wc_w, wc_h, wc_w,
                    (int)spec->outside_wc, [&](int64_t c, int64_t r) { return wc[(size_t)(r * wc_w + c)]; },
                    [&](int64_t k) { return (int64_t)dswx_load<int32_t>(mesh_cg, (size_t)(m_cg + k)); }, spec->shift_cg, mesh_cg_w, cg_h, cg_w,
                    (int)spec->outside_cg, [&](int64_t c, int64_t r) { return cg[(size_t)(r * cg_w + c)]; }, X, Y);
                if (land) land[(size_t)t * (size_t)land_stride + (size_t)(Y * width + X)] = (uint8_t)px.land;
                wc_in += (uint64_t)px.wc_inside;
                cg_in += (uint64_t)px.cg_inside;
                all_out += px.wc_inside == 0;
                n_255 += px.land == 255;
            }
        if (head) {
            const uint64_t n = (uint64_t)height * (uint64_t)width;
            const uint64_t words[DSWX_LAND_MESH_HEAD_WORDS] = {n, wc_in, 9 * n - wc_in, cg_in, n - cg_in, all_out, n_255, 0};
            std::memcpy(reinterpret_cast<unsigned char*>(head) + (size_t)t * sizeof words, words, sizeof words);
        }
    }
    return DSWX_OK;
}

int dswx_land_mesh_device(dswx_ctx_t* ctx, const uint8_t* worldcover, int64_t wc_h, int64_t wc_w, const uint8_t* copernicus, int64_t cg_h,
                          int64_t cg_w, const dswx_land_mesh_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                          const int32_t* mesh_wc, const int32_t* mesh_cg, uint8_t* land, uint64_t* head, void* stream) {
    LandMeshStrides st;
    if (int rc = land_mesh_check(worldcover, wc_h, wc_w, copernicus, cg_h, cg_w, spec, n_tiles, height, width, mesh_wc, mesh_cg, land, head,
                                 &st, true))
        return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) -> int {
        if (!dswx_mesh_work(n_tiles, height, width, land || head)) {
            ctx->last_kernel = DSWX_NO_KERNEL;
            return DSWX_OK;
        }
        LandMeshArgs a = {};
        const unsigned long long nbx = ((unsigned long long)width + LM_RECT_W - 1) / LM_RECT_W,
                                 nby = ((unsigned long long)height + LM_RECT_H - 1) / LM_RECT_H;
        a.wc = worldcover;
        a.cg = copernicus;
        a.wc_stride = (unsigned long long)st.wc;
        a.cg_stride = (unsigned long long)st.cg;
        a.mesh_wc = mesh_wc;
        a.mesh_cg = mesh_cg;
        a.mesh_wc_stride_ints = 2ull * (unsigned long long)spec->mesh_wc_tile_stride_nodes;
        a.mesh_cg_stride_ints = 2ull * (unsigned long long)spec->mesh_cg_tile_stride_nodes;
        a.n_tiles = (unsigned long long)n_tiles;
        a.n_rects = nbx * nby;
        a.px = (unsigned long long)height * (unsigned long long)width;
        a.land_stride = spec->land_tile_stride ? (unsigned long long)spec->land_tile_stride : a.px;
        a.wc_h = (int)wc_h;
        a.wc_w = (int)wc_w;
        a.cg_h = (int)cg_h;
        a.cg_w = (int)cg_w;
        a.height = (int)height;
        a.width = (int)width;
        a.shift_wc = spec->shift_wc;
        a.shift_cg = spec->shift_cg;
        a.mesh_wc_w = (int)mesh_dims(3 * width, spec->shift_wc);
        a.mesh_cg_w = (int)mesh_dims(width, spec->shift_cg);
        a.outside_wc = spec->outside_wc;
        a.outside_cg = spec->outside_cg;
        a.nbx = (unsigned)nbx;
        land_resolve(&a.rule, spec->forest_classes, spec->n_forest_classes, spec->thresholds, spec->year_offset);
        a.land = land;
        a.head = reinterpret_cast<unsigned long long*>(head);
        if (head) HIP_TRY(hipMemsetAsync(head, 0, (size_t)n_tiles * DSWX_LAND_MESH_HEAD_WORDS * sizeof(uint64_t), s));
        const unsigned gx = (unsigned)(a.n_rects < LM_MAX_GRID_X ? a.n_rects : LM_MAX_GRID_X);
        const unsigned gy = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
        hipLaunchKernelGGL(dswx_land_mesh_k, dim3(gx, gy), dim3(LM_BLOCK), 0, s, a);
        HIP_TRY(hipGetLastError());
        char info[256];
        snprintf(info, sizeof info, "dswx_land_mesh_k grid=(%u,%u,1) block=%d rect=%dx%d shift_wc=%d shift_cg=%d head=%d", gx, gy,
                 LM_BLOCK, LM_RECT_H, LM_RECT_W, spec->shift_wc, spec->shift_cg, head ? 1 : 0);
        ctx->last_kernel = info;
        return DSWX_OK;
    });
}

}  // extern "C"
