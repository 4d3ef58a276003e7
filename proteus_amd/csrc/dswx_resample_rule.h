// dswx_resample_rule.h -- what the device kernel and the host statement of the resample (dswx_resample.hip; include/dswx_hip.h
// "resample") share from the position of a destination pixel on (the position itself is dswx_mesh_rule.h): the integer cubic
// weights, which tap is valid, the per-pixel rule in IEEE doubles and the rounding to the output element.  Every product and
// every sum of the rule is ONE double operation rounded on its own: the build passes -ffp-contract=off (proteus_amd/build.py)
// and nothing here may be fused, or device and host stop agreeing bit for bit.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#define RESAMPLE_HD __host__ __device__ __forceinline__

namespace {

// The destination rectangle of one workgroup, one pixel per thread, and the elements of the source window that it stages in
// LDS: a rectangle whose source box (halo included) has more elements gathers from global memory instead.  The tests build
// their shapes around these.
#define DSWX_RESAMPLE_RECT_H 8
#define DSWX_RESAMPLE_RECT_W 32
#define DSWX_RESAMPLE_LDS_ELEMS 4096

enum { RESAMPLE_OUTSIDE = 0, RESAMPLE_BILINEAR_FULL = 1, RESAMPLE_BILINEAR_RENORM = 2, RESAMPLE_CUBIC_FULL = 3 };

// Keys' cubic, a = -0.5 (Catmull-Rom), at f / 256: integers over 2^25 that sum to 2^25, each of magnitude <= 2^25.
RESAMPLE_HD void resample_weights(int f, double* n) {
    const int64_t g = f, g2 = g * g, g3 = g2 * g;
    n[0] = (double)(-65536 * g + 512 * g2 - g3);
    n[1] = (double)(((int64_t)1 << 25) - 1280 * g2 + 3 * g3);
    n[2] = (double)(65536 * g + 1024 * g2 - 3 * g3);
    n[3] = (double)(-256 * g2 + g3);
}

// A tap as the rule sees it.
struct ResampleTap {
    bool valid;
    double v;
};

// The element of a source pixel that lies in the raster, staged as 32 bits (float32: its bits; int16: sign extended): valid
// iff finite and not the nodata value.  The ONE statement of validity by value, for taps from LDS and from global memory.
#define RESAMPLE_INVALID_F32 0x7fc00000u
#define RESAMPLE_INVALID_I16 0x80000000u
template <bool F32> RESAMPLE_HD uint32_t resample_stage(uint32_t raw, int has_nodata, uint32_t nodata) {
    if (F32) {
        if ((raw & 0x7f800000u) == 0x7f800000u) return RESAMPLE_INVALID_F32;          // NaN, +-Inf
        if (has_nodata) {
            float a, b;
            memcpy(&a, &raw, 4);
            memcpy(&b, &nodata, 4);
            if (a == b) return RESAMPLE_INVALID_F32;                                    // compared as a value: -0 == +0
        }
        return raw;
    }
    const int32_t v = (int32_t)(int16_t)(uint16_t)raw;
    if (has_nodata && v == (int32_t)nodata) return RESAMPLE_INVALID_I16;
    return (uint32_t)v;
}
template <bool F32> RESAMPLE_HD ResampleTap resample_tap_of(uint32_t staged) {
    ResampleTap t;
    if (F32) {
        float a;
        memcpy(&a, &staged, 4);
        t.valid = (staged & 0x7f800000u) != 0x7f800000u;
        t.v = t.valid ? (double)a : 0.0;
    } else {
        t.valid = staged != RESAMPLE_INVALID_I16;
        t.v = t.valid ? (double)(int32_t)staged : 0.0;
    }
    return t;
}
RESAMPLE_HD ResampleTap resample_no_tap() {
    ResampleTap t;
    t.valid = false;
    t.v = 0.0;
    return t;
}

struct ResamplePixel {
    int how;              // RESAMPLE_*
    double v;             // the result, if how != RESAMPLE_OUTSIDE
    int64_t rlo, rhi;     // the smallest and the largest source row among the valid taps of the window used, if how != 0
};

// The rule for the pixel at (sx, sy).  tap(c, r) is the tap of source pixel (c, r), which may lie anywhere: a tap outside the
// raster is not valid, and the comparison with the raster comes BEFORE any load.
template <class Tap> RESAMPLE_HD ResamplePixel resample_pixel(bool cubic, int64_t sx, int64_t sy, Tap tap) {
    const int64_t ux = sx - 128, uy = sy - 128;
    const int64_t c0 = ux >> 8, r0 = uy >> 8;
    const int fx = (int)(ux & 255), fy = (int)(uy & 255);
    ResamplePixel px;
    if (cubic) {
        ResampleTap p[4][4];
        bool all = true;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                p[r][c] = tap(c0 - 1 + c, r0 - 1 + r);
                all = all && p[r][c].valid;
            }
        if (all) {
            double nx[4], ny[4], h[4];
            resample_weights(fx, nx);
            resample_weights(fy, ny);
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = ((nx[0] * p[r][0].v + nx[1] * p[r][1].v) + nx[2] * p[r][2].v) + nx[3] * p[r][3].v;
            px.v = (((ny[0] * h[0] + ny[1] * h[1]) + ny[2] * h[2]) + ny[3] * h[3]) * 0x1p-50;
            px.how = RESAMPLE_CUBIC_FULL;
            px.rlo = r0 - 1;
            px.rhi = r0 + 2;
            return px;
        }
        // the bilinear taps are four of the sixteen
        const ResampleTap q[4] = {p[1][1], p[1][2], p[2][1], p[2][2]};
        const int w[4] = {(256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy};
        double S = 0.0;
        int Wt = 0, n = 0;
        px.rlo = r0 + 1, px.rhi = r0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (q[k].valid) {
                S = S + (double)w[k] * q[k].v;
                Wt += w[k];
                ++n;
                const int64_t r = r0 + (k >> 1);
                px.rlo = r < px.rlo ? r : px.rlo;
                px.rhi = r > px.rhi ? r : px.rhi;
            }
        px.how = Wt == 0 ? RESAMPLE_OUTSIDE : (n == 4 ? RESAMPLE_BILINEAR_FULL : RESAMPLE_BILINEAR_RENORM);
        px.v = Wt == 65536 ? S * 0x1p-16 : (Wt ? S / (double)Wt : 0.0);
        return px;
    }
    const int w[4] = {(256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy};
    double S = 0.0;
    int Wt = 0, n = 0;
    px.rlo = r0 + 1, px.rhi = r0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const ResampleTap q = tap(c0 + (k & 1), r0 + (k >> 1));
        if (q.valid) {
            S = S + (double)w[k] * q.v;
            Wt += w[k];
            ++n;
            const int64_t r = r0 + (k >> 1);
            px.rlo = r < px.rlo ? r : px.rlo;
            px.rhi = r > px.rhi ? r : px.rhi;
        }
    }
    px.how = Wt == 0 ? RESAMPLE_OUTSIDE : (n == 4 ? RESAMPLE_BILINEAR_FULL : RESAMPLE_BILINEAR_RENORM);
    px.v = Wt == 65536 ? S * 0x1p-16 : (Wt ? S / (double)Wt : 0.0);
    return px;
}

// The output element as 32 bits (its low bytes are the element).  float32: round to nearest even, subnormals kept, a value
// past FLT_MAX becomes an infinity.  int16: rint (half to even), then clamped.
template <bool F32> RESAMPLE_HD uint32_t resample_element(double v) {
    if (F32) {
        const float f = (float)v;
        uint32_t b;
        memcpy(&b, &f, 4);
        return b;
    }
    double r = rint(v);
    r = r < -32768.0 ? -32768.0 : (r > 32767.0 ? 32767.0 : r);
    return (uint32_t)(uint16_t)(int16_t)(int32_t)r;
}

}  // namespace
