/*
 * batch_resample.c -- a float32 plane INTERPOLATED onto another lattice through a coordinate mesh, from plain C
 * (DSWX_HAS_RESAMPLE): two tiles of a synthetic elevation surface with a few nodata pixels are written to device memory; a mesh
 * is computed here, in C, for a rotation of two degrees about the middle of the tile and 1.3 source pixels per destination
 * pixel -- what a DEM in another projection looks like from the product's grid -- and dswx_resample_device interpolates every
 * destination pixel (cubic, with the bilinear rule where the 4 x 4 window has an invalid tap) with one kernel launch.  The
 * outputs are downloaded and checked, bit for bit, against a loop in C (the definition of include/dswx_hip.h "resample", pixel
 * by pixel, in doubles) and against dswx_resample_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_resample.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -lm -o batch_resample && ./batch_resample [size] [dst]
 *
 * (-std=c11 keeps the compiler from fusing a product and a sum: the definition rounds each on its own.)
 * Exit status 0: the device's outputs, the loop's and the host entry's agree in every bit; 1: they differ, or a call failed.
 * tests/test_gpu_resample.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_RESAMPLE
#error "this header has no resample entries"
#endif

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

#define MESH_SHIFT 5                                  /* a node every 32 destination pixels */
#define NODATA (-9999.0f)
#define OUTSIDE (-32767.0f)

/* floor(a / 2^k) without shifting a negative number */
static int64_t floor_shift(int64_t a, int k) {
    const int64_t d = (int64_t)1 << k;
    return a >= 0 ? a / d : -((-a + d - 1) / d);
}

static void weights(int64_t f, double* n) {
    n[0] = (double)(-65536 * f + 512 * f * f - f * f * f);
    n[1] = (double)(((int64_t)1 << 25) - 1280 * f * f + 3 * f * f * f);
    n[2] = (double)(65536 * f + 1024 * f * f - 3 * f * f * f);
    n[3] = (double)(-256 * f * f + f * f * f);
}

/* 1 and *v if source pixel (c, r) of the tile is a valid tap */
static int tap(const float* tile, int64_t size, int64_t c, int64_t r, double* v) {
    if (c < 0 || c >= size || r < 0 || r >= size) return 0;
    const float p = tile[r * size + c];
    if (!isfinite(p) || p == NODATA) return 0;
    *v = (double)p;
    return 1;
}

int main(int argc, char** argv) {
    const int64_t size = argc > 1 ? atoll(argv[1]) : 211;
    const int64_t dst = argc > 2 ? atoll(argv[2]) : 190;
    const int64_t n_tiles = 2;
    if (size < 1 || size > 20000 || dst < 1 || dst > 20000) {
        fprintf(stderr, "usage: batch_resample [1 <= size <= 20000] [1 <= dst <= 20000]\n");
        return 1;
    }
    if (dswx_abi_version() != DSWX_ABI_VERSION) {
        fprintf(stderr, "header / library ABI mismatch: %d vs %d\n", DSWX_ABI_VERSION, dswx_abi_version());
        return 1;
    }
    dswx_ctx_t* ctx = NULL;
    CHECK(dswx_ctx_create(0, &ctx));               /* DSWX_ERR_NO_DEVICE without an MI355X: there is no CPU fallback */

    /* the plane: a smooth surface, another one per tile, with nodata pixels and one that is not finite */
    const size_t tile_pixels = (size_t)size * (size_t)size, src_bytes = tile_pixels * (size_t)n_tiles * sizeof(float);
    float* plane = malloc(src_bytes);
    if (!plane) return 1;
    for (int64_t t = 0; t < n_tiles; ++t)
        for (int64_t r = 0; r < size; ++r)
            for (int64_t c = 0; c < size; ++c) {
                float v = (float)(300.0 + 100.0 * (double)t + 80.0 * sin((double)c / 11.0) * cos((double)r / 7.0) + 0.37 * (double)c - 0.21 * (double)r);
                if ((c * 31 + r * 17 + t) % 97 == 0) v = NODATA;
                if (c == size / 2 && r == size / 3) v = INFINITY;
                plane[(size_t)t * tile_pixels + (size_t)(r * size + c)] = v;
            }
    void* plane_dev = NULL;
    CHECK(dswx_device_malloc(ctx, src_bytes, &plane_dev));
    CHECK(dswx_memcpy_h2d(ctx, plane_dev, plane, src_bytes));

    /* the mesh: node (i, j) is where the centre of destination pixel (X, Y) = (32 j, 32 i) lies in the source, in 1/256 pixel
     * (source pixel (c, r) has its centre at (256 c + 128, 256 r + 128)); one mesh for both tiles */
    const int64_t step = (int64_t)1 << MESH_SHIFT;
    const int64_t mesh_h = ((dst + step - 1) >> MESH_SHIFT) + 1, mesh_w = mesh_h;
    const size_t mesh_bytes = (size_t)(mesh_h * mesh_w) * 2 * sizeof(int32_t);
    int32_t* mesh = malloc(mesh_bytes);
    if (!mesh) return 1;
    const double angle = 2.0 * 3.14159265358979323846 / 180.0, scale = 1.3, mid_s = 128.0 * (double)size, mid_d = 128.0 * (double)dst;
    for (int64_t i = 0; i < mesh_h; ++i)
        for (int64_t j = 0; j < mesh_w; ++j) {
            const double x = scale * (256.0 * (double)(j * step) + 128.0 - mid_d), y = scale * (256.0 * (double)(i * step) + 128.0 - mid_d);
            mesh[2 * (i * mesh_w + j)] = (int32_t)llround(mid_s + cos(angle) * x - sin(angle) * y);
            mesh[2 * (i * mesh_w + j) + 1] = (int32_t)llround(mid_s + sin(angle) * x + cos(angle) * y);
        }
    void* mesh_dev = NULL;
    CHECK(dswx_device_malloc(ctx, mesh_bytes, &mesh_dev));
    CHECK(dswx_memcpy_h2d(ctx, mesh_dev, mesh, mesh_bytes));

    const float nodata = NODATA, outside = OUTSIDE;
    dswx_resample_spec_t spec;
    memset(&spec, 0, sizeof spec);
    spec.kind = DSWX_RESAMPLE_F32;
    spec.method = DSWX_RESAMPLE_CUBIC;
    spec.shift = MESH_SHIFT;
    spec.has_nodata = 1;
    memcpy(&spec.nodata, &nodata, 4);               /* the bits of the float32 */
    memcpy(&spec.outside, &outside, 4);

    const size_t dst_pixels = (size_t)dst * (size_t)dst, pixels = dst_pixels * (size_t)n_tiles;
    const size_t head_bytes = (size_t)n_tiles * DSWX_RESAMPLE_HEAD_WORDS * sizeof(uint64_t);
    void *dst_dev = NULL, *how_dev = NULL, *head_dev = NULL;
    CHECK(dswx_device_malloc(ctx, pixels * sizeof(float), &dst_dev));
    CHECK(dswx_device_malloc(ctx, pixels, &how_dev));
    CHECK(dswx_device_malloc(ctx, head_bytes, &head_dev));
    const dswx_resample_out_t dev_out = {dst_dev, how_dev, head_dev};
    CHECK(dswx_resample_device(ctx, plane_dev, &spec, n_tiles, size, size, mesh_dev, dst, dst, &dev_out, NULL));   /* asynchronous */
    CHECK(dswx_stream_synchronize(ctx, NULL));

    float* got = malloc(pixels * sizeof *got);
    float* host = malloc(pixels * sizeof *host);
    uint8_t* got_how = malloc(pixels);
    uint8_t* host_how = malloc(pixels);
    uint64_t got_head[2 * DSWX_RESAMPLE_HEAD_WORDS], host_head[2 * DSWX_RESAMPLE_HEAD_WORDS];
    if (!got || !host || !got_how || !host_how) return 1;
    CHECK(dswx_memcpy_d2h(ctx, got, dst_dev, pixels * sizeof *got));
    CHECK(dswx_memcpy_d2h(ctx, got_how, how_dev, pixels));
    CHECK(dswx_memcpy_d2h(ctx, got_head, head_dev, head_bytes));
    const dswx_resample_out_t host_out = {host, host_how, host_head};
    CHECK(dswx_resample_host(plane, &spec, n_tiles, size, size, mesh, dst, dst, &host_out));

    /* the loop: the definition, pixel by pixel */
    int differ = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const float* tile = plane + (size_t)t * tile_pixels;
        uint64_t count[4] = {0, 0, 0, 0};
        for (int64_t Y = 0; Y < dst; ++Y)
            for (int64_t X = 0; X < dst; ++X) {
                const int64_t i = Y >> MESH_SHIFT, fy = Y & (step - 1), j = X >> MESH_SHIFT, fx = X & (step - 1);
                int64_t base[2], frac[2];
                for (int k = 0; k < 2; ++k) {
                    const int64_t v00 = mesh[2 * (i * mesh_w + j) + k], v01 = mesh[2 * (i * mesh_w + j + 1) + k];
                    const int64_t v10 = mesh[2 * ((i + 1) * mesh_w + j) + k], v11 = mesh[2 * ((i + 1) * mesh_w + j + 1) + k];
                    const int64_t num = (step - fy) * ((step - fx) * v00 + fx * v01) + fy * ((step - fx) * v10 + fx * v11);
                    const int64_t u = floor_shift(num + ((int64_t)1 << (2 * MESH_SHIFT - 1)), 2 * MESH_SHIFT) - 128;
                    base[k] = floor_shift(u, 8);
                    frac[k] = u - 256 * base[k];
                }
                const int64_t c0 = base[0], r0 = base[1], gx = frac[0], gy = frac[1];
                double p[4][4] = {{0.0}}, result = 0.0;
                int all = 1, how = 0;
                for (int r = 0; r < 4; ++r)
                    for (int c = 0; c < 4; ++c) all &= tap(tile, size, c0 - 1 + c, r0 - 1 + r, &p[r][c]);
                if (all) {
                    double nx[4], ny[4], h[4];
                    weights(gx, nx);
                    weights(gy, ny);
                    for (int r = 0; r < 4; ++r) h[r] = ((nx[0] * p[r][0] + nx[1] * p[r][1]) + nx[2] * p[r][2]) + nx[3] * p[r][3];
                    result = (((ny[0] * h[0] + ny[1] * h[1]) + ny[2] * h[2]) + ny[3] * h[3]) * 0x1p-50;
                    how = 3;
                } else {
                    const int64_t w[4] = {(256 - gx) * (256 - gy), gx * (256 - gy), (256 - gx) * gy, gx * gy};
                    double s = 0.0, v;
                    int64_t wt = 0;
                    int n = 0;
                    for (int k = 0; k < 4; ++k)
                        if (tap(tile, size, c0 + (k & 1), r0 + (k >> 1), &v)) {
                            s = s + (double)w[k] * v;
                            wt += w[k];
                            ++n;
                        }
                    if (wt) {
                        result = wt == 65536 ? s * 0x1p-16 : s / (double)wt;
                        how = n == 4 ? 1 : 2;
                    }
                }
                const float want = how ? (float)result : OUTSIDE;
                const size_t e = (size_t)t * dst_pixels + (size_t)(Y * dst + X);
                ++count[how];
                const int ok = memcmp(&got[e], &want, 4) == 0 && memcmp(&host[e], &want, 4) == 0 && got_how[e] == how && host_how[e] == how;
                if (!ok && differ < 10)
                    fprintf(stderr, "tile %" PRId64 " pixel (%" PRId64 ", %" PRId64 "): loop %.9g how %d, device %.9g how %u, dswx_resample_host %.9g how %u\n",
                            t, X, Y, (double)want, how, (double)got[e], got_how[e], (double)host[e], host_how[e]);
                differ += !ok;
            }
        const uint64_t* g = got_head + t * DSWX_RESAMPLE_HEAD_WORDS;
        if (g[0] != dst_pixels || g[1] != count[3] || g[2] != count[1] || g[3] != count[2] || g[4] != count[0] || g[7] != 0 ||
            memcmp(g, host_head + t * DSWX_RESAMPLE_HEAD_WORDS, DSWX_RESAMPLE_HEAD_WORDS * sizeof(uint64_t)) != 0) {
            fprintf(stderr, "tile %" PRId64 ": head %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " differs from the loop or the host entry\n", t,
                    g[0], g[1], g[2], g[3], g[4]);
            differ += 1;
        }
        printf("tile %" PRId64 ": %" PRIu64 " cubic, %" PRIu64 " bilinear, %" PRIu64 " renormalised, %" PRIu64 " outside of %zu pixels, source rows %" PRIu64
               " .. %" PRIu64 "\n", t, g[1], g[2], g[3], g[4], dst_pixels, g[5], g[6]);
    }
    printf("%s\n", differ ? "MISMATCH" : "float32 resample: device, loop and host entry agree in every bit");
    free(host_how);
    free(got_how);
    free(host);
    free(got);
    free(mesh);
    free(plane);
    CHECK(dswx_device_free(ctx, head_dev));
    CHECK(dswx_device_free(ctx, how_dev));
    CHECK(dswx_device_free(ctx, dst_dev));
    CHECK(dswx_device_free(ctx, mesh_dev));
    CHECK(dswx_device_free(ctx, plane_dev));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
