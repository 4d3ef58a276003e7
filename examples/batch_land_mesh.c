/*
 * batch_land_mesh.c -- the LAND plane of a resident batch from land-cover maps that are NOT on the HLS grid, from plain C
 * (DSWX_HAS_LAND_MESH): two synthetic source windows per tile -- a "WorldCover" at 1.47 source pixels per fine pixel and a
 * "CGLS" at 0.31 source pixels per HLS pixel, as the real maps lie under a tile at 45 degrees of latitude -- are written to
 * device memory; two meshes are computed here, in C (a scale and a slight shear), and dswx_land_mesh_device reads both windows
 * through them and writes LAND straight into the batch's plane, with the batch's stride, by ONE kernel launch: no [3H][3W]
 * and no [H][W] intermediate exists.  The plane is downloaded and checked against a loop in C (the definition of
 * include/dswx_hip.h: nine nearest-pixel taps, three counts, the hierarchy) and against dswx_land_mesh_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_land_mesh.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -lm -o batch_land_mesh && ./batch_land_mesh [size]
 *
 * Exit status 0: the device's LAND and head, the loop's and the host entry's agree in every byte; 1: they differ, or a call
 * failed.  tests/test_gpu_land_mesh.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_LAND_MESH
#error "this header has no land mesh entries"
#endif

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

#define SHIFT_WC 5                                    /* a node every 32 fine pixels */
#define SHIFT_CG 4                                    /* a node every 16 HLS pixels */

static int64_t mesh_side(int64_t dst, int shift) { return ((dst + ((int64_t)1 << shift) - 1) >> shift) + 1; }

/* node (i, j) of a lattice at `shift`: `scale` source pixels per pixel, a shear of 3 %, and an offset that leaves a strip of the
 * lattice outside the raster */
static int32_t* make_mesh(int64_t dst_h, int64_t dst_w, int shift, double scale, double offset) {
    const int64_t mh = mesh_side(dst_h, shift), mw = mesh_side(dst_w, shift), step = (int64_t)1 << shift;
    int32_t* mesh = malloc((size_t)(mh * mw) * 2 * sizeof *mesh);
    if (!mesh) return NULL;
    for (int64_t i = 0; i < mh; ++i)
        for (int64_t j = 0; j < mw; ++j) {
            const double X = (double)(j * step) + 0.5, Y = (double)(i * step) + 0.5;
            mesh[2 * (i * mw + j)] = (int32_t)llround(256.0 * (scale * X + 0.03 * scale * Y + offset));
            mesh[2 * (i * mw + j) + 1] = (int32_t)llround(256.0 * (0.69 * scale * Y - 0.02 * scale * X + 1.0));
        }
    return mesh;
}

/* the nearest source pixel of pixel (X, Y): the POSITION of include/dswx_hip.h "warp", floor divisions without shifting a
 * negative number */
static void nearest(const int32_t* mesh, int64_t mw, int shift, int64_t X, int64_t Y, int64_t* c, int64_t* r) {
    const int64_t step = (int64_t)1 << shift, i = Y >> shift, fy = Y & (step - 1), j = X >> shift, fx = X & (step - 1);
    int64_t pos[2];
    for (int k = 0; k < 2; ++k) {
        const int64_t v00 = mesh[2 * (i * mw + j) + k], v01 = mesh[2 * (i * mw + j + 1) + k];
        const int64_t v10 = mesh[2 * ((i + 1) * mw + j) + k], v11 = mesh[2 * ((i + 1) * mw + j + 1) + k];
        const int64_t num = (step - fy) * ((step - fx) * v00 + fx * v01) + fy * ((step - fx) * v10 + fx * v11);
        const int64_t rounded = num + ((int64_t)1 << (2 * shift - 1)), d = (int64_t)1 << (2 * shift + 8);
        pos[k] = rounded >= 0 ? rounded / d : -((-rounded + d - 1) / d);
    }
    *c = pos[0];
    *r = pos[1];
}

int main(int argc, char** argv) {
    const int64_t size = argc > 1 ? atoll(argv[1]) : 150;
    const int64_t n_tiles = 2;
    if (size < 1 || size > 3660) {
        fprintf(stderr, "usage: batch_land_mesh [1 <= size <= 3660]\n");
        return 1;
    }
    if (dswx_abi_version() != DSWX_ABI_VERSION) {
        fprintf(stderr, "header / library ABI mismatch: %d vs %d\n", DSWX_ABI_VERSION, dswx_abi_version());
        return 1;
    }
    dswx_ctx_t* ctx = NULL;
    CHECK(dswx_ctx_create(0, &ctx));               /* DSWX_ERR_NO_DEVICE without an MI355X: there is no CPU fallback */
    dswx_batch_geom_t geom = {n_tiles, size, size, 0};
    dswx_batch_t* batch = NULL;
    CHECK(dswx_batch_create(ctx, &geom, DSWX_BATCH_MASKS, &batch));
    dswx_planes_in_t planes;
    CHECK(dswx_batch_planes(batch, &geom, &planes, NULL, NULL));      /* geom.tile_stride is now the batch's */

    /* the source windows: patches of the classes that matter and of some that do not */
    const int64_t wc_h = (int64_t)(3.0 * (double)size * 1.47 * 0.69) + 8, wc_w = (int64_t)(3.0 * (double)size * 1.47 * 0.97) + 8;
    const int64_t cg_h = (int64_t)((double)size * 0.31 * 0.69) + 4, cg_w = (int64_t)((double)size * 0.31) + 4;
    const size_t wc_px = (size_t)(wc_h * wc_w), cg_px = (size_t)(cg_h * cg_w);
    const uint8_t wc_codes[8] = {10, 10, 50, 80, 90, 95, 30, 0}, cg_codes[4] = {111, 113, 20, 200};
    uint8_t* wc = malloc(wc_px * (size_t)n_tiles);
    uint8_t* cg = malloc(cg_px * (size_t)n_tiles);
    if (!wc || !cg) return 1;
    uint64_t state = 88172645463325252ull;
    for (int64_t t = 0; t < n_tiles; ++t) {
        for (int64_t r = 0; r < wc_h; ++r)
            for (int64_t c = 0; c < wc_w; ++c) {
                state ^= state << 13, state ^= state >> 7, state ^= state << 17;
                const uint64_t patch = (uint64_t)((r / 9) * 131 + (c / 7) * 71 + t * 17);
                wc[(size_t)t * wc_px + (size_t)(r * wc_w + c)] = wc_codes[(state % 5 == 0 ? state >> 8 : patch * 2654435761u >> 7) % 8];
            }
        for (size_t k = 0; k < cg_px; ++k) cg[(size_t)t * cg_px + k] = cg_codes[((k / 3) * 2654435761u >> 9) % 4];
    }
    int32_t* mesh_wc = make_mesh(3 * size, 3 * size, SHIFT_WC, 1.47, -6.0);
    int32_t* mesh_cg = make_mesh(size, size, SHIFT_CG, 0.31, -0.8);
    if (!mesh_wc || !mesh_cg) return 1;
    const int64_t mw_wc = mesh_side(3 * size, SHIFT_WC), mw_cg = mesh_side(size, SHIFT_CG);
    const size_t mesh_wc_bytes = (size_t)(mw_wc * mw_wc) * 8, mesh_cg_bytes = (size_t)(mw_cg * mw_cg) * 8;

    void *wc_dev = NULL, *cg_dev = NULL, *mesh_wc_dev = NULL, *mesh_cg_dev = NULL, *head_dev = NULL;
    CHECK(dswx_device_malloc(ctx, wc_px * (size_t)n_tiles, &wc_dev));
    CHECK(dswx_device_malloc(ctx, cg_px * (size_t)n_tiles, &cg_dev));
    CHECK(dswx_device_malloc(ctx, mesh_wc_bytes, &mesh_wc_dev));
    CHECK(dswx_device_malloc(ctx, mesh_cg_bytes, &mesh_cg_dev));
    CHECK(dswx_device_malloc(ctx, (size_t)n_tiles * DSWX_LAND_MESH_HEAD_WORDS * sizeof(uint64_t), &head_dev));
    CHECK(dswx_memcpy_h2d(ctx, wc_dev, wc, wc_px * (size_t)n_tiles));
    CHECK(dswx_memcpy_h2d(ctx, cg_dev, cg, cg_px * (size_t)n_tiles));
    CHECK(dswx_memcpy_h2d(ctx, mesh_wc_dev, mesh_wc, mesh_wc_bytes));
    CHECK(dswx_memcpy_h2d(ctx, mesh_cg_dev, mesh_cg, mesh_cg_bytes));

    const int32_t forest[2] = {111, 113};
    dswx_land_mesh_spec_t spec;
    memset(&spec, 0, sizeof spec);                  /* one mesh pair for both tiles, packed source planes */
    spec.shift_wc = SHIFT_WC;
    spec.shift_cg = SHIFT_CG;
    spec.outside_wc = 0;                            /* what gdal.Warp initialises a destination to */
    spec.outside_cg = 0;
    spec.thresholds[0] = 6, spec.thresholds[1] = 3, spec.thresholds[2] = 7, spec.thresholds[3] = 3;
    spec.year_offset = 21;
    spec.n_forest_classes = 2;
    spec.forest_classes = forest;
    spec.land_tile_stride = geom.tile_stride;       /* straight into the LAND plane of the batch */
    CHECK(dswx_land_mesh_device(ctx, wc_dev, wc_h, wc_w, cg_dev, cg_h, cg_w, &spec, n_tiles, size, size, mesh_wc_dev, mesh_cg_dev,
                                (uint8_t*)planes.land, head_dev, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));

    const size_t tile_pixels = (size_t)(size * size);
    uint8_t* got = malloc(tile_pixels * (size_t)n_tiles);
    uint8_t* host = malloc(tile_pixels * (size_t)n_tiles);
    uint64_t got_head[2 * DSWX_LAND_MESH_HEAD_WORDS], host_head[2 * DSWX_LAND_MESH_HEAD_WORDS];
    if (!got || !host) return 1;
    for (int64_t t = 0; t < n_tiles; ++t)
        CHECK(dswx_memcpy_d2h(ctx, got + (size_t)t * tile_pixels, (const uint8_t*)planes.land + t * geom.tile_stride, tile_pixels));
    CHECK(dswx_memcpy_d2h(ctx, got_head, head_dev, sizeof got_head));
    spec.land_tile_stride = 0;                      /* the host entry writes packed tiles */
    CHECK(dswx_land_mesh_host(wc, wc_h, wc_w, cg, cg_h, cg_w, &spec, n_tiles, size, size, mesh_wc, mesh_cg, host, host_head));

    /* the loop: the definition, pixel by pixel */
    int differ = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        uint64_t wc_in = 0, cg_in = 0, all_out = 0, fill = 0;
        for (int64_t Y = 0; Y < size; ++Y)
            for (int64_t X = 0; X < size; ++X) {
                int water = 0, urban = 0, tree = 0, inside = 0;
                for (int k = 0; k < 9; ++k) {
                    int64_t c, r;
                    nearest(mesh_wc, mw_wc, SHIFT_WC, 3 * X + k % 3, 3 * Y + k / 3, &c, &r);
                    const int in = c >= 0 && c < wc_w && r >= 0 && r < wc_h;
                    const int v = in ? wc[(size_t)t * wc_px + (size_t)(r * wc_w + c)] : 0;
                    inside += in;
                    water += v == 80 || v == 90 || v == 95;
                    urban += v == 50;
                    tree += v == 10;
                }
                int64_t c, r;
                nearest(mesh_cg, mw_cg, SHIFT_CG, X, Y, &c, &r);
                const int in = c >= 0 && c < cg_w && r >= 0 && r < cg_h;
                const int cls = in ? cg[(size_t)t * cg_px + (size_t)(r * cg_w + c)] : 0;
                if (cls != 111 && cls != 113) tree = 0;
                uint8_t want = 255;
                if (tree >= 6) want = 201;
                if (urban >= 3) want = 21;
                if (urban >= 7) want = 121;
                if (water >= 3) want = 200;
                const size_t e = (size_t)t * tile_pixels + (size_t)(Y * size + X);
                if ((got[e] != want || host[e] != want) && differ < 10)
                    fprintf(stderr, "tile %" PRId64 " pixel (%" PRId64 ", %" PRId64 "): loop %u, device %u, dswx_land_mesh_host %u\n", t, X, Y, want, got[e], host[e]);
                differ += got[e] != want || host[e] != want;
                wc_in += (uint64_t)inside, cg_in += (uint64_t)in, all_out += inside == 0, fill += want == 255;
            }
        const uint64_t* g = got_head + t * DSWX_LAND_MESH_HEAD_WORDS;
        const uint64_t want_head[DSWX_LAND_MESH_HEAD_WORDS] = {tile_pixels, wc_in, 9 * tile_pixels - wc_in, cg_in, tile_pixels - cg_in, all_out, fill, 0};
        if (memcmp(g, want_head, sizeof want_head) != 0 || memcmp(g, host_head + t * DSWX_LAND_MESH_HEAD_WORDS, sizeof want_head) != 0) {
            fprintf(stderr, "tile %" PRId64 ": head %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " differs from the loop's or the host entry's\n", t, g[0], g[1], g[2], g[3]);
            differ += 1;
        }
        printf("tile %" PRId64 ": %" PRIu64 " of %zu WorldCover taps inside, %" PRIu64 " of %zu CGLS taps, %" PRIu64 " LAND pixels are fill\n", t, g[1],
               9 * tile_pixels, g[3], tile_pixels, g[6]);
    }
    printf("%s\n", differ ? "MISMATCH" : "land mesh: device, loop and host entry agree in every byte");
    free(host);
    free(got);
    free(mesh_cg);
    free(mesh_wc);
    free(cg);
    free(wc);
    CHECK(dswx_device_free(ctx, head_dev));
    CHECK(dswx_device_free(ctx, mesh_cg_dev));
    CHECK(dswx_device_free(ctx, mesh_wc_dev));
    CHECK(dswx_device_free(ctx, cg_dev));
    CHECK(dswx_device_free(ctx, wc_dev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
