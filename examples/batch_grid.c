/*
 * batch_grid.c -- a layer of a resident batch aggregated onto a coarse grid, from plain C (DSWX_HAS_GRID): a small batch is
 * allocated, generated and classified in HBM, and dswx_batch_grid turns its WTR layer into cells of 30 x 30 pixels with one
 * kernel launch -- per cell how many pixels were water, how many clear and not water, the water fraction of the clear pixels,
 * the fraction of the cell that was observed, and the majority class.  The planes stay in device memory; here they are
 * downloaded, with the WTR layer, and checked against a loop in C and against dswx_grid_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_grid.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_grid && ./batch_grid [n_tiles] [size]
 *
 * Exit status 0: the device's planes, the loop's and the host entry's agree in every cell; 1: they differ, or a call failed.
 * tests/test_gpu_grid.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_GRID
#error "this header has no grid entries"
#endif

#define CELL 30

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

/* the five planes of one cell count, side by side in one allocation: two uint32 counts, then share, coverage and major */
typedef struct planes {
    uint32_t *water, *land;
    uint8_t *share, *coverage, *major;
} planes_t;

static planes_t carve(uint8_t* base, size_t cells) {
    planes_t p;
    p.water = (uint32_t*)base;
    p.land = p.water + cells;
    p.share = (uint8_t*)(p.land + cells);
    p.coverage = p.share + cells;
    p.major = p.coverage + cells;
    return p;
}

static dswx_grid_out_t outputs_of(planes_t p) {
    dswx_grid_out_t o;
    memset(&o, 0, sizeof o);
    o.count[0] = p.water;
    o.count[1] = p.land;
    o.share = p.share;
    o.coverage = p.coverage;
    o.major = p.major;
    return o;
}

int main(int argc, char** argv) {
    const int64_t n_tiles = argc > 1 ? atoll(argv[1]) : 5;
    const int64_t size = argc > 2 ? atoll(argv[2]) : 301;
    if (dswx_abi_version() != DSWX_ABI_VERSION) {
        fprintf(stderr, "header / library ABI mismatch: %d vs %d\n", DSWX_ABI_VERSION, dswx_abi_version());
        return 1;
    }
    dswx_ctx_t* ctx = NULL;
    CHECK(dswx_ctx_create(0, &ctx));               /* DSWX_ERR_NO_DEVICE without an MI355X: there is no CPU fallback */
    dswx_params_t params;
    CHECK(dswx_params_default(&params));

    dswx_batch_geom_t geom = {n_tiles, size, size, 0};
    dswx_batch_t* batch = NULL;
    CHECK(dswx_batch_create(ctx, &geom, 0, &batch));
    CHECK(dswx_batch_synth(batch, 20251010u, 0, NULL));
    CHECK(dswx_batch_classify(batch, &params, DSWX_BATCH_ALL_TILES, NULL));

    /* the saved WTR classes: 1 open water and 2 partial surface water are category 0 ("water"), 0 not water is category 1;
     * snow 252, cloud 253, ocean masked 254 and fill 255 -- every other byte -- are not observations */
    dswx_grid_spec_t spec;
    memset(&spec, 0, sizeof spec);
    spec.n_cats = 2;
    spec.cell_h = spec.cell_w = CELL;
    memset(spec.cat_of_byte, 255, sizeof spec.cat_of_byte);
    spec.cat_of_byte[1] = spec.cat_of_byte[2] = 0;
    spec.cat_of_byte[0] = 1;

    const int64_t cell = size < CELL ? size : CELL;                  /* a cell is never larger than the raster */
    const int64_t g = size > 0 ? (size + cell - 1) / cell : 0;       /* cells down = cells across */
    const size_t pixels = (size_t)size * (size_t)size;
    const size_t cells = (size_t)n_tiles * (size_t)g * (size_t)g;
    const size_t bytes = cells > 0 ? cells * 11 : 16;                /* 2 uint32 planes + 3 byte planes */
    void* dev = NULL;
    CHECK(dswx_device_malloc(ctx, bytes, &dev));
    const dswx_grid_out_t dev_out = outputs_of(carve(dev, cells));
    /* same stream as the classification (NULL = the context's): ordered behind it; asynchronous, so the copy below, which is
     * complete on return, is what waits for it */
    CHECK(dswx_batch_grid(batch, DSWX_PLANE_WTR, &spec, 0, DSWX_BATCH_ALL_TILES, &dev_out, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));
    uint8_t* got_mem = malloc(bytes);
    uint8_t* host_mem = malloc(bytes);
    uint8_t* wtr = malloc(pixels > 0 && n_tiles > 0 ? pixels * (size_t)n_tiles : 1);
    if (!got_mem || !host_mem || !wtr) return 1;
    CHECK(dswx_memcpy_d2h(ctx, got_mem, dev, bytes));
    const planes_t got = carve(got_mem, cells);

    /* the other half: the WTR layer on the host, tile after tile without the padding */
    dswx_planes_out_t layers;
    CHECK(dswx_batch_planes(batch, &geom, NULL, &layers, NULL));
    for (int64_t t = 0; t < n_tiles; ++t)
        if (pixels) CHECK(dswx_memcpy_d2h(ctx, wtr + (size_t)t * pixels, layers.wtr + t * geom.tile_stride, pixels));
    const planes_t host = carve(host_mem, cells);
    const dswx_grid_out_t host_out = outputs_of(host);
    CHECK(dswx_grid_host(wtr, &spec, n_tiles, size, size, 0, &host_out));

    int differ = 0;
    uint64_t mostly_water = 0, never_seen = 0;
    for (int64_t t = 0; t < n_tiles; ++t)
        for (int64_t gy = 0; gy < g; ++gy)
            for (int64_t gx = 0; gx < g; ++gx) {
                const int64_t r1 = (gy + 1) * cell < size ? (gy + 1) * cell : size;
                const int64_t c1 = (gx + 1) * cell < size ? (gx + 1) * cell : size;
                unsigned water = 0, land = 0;
                for (int64_t r = gy * cell; r < r1; ++r)
                    for (int64_t c = gx * cell; c < c1; ++c) {
                        const unsigned v = wtr[(size_t)t * pixels + (size_t)(r * size + c)];
                        if (v == 1 || v == 2) ++water;
                        else if (v == 0) ++land;
                    }
                const unsigned n_pix = (unsigned)((r1 - gy * cell) * (c1 - gx * cell));
                const unsigned share = water + land ? 100 * water / (water + land) : DSWX_GRID_NO_SHARE;
                const unsigned coverage = 100 * (water + land) / n_pix;
                const unsigned major = water + land == 0 ? DSWX_GRID_NONE : water >= land ? 0u : 1u;
                mostly_water += major == 0;
                never_seen += water + land == 0;
                const size_t i = (size_t)((t * g + gy) * g + gx);
                const int dev_ok = got.water[i] == water && got.land[i] == land && got.share[i] == share &&
                                   got.coverage[i] == coverage && got.major[i] == major;
                const int host_ok = host.water[i] == water && host.land[i] == land && host.share[i] == share &&
                                    host.coverage[i] == coverage && host.major[i] == major;
                if ((!dev_ok || !host_ok) && differ < 10) {
                    fprintf(stderr, "cell %zu: loop %u %u %u %u %u, device %u %u %u %u %u, dswx_grid_host %u %u %u %u %u\n", i, water,
                            land, share, coverage, major, got.water[i], got.land[i], got.share[i], got.coverage[i], got.major[i],
                            host.water[i], host.land[i], host.share[i], host.coverage[i], host.major[i]);
                }
                differ += !dev_ok || !host_ok;
            }
    printf("%" PRId64 " tiles of %" PRId64 " x %" PRId64 " pixels, %" PRId64 " x %" PRId64 " cells of %d x %d: %" PRIu64
           " cells mostly water, %" PRIu64 " never observed\n", n_tiles, size, size, g, g, CELL, CELL, mostly_water, never_seen);
    printf("%s\n", differ ? "MISMATCH" : "wtr grid: device, loop and host entry agree in every cell");
    free(wtr);
    free(host_mem);
    free(got_mem);
    CHECK(dswx_device_free(ctx, dev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
