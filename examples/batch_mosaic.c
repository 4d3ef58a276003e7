/*
 * batch_mosaic.c -- a 2 x 2 block of neighbouring tiles of a resident batch mosaicked onto one canvas, from plain C
 * (DSWX_HAS_MOSAIC): a batch of four tiles is allocated, generated and classified in HBM; the tiles are taken as the four
 * neighbours of a 2 x 2 block that overlap by `overlap` pixels, a placement table is written to device memory, and
 * dswx_batch_mosaic turns the WTR layer into five canvas planes with one kernel launch.  The planes stay in device memory;
 * here they are downloaded, with the WTR layer, and checked against a paste loop in C and against dswx_mosaic_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_mosaic.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_mosaic && ./batch_mosaic [size] [overlap]
 *
 * Exit status 0: the device's planes, the loop's and the host entry's agree in every pixel; 1: they differ, or a call failed.
 * tests/test_gpu_mosaic.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_MOSAIC
#error "this header has no mosaic entries"
#endif

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

/* the five planes of one pixel count, side by side in one allocation: two uint16 counts, last_index, then last and share */
typedef struct planes {
    uint16_t *water, *land, *last_index;
    uint8_t *last, *share;
} planes_t;

static planes_t carve(uint8_t* base, size_t pixels) {
    planes_t p;
    p.water = (uint16_t*)base;
    p.land = p.water + pixels;
    p.last_index = p.land + pixels;
    p.last = (uint8_t*)(p.last_index + pixels);
    p.share = p.last + pixels;
    return p;
}

static dswx_stack_out_t outputs_of(planes_t p) {
    dswx_stack_out_t o;
    memset(&o, 0, sizeof o);
    o.count[0] = p.water;
    o.count[1] = p.land;
    o.last = p.last;
    o.last_index = p.last_index;
    o.share = p.share;
    return o;
}

int main(int argc, char** argv) {
    const int64_t size = argc > 1 ? atoll(argv[1]) : 301;
    const int64_t overlap = argc > 2 ? atoll(argv[2]) : 27;
    const int64_t n_tiles = 4;
    if (size < 1 || overlap < 0 || overlap > size) {
        fprintf(stderr, "usage: batch_mosaic [size >= 1] [0 <= overlap <= size]\n");
        return 1;
    }
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

    /* the saved WTR classes as in batch_stack.c; a canvas pixel outside every footprint gets 254 in `last` (there is none
     * in a full 2 x 2 block: the loop below checks that too) */
    dswx_mosaic_spec_t spec;
    memset(&spec, 0, sizeof spec);
    spec.n_cats = 2;
    spec.fill = 255;
    spec.outside = 254;
    memset(spec.cat_of_byte, 255, sizeof spec.cat_of_byte);
    spec.cat_of_byte[1] = spec.cat_of_byte[2] = 0;
    spec.cat_of_byte[0] = 1;

    /* tile 0 top left, 1 top right, 2 bottom left, 3 bottom right: origins size - overlap pixels apart */
    const int64_t step = size - overlap, canvas = size + step;
    const int32_t place[4][2] = {{0, 0}, {0, (int32_t)step}, {(int32_t)step, 0}, {(int32_t)step, (int32_t)step}};
    void* place_dev = NULL;
    CHECK(dswx_device_malloc(ctx, sizeof place, &place_dev));
    CHECK(dswx_memcpy_h2d(ctx, place_dev, place, sizeof place));

    const size_t tile_pixels = (size_t)size * (size_t)size;
    const size_t pixels = (size_t)canvas * (size_t)canvas;
    const size_t bytes = pixels * 8;                         /* 3 uint16 planes + 2 byte planes */
    void* dev = NULL;
    CHECK(dswx_device_malloc(ctx, bytes, &dev));
    const dswx_stack_out_t dev_out = outputs_of(carve(dev, pixels));
    /* same stream as the classification (NULL = the context's): ordered behind it; asynchronous */
    CHECK(dswx_batch_mosaic(batch, DSWX_PLANE_WTR, &spec, 0, DSWX_BATCH_ALL_TILES, place_dev, canvas, canvas, &dev_out, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));
    uint8_t* got_mem = malloc(bytes);
    uint8_t* host_mem = malloc(bytes);
    uint8_t* wtr = malloc(tile_pixels * (size_t)n_tiles);
    /* the paste loop's canvases */
    uint16_t* water = calloc(pixels, sizeof *water);
    uint16_t* land = calloc(pixels, sizeof *land);
    uint16_t* last_index = malloc(pixels * sizeof *last_index);
    uint8_t* last = malloc(pixels);
    if (!got_mem || !host_mem || !wtr || !water || !land || !last_index || !last) return 1;
    CHECK(dswx_memcpy_d2h(ctx, got_mem, dev, bytes));
    const planes_t got = carve(got_mem, pixels);

    /* the other half: the WTR layer on the host, tile after tile without the padding */
    dswx_planes_out_t layers;
    CHECK(dswx_batch_planes(batch, &geom, NULL, &layers, NULL));
    for (int64_t t = 0; t < n_tiles; ++t)
        CHECK(dswx_memcpy_d2h(ctx, wtr + (size_t)t * tile_pixels, layers.wtr + t * geom.tile_stride, tile_pixels));
    const planes_t host = carve(host_mem, pixels);
    const dswx_stack_out_t host_out = outputs_of(host);
    CHECK(dswx_mosaic_host(wtr, &spec, n_tiles, size, size, 0, &place[0][0], canvas, canvas, &host_out));

    /* paste: tile after tile onto the canvas, a later tile over an earlier one where it observed */
    memset(last, 254, pixels);
    for (size_t i = 0; i < pixels; ++i) last_index[i] = DSWX_STACK_NONE;
    for (int64_t t = 0; t < n_tiles; ++t)
        for (int64_t r = 0; r < size; ++r)
            for (int64_t c = 0; c < size; ++c) {
                const size_t i = (size_t)(r + place[t][0]) * (size_t)canvas + (size_t)(c + place[t][1]);
                const unsigned v = wtr[(size_t)t * tile_pixels + (size_t)r * (size_t)size + (size_t)c];
                if (last_index[i] == DSWX_STACK_NONE) last[i] = 255;      /* covered: `fill` until a tile observes it */
                if (v == 1 || v == 2) ++water[i];
                else if (v == 0) ++land[i];
                else continue;
                last[i] = (uint8_t)v;
                last_index[i] = (uint16_t)t;
            }
    int differ = 0;
    uint64_t seen_twice = 0, outside = 0;
    for (size_t i = 0; i < pixels; ++i) {
        const unsigned n_obs = (unsigned)water[i] + land[i];
        const unsigned share = n_obs ? 100u * water[i] / n_obs : DSWX_STACK_NO_SHARE;
        seen_twice += n_obs > 1;
        outside += last[i] == 254;
        const int dev_ok = got.water[i] == water[i] && got.land[i] == land[i] && got.last[i] == last[i] &&
                           got.last_index[i] == last_index[i] && got.share[i] == share;
        const int host_ok = host.water[i] == water[i] && host.land[i] == land[i] && host.last[i] == last[i] &&
                            host.last_index[i] == last_index[i] && host.share[i] == share;
        if ((!dev_ok || !host_ok) && differ < 10) {
            fprintf(stderr, "pixel %zu: loop %u %u %u %u %u, device %u %u %u %u %u, dswx_mosaic_host %u %u %u %u %u\n", i, water[i],
                    land[i], last[i], last_index[i], share, got.water[i], got.land[i], got.last[i], got.last_index[i], got.share[i],
                    host.water[i], host.land[i], host.last[i], host.last_index[i], host.share[i]);
        }
        differ += !dev_ok || !host_ok;
    }
    if (outside) {
        fprintf(stderr, "%" PRIu64 " canvas pixels outside every footprint of a full 2 x 2 block\n", outside);
        differ += 1;
    }
    printf("4 tiles of %zu pixels on a canvas of %" PRId64 " x %" PRId64 ": %" PRIu64 " pixels observed more than once\n", tile_pixels,
           canvas, canvas, seen_twice);
    printf("%s\n", differ ? "MISMATCH" : "wtr mosaic: device, paste loop and host entry agree in every pixel");
    free(last);
    free(last_index);
    free(land);
    free(water);
    free(wtr);
    free(host_mem);
    free(got_mem);
    CHECK(dswx_device_free(ctx, dev));
    CHECK(dswx_device_free(ctx, place_dev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
