/*
 * batch_stack.c -- the tiles of a resident batch composited per pixel, from plain C (DSWX_HAS_STACK): a small batch is
 * allocated, generated and classified in HBM; its tiles are taken as the dates of one place, and dswx_batch_stack turns the
 * WTR layer into five planes with one kernel launch -- how often a pixel was water, how often clear and not water, its
 * latest clear observation, the tile that observation came from, and the share of water among its observations.  The planes
 * stay in device memory; here they are downloaded, with the WTR layer, and checked against a loop in C and against
 * dswx_stack_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_stack.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_stack && ./batch_stack [n_tiles] [size]
 *
 * Exit status 0: the device's planes, the loop's and the host entry's agree in every pixel; 1: they differ, or a call failed.
 * tests/test_gpu_stack.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_STACK
#error "this header has no stack entries"
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
    dswx_stack_spec_t spec;
    memset(&spec, 0, sizeof spec);
    spec.n_cats = 2;
    spec.fill = 255;
    memset(spec.cat_of_byte, 255, sizeof spec.cat_of_byte);
    spec.cat_of_byte[1] = spec.cat_of_byte[2] = 0;
    spec.cat_of_byte[0] = 1;

    const size_t pixels = (size_t)size * (size_t)size;
    const size_t bytes = pixels > 0 ? pixels * 8 : 8;       /* 3 uint16 planes + 2 byte planes */
    void* dev = NULL;
    CHECK(dswx_device_malloc(ctx, bytes, &dev));
    const dswx_stack_out_t dev_out = outputs_of(carve(dev, pixels));
    /* same stream as the classification (NULL = the context's): ordered behind it; asynchronous, so the copy below, which is
     * complete on return, is what waits for it */
    CHECK(dswx_batch_stack(batch, DSWX_PLANE_WTR, &spec, 0, DSWX_BATCH_ALL_TILES, &dev_out, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));
    uint8_t* got_mem = malloc(bytes);
    uint8_t* host_mem = malloc(bytes);
    uint8_t* wtr = malloc(pixels > 0 && n_tiles > 0 ? pixels * (size_t)n_tiles : 1);
    if (!got_mem || !host_mem || !wtr) return 1;
    CHECK(dswx_memcpy_d2h(ctx, got_mem, dev, bytes));
    const planes_t got = carve(got_mem, pixels);

    /* the other half: the WTR layer on the host, tile after tile without the padding */
    dswx_planes_out_t layers;
    CHECK(dswx_batch_planes(batch, &geom, NULL, &layers, NULL));
    for (int64_t t = 0; t < n_tiles; ++t)
        if (pixels) CHECK(dswx_memcpy_d2h(ctx, wtr + (size_t)t * pixels, layers.wtr + t * geom.tile_stride, pixels));
    const planes_t host = carve(host_mem, pixels);
    const dswx_stack_out_t host_out = outputs_of(host);
    CHECK(dswx_stack_host(wtr, &spec, n_tiles, (int64_t)pixels, 0, &host_out));

    int differ = 0;
    uint64_t ever_water = 0, never_seen = 0;
    for (size_t i = 0; i < pixels; ++i) {
        unsigned water = 0, land = 0, last = 255, last_index = DSWX_STACK_NONE;
        for (int64_t t = 0; t < n_tiles; ++t) {
            const unsigned v = wtr[(size_t)t * pixels + i];
            if (v == 1 || v == 2) ++water;
            else if (v == 0) ++land;
            else continue;
            last = v;
            last_index = (unsigned)t;
        }
        const unsigned share = water + land ? 100 * water / (water + land) : DSWX_STACK_NO_SHARE;
        ever_water += water > 0;
        never_seen += water + land == 0;
        const int dev_ok = got.water[i] == water && got.land[i] == land && got.last[i] == last &&
                           got.last_index[i] == last_index && got.share[i] == share;
        const int host_ok = host.water[i] == water && host.land[i] == land && host.last[i] == last &&
                            host.last_index[i] == last_index && host.share[i] == share;
        if ((!dev_ok || !host_ok) && differ < 10) {
            fprintf(stderr, "pixel %zu: loop %u %u %u %u %u, device %u %u %u %u %u, dswx_stack_host %u %u %u %u %u\n", i, water,
                    land, last, last_index, share, got.water[i], got.land[i], got.last[i], got.last_index[i], got.share[i],
                    host.water[i], host.land[i], host.last[i], host.last_index[i], host.share[i]);
        }
        differ += !dev_ok || !host_ok;
    }
    printf("%" PRId64 " tiles of %zu pixels: %" PRIu64 " pixels water at least once, %" PRIu64 " never observed\n", n_tiles,
           pixels, ever_water, never_seen);
    printf("%s\n", differ ? "MISMATCH" : "wtr stack: device, loop and host entry agree in every pixel");
    free(wtr);
    free(host_mem);
    free(got_mem);
    CHECK(dswx_device_free(ctx, dev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
