/*
 * batch_distance.c -- the distance of every pixel of a layer of a resident batch to the nearest water, from plain C
 * (DSWX_HAS_DISTANCE): a small batch is allocated, generated and classified in HBM, and dswx_batch_distance measures, in its
 * WTR layer, the squared distance of every pixel to the nearest water pixel within RADIUS pixels, which pixel that is, the
 * layer with the ring of non-water pixels within the radius marked, and per tile a summary.  The planes stay in device
 * memory; here they are downloaded, with the WTR layer, and every output of the first and the last tile is checked against a
 * brute-force loop over all pairs of a pixel and a water pixel.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_distance.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_distance && ./batch_distance [n_tiles] [size]
 *
 * Exit status 0: the device's planes and the loop's agree in every pixel; 1: they differ, or a call failed.
 * tests/test_gpu_distance.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_DISTANCE
#error "this header has no distance entries"
#endif

#define RADIUS 6
#define MARK 200
#define WORDS DSWX_DISTANCE_SUMMARY_WORDS

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

/* the four outputs side by side in one allocation: summary first (8-byte aligned), then dist2, nearest and within */
static dswx_distance_out_t carve(uint8_t* base, size_t n_tiles, size_t pixels) {
    dswx_distance_out_t o;
    o.summary = (uint64_t*)base;
    o.dist2 = (uint32_t*)(o.summary + n_tiles * WORDS);
    o.nearest = o.dist2 + n_tiles * pixels;
    o.within = (uint8_t*)(o.nearest + n_tiles * pixels);
    return o;
}

static int is_water(unsigned v) { return v == 1 || v == 2; }    /* the saved WTR classes: open and partial surface water */

int main(int argc, char** argv) {
    const int64_t n_tiles = argc > 1 ? atoll(argv[1]) : 3;
    const int64_t size = argc > 2 ? atoll(argv[2]) : 150;
    if (dswx_abi_version() != DSWX_ABI_VERSION) {
        fprintf(stderr, "header / library ABI mismatch: %d vs %d\n", DSWX_ABI_VERSION, dswx_abi_version());
        return 1;
    }
    if (n_tiles < 1 || size < 1 || size > DSWX_DISTANCE_MAX_WIDTH) {
        fprintf(stderr, "at least one tile of 1 .. %d pixels a side\n", DSWX_DISTANCE_MAX_WIDTH);
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

    dswx_distance_spec_t spec;
    memset(&spec, 0, sizeof spec);
    spec.max_radius = RADIUS;
    spec.mark = MARK;
    spec.target_of_byte[1] = spec.target_of_byte[2] = 1;

    const size_t pixels = (size_t)size * (size_t)size;
    const size_t nt = (size_t)n_tiles;
    const size_t bytes = nt * (8 * WORDS + 9 * pixels) + 16;
    void* dev = NULL;
    CHECK(dswx_device_malloc(ctx, bytes, &dev));
    const dswx_distance_out_t dev_out = carve(dev, nt, pixels);
    /* same stream as the classification (NULL = the context's): ordered behind it; asynchronous, so the copy below, which is
     * complete on return, is what waits for it */
    CHECK(dswx_batch_distance(batch, DSWX_PLANE_WTR, &spec, 0, DSWX_BATCH_ALL_TILES, &dev_out, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));
    uint8_t* got_mem = malloc(bytes);
    uint8_t* wtr = malloc(pixels * nt + 1);
    int64_t* water = malloc(8 * pixels + 8);
    if (!got_mem || !wtr || !water) return 1;
    CHECK(dswx_memcpy_d2h(ctx, got_mem, dev, bytes));
    const dswx_distance_out_t got = carve(got_mem, nt, pixels);

    /* the other half: the WTR layer on the host, tile after tile without the padding */
    dswx_planes_out_t layers;
    CHECK(dswx_batch_planes(batch, &geom, NULL, &layers, NULL));
    for (int64_t t = 0; t < n_tiles; ++t)
        CHECK(dswx_memcpy_d2h(ctx, wtr + (size_t)t * pixels, layers.wtr + t * geom.tile_stride, pixels));

    int differ = 0;
    uint64_t ring = 0, far = 0;
    for (int64_t t = 0; t < n_tiles; t += n_tiles > 1 ? n_tiles - 1 : 1) {          /* the first tile and the last */
        const uint8_t* tile = wtr + (size_t)t * pixels;
        const size_t o = (size_t)t * pixels;
        uint64_t sum[WORDS];
        memset(sum, 0, sizeof sum);
        int64_t n_water = 0;
        for (int64_t p = 0; p < (int64_t)pixels; ++p)
            if (is_water(tile[p])) water[n_water++] = p;
        int any = 0;
        for (int64_t p = 0; p < (int64_t)pixels; ++p) {
            const int64_t y = p / size, x = p % size;
            /* every water pixel against this one: the smallest (d2, column, row) within the radius wins */
            uint64_t best = UINT64_MAX;
            int64_t best_q = -1;
            for (int64_t i = 0; i < n_water; ++i) {
                const int64_t qy = water[i] / size, qx = water[i] % size;
                const int64_t d2 = (y - qy) * (y - qy) + (x - qx) * (x - qx);
                if (d2 > RADIUS * RADIUS) continue;
                const uint64_t key = ((uint64_t)d2 << 40) | ((uint64_t)qx << 20) | (uint64_t)qy;
                if (key < best) best = key, best_q = water[i];
            }
            const uint32_t d2 = best_q < 0 ? DSWX_DISTANCE_NONE : (uint32_t)(best >> 40);
            const uint32_t nearest = best_q < 0 ? DSWX_DISTANCE_NONE : (uint32_t)best_q;
            const unsigned within = best_q >= 0 && !is_water(tile[p]) ? MARK : tile[p];
            if (got.dist2[o + p] != d2 || got.nearest[o + p] != nearest || got.within[o + p] != within) {
                if (differ < 10)
                    fprintf(stderr, "tile %" PRId64 " pixel %" PRId64 ": loop %u %u %u, device %u %u %u\n", t, p, d2, nearest, within,
                            got.dist2[o + p], got.nearest[o + p], got.within[o + p]);
                ++differ;
            }
            if (best_q < 0) {
                ++sum[2];
                continue;
            }
            ++sum[d2 ? 1 : 0];
            sum[5] += d2;
            if (!any || d2 > sum[3]) sum[3] = d2, sum[4] = (uint64_t)p, any = 1;     /* the first pixel with the largest */
            if (d2) {
                int b = 0;
                for (uint32_t s = d2; s > 1; s >>= 1) ++b;
                ++sum[8 + b];
            }
        }
        for (int w = 0; w < WORDS; ++w)
            if (got.summary[(size_t)t * WORDS + w] != sum[w]) {
                fprintf(stderr, "tile %" PRId64 " summary word %d: loop %" PRIu64 ", device %" PRIu64 "\n", t, w, sum[w],
                        got.summary[(size_t)t * WORDS + w]);
                ++differ;
            }
        ring += sum[1];
        far += sum[2];
    }
    printf("%" PRId64 " tiles of %" PRId64 " x %" PRId64 " pixels: in the first and the last, %" PRIu64 " pixels within %d pixels of water, %" PRIu64
           " further away\n", n_tiles, size, size, ring, RADIUS, far);
    if (!differ) printf("wtr distance: device and brute force agree in every pixel\n");
    else fprintf(stderr, "wtr distance: %d differences\n", differ);

    free(got_mem);
    free(wtr);
    free(water);
    CHECK(dswx_device_free(ctx, dev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
