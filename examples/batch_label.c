/*
 * batch_label.c -- the water bodies of a layer of a resident batch, from plain C (DSWX_HAS_LABEL): a small batch is allocated,
 * generated and classified in HBM, and dswx_batch_label groups the water pixels of its WTR layer into connected bodies --
 * per pixel the label and the size of its body, the layer with every body of fewer than MIN_SIZE pixels turned into "not
 * water", and per tile a summary.  The planes stay in device memory; here they are downloaded, with the WTR layer, and checked
 * against a flood fill in C and against dswx_label_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_label.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_label && ./batch_label [n_tiles] [size]
 *
 * Exit status 0: the device's planes, the loop's and the host entry's agree in every pixel; 1: they differ, or a call failed.
 * tests/test_gpu_label.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_LABEL
#error "this header has no label entries"
#endif

#define MIN_SIZE 4
#define WORDS DSWX_LABEL_SUMMARY_WORDS

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

/* the four outputs side by side in one allocation: summary first (8-byte aligned), then label, size and sieved */
static dswx_label_out_t carve(uint8_t* base, size_t n_tiles, size_t pixels) {
    dswx_label_out_t o;
    o.summary = (uint64_t*)base;
    o.label = (uint32_t*)(o.summary + n_tiles * WORDS);
    o.size = o.label + n_tiles * pixels;
    o.sieved = (uint8_t*)(o.size + n_tiles * pixels);
    return o;
}

static int is_water(unsigned v) { return v == 1 || v == 2; }    /* the saved WTR classes: open and partial surface water */

int main(int argc, char** argv) {
    const int64_t n_tiles = argc > 1 ? atoll(argv[1]) : 3;
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

    dswx_label_spec_t spec;
    memset(&spec, 0, sizeof spec);
    spec.connectivity = 8;
    spec.replace = 0;                              /* a body that is too small becomes "not water" */
    spec.min_size = MIN_SIZE;
    spec.member_of_byte[1] = spec.member_of_byte[2] = 1;

    const size_t pixels = (size_t)size * (size_t)size;
    const size_t nt = (size_t)n_tiles;
    const size_t bytes = nt * (8 * WORDS + 9 * pixels) + 16;
    void* dev = NULL;
    CHECK(dswx_device_malloc(ctx, bytes, &dev));
    const dswx_label_out_t dev_out = carve(dev, nt, pixels);
    /* same stream as the classification (NULL = the context's): ordered behind it; asynchronous, so the copy below, which is
     * complete on return, is what waits for it */
    CHECK(dswx_batch_label(batch, DSWX_PLANE_WTR, &spec, 0, DSWX_BATCH_ALL_TILES, &dev_out, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));
    uint8_t* got_mem = malloc(bytes);
    uint8_t* host_mem = malloc(bytes);
    uint8_t* wtr = malloc(pixels * nt + 1);
    uint32_t* lab = malloc(4 * pixels + 4);
    int64_t* todo = malloc(8 * pixels + 8);
    int64_t* body = malloc(8 * pixels + 8);
    if (!got_mem || !host_mem || !wtr || !lab || !todo || !body) return 1;
    CHECK(dswx_memcpy_d2h(ctx, got_mem, dev, bytes));
    const dswx_label_out_t got = carve(got_mem, nt, pixels);

    /* the other half: the WTR layer on the host, tile after tile without the padding */
    dswx_planes_out_t layers;
    CHECK(dswx_batch_planes(batch, &geom, NULL, &layers, NULL));
    for (int64_t t = 0; t < n_tiles; ++t)
        if (pixels) CHECK(dswx_memcpy_d2h(ctx, wtr + (size_t)t * pixels, layers.wtr + t * geom.tile_stride, pixels));
    const dswx_label_out_t host = carve(host_mem, nt, pixels);
    CHECK(dswx_label_host(wtr, &spec, n_tiles, size, size, 0, &host));

    int differ = 0;
    uint64_t bodies = 0, kept = 0, largest = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const uint8_t* tile = wtr + (size_t)t * pixels;
        const size_t o = (size_t)t * pixels;
        uint64_t sum[WORDS];
        memset(sum, 0, sizeof sum);
        memset(lab, 0, 4 * pixels);
        /* a flood fill from every water pixel not yet reached, in raster order: the seed is the first pixel of its body */
        for (int64_t seed = 0; seed < (int64_t)pixels; ++seed) {
            if (!is_water(tile[seed])) continue;
            ++sum[1];
            if (lab[seed]) continue;
            int64_t n_todo = 0, n_body = 0;
            todo[n_todo++] = seed;
            lab[seed] = (uint32_t)seed + 1u;
            while (n_todo) {
                const int64_t p = todo[--n_todo], y = p / size, x = p % size;
                body[n_body++] = p;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int64_t yy = y + dy, xx = x + dx;
                        if (yy < 0 || yy >= size || xx < 0 || xx >= size) continue;
                        const int64_t q = yy * size + xx;
                        if (!is_water(tile[q]) || lab[q]) continue;
                        lab[q] = (uint32_t)seed + 1u;
                        todo[n_todo++] = q;
                    }
            }
            ++sum[0];
            if ((uint64_t)n_body > sum[2]) {
                sum[2] = (uint64_t)n_body;
                sum[3] = (uint64_t)seed + 1u;
            }
            if (n_body >= MIN_SIZE) {
                ++sum[4];
                sum[5] += (uint64_t)n_body;
            }
            int b = 0;
            for (int64_t s = n_body; s > 1; s >>= 1) ++b;
            ++sum[8 + b];
            /* every pixel of the body must carry this size */
            for (int64_t i = 0; i < n_body; ++i)
                if (got.size[o + body[i]] != (uint32_t)n_body || host.size[o + body[i]] != (uint32_t)n_body) ++differ;
        }
        for (size_t p = 0; p < pixels; ++p) {
            const unsigned small = lab[p] && got.size[o + p] < MIN_SIZE;
            const unsigned sieved = small ? 0u : tile[p];
            const int dev_ok = got.label[o + p] == lab[p] && got.sieved[o + p] == sieved && (lab[p] || got.size[o + p] == 0);
            const int host_ok = host.label[o + p] == lab[p] && host.sieved[o + p] == sieved && (lab[p] || host.size[o + p] == 0);
            if ((!dev_ok || !host_ok) && differ < 10)
                fprintf(stderr, "tile %" PRId64 " pixel %zu: loop %u %u, device %u %u %u, dswx_label_host %u %u %u\n", t, p, lab[p], sieved,
                        got.label[o + p], got.size[o + p], got.sieved[o + p], host.label[o + p], host.size[o + p], host.sieved[o + p]);
            differ += !dev_ok || !host_ok;
        }
        for (int w = 0; w < WORDS; ++w) {
            if (got.summary[(size_t)t * WORDS + w] != sum[w] || host.summary[(size_t)t * WORDS + w] != sum[w]) {
                fprintf(stderr, "tile %" PRId64 " summary word %d: loop %" PRIu64 ", device %" PRIu64 ", dswx_label_host %" PRIu64 "\n", t, w,
                        sum[w], got.summary[(size_t)t * WORDS + w], host.summary[(size_t)t * WORDS + w]);
                ++differ;
            }
        }
        bodies += sum[0];
        kept += sum[4];
        if (sum[2] > largest) largest = sum[2];
    }
    printf("%" PRId64 " tiles of %" PRId64 " x %" PRId64 " pixels: %" PRIu64 " water bodies, %" PRIu64 " of at least %d pixels, the largest %" PRIu64
           " pixels\n", n_tiles, size, size, bodies, kept, MIN_SIZE, largest);
    printf("%s\n", differ ? "MISMATCH" : "wtr label: device, loop and host entry agree in every pixel");
    free(body);
    free(todo);
    free(lab);
    free(wtr);
    free(host_mem);
    free(got_mem);
    CHECK(dswx_device_free(ctx, dev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
