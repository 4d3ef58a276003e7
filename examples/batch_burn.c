/*
 * batch_burn.c -- polygons burnt into the OCEAN plane of a resident batch, from plain C (DSWX_HAS_BURN): a small batch with
 * masks is allocated and generated in HBM, its OCEAN plane set to 1 (land), and dswx_batch_burn burns a few polygons -- a
 * triangle that leaves the tile, a rectangle with a hole, a sliver -- into it as 0 (ocean), in place, 16 bytes per vertex
 * crossing PCIe instead of the plane; then the batch is classified with the plane it now has.  The plane and the head are
 * downloaded and checked against this file's own scalar loop over the definition in include/dswx_hip.h ("burn").
 *
 *   gcc -std=c11 -O2 -I include examples/batch_burn.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_burn && ./batch_burn [n_tiles] [size]
 *
 * Exit status 0: the device's plane and head and the loop's agree in every byte -- or there is no device, which is said;
 * 1: they differ, or a call failed.  tests/test_gpu_burn.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_BURN
#error "this header has no burn entries"
#endif

#define WORDS DSWX_BURN_HEAD_WORDS
#define PER_TILE 11

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

/* the records of tile t: three rings on one bit, so that the hole is a hole and the sliver cancels where it overlaps */
static void rings_of_tile(int64_t t, int64_t size, dswx_burn_vertex_t* v) {
    const int32_t s = (int32_t)(256 * size), q = s / 4, d = (int32_t)(37 * t);
    const int32_t pts[PER_TILE][2] = {
        {-3 * 256 + d, q}, {s + 700, q / 2 + d}, {s / 2, s + 900},                            /* a triangle that leaves the tile */
        {q + 128, q + 128}, {3 * q + 128, q + 128}, {3 * q + 128, 3 * q - 128}, {q + 128, 3 * q - 128},   /* corners ON centres */
        {2 * q - 300, 2 * q - 200}, {2 * q + 300, 2 * q - 200}, {2 * q + d, 2 * q + 400},     /* inside both: a hole in a hole */
        {5, 5}};                                                                              /* a stub: next is itself */
    const uint32_t next[PER_TILE] = {1, 2, 0, 4, 5, 6, 3, 8, 9, 7, 10};
    for (int i = 0; i < PER_TILE; ++i) {
        v[i].x = pts[i][0], v[i].y = pts[i][1];
        v[i].word = 1u;
        v[i].next = next[i];
    }
}

static int64_t ceil_div(int64_t a, int64_t b) { return a / b + ((a % b != 0) && ((a < 0) == (b < 0))); }   /* b > 0 here */

/* the definition as a scalar loop: toggles, then the prefix along every row; plane burnt in place with 0 */
static void burn_tile(const dswx_burn_vertex_t* v, int64_t count, int64_t size, uint32_t* acc, uint8_t* plane, uint64_t* head) {
    memset(acc, 0, (size_t)(size * size) * 4);
    memset(head, 0, WORDS * 8);
    head[0] = (uint64_t)count;
    for (int64_t i = 0; i < count; ++i) {
        if ((int64_t)v[i].next >= count) {
            ++head[1];
            continue;
        }
        int64_t x0 = v[i].x, y0 = v[i].y, x1 = v[v[i].next].x, y1 = v[v[i].next].y;
        if (y0 == y1) continue;                            /* (every coordinate here is legal) */
        if (y0 > y1) {
            int64_t k = x0; x0 = x1, x1 = k;
            k = y0, y0 = y1, y1 = k;
        }
        int crossed = 0;
        for (int64_t r = 0; r < size; ++r) {
            const int64_t yc = 256 * r + 128;
            if (!(y0 <= yc && yc < y1)) continue;
            crossed = 1;
            int64_t col = ceil_div((x1 - x0) * (yc - y0) + (x0 - 128) * (y1 - y0), 256 * (y1 - y0));
            if (col < 0) col = 0, ++head[5];
            if (col < size) acc[r * size + col] ^= v[i].word, ++head[3];
            else ++head[4];
        }
        head[2] += (uint64_t)crossed;
    }
    for (int64_t r = 0; r < size; ++r) {
        uint32_t run = 0;
        for (int64_t c = 0; c < size; ++c) {
            run ^= acc[r * size + c];
            acc[r * size + c] = run;
            if (run) plane[r * size + c] = 0, ++head[6];
        }
    }
}

int main(int argc, char** argv) {
    const int64_t n_tiles = argc > 1 ? atoll(argv[1]) : 3;
    const int64_t size = argc > 2 ? atoll(argv[2]) : 150;
    if (dswx_abi_version() != DSWX_ABI_VERSION) {
        fprintf(stderr, "header / library ABI mismatch: %d vs %d\n", DSWX_ABI_VERSION, dswx_abi_version());
        return 1;
    }
    if (n_tiles < 1 || size < 8 || size > 4096) {
        fprintf(stderr, "at least one tile of 8 .. 4096 pixels a side\n");
        return 1;
    }
    if (dswx_device_count() <= 0) {
        printf("no device: nothing burnt (there is no CPU fallback; dswx_burn_host is the other half of a comparison)\n");
        return 0;
    }
    dswx_ctx_t* ctx = NULL;
    CHECK(dswx_ctx_create(0, &ctx));
    dswx_params_t params;
    CHECK(dswx_params_default(&params));

    dswx_batch_geom_t geom = {n_tiles, size, size, 0};
    dswx_batch_t* batch = NULL;
    CHECK(dswx_batch_create(ctx, &geom, DSWX_BATCH_MASKS, &batch));
    CHECK(dswx_batch_synth(batch, 20261020u, 0, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));            /* the generator wrote the masks too */
    dswx_planes_in_t in;
    CHECK(dswx_batch_planes(batch, &geom, &in, NULL, NULL));
    const size_t pixels = (size_t)size * (size_t)size, nt = (size_t)n_tiles;
    CHECK(dswx_memset_d(ctx, (void*)(uintptr_t)in.ocean, 1, nt * (size_t)geom.tile_stride));   /* all land (the batch's own memory) */

    /* the records of all tiles, the table, acc and head side by side in one allocation: 16-, 8-, 8- and 4-byte aligned */
    const size_t v_bytes = nt * PER_TILE * sizeof(dswx_burn_vertex_t), f_bytes = (nt + 1) * 8, h_bytes = nt * WORDS * 8;
    dswx_burn_vertex_t* verts = malloc(v_bytes);
    int64_t* first = malloc(f_bytes);
    if (!verts || !first) return 1;
    for (int64_t t = 0; t < n_tiles; ++t) {
        rings_of_tile(t, size, verts + t * PER_TILE);
        first[t] = t * PER_TILE;
    }
    first[n_tiles] = n_tiles * PER_TILE;
    uint8_t* dev = NULL;
    CHECK(dswx_device_malloc(ctx, v_bytes + f_bytes + h_bytes + nt * pixels * 4, (void**)&dev));
    dswx_burn_vertex_t* d_verts = (dswx_burn_vertex_t*)dev;
    int64_t* d_first = (int64_t*)(dev + v_bytes);
    uint64_t* d_head = (uint64_t*)(dev + v_bytes + f_bytes);
    uint32_t* d_acc = (uint32_t*)(dev + v_bytes + f_bytes + h_bytes);
    CHECK(dswx_memcpy_h2d(ctx, d_verts, verts, v_bytes));
    CHECK(dswx_memcpy_h2d(ctx, d_first, first, f_bytes));

    dswx_burn_spec_t spec = {0, 1, 0, 0};                 /* burn 0 = ocean; the strides are the batch's */
    /* same stream as the generator (NULL = the context's): ordered behind it, and the classification behind the burn */
    CHECK(dswx_batch_burn(batch, DSWX_PLANE_OCEAN, d_verts, d_first, &spec, d_acc, d_head, 0, DSWX_BATCH_ALL_TILES, NULL));
    CHECK(dswx_batch_classify(batch, &params, DSWX_BATCH_ALL_TILES, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));

    uint8_t* got = malloc(pixels + 1);
    uint8_t* want = malloc(pixels + 1);
    uint32_t* acc = malloc(pixels * 4 + 4);
    uint64_t* got_head = malloc(h_bytes);
    if (!got || !want || !acc || !got_head) return 1;
    CHECK(dswx_memcpy_d2h(ctx, got_head, d_head, h_bytes));
    int differ = 0;
    uint64_t ocean = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        uint64_t head[WORDS];
        memset(want, 1, pixels);
        burn_tile(verts + t * PER_TILE, PER_TILE, size, acc, want, head);
        CHECK(dswx_memcpy_d2h(ctx, got, in.ocean + t * geom.tile_stride, pixels));
        for (size_t p = 0; p < pixels; ++p)
            if (got[p] != want[p]) {
                if (differ < 10) fprintf(stderr, "tile %" PRId64 " pixel %zu: loop %u, device %u\n", t, p, want[p], got[p]);
                ++differ;
            }
        for (int w = 0; w < WORDS; ++w)
            if (got_head[(size_t)t * WORDS + w] != head[w]) {
                fprintf(stderr, "tile %" PRId64 " head word %d: loop %" PRIu64 ", device %" PRIu64 "\n", t, w, head[w], got_head[(size_t)t * WORDS + w]);
                ++differ;
            }
        ocean += head[6];
    }
    printf("%" PRId64 " tiles of %" PRId64 " x %" PRId64 " pixels: %" PRIu64 " pixels burnt as ocean from %d records a tile, then classified\n",
           n_tiles, size, size, ocean, PER_TILE);
    if (!differ) printf("burn: device and scalar loop agree in every pixel and every head word\n");
    else fprintf(stderr, "burn: %d differences\n", differ);

    free(got);
    free(want);
    free(acc);
    free(got_head);
    free(verts);
    free(first);
    CHECK(dswx_device_free(ctx, dev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
