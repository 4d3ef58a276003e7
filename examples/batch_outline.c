/*
 * batch_outline.c -- the outlines of the water bodies of a resident batch as ordered rings, from plain C (DSWX_HAS_OUTLINE): a
 * small batch is allocated, generated and classified in HBM, dswx_batch_label groups the water pixels of its WTR layer into
 * bodies, and dswx_outline_device traces the bodies of that label plane: first the COUNTING CALL (head alone, no capacity),
 * which says how many edges every tile has, then the call with the capacities that fit.  The working memory is the
 * caller's: dswx_outline_work_bytes says how much.  Everything stays in device memory; here the chain, the rings and the head
 * are downloaded with the label plane and checked against dswx_outline_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_outline.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_outline && ./batch_outline [n_tiles] [size]
 *
 * Exit status 0: the device's outputs and the host entry's agree in every byte; 1: they differ, or a call failed.
 * tests/test_gpu_outline.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_OUTLINE
#error "this header has no outline entries"
#endif

#define RW DSWX_OUTLINE_ROW_WORDS
#define HW DSWX_OUTLINE_HEAD_WORDS

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

/* the three outputs side by side in one allocation: head first (8-byte aligned), then the rings (32 bytes each), then the chain */
static dswx_outline_out_t carve(uint8_t* base, size_t n_tiles, size_t max_edges, size_t max_rings) {
    dswx_outline_out_t o;
    o.head = (uint64_t*)base;
    o.rings = (uint32_t*)(o.head + n_tiles * HW);
    o.chain = o.rings + n_tiles * max_rings * RW;
    (void)max_edges;
    return o;
}

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

    const size_t pixels = (size_t)size * (size_t)size;
    const size_t nt = (size_t)n_tiles;

    /* label the water of WTR: the label plane alone */
    dswx_label_spec_t lspec;
    memset(&lspec, 0, sizeof lspec);
    lspec.connectivity = 8;
    lspec.min_size = 1;
    lspec.member_of_byte[1] = lspec.member_of_byte[2] = 1;
    void* ldev = NULL;
    CHECK(dswx_device_malloc(ctx, 4 * nt * pixels + 16, &ldev));
    dswx_label_out_t lout;
    memset(&lout, 0, sizeof lout);
    lout.label = (uint32_t*)ldev;
    CHECK(dswx_batch_label(batch, DSWX_PLANE_WTR, &lspec, 0, DSWX_BATCH_ALL_TILES, &lout, NULL));

    /* the counting call: head alone and no capacity -- word 0 of every tile is its E, word 7 says that it did not fit */
    dswx_outline_spec_t spec;
    memset(&spec, 0, sizeof spec);
    spec.connectivity = 8;
    uint64_t work_bytes = 0;
    CHECK(dswx_outline_work_bytes(&spec, n_tiles, size, size, &work_bytes));
    void* work = NULL;
    void* hdev = NULL;
    CHECK(dswx_device_malloc(ctx, (size_t)work_bytes, &work));
    CHECK(dswx_device_malloc(ctx, 8 * HW * nt + 8, &hdev));
    dswx_outline_out_t count_out = {NULL, NULL, (uint64_t*)hdev};
    /* same stream as the labelling (NULL = the context's): ordered behind it; asynchronous */
    CHECK(dswx_outline_device(ctx, lout.label, &spec, n_tiles, size, size, &count_out, work, work_bytes, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));
    uint64_t* counted = malloc(8 * HW * nt + 8);
    if (!counted) return 1;
    CHECK(dswx_memcpy_d2h(ctx, counted, hdev, 8 * HW * nt));
    size_t max_edges = 0;
    for (size_t t = 0; t < nt; ++t)
        if (counted[t * HW] > max_edges) max_edges = (size_t)counted[t * HW];
    CHECK(dswx_device_free(ctx, work));
    CHECK(dswx_device_free(ctx, hdev));

    /* the call that fits: a ring has at least 4 edges */
    const size_t max_rings = max_edges / 4;
    spec.max_edges = (int64_t)max_edges;
    spec.max_rings = (int64_t)max_rings;
    CHECK(dswx_outline_work_bytes(&spec, n_tiles, size, size, &work_bytes));
    CHECK(dswx_device_malloc(ctx, (size_t)work_bytes, &work));
    const size_t bytes = nt * (8 * HW + 4 * RW * max_rings + 4 * max_edges) + 16;
    void* dev = NULL;
    CHECK(dswx_device_malloc(ctx, bytes, &dev));
    dswx_outline_out_t dev_out = carve(dev, nt, max_edges, max_rings);
    if (!max_rings) dev_out.rings = NULL;
    CHECK(dswx_outline_device(ctx, lout.label, &spec, n_tiles, size, size, &dev_out, work, work_bytes, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));

    uint8_t* got_mem = malloc(bytes);
    uint8_t* host_mem = malloc(bytes);
    uint32_t* label = malloc(4 * pixels * nt + 4);
    if (!got_mem || !host_mem || !label) return 1;
    memset(host_mem, 0, bytes);
    CHECK(dswx_memcpy_d2h(ctx, got_mem, dev, bytes));
    CHECK(dswx_memcpy_d2h(ctx, label, lout.label, 4 * pixels * nt));
    const dswx_outline_out_t got = carve(got_mem, nt, max_edges, max_rings);
    dswx_outline_out_t host = carve(host_mem, nt, max_edges, max_rings);
    if (!max_rings) host.rings = NULL;
    CHECK(dswx_outline_host(label, &spec, n_tiles, size, size, &host));

    int differ = 0;
    uint64_t edges = 0, rings = 0, holes = 0;
    uint32_t best[RW] = {0};
    int64_t best_tile = -1;
    for (size_t t = 0; t < nt; ++t) {
        for (int w = 0; w < HW; ++w)
            if (got.head[t * HW + w] != host.head[t * HW + w]) {
                fprintf(stderr, "tile %zu head word %d: device %" PRIu64 ", dswx_outline_host %" PRIu64 "\n", t, w, got.head[t * HW + w],
                        host.head[t * HW + w]);
                ++differ;
            }
        if (got.head[t * HW] != counted[t * HW] || got.head[t * HW + 7] != 0) ++differ;      /* the counting call said the same E */
        for (size_t i = t * max_edges; i < (t + 1) * max_edges; ++i)
            if (got.chain[i] != host.chain[i] && differ++ < 10)
                fprintf(stderr, "tile %zu chain entry %zu: device %u, dswx_outline_host %u\n", t, i - t * max_edges, got.chain[i], host.chain[i]);
        for (size_t j = 0; j < max_rings; ++j) {
            const uint32_t* g = got.rings + (t * max_rings + j) * RW;
            const uint32_t* h = host.rings + (t * max_rings + j) * RW;
            if (memcmp(g, h, 4 * RW) != 0 && differ++ < 10) fprintf(stderr, "tile %zu ring %zu differs\n", t, j);
            if (g[3] > best[3]) {
                memcpy(best, g, sizeof best);
                best_tile = (int64_t)t;
            }
        }
        edges += got.head[t * HW];
        rings += got.head[t * HW + 1];
        holes += got.head[t * HW + 5];
    }
    printf("%" PRId64 " tiles of %" PRId64 " x %" PRId64 " pixels: %" PRIu64 " shoreline edges in %" PRIu64 " rings, %" PRIu64
           " of them holes; capacity %zu edges and %zu rings per tile, %" PRIu64 " bytes of working memory\n", n_tiles, size, size, edges, rings,
           holes, max_edges, max_rings, work_bytes);
    if (best_tile >= 0) {
        const int64_t area2 = (int64_t)((uint64_t)best[6] | ((uint64_t)best[7] << 32));
        printf("largest ring: tile %" PRId64 ", body %u, from pixel (%u, %u), %u edges, %u corners, %s of %" PRId64 " half pixels\n", best_tile,
               best[0], (best[1] >> 2) % (uint32_t)size, (best[1] >> 2) / (uint32_t)size, best[3], best[4], area2 > 0 ? "an outer ring" : "a hole",
               area2 > 0 ? area2 : -area2);
    } else {
        printf("largest ring: none\n");
    }
    printf("%s\n", differ ? "MISMATCH" : "wtr outlines: device and host entry agree in every byte");
    free(label);
    free(host_mem);
    free(got_mem);
    free(counted);
    CHECK(dswx_device_free(ctx, dev));
    CHECK(dswx_device_free(ctx, work));
    CHECK(dswx_device_free(ctx, ldev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
