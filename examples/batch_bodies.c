/*
 * batch_bodies.c -- a table of the water bodies of a resident batch, from plain C (DSWX_HAS_BODY_TABLE): a small batch is
 * allocated, generated and classified in HBM, dswx_batch_label groups the water pixels of its WTR layer into bodies, and
 * dswx_batch_body_table renumbers them 1 .. K and writes one 64-byte row per body -- where it is, how large, how long its
 * shoreline, how much of it open and how much partial surface water -- with the WTR layer itself as the value plane.  The
 * capacity of the table is the largest body count of the label summaries (word 0), read before the table is allocated.
 * Everything stays in device memory; here it is downloaded, with the label and WTR planes, and every row checked against a
 * loop in C over those planes and against dswx_body_table_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_bodies.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_bodies && ./batch_bodies [n_tiles] [size]
 *
 * Exit status 0: the device's table, the loop's and the host entry's agree in every row; 1: they differ, or a call failed.
 * tests/test_gpu_body_table.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_BODY_TABLE
#error "this header has no body-table entries"
#endif

#define RW DSWX_BODY_ROW_WORDS
#define HW DSWX_BODY_HEAD_WORDS

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

/* the three outputs side by side in one allocation: head first (8-byte aligned), then the rows (64 bytes each), then dense */
static dswx_body_out_t carve(uint8_t* base, size_t n_tiles, size_t max_rows) {
    dswx_body_out_t o;
    o.head = (uint64_t*)base;
    o.rows = (uint32_t*)(o.head + n_tiles * HW);
    o.dense = o.rows + n_tiles * max_rows * RW;
    return o;
}

static uint64_t word64(const uint32_t* row, int w) { return (uint64_t)row[w] | ((uint64_t)row[w + 1] << 32); }

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

    /* label the water of WTR: label and size planes and the summary, whose word 0 is the number of bodies of a tile */
    dswx_label_spec_t lspec;
    memset(&lspec, 0, sizeof lspec);
    lspec.connectivity = 8;
    lspec.min_size = 1;
    lspec.member_of_byte[1] = lspec.member_of_byte[2] = 1;
    void* ldev = NULL;
    CHECK(dswx_device_malloc(ctx, nt * (8 * DSWX_LABEL_SUMMARY_WORDS + 8 * pixels) + 16, &ldev));
    dswx_label_out_t lout;
    lout.summary = (uint64_t*)ldev;
    lout.label = (uint32_t*)(lout.summary + nt * DSWX_LABEL_SUMMARY_WORDS);
    lout.size = lout.label + nt * pixels;
    lout.sieved = NULL;
    CHECK(dswx_batch_label(batch, DSWX_PLANE_WTR, &lspec, 0, DSWX_BATCH_ALL_TILES, &lout, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));
    uint64_t* summary = malloc(8 * DSWX_LABEL_SUMMARY_WORDS * nt + 8);
    if (!summary) return 1;
    CHECK(dswx_memcpy_d2h(ctx, summary, lout.summary, 8 * DSWX_LABEL_SUMMARY_WORDS * nt));
    size_t max_rows = 0;
    for (size_t t = 0; t < nt; ++t)
        if (summary[t * DSWX_LABEL_SUMMARY_WORDS] > max_rows) max_rows = (size_t)summary[t * DSWX_LABEL_SUMMARY_WORDS];

    /* the table: open water (byte 1) is category 0, partial surface water (byte 2) category 1 */
    dswx_body_spec_t spec;
    memset(&spec, 0, sizeof spec);
    memset(spec.cat_of_byte, 255, sizeof spec.cat_of_byte);
    spec.n_cats = 2;
    spec.cat_of_byte[1] = 0;
    spec.cat_of_byte[2] = 1;
    spec.max_rows = (int64_t)max_rows;
    const size_t bytes = nt * (8 * HW + 4 * RW * max_rows + 4 * pixels) + 16;
    void* dev = NULL;
    CHECK(dswx_device_malloc(ctx, bytes, &dev));
    dswx_body_out_t dev_out = carve(dev, nt, max_rows);
    if (!max_rows) dev_out.rows = NULL;
    /* same stream as the labelling (NULL = the context's): ordered behind it; asynchronous */
    CHECK(dswx_batch_body_table(batch, DSWX_PLANE_WTR, &spec, 0, DSWX_BATCH_ALL_TILES, lout.label, &dev_out, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));

    uint8_t* got_mem = malloc(bytes);
    uint8_t* host_mem = malloc(bytes);
    uint8_t* wtr = malloc(pixels * nt + 1);
    uint32_t* label = malloc(4 * pixels * nt + 4);
    uint32_t* mine = calloc(RW * (max_rows + 1), 4);
    if (!got_mem || !host_mem || !wtr || !label || !mine) return 1;
    CHECK(dswx_memcpy_d2h(ctx, got_mem, dev, bytes));
    CHECK(dswx_memcpy_d2h(ctx, label, lout.label, 4 * pixels * nt));
    const dswx_body_out_t got = carve(got_mem, nt, max_rows);
    dswx_planes_out_t layers;
    CHECK(dswx_batch_planes(batch, &geom, NULL, &layers, NULL));
    for (int64_t t = 0; t < n_tiles; ++t)
        if (pixels) CHECK(dswx_memcpy_d2h(ctx, wtr + (size_t)t * pixels, layers.wtr + t * geom.tile_stride, pixels));
    dswx_body_out_t host = carve(host_mem, nt, max_rows);
    if (!max_rows) host.rows = NULL;
    CHECK(dswx_body_table_host(label, wtr, &spec, n_tiles, size, size, 0, &host));

    int differ = 0;
    uint64_t bodies = 0, shoreline = 0, largest = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const uint32_t* lab = label + (size_t)t * pixels;
        const uint8_t* tile = wtr + (size_t)t * pixels;
        const uint32_t* dense = got.dense + (size_t)t * pixels;
        memset(mine, 0, 4 * RW * (max_rows + 1));
        uint64_t k = 0, members = 0, edges = 0;
        /* one pass in raster order: a root is the first pixel of its body, so its row exists when its pixels arrive */
        for (int64_t p = 0; p < (int64_t)pixels; ++p) {
            const uint32_t L = lab[p];
            if (!L) {
                differ += dense[p] != 0 || host.dense[(size_t)t * pixels + (size_t)p] != 0;
                continue;
            }
            if (L == (uint32_t)p + 1u) {
                uint32_t* r = mine + RW * k++;
                r[0] = L;
                r[2] = r[3] = (uint32_t)(p % size);
                r[4] = (uint32_t)(p / size);
            }
            /* the dense value of a pixel is that of its root, and the rows are in the order of the roots */
            const uint32_t d = dense[L - 1u];
            differ += dense[p] != d || host.dense[(size_t)t * pixels + (size_t)p] != d || d == 0 || d > k || mine[RW * (d - 1u)] != L;
            if (d == 0 || d > k) continue;
            uint32_t* r = mine + RW * (d - 1u);
            const int64_t y = p / size, x = p % size;
            const unsigned e = (x == 0 || lab[p - 1] != L) + (x == size - 1 || lab[p + 1] != L) + (y == 0 || lab[p - size] != L) +
                               (y == size - 1 || lab[p + size] != L);
            ++members;
            edges += e;
            r[1] += 1;
            if ((uint32_t)x < r[2]) r[2] = (uint32_t)x;
            if ((uint32_t)x > r[3]) r[3] = (uint32_t)x;
            r[5] = (uint32_t)y;
            const uint64_t per = word64(r, 6) + e, sx = word64(r, 8) + (uint64_t)x, sy = word64(r, 10) + (uint64_t)y;
            r[6] = (uint32_t)per, r[7] = (uint32_t)(per >> 32);
            r[8] = (uint32_t)sx, r[9] = (uint32_t)(sx >> 32);
            r[10] = (uint32_t)sy, r[11] = (uint32_t)(sy >> 32);
            if (tile[p] == 1) r[12] += 1;
            if (tile[p] == 2) r[13] += 1;
        }
        const uint64_t head[HW] = {k, k, members, 0, edges, 0, 0, 0};
        for (int w = 0; w < HW; ++w)
            if (got.head[(size_t)t * HW + w] != head[w] || host.head[(size_t)t * HW + w] != head[w]) {
                fprintf(stderr, "tile %" PRId64 " head word %d: loop %" PRIu64 ", device %" PRIu64 ", dswx_body_table_host %" PRIu64 "\n", t, w,
                        head[w], got.head[(size_t)t * HW + w], host.head[(size_t)t * HW + w]);
                ++differ;
            }
        if (k != summary[(size_t)t * DSWX_LABEL_SUMMARY_WORDS] || members != summary[(size_t)t * DSWX_LABEL_SUMMARY_WORDS + 1]) ++differ;
        for (size_t j = 0; j < max_rows; ++j)
            for (int w = 0; w < RW; ++w) {
                const uint32_t want = mine[RW * j + w];
                const size_t i = ((size_t)t * max_rows + j) * RW + (size_t)w;
                if ((got.rows[i] != want || host.rows[i] != want) && differ++ < 10)
                    fprintf(stderr, "tile %" PRId64 " row %zu word %d: loop %u, device %u, dswx_body_table_host %u\n", t, j, w, want, got.rows[i],
                            host.rows[i]);
            }
        for (size_t j = 0; j < (size_t)k; ++j)
            if (mine[RW * j + 1] > largest) largest = mine[RW * j + 1];
        bodies += k;
        shoreline += edges;
    }
    printf("%" PRId64 " tiles of %" PRId64 " x %" PRId64 " pixels: %" PRIu64 " water bodies in tables of %zu rows, %" PRIu64
           " shoreline edges, the largest body %" PRIu64 " pixels\n", n_tiles, size, size, bodies, max_rows, shoreline, largest);
    printf("%s\n", differ ? "MISMATCH" : "wtr bodies: device, loop and host entry agree in every row");
    free(mine);
    free(label);
    free(wtr);
    free(host_mem);
    free(got_mem);
    free(summary);
    CHECK(dswx_device_free(ctx, dev));
    CHECK(dswx_device_free(ctx, ldev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
