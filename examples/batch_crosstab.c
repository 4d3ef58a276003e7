/*
 * batch_crosstab.c -- how the classes of one resident batch fall into the classes of another, from plain C
 * (DSWX_HAS_CROSSTAB, additive to ABI v7): two small batches are generated from the same seed and classified in HBM with two
 * parameter sets, dswx_batch_crosstab counts WTR of the first against WTR of the second with one kernel launch -- 2 KiB per
 * tile cross PCIe -- and both layers are downloaded and counted again, by a loop and by dswx_crosstab_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_crosstab.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_crosstab && ./batch_crosstab [n_tiles] [size]
 *
 * Exit status 0: the device's table, the loop's and the host entry's agree in every cell; 1: they differ, or a call failed.
 * tests/test_crosstab.py builds it with gcc, tests/test_gpu_crosstab.py runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_CROSSTAB
#error "this header has no crosstab entries"
#endif

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

/* the classes of the interpreted layers: eight rows and eight columns (col_bits 3), any other byte in class 7 */
#define N_CLASSES 8
static const int wtr_values[7] = {0, 1, 2, 252, 253, 254, 255};
static const char* const wtr_names[N_CLASSES] = {"not water", "open water", "partial", "snow", "cloud", "ocean", "fill", "other"};

int main(int argc, char** argv) {
    const int64_t n_tiles = argc > 1 ? atoll(argv[1]) : 3;
    const int64_t size = argc > 2 ? atoll(argv[2]) : 301;
    if (dswx_abi_version() != DSWX_ABI_VERSION) {
        fprintf(stderr, "header / library ABI mismatch: %d vs %d\n", DSWX_ABI_VERSION, dswx_abi_version());
        return 1;
    }
    dswx_ctx_t* ctx = NULL;
    CHECK(dswx_ctx_create(0, &ctx));               /* DSWX_ERR_NO_DEVICE without an MI355X: there is no CPU fallback */
    dswx_params_t params_a, params_b;
    CHECK(dswx_params_default(&params_a));
    CHECK(dswx_params_default(&params_b));
    params_b.wigt = 0.2;                           /* two of the five tests move: some pixels change class */
    params_b.pswt_1_nir = 1400.0;

    /* batch a with the default padded stride, batch b with contiguous tiles: the strides may differ */
    dswx_batch_geom_t geom_a = {n_tiles, size, size, 0}, geom_b = {n_tiles, size, size, size * size};
    dswx_batch_t *a = NULL, *b = NULL;
    CHECK(dswx_batch_create(ctx, &geom_a, 0, &a));
    CHECK(dswx_batch_create(ctx, &geom_b, 0, &b));
    CHECK(dswx_batch_synth(a, 20251010u, 0, NULL));
    CHECK(dswx_batch_synth(b, 20251010u, 0, NULL));
    CHECK(dswx_batch_classify(a, &params_a, DSWX_BATCH_ALL_TILES, NULL));
    CHECK(dswx_batch_classify(b, &params_b, DSWX_BATCH_ALL_TILES, NULL));

    static dswx_crosstab_pair_t pair;              /* (static: zeroed) */
    pair.plane_a = DSWX_PLANE_WTR;
    pair.plane_b = DSWX_PLANE_WTR;
    pair.spec.a_kind = DSWX_HIST_U8;
    pair.spec.col_bits = 3;
    memset(pair.spec.row_of_bin, N_CLASSES - 1, sizeof pair.spec.row_of_bin);
    memset(pair.spec.col_of_byte, N_CLASSES - 1, sizeof pair.spec.col_of_byte);
    for (int k = 0; k < 7; ++k) pair.spec.row_of_bin[wtr_values[k]] = pair.spec.col_of_byte[wtr_values[k]] = (uint8_t)k;

    uint64_t* cells = malloc(((size_t)n_tiles * DSWX_CROSSTAB_CELLS + 1) * sizeof *cells);
    if (!cells) return 1;
    /* same stream as the classifications (NULL = the context's): ordered behind them, complete on return */
    CHECK(dswx_batch_crosstab(a, b, &pair, 1, 0, DSWX_BATCH_ALL_TILES, cells, NULL));

    /* the other half: WTR of both batches on the host, counted by a loop and by dswx_crosstab_host */
    dswx_planes_out_t out_a, out_b;
    CHECK(dswx_batch_planes(a, &geom_a, NULL, &out_a, NULL));
    CHECK(dswx_batch_planes(b, &geom_b, NULL, &out_b, NULL));
    const uint64_t pixels = (uint64_t)size * (uint64_t)size;
    uint8_t* host_a = malloc(pixels ? pixels : 1);
    uint8_t* host_b = malloc(pixels ? pixels : 1);
    if (!host_a || !host_b) return 1;
    int differ = 0;
    uint64_t total[DSWX_CROSSTAB_CELLS];
    memset(total, 0, sizeof total);
    for (int64_t t = 0; t < n_tiles; ++t) {
        uint64_t loop[DSWX_CROSSTAB_CELLS], entry[DSWX_CROSSTAB_CELLS];
        CHECK(dswx_memcpy_d2h(ctx, host_a, out_a.wtr + t * geom_a.tile_stride, pixels));
        CHECK(dswx_memcpy_d2h(ctx, host_b, out_b.wtr + t * geom_b.tile_stride, pixels));
        memset(loop, 0, sizeof loop);
        for (uint64_t i = 0; i < pixels; ++i)
            ++loop[pair.spec.row_of_bin[host_a[i]] * N_CLASSES + pair.spec.col_of_byte[host_b[i]]];
        CHECK(dswx_crosstab_host(host_a, host_b, &pair.spec, (int64_t)pixels, entry));
        printf("tile %" PRId64 ": wtr x wtr cells", t);
        for (int c = 0; c < DSWX_CROSSTAB_CELLS; ++c) {
            const uint64_t dev = cells[t * DSWX_CROSSTAB_CELLS + c];
            total[c] += dev;
            if (dev) printf(" %d,%d:%" PRIu64, c / N_CLASSES, c % N_CLASSES, dev);
            if (dev != loop[c] || dev != entry[c]) {
                fprintf(stderr, "tile %" PRId64 " cell %d: device %" PRIu64 ", loop %" PRIu64 ", dswx_crosstab_host %" PRIu64 "\n", t,
                        c, dev, loop[c], entry[c]);
                differ = 1;
            }
        }
        printf("\n");
    }

    /* the table of the whole batch: rows the first parameter set, columns the second */
    printf("%-12s", "a \\ b");
    for (int c = 0; c < N_CLASSES; ++c) printf(" %11s", wtr_names[c]);
    printf("\n");
    for (int r = 0; r < N_CLASSES; ++r) {
        printf("%-12s", wtr_names[r]);
        for (int c = 0; c < N_CLASSES; ++c) printf(" %11" PRIu64, total[r * N_CLASSES + c]);
        printf("\n");
    }
    printf("%s\n", differ ? "MISMATCH" : "wtr x wtr: device, loop and host entry agree in every cell");
    free(host_a);
    free(host_b);
    free(cells);
    CHECK(dswx_batch_destroy(a));
    CHECK(dswx_batch_destroy(b));
    CHECK(dswx_ctx_destroy(ctx));
    return differ;
}
