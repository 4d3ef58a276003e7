/*
 * batch_compare.c -- where two resident batches differ, from plain C (DSWX_HAS_COMPARE, additive to ABI v7): two small
 * batches are generated from the same seed and classified in HBM with different thresholds, dswx_batch_compare compares all
 * seven layers of every tile with one kernel launch (32 bytes per tile and layer cross PCIe), and one layer is downloaded
 * from both batches and compared again on the host with dswx_compare_host -- the other half of such a comparison.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_compare.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_compare && ./batch_compare [n_tiles] [size]
 *
 * Exit status 0: the device's and the host's records agree; 1: they differ, or a call failed.
 * tests/test_compare.py builds it with gcc, tests/test_gpu_compare.py runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_COMPARE
#error "this header has no compare entries"
#endif

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

int main(int argc, char** argv) {
    const int64_t n_tiles = argc > 1 ? atoll(argv[1]) : 3;
    const int64_t size = argc > 2 ? atoll(argv[2]) : 301;
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

    /* the seven layers of the default batch, in ascending plane index: the order of the rows of `rec` */
    static const struct { const char* name; int plane; } layers[7] = {
        {"diag", DSWX_PLANE_DIAG}, {"wtr1", DSWX_PLANE_WTR1}, {"wtr2", DSWX_PLANE_WTR2}, {"wtr", DSWX_PLANE_WTR},
        {"bwtr", DSWX_PLANE_BWTR}, {"conf", DSWX_PLANE_CONF}, {"cloud", DSWX_PLANE_CLOUD}};
    uint32_t mask = 0;
    for (int k = 0; k < 7; ++k) mask |= 1u << layers[k].plane;
    dswx_compare_t* rec = malloc(7 * (size_t)(n_tiles ? n_tiles : 1) * sizeof *rec);
    if (!rec) return 1;
    /* same stream as the classifications (NULL = the context's): ordered behind them, complete on return */
    CHECK(dswx_batch_compare(a, b, mask, 0, DSWX_BATCH_ALL_TILES, 0.0, 0.0, 1, rec, NULL));
    for (int k = 0; k < 7; ++k)
        for (int64_t t = 0; t < n_tiles; ++t)
            printf("compare %s %" PRId64 " n_diff %" PRId64 " first %" PRId64 " max %g\n", layers[k].name, t,
                   rec[k * n_tiles + t].n_diff, rec[k * n_tiles + t].first, rec[k * n_tiles + t].max_abs_diff);

    /* the other half: DIAG of both batches on the host */
    dswx_planes_out_t out_a, out_b;
    CHECK(dswx_batch_planes(a, &geom_a, NULL, &out_a, NULL));
    CHECK(dswx_batch_planes(b, &geom_b, NULL, &out_b, NULL));
    const size_t tile_bytes = (size_t)size * (size_t)size * sizeof(uint16_t);
    uint16_t* host_a = malloc(tile_bytes ? tile_bytes : 1);
    uint16_t* host_b = malloc(tile_bytes ? tile_bytes : 1);
    if (!host_a || !host_b) return 1;
    int differ = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        CHECK(dswx_memcpy_d2h(ctx, host_a, out_a.diag + t * geom_a.tile_stride, tile_bytes));
        CHECK(dswx_memcpy_d2h(ctx, host_b, out_b.diag + t * geom_b.tile_stride, tile_bytes));
        dswx_compare_t expect;
        CHECK(dswx_compare_host(host_a, host_b, DSWX_CMP_U16, size * size, 0.0, 0.0, 1, &expect));
        const dswx_compare_t* got = &rec[0 * n_tiles + t];
        if (expect.n_diff != got->n_diff || expect.first != got->first || expect.max_abs_diff != got->max_abs_diff) {
            fprintf(stderr, "diag tile %" PRId64 ": device n_diff %" PRId64 " first %" PRId64 ", host n_diff %" PRId64 " first %" PRId64 "\n",
                    t, got->n_diff, got->first, expect.n_diff, expect.first);
            differ = 1;
        }
    }
    printf("%s\n", differ ? "MISMATCH" : "diag: device and host records agree");
    free(host_a);
    free(host_b);
    free(rec);
    CHECK(dswx_batch_destroy(a));
    CHECK(dswx_batch_destroy(b));
    CHECK(dswx_ctx_destroy(ctx));
    return differ;
}
