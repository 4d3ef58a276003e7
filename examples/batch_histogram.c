/*
 * batch_histogram.c -- how much of each class a resident batch holds, from plain C (DSWX_HAS_HISTOGRAM): a small batch is
 * allocated, generated and classified in HBM, dswx_batch_histogram returns the per-tile counts of the WTR layer (one bin per
 * class byte) and of the DIAG layer (one bin per pattern of the five tests) with one kernel launch -- 2 KiB per tile and
 * layer cross PCIe -- and the WTR layer is downloaded and counted again, by a loop and by dswx_histogram_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_histogram.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_histogram && ./batch_histogram [n_tiles] [size]
 *
 * Exit status 0: the device's counts, the loop's and the host entry's agree in every bin; 1: they differ, or a call failed.
 * tests/test_gpu_histogram.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_HISTOGRAM
#error "this header has no histogram entries"
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

    /* two layers, in ascending plane index: DIAG (10) is row 0 of `bins`, WTR (14) row 1 */
    const uint32_t mask = (1u << DSWX_PLANE_DIAG) | (1u << DSWX_PLANE_WTR);
    const size_t per_plane = (size_t)n_tiles * DSWX_HIST_BINS;
    uint64_t* bins = malloc((2 * per_plane + 1) * sizeof *bins);
    if (!bins) return 1;
    /* same stream as the classification (NULL = the context's): ordered behind it, complete on return; the band arguments
     * (lo, shift) matter for band planes only */
    CHECK(dswx_batch_histogram(batch, mask, 0, DSWX_BATCH_ALL_TILES, 0, 6, bins, NULL));
    const uint64_t* diag = bins;
    const uint64_t* wtr = bins + per_plane;
    const uint64_t pixels = (uint64_t)size * (uint64_t)size;
    int differ = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        uint64_t fired[5] = {0, 0, 0, 0, 0}, sum = 0;
        for (int p = 0; p < 32; ++p)
            for (int k = 0; k < 5; ++k)
                if (p >> k & 1) fired[k] += diag[t * DSWX_HIST_BINS + p];
        for (int b = 0; b < DSWX_HIST_BINS; ++b) sum += diag[t * DSWX_HIST_BINS + b];
        printf("tile %" PRId64 ": tests fired %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 ", nodata %" PRIu64
               ", not a pattern %" PRIu64 "\n", t, fired[0], fired[1], fired[2], fired[3], fired[4], diag[t * DSWX_HIST_BINS + 32],
               diag[t * DSWX_HIST_BINS + 33]);
        if (sum != pixels) {
            fprintf(stderr, "diag tile %" PRId64 ": the bins sum to %" PRIu64 ", not to %" PRIu64 " pixels\n", t, sum, pixels);
            differ = 1;
        }
        printf("tile %" PRId64 ": wtr classes", t);
        for (int b = 0; b < DSWX_HIST_BINS; ++b)
            if (wtr[t * DSWX_HIST_BINS + b]) printf(" %d:%" PRIu64, b, wtr[t * DSWX_HIST_BINS + b]);
        printf("\n");
    }

    /* the other half: WTR on the host, counted by a loop and by dswx_histogram_host */
    dswx_planes_out_t out;
    CHECK(dswx_batch_planes(batch, &geom, NULL, &out, NULL));
    uint8_t* host = malloc(pixels ? pixels : 1);
    if (!host) return 1;
    for (int64_t t = 0; t < n_tiles; ++t) {
        uint64_t loop[DSWX_HIST_BINS], entry[DSWX_HIST_BINS];
        CHECK(dswx_memcpy_d2h(ctx, host, out.wtr + t * geom.tile_stride, pixels));
        memset(loop, 0, sizeof loop);
        for (uint64_t i = 0; i < pixels; ++i) ++loop[host[i]];
        CHECK(dswx_histogram_host(host, DSWX_HIST_U8, 0, 0, (int64_t)pixels, entry));
        for (int b = 0; b < DSWX_HIST_BINS; ++b) {
            const uint64_t dev = wtr[t * DSWX_HIST_BINS + b];
            if (dev != loop[b] || dev != entry[b]) {
                fprintf(stderr, "wtr tile %" PRId64 " bin %d: device %" PRIu64 ", loop %" PRIu64 ", dswx_histogram_host %" PRIu64 "\n",
                        t, b, dev, loop[b], entry[b]);
                differ = 1;
            }
        }
    }
    printf("%s\n", differ ? "MISMATCH" : "wtr: device, loop and host entry agree in every bin");
    free(host);
    free(bins);
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ;
}
