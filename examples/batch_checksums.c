/*
 * batch_checksums.c -- what a resident batch contains, from plain C (ABI v7): a small batch is allocated, generated and
 * classified in HBM, dswx_batch_checksum returns the per-tile checksum of all seven layers with one kernel launch (eight
 * bytes per tile and layer cross PCIe), and one layer is downloaded and its checksums recomputed on the host with
 * dswx_checksum_host -- the way a caller confirms that a resident tile equals a host array or a decoded file.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_checksums.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_checksums && ./batch_checksums [n_tiles] [size]
 *
 * Exit status 0: the device's and the host's checksums agree; 1: they differ, or a call failed.
 * tests/test_checksum_example.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "dswx_hip.h"

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

    /* the seven layers of the default batch, in ascending plane index: the order of the rows of `sums` */
    static const struct { const char* name; int plane; int elem; } layers[7] = {
        {"diag", DSWX_PLANE_DIAG, 2}, {"wtr1", DSWX_PLANE_WTR1, 1}, {"wtr2", DSWX_PLANE_WTR2, 1}, {"wtr", DSWX_PLANE_WTR, 1},
        {"bwtr", DSWX_PLANE_BWTR, 1}, {"conf", DSWX_PLANE_CONF, 1}, {"cloud", DSWX_PLANE_CLOUD, 1}};
    uint32_t mask = 0;
    for (int k = 0; k < 7; ++k) mask |= 1u << layers[k].plane;
    uint64_t* sums = malloc(7 * (size_t)n_tiles * sizeof *sums);
    if (!sums) return 1;
    /* same stream as the classification (NULL = the context's): ordered behind it, complete on return */
    CHECK(dswx_batch_checksum(batch, mask, 0, DSWX_BATCH_ALL_TILES, sums, NULL));
    for (int k = 0; k < 7; ++k)
        for (int64_t t = 0; t < n_tiles; ++t)
            printf("checksum %s %" PRId64 " %016" PRIx64 "\n", layers[k].name, t, sums[k * n_tiles + t]);

    /* the other half of the comparison: DIAG on the host */
    dswx_planes_out_t out;
    CHECK(dswx_batch_planes(batch, &geom, NULL, &out, NULL));
    const size_t tile_bytes = (size_t)size * (size_t)size * sizeof(uint16_t);
    uint16_t* host = malloc(tile_bytes ? tile_bytes : 1);
    if (!host) return 1;
    int differ = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        CHECK(dswx_memcpy_d2h(ctx, host, out.diag + t * geom.tile_stride, tile_bytes));
        uint64_t expect = 0;
        CHECK(dswx_checksum_host(host, tile_bytes, &expect));
        if (expect != sums[0 * n_tiles + t]) {
            fprintf(stderr, "diag tile %" PRId64 ": device %016" PRIx64 ", host %016" PRIx64 "\n", t, sums[t], expect);
            differ = 1;
        }
    }
    printf("%s\n", differ ? "MISMATCH" : "diag: device and host checksums agree");
    free(host);
    free(sums);
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ;
}
