/*
 * batch_warp.c -- the WTR layer of a resident batch resampled onto another lattice through a coordinate mesh, from plain C
 * (DSWX_HAS_WARP): a batch of three tiles is allocated, generated and classified in HBM; a mesh is computed here, in C, for a
 * shift by `shift` pixels plus a rotation of two degrees about the middle of the tile -- what a neighbouring UTM zone looks
 * like from this one -- and written to device memory, and dswx_batch_warp picks for every destination pixel the nearest
 * source pixel with one kernel launch.  The device sees the integers of the mesh and never the rotation.  The outputs stay in
 * device memory; here they are downloaded, with the WTR layer, and checked against a loop in C over the downloaded layer
 * (the definition of include/dswx_hip.h, pixel by pixel) and against dswx_warp_host.
 *
 *   gcc -std=c11 -O2 -I include examples/batch_warp.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -lm -o batch_warp && ./batch_warp [size] [shift]
 *
 * Exit status 0: the device's outputs, the loop's and the host entry's agree in every pixel; 1: they differ, or a call failed.
 * tests/test_gpu_warp.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_WARP
#error "this header has no warp entries"
#endif

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

#define MESH_SHIFT 5                                  /* a node every 32 destination pixels */

int main(int argc, char** argv) {
    const int64_t size = argc > 1 ? atoll(argv[1]) : 301;
    const int64_t move = argc > 2 ? atoll(argv[2]) : 27;
    const int64_t n_tiles = 3;
    if (size < 1 || size > 30000) {
        fprintf(stderr, "usage: batch_warp [1 <= size <= 30000] [shift in pixels]\n");
        return 1;
    }
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

    /* the mesh: node (i, j) is where the centre of destination pixel (X, Y) = (32 j, 32 i) lies in the source, in 1/256 pixel
     * (source pixel (c, r) has its centre at (256 c + 128, 256 r + 128)); one mesh for the three tiles */
    const int64_t step = (int64_t)1 << MESH_SHIFT;
    const int64_t mesh_h = ((size + step - 1) >> MESH_SHIFT) + 1, mesh_w = mesh_h;
    const size_t mesh_bytes = (size_t)(mesh_h * mesh_w) * 2 * sizeof(int32_t);
    int32_t* mesh = malloc(mesh_bytes);
    if (!mesh) return 1;
    const double angle = 2.0 * 3.14159265358979323846 / 180.0, mid = 128.0 * (double)size;
    for (int64_t i = 0; i < mesh_h; ++i)
        for (int64_t j = 0; j < mesh_w; ++j) {
            const double x = 256.0 * (double)(j * step) + 128.0 - mid, y = 256.0 * (double)(i * step) + 128.0 - mid;
            mesh[2 * (i * mesh_w + j)] = (int32_t)llround(mid + cos(angle) * x - sin(angle) * y + 256.0 * (double)move);
            mesh[2 * (i * mesh_w + j) + 1] = (int32_t)llround(mid + sin(angle) * x + cos(angle) * y);
        }
    void* mesh_dev = NULL;
    CHECK(dswx_device_malloc(ctx, mesh_bytes, &mesh_dev));
    CHECK(dswx_memcpy_h2d(ctx, mesh_dev, mesh, mesh_bytes));

    dswx_warp_spec_t spec;
    memset(&spec, 0, sizeof spec);
    spec.elem_bytes = 1;                            /* the WTR layer is a byte plane; the batch entry checks that */
    spec.shift = MESH_SHIFT;
    spec.outside = 255;                             /* the product's fill */

    const size_t tile_pixels = (size_t)size * (size_t)size, pixels = tile_pixels * (size_t)n_tiles;
    const size_t head_bytes = (size_t)n_tiles * DSWX_WARP_HEAD_WORDS * sizeof(uint64_t);
    void *dst_dev = NULL, *index_dev = NULL, *head_dev = NULL;
    CHECK(dswx_device_malloc(ctx, pixels, &dst_dev));
    CHECK(dswx_device_malloc(ctx, pixels * sizeof(uint32_t), &index_dev));
    CHECK(dswx_device_malloc(ctx, head_bytes, &head_dev));
    const dswx_warp_out_t dev_out = {dst_dev, index_dev, head_dev};
    /* same stream as the classification (NULL = the context's): ordered behind it; asynchronous */
    CHECK(dswx_batch_warp(batch, DSWX_PLANE_WTR, &spec, 0, DSWX_BATCH_ALL_TILES, mesh_dev, size, size, &dev_out, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));

    uint8_t* got = malloc(pixels);
    uint32_t* got_index = malloc(pixels * sizeof *got_index);
    uint64_t got_head[3 * DSWX_WARP_HEAD_WORDS], host_head[3 * DSWX_WARP_HEAD_WORDS];
    uint8_t* host = malloc(pixels);
    uint32_t* host_index = malloc(pixels * sizeof *host_index);
    uint8_t* wtr = malloc(pixels);
    if (!got || !got_index || !host || !host_index || !wtr) return 1;
    CHECK(dswx_memcpy_d2h(ctx, got, dst_dev, pixels));
    CHECK(dswx_memcpy_d2h(ctx, got_index, index_dev, pixels * sizeof *got_index));
    CHECK(dswx_memcpy_d2h(ctx, got_head, head_dev, head_bytes));

    /* the other half: the WTR layer on the host, tile after tile without the padding */
    dswx_planes_out_t layers;
    CHECK(dswx_batch_planes(batch, &geom, NULL, &layers, NULL));
    for (int64_t t = 0; t < n_tiles; ++t)
        CHECK(dswx_memcpy_d2h(ctx, wtr + (size_t)t * tile_pixels, layers.wtr + t * geom.tile_stride, tile_pixels));
    const dswx_warp_out_t host_out = {host, host_index, host_head};
    CHECK(dswx_warp_host(wtr, &spec, n_tiles, size, size, mesh, size, size, &host_out));

    /* the loop: the definition, pixel by pixel */
    int differ = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        uint64_t inside = 0;
        for (int64_t Y = 0; Y < size; ++Y)
            for (int64_t X = 0; X < size; ++X) {
                const int64_t i = Y >> MESH_SHIFT, fy = Y & (step - 1), j = X >> MESH_SHIFT, fx = X & (step - 1);
                int64_t pos[2];
                for (int k = 0; k < 2; ++k) {
                    const int64_t v00 = mesh[2 * (i * mesh_w + j) + k], v01 = mesh[2 * (i * mesh_w + j + 1) + k];
                    const int64_t v10 = mesh[2 * ((i + 1) * mesh_w + j) + k], v11 = mesh[2 * ((i + 1) * mesh_w + j + 1) + k];
                    const int64_t num = (step - fy) * ((step - fx) * v00 + fx * v01) + fy * ((step - fx) * v10 + fx * v11);
                    const int64_t rounded = num + ((int64_t)1 << (2 * MESH_SHIFT - 1));
                    /* floor division by 2^(2 shift) and then by 256, without shifting a negative number */
                    const int64_t d = (int64_t)1 << (2 * MESH_SHIFT + 8);
                    pos[k] = rounded >= 0 ? rounded / d : -((-rounded + d - 1) / d);
                }
                const int64_t c = pos[0], r = pos[1];
                const int in = c >= 0 && c < size && r >= 0 && r < size;
                const size_t e = (size_t)t * tile_pixels + (size_t)(Y * size + X);
                const uint8_t want = in ? wtr[(size_t)t * tile_pixels + (size_t)(r * size + c)] : 255;
                const uint32_t want_index = in ? (uint32_t)(r * size + c) : DSWX_WARP_OUTSIDE;
                inside += (uint64_t)in;
                const int ok = got[e] == want && host[e] == want && got_index[e] == want_index && host_index[e] == want_index;
                if (!ok && differ < 10)
                    fprintf(stderr, "tile %" PRId64 " pixel (%" PRId64 ", %" PRId64 "): loop %u %u, device %u %u, dswx_warp_host %u %u\n", t, X, Y,
                            want, want_index, got[e], got_index[e], host[e], host_index[e]);
                differ += !ok;
            }
        const uint64_t* g = got_head + t * DSWX_WARP_HEAD_WORDS;
        if (g[0] != tile_pixels || g[1] != inside || g[2] != tile_pixels - inside || g[7] != 0 ||
            memcmp(g, host_head + t * DSWX_WARP_HEAD_WORDS, DSWX_WARP_HEAD_WORDS * sizeof(uint64_t)) != 0) {
            fprintf(stderr, "tile %" PRId64 ": head %" PRIu64 " %" PRIu64 " %" PRIu64 ", the loop counted %" PRIu64 " inside\n", t, g[0], g[1], g[2], inside);
            differ += 1;
        }
        printf("tile %" PRId64 ": %" PRIu64 " of %zu pixels inside, source rows %" PRIu64 " .. %" PRIu64 ", columns %" PRIu64 " .. %" PRIu64 "\n", t, g[1],
               tile_pixels, g[3], g[4], g[5], g[6]);
    }
    printf("%s\n", differ ? "MISMATCH" : "wtr warp: device, loop and host entry agree in every pixel");
    free(wtr);
    free(host_index);
    free(host);
    free(got_index);
    free(got);
    free(mesh);
    CHECK(dswx_device_free(ctx, head_dev));
    CHECK(dswx_device_free(ctx, index_dev));
    CHECK(dswx_device_free(ctx, dst_dev));
    CHECK(dswx_device_free(ctx, mesh_dev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
