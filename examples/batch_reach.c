/*
 * batch_reach.c -- a ring burnt and BUFFERED into the OCEAN plane of a resident batch, from plain C (DSWX_HAS_REACH): a small
 * batch with masks is allocated and generated in HBM, its OCEAN plane set to 0, dswx_batch_burn sets the inside of a ring to 1
 * and dswx_batch_reach every pixel whose centre lies within a radius of one of its edges -- the polygon grown by the radius, what
 * the reference makes with Buffer(margin) in front of the rasteriser --, in place, 16 bytes per vertex crossing PCIe instead of
 * the plane.  The plane and the head of the reach are downloaded and checked against this file's own loop over every pixel and
 * edge with the predicates of include/dswx_hip.h ("burn", "reach").
 *
 *   gcc -std=c11 -O2 -I include examples/batch_reach.c -L proteus_amd/_lib -ldswx_hip \
 *       -Wl,-rpath,$PWD/proteus_amd/_lib -o batch_reach && ./batch_reach [n_tiles] [size]
 *
 * Exit status 0: the device's plane and head and the loop's agree in every byte -- or there is no device, which is said;
 * 1: they differ, or a call failed.  tests/test_gpu_reach.py builds it with gcc and runs it on the GPU.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dswx_hip.h"

#ifndef DSWX_HAS_REACH
#error "this header has no reach entries"
#endif

#define WORDS DSWX_REACH_HEAD_WORDS
#define PER_TILE 5
#define RADIUS (5 * 256 + 77)                                /* 1/256 pixel */

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc__ = (call);                                                                 \
        if (rc__ != DSWX_OK) {                                                             \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, dswx_last_error());       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

typedef __int128 wide;

/* the records of tile t: a ring that leaves the tile on the right */
static void ring_of_tile(int64_t t, int64_t size, dswx_burn_vertex_t* v) {
    const int32_t s = (int32_t)(256 * size), q = s / 4, d = (int32_t)(37 * t);
    const int32_t pts[PER_TILE][2] = {{q + d, q + 128}, {s + 900, q / 2}, {3 * q + 128, 2 * q + d}, {s - 640, 3 * q + 128}, {q / 2, 3 * q - d}};
    for (int i = 0; i < PER_TILE; ++i) {
        v[i].x = pts[i][0], v[i].y = pts[i][1];
        v[i].word = 1u;
        v[i].next = (uint32_t)((i + 1) % PER_TILE);
    }
}

/* "reach": is the point within RADIUS of the closed segment a -> b, in exact integers */
static int reached(const dswx_burn_vertex_t* a, const dswx_burn_vertex_t* b, int64_t px, int64_t py) {
    const wide R2 = (wide)RADIUS * RADIUS, dx = (wide)b->x - a->x, dy = (wide)b->y - a->y, ux = px - a->x, uy = py - a->y;
    const wide D = dx * dx + dy * dy, t = ux * dx + uy * dy;
    if (D == 0 || t <= 0) return ux * ux + uy * uy <= R2;
    if (t >= D) return (ux - dx) * (ux - dx) + (uy - dy) * (uy - dy) <= R2;
    const wide cr = ux * dy - uy * dx;
    return cr * cr <= R2 * D;                                /* (coordinates of a few thousand pixels: far below 2^127) */
}

/* "burn": does the edge a -> b cross the row of the point at or to the left of it */
static int crosses(const dswx_burn_vertex_t* a, const dswx_burn_vertex_t* b, int64_t px, int64_t py) {
    int64_t x0 = a->x, y0 = a->y, x1 = b->x, y1 = b->y;
    if (y0 == y1) return 0;
    if (y0 > y1) {
        int64_t k = x0; x0 = x1, x1 = k;
        k = y0, y0 = y1, y1 = k;
    }
    return y0 <= py && py < y1 && (x1 - x0) * (py - y0) <= (px - x0) * (y1 - y0);
}

/* the two definitions per pixel and per edge: the plane becomes 1 where the centre is inside or reached; the head of the reach */
static void buffer_tile(const dswx_burn_vertex_t* v, int64_t size, uint8_t* plane, uint64_t* head) {
    memset(head, 0, WORDS * 8);
    head[0] = PER_TILE;
    for (int i = 0; i < PER_TILE; ++i) {
        const dswx_burn_vertex_t *a = v + i, *b = v + v[i].next;
        int any = 0;
        for (int64_t r = 0; r < size; ++r) {
            int row = 0;
            for (int64_t c = 0; c < size && !row; ++c) row = reached(a, b, 256 * c + 128, 256 * r + 128);
            if (!row) continue;
            any = 1;
            ++head[3];
            head[4] += (uint64_t)reached(a, b, -128, 256 * r + 128);
            head[5] += (uint64_t)reached(a, b, 256 * size + 128, 256 * r + 128);
        }
        head[2] += (uint64_t)any;
    }
    for (int64_t r = 0; r < size; ++r)
        for (int64_t c = 0; c < size; ++c) {
            int inside = 0, near = 0;
            for (int i = 0; i < PER_TILE; ++i) {
                inside ^= crosses(v + i, v + v[i].next, 256 * c + 128, 256 * r + 128);
                near |= reached(v + i, v + v[i].next, 256 * c + 128, 256 * r + 128);
            }
            head[6] += (uint64_t)near;
            if (inside || near) plane[r * size + c] = 1;
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
        printf("no device: nothing reached (there is no CPU fallback; dswx_reach_host is the other half of a comparison)\n");
        return 0;
    }
    dswx_ctx_t* ctx = NULL;
    CHECK(dswx_ctx_create(0, &ctx));

    dswx_batch_geom_t geom = {n_tiles, size, size, 0};
    dswx_batch_t* batch = NULL;
    CHECK(dswx_batch_create(ctx, &geom, DSWX_BATCH_MASKS, &batch));
    CHECK(dswx_batch_synth(batch, 20261021u, 0, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));            /* the generator wrote the masks too */
    dswx_planes_in_t in;
    CHECK(dswx_batch_planes(batch, &geom, &in, NULL, NULL));
    const size_t pixels = (size_t)size * (size_t)size, nt = (size_t)n_tiles;
    CHECK(dswx_memset_d(ctx, (void*)(uintptr_t)in.ocean, 0, nt * (size_t)geom.tile_stride));

    /* the records of all tiles, the table, acc and head side by side in one allocation: 16-, 8-, 8- and 4-byte aligned */
    const size_t v_bytes = nt * PER_TILE * sizeof(dswx_burn_vertex_t), f_bytes = (nt + 1) * 8, h_bytes = nt * WORDS * 8;
    dswx_burn_vertex_t* verts = malloc(v_bytes);
    int64_t* first = malloc(f_bytes);
    if (!verts || !first) return 1;
    for (int64_t t = 0; t < n_tiles; ++t) {
        ring_of_tile(t, size, verts + t * PER_TILE);
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

    /* one stream (NULL = the context's): the reach is ordered behind the burn, and both use the same working array */
    dswx_burn_spec_t burn = {1, 0, 0, 0};
    dswx_reach_spec_t reach = {1, 0, 0, 0, RADIUS, 0};
    CHECK(dswx_batch_burn(batch, DSWX_PLANE_OCEAN, d_verts, d_first, &burn, d_acc, NULL, 0, DSWX_BATCH_ALL_TILES, NULL));
    CHECK(dswx_batch_reach(batch, DSWX_PLANE_OCEAN, d_verts, d_first, &reach, d_acc, d_head, 0, DSWX_BATCH_ALL_TILES, NULL));
    CHECK(dswx_stream_synchronize(ctx, NULL));

    uint8_t* got = malloc(pixels + 1);
    uint8_t* want = malloc(pixels + 1);
    uint64_t* got_head = malloc(h_bytes);
    if (!got || !want || !got_head) return 1;
    CHECK(dswx_memcpy_d2h(ctx, got_head, d_head, h_bytes));
    int differ = 0;
    uint64_t set = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        uint64_t head[WORDS];
        memset(want, 0, pixels);
        buffer_tile(verts + t * PER_TILE, size, want, head);
        CHECK(dswx_memcpy_d2h(ctx, got, in.ocean + t * geom.tile_stride, pixels));
        for (size_t p = 0; p < pixels; ++p) {
            set += want[p];
            if (got[p] != want[p]) {
                if (differ < 10) fprintf(stderr, "tile %" PRId64 " pixel %zu: loop %u, device %u\n", t, p, want[p], got[p]);
                ++differ;
            }
        }
        for (int w = 0; w < WORDS; ++w)
            if (got_head[(size_t)t * WORDS + w] != head[w]) {
                fprintf(stderr, "tile %" PRId64 " head word %d: loop %" PRIu64 ", device %" PRIu64 "\n", t, w, head[w], got_head[(size_t)t * WORDS + w]);
                ++differ;
            }
    }
    printf("%" PRId64 " tiles of %" PRId64 " x %" PRId64 " pixels: %" PRIu64 " pixels inside the ring of %d records a tile or within %.2f pixels of it\n",
           n_tiles, size, size, set, PER_TILE, RADIUS / 256.0);
    if (!differ) printf("reach: device and loop agree in every pixel and every head word\n");
    else fprintf(stderr, "reach: %d differences\n", differ);

    free(got);
    free(want);
    free(got_head);
    free(verts);
    free(first);
    CHECK(dswx_device_free(ctx, dev));
    CHECK(dswx_batch_destroy(batch));
    CHECK(dswx_ctx_destroy(ctx));
    return differ ? 1 : 0;
}
