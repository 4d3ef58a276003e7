// dswx_batch_select.h -- what a resident-batch entry (dswx_batch_checksum ... dswx_batch_burn, dswx_batch.hip) may be
// asked for: which tiles, which planes, and where tile `tile0` of a plane begins.  Plain host functions over a plain view of
// a batch, no HIP call and nothing dereferenced, so that tests/native/batch_select_host.cpp drives them without a device.
// Of dswx_host.h they take DSWX_PLANES and dswx_fail.
//
// The house order of refusals of a batch entry: "batch is NULL"; the plane index or the plane mask (and what the entry says
// of the counters); for one uint8 plane its width and its presence; two batches compatible; the feature's own check of
// tolerances / kinds / specs where it takes none of the batch's addresses; the tile range; the presence of masked planes; the
// feature's check of the addresses; "out is NULL" only for a selection that is not empty.
#pragma once

#include <cstdint>
#include <initializer_list>

#include "dswx_host.h"

struct dswx_batch_view {
    int64_t n_tiles, height, width, tile_stride;      // resident tiles; pixels between the tiles of a plane
    int device;
    void* const* ptr;                                 // [DSWX_BATCH_MAX_PLANES], NULL = the batch has no such plane
};

// Resolves DSWX_BATCH_ALL_TILES (against the first view) and refuses a range that leaves any view; `noun`: "the batch" / "a
// batch".  No sum of caller's numbers is formed: nothing overflows.
static inline int dswx_select_tiles(std::initializer_list<const dswx_batch_view*> views, int64_t tile0, int64_t* n_tiles,
                                    const char* noun) {
    const int64_t first = (*views.begin())->n_tiles;
    if (*n_tiles == DSWX_BATCH_ALL_TILES && tile0 >= 0 && tile0 <= first) *n_tiles = first - tile0;
    for (const dswx_batch_view* v : views)
        if (tile0 < 0 || *n_tiles < 0 || tile0 > v->n_tiles || *n_tiles > v->n_tiles - tile0)
            return dswx_fail(DSWX_ERR_ARG, "tiles %lld .. +%lld outside %s (%lld resident)", (long long)tile0, (long long)*n_tiles,
                             noun, (long long)v->n_tiles);
    return DSWX_OK;
}

// Where tile `tile0` of plane `k` begins: tile_stride pixels of the plane's width apart, the counters three int64 apart.
// Formed as an integer: an entry may ask before it has looked at tile0.
static inline char* dswx_select_base(const dswx_batch_view& v, int k, int64_t tile0) {
    const uint64_t step = k == DSWX_PLANE_COUNTERS ? DSWX_N_COUNTERS * sizeof(int64_t) : (uint64_t)v.tile_stride * DSWX_PLANES[k].bytes;
    return reinterpret_cast<char*>(reinterpret_cast<uintptr_t>(v.ptr[k]) + (uint64_t)tile0 * step);
}

// ONE uint8 plane by its index, `lowest` .. DSWX_BATCH_MAX_PLANES - 1 (lowest -1: "no plane" is allowed, *base = NULL):
// not the counters (`no_counters`, e.g. "the counters are not stacked"), one byte per pixel (`what`, e.g. "a stack is a uint8
// plane"), present in the batch -> *base = tile `tile0` of it.
static inline int dswx_select_u8_plane(const dswx_batch_view& v, int plane, int lowest, const char* no_counters, const char* what,
                                       int64_t tile0, const uint8_t** base) {
    if (plane < lowest || plane >= DSWX_BATCH_MAX_PLANES)
        return dswx_fail(DSWX_ERR_ARG, "plane %d: not %d .. %d", plane, lowest, DSWX_BATCH_MAX_PLANES - 1);
    if (plane == DSWX_PLANE_COUNTERS)
        return dswx_fail(DSWX_ERR_ARG, "%s (three int64 per tile): read them (dswx_batch_planes)", no_counters);
    *base = nullptr;
    if (plane < 0) return DSWX_OK;
    const dswx_plane_desc& d = DSWX_PLANES[plane];
    if (d.bytes != 1) return dswx_fail(DSWX_ERR_ARG, "%s, plane %d (%s) has %d bytes per pixel", what, plane, d.name, d.bytes);
    if (!v.ptr[plane]) return dswx_fail(DSWX_ERR_ARG, "the batch has no plane %d (%s)", plane, d.name);
    *base = reinterpret_cast<const uint8_t*>(dswx_select_base(v, plane, tile0));
    return DSWX_OK;
}

// A plane mask: no bit past the table, and -- with `no_counters`, the entry's whole sentence -- not the counters.
static inline int dswx_select_mask(uint32_t plane_mask, const char* no_counters) {
    if (plane_mask >> DSWX_BATCH_MAX_PLANES)
        return dswx_fail(DSWX_ERR_ARG, "plane_mask 0x%x names planes past %d", plane_mask, DSWX_BATCH_MAX_PLANES - 1);
    if (no_counters && ((plane_mask >> DSWX_PLANE_COUNTERS) & 1u)) return dswx_fail(DSWX_ERR_ARG, "%s", no_counters);
    return DSWX_OK;
}

// step(k) for every plane of a checked mask, in rising order; a plane that `a` -- or `b`, when there are two batches -- does
// not have ends the walk.
template <typename Step>
static inline int dswx_select_walk(uint32_t plane_mask, const dswx_batch_view& a, const dswx_batch_view* b, Step step) {
    for (int k = 0; k < DSWX_BATCH_MAX_PLANES; ++k) {
        if (!((plane_mask >> k) & 1u)) continue;
        const char* name = k == DSWX_PLANE_COUNTERS ? "counters" : DSWX_PLANES[k].name;
        if (!b && !a.ptr[k]) return dswx_fail(DSWX_ERR_ARG, "the batch has no plane %d (%s)", k, name);
        if (b && (!a.ptr[k] || !b->ptr[k]))
            return dswx_fail(DSWX_ERR_ARG, "batch %s has no plane %d (%s)", !a.ptr[k] ? (!b->ptr[k] ? "a (nor b)" : "a") : "b", k, name);
        step(k);
    }
    return DSWX_OK;
}

// Two batches whose planes one launch reads side by side: one device, one tile size (the strides may differ).
static inline int dswx_select_compatible(const dswx_batch_view& a, const dswx_batch_view& b) {
    if (a.device != b.device) return dswx_fail(DSWX_ERR_ARG, "the batches are on different devices (%d and %d)", a.device, b.device);
    if (a.height != b.height || a.width != b.width)
        return dswx_fail(DSWX_ERR_ARG, "the batches differ in tile size: %lld x %lld against %lld x %lld", (long long)a.height,
                         (long long)a.width, (long long)b.height, (long long)b.width);
    return DSWX_OK;
}
