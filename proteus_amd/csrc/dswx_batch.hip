// dswx_batch.hip -- resident batches: the planes of a batch allocated by the library (dswx_batch_create) and
// the opt-in measured placement of the output planes (dswx_batch_place_search).  include/dswx_hip.h
// "resident batches" documents the C-ABI; DESIGN.md section 5 has the measurements.
//
// Why placement at all.  On MI355X the rate of the fused kernel follows where its seven WRITE streams lie in
// the address space (reads stream at 7 TB/s anywhere; moving the INPUT planes by 170 GiB changes nothing).
// Moving the packed output region of a 256-tile batch (25.5 GiB) through one large allocation, the same launch
// runs at 0.70 - 0.74 of the HBM peak in some ranges and at 0.79 - 0.80 in others, with a structure of about
// 32 GiB (profiles/r03_write_stream_map.json: reproducible between fresh processes of one box for arenas
// >= 150 GB, similar but not equal between boxes).  Round 3 tried to turn that into a layout RULE (a fixed gap,
// a fixed offset, alternating output and input planes, separate allocations in either order) and none holds
// from one fresh process to the next for an allocation of the batch's own size: the same rule gives 0.70 - 0.80
// (profiles/r03_placement_rule_trials.json).  So the placement stays a measurement -- but one the library
// makes, behind the C-ABI, in two forms: dswx_batch_place_slide (the output planes in a range of the virtual
// address space that is longer than they are and backed chunk by chunk: ~100 candidate placements inside it,
// the chunks under the best one kept, the rest returned) and dswx_batch_place_search (one hipMalloc per output
// plane, each bound to the fastest of a few spare allocations).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "dswx_batch_select.h"
#include "dswx_host.h"
#include "dswx_vmm.h"

using dswx_vmm::VaPool;
using dswx_vmm::VmRange;
using dswx_vmm::chunk_for;
using dswx_vmm::va_pool;

namespace {

constexpr uint64_t kAlign = 256;
inline uint64_t up256(uint64_t v) { return (v + (kAlign - 1)) & ~(kAlign - 1); }

struct PlaneSet {
    std::vector<int> in, out;    // plane indices present, in ABI order
};

PlaneSet planes_of(uint32_t flags) {
    PlaneSet s;
    for (int k = 0; k < 6; ++k) s.in.push_back(DSWX_PLANE_BAND0 + k);
    s.in.push_back(DSWX_PLANE_FMASK);
    if (flags & DSWX_BATCH_MASKS) {
        s.in.push_back(DSWX_PLANE_LAND);
        s.in.push_back(DSWX_PLANE_SHAD);
        s.in.push_back(DSWX_PLANE_OCEAN);
    }
    s.out.push_back(DSWX_PLANE_DIAG);
    s.out.push_back(DSWX_PLANE_WTR1);
    if (flags & DSWX_BATCH_WTR1_AEROSOL) s.out.push_back(DSWX_PLANE_WTR1_AEROSOL);
    s.out.push_back(DSWX_PLANE_WTR2);
    s.out.push_back(DSWX_PLANE_WTR);
    s.out.push_back(DSWX_PLANE_BWTR);
    s.out.push_back(DSWX_PLANE_CONF);
    s.out.push_back(DSWX_PLANE_CLOUD);
    if (flags & DSWX_BATCH_BROWSE) s.out.push_back(DSWX_PLANE_BROWSE);
    return s;
}

int layout_mode(uint32_t flags, uint32_t* mode) {
    *mode = flags & (DSWX_BATCH_SEPARATE_OUTPUTS | DSWX_BATCH_SLIDING_OUTPUTS);
    if (*mode == (DSWX_BATCH_SEPARATE_OUTPUTS | DSWX_BATCH_SLIDING_OUTPUTS))
        return dswx_fail(DSWX_ERR_ARG, "DSWX_BATCH_SEPARATE_OUTPUTS and DSWX_BATCH_SLIDING_OUTPUTS exclude each other");
    return DSWX_OK;
}

}  // namespace

struct dswx_batch {
    dswx_ctx* ctx = nullptr;
    int device = -1;                           // of ctx; kept here so that destroy works after the context is gone
    dswx_batch_geom_t geom = {};
    uint32_t flags = 0;                        // as laid out (a sliding batch that fell back: without the sliding bit)
    uint32_t requested_flags = 0;              // as asked for
    std::string note;                          // why a sliding batch was allocated packed / a placement did nothing
    dswx_batch_layout_t lay = {};
    void* arena = nullptr;
    void* own[DSWX_BATCH_MAX_PLANES] = {};     // SEPARATE_OUTPUTS: the allocation an output plane lives in
    void* ptr[DSWX_BATCH_MAX_PLANES] = {};     // device address of every plane
    VmRange* range = nullptr;                  // SLIDING_OUTPUTS: the range the output region lives in ...
    size_t region_offset = 0;                  // ... and where in it
    int search_candidates = 0, search_probes = 0;
    float first_ms = 0.f, kept_ms = 0.f;
};

static void set_note(dswx_batch* b, const std::string& text) { b->note = text; }

static void bind_structs(const dswx_batch* b, dswx_planes_in_t* in, dswx_planes_out_t* out) {
    if (in) memset(in, 0, sizeof *in);
    if (out) memset(out, 0, sizeof *out);
    for (const dswx_plane_desc& d : DSWX_PLANES)
        if (d.batch >= 0) dswx_plane_set(d, in, out, b->ptr[d.batch]);
}

// ---- The pieces of the entries that work on resident planes (dswx_batch_checksum ... dswx_batch_burn below); the rules
// themselves are in dswx_batch_select.h.
static dswx_batch_view view_of(const dswx_batch* b) {
    return {b->geom.n_tiles, b->geom.height, b->geom.width, b->geom.tile_stride, b->device, b->ptr};
}

// ONE uint8 plane of a batch and a tile range of it, for the entries that take a plane index: the batch, the plane
// (dswx_select_u8_plane), the range -> the view, the resolved n_tiles and tile `tile0` of the plane.
static int select_u8(const dswx_batch* b, int plane, int lowest, const char* no_counters, const char* what, int64_t tile0, int64_t* n_tiles,
                     dswx_batch_view* v, const uint8_t** base) {
    if (!b) return dswx_fail(DSWX_ERR_ARG, "batch is NULL");
    *v = view_of(b);
    if (int rc = dswx_select_u8_plane(*v, plane, lowest, no_counters, what, tile0, base)) return rc;
    return dswx_select_tiles({v}, tile0, n_tiles, "the batch");
}

// The tail of the entries that hand their result to the host: `bytes` of device memory of this call's own -- no scratch of the
// context, nothing to order against its other launches --, launch(dev, stream) fills them, they are copied to `out`, and the
// stream is waited for.
template <typename T, typename Launch>
static int read_back(dswx_ctx* ctx, void* stream, size_t bytes, T* out, const char* entry, const char* what, Launch launch) {
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    dswx_call_scratch scratch(dswx_stream_of(ctx, stream));
    T* dev = nullptr;
    HIP_TRY(scratch.take(&dev, bytes));
    if (int rc = launch(dev, scratch.s)) return rc;
    hipError_t e = hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, scratch.s);
    if (e == hipSuccess) e = scratch.sync();
    if (e != hipSuccess) return dswx_fail(DSWX_ERR_HIP, "%s: reading the %s failed: %s", entry, what, hipGetErrorString(e));
    return DSWX_OK;
}

extern "C" {

int dswx_batch_layout(const dswx_batch_geom_t* geom, uint32_t flags, dswx_batch_layout_t* out) {
    if (!geom || !out) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    if (geom->n_tiles < 0 || geom->height < 0 || geom->width < 0 || geom->tile_stride < 0)
        return dswx_fail(DSWX_ERR_ARG, "negative size");
    uint32_t mode;
    if (int rc = layout_mode(flags, &mode)) return rc;
    if (flags & ~(uint32_t)(DSWX_BATCH_MASKS | DSWX_BATCH_WTR1_AEROSOL | DSWX_BATCH_BROWSE | DSWX_BATCH_SEPARATE_OUTPUTS |
                           DSWX_BATCH_SLIDING_OUTPUTS))
        return dswx_fail(DSWX_ERR_ARG, "unknown batch flag in 0x%x", flags);
    if (geom->height > (1LL << 30) || geom->width > (1LL << 30) || geom->n_tiles > (1LL << 32) ||
        geom->tile_stride > (1LL << 46))
        return dswx_fail(DSWX_ERR_ARG, "batch geometry out of range");
    memset(out, 0, sizeof *out);
    const int64_t P = geom->height * geom->width;
    int64_t stride = geom->tile_stride ? geom->tile_stride : (P + 255) / 256 * 256;
    if (stride < P) return dswx_fail(DSWX_ERR_ARG, "tile_stride smaller than the tile");
    out->tile_stride = stride;
    if (geom->n_tiles && (uint64_t)stride > (1ull << 46) / (uint64_t)geom->n_tiles)          // 64 TiB of pixels: no overflow below
        return dswx_fail(DSWX_ERR_ARG, "batch too large");
    const uint64_t px = (uint64_t)geom->n_tiles * (uint64_t)stride;
    const PlaneSet ps = planes_of(flags);
    for (int k : ps.in) out->plane_bytes[k] = up256(px * DSWX_PLANES[k].bytes);
    for (int k : ps.out) out->plane_bytes[k] = up256(px * DSWX_PLANES[k].bytes);
    out->plane_bytes[DSWX_PLANE_COUNTERS] = up256((uint64_t)geom->n_tiles * DSWX_N_COUNTERS * sizeof(int64_t));

    uint64_t cur = 0;
    auto take = [&](int k) {
        out->plane_offset[k] = cur;
        cur += out->plane_bytes[k] ? out->plane_bytes[k] : kAlign;      // an empty batch still has distinct addresses
    };
    for (int k : ps.in) take(k);
    if (mode == 0)
        for (int k : ps.out) take(k);
    take(DSWX_PLANE_COUNTERS);
    out->arena_bytes = cur;
    if (mode == DSWX_BATCH_SLIDING_OUTPUTS) {       // offsets inside the output REGION, which lives in a range of its own
        cur = 0;
        for (int k : ps.out) take(k);
        out->write_span_bytes = cur;
    }
    if (mode == 0) {
        uint64_t lo = ~0ull, hi = 0;
        for (int k : ps.out) {
            lo = out->plane_offset[k] < lo ? out->plane_offset[k] : lo;
            const uint64_t end = out->plane_offset[k] + out->plane_bytes[k];
            hi = end > hi ? end : hi;
        }
        out->write_span_bytes = hi - lo;
    }
    return DSWX_OK;
}

int dswx_batch_destroy(dswx_batch_t* b) {
    if (!b) return DSWX_OK;
    if (b->device >= 0) (void)hipSetDevice(b->device);
    for (void* p : b->own)
        if (p) (void)hipFree(p);
    if (b->arena) (void)hipFree(b->arena);
    if (b->range) { b->range->destroy(); delete b->range; }
    delete b;
    return DSWX_OK;
}

int dswx_batch_create(dswx_ctx_t* ctx, const dswx_batch_geom_t* geom, uint32_t flags, dswx_batch_t** out) {
    if (!ctx || !geom || !out) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    *out = nullptr;
    dswx_batch_layout_t lay;
    if (int rc = dswx_batch_layout(geom, flags, &lay)) return rc;
    uint32_t mode;
    if (int rc = layout_mode(flags, &mode)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (mode == DSWX_BATCH_SLIDING_OUTPUTS) {
        int vmm = 0;
        if (hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported, ctx->device) != hipSuccess || !vmm)
            return dswx_fail(DSWX_ERR_UNSUPPORTED, "DSWX_BATCH_SLIDING_OUTPUTS needs HIP virtual memory management, which device "
                             "%d does not report; use DSWX_BATCH_SEPARATE_OUTPUTS + dswx_batch_place_search", ctx->device);
    }
    dswx_batch* b = new dswx_batch();
    b->ctx = ctx;
    b->device = ctx->device;
    b->geom = *geom;
    b->requested_flags = flags;
    hipError_t e = hipSuccess;
    if (mode == DSWX_BATCH_SLIDING_OUTPUTS) {
        // the range first: if the address space cannot be had (the reservation refused, or the library's budget of
        // retired addresses spent -- dswx_batch_va_budget), the batch is allocated PACKED instead, with the reason on
        // record: a long-lived service degrades to the first-come rate, it does not fail
        const size_t bytes = lay.write_span_bytes ? lay.write_span_bytes : kAlign;
        b->range = new VmRange();
        if (b->range->create(ctx->device, bytes, chunk_for(bytes)) != hipSuccess) {
            (void)hipGetLastError();
            set_note(b, "DSWX_BATCH_SLIDING_OUTPUTS not honoured, planes packed in one allocation: " + b->range->why);
            delete b->range;
            b->range = nullptr;
            flags &= ~(uint32_t)DSWX_BATCH_SLIDING_OUTPUTS;
            mode = 0;
            if (int rc = dswx_batch_layout(geom, flags, &lay)) { delete b; return rc; }
        }
    }
    b->geom.tile_stride = lay.tile_stride;
    b->flags = flags;
    b->lay = lay;
    e = dswx_locked_malloc(&b->arena, lay.arena_bytes);
    const PlaneSet ps = planes_of(flags);
    if (e == hipSuccess && mode == DSWX_BATCH_SEPARATE_OUTPUTS)
        for (int k : ps.out) {
            e = dswx_locked_malloc(&b->own[k], lay.plane_bytes[k] ? lay.plane_bytes[k] : kAlign);
            if (e != hipSuccess) break;
        }
    if (e != hipSuccess) {
        dswx_batch_destroy(b);
        (void)hipGetLastError();
        uint64_t pooled = 0;
        dswx_vmm::account(0, nullptr, nullptr, nullptr, nullptr, &pooled);
        // (the library does not trim by itself: dswx_batch_pool_trim has a window in which other threads must not allocate)
        return dswx_fail(DSWX_ERR_HIP, "dswx_batch_create: device allocation failed: %s (arena of %llu bytes; the library's pool of "
                         "placement chunks holds %llu bytes that dswx_batch_pool_trim() returns to the device)",
                         hipGetErrorString(e), (unsigned long long)lay.arena_bytes, (unsigned long long)pooled);
    }
    for (int k : ps.in) b->ptr[k] = (char*)b->arena + lay.plane_offset[k];
    for (int k : ps.out)
        b->ptr[k] = b->own[k] ? b->own[k] : (b->range ? b->range->va : (char*)b->arena) + lay.plane_offset[k];
    b->ptr[DSWX_PLANE_COUNTERS] = (char*)b->arena + lay.plane_offset[DSWX_PLANE_COUNTERS];
    *out = b;
    return DSWX_OK;
}

int dswx_batch_va_budget(uint64_t new_budget_bytes, uint64_t* budget_bytes, uint64_t* live_bytes, uint64_t* retired_bytes,
                         uint64_t* loose_bytes, uint64_t* pooled_bytes) {
    dswx_vmm::account(new_budget_bytes, budget_bytes, live_bytes, retired_bytes, loose_bytes, pooled_bytes);
    return DSWX_OK;
}

int dswx_batch_pool_trim(uint64_t* released_bytes) {
    const uint64_t released = dswx_vmm::pool_trim();
    if (released_bytes) *released_bytes = released;
    return DSWX_OK;
}

int dswx_batch_planes(const dswx_batch_t* b, dswx_batch_geom_t* geom, dswx_planes_in_t* in, dswx_planes_out_t* out,
                      int64_t** counters) {
    if (!b) return dswx_fail(DSWX_ERR_ARG, "batch is NULL");
    if (geom) *geom = b->geom;
    bind_structs(b, in, out);
    if (counters) *counters = (int64_t*)b->ptr[DSWX_PLANE_COUNTERS];
    return DSWX_OK;
}

int dswx_batch_info(const dswx_batch_t* b, dswx_batch_info_t* info) {
    if (!b || !info) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    memset(info, 0, sizeof *info);
    info->geom = b->geom;
    info->flags = b->flags;
    info->n_allocations = 1;
    info->bytes_allocated = b->lay.arena_bytes;
    for (int k = 0; k < DSWX_BATCH_MAX_PLANES; ++k)
        if (b->own[k]) {
            ++info->n_allocations;
            info->bytes_allocated += b->lay.plane_bytes[k] ? b->lay.plane_bytes[k] : kAlign;
        }
    if (b->range) {
        ++info->n_allocations;
        info->bytes_allocated += b->range->mapped_bytes();
        info->va_reserved_bytes = b->range->reserved;
    }
    {
        VaPool& pool = va_pool();
        std::lock_guard<std::mutex> lock(dswx_va_mutex());
        info->va_retired_bytes = pool.retired;
        info->va_budget_bytes = pool.budget;
        info->va_pooled_bytes = pool.pooled;
    }
    snprintf(info->note, sizeof info->note, "%s", b->note.c_str());
    info->search_candidates = b->search_candidates;
    info->search_probes = b->search_probes;
    info->first_come_launch_ms = b->first_ms;
    info->kept_launch_ms = b->kept_ms;
    return DSWX_OK;
}

int dswx_batch_classify(dswx_batch_t* b, const dswx_params_t* params, int64_t n_tiles, void* stream) {
    if (!b) return dswx_fail(DSWX_ERR_ARG, "batch is NULL");
    if (n_tiles == DSWX_BATCH_ALL_TILES) n_tiles = b->geom.n_tiles;
    if (n_tiles < 0 || n_tiles > b->geom.n_tiles)
        return dswx_fail(DSWX_ERR_ARG, "n_tiles %lld outside the batch (%lld resident)", (long long)n_tiles,
                         (long long)b->geom.n_tiles);
    if (n_tiles == 0) return DSWX_OK;          // an empty chunk is no work (not "all": a walk's empty last chunk must not re-classify the batch)
    dswx_batch_geom_t g = b->geom;
    g.n_tiles = n_tiles;
    dswx_planes_in_t in;
    dswx_planes_out_t out;
    bind_structs(b, &in, &out);
    return dswx_classify_batch(b->ctx, params, &g, &in, &out, (int64_t*)b->ptr[DSWX_PLANE_COUNTERS], stream);
}

int dswx_batch_synth(dswx_batch_t* b, uint64_t seed, int64_t tile0, void* stream) {
    if (!b) return dswx_fail(DSWX_ERR_ARG, "batch is NULL");
    dswx_planes_in_t in;
    bind_structs(b, &in, nullptr);
    return dswx_synth_batch(b->ctx, seed, tile0, &b->geom, &in, stream);
}

// Per-tile checksums of the selected planes (dswx_checksum.hip), one launch; the device words live in an allocation of
// this call's own -- no scratch of the context, nothing to order against its other launches.
int dswx_batch_checksum(dswx_batch_t* b, uint32_t plane_mask, int64_t tile0, int64_t n_tiles, uint64_t* out, void* stream) {
    if (!b) return dswx_fail(DSWX_ERR_ARG, "batch is NULL");
    if (int rc = dswx_select_mask(plane_mask, nullptr)) return rc;
    const dswx_batch_view v = view_of(b);
    if (int rc = dswx_select_tiles({&v}, tile0, &n_tiles, "the batch")) return rc;
    dswx_checksum_plane planes[DSWX_BATCH_MAX_PLANES];
    int n_planes = 0;
    const uint64_t px = (uint64_t)v.height * (uint64_t)v.width, stride = (uint64_t)v.tile_stride;
    if (int rc = dswx_select_walk(plane_mask, v, nullptr, [&](int k) {
            const bool counters = k == DSWX_PLANE_COUNTERS;
            const uint64_t eb = counters ? sizeof(int64_t) : DSWX_PLANES[k].bytes;
            const uint64_t n = counters ? DSWX_N_COUNTERS : px, st = counters ? DSWX_N_COUNTERS : stride;
            planes[n_planes++] = {dswx_select_base(v, k, tile0), n * eb, st * eb};
        }))
        return rc;
    if (n_planes == 0 || n_tiles == 0) return DSWX_OK;
    return read_back(b->ctx, stream, (size_t)n_planes * (size_t)n_tiles * sizeof(uint64_t), out, "dswx_batch_checksum", "checksums",
                     [&](uint64_t* dev, hipStream_t s) { return dswx_checksum_launch(b->ctx, planes, n_planes, n_tiles, dev, s); });
}

// The selected planes of two resident batches compared pair by pair (dswx_compare.hip), one launch; like the checksums the
// device records live in an allocation of this call's own.
int dswx_batch_compare(dswx_batch_t* a, dswx_batch_t* b, uint32_t plane_mask, int64_t tile0, int64_t n_tiles, double atol,
                       double rtol, int32_t equal_nan, dswx_compare_t* out, void* stream) {
    if (!a || !b) return dswx_fail(DSWX_ERR_ARG, "batch is NULL");
    if (int rc = dswx_select_mask(plane_mask, "the counters are not compared here (24 bytes per tile): compare their checksums instead "
                                              "(dswx_batch_checksum with DSWX_PLANE_COUNTERS)"))
        return rc;
    const dswx_batch_view va = view_of(a), vb = view_of(b);
    if (int rc = dswx_select_compatible(va, vb)) return rc;
    if (int rc = dswx_compare_check_tol(atol, rtol)) return rc;
    if (int rc = dswx_select_tiles({&va, &vb}, tile0, &n_tiles, "a batch")) return rc;
    dswx_compare_pair pairs[DSWX_BATCH_MAX_PLANES];
    int n_pairs = 0;
    const uint64_t px = (uint64_t)va.height * (uint64_t)va.width;
    if (int rc = dswx_select_walk(plane_mask, va, &vb, [&](int k) {
            pairs[n_pairs++] = {dswx_select_base(va, k, tile0), dswx_select_base(vb, k, tile0), DSWX_PLANES[k].kind, px,
                                (uint64_t)va.tile_stride, (uint64_t)vb.tile_stride};
        }))
        return rc;
    if (n_pairs == 0 || n_tiles == 0) return DSWX_OK;
    return read_back(a->ctx, stream, (size_t)n_pairs * (size_t)n_tiles * sizeof(dswx_compare_t), out, "dswx_batch_compare", "records",
                     [&](dswx_compare_t* dev, hipStream_t s) {
                         return dswx_compare_launch(a->ctx, pairs, n_pairs, n_tiles, atol, rtol, equal_nan, dev, s);
                     });
}

// Per-tile histograms of the selected planes (dswx_histogram.hip), one launch; like the checksums the device words live in an
// allocation of this call's own.  The kind of a plane follows the plane table: int16 planes (the bands) are binned linearly
// with band_lo / band_shift, DIAG by its five test bits, every other plane by its byte.
int dswx_batch_histogram(dswx_batch_t* b, uint32_t plane_mask, int64_t tile0, int64_t n_tiles, int32_t band_lo, int32_t band_shift,
                         uint64_t* out, void* stream) {
    if (!b) return dswx_fail(DSWX_ERR_ARG, "batch is NULL");
    if (int rc = dswx_select_mask(plane_mask, "the counters are not histogrammed (three int64 per tile): read them (dswx_batch_planes)"))
        return rc;
    if (int rc = dswx_histogram_check_kind(DSWX_HIST_I16, band_shift)) return rc;
    const dswx_batch_view v = view_of(b);
    if (int rc = dswx_select_tiles({&v}, tile0, &n_tiles, "the batch")) return rc;
    dswx_histogram_plane planes[DSWX_BATCH_MAX_PLANES];
    int n_planes = 0;
    const uint64_t px = (uint64_t)v.height * (uint64_t)v.width;
    if (int rc = dswx_select_walk(plane_mask, v, nullptr, [&](int k) {
            const int kind = k == DSWX_PLANE_DIAG ? DSWX_HIST_DIAG : DSWX_PLANES[k].kind == DSWX_CMP_I16 ? DSWX_HIST_I16 : DSWX_HIST_U8;
            static_assert(DSWX_PLANES[DSWX_PLANE_DIAG].kind == DSWX_CMP_U16, "DIAG is a uint16 plane, every plane is 8 or 16 bits wide");
            planes[n_planes++] = {dswx_select_base(v, k, tile0), kind, kind == DSWX_HIST_I16 ? band_lo : 0,
                                  kind == DSWX_HIST_I16 ? band_shift : 0, px, (uint64_t)v.tile_stride};
        }))
        return rc;
    if (n_planes == 0 || n_tiles == 0) return DSWX_OK;
    return read_back(b->ctx, stream, (size_t)n_planes * (size_t)n_tiles * DSWX_HIST_BINS * sizeof(uint64_t), out, "dswx_batch_histogram",
                     "histograms", [&](uint64_t* dev, hipStream_t s) { return dswx_histogram_launch(b->ctx, planes, n_planes, n_tiles, dev, s); });
}

// Plane pairs of two resident batches (or of one) cross-tabulated (dswx_crosstab.hip), one launch; like the checksums the
// device words live in an allocation of this call's own.  The kind a pair names for its plane a must be the plane table's.
int dswx_batch_crosstab(dswx_batch_t* a, dswx_batch_t* b, const dswx_crosstab_pair_t* pairs, int32_t n_pairs, int64_t tile0,
                        int64_t n_tiles, uint64_t* out, void* stream) {
    if (!a || !b) return dswx_fail(DSWX_ERR_ARG, "batch is NULL");
    if (n_pairs < 0 || n_pairs > DSWX_CROSSTAB_MAX_PAIRS)
        return dswx_fail(DSWX_ERR_ARG, "%d pairs: 0 .. %d per call (their tables ride in the kernel arguments)", n_pairs, DSWX_CROSSTAB_MAX_PAIRS);
    if (n_pairs && !pairs) return dswx_fail(DSWX_ERR_ARG, "pairs is NULL");
    for (int k = 0; k < n_pairs; ++k)
        for (const int p : {pairs[k].plane_a, pairs[k].plane_b}) {
            if (p < 0 || p >= DSWX_BATCH_MAX_PLANES) return dswx_fail(DSWX_ERR_ARG, "pair %d names plane %d: not 0 .. %d", k, p, DSWX_BATCH_MAX_PLANES - 1);
            if (p == DSWX_PLANE_COUNTERS)
                return dswx_fail(DSWX_ERR_ARG, "the counters are not cross-tabulated (three int64 per tile): read them (dswx_batch_planes)");
        }
    const dswx_batch_view va = view_of(a), vb = view_of(b);
    if (int rc = dswx_select_compatible(va, vb)) return rc;
    for (int k = 0; k < n_pairs; ++k)
        if (int rc = dswx_crosstab_check_spec(&pairs[k].spec)) return rc;
    if (int rc = dswx_select_tiles({&va, &vb}, tile0, &n_tiles, "a batch")) return rc;
    dswx_crosstab_item items[DSWX_CROSSTAB_MAX_PAIRS];
    const uint64_t px = (uint64_t)va.height * (uint64_t)va.width;
    for (int k = 0; k < n_pairs; ++k) {
        const int pa = pairs[k].plane_a, pb = pairs[k].plane_b, kind = pairs[k].spec.a_kind;
        const dswx_plane_desc& da = DSWX_PLANES[pa];
        const dswx_plane_desc& db = DSWX_PLANES[pb];
        if (!va.ptr[pa]) return dswx_fail(DSWX_ERR_ARG, "batch a has no plane %d (%s)", pa, da.name);
        if (!vb.ptr[pb]) return dswx_fail(DSWX_ERR_ARG, "batch b has no plane %d (%s)", pb, db.name);
        const bool fits = pa == DSWX_PLANE_DIAG ? kind == DSWX_HIST_DIAG || kind == DSWX_HIST_U16
                          : da.kind == DSWX_CMP_I16 ? kind == DSWX_HIST_I16 : kind == DSWX_HIST_U8;
        if (!fits) return dswx_fail(DSWX_ERR_ARG, "pair %d: a_kind %d does not bin plane %d (%s), %d bytes per pixel", k, kind, pa, da.name, da.bytes);
        if (db.bytes != 1) return dswx_fail(DSWX_ERR_ARG, "pair %d: plane b must be a uint8 plane, plane %d (%s) has %d bytes per pixel", k, pb, db.name, db.bytes);
        items[k] = {dswx_select_base(va, pa, tile0), dswx_select_base(vb, pb, tile0), &pairs[k].spec, px, (uint64_t)va.tile_stride,
                    (uint64_t)vb.tile_stride};
    }
    if (n_pairs == 0 || n_tiles == 0) return DSWX_OK;
    return read_back(a->ctx, stream, (size_t)n_pairs * (size_t)n_tiles * DSWX_CROSSTAB_CELLS * sizeof(uint64_t), out, "dswx_batch_crosstab",
                     "tables", [&](uint64_t* dev, hipStream_t s) { return dswx_crosstab_launch(a->ctx, items, n_pairs, n_tiles, dev, s); });
}

// The tiles of ONE uint8 plane of a resident batch composited per pixel (dswx_stack.hip), one launch, asynchronous: the
// outputs are the caller's device planes, so nothing is allocated, copied or waited for here.
int dswx_batch_stack(dswx_batch_t* b, int32_t plane, const dswx_stack_spec_t* spec, int64_t tile0, int64_t n_tiles,
                     const dswx_stack_out_t* out, void* stream) {
    dswx_batch_view v;
    const uint8_t* base;
    if (int rc = select_u8(b, plane, 0, "the counters are not stacked", "a stack is a uint8 plane", tile0, &n_tiles, &v, &base)) return rc;
    const int64_t px = v.height * v.width;
    int64_t stride = v.tile_stride;
    if (int rc = dswx_stack_check(base, spec, n_tiles, px, &stride, out, true)) return rc;
    dswx_ctx* ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    return dswx_stack_launch(ctx, base, spec, n_tiles, px, stride, out, dswx_stream_of(ctx, stream));
}

// ONE uint8 plane of a resident batch aggregated onto a coarse grid (dswx_grid.hip), one launch, asynchronous: the outputs
// are the caller's device planes, so nothing is allocated, copied or waited for here.
int dswx_batch_grid(dswx_batch_t* b, int32_t plane, const dswx_grid_spec_t* spec, int64_t tile0, int64_t n_tiles,
                    const dswx_grid_out_t* out, void* stream) {
    dswx_batch_view v;
    const uint8_t* base;
    if (int rc = select_u8(b, plane, 0, "the counters are not gridded", "a grid is made of a uint8 plane", tile0, &n_tiles, &v, &base)) return rc;
    int64_t stride = v.tile_stride;
    if (int rc = dswx_grid_check(base, spec, n_tiles, v.height, v.width, &stride, out, true)) return rc;
    dswx_ctx* ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    return dswx_grid_launch(ctx, base, spec, n_tiles, v.height, v.width, stride, out, dswx_stream_of(ctx, stream));
}

// The connected bodies of ONE uint8 plane of a resident batch (dswx_label.hip), asynchronous: the outputs are the caller's
// device planes, so nothing is allocated, copied or waited for here.
int dswx_batch_label(dswx_batch_t* b, int32_t plane, const dswx_label_spec_t* spec, int64_t tile0, int64_t n_tiles,
                     const dswx_label_out_t* out, void* stream) {
    dswx_batch_view v;
    const uint8_t* base;
    if (int rc = select_u8(b, plane, 0, "the counters are not labelled", "bodies are labelled in a uint8 plane", tile0, &n_tiles, &v, &base)) return rc;
    int64_t stride = v.tile_stride;
    if (int rc = dswx_label_check(base, spec, n_tiles, v.height, v.width, &stride, out, true)) return rc;
    dswx_ctx* ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    return dswx_label_launch(ctx, base, spec, n_tiles, v.height, v.width, stride, out, dswx_stream_of(ctx, stream));
}

// The bodies of a label plane of the caller tabulated against ONE uint8 plane of a resident batch, or none
// (dswx_body_table.hip), asynchronous: the label plane and the outputs are the caller's device planes, so nothing is
// allocated, copied or waited for here.
int dswx_batch_body_table(dswx_batch_t* b, int32_t plane, const dswx_body_spec_t* spec, int64_t tile0, int64_t n_tiles,
                          const uint32_t* label, const dswx_body_out_t* out, void* stream) {
    dswx_batch_view v;
    const uint8_t* base;          // NULL for plane -1: no value plane
    if (int rc = select_u8(b, plane, -1, "the counters are not tabulated", "bodies are tabulated against a uint8 plane", tile0, &n_tiles, &v, &base))
        return rc;
    int64_t stride = v.tile_stride;
    if (int rc = dswx_body_check(label, base, spec, n_tiles, v.height, v.width, &stride, out, true)) return rc;
    dswx_ctx* ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    return dswx_body_launch(ctx, label, base, spec, n_tiles, v.height, v.width, stride, out, dswx_stream_of(ctx, stream));
}

// The distance of every pixel to the nearest target in ONE uint8 plane of a resident batch (dswx_distance.hip), asynchronous:
// the outputs are the caller's device planes, so nothing is allocated, copied or waited for here.
int dswx_batch_distance(dswx_batch_t* b, int32_t plane, const dswx_distance_spec_t* spec, int64_t tile0, int64_t n_tiles,
                        const dswx_distance_out_t* out, void* stream) {
    dswx_batch_view v;
    const uint8_t* base;
    if (int rc = select_u8(b, plane, 0, "the counters have no distances", "distances are measured in a uint8 plane", tile0, &n_tiles, &v, &base)) return rc;
    int64_t stride = v.tile_stride;
    if (int rc = dswx_distance_check(base, spec, n_tiles, v.height, v.width, &stride, out, true)) return rc;
    dswx_ctx* ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    return dswx_distance_launch(ctx, base, spec, n_tiles, v.height, v.width, stride, out, dswx_stream_of(ctx, stream));
}

// Polygon rings burnt INTO one uint8 plane of a resident batch (dswx_burn.hip), asynchronous: the plane is both `mask` and `src`
// at the batch's stride -- the first entry here that writes a plane of the batch; acc and head are the caller's device memory,
// so nothing is allocated, copied or waited for here.
int dswx_batch_burn(dswx_batch_t* b, int32_t plane, const dswx_burn_vertex_t* verts, const int64_t* tile_first, const dswx_burn_spec_t* spec,
                    uint32_t* acc, uint64_t* head, int64_t tile0, int64_t n_tiles, void* stream) {
    dswx_batch_view v;
    const uint8_t* base;
    if (int rc = select_u8(b, plane, 0, "the counters are not burnt into", "polygons are burnt into a uint8 plane", tile0, &n_tiles, &v, &base)) return rc;
    if (spec && (spec->mask_tile_stride || spec->src_tile_stride))
        return dswx_fail(DSWX_ERR_ARG, "mask_tile_stride %lld and src_tile_stride %lld must be 0: the plane has the stride of the batch",
                         (long long)spec->mask_tile_stride, (long long)spec->src_tile_stride);
    const dswx_burn_out_t out = {acc, const_cast<uint8_t*>(base), head};
    int64_t mask_stride, src_stride;
    if (int rc = dswx_burn_check(verts, tile_first, spec, n_tiles, v.height, v.width, base, &out, &mask_stride, &src_stride, true)) return rc;
    dswx_ctx* ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    return dswx_burn_launch(ctx, verts, tile_first, spec, n_tiles, v.height, v.width, base, v.tile_stride, v.tile_stride, &out,
                            dswx_stream_of(ctx, stream));
}

// The pixels within a radius of polygon edges set IN one uint8 plane of a resident batch (dswx_reach.hip): the twin of
// dswx_batch_burn above, with the same selection, the same strides and nothing allocated, copied or waited for.
int dswx_batch_reach(dswx_batch_t* b, int32_t plane, const dswx_burn_vertex_t* verts, const int64_t* tile_first, const dswx_reach_spec_t* spec,
                     uint32_t* acc, uint64_t* head, int64_t tile0, int64_t n_tiles, void* stream) {
    dswx_batch_view v;
    const uint8_t* base;
    if (int rc = select_u8(b, plane, 0, "the counters are not reached into", "edges reach into a uint8 plane", tile0, &n_tiles, &v, &base)) return rc;
    if (spec && (spec->mask_tile_stride || spec->src_tile_stride))
        return dswx_fail(DSWX_ERR_ARG, "mask_tile_stride %lld and src_tile_stride %lld must be 0: the plane has the stride of the batch",
                         (long long)spec->mask_tile_stride, (long long)spec->src_tile_stride);
    const dswx_reach_out_t out = {acc, const_cast<uint8_t*>(base), head};
    int64_t mask_stride, src_stride;
    if (int rc = dswx_reach_check(verts, tile_first, spec, n_tiles, v.height, v.width, base, &out, &mask_stride, &src_stride, true)) return rc;
    dswx_ctx* ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    return dswx_reach_launch(ctx, verts, tile_first, spec, n_tiles, v.height, v.width, base, v.tile_stride, v.tile_stride, &out,
                             dswx_stream_of(ctx, stream));
}

// The tiles of ONE uint8 plane of a resident batch placed on a canvas and composited per canvas pixel (dswx_mosaic.hip), one
// launch, asynchronous: the table and the outputs are the caller's device memory, so nothing is allocated, copied or waited
// for here.  place[0] belongs to tile0, and last_index counts from tile0.
int dswx_batch_mosaic(dswx_batch_t* b, int32_t plane, const dswx_mosaic_spec_t* spec, int64_t tile0, int64_t n_tiles,
                      const int32_t* place, int64_t canvas_h, int64_t canvas_w, const dswx_stack_out_t* out, void* stream) {
    dswx_batch_view v;
    const uint8_t* base;
    if (int rc = select_u8(b, plane, 0, "the counters are not mosaicked", "a mosaic is made of a uint8 plane", tile0, &n_tiles, &v, &base)) return rc;
    int64_t stride = v.tile_stride;
    if (int rc = dswx_mosaic_check(base, spec, n_tiles, v.height, v.width, &stride, place, canvas_h, canvas_w, out, true)) return rc;
    dswx_ctx* ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    return dswx_mosaic_launch(ctx, base, spec, n_tiles, v.height, v.width, stride, place, canvas_h, canvas_w, out,
                              dswx_stream_of(ctx, stream));
}

// The tiles of ANY plane of a resident batch but the counters warped through a mesh of source coordinates (dswx_warp.hip), one
// memset and one launch, asynchronous: the mesh and the outputs are the caller's device memory, so nothing is allocated, copied
// or waited for here.  The element size is the plane table's; mesh 0 belongs to tile0.
int dswx_batch_warp(dswx_batch_t* b, int32_t plane, const dswx_warp_spec_t* spec, int64_t tile0, int64_t n_tiles, const int32_t* mesh,
                    int64_t dst_h, int64_t dst_w, const dswx_warp_out_t* out, void* stream) {
    if (!b) return dswx_fail(DSWX_ERR_ARG, "batch is NULL");
    if (plane < 0 || plane >= DSWX_BATCH_MAX_PLANES) return dswx_fail(DSWX_ERR_ARG, "plane %d: not 0 .. %d", plane, DSWX_BATCH_MAX_PLANES - 1);
    if (plane == DSWX_PLANE_COUNTERS)
        return dswx_fail(DSWX_ERR_ARG, "the counters are not warped (three int64 per tile): read them (dswx_batch_planes)");
    const dswx_batch_view v = view_of(b);
    const dswx_plane_desc& d = DSWX_PLANES[plane];
    if (!v.ptr[plane]) return dswx_fail(DSWX_ERR_ARG, "the batch has no plane %d (%s)", plane, d.name);
    if (spec && spec->elem_bytes != d.bytes)
        return dswx_fail(DSWX_ERR_ARG, "elem_bytes %d, but plane %d (%s) has %d bytes per pixel", spec->elem_bytes, plane, d.name, d.bytes);
    if (spec && spec->src_tile_stride)
        return dswx_fail(DSWX_ERR_ARG, "src_tile_stride %lld must be 0: the plane has the stride of the batch", (long long)spec->src_tile_stride);
    if (int rc = dswx_select_tiles({&v}, tile0, &n_tiles, "the batch")) return rc;
    const char* base = dswx_select_base(v, plane, tile0);
    int64_t stride;
    if (int rc = dswx_warp_check(base, spec, n_tiles, v.height, v.width, mesh, dst_h, dst_w, out, &stride, true)) return rc;
    dswx_ctx* ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    return dswx_warp_launch(ctx, base, spec, n_tiles, v.height, v.width, v.tile_stride, mesh, dst_h, dst_w, out, dswx_stream_of(ctx, stream));
}

// `launches` launches of the real kernel over the whole batch, after one untimed launch; ms per launch
static int probe_ms(dswx_batch* b, const dswx_params_t* params, int launches, hipEvent_t e0, hipEvent_t e1, float* ms) {
    hipStream_t s = b->ctx->stream;
    if (int rc = dswx_batch_classify(b, params, DSWX_BATCH_ALL_TILES, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventRecord(e0, s));
    for (int i = 0; i < launches; ++i)
        if (int rc = dswx_batch_classify(b, params, DSWX_BATCH_ALL_TILES, nullptr)) return rc;
    HIP_TRY(hipEventRecord(e1, s));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipEventElapsedTime(ms, e0, e1));
    *ms /= (float)launches;
    return DSWX_OK;
}

int dswx_batch_place_search(dswx_batch_t* b, const dswx_params_t* params, int32_t candidates, int32_t launches,
                            uint64_t keep_free_bytes) {
    if (!b || !params) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    if (!(b->flags & DSWX_BATCH_SEPARATE_OUTPUTS))
        return dswx_fail(DSWX_ERR_ARG, "dswx_batch_place_search needs a DSWX_BATCH_SEPARATE_OUTPUTS batch");
    if (candidates < 1 || launches < 1) return dswx_fail(DSWX_ERR_ARG, "candidates and launches must be positive");
    HIP_TRY(hipSetDevice(b->ctx->device));
    const PlaneSet ps = planes_of(b->flags);
    uint64_t out_bytes = 0;
    for (int k : ps.out) out_bytes += b->lay.plane_bytes[k] ? b->lay.plane_bytes[k] : kAlign;

    // spare sets, side by side (a freed range would simply be handed out again), bounded by free memory
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    int sets = candidates - 1;
    const uint64_t room = free_b > keep_free_bytes ? free_b - keep_free_bytes : 0;
    if ((uint64_t)sets * out_bytes > room) sets = (int)(room / (out_bytes ? out_bytes : 1));
    std::vector<std::vector<void*>> spare(DSWX_BATCH_MAX_PLANES);      // per plane: candidates of ITS size
    bool full = true;
    int complete_sets = 0;
    for (int sidx = 0; sidx < sets && full; ++sidx) {
        for (int k : ps.out) {
            void* p = nullptr;
            if (dswx_locked_malloc(&p, b->lay.plane_bytes[k] ? b->lay.plane_bytes[k] : kAlign) != hipSuccess) {
                (void)hipGetLastError();        // refused: search among what there is
                full = false;
                break;
            }
            spare[k].push_back(p);
        }
        complete_sets += full ? 1 : 0;
    }
    // planes of equal size share a pool: a candidate one plane did not take is a candidate for the next
    auto pool_of = [&](int k) -> std::vector<void*>& {
        for (int j : ps.out)
            if (b->lay.plane_bytes[j] == b->lay.plane_bytes[k]) return spare[j];
        return spare[k];
    };
    for (int k : ps.out) {
        std::vector<void*>& pool = pool_of(k);
        if (&pool != &spare[k]) {
            pool.insert(pool.end(), spare[k].begin(), spare[k].end());
            spare[k].clear();
        }
    }
    void* original[DSWX_BATCH_MAX_PLANES];
    memcpy(original, b->own, sizeof original);

    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = DSWX_OK;
    int probes = 0;
    float first_ms = 0.f, kept_ms = 0.f;
    auto bind = [&](int k, void* p) { b->own[k] = p; b->ptr[k] = p; };
    do {
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
            rc = dswx_fail(DSWX_ERR_HIP, "hipEventCreate failed");
            break;
        }
        if ((rc = probe_ms(b, params, launches, e0, e1, &first_ms))) break;
        kept_ms = first_ms;
        for (int k : ps.out) {
            std::vector<void*>& pool = pool_of(k);
            if (pool.empty()) continue;
            float best_ms;
            if ((rc = probe_ms(b, params, launches, e0, e1, &best_ms))) break;
            int best = -1;
            void* mine = b->own[k];
            for (size_t c = 0; c < pool.size(); ++c) {
                bind(k, pool[c]);
                float ms;
                rc = probe_ms(b, params, launches, e0, e1, &ms);
                bind(k, mine);
                if (rc) break;
                ++probes;
                if (ms < best_ms) { best_ms = ms; best = (int)c; }
            }
            if (rc) break;
            if (best >= 0) {
                bind(k, pool[best]);
                pool[best] = mine;
            }
        }
        if (rc || !probes) break;
        // judge the outcome under equal conditions (the part is warmer now than at first_ms): the chosen planes
        // and the first-come planes back to back; keep the better set
        void* chosen[DSWX_BATCH_MAX_PLANES];
        memcpy(chosen, b->own, sizeof chosen);
        float chosen_ms, again_ms;
        if ((rc = probe_ms(b, params, launches, e0, e1, &chosen_ms))) break;
        for (int k : ps.out) bind(k, original[k]);
        if ((rc = probe_ms(b, params, launches, e0, e1, &again_ms))) break;
        first_ms = again_ms;
        if (chosen_ms < again_ms) {
            for (int k : ps.out) bind(k, chosen[k]);
            kept_ms = chosen_ms;
        } else {
            kept_ms = again_ms;
        }
    } while (false);
    if (rc)          // whatever happened, the planes a caller may already hold stay valid
        for (int k : ps.out) bind(k, original[k]);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    // exactly the allocations the planes point at stay alive
    (void)hipStreamSynchronize(b->ctx->stream);
    std::vector<void*> all;
    for (int k : ps.out) {
        all.push_back(original[k]);
        all.insert(all.end(), spare[k].begin(), spare[k].end());
    }
    std::sort(all.begin(), all.end());       // a first-come plane that lost its place sits in a pool as well
    all.erase(std::unique(all.begin(), all.end()), all.end());
    for (void* p : all) {
        bool bound = false;
        for (int k : ps.out) bound = bound || b->own[k] == p;
        if (!bound) (void)hipFree(p);
    }
    if (rc) return rc;
    b->search_candidates = complete_sets + 1;      // complete spare sets actually obtained + the first-come planes
    b->search_probes = probes;
    b->first_ms = first_ms;
    b->kept_ms = kept_ms;
    return DSWX_OK;
}

// Sliding placement: see include/dswx_hip.h.
int dswx_batch_place_slide(dswx_batch_t* b, const dswx_params_t* params, uint64_t slack_bytes, uint64_t step_bytes,
                           int32_t spread_gaps, int32_t refine_passes, int32_t launches, uint64_t keep_free_bytes) {
    if (!b || !params) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    if (!(b->requested_flags & DSWX_BATCH_SLIDING_OUTPUTS))
        return dswx_fail(DSWX_ERR_ARG, "dswx_batch_place_slide needs a DSWX_BATCH_SLIDING_OUTPUTS batch");
    if (launches < 1 || step_bytes == 0 || spread_gaps < 0 || refine_passes < 0)
        return dswx_fail(DSWX_ERR_ARG, "launches and step_bytes must be positive, spread_gaps / refine_passes not negative");
    HIP_TRY(hipSetDevice(b->ctx->device));
    if (!b->range) {
        // the batch was asked for as a sliding one and allocated packed (dswx_batch_create's fallback): there is nothing
        // to slide; time the planes as they are so that the record is complete, keep the note
        hipEvent_t t0 = nullptr, t1 = nullptr;
        int prc = DSWX_OK;
        float ms = 0.f;
        if (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess) prc = dswx_fail(DSWX_ERR_HIP, "hipEventCreate failed");
        else prc = probe_ms(b, params, launches, t0, t1, &ms);
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        if (prc) return prc;
        b->search_candidates = b->search_probes = 0;
        b->first_ms = b->kept_ms = ms;
        return DSWX_OK;
    }
    const PlaneSet ps = planes_of(b->flags);
    const size_t region = b->lay.write_span_bytes ? b->lay.write_span_bytes : kAlign;
    const size_t step = (size_t)((step_bytes + 255) & ~(uint64_t)255);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    // the wider range is held BESIDE the current one while the search runs
    uint64_t usable = free_b;          // + the pooled chunks of the size the wide range is built from
    {
        std::lock_guard<std::mutex> lock(dswx_va_mutex());
        for (const VaPool::Spare& sp : va_pool().spare)
            if (sp.device == b->ctx->device && sp.chunk == chunk_for(region)) usable += sp.chunk;
    }
    const uint64_t room = usable > keep_free_bytes + region ? usable - keep_free_bytes - region : 0;
    size_t slack = (size_t)(slack_bytes < room ? slack_bytes : room);
    slack = slack / step * step;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    VmRange* wide = nullptr;
    void* first_ptr[DSWX_BATCH_MAX_PLANES];
    memcpy(first_ptr, b->ptr, sizeof first_ptr);
    // a candidate: the output planes in their order, the first at `off`, `gap` bytes of distance added between
    // consecutive planes (0 = packed)
    auto bind_at = [&](char* base, size_t off, size_t gap) {
        size_t n = 0;
        for (int k : ps.out) b->ptr[k] = base + off + b->lay.plane_offset[k] + gap * n++;
    };
    int rc = DSWX_OK, positions = 0;
    float first_ms = 0.f, kept_ms = 0.f;
    do {
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
            rc = dswx_fail(DSWX_ERR_HIP, "hipEventCreate failed");
            break;
        }
        if ((rc = probe_ms(b, params, launches, e0, e1, &first_ms))) break;
        kept_ms = first_ms;
        if (slack == 0) {                           // no room to slide in: the planes stay where they are
            set_note(b, "dswx_batch_place_slide: no device memory to slide in, planes left where they are");
            break;
        }
        wide = new VmRange();
        const size_t chunk = chunk_for(region);
        hipError_t e = wide->create(b->ctx->device, region + slack, chunk);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_note(b, "dswx_batch_place_slide: planes left where they are: " + wide->why);
            delete wide;
            wide = nullptr;
            break;                                  // refused: nothing to choose from
        }
        size_t best_off = 0, best_gap = 0;
        float best_ms = 0.f;
        // lab switch (tests): the candidate with this index is the one kept, whatever the clock says
        const int force = b->ctx->place_force_candidate;
        auto consider = [&](size_t off, size_t gap) {
            bind_at(wide->va, off, gap);
            float ms;
            if ((rc = probe_ms(b, params, launches, e0, e1, &ms))) return;
            if (positions == 0 || (force >= 0 ? positions == force : ms < best_ms)) { best_ms = ms; best_off = off; best_gap = gap; }
            ++positions;
        };
        // (1) the packed region at every step of the range
        for (size_t off = 0; off + region <= wide->reserved && !rc; off += step) consider(off, 0);
        // (2) the planes spread over the range with equal gaps (each write stream in a neighbourhood of its own),
        //     if the range is long enough for gaps of at least one step
        const size_t n_out = ps.out.size();
        if (!rc && spread_gaps > 0 && n_out > 1) {
            const size_t max_gap = (wide->reserved - region) / (n_out - 1) / step * step;
            for (int g = 1; g <= spread_gaps && !rc; ++g) {
                const size_t gap = max_gap * (size_t)g / (size_t)spread_gaps / step * step;
                if (gap) consider(0, gap);
            }
        }
        if (rc) break;
        // (3) refinement: from the best candidate, every plane in turn (DIAG first) tries the other free places of the
        //     range on a coarser grid and keeps the one under which the launch runs fastest -- the per-plane freedom of
        //     dswx_batch_place_search without its spare allocations (the range is already mapped)
        std::vector<size_t> pos(n_out), len(n_out);
        {
            size_t n = 0;
            for (int k : ps.out) {
                pos[n] = best_off + b->lay.plane_offset[k] + best_gap * n;
                len[n] = b->lay.plane_bytes[k] ? b->lay.plane_bytes[k] : kAlign;
                ++n;
            }
        }
        char* const wide_va = wide->va;          // (`wide` itself is handed to the batch below)
        auto bind_pos = [&]() {
            size_t n = 0;
            for (int k : ps.out) b->ptr[k] = wide_va + pos[n++];
        };
        for (int pass = 0; pass < refine_passes && force < 0 && !rc; ++pass) {
            const size_t rstep = step * 2;
            for (size_t i = 0; i < n_out && !rc; ++i) {
                bind_pos();
                float here_ms;
                if ((rc = probe_ms(b, params, launches, e0, e1, &here_ms))) break;
                size_t best_q = pos[i];
                const size_t mine = pos[i];
                for (size_t q = 0; q + len[i] <= wide->reserved && !rc; q += rstep) {
                    bool clash = false;
                    for (size_t j = 0; j < n_out; ++j)
                        clash = clash || (j != i && q < pos[j] + len[j] && pos[j] < q + len[i]);
                    if (clash || q == mine) continue;
                    pos[i] = q;
                    bind_pos();
                    float ms;
                    if ((rc = probe_ms(b, params, launches, e0, e1, &ms))) break;
                    ++positions;
                    if (ms < here_ms) { here_ms = ms; best_q = q; }
                }
                pos[i] = best_q;
            }
        }
        if (rc) break;
        // equal conditions (the part is warmer now): the best candidate and the first-come range back to back
        float chosen_ms, again_ms;
        bind_pos();
        if ((rc = probe_ms(b, params, launches, e0, e1, &chosen_ms))) break;
        memcpy(b->ptr, first_ptr, sizeof first_ptr);
        if ((rc = probe_ms(b, params, launches, e0, e1, &again_ms))) break;
        first_ms = again_ms;
        if (force >= 0 || chosen_ms < again_ms) {
            // keep the chosen placement: its chunks -- the physical memory -- move into a fresh range (addresses no kernel
            // has used), the wide range is dropped whole, which is what gives its other chunks back to the device
            (void)hipStreamSynchronize(b->ctx->stream);
            std::vector<std::pair<size_t, size_t>> keep;
            for (size_t i = 0; i < n_out; ++i) keep.push_back({pos[i], pos[i] + len[i]});
            size_t base = 0;
            VmRange* home = wide->rehome(keep, &base);
            if (!home) {
                set_note(b, "dswx_batch_place_slide: the chosen chunks could not be moved (" + wide->why + "), planes left where they were");
                kept_ms = again_ms;
            } else {
                size_t n = 0;
                for (int k : ps.out) b->ptr[k] = home->va + (pos[n++] - base);
                float homed_ms;
                if ((rc = probe_ms(b, params, launches, e0, e1, &homed_ms))) {
                    memcpy(b->ptr, first_ptr, sizeof first_ptr);
                    (void)hipStreamSynchronize(b->ctx->stream);
                    home->destroy();
                    delete home;
                    break;
                }
                if (force >= 0 || homed_ms < again_ms) {
                    (void)hipStreamSynchronize(b->ctx->stream);
                    b->range->destroy();
                    delete b->range;
                    b->range = home;
                    b->region_offset = pos[0] - base;
                    kept_ms = homed_ms;
                } else {            // under its new addresses the placement is no better than the first-come one: drop it
                    memcpy(b->ptr, first_ptr, sizeof first_ptr);
                    (void)hipStreamSynchronize(b->ctx->stream);
                    home->destroy();
                    delete home;
                    kept_ms = again_ms;
                }
            }
        } else {
            kept_ms = again_ms;
        }
    } while (false);
    if (rc) memcpy(b->ptr, first_ptr, sizeof first_ptr);
    (void)hipStreamSynchronize(b->ctx->stream);
    if (wide) { wide->destroy(); delete wide; }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc) return rc;
    b->search_candidates = positions;
    b->search_probes = positions;
    b->first_ms = first_ms;
    b->kept_ms = kept_ms;
    return DSWX_OK;
}

}  // extern "C"
