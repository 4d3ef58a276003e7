// dswx_host.h -- host-side internals shared by the translation units of libdswx_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>

#include "dswx_device.h"
#include "dswx_mesh_rule.h"

// A grow-only device allocation of a context.
struct dswx_workspace {
    void* p = nullptr;
    size_t bytes = 0;
};

struct dswx_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    // The grow-only device workspaces (dswx_ws_reserve below), freed in a loop by dswx_ctx_destroy:
    //   WS_STAGE    staging arena of dswx_classify_host (pageable planes: one tile; lab pipeline: three slots)
    //   WS_PARTIALS the vector kernels' per-wave counter partials
    //   WS_FOLD     accumulators of the folded counters (launches of a few tiles, dswx_classify_lut.hip): zeroed when
    //                allocated, left zero by every launch that completes; a launch path that fails marks them dirty
    //   WS_COVER    'cover' mode: state byte per pixel + bitmap dword per 8-pixel group + final snow bits
    //   WS_UNTILE   dswx_untile_device for Float32 + floating-point predictor (the byte-wise running sums)
    enum { WS_STAGE, WS_PARTIALS, WS_FOLD, WS_COVER, WS_UNTILE, WS_COUNT };
    dswx_workspace ws[WS_COUNT];
    bool fold_clean = false;
    // The workspaces of a context (tables, counter partials, fold accumulators, 'cover' scratch, the Float32 untile
    // scratch) are shared by all its launches.  Launches on ONE stream are ordered by the stream; a launch on a different stream than the previous one
    // waits for it (dswx_ws_enter / dswx_ws_leave in dswx_hip.hip: an event recorded behind every launch on a caller's
    // stream, or on the context's own stream at the moment the stream changes) -- two launches of one context never
    // overlap on the GPU (the fold accumulators would otherwise be left non-zero for good).
    hipStream_t ws_last = nullptr;         // the stream of the last launch that used the workspaces
    bool ws_used = false;
    hipEvent_t ws_event = nullptr;
    // device copy of the lookup tables of the table-driven kernel (rebuilt per call)
    void* tables = nullptr;
    bool tables_valid = false;             // the device tables match tables_params, built on tables_stream
    hipStream_t tables_stream = nullptr;
    alignas(8) unsigned char tables_params[1024] = {};
    // pipelined host path (pinned host buffers): copy streams, per-slot events, pinned counter scratch
    hipStream_t h2d_stream = nullptr, d2h_stream = nullptr;
    hipEvent_t pipe_in[3] = {nullptr, nullptr, nullptr}, pipe_k[3] = {nullptr, nullptr, nullptr},
               pipe_out[3] = {nullptr, nullptr, nullptr};
    int64_t* pipe_counters = nullptr;      // hipHostMalloc, [pipe_counters_cap][3]
    size_t pipe_counters_cap = 0;
    // Fixed in production; libdswx_lab.so (experiments, A/B tools, variant tests) changes them through
    // dswx_lab_configure -- the product library reads no environment variable.
    int cover_kernel = 8;                  // 'cover' stage 2: words per window row (8 = 256-column windows, 4 = 128)
    int host_pipeline = 2;                 // page-locked host planes: 2 zero copy, 1 staged three-stream pipeline (lab A/B),
                                           // 0 forces the synchronous path
    int host_chunks = 8;                   // pieces per tile of the pipelined host path
    int shadow_kernel = 0;                 // 2 forces the general one-pixel kernel dswx_shadow_v2 (tests: the exact arithmetic alone);
                                           // 3: the filter kernel in two launches, even block rows then odd (Infinity Cache probe)
    int shadow_grid_pad = 1;               // dswx_shadow_v3: grid.x rounded up to a multiple of this (lab A/B, see the launch)
    std::string last_kernel;
    int tune_lut_wps = 0;    // table-driven kernel: launch bound (4, 5, 6; 0 = automatic)
    int tune_lut_interleave = -1;   // table-driven kernel: tiles whose blocks are interleaved in dispatch order (-1 = the
                                    // product default, dswx_lut_launch: none; 0 / 1 = none).  Measured in round 4 on
                                    // three first-come arenas, 256 tiles, GB/s: none 5976 / 5618 / 6292, G = 4 6006 /
                                    // 5633 / 6397, G = 8 5941 / 5623 / 6354, G = 16 5731 / 5352 / 6285, G = 64 5624 /
                                    // 5201 / 6290, G = 256 5606 / 5214 / 6187 (profiles/r04_ab_interleave.json): spreading
                                    // the 14 streams over many tiles does not lift a badly placed arena and costs 2 - 7 %
                                    // beyond G = 8; kept as a lab switch only
    int tune_wps = 6;        // launch bound of the direct kernel without masks (4, 6, 8)
    int tune_fold = 1;       // 0: always the separate dswx_counters_finish launch (lab A/B of the folded counters)
    int place_force_candidate = -1;   // dswx_batch_place_slide: >= 0 keeps the candidate with that index (packed region at
                                      // offset index * step of the wide range) WHATEVER it measures, without refinement --
                                      // tests only (the kept-placement + trim-while-live case must not hang on a timing)
    int fused_variant = -1;  // -1 automatic = the table-driven kernel (every layout since round 6); 0 forces the direct
                             // kernel, 3 the table-driven one (lab A/B and the variant parity tests)
};

// Orders the launches that use the workspaces above across streams (dswx_hip.hip): enter before the first launch (and
// before growing a workspace: its hipStreamSynchronize(s) then covers the other streams' work too), leave after the last.
int dswx_ws_enter(dswx_ctx* ctx, hipStream_t s);
int dswx_ws_leave(dswx_ctx* ctx, hipStream_t s);

// records a printf-style message for dswx_last_error() and returns `code`
int dswx_fail(int code, const char* fmt, ...);
// validates `p` and derives the kernel parameter block (integer thresholds, exact-quotient
// constants, aerosol table); DSWX_ERR_ARG with a message for unusable thresholds
int dswx_make_dev_params(const dswx_params_t* p, DevParams* d);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return dswx_fail(DSWX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                             __FILE__, __LINE__);                                                  \
    } while (0)

// The hipMalloc calls of THIS library go through one mutex, the one dswx_batch_pool_trim (dswx_vmm.h) holds while it frees a
// retired range's addresses and reserves them again: between those two calls the addresses are up for grabs, and an
// allocation of another thread of this library must not be the one that takes them (a stress of four threads creating and
// placing batches lost one range in two hundred that way).  The fence covers nothing else: hipHostMalloc, stream and event
// creation, the runtime's own allocations (module load, first launch of a kernel) and every allocation of the caller's
// threads can still land there -- the account reports such a loss (dswx_batch_va_budget: loose_bytes), and the header asks
// callers to trim when nothing else in the process allocates.  (VmRange::destroy itself only retires a range.)
std::mutex& dswx_va_mutex();
template <typename T>
static inline hipError_t dswx_locked_malloc(T** p, size_t n) {
    std::lock_guard<std::mutex> lock(dswx_va_mutex());
    return hipMalloc(reinterpret_cast<void**>(p), n);
}

// The stream of an entry that takes one: the caller's, or the context's own for NULL.
static inline hipStream_t dswx_stream_of(const dswx_ctx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->stream; }

// Device memory that one call owns: up to four allocations, used on ONE stream and freed when the call returns, however
// it returns.  What is queued must not outlive the allocation: unless the call's last act on the stream was a successful
// sync(), the destructor waits for the stream (result ignored: nothing is left to do about it) before it frees.
struct dswx_call_scratch {
    hipStream_t s;
    void* p[4] = {nullptr, nullptr, nullptr, nullptr};
    int n = 0;
    bool queued = false;      // work may have been queued on `s` since the last successful sync()
    explicit dswx_call_scratch(hipStream_t stream) : s(stream) {}
    dswx_call_scratch(const dswx_call_scratch&) = delete;      // one owner: the call
    template <typename T>
    hipError_t take(T** out, size_t bytes) {
        if (n == 4) return hipErrorOutOfMemory;
        const hipError_t e = dswx_locked_malloc(out, bytes);
        if (e == hipSuccess) { p[n++] = *out; queued = true; }
        return e;
    }
    hipError_t sync() {
        const hipError_t e = hipStreamSynchronize(s);
        if (e == hipSuccess) queued = false;
        return e;
    }
    ~dswx_call_scratch() {
        if (queued) (void)hipStreamSynchronize(s);
        for (int i = 0; i < n; ++i) (void)hipFree(p[i]);
    }
};

static inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Unaligned host accesses (a host buffer may sit at any address): element `index` of an array of T that begins at `base`.
// The index is ALWAYS in elements of T; a field at a byte offset is addressed at the call, static_cast<unsigned char*>(base) + bytes.
template <class T> static inline T dswx_load(const void* base, size_t index) {
    T v;
    std::memcpy(&v, static_cast<const unsigned char*>(base) + index * sizeof(T), sizeof(T));
    return v;
}
template <class T> static inline void dswx_store(void* base, size_t index, T v) {
    std::memcpy(static_cast<unsigned char*>(base) + index * sizeof(T), &v, sizeof(T));
}

// ---- The frame of a raster entry.  The geometry refusals of a tiled plane, in the house order; an entry with a refusal of
// its own between two of them calls the three parts, every other one dswx_tile_geometry_check.
// A stride of 0 is the tile itself; `what` names the stride in the refusal.
static inline int dswx_tile_stride_check(int64_t* stride, int64_t n_elems, const char* what = "tile_stride") {
    if (*stride == 0) *stride = n_elems;
    if (*stride < n_elems) return dswx_fail(DSWX_ERR_ARG, "%s smaller than the tile", what);
    return DSWX_OK;
}
// `tiles32`: the kernels number the tiles in 32 bits (the stack and the mosaic have a smaller limit of their own)
static inline int dswx_tile_extent_check(int64_t stride, int64_t n_tiles, bool tiles32) {
    if ((tiles32 && n_tiles > (1LL << 32)) || stride > (1LL << 46) || (n_tiles && (uint64_t)stride > (1ull << 46) / (uint64_t)n_tiles))
        return dswx_fail(DSWX_ERR_ARG, "plane too large");
    return DSWX_OK;
}
static inline int dswx_tile_plane_check(const void* plane, int64_t n_tiles, int64_t n_elems, const char* what = "plane") {
    if (!plane && n_tiles > 0 && n_elems > 0) return dswx_fail(DSWX_ERR_ARG, "%s is NULL", what);
    return DSWX_OK;
}
static inline int dswx_tile_geometry_check(const void* plane, int64_t n_tiles, int64_t n_elems, int64_t* stride, bool tiles32) {
    if (int rc = dswx_tile_stride_check(stride, n_elems)) return rc;
    if (int rc = dswx_tile_extent_check(*stride, n_tiles, tiles32)) return rc;
    return dswx_tile_plane_check(plane, n_tiles, n_elems);
}

// Per-category count outputs (`count[max_cats]`, of any element type): none beyond n_cats, and some output wanted at all
template <class P> static inline int dswx_outputs_check(P* const* count, int max_cats, int n_cats, bool any_other) {
    bool any = any_other;
    for (int k = 0; k < max_cats; ++k) {
        if (count[k] && k >= n_cats) return dswx_fail(DSWX_ERR_ARG, "count[%d] is not NULL but n_cats is %d", k, n_cats);
        any = any || count[k];
    }
    if (!any) return dswx_fail(DSWX_ERR_ARG, "every output is NULL");
    return DSWX_OK;
}

// The tail of a *_device entry, behind the checks of its arguments: the context, its device, and `launch` on the caller's
// stream or the context's own.
template <class Launch> static inline int dswx_device_entry(dswx_ctx* ctx, void* stream, Launch launch) {
    if (!ctx) return dswx_fail(DSWX_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return launch(dswx_stream_of(ctx, stream));
}
// last_kernel of a launch that had nothing to do
constexpr const char* DSWX_NO_KERNEL = "none (empty input)";

// Grows workspace `w` of a context to at least `need` bytes (dswx_hip.hip): the one place a workspace is freed and
// allocated again.  The free waits first for the work that may still use the old allocation: stream `s` (after
// dswx_ws_enter that covers the context's work on other streams too), or the whole device.
int dswx_ws_reserve(dswx_workspace& w, size_t need, hipStream_t s, bool whole_device = false);

// ---- The 22 planes of a classify call: the pointers of dswx_planes_in_t, then those of dswx_planes_out_t, in ABI order
// (for the first 19 that is the DSWX_PLANE_* numbering of the batch layout).  The ONE statement of which planes there
// are, where their pointers live, how wide a pixel is and which are inputs; every host loop over "the planes" walks it.
struct dswx_plane_desc {
    const char* name;
    bool input;               // a pointer of dswx_planes_in_t (else of dswx_planes_out_t)
    unsigned char bytes;      // per pixel
    signed char batch;        // DSWX_PLANE_* index; -1: not part of a batch (the float64 index planes)
    unsigned short offset;    // of the pointer inside its struct
    signed char kind;         // DSWX_CMP_* of its pixels (dswx_batch_compare)
};
#define DSWX_BAND_(k) {"band[" #k "]", true, 2, DSWX_PLANE_BAND0 + k, offsetof(dswx_planes_in_t, band) + k * sizeof(void*), DSWX_CMP_I16}
#define DSWX_IN_(f, idx) {#f, true, 1, idx, offsetof(dswx_planes_in_t, f), DSWX_CMP_U8}
#define DSWX_OUT_(f, bytes, idx) \
    {#f, false, bytes, idx, offsetof(dswx_planes_out_t, f), bytes == 1 ? DSWX_CMP_U8 : bytes == 2 ? DSWX_CMP_U16 : DSWX_CMP_F64}
constexpr dswx_plane_desc DSWX_PLANES[] = {
    DSWX_BAND_(0), DSWX_BAND_(1), DSWX_BAND_(2), DSWX_BAND_(3), DSWX_BAND_(4), DSWX_BAND_(5),
    DSWX_IN_(fmask, DSWX_PLANE_FMASK), DSWX_IN_(land, DSWX_PLANE_LAND), DSWX_IN_(shad, DSWX_PLANE_SHAD),
    DSWX_IN_(ocean, DSWX_PLANE_OCEAN),
    DSWX_OUT_(diag, 2, DSWX_PLANE_DIAG), DSWX_OUT_(wtr1, 1, DSWX_PLANE_WTR1),
    DSWX_OUT_(wtr1_aerosol, 1, DSWX_PLANE_WTR1_AEROSOL), DSWX_OUT_(wtr2, 1, DSWX_PLANE_WTR2),
    DSWX_OUT_(wtr, 1, DSWX_PLANE_WTR), DSWX_OUT_(bwtr, 1, DSWX_PLANE_BWTR), DSWX_OUT_(conf, 1, DSWX_PLANE_CONF),
    DSWX_OUT_(cloud, 1, DSWX_PLANE_CLOUD), DSWX_OUT_(browse, 1, DSWX_PLANE_BROWSE),
    DSWX_OUT_(mndwi, 8, -1), DSWX_OUT_(ndvi, 8, -1), DSWX_OUT_(awesh, 8, -1),
};
#undef DSWX_BAND_
#undef DSWX_IN_
#undef DSWX_OUT_
constexpr int DSWX_N_PLANES = sizeof DSWX_PLANES / sizeof DSWX_PLANES[0];

constexpr bool dswx_planes_in_abi_order() {     // every pointer of both structs, once, in order; batch index = position
    constexpr int n_in = sizeof(dswx_planes_in_t) / sizeof(void*);
    for (int i = 0; i < DSWX_N_PLANES; ++i) {
        const dswx_plane_desc& d = DSWX_PLANES[i];
        if (d.input != (i < n_in) || d.offset != (d.input ? i : i - n_in) * sizeof(void*)) return false;
        if (d.batch != (i < DSWX_PLANE_COUNTERS ? i : -1)) return false;
    }
    return true;
}
static_assert(sizeof(dswx_planes_in_t) + sizeof(dswx_planes_out_t) == DSWX_N_PLANES * sizeof(void*) &&
              dswx_planes_in_abi_order(), "DSWX_PLANES does not match dswx_planes_in_t / dswx_planes_out_t");

// The pointer of plane `d` in an (in, out) pair, read and replaced as a plain address; a NULL struct has no planes.
static inline char* dswx_plane_get(const dswx_plane_desc& d, const dswx_planes_in_t* in, const dswx_planes_out_t* out) {
    const char* s = d.input ? reinterpret_cast<const char*>(in) : reinterpret_cast<const char*>(out);
    char* p = nullptr;
    if (s) std::memcpy(&p, s + d.offset, sizeof p);
    return p;
}
static inline void dswx_plane_set(const dswx_plane_desc& d, dswx_planes_in_t* in, dswx_planes_out_t* out, const void* p) {
    char* s = d.input ? reinterpret_cast<char*>(in) : reinterpret_cast<char*>(out);
    if (s) std::memcpy(s + d.offset, &p, sizeof p);
}

// Launches of at most this many tiles sum the coverage counters inside the fused kernel (last-block-done) instead of in
// the separate dswx_counters_finish launch, which is ~10 us + a kernel boundary: a quarter of a single-tile call, 0.09 % of
// a 256-tile one (measurements in DESIGN.md section 5).
constexpr int DSWX_FOLD_MAX_TILES = 16;

// ---- table-driven production kernel (dswx_classify_lut.hip)
int dswx_lut_fold_group_log2(bool extras);
void dswx_lut_geometry(const dswx_ctx* ctx, long long groups, bool extras, int lead_max, int* threads, long long* gx);
int dswx_lut_launch(dswx_ctx* ctx, const KArgs& args, bool masks, dim3 grid, dim3 block, hipStream_t stream,
                    char* info, size_t info_len);

// ---- checksums (dswx_checksum.hip): one plane of a launch, in bytes (the kernel does not know element sizes)
struct dswx_checksum_plane {
    const void* base;
    uint64_t tile_bytes;      // checksummed bytes of every tile, from its start
    uint64_t stride_bytes;    // between tiles
};
int dswx_checksum_launch(dswx_ctx* ctx, const dswx_checksum_plane* planes, int n_planes, int64_t n_tiles, uint64_t* out,
                         hipStream_t s);

// ---- compare (dswx_compare.hip): one plane pair of a launch, in elements of its kind
struct dswx_compare_pair {
    const void* a;
    const void* b;
    int kind;                 // DSWX_CMP_*
    uint64_t n_elems;         // compared elements of every tile, from its start
    uint64_t a_stride_elems, b_stride_elems;      // between tiles
};
int dswx_compare_elem_bytes(int kind);            // 0: not a kind
int dswx_compare_check_tol(double atol, double rtol);
int dswx_compare_launch(dswx_ctx* ctx, const dswx_compare_pair* pairs, int n_pairs, int64_t n_tiles, double atol, double rtol,
                        int equal_nan, dswx_compare_t* out, hipStream_t s);

// ---- histogram (dswx_histogram.hip): one plane of a launch, in elements of its kind
struct dswx_histogram_plane {
    const void* base;
    int kind;                 // DSWX_HIST_*
    int lo, shift;            // DSWX_HIST_U16 / DSWX_HIST_I16
    uint64_t n_elems;         // counted elements of every tile, from its start
    uint64_t stride_elems;    // between tiles
};
int dswx_histogram_elem_bytes(int kind);          // 0: not a kind
int dswx_histogram_check_kind(int kind, int shift);
int dswx_histogram_launch(dswx_ctx* ctx, const dswx_histogram_plane* planes, int n_planes, int64_t n_tiles, uint64_t* out,
                          hipStream_t s);

// ---- crosstab (dswx_crosstab.hip): one plane pair of a launch, a in elements of spec->a_kind, b in bytes
struct dswx_crosstab_item {
    const void* a;
    const void* b;
    const dswx_crosstab_spec_t* spec;
    uint64_t n_elems;         // counted pairs of every tile, from its start
    uint64_t a_stride_elems, b_stride_elems;      // between tiles
};
int dswx_crosstab_check_spec(const dswx_crosstab_spec_t* spec);
int dswx_crosstab_launch(dswx_ctx* ctx, const dswx_crosstab_item* items, int n_pairs, int64_t n_tiles, uint64_t* out,
                         hipStream_t s);

// ---- stack (dswx_stack.hip): the shared checks of the entries (resolves a stride of 0; `align`: the uint16 outputs must be
// 2-byte aligned), and the one launch for arguments that passed them
int dswx_stack_check(const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems, int64_t* stride,
                     const dswx_stack_out_t* out, bool align);
int dswx_stack_launch(dswx_ctx* ctx, const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems,
                      int64_t stride, const dswx_stack_out_t* out, hipStream_t s);

// ---- grid (dswx_grid.hip): the shared checks of the entries (resolves a stride of 0; `align`: the uint32 outputs must be
// 4-byte aligned), and the one launch for arguments that passed them
int dswx_grid_check(const uint8_t* plane, const dswx_grid_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                    int64_t* stride, const dswx_grid_out_t* out, bool align);
int dswx_grid_launch(dswx_ctx* ctx, const uint8_t* plane, const dswx_grid_spec_t* spec, int64_t n_tiles, int64_t height,
                     int64_t width, int64_t stride, const dswx_grid_out_t* out, hipStream_t s);

// ---- label (dswx_label.hip): the shared checks of the entries (resolves a stride of 0; `align`: label and size must be
// 4-byte and summary 8-byte aligned), and the launches for arguments that passed them
int dswx_label_check(const uint8_t* plane, const dswx_label_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                     int64_t* stride, const dswx_label_out_t* out, bool align);
int dswx_label_launch(dswx_ctx* ctx, const uint8_t* plane, const dswx_label_spec_t* spec, int64_t n_tiles, int64_t height,
                      int64_t width, int64_t stride, const dswx_label_out_t* out, hipStream_t s);

// ---- body table (dswx_body_table.hip): the shared checks of the entries (resolves a value stride of 0; `align`: label and
// dense must be 4-byte and rows and head 8-byte aligned), and the launches for arguments that passed them
int dswx_body_check(const uint32_t* label, const uint8_t* value, const dswx_body_spec_t* spec, int64_t n_tiles, int64_t height,
                    int64_t width, int64_t* stride, const dswx_body_out_t* out, bool align);
int dswx_body_launch(dswx_ctx* ctx, const uint32_t* label, const uint8_t* value, const dswx_body_spec_t* spec, int64_t n_tiles,
                     int64_t height, int64_t width, int64_t stride, const dswx_body_out_t* out, hipStream_t s);

// ---- distance (dswx_distance.hip): the shared checks of the entries (resolves a stride of 0; `align`: dist2 and nearest
// must be 4-byte and summary 8-byte aligned), and the launches for arguments that passed them
int dswx_distance_check(const uint8_t* plane, const dswx_distance_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                        int64_t* stride, const dswx_distance_out_t* out, bool align);
int dswx_distance_launch(dswx_ctx* ctx, const uint8_t* plane, const dswx_distance_spec_t* spec, int64_t n_tiles, int64_t height,
                         int64_t width, int64_t stride, const dswx_distance_out_t* out, hipStream_t s);

// ---- outline (dswx_outline.hip): the launches for arguments that passed the checks of dswx_outline_device
int dswx_outline_launch(dswx_ctx* ctx, const uint32_t* ids, const dswx_outline_spec_t* spec, int64_t n_tiles, int64_t height,
                        int64_t width, const dswx_outline_out_t* out, void* work, hipStream_t s);

// ---- burn (dswx_burn.hip): the shared checks of the entries (resolves the two strides of the spec, 0 = height * width;
// `align`: verts must be 16-byte, acc 4-byte and tile_first and head 8-byte aligned), and the launches for arguments that
// passed them, with the strides given apart from the spec (a batch has its own)
int dswx_burn_check(const void* verts, const int64_t* tile_first, const dswx_burn_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                    const uint8_t* src, const dswx_burn_out_t* out, int64_t* mask_stride, int64_t* src_stride, bool align);
int dswx_burn_launch(dswx_ctx* ctx, const void* verts, const int64_t* tile_first, const dswx_burn_spec_t* spec, int64_t n_tiles, int64_t height,
                     int64_t width, const uint8_t* src, int64_t mask_stride, int64_t src_stride, const dswx_burn_out_t* out, hipStream_t s);

// ---- reach (dswx_reach.hip): as for the burn: its checks are dswx_burn_check plus the radius and the reserved word
int dswx_reach_check(const void* verts, const int64_t* tile_first, const dswx_reach_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                     const uint8_t* src, const dswx_reach_out_t* out, int64_t* mask_stride, int64_t* src_stride, bool align);
int dswx_reach_launch(dswx_ctx* ctx, const void* verts, const int64_t* tile_first, const dswx_reach_spec_t* spec, int64_t n_tiles, int64_t height,
                      int64_t width, const uint8_t* src, int64_t mask_stride, int64_t src_stride, const dswx_reach_out_t* out, hipStream_t s);

// ---- mosaic (dswx_mosaic.hip): the shared checks of the entries (resolves a stride of 0; `align`: the uint16 outputs must
// be 2-byte and the placement table 4-byte aligned), and the launch for arguments that passed them
int dswx_mosaic_check(const uint8_t* plane, const dswx_mosaic_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                      int64_t* stride, const int32_t* place, int64_t canvas_h, int64_t canvas_w, const dswx_stack_out_t* out,
                      bool align);
int dswx_mosaic_launch(dswx_ctx* ctx, const uint8_t* plane, const dswx_mosaic_spec_t* spec, int64_t n_tiles, int64_t height,
                       int64_t width, int64_t stride, const int32_t* place, int64_t canvas_h, int64_t canvas_w,
                       const dswx_stack_out_t* out, hipStream_t s);

// ---- warp (dswx_warp.hip): the shared checks of the entries (resolves the stride of the plane, 0 = height * width; `align`:
// mesh and src_index must be 4-byte, head 8-byte and plane and dst elem_bytes aligned), and the memset and the launch for
// arguments that passed them, with the stride of the plane given apart from the spec (a batch has its own)
int dswx_warp_check(const void* plane, const dswx_warp_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                    const int32_t* mesh, int64_t dst_h, int64_t dst_w, const dswx_warp_out_t* out, int64_t* src_stride, bool align);
int dswx_warp_launch(dswx_ctx* ctx, const void* plane, const dswx_warp_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                     int64_t src_stride, const int32_t* mesh, int64_t dst_h, int64_t dst_w, const dswx_warp_out_t* out, hipStream_t s);
// ---- what the warp and the resample entries (dswx_resample.hip) share, defined in dswx_warp.hip.  The geometry half of their
// checks: shift, reserved, sizes, strides
int dswx_mesh_geometry_check(int shift, int reserved, int64_t src_tile_stride, int64_t mesh_tile_stride_nodes, int64_t n_tiles,
                             int64_t height, int64_t width, int64_t dst_h, int64_t dst_w, int64_t* src_stride);
// is there anything to do: tiles, destination pixels and an output that is wanted
static inline bool dswx_mesh_work(int64_t n_tiles, int64_t dst_h, int64_t dst_w, bool wanted) {
    return n_tiles > 0 && dst_h > 0 && dst_w > 0 && wanted;
}
// the pointer half: a mesh and (if `plane_read`) a plane where there is work, then (`align`) mesh, src_index (NULL: none), head,
// plane and dst
int dswx_mesh_pointer_check(bool work, const void* plane, bool plane_read, int elem_bytes, const int32_t* mesh, const void* dst,
                            const uint32_t* src_index, const uint64_t* head, bool align);
// before the launch of either kernel: the fields that WarpArgs and ResArgs have in common, for rectangles of rect_h x rect_w
// pixels; a wanted head (8 words per tile) set to 0xFF bytes; grid.y (past 65535 tiles the workgroups of a row walk the tiles)
template <class Args>
static inline int dswx_mesh_launch_prepare(Args& a, const void* plane, int64_t src_stride, int elem_bytes, const int32_t* mesh,
                                           int64_t mesh_tile_stride_nodes, int shift, int64_t n_tiles, int64_t height, int64_t width,
                                           int64_t dst_h, int64_t dst_w, int rect_h, int rect_w, void* dst, uint64_t* head, hipStream_t s,
                                           unsigned* grid_y) {
    static_assert(DSWX_WARP_HEAD_WORDS == 8 && DSWX_RESAMPLE_HEAD_WORDS == 8, "one head of 8 words per tile");
    const unsigned long long nbx = ((unsigned long long)dst_w + rect_w - 1) / rect_w, nby = ((unsigned long long)dst_h + rect_h - 1) / rect_h;
    a.plane = static_cast<const unsigned char*>(plane);
    a.src_stride_bytes = (unsigned long long)src_stride * (unsigned)elem_bytes;
    a.mesh = mesh;
    a.mesh_stride_ints = 2ull * (unsigned long long)mesh_tile_stride_nodes;
    a.n_tiles = (unsigned long long)n_tiles;
    a.n_rects = nbx * nby;
    a.dst_px = (unsigned long long)dst_h * (unsigned long long)dst_w;
    a.height = (int)height;
    a.width = (int)width;
    a.dst_h = (int)dst_h;
    a.dst_w = (int)dst_w;
    a.shift = shift;
    a.mesh_w = (int)mesh_dims(dst_w, shift);
    a.nbx = (unsigned)nbx;
    a.dst = static_cast<unsigned char*>(dst);
    a.head = reinterpret_cast<unsigned long long*>(head);
    if (head) HIP_TRY(hipMemsetAsync(head, 0xFF, (size_t)n_tiles * 8 * sizeof(uint64_t), s));
    *grid_y = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
    return DSWX_OK;
}

// ---- 'cover' mode stage 2 (dswx_cover.hip): appends its description to `info`
int dswx_cover_stage2_launch(dswx_ctx* ctx, const KArgs& c2, long long n_tiles, hipStream_t stream, char* info,
                             size_t info_len);
