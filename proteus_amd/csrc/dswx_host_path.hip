// dswx_host_path.hip -- dswx_classify_host: the host-pointer entry of the classifier.
// Pageable buffers (and memory a caller page-locked itself): one tile at a time, copy -> classify -> copy on one
// stream.  Buffers from dswx_host_alloc: ZERO COPY -- the kernels read the input planes and write the
// layers across PCIe themselves, both directions at once (3.9 Gpixel/s for 13 B in + 8 B out per pixel,
// measured on four 3660^2 tiles; the staged three-stream pipeline below it reaches 3.05 and stays as a lab A/B).
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>

#include <map>
#include <mutex>

#include "dswx_host.h"

// The page-locked spans this library handed out (dswx_host_alloc): allocated AND resident, the only host memory
// the kernels are let loose on directly (zero copy).  Memory a caller registered itself (hipHostRegister) is
// page-locked in HIP's eyes too, but its pages need not be resident -- see the note in dswx_classify_host.
// (heap objects that are never destroyed: frees that arrive while the process exits must still find them)
static std::mutex& g_spans_mutex = *new std::mutex;
static std::map<uintptr_t, size_t>& g_spans = *new std::map<uintptr_t, size_t>;        // base -> bytes

static bool in_own_span(const void* p, size_t bytes) {
    if (!p) return true;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lock(g_spans_mutex);
    auto it = g_spans.upper_bound(a);
    if (it == g_spans.begin()) return false;
    --it;
    return a >= it->first && a + bytes <= it->first + it->second;
}

extern "C" {

int dswx_host_alloc(dswx_ctx_t* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = bytes ? bytes : 1;
    HIP_TRY(hipHostMalloc(out, n, hipHostMallocDefault));
    std::lock_guard<std::mutex> lock(g_spans_mutex);
    g_spans[reinterpret_cast<uintptr_t>(*out)] = n;
    return DSWX_OK;
}

int dswx_host_free(dswx_ctx_t* ctx, void* ptr) {
    // ctx may be NULL: a span can outlive the context it was allocated through (a host array still alive when its
    // context is destroyed); page-locked host memory is not tied to the current device
    if (!ptr) return DSWX_OK;
    {
        std::lock_guard<std::mutex> lock(g_spans_mutex);
        g_spans.erase(reinterpret_cast<uintptr_t>(ptr));
    }
    if (ctx) HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipHostFree(ptr));
    return DSWX_OK;
}

// Is `p` page-locked host memory HIP knows about (hipHostMalloc / hipHostRegister)?
static bool is_pinned_host(const void* p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();          // plain malloc memory: not an error for us
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

// The page-locked counter scratch of the context (zero copy: the kernels write it; staged pipeline: per-chunk counts),
// grown to `rows` x 3 counters
static int pipe_counters_reserve(dswx_ctx* ctx, size_t rows) {
    if (rows <= ctx->pipe_counters_cap) return DSWX_OK;
    if (ctx->pipe_counters) HIP_TRY(hipHostFree(ctx->pipe_counters));
    ctx->pipe_counters = nullptr; ctx->pipe_counters_cap = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ctx->pipe_counters), rows * 3 * sizeof(int64_t)));
    ctx->pipe_counters_cap = rows;
    return DSWX_OK;
}

// One staging slot of the two copying paths: the planes that are given, `px` pixels of each, back to back in ABI order,
// every plane rounded up to `round` bytes (a power of two); one 256-byte line for the counters behind them.
struct StageSlot {
    size_t off[DSWX_N_PLANES], o_cnt, bytes;
};
static StageSlot stage_layout(const dswx_planes_in_t* in, const dswx_planes_out_t* out, size_t px, size_t round) {
    StageSlot L;
    size_t off = 0;
    for (int i = 0; i < DSWX_N_PLANES; ++i) {
        L.off[i] = off;
        if (dswx_plane_get(DSWX_PLANES[i], in, out)) off += (px * DSWX_PLANES[i].bytes + round - 1) & ~(round - 1);
    }
    L.o_cnt = off;
    L.bytes = off + 256;
    return L;
}
// Queues on `s` the upload of `n` pixels from pixel `hoff` of every input plane into the slot at `base`, and points
// din / dout at the slot's planes
static int stage_upload(const StageSlot& L, char* base, const dswx_planes_in_t* in, const dswx_planes_out_t* out, size_t hoff,
                        size_t n, hipStream_t s, dswx_planes_in_t* din, dswx_planes_out_t* dout) {
    for (int i = 0; i < DSWX_N_PLANES; ++i) {
        const dswx_plane_desc& d = DSWX_PLANES[i];
        const char* h = dswx_plane_get(d, in, out);
        if (!h) continue;
        if (d.input) HIP_TRY(hipMemcpyAsync(base + L.off[i], h + hoff * d.bytes, n * d.bytes, hipMemcpyHostToDevice, s));
        dswx_plane_set(d, din, dout, base + L.off[i]);
    }
    return DSWX_OK;
}
// ... and the way back: `n` pixels of every output plane from the slot to pixel `hoff` of the host plane
static int stage_download(const StageSlot& L, const char* base, const dswx_planes_out_t* out, size_t hoff, size_t n,
                          hipStream_t s) {
    for (int i = 0; i < DSWX_N_PLANES; ++i) {
        const dswx_plane_desc& d = DSWX_PLANES[i];
        char* h = d.input ? nullptr : dswx_plane_get(d, nullptr, out);
        if (h) HIP_TRY(hipMemcpyAsync(h + hoff * d.bytes, base + L.off[i], n * d.bytes, hipMemcpyDeviceToHost, s));
    }
    return DSWX_OK;
}

// Zero-copy host path.  Page-locked host memory is mapped into the device's address space, so the
// device-pointer entry can be handed the host planes as they are: the fused kernel's streaming loads become
// PCIe reads, its streaming stores PCIe writes, and the link runs in both directions for the whole launch --
// no staging buffers in HBM, no chunking, no copy engine hand-offs, and every mode (also 'cover': its scratch
// planes stay in HBM, only the inputs and the finished layers cross the link) takes the same path.
static int classify_host_zero_copy(dswx_ctx_t* ctx, const dswx_params_t* params, int64_t n_tiles, int64_t height,
                                   int64_t width, const dswx_planes_in_t* in, const dswx_planes_out_t* out,
                                   int64_t* counters) {
    hipError_t err = hipSuccess;
    auto dev = [&](const void* h) -> void* {
        void* d = nullptr;
        if (h && err == hipSuccess) err = hipHostGetDevicePointer(&d, const_cast<void*>(h), 0);
        return d;
    };
    dswx_planes_in_t din{};
    dswx_planes_out_t dout{};
    for (const dswx_plane_desc& d : DSWX_PLANES) dswx_plane_set(d, &din, &dout, dev(dswx_plane_get(d, in, out)));
    if (err != hipSuccess) return dswx_fail(DSWX_ERR_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(err));
    int64_t* dcnt = nullptr;
    if (counters) {          // the caller's counters may be pageable: a page-locked span of the context receives them
        if (int rc = pipe_counters_reserve(ctx, (size_t)n_tiles)) return rc;
        dcnt = static_cast<int64_t*>(dev(ctx->pipe_counters));
        if (err != hipSuccess) return dswx_fail(DSWX_ERR_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(err));
    }
    const int rc = dswx_classify_device_2d(ctx, params, n_tiles, height, width, &din, &dout, dcnt, ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (counters) std::memcpy(counters, ctx->pipe_counters, (size_t)n_tiles * 3 * sizeof(int64_t));
    ctx->last_kernel += " on page-locked host planes (zero copy across PCIe)";
    return DSWX_OK;
}

// Pipelined host path (lab A/B since the zero-copy path: host_pipeline = 1): every tile is cut into `host_chunks` flat pixel ranges (the chain is
// per pixel, so any cut is legal outside 'cover' mode) that flow through three device slots:
// chunk c+1 uploads on the H2D stream while chunk c is classified on the compute stream and
// chunk c-1 downloads on the D2H stream.  Needs page-locked host buffers (dswx_host_alloc or
// hipHostRegister), otherwise the copies are not asynchronous.  Counters are summed per tile
// on the host from per-chunk partial counts.
static int classify_host_pipelined(dswx_ctx_t* ctx, const dswx_params_t* params, int64_t n_tiles, int64_t P,
                                   const dswx_planes_in_t* in, const dswx_planes_out_t* out, int64_t* counters) {
    constexpr int NSLOT = 3;
    if (!ctx->h2d_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->h2d_stream, hipStreamNonBlocking));
    if (!ctx->d2h_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->d2h_stream, hipStreamNonBlocking));
    for (int i = 0; i < NSLOT; ++i) {
        if (!ctx->pipe_in[i]) HIP_TRY(hipEventCreateWithFlags(&ctx->pipe_in[i], hipEventDisableTiming));
        if (!ctx->pipe_k[i]) HIP_TRY(hipEventCreateWithFlags(&ctx->pipe_k[i], hipEventDisableTiming));
        if (!ctx->pipe_out[i]) HIP_TRY(hipEventCreateWithFlags(&ctx->pipe_out[i], hipEventDisableTiming));
    }
    // chunk size: a multiple of 2048 pixels (one block of the fused kernel), >= 64 Ki pixels
    int64_t chunk = (P + ctx->host_chunks - 1) / ctx->host_chunks;
    if (chunk < 65536) chunk = 65536;
    chunk = (chunk + 2047) / 2048 * 2048;
    const int64_t per_tile = (P + chunk - 1) / chunk;
    const int64_t n_chunks = per_tile * n_tiles;
    if (int rc = pipe_counters_reserve(ctx, (size_t)n_chunks)) return rc;
    // (no rounding: every plane of a slot is 256-byte aligned because chunk % 2048 == 0)
    const StageSlot L = stage_layout(in, out, (size_t)chunk, 1);
    dswx_workspace& stage = ctx->ws[dswx_ctx::WS_STAGE];
    if (int rc = dswx_ws_reserve(stage, L.bytes * NSLOT, nullptr, true)) return rc;
    char* const arena = static_cast<char*>(stage.p);
    hipStream_t sc = ctx->stream, sh = ctx->h2d_stream, sd = ctx->d2h_stream;
    bool slot_used[NSLOT] = {false, false, false};
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int slot = (int)(c % NSLOT);
        const int64_t tile = c / per_tile, px0 = (c % per_tile) * chunk;
        const int64_t n = (P - px0 < chunk) ? P - px0 : chunk;
        const size_t hoff = (size_t)tile * (size_t)P + (size_t)px0;
        char* base = arena + L.bytes * slot;
        dswx_planes_in_t din{};
        dswx_planes_out_t dout{};
        // ---- upload (after the slot's previous download finished)
        if (slot_used[slot]) HIP_TRY(hipStreamWaitEvent(sh, ctx->pipe_out[slot], 0));
        if (int rc = stage_upload(L, base, in, out, hoff, (size_t)n, sh, &din, &dout)) return rc;
        HIP_TRY(hipEventRecord(ctx->pipe_in[slot], sh));
        // ---- classify
        int64_t* dcnt = counters ? reinterpret_cast<int64_t*>(base + L.o_cnt) : nullptr;
        HIP_TRY(hipStreamWaitEvent(sc, ctx->pipe_in[slot], 0));
        const int rc = dswx_classify_device(ctx, params, 1, n, &din, &dout, dcnt, sc);
        if (rc) { (void)hipDeviceSynchronize(); return rc; }
        HIP_TRY(hipEventRecord(ctx->pipe_k[slot], sc));
        // ---- download
        HIP_TRY(hipStreamWaitEvent(sd, ctx->pipe_k[slot], 0));
        if (int drc = stage_download(L, base, out, hoff, (size_t)n, sd)) return drc;
        if (counters)
            HIP_TRY(hipMemcpyAsync(ctx->pipe_counters + c * 3, dcnt, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, sd));
        HIP_TRY(hipEventRecord(ctx->pipe_out[slot], sd));
        slot_used[slot] = true;
    }
    HIP_TRY(hipStreamSynchronize(sd));
    HIP_TRY(hipStreamSynchronize(sc));
    HIP_TRY(hipStreamSynchronize(sh));
    if (counters)
        for (int64_t t = 0; t < n_tiles; ++t)
            for (int j = 0; j < 3; ++j) {
                int64_t sum = 0;
                for (int64_t q = 0; q < per_tile; ++q) sum += ctx->pipe_counters[(t * per_tile + q) * 3 + j];
                counters[t * 3 + j] = sum;
            }
    ctx->last_kernel += " x" + std::to_string(n_chunks) + " chunks, pipelined over 3 streams (pinned host buffers)";
    return DSWX_OK;
}

int dswx_classify_host(dswx_ctx_t* ctx, const dswx_params_t* params, int64_t n_tiles, int64_t height,
                       int64_t width, const dswx_planes_in_t* in, const dswx_planes_out_t* out,
                       int64_t* counters) {
    if (!ctx || !params || !in || !out) return dswx_fail(DSWX_ERR_ARG, "NULL argument");
    if (n_tiles < 0 || height < 0 || width < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    for (int k = 0; k < 6; ++k)
        if (!in->band[k]) return dswx_fail(DSWX_ERR_ARG, "band[%d] is NULL", k);
    if (!in->fmask) return dswx_fail(DSWX_ERR_ARG, "fmask is NULL");
    {   // validate parameters before touching the device
        DevParams tmp;
        int rc = dswx_make_dev_params(params, &tmp);
        if (rc) return rc;
    }
    const int64_t P = height * width;
    if (n_tiles == 0 || P == 0) return DSWX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->host_pipeline == 2 || (ctx->host_pipeline && params->mask_adjacent_to_cloud_mode != DSWX_ADJ_COVER)) {
        // zero copy (product): every plane inside a span of dswx_host_alloc; staged pipeline (lab): any page-locked
        // memory, first AND last byte of every plane
        const size_t npx = (size_t)n_tiles * (size_t)P;
        const bool own = ctx->host_pipeline == 2;
        auto ok_span = [&](const void* p, size_t bytes) {
            if (!p) return true;
            if (own) return in_own_span(p, bytes);
            return is_pinned_host(p) && is_pinned_host(static_cast<const char*>(p) + bytes - 1);
        };
        bool pinned = true;
        for (const dswx_plane_desc& d : DSWX_PLANES) pinned = pinned && ok_span(dswx_plane_get(d, in, out), npx * d.bytes);
        if (pinned && ctx->host_pipeline == 2) return classify_host_zero_copy(ctx, params, n_tiles, height, width, in, out, counters);
        if (pinned) return classify_host_pipelined(ctx, params, n_tiles, P, in, out, counters);
    }
    // (Page-locking pageable planes IN PLACE for the duration of the call -- hipHostRegister on page-merged ranges, then
    // the zero-copy path -- was built and measured in round 2: 4.5 - 5.2 ms instead of 10.7 ms per 3660^2 tile from plain
    // numpy arrays.  It is NOT used: about one run in twenty of the parity suite came back with a few wrong pixels in a
    // freshly allocated, never-touched output array.  Transiently registered user memory is not pinned the way
    // hipHostMalloc memory is (the driver follows the CPU page tables through MMU notifiers), and kernel WRITES into
    // pages that are being faulted in, migrated or collapsed underneath were not reliable.  Pageable planes are copied.)
    // pageable host buffers (or 'cover' mode): one tile at a time through a grow-only device
    // arena: planes at 256-byte aligned offsets so the vector kernel is always eligible
    hipStream_t s = ctx->stream;
    const StageSlot L = stage_layout(in, out, (size_t)P, 256);
    // (every tile below ends in hipStreamSynchronize(s), so nothing of this path is in flight here: the stream the
    // grow waits for is idle unless a caller's earlier work is still queued on it)
    dswx_workspace& stage = ctx->ws[dswx_ctx::WS_STAGE];
    if (int rc = dswx_ws_reserve(stage, L.bytes, s)) return rc;
    char* base = static_cast<char*>(stage.p);
    for (int64_t t = 0; t < n_tiles; ++t) {
        const size_t sh = (size_t)t * (size_t)P;
        dswx_planes_in_t din{};
        dswx_planes_out_t dout{};
        if (int rc = stage_upload(L, base, in, out, sh, (size_t)P, s, &din, &dout)) return rc;
        int64_t* dcnt = counters ? reinterpret_cast<int64_t*>(base + L.o_cnt) : nullptr;
        int rc = dswx_classify_device_2d(ctx, params, 1, height, width, &din, &dout, dcnt, s);
        if (rc) return rc;
        if (int drc = stage_download(L, base, out, sh, (size_t)P, s)) return drc;
        if (counters) HIP_TRY(hipMemcpyAsync(counters + t * 3, dcnt, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return DSWX_OK;
}

}  // extern "C"
