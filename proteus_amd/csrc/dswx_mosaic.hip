// dswx_mosaic.hip -- the tiles of a plane placed on one canvas and composited per canvas pixel (DSWX_HAS_MOSAIC, additive to
// ABI v7): a stack with placements.  include/dswx_hip.h "mosaic" states the definition; proteus_amd/mosaic.py is its numpy
// statement and dswx_mosaic_host below the scalar one.  The per-byte and per-pixel rule is dswx_stack_rule.h, unchanged and
// compiled for both sides, and the table, the unit, the stores and the checks of the outputs are dswx_stack_core.h, shared with
// the stack entries; what is here is geometry: which tiles cover a pixel.
//
// OWNERSHIP.  A workgroup of 256 threads owns a rectangle of the canvas, MOSAIC_ROWS = 4 rows x MOSAIC_COLS = 1024 columns,
// blocks numbered row-major along grid.x.  One wave owns each row, so "does tile t cover my row" is the same in every lane:
// the wave index goes through readfirstlane and the row test is a scalar branch.  A thread owns MOSAIC_PPT = 16 consecutive
// pixels of its row, a unit; a unit never straddles a canvas row, and the last unit of a row (canvas_w % 16 pixels) is stored
// element by element.  The state of a pixel stays in registers for the whole walk as in the stack kernel -- the packed uint64
// counts and the tile << 8 | byte word -- plus ONE covered bit, 16 bits per thread, which is all that `outside` needs.
//
// CULLING.  A block cannot walk 65535 tiles per pixel to find the few that touch it, so it walks the placement table in
// chunks of MOSAIC_CHUNK = 256: thread j tests tile c + j against the block's rectangle in 64-bit arithmetic (INT32_MIN and
// INT32_MAX are ordinary placements), and the survivors are compacted IN ORDER into a list in LDS: a ballot and a popcount of
// the lanes below give the position inside the wave, four wave totals in LDS the position of the wave.  Tile order is what
// `last` depends on, so the list is only ever appended to and consumed front to back.  The list holds MOSAIC_LIST = 512
// entries; it is consumed when the next chunk might not fit (more than 256 entries) and at the end, so a sparse table (random
// placements, a few survivors per chunk) still fills whole rounds of loads, and a dense one (every tile over the block) is
// consumed every second chunk.  Two barriers per chunk; none inside the walk.  The thread that culls a tile also does the
// 64-bit arithmetic of the walk ONCE per tile and block (MosaicEntry: the tile row and column of the rectangle's corner, which
// fit an int because the tile meets the rectangle, and the byte offset of that pixel): 24 bytes per entry, 12 KiB.
//
// THE WALK.  The list is consumed in rounds of MOSAIC_U = 8 entries: the 16-byte loads of the round are issued before the
// first is counted, as in the stack kernel, 128 bytes in flight per thread; the table of increments is the stack kernel's
// eight lane-indexed replicas (dswx_stack_core.h has the bank arithmetic).  For a list entry the unit of a lane is one of three
// cases.  Wholly inside the tile's columns: one unaligned 16-byte load and exactly the stack kernel's unit (gfx950 performs
// unaligned 16-byte global accesses in hardware).  Wholly outside, or the row not covered (the same in every lane): skipped.
// Cut by a tile edge: ALSO one 16-byte load, from the unit's first pixel on -- those 16 bytes leave the tile's row but they
// are bytes of the tile, except in front of its first byte or behind its last, where the tile's first or last 16 bytes are
// loaded instead and shifted into place.  So no load touches a byte outside the first height * width bytes of a tile, and
// every load is a vector load.  The bytes of the pixels that the tile does not cover are then replaced by a NEUTRAL byte, one
// that the spec does not count (about twenty instructions per cut unit), and the unit is counted as a whole one; only a
// spec in which all 256 bytes are observations takes the masked form of the unit, which zeroes the increments instead.  The pixels of a ragged last
// unit that lie beyond the canvas are not masked at all: their accumulators are never stored.  A tile of fewer than 16 bytes
// has no room for a vector load: such planes take an instantiation of their own (TINY) that walks the list byte by byte.
//
// WHERE THIS LEAVES THE ISSUE'S SKETCH, AND WHY (256 tiles of 3660 x 3660 at the identity placement, beside the stack kernel
// on the same bytes, 0.68 ms with every output).  The sketch loads "only the covered bytes" of a cut unit.  The first version
// did, byte by byte under unrolled predicates: 6.55 ms.  Every byte load was followed by its use, so a wave with ONE cut lane
// -- the ragged last unit of a 3660-pixel row is one -- paid up to 12 memory latencies per tile, one after the other.  One
// vector load per cut unit and a masked unit beside the whole one: 2.8 ms -- the wave still ran both forms of the unit for
// every tile, and the address arithmetic was 64-bit per lane and entry.  The arithmetic moved into the cull: 2.2 ms.  The
// neutral byte, and nothing at all for pixels beyond the canvas: 1.21 ms; a ragged canvas then costs nothing.  What is left against the stack kernel is the geometry in front of every unit, about 35
// instructions per entry and lane against the 98 of counting 16 bytes with `last`: two ds_read of the entry and five
// v_readfirstlane, the column of the unit and its clamps, three compares with their exec masks (covered at all, leaves the
// row, cut inside the canvas), two v_lshl_add_u64 for the address.  Measured: tools/mosaic_rate.py, DESIGN.md section 5.
#include <hip/hip_runtime.h>
#include <cstdio>

#include "dswx_stack_core.h"

namespace {

// the stack kernel's constants under the names that the text above and last_kernel use
constexpr int MOSAIC_BLOCK = STACK_BLOCK, MOSAIC_PPT = STACK_PPT, MOSAIC_U = STACK_U, MOSAIC_REPLICAS = STACK_REPLICAS;
constexpr int MOSAIC_ROWS = MOSAIC_BLOCK / 64;           // canvas rows of a block: one wave each
constexpr int MOSAIC_COLS = 64 * MOSAIC_PPT;             // canvas columns of a block
constexpr int MOSAIC_CHUNK = MOSAIC_BLOCK;               // placements tested per step
constexpr int MOSAIC_LIST = 2 * MOSAIC_CHUNK;            // surviving tiles held in LDS
constexpr int64_t MOSAIC_MAX_SIDE = 1LL << 30;

struct MosaicArgs {
    const unsigned char* plane;
    unsigned long long stride;                           // bytes between tiles
    unsigned long long n_elems;                          // height * width
    const int* place;                                    // [n_tiles][2] = row0, col0
    int n_tiles, height, width, canvas_h, canvas_w;
    unsigned nbx;                                        // blocks along a canvas row
    StackCoreArgs c;                                     // outputs and spec
    int outside;
    int neutral;                                         // a byte that is not an observation, -1 if every byte is one
};
static_assert(sizeof(MosaicArgs) <= 4096, "kernel arguments");

// The bytes of `w` whose bit of `mask` is not set replaced by the byte `neutral`: what a cut unit does to the pixels that the
// tile does not cover, where the spec has a byte that is not an observation -- the unit then counts as a whole one.
__device__ __forceinline__ u32x4 neutralise(const u32x4& w, unsigned mask, unsigned neutral) {
    const uint32_t splat = neutral * 0x01010101u;
    u32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t nib = (mask >> (4 * k)) & 0xfu;
        const uint32_t keep = ((nib * 0x00204081u) & 0x01010101u) * 0xffu;      // bit b of the nibble -> byte b, 0x00 or 0xff
        r[k] = (w[k] & keep) | (splat & ~keep);
    }
    return r;
}

// x clamped to 0 .. top (one v_med3_i32)
__device__ __forceinline__ int clamp_i(int x, int, int top) { return x < 0 ? 0 : (x > top ? top : x); }

// byte i of the result = byte i + d of `w`, zeros where there is none; d != 0, -15 .. 15
__device__ __forceinline__ u32x4 shift_bytes(const u32x4& w, int d) {
    uint64_t a = w[0] | ((uint64_t)w[1] << 32), b = w[2] | ((uint64_t)w[3] << 32);
    if (d > 0) {
        const int s = 8 * d;
        if (s >= 64) { a = b >> (s - 64); b = 0; }
        else { a = (a >> s) | (b << (64 - s)); b >>= s; }
    } else {
        const int s = -8 * d;
        if (s >= 64) { b = a << (s - 64); a = 0; }
        else { b = (b << s) | (a >> (64 - s)); a <<= s; }
    }
    return u32x4{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
}

// What the walk needs of a surviving tile, worked out ONCE per tile and block by the thread that culled it, so that the walk
// is 32-bit arithmetic: the tile row of the block's first row and the tile column of its first column -- both fit an int
// BECAUSE the tile meets the rectangle: -MOSAIC_ROWS < rr < height, -MOSAIC_COLS < cc < width -- and the byte offset of that
// (possibly virtual) tile pixel from the plane's address.
struct MosaicEntry {
    int t, rr, cc, unused;
};

// TINY: a tile has fewer than 16 bytes, so no 16-byte load fits into one (dswx_mosaic_launch chooses)
template <bool LATEST, bool TINY>
__global__ __launch_bounds__(MOSAIC_BLOCK, 3) void dswx_mosaic_k(const MosaicArgs a) {
    __shared__ __attribute__((aligned(16))) uint64_t tab[256 * MOSAIC_REPLICAS];
    __shared__ __attribute__((aligned(16))) MosaicEntry list_e[MOSAIC_LIST];
    __shared__ __attribute__((aligned(8))) long long list_base[MOSAIC_LIST];
    __shared__ int wave_hits[MOSAIC_ROWS];
    const uint64_t* const mine = stack_fill_table(tab, a.c);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the rectangle of the block, [Y0, Y1) x [X0, X1), and the unit of this thread: row Y, columns X .. X + nvalid - 1
    const unsigned by = blockIdx.x / a.nbx, bx = blockIdx.x - by * a.nbx;
    const long long Y0 = (long long)by * MOSAIC_ROWS, X0 = (long long)bx * MOSAIC_COLS;
    const long long Y1 = Y0 + MOSAIC_ROWS < a.canvas_h ? Y0 + MOSAIC_ROWS : a.canvas_h;
    const long long X1 = X0 + MOSAIC_COLS < a.canvas_w ? X0 + MOSAIC_COLS : a.canvas_w;
    const long long Y = Y0 + wave, X = X0 + (long long)lane * MOSAIC_PPT;
    const int nvalid = X >= a.canvas_w ? 0 : (a.canvas_w - X < MOSAIC_PPT ? (int)(a.canvas_w - X) : MOSAIC_PPT);
    const bool live = Y < a.canvas_h && nvalid > 0;
    const int lane16 = lane * MOSAIC_PPT;
    const unsigned real = (1u << nvalid) - 1u;                       // the pixels of the unit that are pixels of the canvas
    const long long wave_rows = (long long)wave * a.width;           // bytes from the block's first row to this wave's
    const uint32_t none = stack_latest_none(a.c.fill);
    uint64_t acc[MOSAIC_PPT];
    uint32_t latest[MOSAIC_PPT];
#pragma unroll
    for (int i = 0; i < MOSAIC_PPT; ++i) {
        acc[i] = 0;
        latest[i] = none;
    }
    unsigned covered = 0;                                            // bit i: some tile covers pixel i of the unit
    int n = 0;                                                       // entries of the list (the same in every thread)
    for (int c0 = 0;; c0 += MOSAIC_CHUNK) {
        if (c0 < a.n_tiles) {
            // cull: tile c0 + threadIdx.x against the rectangle, the survivors appended in tile order
            const int t = c0 + (int)threadIdx.x;
            long long r0 = 0, q0 = 0;
            bool hit = false;
            if (t < a.n_tiles) {
                r0 = a.place[2 * (size_t)t];
                q0 = a.place[2 * (size_t)t + 1];
                hit = a.height > 0 && a.width > 0 && r0 < Y1 && r0 + a.height > Y0 && q0 < X1 && q0 + a.width > X0;
            }
            const unsigned long long ballot = __ballot(hit);
            const int before = __popcll(ballot & ((1ull << lane) - 1ull));
            if (lane == 0) wave_hits[wave] = __popcll(ballot);
            __syncthreads();
            int at = n, total = 0;
#pragma unroll
            for (int w = 0; w < MOSAIC_ROWS; ++w) {
                const int h = wave_hits[w];
                at += w < wave ? h : 0;
                total += h;
            }
            if (hit) {
                const long long rr = Y0 - r0, cc = X0 - q0;
                list_e[at + before] = MosaicEntry{t, (int)rr, (int)cc, 0};
                list_base[at + before] = (long long)((unsigned long long)t * a.stride) + rr * a.width + cc;
            }
            n = __builtin_amdgcn_readfirstlane(n + total);          // at most (MOSAIC_LIST - MOSAIC_CHUNK) + MOSAIC_CHUNK
            __syncthreads();
        }
        const bool done = c0 + MOSAIC_CHUNK >= a.n_tiles;
        if (n > MOSAIC_LIST - MOSAIC_CHUNK || done) {
            // consume the list front to back, MOSAIC_U entries a round: the loads first, then the counting.  (The next
            // chunk writes the list only behind its first barrier, which every thread reaches after this walk.)
            if (live && !TINY) {
                for (int e0 = 0; e0 < n; e0 += MOSAIC_U) {
                    // the entries of the round (e0 is a multiple of MOSAIC_U: the reads stay inside the list, and what lies
                    // behind entry n - 1 is not used)
                    MosaicEntry ent[MOSAIC_U];
                    long long base[MOSAIC_U];
#pragma unroll
                    for (int j = 0; j < MOSAIC_U; ++j) {
                        ent[j] = list_e[e0 + j];
                        base[j] = list_base[e0 + j];
                    }
                    u32x4 v[MOSAIC_U];
                    unsigned m[MOSAIC_U];                            // the pixels of the unit that entry j covers
                    uint32_t tile[MOSAIC_U];
#pragma unroll
                    for (int j = 0; j < MOSAIC_U; ++j) {
                        v[j] = u32x4{0u, 0u, 0u, 0u};
                        m[j] = 0;
                        tile[j] = (uint32_t)__builtin_amdgcn_readfirstlane(ent[j].t);
                        const int r = __builtin_amdgcn_readfirstlane(ent[j].rr) + wave;      // the same in every lane
                        if (e0 + j < n && (unsigned)r < (unsigned)a.height) {
                            const int c = __builtin_amdgcn_readfirstlane(ent[j].cc) + lane16;  // tile column of pixel 0 of the unit
                            const int lo = clamp_i(-c, 0, MOSAIC_PPT);           // the unit's pixels lo .. hi - 1 are covered
                            const int hi = clamp_i(a.width - c, 0, nvalid);
                            if (lo < hi) {
                                const unsigned lo_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base[j]);
                                const unsigned hi_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)base[j] >> 32));
                                long long off = (long long)(((unsigned long long)hi_hi << 32) | lo_hi) + wave_rows + lane16;
                                int d = 0;
                                if (c < 0 || c + MOSAIC_PPT > a.width) {
                                    // the 16 bytes from byte (r, c) on leave the tile's row: they are still the tile's bytes
                                    // unless they begin in front of the tile or end behind it -- then the tile's first or last
                                    // 16 bytes are loaded and shifted into place
                                    const long long o = (long long)r * a.width + c;
                                    const long long last16 = (long long)a.n_elems - MOSAIC_PPT;
                                    const long long from = o < 0 ? 0 : (o > last16 ? last16 : o);
                                    d = (int)(o - from);
                                    off -= d;
                                }
                                u32x4 w = ldg_u<u32x4_b, u32x4, true>(a.plane + off);
                                if (d) w = shift_bytes(w, d);
                                const unsigned mask = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
                                covered |= mask;
                                m[j] = 0xffffu;
                                if (mask != real) {                  // a tile edge INSIDE the canvas cuts the unit
                                    if (a.neutral >= 0) w = neutralise(w, mask, (unsigned)a.neutral);
                                    else m[j] = mask;
                                }
                                v[j] = w;
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < MOSAIC_U; ++j) {
                        if (m[j] == 0xffffu) stack_unit<LATEST, false>(v[j], m[j], tile[j], mine, acc, latest);
                        else if (m[j]) stack_unit<LATEST, true>(v[j], m[j], tile[j], mine, acc, latest);
                    }
                }
            }
            if (live && TINY) {
                // tiles of fewer than 16 bytes: byte by byte, one entry after the other
#pragma unroll 1
                for (int e = 0; e < n; ++e) {
                    const MosaicEntry ent = list_e[e];
                    const int t = __builtin_amdgcn_readfirstlane(ent.t);
                    const int r = __builtin_amdgcn_readfirstlane(ent.rr) + wave;
                    if ((unsigned)r >= (unsigned)a.height) continue;             // the same in every lane
                    const int c = __builtin_amdgcn_readfirstlane(ent.cc) + lane16;
                    const int lo = clamp_i(-c, 0, MOSAIC_PPT);
                    const int hi = clamp_i(a.width - c, 0, nvalid);
                    if (lo < hi) {
                        const long long off = list_base[e] + wave_rows + lane16;
#pragma unroll
                        for (int i = 0; i < MOSAIC_PPT; ++i)
                            if (i >= lo && i < hi) {
                                const unsigned byte = a.plane[off + i];
                                stack_step(acc[i], latest[i], mine[byte * MOSAIC_REPLICAS], (uint32_t)t, byte);
                            }
                        covered |= ((1u << hi) - 1u) & ~((1u << lo) - 1u);
                    }
                }
            }
            n = 0;
        }
        if (done) break;
    }
    if (!live) return;
    const unsigned long long e = (unsigned long long)Y * (unsigned long long)a.canvas_w + (unsigned long long)X;
    const unsigned outside = (unsigned)a.outside;
#pragma unroll
    for (int k = 0; k < DSWX_STACK_MAX_CATS; ++k)
        if (a.c.count[k]) store_u16(a.c.count[k] + e, nvalid, [&](int i) { return stack_count(acc[i], k); });
    if (LATEST && a.c.last) store_u8(a.c.last + e, nvalid, [&](int i) { return ((covered >> i) & 1u) ? stack_last(latest[i]) : outside; });
    if (LATEST && a.c.last_index) store_u16(a.c.last_index + e, nvalid, [&](int i) { return stack_last_index(latest[i]); });
    if (a.c.share) store_u8(a.c.share + e, nvalid, [&](int i) { return stack_share(acc[i]); });
}

}  // namespace

// The checks that the device and the host entry share, in the house order: the arguments before any context, nothing
// written by a refused call.  `align` = the uint16 outputs must be 2-byte and the table 4-byte aligned (the device entry).
int dswx_mosaic_check(const uint8_t* plane, const dswx_mosaic_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                      int64_t* stride, const int32_t* place, int64_t canvas_h, int64_t canvas_w, const dswx_stack_out_t* out,
                      bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (int rc = stack_spec_check(spec->n_cats, spec->fill)) return rc;
    if (spec->outside < 0 || spec->outside > 255) return dswx_fail(DSWX_ERR_ARG, "outside %d outside 0 .. 255", spec->outside);
    if (spec->reserved != 0) return dswx_fail(DSWX_ERR_ARG, "reserved is %d, not 0", spec->reserved);
    if (n_tiles < 0 || height < 0 || width < 0 || *stride < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (canvas_h < 0 || canvas_w < 0) return dswx_fail(DSWX_ERR_ARG, "negative canvas size %lld x %lld", (long long)canvas_h, (long long)canvas_w);
    if (height > MOSAIC_MAX_SIDE || width > MOSAIC_MAX_SIDE) return dswx_fail(DSWX_ERR_ARG, "raster too large");
    if (canvas_h > MOSAIC_MAX_SIDE || canvas_w > MOSAIC_MAX_SIDE || (canvas_w && canvas_h > (1LL << 46) / canvas_w))
        return dswx_fail(DSWX_ERR_ARG, "canvas %lld x %lld too large", (long long)canvas_h, (long long)canvas_w);
    const int64_t n_elems = height * width;
    if (int rc = dswx_tile_stride_check(stride, n_elems)) return rc;
    if (int rc = stack_tiles_check(n_tiles)) return rc;
    if (int rc = dswx_tile_extent_check(*stride, n_tiles, false)) return rc;
    if (int rc = dswx_tile_plane_check(plane, n_tiles, n_elems)) return rc;
    if (!place && n_tiles > 0) return dswx_fail(DSWX_ERR_ARG, "place is NULL");
    if (int rc = stack_out_check(out, spec->n_cats, align)) return rc;
    if (align && !aligned_to(place, 4)) return dswx_fail(DSWX_ERR_ALIGN, "place not 4-byte aligned");
    return DSWX_OK;
}

// One launch; the arguments have passed dswx_mosaic_check (stride resolved).
int dswx_mosaic_launch(dswx_ctx* ctx, const uint8_t* plane, const dswx_mosaic_spec_t* spec, int64_t n_tiles, int64_t height,
                       int64_t width, int64_t stride, const int32_t* place, int64_t canvas_h, int64_t canvas_w,
                       const dswx_stack_out_t* out, hipStream_t s) {
    if (canvas_h == 0 || canvas_w == 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    const unsigned long long nbx = ((unsigned long long)canvas_w + MOSAIC_COLS - 1) / MOSAIC_COLS;
    const unsigned long long nby = ((unsigned long long)canvas_h + MOSAIC_ROWS - 1) / MOSAIC_ROWS;
    // (grid.x x 256 threads must stay below 2^32: the runtime refuses a larger launch)
    if (nbx * nby * MOSAIC_BLOCK >= (1ull << 32)) return dswx_fail(DSWX_ERR_ARG, "canvas too large for one launch");
    MosaicArgs a = {};
    a.plane = plane;
    a.stride = (unsigned long long)stride;
    a.n_elems = (unsigned long long)(height * width);
    a.place = place;
    a.n_tiles = (int)n_tiles;
    a.height = (int)height;
    a.width = (int)width;
    a.canvas_h = (int)canvas_h;
    a.canvas_w = (int)canvas_w;
    a.nbx = (unsigned)nbx;
    a.outside = spec->outside;
    a.neutral = -1;
    for (int b = 255; b >= 0; --b)
        if (spec->cat_of_byte[b] >= spec->n_cats) a.neutral = b;
    stack_core_args(a.c, out, spec->n_cats, spec->fill, spec->cat_of_byte);
    const bool latest = stack_wants_latest(out);
    const unsigned gx = (unsigned)(nbx * nby);
    const bool tiny = height * width < MOSAIC_PPT;      // no 16-byte load fits into a tile: the byte-by-byte instantiation
    if (latest && tiny) hipLaunchKernelGGL((dswx_mosaic_k<true, true>), dim3(gx), dim3(MOSAIC_BLOCK), 0, s, a);
    else if (latest) hipLaunchKernelGGL((dswx_mosaic_k<true, false>), dim3(gx), dim3(MOSAIC_BLOCK), 0, s, a);
    else if (tiny) hipLaunchKernelGGL((dswx_mosaic_k<false, true>), dim3(gx), dim3(MOSAIC_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((dswx_mosaic_k<false, false>), dim3(gx), dim3(MOSAIC_BLOCK), 0, s, a);
    HIP_TRY(hipGetLastError());
    char info[256];
    snprintf(info, sizeof info, "dswx_mosaic_k grid=(%u,1,1) block=%d rect=%dx%d pixels_per_thread=%d tiles_in_flight=%d list=%d replicas=%d latest=%d tiny=%d",
             gx, MOSAIC_BLOCK, MOSAIC_ROWS, MOSAIC_COLS, MOSAIC_PPT, MOSAIC_U, MOSAIC_LIST, MOSAIC_REPLICAS, latest ? 1 : 0, tiny ? 1 : 0);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_mosaic_host(const uint8_t* plane, const dswx_mosaic_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                     int64_t stride, const int32_t* place, int64_t canvas_h, int64_t canvas_w, const dswx_stack_out_t* out) {
    if (int rc = dswx_mosaic_check(plane, spec, n_tiles, height, width, &stride, place, canvas_h, canvas_w, out, false)) return rc;
    if (height == 0 || width == 0) n_tiles = 0;          // an empty raster covers nothing
    uint64_t inc_of[256];
    for (int b = 0; b < 256; ++b) inc_of[b] = stack_increment(spec->cat_of_byte, spec->n_cats, (unsigned)b);
    constexpr int64_t CHUNK = 4096;                      // pixels of a canvas row whose state is walked through the tiles together
    uint64_t acc[CHUNK];
    uint32_t latest[CHUNK];
    bool covered[CHUNK];
    for (int64_t Y = 0; Y < canvas_h; ++Y)
        for (int64_t X0 = 0; X0 < canvas_w; X0 += CHUNK) {
            const int64_t n = canvas_w - X0 < CHUNK ? canvas_w - X0 : CHUNK;
            for (int64_t i = 0; i < n; ++i) {
                acc[i] = 0;
                latest[i] = stack_latest_none(spec->fill);
                covered[i] = false;
            }
            for (int64_t t = 0; t < n_tiles; ++t) {
                const int64_t r = Y - dswx_load<int32_t>(place, (size_t)(2 * t)), q0 = dswx_load<int32_t>(place, (size_t)(2 * t + 1));
                if (r < 0 || r >= height) continue;
                const int64_t xa = q0 > X0 ? q0 : X0, xb = q0 + width < X0 + n ? q0 + width : X0 + n;
                const uint8_t* row = plane + (size_t)t * (size_t)stride + (size_t)(r * width);
                for (int64_t x = xa; x < xb; ++x) {
                    const uint8_t byte = row[x - q0];
                    stack_step(acc[x - X0], latest[x - X0], inc_of[byte], (uint32_t)t, byte);
                    covered[x - X0] = true;
                }
            }
            const int64_t e0 = Y * canvas_w + X0;
            for (int64_t i = 0; i < n; ++i)
                stack_put_pixel(out, e0 + i, acc[i], latest[i], covered[i] ? stack_last(latest[i]) : (unsigned)spec->outside);
        }
    return DSWX_OK;
}

int dswx_mosaic_device(dswx_ctx_t* ctx, const uint8_t* plane, const dswx_mosaic_spec_t* spec, int64_t n_tiles, int64_t height,
                       int64_t width, int64_t stride, const int32_t* place, int64_t canvas_h, int64_t canvas_w,
                       const dswx_stack_out_t* out, void* stream) {
    if (int rc = dswx_mosaic_check(plane, spec, n_tiles, height, width, &stride, place, canvas_h, canvas_w, out, true)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) {
        return dswx_mosaic_launch(ctx, plane, spec, n_tiles, height, width, stride, place, canvas_h, canvas_w, out, s);
    });
}

}  // extern "C"
