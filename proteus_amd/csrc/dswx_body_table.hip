// dswx_body_table.hip -- the labelled bodies of a plane renumbered 1 .. K and tabulated, one 64-byte row per body
// (DSWX_HAS_BODY_TABLE, additive to ABI v7), without the label plane crossing PCIe.  include/dswx_hip.h "body table" states the
// definition; proteus_amd/bodies.py is its numpy statement and dswx_body_table_host below the scalar one -- dswx_body_rule.h
// is compiled for both sides.
//
// The first entry whose OUTPUT SIZE depends on the data: the row of a body is its rank among the roots, so a device-wide
// prefix sum over the roots comes first and a scatter into the rows last.  `dense` is the working array of the prefix sum:
// between launches 1 and 3 the first element of every chunk of CHUNK = 4096 elements holds that chunk's partial, and nothing
// else of it is defined.
//
// NO WORKGROUP EVER WAITS FOR ANOTHER: no decoupled look-back, no flag, no spin, no cooperative launch.  The prefix sum is
// reduce, scan of the partials, apply, as successive launches on the stream.  EVERY LOOP HAS A STATIC TRIP COUNT (the tiles of
// a grid column, the steps of the scan, 16 elements, the shuffle distances, PEEL rounds).
//   1 dswx_body_count_k   a workgroup owns a chunk of one tile, a thread 16 consecutive elements (16-byte loads): the roots
//                         (label == index + 1) of the chunk are counted and the count stored at dense[first element of the
//                         chunk].
//   2 dswx_body_scan_k    one workgroup per tile turns those counts into exclusive prefix sums IN PLACE, SCAN_STEP = 256 chunks
//                         per step with a running carry, and writes K and min(K, max_rows) into the head.
//   3 dswx_body_rank_k    reads the chunk's prefix BEFORE anything of the chunk is overwritten (one thread, then a barrier),
//                         scans the root counts of its threads, stores dense = 1 + rank at every root and begins the root's
//                         row: label, y_min = (label - 1) / width, and x_min = 0xFFFFFFFF so that atomicMin has its identity
//                         (everything else of the row is the memset's zero).
//   4 dswx_body_fill_k    the hot launch.  A workgroup owns a RECTANGLE of 32 x 128 pixels of one tile (so that the row
//                         segments of a body that lie below each other meet in one workgroup), a thread 16 consecutive
//                         pixels of a row: its 16 labels, the 16 above and the 16 below (a re-read that hits the Infinity
//                         Cache), the two beside, and 16 value bytes.  Per RUN of equal labels it checks the bound, then loads
//                         label[L - 1] and dense[L - 1] together: well-formed iff the first is L, and the second is then the
//                         dense value.  It walks its pixels once, accumulating area, edge count, category counts, coordinate
//                         sums and the x range of the current run, all RELATIVE to the rectangle (32 bits hold them); the run
//                         that ENDS at element i is handed in at step i by every lane at once: PEEL rounds pick the first lane
//                         that still has a run and sum every lane with the same body into that lane (y_max is the row of the
//                         LAST matching lane: rows rise with the lane); a leader nobody shares a body with skips the sums.
//                         The leaders, and what is left, add to the WORKGROUP'S TABLE in LDS: 256 slots, the slot of a body by
//                         a hash of its dense value, claimed by compare-and-swap; a body whose slot is another's goes straight
//                         to its row.  After a barrier one thread per used slot sends ONE set of atomicAdd / atomicMin /
//                         atomicMax (32- and 64-bit) to the row, with the rectangle's origin added in 64 bits.  A lake
//                         interior is one set of atomics per 4096 pixels, a shoreline one per rectangle it crosses.  dense is
//                         stored for the thread's pixels; the head's three sums go through LDS.
// A root's dense value is rewritten by launch 4 with the value launch 3 stored, while other threads read it: the same bytes.
// DESIGN.md section 5 has the bytes per pixel of each launch and what was measured.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#include "dswx_host.h"
#include "dswx_body_rule.h"

namespace {

typedef u32x4 __attribute__((aligned(1))) body_u32x4_b;  // 16 bytes anywhere (the value plane)
typedef u32x4 __attribute__((aligned(4))) body_u32x4_w;  // four uint32 at a 4-byte address (label, dense)

constexpr int BODY_BLOCK = 256;
constexpr int BODY_PPT = 16;                             // elements of a thread
constexpr int BODY_WAVES = BODY_BLOCK / 64;
constexpr int BODY_PEEL = 2;                             // rounds of wave-wide combining per run slot (launch 4)
constexpr int BODY_CHUNK = DSWX_BODY_CHUNK;
constexpr int BODY_RECT_H = DSWX_BODY_RECT_H, BODY_RECT_W = DSWX_BODY_RECT_W;   // the rectangle of a workgroup in launch 4
constexpr int BODY_SEGS = BODY_RECT_W / BODY_PPT;        // threads along a row of the rectangle
constexpr int BODY_SLOT_BITS = 8, BODY_SLOTS = 1 << BODY_SLOT_BITS;              // bodies in a workgroup's table in LDS: 11 KiB
static_assert(BODY_SLOTS <= BODY_BLOCK, "a thread resets and flushes at most one slot");
static_assert(BODY_RECT_H * BODY_SEGS == BODY_BLOCK, "one thread per 16 pixels of the rectangle");
constexpr int64_t BODY_MAX_PIXELS = 1LL << 31;
constexpr int64_t BODY_MAX_ROWS = 1LL << 31;
static_assert(BODY_BLOCK * BODY_PPT == BODY_CHUNK, "a workgroup's threads cover a chunk");
static_assert(DSWX_BODY_SCAN_STEP == BODY_BLOCK, "the scan launch takes one partial per thread and step");
static_assert(BODY_BLOCK == 256, "the category table is copied one byte per thread");

struct BodyArgs {
    const unsigned* label;
    const unsigned char* value;                          // nullptr: n_cats == 0
    unsigned long long vstride;                          // bytes between tiles of value
    unsigned long long n_elems;                          // height * width <= 2^31
    long long n_tiles;
    unsigned height, width;
    unsigned chunks;                                     // per tile, <= 2^19
    unsigned rx, ry;                                     // rectangles across / down (launch 4)
    int n_cats;
    unsigned long long max_rows;                         // <= 2^31
    unsigned* dense;
    unsigned* rows;                                      // nullptr: not wanted or max_rows == 0
    unsigned long long* head;
    unsigned char cat[256];
};

__device__ __forceinline__ unsigned body_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned body_wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned u = __shfl_xor(v, o);
        v = u < v ? u : v;
    }
    return v;
}
__device__ __forceinline__ unsigned body_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    return v;
}
// the inclusive prefix sum of v over the lanes of a wave
__device__ __forceinline__ unsigned body_wave_scan(unsigned v, unsigned lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o);
        if (lane >= (unsigned)o) v += u;
    }
    return v;
}

// The 16 elements at `first` of a uint32 plane of n elements (launches 1 and 3: a tile as a flat run); an element outside
// [0, n) reads as 0 and is never loaded.
__device__ __forceinline__ void body_load16(const unsigned* plane, long long first, long long n, unsigned (&v)[BODY_PPT]) {
    if (first >= 0 && first + BODY_PPT <= n) {
#pragma unroll
        for (int i = 0; i < BODY_PPT; i += 4) {
            const u32x4 q = *reinterpret_cast<const body_u32x4_w*>(plane + first + i);
            v[i] = q.x, v[i + 1] = q.y, v[i + 2] = q.z, v[i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < BODY_PPT; ++i) v[i] = first + i >= 0 && first + i < n ? plane[first + i] : 0u;
    }
}
__device__ __forceinline__ void body_store16(unsigned* plane, long long first, long long n, const unsigned (&v)[BODY_PPT]) {
    if (first + BODY_PPT <= n) {
#pragma unroll
        for (int i = 0; i < BODY_PPT; i += 4) *reinterpret_cast<body_u32x4_w*>(plane + first + i) = u32x4{v[i], v[i + 1], v[i + 2], v[i + 3]};
    } else {
#pragma unroll
        for (int i = 0; i < BODY_PPT; ++i)
            if (first + i < n) plane[first + i] = v[i];
    }
}
// bit i: element first + i is a root (an element behind the tile was read as 0: never a root)
__device__ __forceinline__ unsigned body_root_mask(const unsigned (&v)[BODY_PPT], unsigned long long first) {
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < BODY_PPT; ++i)
        if (body_is_root(v[i], first + i)) m |= 1u << i;
    return m;
}

// ---- launch 1: the roots of every chunk -------------------------------------------------------------------------------------
__global__ __launch_bounds__(BODY_BLOCK) void dswx_body_count_k(const BodyArgs a) {
    __shared__ unsigned wtot[BODY_WAVES];
    const unsigned long long chunk_first = (unsigned long long)blockIdx.x * BODY_CHUNK;          // < n_elems: chunks = ceil
    const unsigned long long first = chunk_first + (unsigned long long)threadIdx.x * BODY_PPT;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        unsigned c = 0;
        if (first < a.n_elems) {
            unsigned v[BODY_PPT];
            body_load16(a.label + (unsigned long long)t * a.n_elems, (long long)first, (long long)a.n_elems, v);
            c = __popc(body_root_mask(v, first));
        }
        c = body_wave_sum(c);
        if (lane == 0) wtot[wave] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned sum = 0;
#pragma unroll
            for (int w = 0; w < BODY_WAVES; ++w) sum += wtot[w];
            a.dense[(unsigned long long)t * a.n_elems + chunk_first] = sum;
        }
        __syncthreads();                                 // (wtot is written again for the next tile)
    }
}

// ---- launch 2: the chunk counts of a tile become exclusive prefix sums, in place ----------------------------------------------
__global__ __launch_bounds__(BODY_BLOCK) void dswx_body_scan_k(const BodyArgs a) {
    __shared__ unsigned wtot[BODY_WAVES];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (long long t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        unsigned* const d = a.dense + (unsigned long long)t * a.n_elems;
        unsigned carry = 0;                              // the roots of the chunks before `base` (<= 2^31)
        for (unsigned base = 0; base < a.chunks; base += DSWX_BODY_SCAN_STEP) {                  // ceil(chunks / 256) steps
            const unsigned c = base + threadIdx.x;
            const unsigned val = c < a.chunks ? d[(unsigned long long)c * BODY_CHUNK] : 0u;
            const unsigned inc = body_wave_scan(val, lane);
            if (lane == 63) wtot[wave] = inc;
            __syncthreads();
            unsigned before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < BODY_WAVES; ++w) {
                if ((unsigned)w < wave) before += wtot[w];
                total += wtot[w];
            }
            if (c < a.chunks) d[(unsigned long long)c * BODY_CHUNK] = carry + before + inc - val;
            carry += total;
            __syncthreads();                             // (wtot is written again in the next step)
        }
        if (threadIdx.x == 0 && a.head) {
            a.head[(unsigned long long)t * DSWX_BODY_HEAD_WORDS + BODY_HEAD_K] = carry;
            a.head[(unsigned long long)t * DSWX_BODY_HEAD_WORDS + BODY_HEAD_ROWS] = carry < a.max_rows ? carry : a.max_rows;
        }
    }
}

// ---- launch 3: the rank of every root, and the beginning of its row ---------------------------------------------------------
__global__ __launch_bounds__(BODY_BLOCK) void dswx_body_rank_k(const BodyArgs a) {
    __shared__ unsigned wtot[BODY_WAVES];
    __shared__ unsigned chunk_base;
    const unsigned long long chunk_first = (unsigned long long)blockIdx.x * BODY_CHUNK;
    const unsigned long long first = chunk_first + (unsigned long long)threadIdx.x * BODY_PPT;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        unsigned* const d = a.dense + (unsigned long long)t * a.n_elems;
        unsigned m = 0;
        if (first < a.n_elems) {
            unsigned v[BODY_PPT];
            body_load16(a.label + (unsigned long long)t * a.n_elems, (long long)first, (long long)a.n_elems, v);
            m = body_root_mask(v, first);
        }
        // the prefix of this chunk lies in its first element, which only this workgroup writes in this launch, and only
        // behind the barrier below
        if (threadIdx.x == 0) chunk_base = d[chunk_first];
        const unsigned c = __popc(m);
        const unsigned inc = body_wave_scan(c, lane);
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        unsigned rank = chunk_base + inc - c;
#pragma unroll
        for (int w = 0; w < BODY_WAVES; ++w)
            if ((unsigned)w < wave) rank += wtot[w];
        __syncthreads();                                 // (every thread has read chunk_base and wtot)
#pragma unroll
        for (int i = 0; i < BODY_PPT; ++i)
            if ((m >> i) & 1u) {
                const unsigned p = (unsigned)(first + i);                    // (a root lies inside the tile: p < 2^31)
                d[p] = rank + 1u;
                if (a.rows && rank < a.max_rows) {
                    unsigned* const row = a.rows + ((unsigned long long)t * a.max_rows + rank) * DSWX_BODY_ROW_WORDS;
                    row[BODY_LABEL] = p + 1u;
                    row[BODY_X_MIN] = 0xFFFFFFFFu;
                    row[BODY_Y_MIN] = p / a.width;
                }
                ++rank;
            }
    }
}

// ---- launch 4: dense for every element, the rows, the head ------------------------------------------------------------------
// One combined contribution of a body (dense value dv >= 1) to its row, if it has one.
__device__ __forceinline__ void body_emit(const BodyArgs& a, long long t, unsigned dv, unsigned area, unsigned perimeter,
                                          unsigned long long sum_x, unsigned long long sum_y, unsigned x_min, unsigned x_max,
                                          unsigned y_max, unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
    if ((unsigned long long)(dv - 1u) >= a.max_rows) return;                 // truncated: no row, never another body's
    unsigned* const row = a.rows + ((unsigned long long)t * a.max_rows + (dv - 1u)) * DSWX_BODY_ROW_WORDS;
    atomicAdd(row + BODY_AREA, area);
    atomicMin(row + BODY_X_MIN, x_min);
    atomicMax(row + BODY_X_MAX, x_max);
    atomicMax(row + BODY_Y_MAX, y_max);
    atomicAdd(reinterpret_cast<unsigned long long*>(row + BODY_PERIMETER), (unsigned long long)perimeter);
    atomicAdd(reinterpret_cast<unsigned long long*>(row + BODY_SUM_X), sum_x);
    atomicAdd(reinterpret_cast<unsigned long long*>(row + BODY_SUM_Y), sum_y);
    if (c0) atomicAdd(row + BODY_COUNT + 0, c0);
    if (c1) atomicAdd(row + BODY_COUNT + 1, c1);
    if (c2) atomicAdd(row + BODY_COUNT + 2, c2);
    if (c3) atomicAdd(row + BODY_COUNT + 3, c3);
}

// The workgroup's table in LDS: BODY_SLOTS bodies, each the sums of the workgroup's rectangle RELATIVE to the rectangle's
// origin (at most 4096 pixels of at most 127 and 31: 32 bits hold them), flushed to the rows once per workgroup.
constexpr int SLOT_AREA = 0, SLOT_PER = 1, SLOT_SX = 2, SLOT_SY = 3, SLOT_X_MIN = 4, SLOT_X_MAX = 5, SLOT_Y_MAX = 6, SLOT_COUNT = 7,
              SLOT_WORDS = 11;
struct BodyPiece {                                       // a contribution inside the rectangle; x and y are relative
    unsigned area, per, sx, sy, x_min, x_max, y_max, c01, c23;
};
// Adds a piece to the slot of its body; false when the slot belongs to another body (the caller then goes to the row itself).
__device__ __forceinline__ bool body_slot_add(unsigned* key, unsigned (*acc)[SLOT_WORDS], unsigned dv, const BodyPiece& q) {
    const unsigned s = (dv * 2654435761u) >> (32 - BODY_SLOT_BITS);
    const unsigned old = atomicCAS(key + s, 0u, dv);
    if (old != 0u && old != dv) return false;
    atomicAdd(&acc[s][SLOT_AREA], q.area);
    atomicAdd(&acc[s][SLOT_PER], q.per);
    atomicAdd(&acc[s][SLOT_SX], q.sx);
    atomicAdd(&acc[s][SLOT_SY], q.sy);
    atomicMin(&acc[s][SLOT_X_MIN], q.x_min);
    atomicMax(&acc[s][SLOT_X_MAX], q.x_max);
    atomicMax(&acc[s][SLOT_Y_MAX], q.y_max);
    if (q.c01 & 0xffffu) atomicAdd(&acc[s][SLOT_COUNT + 0], q.c01 & 0xffffu);
    if (q.c01 >> 16) atomicAdd(&acc[s][SLOT_COUNT + 1], q.c01 >> 16);
    if (q.c23 & 0xffffu) atomicAdd(&acc[s][SLOT_COUNT + 2], q.c23 & 0xffffu);
    if (q.c23 >> 16) atomicAdd(&acc[s][SLOT_COUNT + 3], q.c23 >> 16);
    return true;
}

// up to 16 elements of a row at a 4-byte address; those from nv on are 0 and not loaded
__device__ __forceinline__ void body_load_row16(const unsigned* p, int nv, unsigned (&v)[BODY_PPT]) {
    if (nv == BODY_PPT) {
#pragma unroll
        for (int i = 0; i < BODY_PPT; i += 4) {
            const u32x4 q = *reinterpret_cast<const body_u32x4_w*>(p + i);
            v[i] = q.x, v[i + 1] = q.y, v[i + 2] = q.z, v[i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < BODY_PPT; ++i) v[i] = i < nv ? p[i] : 0u;
    }
}

__global__ __launch_bounds__(BODY_BLOCK) void dswx_body_fill_k(const BodyArgs a) {
    __shared__ unsigned char cat[256];
    __shared__ unsigned long long part[3];
    __shared__ unsigned key[BODY_SLOTS];
    __shared__ unsigned acc[BODY_SLOTS][SLOT_WORDS];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    cat[tid] = (unsigned char)body_cat(a.cat[tid], a.n_cats);
    // the workgroup's rectangle of BODY_RECT_H x BODY_RECT_W pixels and the thread's 16 pixels of one row of it
    const unsigned ryi = blockIdx.x / a.rx, rxi = blockIdx.x - ryi * a.rx;
    const unsigned lr = tid / BODY_SEGS, seg = tid - lr * BODY_SEGS;
    const unsigned rect_y = ryi * BODY_RECT_H, rect_x = rxi * BODY_RECT_W;
    const unsigned y = rect_y + lr, x0 = rect_x + seg * BODY_PPT;
    const unsigned W = a.width, H = a.height;
    const int nv = y < H && x0 < W ? (W - x0 < (unsigned)BODY_PPT ? (int)(W - x0) : BODY_PPT) : 0;
    const unsigned long long first = (unsigned long long)y * W + x0;        // (inside the tile where nv > 0)
    // (no thread leaves early: the wave-wide steps below need every lane; a thread outside the raster has no pixel)
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        if (tid < 3) part[tid] = 0ull;
        if (tid < BODY_SLOTS) {
            key[tid] = 0u;
#pragma unroll
            for (int w = 0; w < SLOT_WORDS; ++w) acc[tid][w] = w == SLOT_X_MIN ? 0xFFFFFFFFu : 0u;
        }
        __syncthreads();                                 // (the category table the first time, the partials and slots every time)
        const unsigned* const lab = a.label + (unsigned long long)t * a.n_elems;
        unsigned* const den = a.dense + (unsigned long long)t * a.n_elems;
        unsigned r[BODY_PPT], d[BODY_PPT];
        unsigned ud = 0;                                 // two bits per element: its edges upward and downward
        unsigned before = 0, after = 0;                  // the labels beside the thread's elements
        u32x4 vb = u32x4{0u, 0u, 0u, 0u};
        unsigned good = 0, bad = 0, edges = 0;
        if (nv > 0) {
            body_load_row16(lab + first, nv, r);
            {
                unsigned o[BODY_PPT];
                if (y > 0) body_load_row16(lab + first - W, nv, o);
#pragma unroll
                for (int i = 0; i < BODY_PPT; ++i) ud += (y == 0 || o[i] != r[i] ? 1u : 0u) << (2 * i);
                if (y + 1 < H) body_load_row16(lab + first + W, nv, o);
#pragma unroll
                for (int i = 0; i < BODY_PPT; ++i) ud += (y + 1 == H || o[i] != r[i] ? 1u : 0u) << (2 * i);
            }
            if (x0 > 0) before = lab[first - 1];
            if (x0 + BODY_PPT < W) after = lab[first + BODY_PPT];
            if (a.value) {
                const unsigned char* const src = a.value + (unsigned long long)t * a.vstride + first;
                if (nv == BODY_PPT) vb = ldg_u<body_u32x4_b, u32x4, false>(src);
                else
#pragma unroll
                    for (int i = 0; i < BODY_PPT; ++i)
                        if (i < nv) vb[i / 4] |= (unsigned)src[i] << (8 * (i % 4));
            }
            // dense per element: per run one bound check, then label[L - 1] and dense[L - 1] together
#pragma unroll
            for (int i = 0; i < BODY_PPT; ++i) {
                const unsigned L = r[i];
                d[i] = 0u;
                if (L) {
                    if (i > 0 && L == r[i > 0 ? i - 1 : 0] && d[i > 0 ? i - 1 : 0]) d[i] = d[i > 0 ? i - 1 : 0];
                    else if (body_in_reach(L, first + i)) {                  // L - 1 <= first + i < n: inside the tile
                        const unsigned target = lab[L - 1u], dv = den[L - 1u];
                        if (target == L) d[i] = dv;
                    }
                    if (d[i]) ++good;
                    else ++bad;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < BODY_PPT; ++i) r[i] = 0u, d[i] = 0u;
        }
        // one walk over the 16 pixels of the row; the run that ends at element i is handed in at step i.  x and y of a piece
        // are relative to the rectangle.
        BodyPiece q = {0u, 0u, 0u, 0u, 0xFFFFFFFFu, 0u, lr, 0u, 0u};
#pragma unroll
        for (int i = 0; i < BODY_PPT; ++i) {
            const unsigned cur = d[i];
            if (cur) {
                const unsigned x = x0 + i, xr = seg * BODY_PPT + i;
                const unsigned left = x == 0u || (i > 0 ? r[i > 0 ? i - 1 : 0] : before) != r[i];
                const unsigned right = x == W - 1u || (i < BODY_PPT - 1 ? r[i < BODY_PPT - 1 ? i + 1 : i] : after) != r[i];
                const unsigned e = ((ud >> (2 * i)) & 3u) + left + right;
                edges += e;
                ++q.area;
                q.per += e;
                q.sx += xr;
                q.sy += lr;
                q.x_min = xr < q.x_min ? xr : q.x_min;
                q.x_max = xr > q.x_max ? xr : q.x_max;
                if (a.value) {
                    const unsigned c = cat[(vb[i / 4] >> (8 * (i % 4))) & 0xffu];
                    q.c01 += (c == 0u ? 1u : 0u) + (c == 1u ? 0x10000u : 0u);
                    q.c23 += (c == 2u ? 1u : 0u) + (c == 3u ? 0x10000u : 0u);
                }
            }
            if (!a.rows) continue;                       // (uniform)
            bool pend = cur && (i == BODY_PPT - 1 || d[i < BODY_PPT - 1 ? i + 1 : i] != cur);
            const bool ends = pend;
            if (__any(pend)) {                           // (wave-uniform)
                BodyPiece own = q;                       // what this lane deposits, if it does
                bool deposit = pend;
#pragma unroll 1
                for (int round = 0; round < BODY_PEEL; ++round) {
                    const unsigned long long todo = __ballot(pend);
                    if (!todo) break;                    // (wave-uniform)
                    const int leader = __ffsll((long long)todo) - 1;
                    const unsigned lead = __shfl(cur, leader);
                    const bool match = pend && cur == lead;
                    const unsigned long long mm = __ballot(match);
                    pend = pend && !match;
                    if (mm == (1ull << leader)) continue;                    // (wave-uniform) nobody shares the leader's body
                    const int last = 63 - __clzll((long long)mm);
                    BodyPiece w;
                    const unsigned s_ap = body_wave_sum(match ? q.area | (q.per << 16) : 0u);      // <= 1024 | 4096 << 16
                    w.area = s_ap & 0xffffu;
                    w.per = s_ap >> 16;
                    w.sx = body_wave_sum(match ? q.sx : 0u);
                    w.sy = body_wave_sum(match ? q.sy : 0u);
                    w.x_min = body_wave_min(match ? q.x_min : 0xFFFFFFFFu);
                    w.x_max = body_wave_max(match ? q.x_max : 0u);
                    w.y_max = __shfl(lr, last);          // (rows rise with the lane)
                    w.c01 = 0u, w.c23 = 0u;
                    if (a.value) {                       // (uniform)
                        w.c01 = body_wave_sum(match ? q.c01 : 0u);
                        if (a.n_cats > 2) w.c23 = body_wave_sum(match ? q.c23 : 0u);
                    }
                    if (match) deposit = false;
                    if (lane == (unsigned)leader) own = w, deposit = true;
                }
                // the leaders with what they collected, and what was left: into the workgroup's table, or straight to the row
                if (deposit && !body_slot_add(key, acc, cur, own))
                    body_emit(a, t, cur, own.area, own.per, (unsigned long long)own.area * rect_x + own.sx,
                              (unsigned long long)own.area * rect_y + own.sy, rect_x + own.x_min, rect_x + own.x_max,
                              rect_y + own.y_max, own.c01 & 0xffffu, own.c01 >> 16, own.c23 & 0xffffu, own.c23 >> 16);
            }
            if (ends) q = BodyPiece{0u, 0u, 0u, 0u, 0xFFFFFFFFu, 0u, lr, 0u, 0u};
        }
        if (nv > 0) {
            if (nv == BODY_PPT) body_store16(den, (long long)first, (long long)a.n_elems, d);
            else
#pragma unroll
                for (int i = 0; i < BODY_PPT; ++i)
                    if (i < nv) den[first + i] = d[i];
        }
        if (a.head) {                                    // (uniform)
            good = body_wave_sum(good);
            bad = body_wave_sum(bad);
            edges = body_wave_sum(edges);
            if (lane == 0) {
                if (good) atomicAdd(&part[0], (unsigned long long)good);
                if (bad) atomicAdd(&part[1], (unsigned long long)bad);
                if (edges) atomicAdd(&part[2], (unsigned long long)edges);
            }
        }
        __syncthreads();
        if (a.head && tid < 3 && part[tid])
            atomicAdd(a.head + (unsigned long long)t * DSWX_BODY_HEAD_WORDS + BODY_HEAD_MEMBERS + tid, part[tid]);
        if (a.rows && tid < BODY_SLOTS && key[tid]) {
            const unsigned* const s = acc[tid];
            body_emit(a, t, key[tid], s[SLOT_AREA], s[SLOT_PER], (unsigned long long)s[SLOT_AREA] * rect_x + s[SLOT_SX],
                      (unsigned long long)s[SLOT_AREA] * rect_y + s[SLOT_SY], rect_x + s[SLOT_X_MIN], rect_x + s[SLOT_X_MAX],
                      rect_y + s[SLOT_Y_MAX], s[SLOT_COUNT], s[SLOT_COUNT + 1], s[SLOT_COUNT + 2], s[SLOT_COUNT + 3]);
        }
        __syncthreads();                                 // (the partials and the slots are reset for the next tile)
    }
}

}  // namespace

// The checks that the device and the host entry share, in the house order: the arguments before any context, nothing
// written by a refused call.  `align` = label and dense must be 4-byte and rows and head 8-byte aligned (the device entry).
int dswx_body_check(const uint32_t* label, const uint8_t* value, const dswx_body_spec_t* spec, int64_t n_tiles, int64_t height,
                    int64_t width, int64_t* stride, const dswx_body_out_t* out, bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (spec->n_cats < 0 || spec->n_cats > DSWX_BODY_MAX_CATS)
        return dswx_fail(DSWX_ERR_ARG, "n_cats %d outside 0 .. %d", spec->n_cats, DSWX_BODY_MAX_CATS);
    if (value && spec->n_cats == 0) return dswx_fail(DSWX_ERR_ARG, "a value plane with n_cats 0: nothing of it would be counted");
    if (!value && spec->n_cats > 0) return dswx_fail(DSWX_ERR_ARG, "value is NULL with n_cats %d", spec->n_cats);
    if (n_tiles < 0 || height < 0 || width < 0 || *stride < 0 || spec->max_rows < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (height > BODY_MAX_PIXELS || width > BODY_MAX_PIXELS || height * width > BODY_MAX_PIXELS)
        return dswx_fail(DSWX_ERR_ARG, "raster too large: height * width above 2^31, a label would not fit 32 bits");
    const int64_t n_elems = height * width;
    if (int rc = dswx_tile_stride_check(stride, n_elems, "value_stride")) return rc;
    if (int rc = dswx_tile_extent_check(*stride, n_tiles, true)) return rc;
    if (spec->max_rows > BODY_MAX_ROWS) return dswx_fail(DSWX_ERR_ARG, "max_rows %lld above 2^31", (long long)spec->max_rows);
    if (!out->dense) return dswx_fail(DSWX_ERR_ARG, "dense is NULL: it is the working array and always required");
    if (int rc = dswx_tile_plane_check(label, n_tiles, n_elems, "label")) return rc;
    if (!out->rows && spec->max_rows > 0) return dswx_fail(DSWX_ERR_ARG, "rows is NULL with max_rows %lld", (long long)spec->max_rows);
    if (align) {
        if (!aligned_to(label, 4)) return dswx_fail(DSWX_ERR_ALIGN, "label not 4-byte aligned");
        if (!aligned_to(out->dense, 4)) return dswx_fail(DSWX_ERR_ALIGN, "dense not 4-byte aligned");
        if (!aligned_to(out->rows, 8)) return dswx_fail(DSWX_ERR_ALIGN, "rows not 8-byte aligned");
        if (!aligned_to(out->head, 8)) return dswx_fail(DSWX_ERR_ALIGN, "head not 8-byte aligned");
    }
    return DSWX_OK;
}

// The launches; the arguments have passed dswx_body_check (stride resolved).
int dswx_body_launch(dswx_ctx* ctx, const uint32_t* label, const uint8_t* value, const dswx_body_spec_t* spec, int64_t n_tiles,
                     int64_t height, int64_t width, int64_t stride, const dswx_body_out_t* out, hipStream_t s) {
    if (n_tiles == 0 || height == 0 || width == 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    BodyArgs a = {};
    a.label = label;
    a.value = value;
    a.vstride = (unsigned long long)stride;
    a.n_elems = (unsigned long long)(height * width);
    a.n_tiles = n_tiles;
    a.height = (unsigned)height;
    a.width = (unsigned)width;
    a.chunks = (unsigned)((a.n_elems + BODY_CHUNK - 1) / BODY_CHUNK);
    a.rx = (unsigned)((width + BODY_RECT_W - 1) / BODY_RECT_W);
    a.ry = (unsigned)((height + BODY_RECT_H - 1) / BODY_RECT_H);
    a.n_cats = spec->n_cats;
    a.max_rows = (unsigned long long)spec->max_rows;
    a.dense = out->dense;
    a.rows = spec->max_rows > 0 ? out->rows : nullptr;
    a.head = reinterpret_cast<unsigned long long*>(out->head);
    std::memcpy(a.cat, spec->cat_of_byte, 256);
    const unsigned gy = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
    const dim3 block(BODY_BLOCK);
    if (a.rows) HIP_TRY(hipMemsetAsync(a.rows, 0, (size_t)n_tiles * (size_t)a.max_rows * DSWX_BODY_ROW_WORDS * sizeof(uint32_t), s));
    if (a.head) HIP_TRY(hipMemsetAsync(a.head, 0, (size_t)n_tiles * DSWX_BODY_HEAD_WORDS * sizeof(uint64_t), s));
    hipLaunchKernelGGL(dswx_body_count_k, dim3(a.chunks, gy), block, 0, s, a);
    hipLaunchKernelGGL(dswx_body_scan_k, dim3(gy), block, 0, s, a);
    hipLaunchKernelGGL(dswx_body_rank_k, dim3(a.chunks, gy), block, 0, s, a);
    // (height * width <= 2^31: at most 2^26 rectangles, where the raster is one pixel wide)
    hipLaunchKernelGGL(dswx_body_fill_k, dim3(a.rx * a.ry, gy), block, 0, s, a);
    HIP_TRY(hipGetLastError());
    char info[320];
    snprintf(info, sizeof info, "dswx_body_count_k/rank_k grid=(%u,%u,1) block=%d chunk=%d + dswx_body_scan_k grid=(%u,1,1) step=%d + dswx_body_fill_k grid=(%u,%u,1) rect=%dx%d n_cats=%d max_rows=%llu",
             a.chunks, gy, BODY_BLOCK, BODY_CHUNK, gy, DSWX_BODY_SCAN_STEP, a.rx * a.ry, gy, BODY_RECT_H, BODY_RECT_W, a.n_cats, a.max_rows);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_body_table_host(const uint32_t* label, const uint8_t* value, const dswx_body_spec_t* spec, int64_t n_tiles, int64_t height,
                         int64_t width, int64_t stride, const dswx_body_out_t* out) {
    if (int rc = dswx_body_check(label, value, spec, n_tiles, height, width, &stride, out, false)) return rc;
    if (n_tiles == 0 || height == 0 || width == 0) return DSWX_OK;
    const int64_t n = height * width, max_rows = spec->max_rows;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const uint32_t* lab = reinterpret_cast<const uint32_t*>(reinterpret_cast<const unsigned char*>(label) + (size_t)t * (size_t)n * 4);
        uint32_t* den = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(out->dense) + (size_t)t * (size_t)n * 4);
        uint32_t* rows = out->rows ? reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(out->rows) +
                                                                 (size_t)t * (size_t)max_rows * DSWX_BODY_ROW_WORDS * 4)
                                   : nullptr;
        const uint8_t* val = value ? value + (size_t)t * (size_t)stride : nullptr;
        if (rows) std::memset(rows, 0, (size_t)max_rows * DSWX_BODY_ROW_WORDS * 4);
        // the roots in rising order: their ranks, and the beginning of their rows
        uint64_t k = 0;
        for (int64_t p = 0; p < n; ++p) {
            const bool root = body_is_root(dswx_load<uint32_t>(lab, p), (uint64_t)p);
            dswx_store<uint32_t>(den, p, root ? (uint32_t)(k + 1) : 0u);
            if (!root) continue;
            if (rows && (int64_t)k < max_rows) {
                uint32_t* row = rows + (size_t)k * DSWX_BODY_ROW_WORDS;
                dswx_store<uint32_t>(row, BODY_LABEL, (uint32_t)p + 1u);
                dswx_store<uint32_t>(row, BODY_X_MIN, 0xFFFFFFFFu);
                dswx_store<uint32_t>(row, BODY_Y_MIN, (uint32_t)(p / width));
            }
            ++k;
        }
        // every pixel: a root lies at or before the pixels that name it, so its dense value is final when it is read
        uint64_t good = 0, bad = 0, edges = 0;
        for (int64_t y = 0; y < height; ++y)
            for (int64_t x = 0; x < width; ++x) {
                const int64_t p = y * width + x;
                const uint32_t L = dswx_load<uint32_t>(lab, p);
                if (!L) continue;
                uint32_t dv = 0;
                if (body_in_reach(L, (uint64_t)p) && dswx_load<uint32_t>(lab, (int64_t)L - 1) == L) dv = dswx_load<uint32_t>(den, (int64_t)L - 1);
                dswx_store<uint32_t>(den, p, dv);
                if (!dv) {
                    ++bad;
                    continue;
                }
                ++good;
                const uint32_t e = (x == 0 || dswx_load<uint32_t>(lab, p - 1) != L ? 1u : 0u) + (x == width - 1 || dswx_load<uint32_t>(lab, p + 1) != L ? 1u : 0u) +
                                   (y == 0 || dswx_load<uint32_t>(lab, p - width) != L ? 1u : 0u) + (y == height - 1 || dswx_load<uint32_t>(lab, p + width) != L ? 1u : 0u);
                edges += e;
                if (!rows || (int64_t)dv - 1 >= max_rows) continue;
                uint32_t* row = rows + (size_t)(dv - 1u) * DSWX_BODY_ROW_WORDS;
                dswx_store<uint32_t>(row, BODY_AREA, dswx_load<uint32_t>(row, BODY_AREA) + 1u);
                if ((uint32_t)x < dswx_load<uint32_t>(row, BODY_X_MIN)) dswx_store<uint32_t>(row, BODY_X_MIN, (uint32_t)x);
                if ((uint32_t)x > dswx_load<uint32_t>(row, BODY_X_MAX)) dswx_store<uint32_t>(row, BODY_X_MAX, (uint32_t)x);
                if ((uint32_t)y > dswx_load<uint32_t>(row, BODY_Y_MAX)) dswx_store<uint32_t>(row, BODY_Y_MAX, (uint32_t)y);
                dswx_store<uint64_t>(row + BODY_PERIMETER, 0, dswx_load<uint64_t>(row + BODY_PERIMETER, 0) + e);
                dswx_store<uint64_t>(row + BODY_SUM_X, 0, dswx_load<uint64_t>(row + BODY_SUM_X, 0) + (uint64_t)x);
                dswx_store<uint64_t>(row + BODY_SUM_Y, 0, dswx_load<uint64_t>(row + BODY_SUM_Y, 0) + (uint64_t)y);
                if (val) {
                    const unsigned c = body_cat(spec->cat_of_byte[val[p]], spec->n_cats);
                    if (c != BODY_NOT_COUNTED) dswx_store<uint32_t>(row, BODY_COUNT + (int64_t)c, dswx_load<uint32_t>(row, BODY_COUNT + (int64_t)c) + 1u);
                }
            }
        if (out->head) {
            const uint64_t head[DSWX_BODY_HEAD_WORDS] = {k, k < (uint64_t)max_rows ? k : (uint64_t)max_rows, good, bad, edges, 0, 0, 0};
            for (int w = 0; w < DSWX_BODY_HEAD_WORDS; ++w) dswx_store<uint64_t>(out->head, (size_t)(t * DSWX_BODY_HEAD_WORDS + w), head[w]);
        }
    }
    return DSWX_OK;
}

int dswx_body_table_device(dswx_ctx_t* ctx, const uint32_t* label, const uint8_t* value, const dswx_body_spec_t* spec, int64_t n_tiles,
                           int64_t height, int64_t width, int64_t stride, const dswx_body_out_t* out, void* stream) {
    if (int rc = dswx_body_check(label, value, spec, n_tiles, height, width, &stride, out, true)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) { return dswx_body_launch(ctx, label, value, spec, n_tiles, height, width, stride, out, s); });
}

}  // extern "C"
