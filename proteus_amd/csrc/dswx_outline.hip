// dswx_outline.hip -- the outlines of the regions of an id plane as ordered rings of pixel edges (DSWX_HAS_OUTLINE, additive to
// ABI v7), without the 4-byte plane crossing PCIe.  include/dswx_hip.h "outline" states the definition; proteus_amd/outline.py
// is its numpy statement and dswx_outline_host below the scalar one -- dswx_outline_rule.h is compiled for both sides.
//
// The boundary edges are what the body table's perimeter counts; what is new is their ORDER.  Every edge has exactly one
// successor, so the edges fall into cycles; a cycle is found by POINTER JUMPING: every edge keeps (next, min, off) -- an edge
// 2^k steps ahead, the smallest edge among the 2^k from itself on, and how far ahead that one lies -- and a round doubles the
// reach by reading the state of `next`.  After ceil(log2 L) rounds min is the ring's start and off the distance to it.
// Edges are numbered in the order of their keys (a prefix sum over the pixels), so the comparisons are on those numbers.
//
// NO WORKGROUP EVER WAITS FOR ANOTHER: every dependence is a kernel boundary.  The launches, all of them over every tile:
//   1 dswx_outline_count_k       a workgroup owns a chunk of 4096 pixels, a thread 16 of them: the 4-bit edge mask of every
//                                pixel goes to `mask`, the chunk's edge count to base[first pixel of the chunk].
//   2 dswx_outline_scan_k        one workgroup per tile turns those counts into exclusive prefix sums in place (256 chunks
//                                per step with a running carry), notes E and whether it fits, clears the round flags and
//                                begins the head.
//   3 dswx_outline_base_k        base[p] = the number of the first edge of pixel p (from the masks alone).
//   4 dswx_outline_emit_k        for every edge its state {next | corner << 31, min = own number, off = 0, key}; the number
//                                of a successor is base[its pixel] + the set directions of that pixel below its own.
//   5 dswx_outline_jump_k x N    one round each, reading one copy of the states and writing the other; N = ceil(log2 cap),
//                                cap = min(max_edges, 4 * height * width), fixed by the capacity so that nothing is read
//                                back.  A round in which no edge of a tile took a smaller minimum leaves that tile finished:
//                                the workgroups of the rounds behind it return at once on its flag.
//   6 dswx_outline_ring_count_k  a workgroup owns 4096 edges: the ring starts (min == own number) get their length
//                                L = off[successor] + 1; per chunk the number of starts and the sum of their lengths.
//   7 dswx_outline_ring_scan_k   one workgroup per tile scans those pairs: R, and the rest of the head.
//   8 dswx_outline_ring_rank_k   row index and chain offset of every ring; its row begins, its sums are cleared.
//   9 dswx_outline_scatter_k     chain[offset + (L - off) % L] = key; area2 and corners combined over runs of lanes of one
//                                ring before one set of atomics.
//  10 dswx_outline_finish_k      the sums into the rows; outer rings, holes and corners into the head.
// plus one hipMemsetAsync each of `chain` and `rings`: 9 + N launches.  DESIGN.md section 5 has the bytes per edge.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dswx_host.h"
#include "dswx_body_rule.h"
#include "dswx_outline_rule.h"

namespace {

typedef u32x4 __attribute__((aligned(16))) out_u32x4;

constexpr int OUT_BLOCK = 256;
constexpr int OUT_PPT = 16;                              // pixels, or edges, of a thread in the chunked launches
constexpr int OUT_WAVES = OUT_BLOCK / 64;
constexpr int OUT_CHUNK = DSWX_OUTLINE_CHUNK;
static_assert(DSWX_OUTLINE_CHUNK == DSWX_BODY_CHUNK && DSWX_OUTLINE_SCAN_STEP == DSWX_BODY_SCAN_STEP, "the scan of the body table");
static_assert(OUT_BLOCK * OUT_PPT == OUT_CHUNK && DSWX_OUTLINE_SCAN_STEP == OUT_BLOCK, "a workgroup's threads cover a chunk");
constexpr int64_t OUT_MAX_PIXELS = 1LL << 30;
constexpr int64_t OUT_MAX_CAP = 1LL << 31;
constexpr unsigned OUT_CORNER = 0x80000000u;             // in `next`: the successor has another direction
constexpr int OUT_MAX_ROUNDS = 31;
constexpr unsigned OUT_NO_RING = 0xFFFFFFFFu;

// What a tile's launches tell each other (in `work`, written by launch 2 first).
struct OutlineInfo {
    unsigned long long E;                                // the edges of the tile
    unsigned long long R;                                // its rings (launch 7)
    unsigned ok;                                         // E <= max_edges: everything behind launch 2 runs
    unsigned fin;                                        // the copy of the states that the last round wrote
    unsigned flag[OUT_MAX_ROUNDS + 1];                   // flag[k]: an edge took a smaller minimum in round k
};
static_assert(sizeof(OutlineInfo) <= 256, "the info block of a tile");

// Where the parts of a tile's working memory lie; every offset and the size are multiples of 16.
struct OutlineLayout {
    unsigned long long cap;                              // min(max_edges, 4 * n): the edges a tile can have and still fit
    unsigned long long base, mask, st0, st1, acc, part, info, per_tile;
    unsigned chunks_p, chunks_e, rounds, acc_blocks;
};
inline unsigned long long up16(unsigned long long v) { return (v + 15ull) & ~15ull; }
OutlineLayout outline_layout(int64_t max_edges, int64_t height, int64_t width) {
    OutlineLayout l = {};
    const unsigned long long n = (unsigned long long)(height * width);
    l.cap = (unsigned long long)max_edges < 4ull * n ? (unsigned long long)max_edges : 4ull * n;
    l.chunks_p = (unsigned)((n + OUT_CHUNK - 1) / OUT_CHUNK);
    l.chunks_e = (unsigned)((l.cap + OUT_CHUNK - 1) / OUT_CHUNK);
    while ((1ull << l.rounds) < l.cap) ++l.rounds;       // <= 31
    const unsigned long long rings = l.cap / 4ull;       // a ring has at least 4 edges
    l.acc_blocks = (unsigned)((rings + OUT_BLOCK - 1) / OUT_BLOCK);
    unsigned long long at = 0;
    l.base = at, at += up16(4ull * n);
    l.mask = at, at += up16(n);
    l.st0 = at, at += 16ull * l.cap;
    l.st1 = at, at += 16ull * l.cap;
    l.acc = at, at += 16ull * rings;
    l.part = at, at += up16(8ull * l.chunks_e);
    l.info = at, at += 256ull;
    l.per_tile = at;
    return l;
}

struct OutlineArgs {
    const unsigned* ids;
    unsigned char* work;                                 // 16-byte aligned
    OutlineLayout l;
    unsigned long long n_elems;                          // height * width <= 2^30
    long long n_tiles;
    unsigned height, width;
    int connectivity;
    unsigned round;                                      // of dswx_outline_jump_k
    unsigned long long max_edges, max_rings;             // <= 2^31: the strides of chain and rings
    unsigned* chain;                                     // nullptr: not wanted
    unsigned* rings;                                     // nullptr: not wanted or max_rings == 0
    unsigned long long* head;                            // nullptr: not wanted
};

struct DevIds {
    const unsigned* p;
    __device__ __forceinline__ unsigned operator()(uint64_t i) const { return p[i]; }
};

__device__ __forceinline__ unsigned char* tile_work(const OutlineArgs& a, long long t) { return a.work + (unsigned long long)t * a.l.per_tile; }
__device__ __forceinline__ unsigned* w_base(const OutlineArgs& a, long long t) { return reinterpret_cast<unsigned*>(tile_work(a, t) + a.l.base); }
__device__ __forceinline__ unsigned char* w_mask(const OutlineArgs& a, long long t) { return tile_work(a, t) + a.l.mask; }
__device__ __forceinline__ out_u32x4* w_state(const OutlineArgs& a, long long t, unsigned which) {
    return reinterpret_cast<out_u32x4*>(tile_work(a, t) + (which ? a.l.st1 : a.l.st0));
}
__device__ __forceinline__ unsigned long long* w_acc(const OutlineArgs& a, long long t) {
    return reinterpret_cast<unsigned long long*>(tile_work(a, t) + a.l.acc);
}
__device__ __forceinline__ unsigned* w_part(const OutlineArgs& a, long long t) { return reinterpret_cast<unsigned*>(tile_work(a, t) + a.l.part); }
__device__ __forceinline__ OutlineInfo* w_info(const OutlineArgs& a, long long t) { return reinterpret_cast<OutlineInfo*>(tile_work(a, t) + a.l.info); }

__device__ __forceinline__ unsigned out_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the inclusive prefix sum of v over the lanes of a wave
__device__ __forceinline__ unsigned out_wave_scan(unsigned v, unsigned lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o);
        if (lane >= (unsigned)o) v += u;
    }
    return v;
}
__device__ __forceinline__ long long out_shfl_up64(long long v, int o) {
    const unsigned lo = __shfl_up((unsigned)(unsigned long long)v, o), hi = __shfl_up((unsigned)((unsigned long long)v >> 32), o);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// The exclusive prefix of v over the threads of the workgroup and (in *total) the workgroup's sum; two barriers.
__device__ __forceinline__ unsigned out_block_scan(unsigned v, unsigned* wtot, unsigned* total) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned inc = out_wave_scan(v, lane);
    if (lane == 63u) wtot[wave] = inc;
    __syncthreads();
    unsigned before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < OUT_WAVES; ++w) {
        if ((unsigned)w < wave) before += wtot[w];
        sum += wtot[w];
    }
    __syncthreads();                                     // (wtot may be written again)
    *total = sum;
    return before + inc - v;
}

// the successor of edge (p at (x, y), d) as the number of that edge, with OUT_CORNER when its direction is another
__device__ __forceinline__ unsigned out_succ_number(const OutlineArgs& a, const unsigned* ids, const unsigned* base, const unsigned char* mask,
                                                    unsigned x, unsigned y, unsigned d, unsigned v) {
    const OutlineEdge s = outline_succ(DevIds{ids}, (int64_t)x, (int64_t)y, d, (int64_t)a.width, (int64_t)a.height, v, a.connectivity);
    const unsigned long long q = (unsigned long long)s.y * a.width + (unsigned long long)s.x;    // inside the tile: it holds v
    const unsigned e = base[q] + __popc((unsigned)mask[q] & ((1u << s.d) - 1u));
    return e | (s.d != d ? OUT_CORNER : 0u);
}

// ---- launch 1: the edge mask of every pixel, the edges of every chunk -------------------------------------------------------
__global__ __launch_bounds__(OUT_BLOCK) void dswx_outline_count_k(const OutlineArgs a) {
    __shared__ unsigned wtot[OUT_WAVES];
    const unsigned long long chunk_first = (unsigned long long)blockIdx.x * OUT_CHUNK;           // < n_elems: chunks = ceil
    const unsigned long long first = chunk_first + (unsigned long long)threadIdx.x * OUT_PPT;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const unsigned* const ids = a.ids + (unsigned long long)t * a.n_elems;
        unsigned char* const mask = w_mask(a, t);
        unsigned c = 0;
        if (first < a.n_elems) {
            unsigned y = (unsigned)(first / a.width), x = (unsigned)(first - (unsigned long long)y * a.width);
            unsigned m[OUT_PPT];
#pragma unroll
            for (int i = 0; i < OUT_PPT; ++i) {
                m[i] = 0u;
                if (first + i < a.n_elems) {
                    const unsigned v = ids[first + i];
                    if (v) m[i] = outline_mask(DevIds{ids}, (int64_t)x, (int64_t)y, (int64_t)a.width, (int64_t)a.height, v);
                    c += __popc(m[i]);
                    if (++x == a.width) x = 0u, ++y;
                }
            }
            if (first + OUT_PPT <= a.n_elems) {          // (the masks of a tile begin at a multiple of 16 bytes, `first` is one)
                u32x4 q;
#pragma unroll
                for (int w = 0; w < 4; ++w) q[w] = m[4 * w] | (m[4 * w + 1] << 8) | (m[4 * w + 2] << 16) | (m[4 * w + 3] << 24);
                *reinterpret_cast<out_u32x4*>(mask + first) = q;
            } else {
#pragma unroll
                for (int i = 0; i < OUT_PPT; ++i)
                    if (first + i < a.n_elems) mask[first + i] = (unsigned char)m[i];
            }
        }
        c = out_wave_sum(c);
        if (lane == 0) wtot[wave] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned sum = 0;
#pragma unroll
            for (int w = 0; w < OUT_WAVES; ++w) sum += wtot[w];
            w_base(a, t)[chunk_first] = sum;             // <= 4 * 4096
        }
        __syncthreads();                                 // (wtot is written again for the next tile)
    }
}

// ---- launch 2: the chunk counts of a tile become exclusive prefix sums, in place; E; the head begins ---------------------------
__global__ __launch_bounds__(OUT_BLOCK) void dswx_outline_scan_k(const OutlineArgs a) {
    __shared__ unsigned wtot[OUT_WAVES];
    for (long long t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        unsigned* const b = w_base(a, t);
        unsigned long long carry = 0;                    // the edges of the chunks before `first` (<= 2^32)
        for (unsigned first = 0; first < a.l.chunks_p; first += DSWX_OUTLINE_SCAN_STEP) {
            const unsigned c = first + threadIdx.x;
            const unsigned val = c < a.l.chunks_p ? b[(unsigned long long)c * OUT_CHUNK] : 0u;
            unsigned total;
            const unsigned before = out_block_scan(val, wtot, &total);
            // (a tile that does not fit may pass 2^32 here: its prefixes wrap and nothing reads them)
            if (c < a.l.chunks_p) b[(unsigned long long)c * OUT_CHUNK] = (unsigned)carry + before;
            carry += total;
        }
        OutlineInfo* const info = w_info(a, t);
        const bool ok = carry <= a.max_edges;
        if (threadIdx.x <= OUT_MAX_ROUNDS) info->flag[threadIdx.x] = 0u;
        if (threadIdx.x == 0) {
            info->E = carry;
            info->R = 0ull;
            info->ok = ok ? 1u : 0u;
            info->fin = 0u;
        }
        if (a.head && threadIdx.x < DSWX_OUTLINE_HEAD_WORDS) {
            const unsigned w = threadIdx.x;
            a.head[(unsigned long long)t * DSWX_OUTLINE_HEAD_WORDS + w] =
                w == OUTLINE_HEAD_E ? carry : w == OUTLINE_HEAD_WRITTEN ? (ok ? carry : 0ull) : w == OUTLINE_HEAD_OVERFLOW ? (ok ? 0ull : 1ull) : 0ull;
        }
    }
}

// ---- launch 3: the number of the first edge of every pixel --------------------------------------------------------------------
__global__ __launch_bounds__(OUT_BLOCK) void dswx_outline_base_k(const OutlineArgs a) {
    __shared__ unsigned wtot[OUT_WAVES];
    __shared__ unsigned chunk_base;
    const unsigned long long chunk_first = (unsigned long long)blockIdx.x * OUT_CHUNK;
    const unsigned long long first = chunk_first + (unsigned long long)threadIdx.x * OUT_PPT;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        if (!w_info(a, t)->ok) continue;                 // (uniform)
        unsigned* const b = w_base(a, t);
        const unsigned char* const mask = w_mask(a, t);
        unsigned m[OUT_PPT], c = 0;
#pragma unroll
        for (int i = 0; i < OUT_PPT; ++i) {
            m[i] = first + i < a.n_elems ? (unsigned)mask[first + i] : 0u;
            c += __popc(m[i]);
        }
        // the prefix of this chunk lies in its first element, which only this workgroup writes in this launch, and only
        // behind the barriers of the scan
        if (threadIdx.x == 0) chunk_base = b[chunk_first];
        unsigned total;
        const unsigned before = out_block_scan(c, wtot, &total);
        unsigned e = chunk_base + before;
#pragma unroll
        for (int i = 0; i < OUT_PPT; ++i)
            if (first + i < a.n_elems) {
                b[first + i] = e;
                e += __popc(m[i]);
            }
        __syncthreads();                                 // (chunk_base is written again for the next tile)
    }
}

// ---- launch 4: the state of every edge before the first round ----------------------------------------------------------------
__global__ __launch_bounds__(OUT_BLOCK) void dswx_outline_emit_k(const OutlineArgs a) {
    const unsigned long long first = (unsigned long long)blockIdx.x * OUT_CHUNK + (unsigned long long)threadIdx.x * OUT_PPT;
    if (first >= a.n_elems) return;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        if (!w_info(a, t)->ok) continue;
        const unsigned* const ids = a.ids + (unsigned long long)t * a.n_elems;
        const unsigned* const b = w_base(a, t);
        const unsigned char* const mask = w_mask(a, t);
        out_u32x4* const st = w_state(a, t, 0u);
        unsigned y = (unsigned)(first / a.width), x = (unsigned)(first - (unsigned long long)y * a.width);
        for (int i = 0; i < OUT_PPT && first + i < a.n_elems; ++i) {
            const unsigned p = (unsigned)(first + i), m = mask[p];
            if (m) {
                const unsigned v = ids[p];
                unsigned e = b[p];                       // < E <= cap: the tile fits
                for (unsigned d = 0; d < 4u; ++d)
                    if ((m >> d) & 1u) {
                        st[e] = u32x4{out_succ_number(a, ids, b, mask, x, y, d, v), e, 0u, 4u * p + d};
                        ++e;
                    }
            }
            if (++x == a.width) x = 0u, ++y;
        }
    }
}

// ---- launch 5, once per round: next, min and off of every edge from the state of `next` ----------------------------------------
__global__ __launch_bounds__(OUT_BLOCK) void dswx_outline_jump_k(const OutlineArgs a) {
    const unsigned long long e = (unsigned long long)blockIdx.x * OUT_BLOCK + threadIdx.x;
    const unsigned k = a.round;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        OutlineInfo* const info = w_info(a, t);
        if (!info->ok || (k > 0u && !info->flag[k - 1u])) continue;          // (uniform) too large, or finished already
        if ((unsigned long long)blockIdx.x * OUT_BLOCK >= info->E) continue;   // (uniform)
        // (a round of a tile runs only if every round before it ran: the states of round k lie in copy k & 1)
        const out_u32x4* const src = w_state(a, t, k & 1u);
        out_u32x4* const dst = w_state(a, t, (k + 1u) & 1u);
        if (blockIdx.x == 0 && threadIdx.x == 0) info->fin = (k + 1u) & 1u;
        bool take = false;
        if (e < info->E) {
            const u32x4 s = src[e];
            const u32x4 o = src[s.x & ~OUT_CORNER];
            take = o.y < s.y;                            // strict: the first occurrence wins
            dst[e] = u32x4{(o.x & ~OUT_CORNER) | (s.x & OUT_CORNER), take ? o.y : s.y, take ? (1u << k) + o.z : s.z, s.w};
        }
        if (__any(take) && (threadIdx.x & 63u) == 0u) info->flag[k] = 1u;
    }
}

// ---- launch 6: the length of every ring at its start; starts and lengths per chunk of edges -----------------------------------
__global__ __launch_bounds__(OUT_BLOCK) void dswx_outline_ring_count_k(const OutlineArgs a) {
    __shared__ unsigned wtot[OUT_WAVES];
    const unsigned long long first = (unsigned long long)blockIdx.x * OUT_CHUNK + (unsigned long long)threadIdx.x * OUT_PPT;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const OutlineInfo* const info = w_info(a, t);
        if (!info->ok) continue;                         // (uniform)
        const unsigned long long E = info->E;
        const out_u32x4* const st = w_state(a, t, info->fin);
        out_u32x4* const ring = w_state(a, t, info->fin ^ 1u);
        const unsigned* const ids = a.ids + (unsigned long long)t * a.n_elems;
        unsigned count = 0, length = 0;
        for (int i = 0; i < OUT_PPT && first + i < E; ++i) {
            const unsigned e = (unsigned)(first + i);
            const u32x4 s = st[e];
            if (s.y != e) continue;
            const unsigned p = s.w >> 2, d = s.w & 3u, y = p / a.width, x = p - y * a.width;
            const unsigned nx = out_succ_number(a, ids, w_base(a, t), w_mask(a, t), x, y, d, ids[p]) & ~OUT_CORNER;
            const unsigned L = st[nx].z + 1u;
            ring[e] = u32x4{L, 0u, 0u, 0u};
            ++count;
            length += L;
        }
        unsigned tc, tl;
        out_block_scan(count, wtot, &tc);
        out_block_scan(length, wtot, &tl);
        if (threadIdx.x == 0) {
            w_part(a, t)[2ull * blockIdx.x] = tc;
            w_part(a, t)[2ull * blockIdx.x + 1] = tl;
        }
    }
}

// ---- launch 7: those pairs become exclusive prefix sums; R and the rest of the head -------------------------------------------
__global__ __launch_bounds__(OUT_BLOCK) void dswx_outline_ring_scan_k(const OutlineArgs a) {
    __shared__ unsigned wtot[OUT_WAVES];
    for (long long t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        OutlineInfo* const info = w_info(a, t);
        if (!info->ok) continue;                         // (uniform)
        unsigned* const part = w_part(a, t);
        const unsigned chunks = (unsigned)((info->E + OUT_CHUNK - 1) / OUT_CHUNK);
        unsigned carry_c = 0, carry_l = 0;               // <= 2^29 and <= 2^31
        for (unsigned first = 0; first < chunks; first += DSWX_OUTLINE_SCAN_STEP) {
            const unsigned c = first + threadIdx.x;
            const unsigned vc = c < chunks ? part[2ull * c] : 0u, vl = c < chunks ? part[2ull * c + 1] : 0u;
            unsigned tc, tl;
            const unsigned bc = out_block_scan(vc, wtot, &tc), bl = out_block_scan(vl, wtot, &tl);
            if (c < chunks) part[2ull * c] = carry_c + bc, part[2ull * c + 1] = carry_l + bl;
            carry_c += tc, carry_l += tl;
        }
        if (threadIdx.x == 0) {
            info->R = carry_c;
            if (a.head) {
                a.head[(unsigned long long)t * DSWX_OUTLINE_HEAD_WORDS + OUTLINE_HEAD_R] = carry_c;
                a.head[(unsigned long long)t * DSWX_OUTLINE_HEAD_WORDS + OUTLINE_HEAD_ROWS] = carry_c < a.max_rings ? carry_c : a.max_rings;
            }
        }
    }
}

// ---- launch 8: the row and the chain offset of every ring ----------------------------------------------------------------------
__global__ __launch_bounds__(OUT_BLOCK) void dswx_outline_ring_rank_k(const OutlineArgs a) {
    __shared__ unsigned wtot[OUT_WAVES];
    const unsigned long long first = (unsigned long long)blockIdx.x * OUT_CHUNK + (unsigned long long)threadIdx.x * OUT_PPT;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const OutlineInfo* const info = w_info(a, t);
        if (!info->ok) continue;                         // (uniform)
        const unsigned long long E = info->E;
        const out_u32x4* const st = w_state(a, t, info->fin);
        out_u32x4* const ring = w_state(a, t, info->fin ^ 1u);
        unsigned long long* const acc = w_acc(a, t);
        const unsigned* const ids = a.ids + (unsigned long long)t * a.n_elems;
        unsigned starts = 0, count = 0, length = 0;      // bit i: edge first + i starts a ring
        for (int i = 0; i < OUT_PPT && first + i < E; ++i)
            if (st[first + i].y == (unsigned)(first + i)) {
                starts |= 1u << i;
                ++count;
                length += ring[first + i].x;
            }
        unsigned tc, tl;
        unsigned r = out_block_scan(count, wtot, &tc), o = out_block_scan(length, wtot, &tl);
        r += w_part(a, t)[2ull * blockIdx.x];
        o += w_part(a, t)[2ull * blockIdx.x + 1];
        for (int i = 0; i < OUT_PPT; ++i)
            if ((starts >> i) & 1u) {
                const unsigned e = (unsigned)(first + i), L = ring[e].x, key = st[e].w;
                ring[e] = u32x4{L, r, o, 0u};
                acc[2ull * r] = 0ull, acc[2ull * r + 1] = 0ull;              // r < E / 4 <= cap / 4
                if (a.rings && r < a.max_rings) {
                    unsigned* const row = a.rings + ((unsigned long long)t * a.max_rings + r) * DSWX_OUTLINE_ROW_WORDS;
                    row[OUTLINE_ID] = ids[key >> 2];
                    row[OUTLINE_START] = key;
                    row[OUTLINE_OFFSET] = o;
                    row[OUTLINE_LENGTH] = L;
                }
                ++r;
                o += L;
            }
    }
}

// ---- launch 9: every edge to its place in the chain; the sums of the rings -----------------------------------------------------
__global__ __launch_bounds__(OUT_BLOCK) void dswx_outline_scatter_k(const OutlineArgs a) {
    const unsigned long long e = (unsigned long long)blockIdx.x * OUT_BLOCK + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const OutlineInfo* const info = w_info(a, t);
        if (!info->ok || (unsigned long long)blockIdx.x * OUT_BLOCK >= info->E) continue;          // (uniform)
        const out_u32x4* const st = w_state(a, t, info->fin);
        const out_u32x4* const ring = w_state(a, t, info->fin ^ 1u);
        unsigned r = OUT_NO_RING, corners = 0;
        long long area2 = 0;
        if (e < info->E) {
            const u32x4 s = st[e];
            const u32x4 g = ring[s.y];                   // {L, row, offset} of the ring's start
            r = g.y;
            if (a.chain) a.chain[(unsigned long long)t * a.max_edges + g.z + (s.z ? g.x - s.z : 0u)] = s.w;
            const unsigned p = s.w >> 2, y = p / a.width, x = p - y * a.width;
            area2 = outline_area2((int64_t)x, (int64_t)y, s.w & 3u);
            corners = s.x >> 31;
        }
        // the lanes of one ring that follow each other are summed into the last of them (a segmented scan): one set of
        // atomics per run; every lane takes part in the shuffles
        const unsigned before = __shfl_up(r, 1);
        bool head_of_run = lane == 0u || before != r;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long ua = out_shfl_up64(area2, o);
            const unsigned uc = __shfl_up(corners, o);
            const int uh = __shfl_up((int)head_of_run, o);
            if (lane >= (unsigned)o && !head_of_run) {
                area2 += ua;
                corners += uc;
                head_of_run = uh != 0;
            }
        }
        const unsigned after = __shfl_down(r, 1);
        if (r != OUT_NO_RING && (lane == 63u || after != r)) {
            unsigned long long* const acc = w_acc(a, t) + 2ull * r;
            if (area2) atomicAdd(acc, (unsigned long long)area2);
            if (corners) atomicAdd(acc + 1, (unsigned long long)corners);
        }
    }
}

// ---- launch 10: the sums into the rows and the head --------------------------------------------------------------------------
__global__ __launch_bounds__(OUT_BLOCK) void dswx_outline_finish_k(const OutlineArgs a) {
    __shared__ unsigned wtot[OUT_WAVES];
    const unsigned long long r = (unsigned long long)blockIdx.x * OUT_BLOCK + threadIdx.x;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        const OutlineInfo* const info = w_info(a, t);
        if (!info->ok || (unsigned long long)blockIdx.x * OUT_BLOCK >= info->R) continue;          // (uniform)
        unsigned outer = 0, holes = 0, corners = 0;
        if (r < info->R) {
            const unsigned long long* const acc = w_acc(a, t) + 2ull * r;
            const long long area2 = (long long)acc[0];
            corners = (unsigned)acc[1];
            outer = area2 > 0, holes = area2 < 0;
            if (a.rings && r < a.max_rings) {
                unsigned* const row = a.rings + ((unsigned long long)t * a.max_rings + r) * DSWX_OUTLINE_ROW_WORDS;
                row[OUTLINE_CORNERS] = corners;
                row[OUTLINE_AREA2] = (unsigned)acc[0];               // (rings need only be 4-byte aligned)
                row[OUTLINE_AREA2 + 1] = (unsigned)(acc[0] >> 32);
            }
        }
        if (!a.head) continue;                           // (uniform)
        unsigned to, th, tc;
        out_block_scan(outer, wtot, &to);
        out_block_scan(holes, wtot, &th);
        out_block_scan(corners, wtot, &tc);              // <= 256 rings of at most 2^31 corners in all
        if (threadIdx.x == 0) {
            unsigned long long* const head = a.head + (unsigned long long)t * DSWX_OUTLINE_HEAD_WORDS;
            if (to) atomicAdd(head + OUTLINE_HEAD_OUTER, (unsigned long long)to);
            if (th) atomicAdd(head + OUTLINE_HEAD_HOLES, (unsigned long long)th);
            if (tc) atomicAdd(head + OUTLINE_HEAD_CORNERS, (unsigned long long)tc);
        }
    }
}

// unaligned host accesses (a host buffer may sit at any address)
struct HostIds {
    const unsigned char* p;
    inline uint32_t operator()(uint64_t i) const { return dswx_load<uint32_t>(p, (size_t)i); }
};

// The checks that the entries share, in the house order: the arguments before any context, nothing written by a refused
// call.  `device`: the alignments, and the working memory.
int outline_check(const uint32_t* ids, const dswx_outline_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                  const dswx_outline_out_t* out, bool device, const void* work, uint64_t work_bytes) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (spec->connectivity != 4 && spec->connectivity != 8) return dswx_fail(DSWX_ERR_ARG, "connectivity %d is neither 4 nor 8", spec->connectivity);
    if (spec->reserved != 0) return dswx_fail(DSWX_ERR_ARG, "reserved is %d, not 0", spec->reserved);
    if (n_tiles < 0 || height < 0 || width < 0 || spec->max_edges < 0 || spec->max_rings < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (height > OUT_MAX_PIXELS || width > OUT_MAX_PIXELS || height * width > OUT_MAX_PIXELS)
        return dswx_fail(DSWX_ERR_ARG, "raster too large: height * width above 2^30, a key would not fit 32 bits");
    if (spec->max_edges > OUT_MAX_CAP) return dswx_fail(DSWX_ERR_ARG, "max_edges %lld above 2^31", (long long)spec->max_edges);
    if (spec->max_rings > OUT_MAX_CAP) return dswx_fail(DSWX_ERR_ARG, "max_rings %lld above 2^31", (long long)spec->max_rings);
    if (n_tiles > (1LL << 32)) return dswx_fail(DSWX_ERR_ARG, "plane too large: more than 2^32 tiles");
    if (!ids && n_tiles > 0 && height * width > 0) return dswx_fail(DSWX_ERR_ARG, "ids is NULL");
    if (!out->rings && spec->max_rings > 0) return dswx_fail(DSWX_ERR_ARG, "rings is NULL with max_rings %lld", (long long)spec->max_rings);
    if (!out->chain && out->rings) return dswx_fail(DSWX_ERR_ARG, "chain is NULL with rings wanted: a row names a place in the chain");
    if (device) {
        uint64_t need = 0;
        if (int rc = dswx_outline_work_bytes(spec, n_tiles, height, width, &need)) return rc;
        if (!work) return dswx_fail(DSWX_ERR_ARG, "work_device is NULL");
        if (work_bytes < need) return dswx_fail(DSWX_ERR_ARG, "work_bytes %llu below the %llu of dswx_outline_work_bytes", (unsigned long long)work_bytes, (unsigned long long)need);
        if (!aligned_to(ids, 4)) return dswx_fail(DSWX_ERR_ALIGN, "ids not 4-byte aligned");
        if (!aligned_to(out->chain, 4)) return dswx_fail(DSWX_ERR_ALIGN, "chain not 4-byte aligned");
        if (!aligned_to(out->rings, 4)) return dswx_fail(DSWX_ERR_ALIGN, "rings not 4-byte aligned");
        if (!aligned_to(out->head, 8)) return dswx_fail(DSWX_ERR_ALIGN, "head not 8-byte aligned");
        if (!aligned_to(work, 8)) return dswx_fail(DSWX_ERR_ALIGN, "work_device not 8-byte aligned");
    }
    return DSWX_OK;
}

}  // namespace

// The launches; the arguments have passed outline_check.
int dswx_outline_launch(dswx_ctx* ctx, const uint32_t* ids, const dswx_outline_spec_t* spec, int64_t n_tiles, int64_t height,
                        int64_t width, const dswx_outline_out_t* out, void* work, hipStream_t s) {
    if (n_tiles == 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    OutlineArgs a = {};
    a.ids = ids;
    a.work = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(work) + 15u) & ~(uintptr_t)15u);
    a.l = outline_layout(spec->max_edges, height, width);
    a.n_elems = (unsigned long long)(height * width);
    a.n_tiles = n_tiles;
    a.height = (unsigned)height;
    a.width = (unsigned)width;
    a.connectivity = spec->connectivity;
    a.max_edges = (unsigned long long)spec->max_edges;
    a.max_rings = (unsigned long long)spec->max_rings;
    a.chain = out->chain;
    a.rings = spec->max_rings > 0 ? out->rings : nullptr;
    a.head = reinterpret_cast<unsigned long long*>(out->head);
    const unsigned gy = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
    const dim3 block(OUT_BLOCK);
    if (a.chain && a.max_edges) HIP_TRY(hipMemsetAsync(a.chain, 0, (size_t)n_tiles * (size_t)a.max_edges * sizeof(uint32_t), s));
    if (a.rings) HIP_TRY(hipMemsetAsync(a.rings, 0, (size_t)n_tiles * (size_t)a.max_rings * DSWX_OUTLINE_ROW_WORDS * sizeof(uint32_t), s));
    // an empty raster has chunks_p == 0: only the scan runs, for E = 0 in the head
    if (a.l.chunks_p) hipLaunchKernelGGL(dswx_outline_count_k, dim3(a.l.chunks_p, gy), block, 0, s, a);
    hipLaunchKernelGGL(dswx_outline_scan_k, dim3(gy), block, 0, s, a);
    const unsigned edge_blocks = (unsigned)((a.l.cap + OUT_BLOCK - 1) / OUT_BLOCK);      // <= 2^23
    if (a.l.cap) {
        hipLaunchKernelGGL(dswx_outline_base_k, dim3(a.l.chunks_p, gy), block, 0, s, a);
        hipLaunchKernelGGL(dswx_outline_emit_k, dim3(a.l.chunks_p, gy), block, 0, s, a);
        for (unsigned k = 0; k < a.l.rounds; ++k) {
            a.round = k;
            hipLaunchKernelGGL(dswx_outline_jump_k, dim3(edge_blocks, gy), block, 0, s, a);
        }
        hipLaunchKernelGGL(dswx_outline_ring_count_k, dim3(a.l.chunks_e, gy), block, 0, s, a);
        hipLaunchKernelGGL(dswx_outline_ring_scan_k, dim3(gy), block, 0, s, a);
        hipLaunchKernelGGL(dswx_outline_ring_rank_k, dim3(a.l.chunks_e, gy), block, 0, s, a);
        hipLaunchKernelGGL(dswx_outline_scatter_k, dim3(edge_blocks, gy), block, 0, s, a);
        if (a.l.acc_blocks && (a.rings || a.head)) hipLaunchKernelGGL(dswx_outline_finish_k, dim3(a.l.acc_blocks, gy), block, 0, s, a);
    }
    HIP_TRY(hipGetLastError());
    char info[320];
    snprintf(info, sizeof info, "dswx_outline_count_k/base_k/emit_k grid=(%u,%u,1) block=%d chunk=%d + dswx_outline_scan_k/ring_scan_k grid=(%u,1,1) + dswx_outline_jump_k x %u and scatter_k grid=(%u,%u,1) + dswx_outline_ring_count_k/ring_rank_k grid=(%u,%u,1) + dswx_outline_finish_k grid=(%u,%u,1) connectivity=%d cap=%llu",
             a.l.chunks_p, gy, OUT_BLOCK, OUT_CHUNK, gy, a.l.cap ? a.l.rounds : 0u, edge_blocks, gy, a.l.chunks_e, gy, a.l.acc_blocks, gy, a.connectivity, a.l.cap);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_outline_work_bytes(const dswx_outline_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width, uint64_t* bytes) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!bytes) return dswx_fail(DSWX_ERR_ARG, "bytes is NULL");
    if (n_tiles < 0 || height < 0 || width < 0 || spec->max_edges < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (height > OUT_MAX_PIXELS || width > OUT_MAX_PIXELS || height * width > OUT_MAX_PIXELS)
        return dswx_fail(DSWX_ERR_ARG, "raster too large: height * width above 2^30, a key would not fit 32 bits");
    if (spec->max_edges > OUT_MAX_CAP) return dswx_fail(DSWX_ERR_ARG, "max_edges %lld above 2^31", (long long)spec->max_edges);
    if (n_tiles > (1LL << 32)) return dswx_fail(DSWX_ERR_ARG, "plane too large: more than 2^32 tiles");
    const OutlineLayout l = outline_layout(spec->max_edges, height, width);   // per_tile < 2^38
    if (n_tiles && l.per_tile > (1ull << 62) / (uint64_t)n_tiles) return dswx_fail(DSWX_ERR_ARG, "plane too large: the working memory would pass 2^62 bytes");
    *bytes = 16ull + (uint64_t)n_tiles * l.per_tile;     // 16: the entry rounds work_device up to 16 bytes
    return DSWX_OK;
}

int dswx_outline_host(const uint32_t* ids, const dswx_outline_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                      const dswx_outline_out_t* out) {
    if (int rc = outline_check(ids, spec, n_tiles, height, width, out, false, nullptr, 0)) return rc;
    const int64_t n = height * width, max_edges = spec->max_edges, max_rings = spec->max_rings;
    std::vector<unsigned char> todo((size_t)n);          // per pixel: its boundary edges that no ring has taken yet
    for (int64_t t = 0; t < n_tiles; ++t) {
        const HostIds get = {reinterpret_cast<const unsigned char*>(ids) + (size_t)t * (size_t)n * 4};
        unsigned char* const chain = out->chain ? reinterpret_cast<unsigned char*>(out->chain) + (size_t)t * (size_t)max_edges * 4 : nullptr;
        unsigned char* const rings = out->rings ? reinterpret_cast<unsigned char*>(out->rings) + (size_t)t * (size_t)max_rings * DSWX_OUTLINE_ROW_WORDS * 4 : nullptr;
        if (chain) std::memset(chain, 0, (size_t)max_edges * 4);
        if (rings) std::memset(rings, 0, (size_t)max_rings * DSWX_OUTLINE_ROW_WORDS * 4);
        uint64_t E = 0;
        for (int64_t y = 0; y < height; ++y)
            for (int64_t x = 0; x < width; ++x) {
                const uint32_t v = get((uint64_t)(y * width + x));
                const unsigned m = v ? outline_mask(get, x, y, width, height, v) : 0u;
                todo[(size_t)(y * width + x)] = (unsigned char)m;
                E += (uint64_t)__builtin_popcount(m);
            }
        uint64_t head[DSWX_OUTLINE_HEAD_WORDS] = {E, 0, 0, 0, 0, 0, 0, 0};
        if (E > (uint64_t)max_edges) head[OUTLINE_HEAD_OVERFLOW] = 1;
        else {
            uint64_t R = 0, at = 0;
            // the keys in rising order: an edge that no ring has taken is the smallest of its ring, so it starts the next one
            for (int64_t p = 0; p < n; ++p)
                for (unsigned d0 = 0; d0 < 4u && todo[(size_t)p]; ++d0) {
                    if (!((todo[(size_t)p] >> d0) & 1u)) continue;
                    const uint32_t v = get((uint64_t)p);
                    const uint64_t offset = at;
                    uint32_t corners = 0;
                    int64_t area2 = 0;
                    OutlineEdge e = {p % width, p / width, d0};
                    do {
                        const int64_t q = e.y * width + e.x;
                        todo[(size_t)q] = (unsigned char)(todo[(size_t)q] & ~(1u << e.d));
                        if (chain) dswx_store<uint32_t>(chain, (size_t)at, (uint32_t)(4 * q) + e.d);
                        ++at;
                        area2 += outline_area2(e.x, e.y, e.d);
                        const OutlineEdge f = outline_succ(get, e.x, e.y, e.d, width, height, v, spec->connectivity);
                        corners += f.d != e.d;
                        e = f;
                    } while ((e.y * width + e.x != p || e.d != d0) && at < E);   // (the map is a bijection: `at` never gets there)
                    if (rings && R < (uint64_t)max_rings) {
                        unsigned char* const row = rings + (size_t)R * DSWX_OUTLINE_ROW_WORDS * 4;
                        dswx_store<uint32_t>(row, OUTLINE_ID, v);
                        dswx_store<uint32_t>(row, OUTLINE_START, (uint32_t)(4 * p) + d0);
                        dswx_store<uint32_t>(row, OUTLINE_OFFSET, (uint32_t)offset);
                        dswx_store<uint32_t>(row, OUTLINE_LENGTH, (uint32_t)(at - offset));
                        dswx_store<uint32_t>(row, OUTLINE_CORNERS, corners);
                        dswx_store<uint64_t>(row + OUTLINE_AREA2 * 4, 0, (uint64_t)area2);
                    }
                    ++R;
                    head[OUTLINE_HEAD_OUTER] += area2 > 0;
                    head[OUTLINE_HEAD_HOLES] += area2 < 0;
                    head[OUTLINE_HEAD_CORNERS] += corners;
                }
            head[OUTLINE_HEAD_R] = R;
            head[OUTLINE_HEAD_ROWS] = R < (uint64_t)max_rings ? R : (uint64_t)max_rings;
            head[OUTLINE_HEAD_WRITTEN] = E;
        }
        if (out->head)
            for (int w = 0; w < DSWX_OUTLINE_HEAD_WORDS; ++w) dswx_store<uint64_t>(out->head, (size_t)(t * DSWX_OUTLINE_HEAD_WORDS + w), head[w]);
    }
    return DSWX_OK;
}

int dswx_outline_device(dswx_ctx_t* ctx, const uint32_t* ids, const dswx_outline_spec_t* spec, int64_t n_tiles, int64_t height,
                        int64_t width, const dswx_outline_out_t* out, void* work_device, uint64_t work_bytes, void* stream) {
    if (int rc = outline_check(ids, spec, n_tiles, height, width, out, true, work_device, work_bytes)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) { return dswx_outline_launch(ctx, ids, spec, n_tiles, height, width, out, work_device, s); });
}

}  // extern "C"
