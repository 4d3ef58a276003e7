// dswx_label.hip -- the connected bodies of a plane (DSWX_HAS_LABEL, additive to ABI v7): per pixel the label and the size of
// its body, a sieved copy of the plane and a per-tile summary, without the plane crossing PCIe.  include/dswx_hip.h "label"
// states the definition; proteus_amd/label.py is its numpy statement (min-propagation to a fixed point) and dswx_label_host
// below the scalar one -- dswx_label_rule.h is compiled for both sides.
//
// The first entry whose result at a pixel depends on pixels arbitrarily far away: neither a reduction nor a stencil.  The
// algorithm is union-find in its LABEL-EQUIVALENCE form, and `label` is its working array from the first launch to the last:
//     label[p] == 0            p is not a member (never changes);
//     label[p] == 1 + parent   otherwise, with parent <= p ALWAYS (a pixel starts as its own parent or below, and a parent is
//                              only ever lowered: merging is atomicMin on the larger root).
// So a find walks STRICTLY DOWNWARD and ends at a root (label[r] == r + 1); the root of a finished body is its smallest
// index, which is the definition's label; and a flattened entry (1 + root) is itself a valid parent, so launch 3 may rewrite
// the plane in place while other threads still walk through it.  A reader that sees an OLD parent of a pixel sees an
// ancestor-or-former-ancestor of the same body: stale values cost steps, never correctness, and a union does not rely on
// what a find saw -- it relies on what its atomicMin RETURNED.
//
// NO WORKGROUP EVER WAITS FOR ANOTHER: no flag, no spin, no cooperative launch, no grid barrier.  What depends on a whole
// phase is the next launch on the stream.  EVERY LOOP TERMINATES: a static trip count, or a quantity that strictly decreases,
// stated at the loop.
//   1 dswx_label_local_k    a workgroup owns a rectangle of RECT_H x RECT_W = 32 x 128 pixels of one tile, a thread 16
//                           consecutive pixels of a row: one 16-byte load at any address (bytes past the row end or the tile
//                           are never counted, bytes past the tile never read), member bits from the 256-bit table in LDS
//                           (eight words in eight banks: conflict-free by construction), the row run inside the thread by bit
//                           arithmetic, then unions in LDS: a run with the run of the thread to its left, and with the row
//                           above -- one union per CONTACT, not per pixel (a pixel whose left neighbour in the same run made
//                           the same union skips it).  After a barrier every pixel finds its local root and writes label = 1 +
//                           the GLOBAL index of it, and zeroes size.  Row-major order inside the rectangle agrees with the
//                           tile's, so the local root is the smallest global index too.
//   2 dswx_label_seam_k     one thread per pixel of the left column and the top row of every rectangle; unions across the seam
//                           on the global plane (atomicMin, finds through agent-scope loads: other workgroups are merging in
//                           the same launch), the corner diagonals included for connectivity 8.  A pixel whose predecessor
//                           along the seam made the same union skips it: an all-member tile makes one union per rectangle
//                           and seam, not one per pixel.
//   3 dswx_label_flatten_k  every pixel finds its root and stores 1 + root; size[root] += pixels, equal roots combined first
//                           in the thread's 16 pixels (runs) and then across the wave (two rounds peel the two commonest
//                           roots; what is left adds for itself): a lake of ten million pixels is ten thousand atomics.
//   4 dswx_label_finish_k   size[root] to every member, sieved from the plane's byte, and the roots into the summary: partials
//                           of the workgroup in LDS, then 64-bit global atomics; words 2 and 3 travel as ONE key (label_key)
//                           under atomicMax in word 2.
//   5 dswx_label_key_k      unpacks that key into words 2 and 3 (one thread per tile).
// Launches 3 .. 5 treat a tile as a flat run of height * width elements.  DESIGN.md section 5 has the bytes per pixel of each
// launch and what was measured.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#include "dswx_host.h"
#include "dswx_label_rule.h"

namespace {

typedef u32x4 __attribute__((aligned(1))) u32x4_b;      // 16 bytes anywhere (the plane, sieved)
typedef u32x4 __attribute__((aligned(4))) u32x4_w;      // four uint32 at a 4-byte address (label, size)

constexpr int LABEL_BLOCK = 256;
constexpr int LABEL_PPT = 16;                            // pixels of a thread = bytes of a load
constexpr int RECT_H = DSWX_LABEL_RECT_H, RECT_W = DSWX_LABEL_RECT_W;
constexpr int LABEL_SEGS = RECT_W / LABEL_PPT;           // threads along a row of the rectangle
constexpr int LABEL_PEEL = 2;                            // rounds of wave-wide combining per run slot (launch 3)
constexpr int LABEL_CHUNK = LABEL_BLOCK * LABEL_PPT;     // elements of a workgroup in the flat launches
constexpr int64_t LABEL_MAX_PIXELS = 1LL << 31;
static_assert(RECT_H * LABEL_SEGS == LABEL_BLOCK, "one thread per 16 pixels of the rectangle");
static_assert(LABEL_PPT == 16, "a thread's member bits are a uint16 and its load is 16 bytes");

struct LabelArgs {
    const unsigned char* plane;
    unsigned long long stride;                           // bytes between tiles of the plane
    unsigned long long n_elems;                          // height * width <= 2^31
    long long n_tiles;
    unsigned height, width;                              // (each <= 2^31)
    unsigned rx, ry;                                     // rectangles across / down
    unsigned long long seam_v, seam_h;                   // seam pixels of a tile: (rx - 1) * height, (ry - 1) * width
    int conn8;
    unsigned min_size, replace;
    unsigned* label;
    unsigned* size;
    unsigned char* sieved;
    unsigned long long* summary;
    unsigned bits[8];                                    // member_of_byte as 256 bits
};

// ---- launch 1: a rectangle in LDS -------------------------------------------------------------------------------------------
// The root of p in the rectangle's array.  TERMINATES: lab[p] <= p always, so p strictly decreases until lab[p] == p.
__device__ __forceinline__ unsigned local_find(const volatile unsigned* lab, unsigned p) {
    for (unsigned q = lab[p]; q != p; q = lab[p]) p = q;
    return p;
}
// Unite the bodies of a and b.  TERMINATES: every round that does not return replaces the larger of two DIFFERENT roots by a
// strictly smaller index (the old value of lab[a], which is < a because it was not a itself), so a + b strictly decreases.
__device__ __forceinline__ void local_union(unsigned* lab, unsigned a, unsigned b) {
    for (;;) {
        a = local_find(lab, a);
        b = local_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        const unsigned old = atomicMin(lab + a, b);
        if (old == a) return;                            // a was still a root: it hangs below b now
        a = old;                                         // it was not: what it hung below must meet b too
    }
}

__global__ __launch_bounds__(LABEL_BLOCK) void dswx_label_local_k(const LabelArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned lab[RECT_H * RECT_W];
    __shared__ unsigned msk[LABEL_BLOCK];
    __shared__ unsigned bits[8];
    const unsigned tid = threadIdx.x;
    if (tid < 8) bits[tid] = a.bits[tid];
    const unsigned ryi = blockIdx.x / a.rx, rxi = blockIdx.x - ryi * a.rx;
    const unsigned lr = tid / LABEL_SEGS, seg = tid - lr * LABEL_SEGS;
    const unsigned y = ryi * RECT_H + lr, x = rxi * RECT_W + seg * LABEL_PPT;
    const int nv = y < a.height && x < a.width ? (a.width - x < (unsigned)LABEL_PPT ? (int)(a.width - x) : LABEL_PPT) : 0;
    const unsigned long long off = (unsigned long long)y * a.width + x;
    const unsigned base = tid * LABEL_PPT;               // local index of the thread's first pixel = lr * RECT_W + seg * 16
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        __syncthreads();                                 // (the table the first time; lab and msk of the tile before)
        // the bytes: one 16-byte load where it ends inside the tile, else the valid bytes one by one
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        const unsigned char* const tile = a.plane + (unsigned long long)t * a.stride;
        if (nv > 0) {
            if (off + LABEL_PPT <= a.n_elems) v = ldg_u<u32x4_b, u32x4, false>(tile + off);
            else
#pragma unroll
                for (int i = 0; i < LABEL_PPT; ++i)
                    if (i < nv) v[i / 4] |= (unsigned)tile[off + i] << (8 * (i % 4));
        }
        unsigned m = 0;
#pragma unroll
        for (int i = 0; i < LABEL_PPT; ++i)
            if (i < nv && label_is_member(bits, (v[i / 4] >> (8 * (i % 4))) & 0xffu)) m |= 1u << i;
        msk[tid] = m;
        // every member starts below the first pixel of its run inside the thread
        {
            unsigned start = 0, init[LABEL_PPT];
#pragma unroll
            for (int i = 0; i < LABEL_PPT; ++i) {
                if (!(i > 0 && ((m >> (i - 1)) & 1u))) start = (unsigned)i;
                init[i] = (m >> i) & 1u ? base + start : 0xFFFFFFFFu;
            }
#pragma unroll
            for (int i = 0; i < LABEL_PPT; i += 4)
                *reinterpret_cast<u32x4*>(lab + base + i) = u32x4{init[i], init[i + 1], init[i + 2], init[i + 3]};
        }
        __syncthreads();
        if (m) {
            // the run that begins the thread with the run that ends the thread to its left
            if ((m & 1u) && seg > 0 && (msk[tid - 1] >> (LABEL_PPT - 1))) local_union(lab, base, base - 1);
            if (lr > 0) {
                // the row above, columns x - 1 .. x + 16, as bits 0 .. 17
                const unsigned up = (seg > 0 ? msk[tid - LABEL_SEGS - 1] >> (LABEL_PPT - 1) : 0u) | (msk[tid - LABEL_SEGS] << 1) |
                                    (seg < LABEL_SEGS - 1 ? (msk[tid - LABEL_SEGS + 1] & 1u) << (LABEL_PPT + 1) : 0u);
#pragma unroll
                for (int i = 0; i < LABEL_PPT; ++i) {
                    if (!((m >> i) & 1u)) continue;
                    const unsigned p = base + i;
                    const bool prev = i > 0 && ((m >> (i - 1)) & 1u);        // the left neighbour is of the same run
                    const bool ul = (up >> i) & 1u, u = (up >> (i + 1)) & 1u, ur = (up >> (i + 2)) & 1u;
                    if (!a.conn8) {
                        // (prev && ul: the left neighbour met the pixel above IT, which is adjacent to the one above this)
                        if (u && !(prev && ul)) local_union(lab, p, p - RECT_W);
                    } else if (!prev) {
                        // the three above are adjacent to each other through the middle one: with it, one union does
                        if (u) local_union(lab, p, p - RECT_W);
                        else {
                            if (ul) local_union(lab, p, p - RECT_W - 1);
                            if (ur) local_union(lab, p, p - RECT_W + 1);
                        }
                    } else if (!u && ur) {
                        // the left neighbour has met up-left and up; up-right is new only where up does not join it
                        local_union(lab, p, p - RECT_W + 1);
                    }
                }
            }
        }
        __syncthreads();
        if (nv > 0) {
            unsigned out[LABEL_PPT];
            unsigned prev_root = 0;
#pragma unroll
            for (int i = 0; i < LABEL_PPT; ++i) {
                out[i] = 0u;
                if ((m >> i) & 1u) {
                    // (a pixel of the same run as its left neighbour has that neighbour's root)
                    const unsigned r = i > 0 && ((m >> (i - 1)) & 1u) ? prev_root : local_find(lab, base + i);
                    prev_root = r;
                    const unsigned rr = r / RECT_W, rc = r - rr * RECT_W;
                    out[i] = 1u + (unsigned)((unsigned long long)(ryi * RECT_H + rr) * a.width + (rxi * RECT_W + rc));
                }
            }
            unsigned* const lp = a.label + (unsigned long long)t * a.n_elems + off;
            unsigned* const sp = a.size ? a.size + (unsigned long long)t * a.n_elems + off : nullptr;
            if (nv == LABEL_PPT) {
#pragma unroll
                for (int i = 0; i < LABEL_PPT; i += 4) {
                    *reinterpret_cast<u32x4_w*>(lp + i) = u32x4{out[i], out[i + 1], out[i + 2], out[i + 3]};
                    if (sp) *reinterpret_cast<u32x4_w*>(sp + i) = u32x4{0u, 0u, 0u, 0u};
                }
            } else {
#pragma unroll
                for (int i = 0; i < LABEL_PPT; ++i)
                    if (i < nv) {
                        lp[i] = out[i];
                        if (sp) sp[i] = 0u;
                    }
            }
        }
    }
}

// ---- launch 2: the seams, on the global plane -------------------------------------------------------------------------------
// Other workgroups lower parents while this one reads them, so a find reads through agent-scope loads (past this CU's L1).
// TERMINATES: label[p] <= p + 1 always, so p strictly decreases until label[p] == p + 1.  (p is a member, and the parent of a
// member is a member: the value read is never 0.)
__device__ __forceinline__ unsigned seam_find(unsigned* lab, unsigned p) {
    for (unsigned q = __hip_atomic_load(lab + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); q != p + 1u;
         q = __hip_atomic_load(lab + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        p = q - 1u;
    return p;
}
// TERMINATES as local_union does: a + b strictly decreases, because the value that atomicMin returns for a pixel that was no
// longer a root is below that pixel.  What a find saw may be stale; only the returned value decides.
__device__ __forceinline__ void seam_union(unsigned* lab, unsigned a, unsigned b) {
    for (;;) {
        a = seam_find(lab, a);
        b = seam_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        const unsigned old = atomicMin(lab + a, b + 1u);
        if (old == a + 1u) return;
        a = old - 1u;
    }
}

__global__ __launch_bounds__(LABEL_BLOCK) void dswx_label_seam_k(const LabelArgs a) {
    const unsigned long long k = (unsigned long long)blockIdx.x * LABEL_BLOCK + threadIdx.x;
    if (k >= a.seam_v + a.seam_h) return;                // (no barrier in this kernel)
    const unsigned long long W = a.width;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        unsigned* const lab = a.label + (unsigned long long)t * a.n_elems;
        if (k < a.seam_v) {
            // pixel (y, x) of the left column of a rectangle against column x - 1
            const unsigned s = (unsigned)(k / a.height), y = (unsigned)(k - (unsigned long long)s * a.height);
            const unsigned x = (s + 1u) * RECT_W;
            const unsigned p = (unsigned)(y * W + x);
            if (!lab[p]) continue;
            if (lab[p - 1]) {
                // the pixel above is of the same rectangle and met ITS left neighbour, which is adjacent to this one's
                const bool same = (y % RECT_H) != 0 && lab[p - W] && lab[p - W - 1];
                if (!same) seam_union(lab, p, p - 1);
            } else if (a.conn8) {
                if (y > 0 && lab[p - W - 1]) seam_union(lab, p, (unsigned)(p - W - 1));
                if (y + 1 < a.height && lab[p + W - 1]) seam_union(lab, p, (unsigned)(p + W - 1));
            }
        } else {
            // pixel (y, x) of the top row of a rectangle against row y - 1
            const unsigned long long kh = k - a.seam_v;
            const unsigned s = (unsigned)(kh / a.width), x = (unsigned)(kh - (unsigned long long)s * a.width);
            const unsigned y = (s + 1u) * RECT_H;
            const unsigned p = (unsigned)(y * W + x);
            if (!lab[p]) continue;
            const bool prev = (x % RECT_W) != 0 && lab[p - 1];               // the left neighbour, of the same rectangle
            const bool u = lab[p - W], ul = x > 0 && lab[p - W - 1], ur = x + 1 < a.width && lab[p - W + 1];
            if (!a.conn8) {
                if (u && !(prev && ul)) seam_union(lab, p, (unsigned)(p - W));
            } else if (!prev) {
                if (u) seam_union(lab, p, (unsigned)(p - W));
                else {
                    if (ul) seam_union(lab, p, (unsigned)(p - W - 1));
                    if (ur) seam_union(lab, p, (unsigned)(p - W + 1));
                }
            } else if (!u && ur) {
                seam_union(lab, p, (unsigned)(p - W + 1));
            }
        }
    }
}

// ---- launches 3 and 4: a tile as a flat run of elements ---------------------------------------------------------------------
// Nobody merges any more: roots are final.  Other threads of this launch replace parents by roots meanwhile, and either is an
// ancestor.  TERMINATES: label[p] <= p + 1, p strictly decreases.
__device__ __forceinline__ unsigned flat_find(const unsigned* lab, unsigned p) {
    for (unsigned q = lab[p]; q != p + 1u; q = lab[p]) p = q - 1u;
    return p;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the 16 elements at `first` of a uint32 plane of n elements; those behind the end are 0
__device__ __forceinline__ void load16(const unsigned* plane, unsigned long long first, unsigned long long n, unsigned (&v)[LABEL_PPT]) {
    if (first + LABEL_PPT <= n) {
#pragma unroll
        for (int i = 0; i < LABEL_PPT; i += 4) {
            const u32x4 q = *reinterpret_cast<const u32x4_w*>(plane + first + i);
            v[i] = q.x, v[i + 1] = q.y, v[i + 2] = q.z, v[i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < LABEL_PPT; ++i) v[i] = first + i < n ? plane[first + i] : 0u;
    }
}
__device__ __forceinline__ void store16(unsigned* plane, unsigned long long first, unsigned long long n, const unsigned (&v)[LABEL_PPT]) {
    if (first + LABEL_PPT <= n) {
#pragma unroll
        for (int i = 0; i < LABEL_PPT; i += 4) *reinterpret_cast<u32x4_w*>(plane + first + i) = u32x4{v[i], v[i + 1], v[i + 2], v[i + 3]};
    } else {
#pragma unroll
        for (int i = 0; i < LABEL_PPT; ++i)
            if (first + i < n) plane[first + i] = v[i];
    }
}

__global__ __launch_bounds__(LABEL_BLOCK) void dswx_label_flatten_k(const LabelArgs a) {
    const unsigned long long first = ((unsigned long long)blockIdx.x * LABEL_BLOCK + threadIdx.x) * LABEL_PPT;
    const unsigned lane = threadIdx.x & 63u;
    // (no thread leaves early: the wave-wide steps below need every lane; a thread behind the tile has no member)
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        unsigned* const lab = a.label + (unsigned long long)t * a.n_elems;
        unsigned v[LABEL_PPT];
        bool any = false;
        if (first < a.n_elems) {
            load16(lab, first, a.n_elems, v);
            unsigned parent_before = 0;
#pragma unroll
            for (int i = 0; i < LABEL_PPT; ++i) {
                const unsigned parent = v[i];
                // (the parent of the element before: the same root, without a second walk)
                if (parent) v[i] = i > 0 && parent == parent_before ? v[i - 1] : 1u + flat_find(lab, parent - 1u);
                any = any || parent;
                parent_before = parent;
            }
            if (any) store16(lab, first, a.n_elems, v);
        } else {
#pragma unroll
            for (int i = 0; i < LABEL_PPT; ++i) v[i] = 0u;
        }
        if (!a.size) continue;                           // (uniform)
        unsigned* const size = a.size + (unsigned long long)t * a.n_elems;
        // Runs of equal labels inside the thread; the run that ENDS at element i is handed in at step i by every lane at once.
        unsigned run = 0;
#pragma unroll
        for (int i = 0; i < LABEL_PPT; ++i) {
            run = v[i] ? run + 1u : 0u;
            bool pend = v[i] && (i == LABEL_PPT - 1 || v[i + 1 < LABEL_PPT ? i + 1 : i] != v[i]);
            const unsigned cnt = run;
            if (pend) run = 0u;
            if (!__any(pend)) continue;                  // (wave-uniform)
            // Two rounds: the label of the first lane that still has a run, summed over every lane that has the same.
#pragma unroll
            for (int round = 0; round < LABEL_PEEL; ++round) {
                const unsigned long long todo = __ballot(pend);
                if (!todo) break;                        // (wave-uniform)
                const int leader = __ffsll((long long)todo) - 1;
                const unsigned r = __shfl(v[i], leader);
                const bool match = pend && v[i] == r;
                const unsigned sum = wave_sum(match ? cnt : 0u);
                if (lane == (unsigned)leader) atomicAdd(size + (r - 1u), sum);
                pend = pend && !match;
            }
            if (pend) atomicAdd(size + (v[i] - 1u), cnt);
        }
    }
}

__global__ __launch_bounds__(LABEL_BLOCK) void dswx_label_finish_k(const LabelArgs a) {
    __shared__ unsigned long long part[DSWX_LABEL_SUMMARY_WORDS];
    const unsigned long long first = ((unsigned long long)blockIdx.x * LABEL_BLOCK + threadIdx.x) * LABEL_PPT;
    for (long long t = blockIdx.y; t < a.n_tiles; t += gridDim.y) {
        if (a.summary) {
            if (threadIdx.x < DSWX_LABEL_SUMMARY_WORDS) part[threadIdx.x] = 0ull;
            __syncthreads();
        }
        if (first < a.n_elems) {
            const unsigned* const lab = a.label + (unsigned long long)t * a.n_elems;
            unsigned* const size = a.size + (unsigned long long)t * a.n_elems;
            unsigned v[LABEL_PPT], sz[LABEL_PPT];
            load16(lab, first, a.n_elems, v);
            unsigned members = 0;
            bool any = false;
#pragma unroll
            for (int i = 0; i < LABEL_PPT; ++i) {
                sz[i] = 0u;
                if (!v[i]) continue;
                any = true;
                ++members;
                // only the entries of roots are read, and only entries that are not a root's are written: no race
                sz[i] = i > 0 && v[i] == v[i - 1] ? sz[i - 1] : size[v[i] - 1u];
                if (a.summary && (unsigned long long)v[i] == first + i + 1u) {           // a root: one body
                    atomicAdd(&part[0], 1ull);
                    atomicMax(&part[2], (unsigned long long)label_key(sz[i], v[i]));
                    if (sz[i] >= a.min_size) {
                        atomicAdd(&part[4], 1ull);
                        atomicAdd(&part[5], (unsigned long long)sz[i]);
                    }
                    atomicAdd(&part[8 + label_size_bin(sz[i])], 1ull);
                }
            }
            if (any) store16(size, first, a.n_elems, sz);
            if (a.summary && members) atomicAdd(&part[1], (unsigned long long)members);
            if (a.sieved) {
                const unsigned char* const src = a.plane + (unsigned long long)t * a.stride + first;
                unsigned char* const dst = a.sieved + (unsigned long long)t * a.n_elems + first;
                if (first + LABEL_PPT <= a.n_elems) {
                    u32x4 b = ldg_u<u32x4_b, u32x4, false>(src);
#pragma unroll
                    for (int i = 0; i < LABEL_PPT; ++i) {
                        const unsigned byte = (b[i / 4] >> (8 * (i % 4))) & 0xffu;
                        const unsigned o = label_sieve(byte, v[i] != 0u, sz[i], a.min_size, a.replace);
                        b[i / 4] = (b[i / 4] & ~(0xffu << (8 * (i % 4)))) | (o << (8 * (i % 4)));
                    }
                    stg_u<u32x4_b, u32x4, false>(dst, b);
                } else {
#pragma unroll
                    for (int i = 0; i < LABEL_PPT; ++i)
                        if (first + i < a.n_elems) dst[i] = (unsigned char)label_sieve(src[i], v[i] != 0u, sz[i], a.min_size, a.replace);
                }
            }
        }
        if (a.summary) {
            __syncthreads();
            if (threadIdx.x < DSWX_LABEL_SUMMARY_WORDS && part[threadIdx.x]) {
                unsigned long long* const w = a.summary + (unsigned long long)t * DSWX_LABEL_SUMMARY_WORDS + threadIdx.x;
                if (threadIdx.x == 2) atomicMax(w, part[2]);
                else atomicAdd(w, part[threadIdx.x]);
            }
            __syncthreads();                             // (the partials are zeroed again for the next tile)
        }
    }
}

__global__ void dswx_label_key_k(unsigned long long* summary, long long n_tiles) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const unsigned long long key = summary[t * DSWX_LABEL_SUMMARY_WORDS + 2];
    summary[t * DSWX_LABEL_SUMMARY_WORDS + 2] = label_key_size(key);
    summary[t * DSWX_LABEL_SUMMARY_WORDS + 3] = label_key_label(key);
}

// The scalar union-find of the host entry, on the caller's label plane in the encoding of the kernels (0 / 1 + parent).
// TERMINATES: the parent of p is at most p, so p strictly decreases; the walk halves the path behind it.
inline uint32_t host_find(uint32_t* lab, uint32_t p) {
    for (;;) {
        const uint32_t q = dswx_load<uint32_t>(lab, p) - 1u;
        if (q == p) return p;
        const uint32_t g = dswx_load<uint32_t>(lab, q);              // (the grandparent, <= q + 1: still at or below p)
        dswx_store<uint32_t>(lab, p, g);
        p = q;
    }
}
inline void host_union(uint32_t* lab, uint32_t a, uint32_t b) {
    a = host_find(lab, a);
    b = host_find(lab, b);
    if (a == b) return;
    if (a < b) dswx_store<uint32_t>(lab, b, a + 1u);
    else dswx_store<uint32_t>(lab, a, b + 1u);
}

}  // namespace

// The checks that the device and the host entry share, in the house order: the arguments before any context, nothing
// written by a refused call.  `align` = label and size must be 4-byte and summary 8-byte aligned (the device entry).
int dswx_label_check(const uint8_t* plane, const dswx_label_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                     int64_t* stride, const dswx_label_out_t* out, bool align) {
    if (!spec) return dswx_fail(DSWX_ERR_ARG, "spec is NULL");
    if (!out) return dswx_fail(DSWX_ERR_ARG, "out is NULL");
    if (spec->connectivity != 4 && spec->connectivity != 8)
        return dswx_fail(DSWX_ERR_ARG, "connectivity %d: 4 or 8", spec->connectivity);
    if (spec->replace < 0 || spec->replace > 255) return dswx_fail(DSWX_ERR_ARG, "replace %d outside 0 .. 255", spec->replace);
    if (spec->min_size == 0) return dswx_fail(DSWX_ERR_ARG, "min_size is 0: at least 1");
    if (n_tiles < 0 || height < 0 || width < 0 || *stride < 0) return dswx_fail(DSWX_ERR_ARG, "negative size");
    if (height > LABEL_MAX_PIXELS || width > LABEL_MAX_PIXELS || height * width > LABEL_MAX_PIXELS)
        return dswx_fail(DSWX_ERR_ARG, "raster too large: height * width above 2^31, a label would not fit 32 bits");
    const int64_t n_elems = height * width;
    if (int rc = dswx_tile_geometry_check(plane, n_tiles, n_elems, stride, true)) return rc;
    if (!out->label) return dswx_fail(DSWX_ERR_ARG, "label is NULL: it is the working array and always required");
    if (!out->size && (out->sieved || out->summary))
        return dswx_fail(DSWX_ERR_ARG, "size is NULL but %s is wanted: size is required for it", out->sieved ? "sieved" : "summary");
    if (align) {
        if (!aligned_to(out->label, 4)) return dswx_fail(DSWX_ERR_ALIGN, "label not 4-byte aligned");
        if (!aligned_to(out->size, 4)) return dswx_fail(DSWX_ERR_ALIGN, "size not 4-byte aligned");
        if (!aligned_to(out->summary, 8)) return dswx_fail(DSWX_ERR_ALIGN, "summary not 8-byte aligned");
    }
    return DSWX_OK;
}

// The launches; the arguments have passed dswx_label_check (stride resolved).
int dswx_label_launch(dswx_ctx* ctx, const uint8_t* plane, const dswx_label_spec_t* spec, int64_t n_tiles, int64_t height,
                      int64_t width, int64_t stride, const dswx_label_out_t* out, hipStream_t s) {
    if (n_tiles == 0 || height == 0 || width == 0) {
        ctx->last_kernel = DSWX_NO_KERNEL;
        return DSWX_OK;
    }
    LabelArgs a = {};
    a.plane = plane;
    a.stride = (unsigned long long)stride;
    a.n_elems = (unsigned long long)(height * width);
    a.n_tiles = n_tiles;
    a.height = (unsigned)height;
    a.width = (unsigned)width;
    a.rx = (unsigned)((width + RECT_W - 1) / RECT_W);
    a.ry = (unsigned)((height + RECT_H - 1) / RECT_H);
    a.seam_v = (unsigned long long)(a.rx - 1) * a.height;
    a.seam_h = (unsigned long long)(a.ry - 1) * a.width;
    a.conn8 = spec->connectivity == 8;
    a.min_size = spec->min_size;
    a.replace = (unsigned)spec->replace;
    a.label = out->label;
    a.size = out->size;
    a.sieved = out->sieved;
    a.summary = reinterpret_cast<unsigned long long*>(out->summary);
    label_member_bits(spec->member_of_byte, a.bits);
    // (height * width <= 2^31: at most 2^19 rectangles or chunks and 2^23 blocks of seam pixels -- every grid.x fits)
    const unsigned gy = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
    const unsigned rects = a.rx * a.ry;
    const unsigned chunks = (unsigned)((a.n_elems + LABEL_CHUNK - 1) / LABEL_CHUNK);
    const unsigned long long seams = a.seam_v + a.seam_h;
    const dim3 block(LABEL_BLOCK);
    if (out->summary) HIP_TRY(hipMemsetAsync(out->summary, 0, (size_t)n_tiles * DSWX_LABEL_SUMMARY_WORDS * sizeof(uint64_t), s));
    hipLaunchKernelGGL(dswx_label_local_k, dim3(rects, gy), block, 0, s, a);
    if (seams) hipLaunchKernelGGL(dswx_label_seam_k, dim3((unsigned)((seams + LABEL_BLOCK - 1) / LABEL_BLOCK), gy), block, 0, s, a);
    hipLaunchKernelGGL(dswx_label_flatten_k, dim3(chunks, gy), block, 0, s, a);
    if (out->size) hipLaunchKernelGGL(dswx_label_finish_k, dim3(chunks, gy), block, 0, s, a);
    if (out->summary)
        hipLaunchKernelGGL(dswx_label_key_k, dim3((unsigned)((n_tiles + LABEL_BLOCK - 1) / LABEL_BLOCK)), block, 0, s, a.summary,
                           (long long)n_tiles);
    HIP_TRY(hipGetLastError());
    char info[256];
    snprintf(info, sizeof info, "dswx_label_local_k grid=(%u,%u,1) block=%d rect=%dx%d + seam_k pixels=%llu + flatten_k/finish_k grid=(%u,%u,1) connectivity=%d",
             rects, gy, LABEL_BLOCK, RECT_H, RECT_W, seams, chunks, gy, a.conn8 ? 8 : 4);
    ctx->last_kernel = info;
    return DSWX_OK;
}

extern "C" {

int dswx_label_host(const uint8_t* plane, const dswx_label_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                    int64_t stride, const dswx_label_out_t* out) {
    if (int rc = dswx_label_check(plane, spec, n_tiles, height, width, &stride, out, false)) return rc;
    if (n_tiles == 0 || height == 0 || width == 0) return DSWX_OK;
    const int64_t n = height * width;
    const bool conn8 = spec->connectivity == 8;
    uint32_t bits[8];
    label_member_bits(spec->member_of_byte, bits);
    for (int64_t t = 0; t < n_tiles; ++t) {
        const uint8_t* tile = plane + (size_t)t * (size_t)stride;
        uint32_t* lab = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(out->label) + (size_t)t * (size_t)n * 4);
        // one pass in raster order: a member starts as its own root and meets the members before it
        for (int64_t y = 0; y < height; ++y)
            for (int64_t x = 0; x < width; ++x) {
                const int64_t p = y * width + x;
                if (!label_is_member(bits, tile[p])) {
                    dswx_store<uint32_t>(lab, p, 0u);
                    continue;
                }
                dswx_store<uint32_t>(lab, p, (uint32_t)p + 1u);
                if (x > 0 && dswx_load<uint32_t>(lab, p - 1)) host_union(lab, (uint32_t)p, (uint32_t)(p - 1));
                if (y > 0) {
                    if (dswx_load<uint32_t>(lab, p - width)) host_union(lab, (uint32_t)p, (uint32_t)(p - width));
                    if (conn8 && x > 0 && dswx_load<uint32_t>(lab, p - width - 1)) host_union(lab, (uint32_t)p, (uint32_t)(p - width - 1));
                    if (conn8 && x + 1 < width && dswx_load<uint32_t>(lab, p - width + 1)) host_union(lab, (uint32_t)p, (uint32_t)(p - width + 1));
                }
            }
        // in rising order the parent of a pixel is flat already when the pixel is reached
        uint32_t* size = out->size ? reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(out->size) + (size_t)t * (size_t)n * 4) : nullptr;
        for (int64_t p = 0; p < n; ++p) {
            const uint32_t v = dswx_load<uint32_t>(lab, p);
            if (size) dswx_store<uint32_t>(size, p, 0u);
            if (!v) continue;
            const uint32_t r = dswx_load<uint32_t>(lab, v - 1u);
            dswx_store<uint32_t>(lab, p, r);
            if (size) dswx_store<uint32_t>(size, r - 1u, dswx_load<uint32_t>(size, r - 1u) + 1u);
        }
        if (!size) continue;
        uint64_t sum[DSWX_LABEL_SUMMARY_WORDS] = {};
        uint64_t key = 0;
        for (int64_t p = 0; p < n; ++p) {
            const uint32_t v = dswx_load<uint32_t>(lab, p);
            const uint32_t sz = v ? dswx_load<uint32_t>(size, v - 1u) : 0u;                  // (a root is before its pixels: still its count)
            if (v && (int64_t)v != p + 1) dswx_store<uint32_t>(size, p, sz);
            if (out->sieved) out->sieved[(size_t)t * (size_t)n + (size_t)p] = (uint8_t)label_sieve(tile[p], v != 0u, sz, spec->min_size, (unsigned)spec->replace);
            if (!v) continue;
            ++sum[1];
            if ((int64_t)v != p + 1) continue;
            ++sum[0];
            const uint64_t k = label_key(sz, v);
            if (k > key) key = k;
            if (sz >= spec->min_size) {
                ++sum[4];
                sum[5] += sz;
            }
            ++sum[8 + label_size_bin(sz)];
        }
        sum[2] = label_key_size(key);
        sum[3] = label_key_label(key);
        if (out->summary)
            for (int w = 0; w < DSWX_LABEL_SUMMARY_WORDS; ++w) dswx_store<uint64_t>(out->summary, t * DSWX_LABEL_SUMMARY_WORDS + w, sum[w]);
    }
    return DSWX_OK;
}

int dswx_label_device(dswx_ctx_t* ctx, const uint8_t* plane, const dswx_label_spec_t* spec, int64_t n_tiles, int64_t height,
                      int64_t width, int64_t stride, const dswx_label_out_t* out, void* stream) {
    if (int rc = dswx_label_check(plane, spec, n_tiles, height, width, &stride, out, true)) return rc;
    return dswx_device_entry(ctx, stream, [&](hipStream_t s) { return dswx_label_launch(ctx, plane, spec, n_tiles, height, width, stride, out, s); });
}

}  // extern "C"
