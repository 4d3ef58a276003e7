// outline_host_san.cpp -- dswx_outline_host and dswx_outline_rule.h (proteus_amd/csrc/dswx_outline.hip) under ASan + UBSan on
// the CPU: the source is compiled INTO this program (tests/test_outline.py has the command line), which calls the host entry
// with the id plane and every output in heap blocks of exactly the bytes the entry may touch, at odd addresses inside them,
// and checks the result against what the definition demands, written out here another way: the chain is a permutation of the
// boundary edges counted by four comparisons per pixel; inside a ring every entry is followed by its successor, worked out
// here from the three pixels around the edge's end corner; a ring starts at its smallest key and the starts rise; offsets,
// lengths, corners and area2 are those of the chain; the head is their sum.  The planes are noise with few ids, noise with
// wild values (0xFFFFFFFF among them) and single regions.  No device, no context: the launch half of the source is linked
// but never called.  Prints one JSON line; exit status 0 = every case in order.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dswx_hip.h"

static char last_error[512];
int dswx_fail(int code, const char* fmt, ...) {          // (of dswx_hip.hip, which is not part of this program)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
    return code;
}

namespace {

uint32_t rng_state = 20261020u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// a heap block of exactly n + off bytes; the payload starts `off` bytes in, so one byte past it is outside the block
struct Block {
    uint8_t* mem;
    uint8_t* p;
    size_t n;
    Block(size_t n_, size_t off, int fill) : mem(static_cast<uint8_t*>(std::malloc(n_ + off ? n_ + off : 1))), p(mem + off), n(n_) {
        std::memset(mem, fill, n + off);
    }
    ~Block() { std::free(mem); }
    Block(const Block&) = delete;
};

uint32_t get_u32(const uint8_t* p, size_t i) {
    uint32_t v;
    std::memcpy(&v, p + 4 * i, 4);
    return v;
}
void put_u32(uint8_t* p, size_t i, uint32_t v) { std::memcpy(p + 4 * i, &v, 4); }
uint64_t get_u64(const uint8_t* p, size_t byte) {
    uint64_t v;
    std::memcpy(&v, p + byte, 8);
    return v;
}

struct Raster {
    const uint32_t* v;
    int64_t H, W;
    uint32_t at(int64_t x, int64_t y) const { return x < 0 || y < 0 || x >= W || y >= H ? 0u : v[y * W + x]; }
};

// The successor of a key, by the corner the edge ENDS at: of the four pixels around that corner, the one the edge belongs to
// (behind, on the region's side), the one across the edge, and the two ahead.
uint32_t successor(const Raster& r, uint32_t key, int conn) {
    static const int tx[4] = {1, 0, -1, 0}, ty[4] = {0, 1, 0, -1}, ox[4] = {0, 1, 0, -1}, oy[4] = {-1, 0, 1, 0};
    const int64_t p = key >> 2, x = p % r.W, y = p / r.W;
    const int d = (int)(key & 3u);
    const uint32_t v = r.v[p];
    const int64_t ax = x + tx[d], ay = y + ty[d], bx = ax + ox[d], by = ay + oy[d];
    const bool a = r.at(ax, ay) == v, b = r.at(bx, by) == v;
    const bool left = conn == 4 ? a && b : b, straight = !left && a && (conn == 4 ? true : !b);
    if (left) return (uint32_t)(4 * (by * r.W + bx)) + (uint32_t)((d + 3) % 4);
    if (straight) return (uint32_t)(4 * (ay * r.W + ax)) + (uint32_t)d;
    return (uint32_t)(4 * p) + (uint32_t)((d + 1) % 4);
}

// `want`: 0 head alone, 1 chain alone, 2 chain + head, 3 all three; `fit`: 0 exactly E, 1 room to spare, 2 one edge short
int run_case(int64_t T, int64_t H, int64_t W, int conn, int kind, size_t off, int want, int fit, int rows_mode) {
    const int64_t n = H * W;
    std::vector<uint32_t> ids((size_t)(T * n), 0u);
    const uint32_t wild[] = {0u, 0u, 1u, 2u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (auto& v : ids) v = kind == 0 ? rnd() % 3u : kind == 1 ? wild[rnd() % 8u] : kind == 2 ? 0xFFFFFFFFu : (rnd() % 100u < 60u ? 5u : 0u);
    // E and R per tile, counted here
    std::vector<uint64_t> E((size_t)T, 0);
    uint64_t e_max = 0;
    for (int64_t t = 0; t < T; ++t) {
        const Raster r = {ids.data() + t * n, H, W};
        for (int64_t y = 0; y < H; ++y)
            for (int64_t x = 0; x < W; ++x) {
                const uint32_t v = r.at(x, y);
                if (v) E[(size_t)t] += (r.at(x, y - 1) != v) + (r.at(x + 1, y) != v) + (r.at(x, y + 1) != v) + (r.at(x - 1, y) != v);
            }
        if (E[(size_t)t] > e_max) e_max = E[(size_t)t];
    }
    dswx_outline_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.connectivity = conn;
    spec.max_edges = fit == 0 ? (int64_t)e_max : fit == 1 ? (int64_t)e_max + 3 : e_max ? (int64_t)e_max - 1 : 0;
    spec.max_rings = want < 3 ? 0 : rows_mode == 0 ? (int64_t)(e_max / 4) : rows_mode == 1 ? (int64_t)(e_max / 4) + 2 : (int64_t)(e_max / 8);
    const int64_t ME = spec.max_edges, MR = spec.max_rings;
    Block plane(4 * (size_t)(T * n), 1 + off, 0);
    for (size_t i = 0; i < ids.size(); ++i) put_u32(plane.p, i, ids[i]);
    Block chain(4 * (size_t)(T * ME), 3 - (off % 3), 0xEE), rings(32 * (size_t)(T * MR), 1 + off, 0xEE), head(64 * (size_t)T, 5, 0xEE);
    dswx_outline_out_t out;
    std::memset(&out, 0, sizeof out);
    if (want >= 1) out.chain = reinterpret_cast<uint32_t*>(chain.p);
    if (want == 0 || want >= 2) out.head = reinterpret_cast<uint64_t*>(head.p);
    if (want >= 3 && MR > 0) out.rings = reinterpret_cast<uint32_t*>(rings.p);
    const int rc = dswx_outline_host(reinterpret_cast<const uint32_t*>(plane.p), &spec, T, H, W, &out);
    if (rc != DSWX_OK) {
        std::fprintf(stderr, "dswx_outline_host failed (%d): %s\n", rc, last_error);
        return 1;
    }
    int bad = 0;
    for (int64_t t = 0; t < T; ++t) {
        const Raster r = {ids.data() + t * n, H, W};
        const uint64_t e = E[(size_t)t];
        const bool over = e > (uint64_t)ME;
        uint64_t R = 0, outer = 0, holes = 0, corners_all = 0;
        if (out.chain) {
            const uint8_t* c = chain.p + 4 * (size_t)(t * ME);
            const uint64_t used = over ? 0 : e;
            for (uint64_t i = used; i < (uint64_t)ME; ++i) bad += get_u32(c, (size_t)i) != 0u;
            std::vector<uint8_t> seen((size_t)(4 * n), 0);
            uint64_t i = 0;
            uint32_t last_start = 0;
            while (i < used) {
                // a ring: from its start until the successor is the start again
                const uint32_t start = get_u32(c, (size_t)i);
                bad += R > 0 && start <= last_start;
                last_start = start;
                uint64_t j = i;
                uint32_t corners = 0;
                int64_t area2 = 0;
                for (;;) {
                    const uint32_t key = get_u32(c, (size_t)j);
                    if ((int64_t)(key >> 2) >= n || !r.v[key >> 2] || seen[key]) {
                        ++bad;
                        break;
                    }
                    seen[key] = 1;
                    bad += key < start;
                    const int64_t x = (int64_t)(key >> 2) % W, y = (int64_t)(key >> 2) / W;
                    const int d = (int)(key & 3u);
                    const int64_t x1 = x + (d == 1 || d == 2), y1 = y + (d == 2 || d == 3), x2 = x + (d == 0 || d == 1), y2 = y + (d == 1 || d == 2);
                    area2 += x1 * y2 - x2 * y1;
                    const uint32_t nx = successor(r, key, conn);
                    corners += (nx & 3u) != (key & 3u);
                    ++j;
                    if (nx == start) break;
                    if (j >= used || get_u32(c, (size_t)j) != nx) {
                        ++bad;
                        break;
                    }
                }
                if (out.rings && R < (uint64_t)MR) {
                    const uint8_t* g = rings.p + 32 * (size_t)(t * MR + (int64_t)R);
                    const uint32_t w32[6] = {r.v[start >> 2], start, (uint32_t)i, (uint32_t)(j - i), corners, 0u};
                    for (int w = 0; w < 6; ++w) bad += get_u32(g, (size_t)w) != w32[w];
                    bad += get_u64(g, 24) != (uint64_t)area2;
                }
                outer += area2 > 0, holes += area2 < 0, corners_all += corners;
                ++R;
                i = j;
            }
            if (!over) {                                             // every boundary edge is in the chain, once
                uint64_t in_chain = 0;
                for (auto s : seen) in_chain += s;
                bad += in_chain != e;
            }
            if (out.rings)
                for (int64_t k = (int64_t)(R < (uint64_t)MR ? R : (uint64_t)MR); k < MR; ++k)
                    for (int w = 0; w < 8; ++w) bad += get_u32(rings.p + 32 * (size_t)(t * MR + k), (size_t)w) != 0u;
        }
        if (out.head) {
            const uint8_t* h = head.p + 64 * (size_t)t;
            bad += get_u64(h, 0) != e || get_u64(h, 56) != (over ? 1u : 0u) || get_u64(h, 24) != (over ? 0u : e);
            if (over)
                for (int w = 1; w < 7; ++w) bad += get_u64(h, (size_t)(8 * w)) != 0u;
            else if (out.chain) {
                const uint64_t want_h[7] = {e, R, R < (uint64_t)MR ? R : (uint64_t)MR, e, outer, holes, corners_all};
                for (int w = 0; w < 7; ++w) bad += get_u64(h, (size_t)(8 * w)) != want_h[w];
            }
        }
    }
    // the outputs that were not wanted
    if (!out.head)
        for (size_t i = 0; i < head.n; ++i) bad += head.p[i] != 0xEE;
    if (!out.chain)
        for (size_t i = 0; i < chain.n; ++i) bad += chain.p[i] != 0xEE;
    if (!out.rings)
        for (size_t i = 0; i < rings.n; ++i) bad += rings.p[i] != 0xEE;
    if (bad)
        std::fprintf(stderr, "%lld x %lld x %lld, connectivity %d, kind %d, max_edges %lld, max_rings %lld, want %d: %d values differ\n", (long long)T,
                     (long long)H, (long long)W, conn, kind, (long long)ME, (long long)MR, want, bad);
    return bad != 0;
}

}  // namespace

int main() {
    int failures = 0, cases = 0;
    const int64_t shapes[][2] = {{1, 1}, {1, 19}, {23, 1}, {2, 3}, {5, 17}, {31, 33}, {33, 129}, {65, 100}};
    for (const auto& s : shapes)
        for (int kind = 0; kind < 4; ++kind)
            for (int64_t T : {0, 1, 3}) {
                failures += run_case(T, s[0], s[1], cases % 2 ? 8 : 4, kind, (size_t)(cases % 4), cases % 4, (cases / 4) % 3, (cases / 2) % 3);
                ++cases;
            }
    for (int i = 0; i < 8; ++i) {                                    // every output, fitting, both connectivities
        failures += run_case(2, 40, 37, i % 2 ? 8 : 4, i % 4, (size_t)i % 4, 3, i / 4, 0);
        ++cases;
    }
    // refusals read and write nothing: NULL or wild buffers would fault if they did
    dswx_outline_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.connectivity = 4;
    dswx_outline_out_t out;
    std::memset(&out, 0, sizeof out);
    out.head = reinterpret_cast<uint64_t*>(16);
    const uint32_t* wild_ids = reinterpret_cast<const uint32_t*>(16);
    failures += dswx_outline_host(wild_ids, &spec, 1, 1 << 15, (1 << 15) + 1, &out) != DSWX_ERR_ARG;
    failures += dswx_outline_host(wild_ids, nullptr, 1, 10, 10, &out) != DSWX_ERR_ARG;
    failures += dswx_outline_host(wild_ids, &spec, 1, 10, 10, nullptr) != DSWX_ERR_ARG;
    spec.connectivity = 6;
    failures += dswx_outline_host(wild_ids, &spec, 1, 10, 10, &out) != DSWX_ERR_ARG;
    spec.connectivity = 8;
    spec.reserved = 1;
    failures += dswx_outline_host(wild_ids, &spec, 1, 10, 10, &out) != DSWX_ERR_ARG;
    spec.reserved = 0;
    spec.max_rings = 3;
    failures += dswx_outline_host(wild_ids, &spec, 1, 10, 10, &out) != DSWX_ERR_ARG;                    // no rings
    out.rings = reinterpret_cast<uint32_t*>(16);
    failures += dswx_outline_host(wild_ids, &spec, 1, 10, 10, &out) != DSWX_ERR_ARG;                    // rings without a chain
    out.rings = nullptr;
    spec.max_rings = 0;
    spec.max_edges = -1;
    failures += dswx_outline_host(wild_ids, &spec, 1, 10, 10, &out) != DSWX_ERR_ARG;
    spec.max_edges = 0;
    failures += dswx_outline_host(nullptr, &spec, 1, 10, 10, &out) != DSWX_ERR_ARG;
    failures += dswx_outline_host(nullptr, &spec, 0, 10, 10, &out) != DSWX_OK;
    uint64_t bytes = 0;
    failures += dswx_outline_work_bytes(&spec, 3, 10, 10, &bytes) != DSWX_OK || bytes < 16;
    failures += dswx_outline_work_bytes(&spec, 3, 10, 10, nullptr) != DSWX_ERR_ARG;
    std::printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
    return failures ? 1 : 0;
}
