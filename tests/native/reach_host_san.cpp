// reach_host_san.cpp -- dswx_reach_host (proteus_amd/csrc/dswx_reach.hip and dswx_burn.hip, whose checks it shares, compiled
// into this program) and the rule header under ASan + UBSan on the HOST: every buffer in a heap block of exactly the bytes the
// entry may touch, at odd addresses.  No device is used: the kernels of the translation units are compiled and never launched.
// tests/test_reach.py builds and runs it as a child process; the last line of standard output is a JSON record.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dswx_hip.h"

static char g_error[512];
int dswx_fail(int code, const char* fmt, ...) {          // (of dswx_hip.hip, which is not part of this program)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return code;
}

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return g_state;
}
int64_t rnd_in(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

// A heap block of exactly `bytes` bytes whose payload begins `off` bytes in: ASan sees the first byte past either end.
struct Block {
    std::vector<unsigned char>* raw;
    unsigned char* p;
    Block(size_t bytes, size_t off, int fill) : raw(new std::vector<unsigned char>(bytes + off, (unsigned char)fill)), p(raw->data() + off) {}
    ~Block() { delete raw; }
};

// The definition once more, per pixel and per edge.  128 bits do not hold (u x d)^2 at the extremes, so the last line compares
// |u x d| / sqrt(D) with R as a product of two 128-bit halves: (u x d)^2 <= R^2 D with both sides split at 2^64.
typedef unsigned __int128 u128;
struct U256 {
    u128 hi, lo;
};
U256 mul(u128 a, u128 b) {                               // a, b < 2^128
    const u128 m = ((u128)1 << 64) - 1, a0 = a & m, a1 = a >> 64, b0 = b & m, b1 = b >> 64;
    const u128 p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const u128 mid = (p00 >> 64) + (p01 & m) + (p10 & m);
    return {p11 + (p01 >> 64) + (p10 >> 64) + (mid >> 64), (mid << 64) | (p00 & m)};
}
bool le(const U256& a, const U256& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo <= b.lo); }

uint32_t pixel(const std::vector<dswx_burn_vertex_t>& v, int64_t c, int64_t r, int64_t R) {
    const __int128 px = 256 * c + 128, py = 256 * r + 128, m = DSWX_BURN_MAX_COORD;
    uint32_t acc = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        if (v[i].next >= v.size()) continue;
        const __int128 ax = v[i].x, ay = v[i].y, bx = v[v[i].next].x, by = v[v[i].next].y;
        if (ax > m || ax < -m || ay > m || ay < -m || bx > m || bx < -m || by > m || by < -m) continue;
        const __int128 dx = bx - ax, dy = by - ay, ux = px - ax, uy = py - ay, D = dx * dx + dy * dy, t = ux * dx + uy * dy;
        bool hit;
        if (D == 0 || t <= 0) hit = ux * ux + uy * uy <= (__int128)R * R;
        else if (t >= D) hit = (px - bx) * (px - bx) + (py - by) * (py - by) <= (__int128)R * R;
        else {
            __int128 cr = ux * dy - uy * dx;
            if (cr < 0) cr = -cr;
            hit = le(mul((u128)cr, (u128)cr), mul((u128)((__int128)R * R), (u128)D));
        }
        acc += hit;
    }
    return acc;
}

int one_case(int64_t n_tiles, int64_t H, int64_t W, int kind, size_t off) {
    std::vector<std::vector<dswx_burn_vertex_t>> tiles((size_t)n_tiles);
    std::vector<int64_t> first((size_t)n_tiles + 1, 0);
    const int64_t m = DSWX_BURN_MAX_COORD;
    // kind 0: no records; 1: small coordinates, a small radius; 2: multiples of 128 (centres ON edges and circles), radius a
    // multiple of 128; 3: the extremes, legal and just past it, with the largest radius
    const int64_t R = kind == 1 ? rnd_in(0, 1500) : kind == 2 ? 128 * rnd_in(0, 12) : kind == 3 ? DSWX_REACH_MAX_RADIUS - (int64_t)(rnd() % 3) : 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t count = kind == 0 ? 0 : rnd_in(0, 9);
        for (int64_t i = 0; i < count; ++i) {
            dswx_burn_vertex_t q;
            if (kind == 1) q.x = (int32_t)rnd_in(-6 * 256, 18 * 256), q.y = (int32_t)rnd_in(-6 * 256, 18 * 256);
            else if (kind == 2) q.x = (int32_t)(128 * rnd_in(-6, 28)), q.y = (int32_t)(128 * rnd_in(-6, 28));
            else {
                // an extreme, or a coordinate about one radius from the tile: there the last branch of the predicate decides
                const int64_t near_tile = (rnd() & 1 ? -1 : 1) * (DSWX_REACH_MAX_RADIUS + rnd_in(-3000, 3000));
                q.x = (int32_t)(rnd() % 3 == 0 ? near_tile : rnd() % 2 ? rnd_in(-m - 1, m + 1) : (rnd() & 1 ? m : -m));
                q.y = (int32_t)(rnd() % 3 == 0 ? near_tile : rnd() % 2 ? rnd_in(-m - 1, m + 1) : (rnd() & 1 ? m : -m));
            }
            q.word = (uint32_t)rnd();
            q.next = rnd() % 8 ? (uint32_t)rnd_in(0, count - 1) : (uint32_t)rnd();
            tiles[(size_t)t].push_back(q);
        }
        first[(size_t)t + 1] = first[(size_t)t] + count;
    }
    const size_t total = (size_t)first[(size_t)n_tiles], n = (size_t)(H * W);
    const int64_t ms = kind == 3 ? H * W + 5 : 0, ss = kind == 2 ? H * W + 3 : 0;
    const size_t mask_bytes = (size_t)n_tiles * (size_t)(ms ? ms : H * W), src_bytes = (size_t)n_tiles * (size_t)(ss ? ss : H * W);
    Block verts(total * 16, off, 0), table(((size_t)n_tiles + 1) * 8, off, 0), acc((size_t)n_tiles * n * 4, off, 0xA5);
    Block mask(mask_bytes, off, 0xA5), head((size_t)n_tiles * 64, off, 0xA5), src(src_bytes, off, 0);
    size_t at = 0;
    for (auto& tile : tiles)
        for (auto& q : tile) memcpy(verts.p + 16 * at++, &q, 16);
    memcpy(table.p, first.data(), first.size() * 8);
    for (size_t i = 0; i < src_bytes; ++i) src.p[i] = (unsigned char)rnd();
    const bool with_src = kind != 1;
    dswx_reach_spec_t spec = {200, 3, ms, ss, (uint32_t)R, 0};
    dswx_reach_out_t out = {reinterpret_cast<uint32_t*>(acc.p), mask.p, reinterpret_cast<uint64_t*>(head.p)};
    const int rc = dswx_reach_host(reinterpret_cast<const dswx_burn_vertex_t*>(verts.p), reinterpret_cast<const int64_t*>(table.p), &spec, n_tiles, H, W,
                                   with_src ? src.p : nullptr, &out);
    if (rc != DSWX_OK) {
        fprintf(stderr, "case %lld x %lld x %lld kind %d: rc %d %s\n", (long long)n_tiles, (long long)H, (long long)W, kind, rc, g_error);
        return 1;
    }
    int bad = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        uint64_t reached = 0;
        for (int64_t r = 0; r < H; ++r)
            for (int64_t c = 0; c < W; ++c) {
                const uint32_t want = pixel(tiles[(size_t)t], c, r, R);
                uint32_t got;
                memcpy(&got, acc.p + ((size_t)t * n + (size_t)(r * W + c)) * 4, 4);
                const unsigned char mk = mask.p[(size_t)t * (size_t)(ms ? ms : H * W) + (size_t)(r * W + c)];
                const unsigned char other = with_src ? src.p[(size_t)t * (size_t)(ss ? ss : H * W) + (size_t)(r * W + c)] : 3;
                bad += got != want || mk != (want ? 200 : other);
                reached += want != 0;
            }
        uint64_t h[8];
        memcpy(h, head.p + (size_t)t * 64, 64);
        bad += h[0] != tiles[(size_t)t].size() || h[6] != reached || h[7] != 0;
        for (int64_t g = H * W; g < ms; ++g) bad += mask.p[(size_t)t * (size_t)ms + (size_t)g] != 0xA5;      // between the rasters
    }
    if (bad) fprintf(stderr, "case %lld x %lld x %lld kind %d: %d differences\n", (long long)n_tiles, (long long)H, (long long)W, kind, bad);
    return bad != 0;
}

}  // namespace

int main() {
    int cases = 0, failures = 0;
    const int64_t shapes[][3] = {{0, 4, 4}, {1, 1, 1}, {3, 12, 12}, {2, 5, 9}, {4, 1, 12}, {2, 12, 1}, {2, 0, 5}, {2, 5, 0}, {5, 7, 3}};
    for (int round = 0; round < 4; ++round)
        for (const auto& s : shapes)
            for (int kind = 0; kind < 4; ++kind) {
                failures += one_case(s[0], s[1], s[2], kind, (size_t)((cases * 5 + 1) % 8));
                ++cases;
            }
    printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
    return failures ? 1 : 0;
}
