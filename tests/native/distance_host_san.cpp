// distance_host_san.cpp -- dswx_distance_host and dswx_distance_rule.h (proteus_amd/csrc/dswx_distance.hip) under ASan + UBSan
// on the CPU: the source is compiled INTO this program (tests/test_distance.py has the command line), which calls the host
// entry with the plane and every output in heap blocks of exactly the bytes the entry may touch, at odd addresses inside
// them, and compares with a loop over all pairs of a pixel and a target written here.  No device, no context: the launch half
// of the source is linked but never called.  Prints one JSON line; exit status 0 = every case equal.
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

uint32_t rng_state = 20261019u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// a heap block of exactly n + off bytes; the payload starts `off` bytes in, so one byte past it is outside the block
struct Block {
    uint8_t* mem;
    uint8_t* p;
    Block(size_t n, size_t off, int fill) : mem(static_cast<uint8_t*>(std::malloc(n + off ? n + off : 1))), p(mem + off) {
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
uint64_t get_u64(const uint8_t* p, size_t i) {
    uint64_t v;
    std::memcpy(&v, p + 8 * i, 8);
    return v;
}

// `want`: 0 dist2 alone, 1 dist2 + nearest, 2 all four (within only with a radius), 3 dist2 + summary.  `per_mille`: targets.
int run_case(int64_t T, int64_t H, int64_t W, uint32_t R, unsigned per_mille, int64_t extra, size_t off, int want) {
    dswx_distance_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.max_radius = R;
    spec.mark = 77;
    spec.target_of_byte[0xA5] = 1;                                    // the padding byte is a TARGET: reading it would show
    spec.target_of_byte[1] = 9;
    spec.target_of_byte[255] = 255;
    const int64_t n = H * W, stride = n + extra;
    const size_t span = T ? (size_t)((T - 1) * stride + n) : 0;     // the last tile's padding does not exist
    Block plane(span, off, 0xA5);
    for (int64_t t = 0; t < T; ++t)
        for (int64_t i = 0; i < n; ++i) plane.p[t * stride + i] = rnd() % 1000 < per_mille ? (rnd() % 2 ? 1 : 255) : (uint8_t)(2 + rnd() % 100);
    const size_t px = (size_t)(T * n);
    const bool w_near = want == 1 || want == 2, w_within = want == 2 && R, w_sum = want >= 2;
    Block dist2(4 * px, 1 + off, 0xEE), nearest(4 * px, 3, 0xEE), within(px, 5, 0xEE), summary(8 * DSWX_DISTANCE_SUMMARY_WORDS * (size_t)T, 1, 0xEE);
    dswx_distance_out_t out;
    std::memset(&out, 0, sizeof out);
    out.dist2 = reinterpret_cast<uint32_t*>(dist2.p);
    if (w_near) out.nearest = reinterpret_cast<uint32_t*>(nearest.p);
    if (w_within) out.within = within.p;
    if (w_sum) out.summary = reinterpret_cast<uint64_t*>(summary.p);
    const int rc = dswx_distance_host(plane.p, &spec, T, H, W, extra ? stride : 0, &out);
    if (rc != DSWX_OK) {
        std::fprintf(stderr, "dswx_distance_host failed (%d): %s\n", rc, last_error);
        return 1;
    }
    int bad = 0;
    std::vector<int64_t> targets;
    for (int64_t t = 0; t < T; ++t) {
        const uint8_t* tile = plane.p + t * stride;
        targets.clear();
        for (int64_t p = 0; p < n; ++p)
            if (spec.target_of_byte[tile[p]]) targets.push_back(p);
        uint64_t sum[DSWX_DISTANCE_SUMMARY_WORDS] = {};
        bool any = false;
        for (int64_t p = 0; p < n; ++p) {
            const int64_t y = p / W, x = p % W;
            uint64_t best = UINT64_MAX;
            int64_t best_q = -1;
            for (int64_t q : targets) {                                   // the smallest (d2, column, row) within the radius
                const int64_t qy = q / W, qx = q % W, d = (y - qy) * (y - qy) + (x - qx) * (x - qx);
                if (R && d > (int64_t)R * R) continue;
                const uint64_t key = ((uint64_t)d << 40) | ((uint64_t)qx << 20) | (uint64_t)qy;
                if (key < best) best = key, best_q = q;
            }
            const uint32_t d2 = best_q < 0 ? DSWX_DISTANCE_NONE : (uint32_t)(best >> 40);
            const size_t i = (size_t)(t * n + p);
            bad += get_u32(dist2.p, i) != d2;
            if (w_near) bad += get_u32(nearest.p, i) != (best_q < 0 ? DSWX_DISTANCE_NONE : (uint32_t)best_q);
            if (w_within) bad += within.p[i] != (best_q >= 0 && d2 ? 77 : tile[p]);
            if (best_q < 0) {
                ++sum[2];
                continue;
            }
            ++sum[d2 ? 1 : 0];
            sum[5] += d2;
            if (!any || d2 > sum[3]) sum[3] = d2, sum[4] = (uint64_t)p, any = true;      // (indices rise: the first of the largest stays)
            if (d2) {
                int b = 0;
                for (uint32_t s = d2; s > 1; s >>= 1) ++b;
                ++sum[8 + b];
            }
        }
        if (w_sum)
            for (int w = 0; w < DSWX_DISTANCE_SUMMARY_WORDS; ++w) bad += get_u64(summary.p, (size_t)t * DSWX_DISTANCE_SUMMARY_WORDS + w) != sum[w];
    }
    // the planes that were not wanted
    if (!w_near)
        for (size_t i = 0; i < 4 * px; ++i) bad += nearest.p[i] != 0xEE;
    if (!w_within)
        for (size_t i = 0; i < px; ++i) bad += within.p[i] != 0xEE;
    if (!w_sum)
        for (size_t i = 0; i < 8 * DSWX_DISTANCE_SUMMARY_WORDS * (size_t)T; ++i) bad += summary.p[i] != 0xEE;
    if (bad) std::fprintf(stderr, "%lld x %lld x %lld, radius %u, %u per mille: %d values differ\n", (long long)T, (long long)H, (long long)W, R,
                          per_mille, bad);
    return bad != 0;
}

}  // namespace

int main() {
    int failures = 0, cases = 0;
    const int64_t shapes[][2] = {{1, 1}, {1, 19}, {23, 1}, {2, 15}, {5, 17}, {31, 33}, {33, 70}, {65, 40}};
    const unsigned per_mille[] = {0, 2, 50, 500, 1000};
    const uint32_t radii[] = {0, 1, 3, 100};
    for (const auto& s : shapes)
        for (unsigned d : per_mille)
            for (int64_t T : {0, 1, 3}) {
                failures += run_case(T, s[0], s[1], radii[cases % 4], d, cases % 3 ? 3 : 0, (size_t)(cases % 4), (cases / 4) % 4);
                ++cases;
            }
    // refusals read and write nothing: NULL or wild buffers would fault if they did
    dswx_distance_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    dswx_distance_out_t out;
    std::memset(&out, 0, sizeof out);
    out.dist2 = reinterpret_cast<uint32_t*>(16);
    const uint8_t* wild = reinterpret_cast<const uint8_t*>(16);
    failures += dswx_distance_host(wild, &spec, 1, 46341, 1, 0, &out) != DSWX_ERR_ARG;
    failures += dswx_distance_host(wild, &spec, 1, 1, DSWX_DISTANCE_MAX_WIDTH + 1, 0, &out) != DSWX_ERR_ARG;
    failures += dswx_distance_host(wild, &spec, 1, 10, 10, 99, &out) != DSWX_ERR_ARG;
    out.within = reinterpret_cast<uint8_t*>(16);
    failures += dswx_distance_host(wild, &spec, 1, 10, 10, 0, &out) != DSWX_ERR_ARG;                 // within without a radius
    out.within = nullptr;
    spec.mark = 256;
    failures += dswx_distance_host(wild, &spec, 1, 10, 10, 0, &out) != DSWX_ERR_ARG;
    spec.mark = 0;
    out.dist2 = nullptr;
    failures += dswx_distance_host(wild, &spec, 1, 10, 10, 0, &out) != DSWX_ERR_ARG;
    out.dist2 = reinterpret_cast<uint32_t*>(16);
    failures += dswx_distance_host(nullptr, &spec, 0, 10, 10, 0, &out) != DSWX_OK;
    std::printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
    return failures ? 1 : 0;
}
