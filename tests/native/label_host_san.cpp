// label_host_san.cpp -- dswx_label_host and dswx_label_rule.h (proteus_amd/csrc/dswx_label.hip) under ASan + UBSan on the CPU:
// the source is compiled INTO this program (tests/test_label.py has the command line), which calls the host entry with the
// plane and every output in heap blocks of exactly the bytes the entry may touch, at odd addresses inside them, and compares
// with a flood fill written here.  No device, no context: the launch half of the source is linked but never called.  Prints
// one JSON line; exit status 0 = every case equal.
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

// `want`: 0 label alone, 1 label + size, 2 all four
int run_case(int64_t T, int64_t H, int64_t W, int conn, uint32_t min_size, unsigned density, int64_t extra, size_t off, int want) {
    dswx_label_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.connectivity = conn;
    spec.replace = 77;
    spec.min_size = min_size;
    spec.member_of_byte[0xA5] = 1;                                    // the padding byte is a MEMBER: reading it would show
    for (int b = 0; b < 256; ++b)
        if (rnd() % 100 < density) spec.member_of_byte[b] = (uint8_t)(1 + rnd() % 255);
    const int64_t n = H * W, stride = n + extra;
    const size_t span = T ? (size_t)((T - 1) * stride + n) : 0;     // the last tile's padding does not exist
    Block plane(span, off, 0xA5);
    for (int64_t t = 0; t < T; ++t)
        for (int64_t i = 0; i < n; ++i) plane.p[t * stride + i] = (uint8_t)rnd();
    const size_t px = (size_t)(T * n);
    Block label(4 * px, 1 + off, 0xEE), size(4 * px, 3, 0xEE), sieved(px, 5, 0xEE), summary(8 * DSWX_LABEL_SUMMARY_WORDS * (size_t)T, 1, 0xEE);
    dswx_label_out_t out;
    std::memset(&out, 0, sizeof out);
    out.label = reinterpret_cast<uint32_t*>(label.p);
    if (want >= 1) out.size = reinterpret_cast<uint32_t*>(size.p);
    if (want >= 2) {
        out.sieved = sieved.p;
        out.summary = reinterpret_cast<uint64_t*>(summary.p);
    }
    const int rc = dswx_label_host(plane.p, &spec, T, H, W, extra ? stride : 0, &out);
    if (rc != DSWX_OK) {
        std::fprintf(stderr, "dswx_label_host failed (%d): %s\n", rc, last_error);
        return 1;
    }
    int bad = 0;
    std::vector<uint32_t> lab((size_t)n), sz((size_t)n);
    std::vector<int64_t> todo;
    for (int64_t t = 0; t < T; ++t) {
        const uint8_t* tile = plane.p + t * stride;
        std::fill(lab.begin(), lab.end(), 0u);
        std::fill(sz.begin(), sz.end(), 0u);
        uint64_t sum[DSWX_LABEL_SUMMARY_WORDS] = {};
        // a flood fill from every member not yet reached, in raster order: the seed is the smallest index of its body
        for (int64_t seed = 0; seed < n; ++seed) {
            if (!spec.member_of_byte[tile[seed]]) continue;
            ++sum[1];
            if (lab[(size_t)seed]) continue;
            std::vector<int64_t> body;
            todo.assign(1, seed);
            lab[(size_t)seed] = (uint32_t)seed + 1u;
            while (!todo.empty()) {
                const int64_t p = todo.back(), y = p / W, x = p % W;
                todo.pop_back();
                body.push_back(p);
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((!dy && !dx) || (conn == 4 && dy && dx)) continue;
                        const int64_t yy = y + dy, xx = x + dx;
                        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                        const int64_t q = yy * W + xx;
                        if (!spec.member_of_byte[tile[q]] || lab[(size_t)q]) continue;
                        lab[(size_t)q] = (uint32_t)seed + 1u;
                        todo.push_back(q);
                    }
            }
            for (int64_t p : body) sz[(size_t)p] = (uint32_t)body.size();
            ++sum[0];
            if (body.size() > sum[2]) {                               // (seeds rise: the first of the largest stays)
                sum[2] = body.size();
                sum[3] = (uint64_t)seed + 1u;
            }
            if (body.size() >= min_size) {
                ++sum[4];
                sum[5] += body.size();
            }
            int b = 0;
            for (size_t s = body.size(); s > 1; s >>= 1) ++b;
            ++sum[8 + b];
        }
        for (int64_t p = 0; p < n; ++p) {
            const size_t i = (size_t)(t * n + p);
            bad += get_u32(label.p, i) != lab[(size_t)p];
            if (want >= 1) bad += get_u32(size.p, i) != sz[(size_t)p];
            if (want >= 2) bad += sieved.p[i] != (lab[(size_t)p] && sz[(size_t)p] < min_size ? 77 : tile[p]);
        }
        if (want >= 2)
            for (int w = 0; w < DSWX_LABEL_SUMMARY_WORDS; ++w) bad += get_u64(summary.p, (size_t)t * DSWX_LABEL_SUMMARY_WORDS + w) != sum[w];
    }
    // the planes that were not wanted
    if (want < 1)
        for (size_t i = 0; i < 4 * px; ++i) bad += size.p[i] != 0xEE;
    if (want < 2) {
        for (size_t i = 0; i < px; ++i) bad += sieved.p[i] != 0xEE;
        for (size_t i = 0; i < 8 * DSWX_LABEL_SUMMARY_WORDS * (size_t)T; ++i) bad += summary.p[i] != 0xEE;
    }
    if (bad) std::fprintf(stderr, "%lld x %lld x %lld, connectivity %d, min_size %u: %d values differ\n", (long long)T, (long long)H,
                          (long long)W, conn, min_size, bad);
    return bad != 0;
}

}  // namespace

int main() {
    int failures = 0, cases = 0;
    const int64_t shapes[][2] = {{1, 1}, {1, 19}, {23, 1}, {2, 15}, {5, 17}, {31, 33}, {33, 129}, {65, 100}};
    const unsigned densities[] = {10, 50, 59, 90, 100};
    for (const auto& s : shapes)
        for (unsigned d : densities)
            for (int64_t T : {0, 1, 3}) {
                failures += run_case(T, s[0], s[1], cases % 2 ? 8 : 4, 1u + (uint32_t)(cases % 5), d, cases % 3 ? 3 : 0, (size_t)(cases % 4), cases % 3);
                ++cases;
            }
    // refusals read and write nothing: NULL or wild buffers would fault if they did
    dswx_label_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.connectivity = 8;
    spec.min_size = 1;
    dswx_label_out_t out;
    std::memset(&out, 0, sizeof out);
    out.label = reinterpret_cast<uint32_t*>(16);
    failures += dswx_label_host(reinterpret_cast<const uint8_t*>(16), &spec, 1, 1 << 16, (1 << 15) + 1, 0, &out) != DSWX_ERR_ARG;
    failures += dswx_label_host(reinterpret_cast<const uint8_t*>(16), &spec, 1, 10, 10, 99, &out) != DSWX_ERR_ARG;
    out.sieved = reinterpret_cast<uint8_t*>(16);
    failures += dswx_label_host(reinterpret_cast<const uint8_t*>(16), &spec, 1, 10, 10, 0, &out) != DSWX_ERR_ARG;      // no size
    out.sieved = nullptr;
    spec.connectivity = 6;
    failures += dswx_label_host(reinterpret_cast<const uint8_t*>(16), &spec, 1, 10, 10, 0, &out) != DSWX_ERR_ARG;
    spec.connectivity = 4;
    failures += dswx_label_host(nullptr, &spec, 0, 10, 10, 0, &out) != DSWX_OK;
    std::printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
    return failures ? 1 : 0;
}
