// grid_host_san.cpp -- dswx_grid_host and dswx_grid_rule.h (proteus_amd/csrc/dswx_grid.hip) under ASan + UBSan on the CPU: the
// source is compiled INTO this program (tests/test_grid.py has the command line), which calls the host entry on ragged grids
// with the plane and every output in heap blocks of exactly the bytes the entry may touch, at odd addresses inside them, and
// compares with a loop over the pixels written here.  No device, no context: the launch half of the source is linked but
// never called.  Prints one JSON line; exit status 0 = every case equal.
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

uint32_t rng_state = 20251019u;
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

int run_case(int64_t T, int64_t H, int64_t W, int cell_h, int cell_w, int n_cats, int64_t extra, size_t off) {
    dswx_grid_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.n_cats = n_cats;
    spec.cell_h = cell_h;
    spec.cell_w = cell_w;
    for (int b = 0; b < 256; ++b) spec.cat_of_byte[b] = (uint8_t)(rnd() % 6);
    const int64_t n = H * W, stride = n + extra;
    const size_t span = T ? (size_t)((T - 1) * stride + n) : 0;     // the last tile's padding does not exist
    Block plane(span, off, 0xA5);
    for (int64_t t = 0; t < T; ++t)
        for (int64_t i = 0; i < n; ++i) plane.p[t * stride + i] = (uint8_t)rnd();
    const int64_t ch = cell_h < H ? cell_h : H, cw = cell_w < W ? cell_w : W;
    const int64_t gh = n ? (H + ch - 1) / ch : 0, gw = n ? (W + cw - 1) / cw : 0;
    const size_t cells = (size_t)(T * gh * gw);
    Block c0(4 * cells, 1, 0xEE), c1(4 * cells, 3, 0xEE), c2(4 * cells, 2, 0xEE), c3(4 * cells, 4, 0xEE);
    Block share(cells, 1, 0xEE), coverage(cells, 0, 0xEE), major(cells, 5, 0xEE);
    Block* counts[4] = {&c0, &c1, &c2, &c3};
    dswx_grid_out_t out;
    std::memset(&out, 0, sizeof out);
    for (int k = 0; k < n_cats; ++k) out.count[k] = reinterpret_cast<uint32_t*>(counts[k]->p);
    out.share = share.p;
    out.coverage = coverage.p;
    out.major = major.p;
    const int rc = dswx_grid_host(plane.p, &spec, T, H, W, extra ? stride : 0, &out);
    if (rc != DSWX_OK) {
        std::fprintf(stderr, "dswx_grid_host failed (%d): %s\n", rc, last_error);
        return 1;
    }
    int bad = 0;
    for (int64_t t = 0; t < T; ++t)
        for (int64_t gy = 0; gy < gh; ++gy)
            for (int64_t gx = 0; gx < gw; ++gx) {
                const int64_t r1 = (gy + 1) * ch < H ? (gy + 1) * ch : H, q1 = (gx + 1) * cw < W ? (gx + 1) * cw : W;
                uint32_t cnt[4] = {0, 0, 0, 0};
                for (int64_t r = gy * ch; r < r1; ++r)
                    for (int64_t q = gx * cw; q < q1; ++q) {
                        const unsigned c = spec.cat_of_byte[plane.p[t * stride + r * W + q]];
                        if (c < (unsigned)n_cats) ++cnt[c];
                    }
                const uint32_t n_obs = cnt[0] + cnt[1] + cnt[2] + cnt[3];
                const uint32_t n_pix = (uint32_t)((r1 - gy * ch) * (q1 - gx * cw));
                unsigned best = 0;
                for (unsigned k = 1; k < 4; ++k)
                    if (cnt[k] > cnt[best]) best = k;
                const size_t i = (size_t)((t * gh + gy) * gw + gx);
                for (int k = 0; k < n_cats; ++k) bad += get_u32(counts[k]->p, i) != cnt[k];
                bad += share.p[i] != (n_obs ? 100u * cnt[0] / n_obs : 255u);
                bad += coverage.p[i] != 100u * n_obs / n_pix;
                bad += major.p[i] != (n_obs ? best : 255u);
            }
    for (int k = n_cats; k < 4; ++k)                                  // the planes that were not wanted
        for (size_t i = 0; i < 4 * cells; ++i) bad += counts[k]->p[i] != 0xEE;
    if (bad) std::fprintf(stderr, "%lld x %lld x %lld, cells %d x %d, %d categories: %d values differ\n", (long long)T, (long long)H,
                          (long long)W, cell_h, cell_w, n_cats, bad);
    return bad != 0;
}

}  // namespace

int main() {
    int failures = 0, cases = 0;
    const int64_t shapes[][2] = {{1, 1}, {2, 15}, {5, 17}, {31, 33}, {65, 100}, {7, 1}};
    const int cells[][2] = {{1, 1}, {3, 7}, {30, 30}, {2, 16}, {4, 17}, {1000, 1000}, {66, 5}};
    for (const auto& s : shapes)
        for (const auto& c : cells)
            for (int64_t T : {0, 1, 3}) {
                failures += run_case(T, s[0], s[1], c[0], c[1], 1 + cases % 4, cases % 2 ? 3 : 0, (size_t)(cases % 3));
                ++cases;
            }
    // refusals read and write nothing: NULL buffers would fault if they did
    dswx_grid_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.n_cats = 2;
    spec.cell_h = spec.cell_w = 5000;
    dswx_grid_out_t out;
    std::memset(&out, 0, sizeof out);
    out.share = reinterpret_cast<uint8_t*>(16);
    failures += dswx_grid_host(reinterpret_cast<const uint8_t*>(16), &spec, 1, 5000, 5000, 0, &out) != DSWX_ERR_ARG;
    failures += dswx_grid_host(reinterpret_cast<const uint8_t*>(16), &spec, 1, 10, 10, 99, &out) != DSWX_ERR_ARG;
    failures += dswx_grid_host(nullptr, &spec, 0, 10, 10, 0, &out) != DSWX_OK;
    std::printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
    return failures ? 1 : 0;
}
