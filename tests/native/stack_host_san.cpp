// stack_host_san.cpp -- dswx_stack_host and dswx_mosaic_host with what they share (proteus_amd/csrc/dswx_stack.hip,
// dswx_mosaic.hip, dswx_stack_core.h, dswx_stack_rule.h) under ASan + UBSan on the CPU: both sources are compiled INTO this
// program (tests/test_stack.py has the command line), which calls the host entries with every plane, table and output in heap
// blocks of exactly the bytes the entry may touch, at odd addresses inside them, and compares with a composite per pixel
// written here.  No device, no context: the launch halves of the sources are linked but never called.  Prints one JSON line;
// exit status 0 = every case equal.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

uint32_t rng_state = 20261021u;
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

uint16_t get_u16(const uint8_t* p, size_t i) {
    uint16_t v;
    std::memcpy(&v, p + 2 * i, 2);
    return v;
}

// The outputs of one call, every plane of `elems` elements in a block of its own; `want` bit 0: the counts below n_cats,
// 1: last, 2: last_index, 3: share.  The uint16 planes sit at odd addresses.
struct Outputs {
    Block c0, c1, c2, c3, last, index, share;
    Block* counts[4];
    dswx_stack_out_t out;
    int n_cats, want;
    Outputs(size_t elems, int n_cats_, int want_)
        : c0(2 * elems, 1, 0xEE), c1(2 * elems, 3, 0xEE), c2(2 * elems, 5, 0xEE), c3(2 * elems, 7, 0xEE), last(elems, 1, 0xEE),
          index(2 * elems, 3, 0xEE), share(elems, 2, 0xEE), counts{&c0, &c1, &c2, &c3}, n_cats(n_cats_), want(want_) {
        std::memset(&out, 0, sizeof out);
        if (want & 1)
            for (int k = 0; k < n_cats; ++k) out.count[k] = reinterpret_cast<uint16_t*>(counts[k]->p);
        if (want & 2) out.last = last.p;
        if (want & 4) out.last_index = reinterpret_cast<uint16_t*>(index.p);
        if (want & 8) out.share = share.p;
    }
    // pixel i against the composite of its observations: cnt[4], the latest byte and tile (or what stands for none)
    int differs(size_t i, const unsigned* cnt, unsigned last_byte, unsigned last_tile) const {
        int bad = 0;
        const unsigned n_obs = cnt[0] + cnt[1] + cnt[2] + cnt[3];
        if (want & 1)
            for (int k = 0; k < n_cats; ++k) bad += get_u16(counts[k]->p, i) != cnt[k];
        if (want & 2) bad += last.p[i] != last_byte;
        if (want & 4) bad += get_u16(index.p, i) != last_tile;
        if (want & 8) bad += share.p[i] != (n_obs ? 100u * cnt[0] / n_obs : (unsigned)DSWX_STACK_NO_SHARE);
        return bad;
    }
    // the planes that were not wanted are as they were
    int untouched(size_t elems) const {
        int bad = 0;
        for (int k = (want & 1) ? n_cats : 0; k < 4; ++k)
            for (size_t i = 0; i < 2 * elems; ++i) bad += counts[k]->p[i] != 0xEE;
        for (size_t i = 0; i < elems && !(want & 2); ++i) bad += last.p[i] != 0xEE;
        for (size_t i = 0; i < 2 * elems && !(want & 4); ++i) bad += index.p[i] != 0xEE;
        for (size_t i = 0; i < elems && !(want & 8); ++i) bad += share.p[i] != 0xEE;
        return bad;
    }
};

// cat_of_byte of a case: `every` = all 256 bytes are observations
void fill_cats(uint8_t* cat_of_byte, int n_cats, bool every) {
    for (int b = 0; b < 256; ++b) cat_of_byte[b] = (uint8_t)(every ? rnd() % (unsigned)n_cats : rnd() % 6);
}

int stack_case(int64_t T, int64_t n, int64_t extra, int n_cats, int want, size_t off) {
    dswx_stack_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.n_cats = n_cats;
    spec.fill = (int)(rnd() & 255u);
    fill_cats(spec.cat_of_byte, n_cats, false);
    const int64_t stride = n + extra;
    const size_t span = T && n ? (size_t)((T - 1) * stride + n) : 0;      // the last tile's padding does not exist
    Block stack(span, off, 0xA5);
    for (int64_t t = 0; t < T; ++t)
        for (int64_t i = 0; i < n; ++i) stack.p[t * stride + i] = (uint8_t)rnd();
    Outputs o((size_t)n, n_cats, want);
    const int rc = dswx_stack_host(stack.p, &spec, T, n, extra ? stride : 0, &o.out);
    if (rc != DSWX_OK) {
        std::fprintf(stderr, "dswx_stack_host failed (%d): %s\n", rc, last_error);
        return 1;
    }
    int bad = o.untouched((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        unsigned cnt[4] = {0, 0, 0, 0}, last_byte = (unsigned)spec.fill, last_tile = DSWX_STACK_NONE;
        for (int64_t t = 0; t < T; ++t) {
            const unsigned byte = stack.p[t * stride + i], c = spec.cat_of_byte[byte];
            if (c >= (unsigned)n_cats) continue;
            ++cnt[c];
            last_byte = byte;
            last_tile = (unsigned)t;
        }
        bad += o.differs((size_t)i, cnt, last_byte, last_tile);
    }
    if (bad) std::fprintf(stderr, "stack %lld tiles x %lld elements + %lld, %d categories, outputs %d: %d values differ\n", (long long)T,
                          (long long)n, (long long)extra, n_cats, want, bad);
    return bad != 0;
}

int mosaic_case(int64_t T, int64_t H, int64_t W, int64_t extra, const int32_t (*place)[2], int64_t CH, int64_t CW, int n_cats,
                bool every, int want, size_t off) {
    dswx_mosaic_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.n_cats = n_cats;
    spec.fill = (int)(rnd() & 255u);
    spec.outside = (int)(rnd() & 255u);
    fill_cats(spec.cat_of_byte, n_cats, every);
    const int64_t n = H * W, stride = n + extra;
    const size_t span = T && n ? (size_t)((T - 1) * stride + n) : 0;
    Block plane(span, off, 0xA5), table((size_t)T * 8, 1 + 2 * off, 0xA5);
    for (int64_t t = 0; t < T; ++t) {
        for (int64_t i = 0; i < n; ++i) plane.p[t * stride + i] = (uint8_t)rnd();
        std::memcpy(table.p + 8 * t, place[t], 8);
    }
    Outputs o((size_t)(CH * CW), n_cats, want);
    const int rc = dswx_mosaic_host(plane.p, &spec, T, H, W, extra ? stride : 0, reinterpret_cast<const int32_t*>(table.p), CH, CW, &o.out);
    if (rc != DSWX_OK) {
        std::fprintf(stderr, "dswx_mosaic_host failed (%d): %s\n", rc, last_error);
        return 1;
    }
    int bad = o.untouched((size_t)(CH * CW));
    for (int64_t Y = 0; Y < CH; ++Y)
        for (int64_t X = 0; X < CW; ++X) {
            unsigned cnt[4] = {0, 0, 0, 0}, last_byte = (unsigned)spec.outside, last_tile = DSWX_STACK_NONE;
            for (int64_t t = 0; t < T; ++t) {
                const int64_t r = Y - (int64_t)place[t][0], q = X - (int64_t)place[t][1];
                if (r < 0 || r >= H || q < 0 || q >= W) continue;
                if (last_tile == DSWX_STACK_NONE) last_byte = (unsigned)spec.fill;      // covered: not `outside` any more
                const unsigned byte = plane.p[t * stride + r * W + q], c = spec.cat_of_byte[byte];
                if (c >= (unsigned)n_cats) continue;
                ++cnt[c];
                last_byte = byte;
                last_tile = (unsigned)t;
            }
            bad += o.differs((size_t)(Y * CW + X), cnt, last_byte, last_tile);
        }
    if (bad) std::fprintf(stderr, "mosaic %lld tiles of %lld x %lld + %lld at (%d, %d) .., %d categories, outputs %d: %d values differ\n",
                          (long long)T, (long long)H, (long long)W, (long long)extra, T ? place[0][0] : 0, T ? place[0][1] : 0, n_cats, want, bad);
    return bad != 0;
}

bool refused(int rc, int code, const char* text) { return rc == code && std::strstr(last_error, text) != nullptr; }

}  // namespace

int main() {
    int failures = 0, cases = 0;
    const int wants[] = {15, 1, 2, 4, 8, 9, 6};
    for (int64_t T : {0, 1, 9})
        for (int64_t n : {0, 15, 16, 33})
            for (int64_t extra : {0, 3})
                for (int rep = 0; rep < 2; ++rep) {
                    failures += stack_case(T, n, extra, 1 + cases % 4, wants[cases % 7], (size_t)(cases % 3));
                    ++cases;
                }
    // three tiles on a 7 x 20 canvas: inside, over every edge and corner, coinciding, wholly outside, at the ends of int32
    const int32_t lo = INT32_MIN, hi = INT32_MAX;
    const int32_t places[][3][2] = {
        {{0, 0}, {2, 3}, {6, 19}},     {{-1, -2}, {-2, 17}, {5, -4}}, {{-2, 5}, {6, 5}, {2, -4}}, {{2, 19}, {1, 1}, {1, 2}},
        {{3, 8}, {3, 8}, {3, 8}},      {{lo, 0}, {0, hi}, {hi, lo}},  {{lo, lo}, {4, 16}, {hi, hi}}, {{0, lo}, {lo, 7}, {6, 0}},
        {{-3, 0}, {7, 0}, {0, 20}},    {{0, -5}, {-2, -4}, {6, 15}},
    };
    const int64_t tiles[][2] = {{3, 5}, {1, 1}};
    for (const auto& p : places)
        for (const auto& hw : tiles)
            for (int64_t extra : {0, 3})
                for (int every = 0; every < 2; ++every) {
                    failures += mosaic_case(3, hw[0], hw[1], extra, p, 7, 20, 1 + cases % 4, every != 0, wants[cases % 7], (size_t)(cases % 3));
                    ++cases;
                }
    // no tiles: the outside values; an empty tile raster covers nothing; an empty canvas writes nothing
    failures += mosaic_case(0, 3, 5, 0, places[0], 7, 20, 2, false, 15, 1);
    failures += mosaic_case(3, 0, 5, 0, places[0], 7, 20, 2, false, 15, 0);
    failures += mosaic_case(3, 3, 5, 0, places[0], 0, 20, 2, false, 15, 2);
    cases += 3;
    // refusals read and write nothing: the buffers do not exist
    dswx_stack_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.n_cats = 2;
    dswx_mosaic_spec_t mspec;
    std::memset(&mspec, 0, sizeof mspec);
    mspec.n_cats = 2;
    dswx_stack_out_t out;
    std::memset(&out, 0, sizeof out);
    const uint8_t* const nowhere = reinterpret_cast<const uint8_t*>(16);
    const int32_t* const no_table = reinterpret_cast<const int32_t*>(16);
    failures += !refused(dswx_stack_host(nowhere, &spec, 2, 10, 0, &out), DSWX_ERR_ARG, "every output is NULL");
    failures += !refused(dswx_mosaic_host(nowhere, &mspec, 2, 2, 5, 0, no_table, 7, 20, &out), DSWX_ERR_ARG, "every output is NULL");
    out.count[2] = reinterpret_cast<uint16_t*>(16);
    failures += !refused(dswx_stack_host(nowhere, &spec, 2, 10, 0, &out), DSWX_ERR_ARG, "count[2] is not NULL but n_cats is 2");
    failures += !refused(dswx_mosaic_host(nowhere, &mspec, 2, 2, 5, 0, no_table, 7, 20, &out), DSWX_ERR_ARG, "count[2] is not NULL but n_cats is 2");
    out.count[2] = nullptr;
    out.share = reinterpret_cast<uint8_t*>(16);
    failures += !refused(dswx_stack_host(nowhere, &spec, 2, 10, 9, &out), DSWX_ERR_ARG, "tile_stride smaller than the tile");
    failures += !refused(dswx_mosaic_host(nowhere, &mspec, 2, 2, 5, 9, no_table, 7, 20, &out), DSWX_ERR_ARG, "tile_stride smaller than the tile");
    failures += !refused(dswx_stack_host(nowhere, &spec, 65536, 10, 0, &out), DSWX_ERR_ARG, "above DSWX_STACK_MAX_TILES");
    failures += !refused(dswx_mosaic_host(nowhere, &mspec, 65536, 2, 5, 0, no_table, 7, 20, &out), DSWX_ERR_ARG, "above DSWX_STACK_MAX_TILES");
    failures += !refused(dswx_stack_host(nullptr, &spec, 2, 10, 0, &out), DSWX_ERR_ARG, "stack is NULL");
    failures += !refused(dswx_mosaic_host(nullptr, &mspec, 2, 2, 5, 0, no_table, 7, 20, &out), DSWX_ERR_ARG, "plane is NULL");
    spec.fill = mspec.fill = 256;
    failures += !refused(dswx_stack_host(nowhere, &spec, 2, 10, 0, &out), DSWX_ERR_ARG, "fill 256 outside 0 .. 255");
    failures += !refused(dswx_mosaic_host(nowhere, &mspec, 2, 2, 5, 0, no_table, 7, 20, &out), DSWX_ERR_ARG, "fill 256 outside 0 .. 255");
    cases += 12;
    std::printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
    return failures ? 1 : 0;
}
