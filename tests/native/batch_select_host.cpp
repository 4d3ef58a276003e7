// batch_select_host.cpp -- proteus_amd/csrc/dswx_batch_select.h (what a resident-batch entry may be asked for: tile ranges,
// one uint8 plane, plane masks, two batches, base addresses) under ASan + UBSan on the CPU (tests/test_batch_select.py has
// the command line).  The views are made here, their plane addresses are numbers that nothing dereferences; every refusal is
// compared with its status code and its whole text, written out below.  No device, no context.  Prints one JSON line; exit
// status 0 = every case as expected.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dswx_batch_select.h"

static char last_error[512];
int dswx_fail(int code, const char* fmt, ...) {          // (of dswx_hip.hip, which is not part of this program)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
    return code;
}

namespace {

int failures = 0, cases = 0;

// `rc` and the recorded text against what is expected: NULL = DSWX_OK and nothing recorded
void expect(int rc, const char* text, const char* what) {
    ++cases;
    const bool good = text ? rc == DSWX_ERR_ARG && !std::strcmp(last_error, text) : rc == DSWX_OK && !last_error[0];
    if (!good) {
        ++failures;
        std::fprintf(stderr, "%s: rc %d \"%s\", expected \"%s\"\n", what, rc, last_error, text ? text : "(DSWX_OK)");
    }
    last_error[0] = 0;
}
void expect_true(bool good, const char* what) {
    ++cases;
    if (!good) {
        ++failures;
        std::fprintf(stderr, "%s\n", what);
    }
}

const char* const NAMES[DSWX_PLANE_COUNTERS] = {"band[0]", "band[1]", "band[2]", "band[3]", "band[4]", "band[5]", "fmask", "land", "shad",
                                                "ocean", "diag", "wtr1", "wtr1_aerosol", "wtr2", "wtr", "bwtr", "conf", "cloud", "browse"};
const int WIDTH[DSWX_PLANE_COUNTERS] = {2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1};

// a batch without masks and extra layers: no land, shad, ocean, wtr1_aerosol, browse; plane k "at" 0x100000 * (k + 1)
struct Fake {
    void* ptr[DSWX_BATCH_MAX_PLANES];
    dswx_batch_view v;
    Fake(int64_t n_tiles, int64_t h, int64_t w, int64_t stride, int device = 0) : v{n_tiles, h, w, stride, device, ptr} {
        for (int k = 0; k < DSWX_BATCH_MAX_PLANES; ++k) ptr[k] = reinterpret_cast<void*>(uintptr_t(0x100000) * (k + 1));
        for (int k : {DSWX_PLANE_LAND, DSWX_PLANE_SHAD, DSWX_PLANE_OCEAN, DSWX_PLANE_WTR1_AEROSOL, DSWX_PLANE_BROWSE}) ptr[k] = nullptr;
    }
};
uintptr_t at(int k) { return uintptr_t(0x100000) * (k + 1); }

void tile_ranges() {
    char text[256];
    for (int64_t n : {0, 1, 5})
        for (int64_t tile0 : {(int64_t)-1, (int64_t)0, n - 1, n, n + 1})
            for (int64_t asked : {(int64_t)-2, (int64_t)DSWX_BATCH_ALL_TILES, (int64_t)0, (int64_t)1, n - tile0, n - tile0 + 1, INT64_MAX}) {
                Fake f(n, 8, 16, 128);
                // the rule, stated with a sum that cannot overflow here
                int64_t nt = asked;
                if (nt == DSWX_BATCH_ALL_TILES && tile0 >= 0 && tile0 <= n) nt = n - tile0;
                const bool inside = tile0 >= 0 && nt >= 0 && (__int128)tile0 + nt <= n;
                std::snprintf(text, sizeof text, "tiles %lld .. +%lld outside the batch (%lld resident)", (long long)tile0, (long long)nt, (long long)n);
                int64_t got = asked;
                expect(dswx_select_tiles({&f.v}, tile0, &got, "the batch"), inside ? nullptr : text, "tile range");
                expect_true(got == nt, "tile range: the resolved count");
            }
    Fake five(5, 8, 16, 128), three(3, 8, 16, 128);
    int64_t nt = DSWX_BATCH_ALL_TILES;
    expect(dswx_select_tiles({&five.v}, 6, &nt, "the batch"), "tiles 6 .. +-1 outside the batch (5 resident)", "ALL_TILES past the end");
    nt = INT64_MAX;
    expect(dswx_select_tiles({&five.v}, 5, &nt, "the batch"), "tiles 5 .. +9223372036854775807 outside the batch (5 resident)", "INT64_MAX");
    // two views: ALL_TILES is "up to the last of the first", every view is held against the range, the first that fails is named
    nt = DSWX_BATCH_ALL_TILES;
    expect(dswx_select_tiles({&five.v, &three.v}, 0, &nt, "a batch"), "tiles 0 .. +5 outside a batch (3 resident)", "5 and 3, all");
    nt = DSWX_BATCH_ALL_TILES;
    expect(dswx_select_tiles({&three.v, &five.v}, 0, &nt, "a batch"), nullptr, "3 and 5, all");
    expect_true(nt == 3, "3 and 5, all: 3 tiles");
    nt = DSWX_BATCH_ALL_TILES;
    expect(dswx_select_tiles({&five.v, &three.v}, 4, &nt, "a batch"), "tiles 4 .. +1 outside a batch (3 resident)", "5 and 3, from 4");
    nt = DSWX_BATCH_ALL_TILES;
    expect(dswx_select_tiles({&three.v, &five.v}, 4, &nt, "a batch"), "tiles 4 .. +-1 outside a batch (3 resident)", "3 and 5, from 4");
    nt = 2;
    expect(dswx_select_tiles({&five.v, &three.v}, 2, &nt, "a batch"), "tiles 2 .. +2 outside a batch (3 resident)", "5 and 3, 2 .. 3");
    nt = 2;
    expect(dswx_select_tiles({&five.v, &three.v}, 1, &nt, "a batch"), nullptr, "5 and 3, 1 .. 2");
}

void plane_pick() {
    char text[256];
    for (int lowest : {-1, 0})
        for (int64_t tile0 : {0, 3})
            for (int plane = -2; plane <= DSWX_BATCH_MAX_PLANES; ++plane) {
                Fake f(5, 5, 7, 40);
                const uint8_t* base = reinterpret_cast<const uint8_t*>(uintptr_t(1));
                const char* want = text;
                if (plane < lowest || plane >= DSWX_BATCH_MAX_PLANES)
                    std::snprintf(text, sizeof text, "plane %d: not %d .. 19", plane, lowest);
                else if (plane == DSWX_PLANE_COUNTERS)
                    std::snprintf(text, sizeof text, "the counters are not stacked (three int64 per tile): read them (dswx_batch_planes)");
                else if (plane == -1)
                    want = nullptr;
                else if (WIDTH[plane] != 1)
                    std::snprintf(text, sizeof text, "a stack is a uint8 plane, plane %d (%s) has 2 bytes per pixel", plane, NAMES[plane]);
                else if (!f.ptr[plane])
                    std::snprintf(text, sizeof text, "the batch has no plane %d (%s)", plane, NAMES[plane]);
                else
                    want = nullptr;
                expect(dswx_select_u8_plane(f.v, plane, lowest, "the counters are not stacked", "a stack is a uint8 plane", tile0, &base), want, "plane pick");
                if (!want) expect_true(reinterpret_cast<uintptr_t>(base) == (plane < 0 ? 0 : at(plane) + (uintptr_t)tile0 * 40), "plane pick: the address");
            }
    Fake f(5, 5, 7, 40);
    const uint8_t* base = nullptr;
    expect(dswx_select_u8_plane(f.v, -1, 0, "the counters have no distances", "distances are measured in a uint8 plane", 0, &base),
           "plane -1: not 0 .. 19", "-1 where a plane is needed");
    expect(dswx_select_u8_plane(f.v, -2, -1, "the counters are not tabulated", "bodies are tabulated against a uint8 plane", 0, &base),
           "plane -2: not -1 .. 19", "-2 where none is allowed");
    expect(dswx_select_u8_plane(f.v, DSWX_PLANE_COUNTERS, -1, "the counters are not tabulated", "bodies are tabulated against a uint8 plane", 0, &base),
           "the counters are not tabulated (three int64 per tile): read them (dswx_batch_planes)", "the counters");
    expect(dswx_select_u8_plane(f.v, DSWX_PLANE_BAND0, 0, "the counters are not gridded", "a grid is made of a uint8 plane", 0, &base),
           "a grid is made of a uint8 plane, plane 0 (band[0]) has 2 bytes per pixel", "a band");
    expect(dswx_select_u8_plane(f.v, DSWX_PLANE_DIAG, 0, "the counters are not labelled", "bodies are labelled in a uint8 plane", 0, &base),
           "bodies are labelled in a uint8 plane, plane 10 (diag) has 2 bytes per pixel", "DIAG");
    expect(dswx_select_u8_plane(f.v, DSWX_PLANE_LAND, 0, "the counters are not labelled", "bodies are labelled in a uint8 plane", 0, &base),
           "the batch has no plane 7 (land)", "an absent plane");
    // an entry picks the plane before it has looked at the range: any tile0 must do, the address is not used then
    expect(dswx_select_u8_plane(f.v, DSWX_PLANE_WTR, 0, "", "", -1, &base), nullptr, "tile0 -1");
    expect(dswx_select_u8_plane(f.v, DSWX_PLANE_WTR, 0, "", "", INT64_MAX, &base), nullptr, "tile0 INT64_MAX");
}

void mask_walk() {
    char text[256];
    Fake f(5, 5, 7, 40), g(5, 5, 7, 48);
    const char* sentence = "the counters are not histogrammed (three int64 per tile): read them (dswx_batch_planes)";
    uint32_t present = 0;
    for (int k = 0; k < DSWX_BATCH_MAX_PLANES; ++k)
        if (f.ptr[k]) present |= 1u << k;
    expect(dswx_select_mask(0, sentence), nullptr, "mask 0");
    expect(dswx_select_mask(present, nullptr), nullptr, "every present plane and the counters");
    expect(dswx_select_mask(present, sentence), sentence, "the counters refused");
    expect(dswx_select_mask(1u << DSWX_PLANE_COUNTERS, nullptr), nullptr, "the counters allowed");
    expect(dswx_select_mask(present & ~(1u << DSWX_PLANE_COUNTERS), sentence), nullptr, "every present plane");
    expect(dswx_select_mask(1u << DSWX_BATCH_MAX_PLANES, sentence), "plane_mask 0x100000 names planes past 19", "the first bit past the end");
    expect(dswx_select_mask(0x80000000u | present, sentence), "plane_mask 0x800bec7f names planes past 19", "the last bit, before the counters");
    std::vector<int> seen;
    auto note = [&](int k) { seen.push_back(k); };
    expect(dswx_select_walk(0, f.v, nullptr, note), nullptr, "walk of nothing");
    expect_true(seen.empty(), "walk of nothing: no visit");
    for (int k = 0; k < DSWX_BATCH_MAX_PLANES; ++k) {
        seen.clear();
        const char* name = k == DSWX_PLANE_COUNTERS ? "counters" : NAMES[k];
        std::snprintf(text, sizeof text, "the batch has no plane %d (%s)", k, name);
        expect(dswx_select_walk(1u << k, f.v, nullptr, note), f.ptr[k] ? nullptr : text, "walk of one plane");
        expect_true(f.ptr[k] ? seen == std::vector<int>{k} : seen.empty(), "walk of one plane: the visit");
    }
    seen.clear();
    expect(dswx_select_walk(present, f.v, nullptr, note), nullptr, "walk of every present plane");
    expect_true(seen == std::vector<int>({0, 1, 2, 3, 4, 5, 6, 10, 11, 13, 14, 15, 16, 17, 19}), "walk: rising order, the counters last");
    seen.clear();
    expect(dswx_select_walk(present | 1u << DSWX_PLANE_SHAD, f.v, nullptr, note), "the batch has no plane 8 (shad)", "a missing plane among present ones");
    expect_true(seen == std::vector<int>({0, 1, 2, 3, 4, 5, 6}), "walk: the planes before the missing one, none after");
    f.ptr[DSWX_PLANE_COUNTERS] = nullptr;
    expect(dswx_select_walk(1u << DSWX_PLANE_COUNTERS, f.v, nullptr, note), "the batch has no plane 19 (counters)", "no counters");
    // two batches: which of them lacks the plane
    g.ptr[DSWX_PLANE_LAND] = reinterpret_cast<void*>(uintptr_t(64));
    g.ptr[DSWX_PLANE_WTR] = nullptr;
    seen.clear();
    expect(dswx_select_walk(1u << DSWX_PLANE_FMASK | 1u << DSWX_PLANE_LAND, f.v, &g.v, note), "batch a has no plane 7 (land)", "a lacks it");
    expect(dswx_select_walk(1u << DSWX_PLANE_FMASK | 1u << DSWX_PLANE_LAND, g.v, &f.v, note), "batch b has no plane 7 (land)", "b lacks it");
    expect(dswx_select_walk(1u << DSWX_PLANE_FMASK | 1u << DSWX_PLANE_OCEAN, f.v, &g.v, note), "batch a (nor b) has no plane 9 (ocean)", "both lack it");
    expect(dswx_select_walk(1u << DSWX_PLANE_WTR | 1u << DSWX_PLANE_BROWSE, f.v, &g.v, note), "batch b has no plane 14 (wtr)", "the lower plane is named");
    expect_true(seen == std::vector<int>({6, 6, 6}), "two batches: fmask visited each time, nothing else");
    seen.clear();
    expect(dswx_select_walk(1u << DSWX_PLANE_BAND0 | 1u << DSWX_PLANE_CLOUD, f.v, &g.v, note), nullptr, "both have them");
    expect_true(seen == std::vector<int>({0, 17}), "two batches: the visits");
}

void compatible() {
    Fake a(5, 8, 16, 128), other_stride(3, 8, 16, 256), other_device(5, 8, 16, 128, 1), taller(5, 9, 16, 256), wider(5, 8, 17, 256);
    expect(dswx_select_compatible(a.v, a.v), nullptr, "a batch and itself");
    expect(dswx_select_compatible(a.v, other_stride.v), nullptr, "tile counts and strides may differ");
    expect(dswx_select_compatible(a.v, other_device.v), "the batches are on different devices (0 and 1)", "devices");
    expect(dswx_select_compatible(other_device.v, a.v), "the batches are on different devices (1 and 0)", "devices, the other way");
    expect(dswx_select_compatible(a.v, taller.v), "the batches differ in tile size: 8 x 16 against 9 x 16", "height");
    expect(dswx_select_compatible(wider.v, a.v), "the batches differ in tile size: 8 x 17 against 8 x 16", "width");
    other_device.v.height = 9;
    expect(dswx_select_compatible(a.v, other_device.v), "the batches are on different devices (0 and 1)", "the device before the size");
}

void base_address() {
    Fake f(5, 5, 7, 40);
    for (int64_t tile0 : {0, 1, 3}) {
        const uintptr_t t = (uintptr_t)tile0;
        expect_true(reinterpret_cast<uintptr_t>(dswx_select_base(f.v, DSWX_PLANE_BAND0 + 2, tile0)) == at(2) + t * 40 * 2, "a band: 2 bytes per pixel");
        expect_true(reinterpret_cast<uintptr_t>(dswx_select_base(f.v, DSWX_PLANE_DIAG, tile0)) == at(10) + t * 40 * 2, "DIAG: 2 bytes per pixel");
        expect_true(reinterpret_cast<uintptr_t>(dswx_select_base(f.v, DSWX_PLANE_CONF, tile0)) == at(16) + t * 40, "a layer: 1 byte per pixel");
        expect_true(reinterpret_cast<uintptr_t>(dswx_select_base(f.v, DSWX_PLANE_FMASK, tile0)) == at(6) + t * 40, "fmask: 1 byte per pixel");
        expect_true(reinterpret_cast<uintptr_t>(dswx_select_base(f.v, DSWX_PLANE_COUNTERS, tile0)) == at(19) + t * 24, "the counters: 3 x int64 per tile");
    }
    Fake far(int64_t(1) << 32, 3660, 3660, 13395712);       // tile offsets past 2^32 bytes
    expect_true(reinterpret_cast<uintptr_t>(dswx_select_base(far.v, DSWX_PLANE_BAND0, (int64_t(1) << 32) - 1)) ==
                    at(0) + uintptr_t(0xFFFFFFFFu) * 13395712u * 2u, "a band of the last of 2^32 tiles");
}

}  // namespace

int main() {
    tile_ranges();
    plane_pick();
    mask_walk();
    compatible();
    base_address();
    std::printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
    return failures ? 1 : 0;
}
