// land_mesh_host_san.cpp -- the LAND rule read through two meshes (proteus_amd/csrc/dswx_land_mesh_rule.h) and its host entry
// dswx_land_mesh_host (dswx_land_mesh.hip, compiled into this program with dswx_warp.hip for the shared geometry checks), under
// ASan + UBSan on the HOST: garbage meshes with INT32 extremes over tiny rasters, on heap blocks of exactly the bytes the entry
// may touch, at odd addresses, against a plain loop written here with positions in 128-bit integers.  No device is used: the
// kernels of the translation units are compiled and never launched.  tests/test_land_mesh.py builds and runs it as a child
// process; the last line of standard output is a JSON record.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dswx_hip.h"
#include "dswx_land_mesh_rule.h"

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

const int32_t SPECIAL[5] = {INT32_MIN, INT32_MAX, 0, 1, -1};
int32_t any_node() { return rnd() % 4 == 0 ? SPECIAL[rnd() % 5] : (rnd() % 2 ? (int32_t)rnd() : (int32_t)rnd_in(-3000, 3000)); }

// A heap block of exactly `bytes` bytes whose payload begins `off` bytes in: ASan sees the first byte past either end.
struct Block {
    std::vector<unsigned char>* raw;
    unsigned char* p;
    Block(size_t bytes, size_t off, int fill) : raw(new std::vector<unsigned char>(bytes + off, (unsigned char)fill)), p(raw->data() + off) {}
    ~Block() { delete raw; }
};

__int128 floor_div(__int128 a, __int128 b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }      // b > 0
int64_t wide_coord(const int32_t v[4], int64_t fx, int64_t fy, int s) {
    if (s == 0) return v[0];
    const __int128 step = (__int128)1 << s;
    const __int128 num = (step - fy) * ((step - fx) * v[0] + fx * v[1]) + fy * ((step - fx) * v[2] + fx * v[3]);
    return (int64_t)floor_div(num + ((__int128)1 << (2 * s - 1)), (__int128)1 << (2 * s));
}
// the nearest source pixel of destination pixel (X, Y) from `mesh` = int32 [mesh_h][mesh_w][2] at any address
void wide_pixel(const unsigned char* mesh, int64_t mesh_w, int s, int64_t X, int64_t Y, int64_t* c, int64_t* r) {
    const int64_t step = (int64_t)1 << s, i = Y >> s, j = X >> s;
    int32_t v[2][4];
    for (int q = 0; q < 4; ++q)
        for (int k = 0; k < 2; ++k) memcpy(&v[k][q], mesh + 4 * (2 * ((i + (q >> 1)) * mesh_w + j + (q & 1)) + k), 4);
    *c = (int64_t)floor_div(wide_coord(v[0], X & (step - 1), Y & (step - 1), s), 256);
    *r = (int64_t)floor_div(wide_coord(v[1], X & (step - 1), Y & (step - 1), s), 256);
}

struct Shape {
    int64_t n, H, W, wc_h, wc_w, cg_h, cg_w;
    int s_wc, s_cg;
};

// A mesh of a dh x dw lattice: a gentle affine map of `scale` / 256 source pixels per pixel that leaves part of the lattice
// outside the raster, with some nodes replaced by arbitrary values.  Exactly the ints that the entry may read.
struct Mesh {
    int64_t mesh_h, mesh_w, stride;
    Block b;
    Mesh(int64_t n, int64_t dh, int64_t dw, int s, int scale, bool per_tile, size_t off)
        : mesh_h(mesh_dims(dh, s)), mesh_w(mesh_dims(dw, s)), stride(per_tile ? mesh_h * mesh_w + 3 : 0),
          b(n > 0 ? (size_t)(((per_tile ? n - 1 : 0) * stride + mesh_h * mesh_w) * 8) : 0, off, 0x5A) {
        if (n <= 0) return;
        const int64_t step = (int64_t)1 << s;
        for (int64_t t = 0; t < (per_tile ? n : 1); ++t)
            for (int64_t i = 0; i < mesh_h; ++i)
                for (int64_t j = 0; j < mesh_w; ++j) {
                    int32_t xy[2] = {(int32_t)(scale * j * step + scale / 9 * i * step - 300 + 40 * t + rnd_in(-64, 64)),
                                     (int32_t)(scale * i * step - scale / 12 * j * step - 200 + rnd_in(-64, 64))};
                    if (rnd() % 8 == 0) xy[rnd() % 2] = any_node();
                    memcpy(b.p + (size_t)((t * stride + i * mesh_w + j) * 8), xy, 8);
                }
    }
    const unsigned char* tile(int64_t t) const { return b.p + (size_t)(t * stride * 8); }
};

size_t plane_bytes(int64_t n, int64_t h, int64_t w, int64_t stride) { return n > 0 ? (size_t)((n - 1) * (stride ? stride : h * w) + h * w) : 0; }

int land_case(const Shape& g, int variant, size_t off) {
    const bool per_tile = (variant & 1) != 0, padded = (variant & 2) != 0, wild = (variant & 4) != 0;
    const Mesh m_wc(g.n, 3 * g.H, 3 * g.W, g.s_wc, 100, per_tile, off), m_cg(g.n, g.H, g.W, g.s_cg, 90, per_tile, off);
    const int64_t wc_stride = padded ? g.wc_h * g.wc_w + 5 : 0, cg_stride = padded ? g.cg_h * g.cg_w + 3 : 0;
    const int64_t land_stride = padded ? g.H * g.W + 7 : 0, ls = land_stride ? land_stride : g.H * g.W;
    const size_t px = (size_t)(g.H * g.W);
    Block wc(plane_bytes(g.n, g.wc_h, g.wc_w, wc_stride), off, 0), cg(plane_bytes(g.n, g.cg_h, g.cg_w, cg_stride), off, 0);
    Block land(plane_bytes(g.n, g.H, g.W, land_stride), off, 0xA5), head((size_t)(g.n > 0 ? g.n : 0) * 64, off, 0xA5);
    const unsigned char wc_codes[8] = {10, 50, 80, 90, 95, 0, 30, 255}, cg_codes[6] = {111, 113, 20, 0, 255, 200};
    for (size_t i = 0; i < plane_bytes(g.n, g.wc_h, g.wc_w, wc_stride); ++i) wc.p[i] = wc_codes[rnd() % 8];
    for (size_t i = 0; i < plane_bytes(g.n, g.cg_h, g.cg_w, cg_stride); ++i) cg.p[i] = cg_codes[rnd() % 6];
    const int32_t forest[5] = {111, 200, -7, 256, 255};
    dswx_land_mesh_spec_t spec = {};
    spec.shift_wc = g.s_wc, spec.shift_cg = g.s_cg;
    spec.outside_wc = wild ? 80u : 10u, spec.outside_cg = wild ? 255u : 3u;
    const int32_t thr[4] = {wild ? -2 : 4, wild ? 10 : 2, wild ? INT32_MAX : 5, wild ? INT32_MIN + 9 : 3};
    memcpy(spec.thresholds, thr, sizeof thr);
    spec.year_offset = wild ? INT32_MAX : 21;
    spec.n_forest_classes = (variant & 8) ? 0 : 5;
    spec.forest_classes = (variant & 8) ? nullptr : forest;
    spec.wc_tile_stride = wc_stride, spec.cg_tile_stride = cg_stride, spec.land_tile_stride = land_stride;
    spec.mesh_wc_tile_stride_nodes = m_wc.stride, spec.mesh_cg_tile_stride_nodes = m_cg.stride;
    if (wild) spec.thresholds[3] = 12;                   // never water: the developed classes and their wrap show
    g_error[0] = 0;
    const int rc = dswx_land_mesh_host(wc.p, g.wc_h, g.wc_w, cg.p, g.cg_h, g.cg_w, &spec, g.n, g.H, g.W, reinterpret_cast<const int32_t*>(m_wc.b.p),
                                       reinterpret_cast<const int32_t*>(m_cg.b.p), land.p, reinterpret_cast<uint64_t*>(head.p));
    int bad = rc != DSWX_OK;
    for (int64_t t = 0; t < g.n && !bad; ++t) {
        uint64_t wc_in = 0, cg_in = 0, all_out = 0, n255 = 0;
        const unsigned char* const wt = wc.p + (size_t)(t * (wc_stride ? wc_stride : g.wc_h * g.wc_w));
        const unsigned char* const ct = cg.p + (size_t)(t * (cg_stride ? cg_stride : g.cg_h * g.cg_w));
        for (int64_t Y = 0; Y < g.H; ++Y)
            for (int64_t X = 0; X < g.W; ++X) {
                int water = 0, urban = 0, tree = 0, inside = 0;
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) {
                        int64_t c, r;
                        wide_pixel(m_wc.tile(t), m_wc.mesh_w, g.s_wc, 3 * X + j, 3 * Y + i, &c, &r);
                        const bool in = c >= 0 && c < g.wc_w && r >= 0 && r < g.wc_h;
                        const int v = in ? wt[r * g.wc_w + c] : (int)spec.outside_wc;
                        inside += in;
                        water += v == 80 || v == 90 || v == 95;
                        urban += v == 50;
                        tree += v == 10;
                    }
                int64_t c, r;
                wide_pixel(m_cg.tile(t), m_cg.mesh_w, g.s_cg, X, Y, &c, &r);
                const bool in = c >= 0 && c < g.cg_w && r >= 0 && r < g.cg_h;
                const int cls = in ? ct[r * g.cg_w + c] : (int)spec.outside_cg;
                bool is_forest = false;
                for (int k = 0; k < spec.n_forest_classes; ++k) is_forest = is_forest || forest[k] == cls;
                if (!is_forest) tree = 0;
                int v = 255;
                if (tree >= spec.thresholds[0]) v = 201;
                if (urban >= spec.thresholds[1]) v = (int)((uint32_t)spec.year_offset & 0xffu);
                if (urban >= spec.thresholds[2]) v = (int)((100u + (uint32_t)spec.year_offset) & 0xffu);
                if (water >= spec.thresholds[3]) v = 200;
                bad += land.p[(size_t)(t * ls + Y * g.W + X)] != v;
                wc_in += (uint64_t)inside, cg_in += in, all_out += inside == 0, n255 += v == 255;
            }
        const uint64_t words[8] = {px, wc_in, 9 * px - wc_in, cg_in, px - cg_in, all_out, n255, 0};
        if (px) bad += memcmp(head.p + (size_t)t * 64, words, 64) != 0;
        else
            for (int k = 0; k < 64; ++k) bad += head.p[(size_t)t * 64 + (size_t)k] != 0xA5;      // an empty lattice writes nothing
        if (t + 1 < g.n)
            for (int64_t k = (int64_t)px; k < ls; ++k) bad += land.p[(size_t)(t * ls + k)] != 0xA5;      // the padding is untouched
    }
    if (bad)
        fprintf(stderr, "land mesh %lld x %lld x %lld (wc %lld x %lld, cg %lld x %lld) shifts %d %d variant %d: %d differences (%s)\n", (long long)g.n,
                (long long)g.H, (long long)g.W, (long long)g.wc_h, (long long)g.wc_w, (long long)g.cg_h, (long long)g.cg_w, g.s_wc, g.s_cg, variant, bad,
                g_error);
    return bad != 0;
}

}  // namespace

int main() {
    int cases = 0, failures = 0;
    // every shift, lattices of 1 x 1, one pixel past a multiple of the step, empty tiles, lattices and rasters
    const Shape shapes[] = {{2, 5, 7, 9, 11, 4, 6, 0, 0},  {1, 1, 1, 1, 1, 1, 1, 0, 8},   {1, 1, 1, 6, 6, 3, 3, 8, 0},  {1, 3, 86, 12, 30, 5, 9, 8, 7},
                            {3, 4, 5, 10, 14, 4, 5, 2, 1}, {2, 9, 6, 20, 13, 8, 6, 3, 2}, {2, 3, 3, 7, 7, 3, 3, 1, 4},  {2, 7, 3, 15, 8, 6, 3, 4, 3},
                            {0, 4, 4, 9, 9, 3, 3, 2, 2},   {2, 0, 5, 9, 9, 3, 3, 1, 1},   {2, 5, 0, 9, 9, 3, 3, 3, 5},  {2, 3, 3, 0, 4, 3, 3, 1, 6},
                            {2, 3, 4, 5, 0, 0, 3, 5, 2},   {2, 2, 3, 6, 6, 3, 0, 6, 0},   {3, 12, 9, 30, 25, 9, 8, 7, 5}, {1, 6, 11, 17, 29, 4, 7, 6, 8}};
    int k = 0;
    for (const Shape& g : shapes)
        for (int variant = 0; variant < 16; ++variant, ++k, ++cases) failures += land_case(g, variant, (size_t)(2 * (k % 4) + 1));
    printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
    return failures ? 1 : 0;
}
