// body_table_host_san.cpp -- dswx_body_table_host and dswx_body_rule.h (proteus_amd/csrc/dswx_body_table.hip) under ASan + UBSan
// on the CPU: the source is compiled INTO this program (tests/test_body_table.py has the command line), which calls the host
// entry with the label plane, the value plane and every output in heap blocks of exactly the bytes the entry may touch, at odd
// addresses inside them, and compares with the definition written out here.  The label planes come from a flood fill; in a
// third of the cases some labels are then replaced by wild values, which the entry must survive without reading outside the
// tile.  No device, no context: the launch half of the source is linked but never called.  Prints one JSON line; exit status
// 0 = every case equal.
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

struct Row {
    uint32_t label, area, x_min, x_max, y_min, y_max;
    uint64_t perimeter, sum_x, sum_y;
    uint32_t count[4];
};

// `want`: 0 dense alone, 1 dense + head, 2 all three
int run_case(int64_t T, int64_t H, int64_t W, int conn, unsigned density, int n_cats, int64_t extra, size_t off, int want, int rows_mode,
             bool wild) {
    const int64_t n = H * W, stride = n + extra;
    // the label plane: a flood fill of random members, every tile from its own pixel 0
    std::vector<uint32_t> lab((size_t)(T * n), 0u);
    std::vector<int64_t> todo;
    int64_t k_max = 0;
    for (int64_t t = 0; t < T; ++t) {
        std::vector<uint8_t> member((size_t)n);
        for (auto& m : member) m = rnd() % 100 < density;
        uint32_t* l = lab.data() + t * n;
        int64_t k = 0;
        for (int64_t seed = 0; seed < n; ++seed) {
            if (!member[(size_t)seed] || l[seed]) continue;
            ++k;
            todo.assign(1, seed);
            l[seed] = (uint32_t)seed + 1u;
            while (!todo.empty()) {
                const int64_t p = todo.back(), y = p / W, x = p % W;
                todo.pop_back();
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((!dy && !dx) || (conn == 4 && dy && dx)) continue;
                        const int64_t yy = y + dy, xx = x + dx;
                        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                        const int64_t q = yy * W + xx;
                        if (!member[(size_t)q] || l[q]) continue;
                        l[q] = (uint32_t)seed + 1u;
                        todo.push_back(q);
                    }
            }
        }
        if (wild)
            for (int i = 0; i < 6 && n > 0; ++i) {
                const uint32_t choice[] = {(uint32_t)n + 1u, 0xFFFFFFFFu, 0x80000000u, 1u + rnd() % (uint32_t)n, 0u, (uint32_t)n};
                l[rnd() % (uint32_t)n] = choice[rnd() % 6];
            }
        k = 0;
        for (int64_t p = 0; p < n; ++p) k += l[p] == (uint32_t)p + 1u;
        if (k > k_max) k_max = k;
    }
    dswx_body_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    spec.n_cats = n_cats;
    for (int b = 0; b < 256; ++b) spec.cat_of_byte[b] = (uint8_t)(rnd() % 7);
    spec.cat_of_byte[0xA5] = 0;                                       // the padding byte is COUNTED: reading it would show
    spec.max_rows = want < 2 ? 0 : rows_mode == 0 ? k_max : rows_mode == 1 ? k_max + 2 : k_max / 2;
    const int64_t R = spec.max_rows;
    const size_t px = (size_t)(T * n);
    Block label(4 * px, 1 + off, 0), value(T ? (size_t)((T - 1) * stride + n) : 0, off, 0xA5);
    for (size_t i = 0; i < px; ++i) put_u32(label.p, i, lab[i]);
    for (int64_t t = 0; t < T; ++t)
        for (int64_t i = 0; i < n; ++i) value.p[t * stride + i] = (uint8_t)rnd();
    Block dense(4 * px, 3, 0xEE), rows(64 * (size_t)(T * R), 5 - off, 0xEE), head(64 * (size_t)T, 1, 0xEE);
    dswx_body_out_t out;
    std::memset(&out, 0, sizeof out);
    out.dense = reinterpret_cast<uint32_t*>(dense.p);
    if (want >= 1) out.head = reinterpret_cast<uint64_t*>(head.p);
    if (want >= 2 && R > 0) out.rows = reinterpret_cast<uint32_t*>(rows.p);
    const int rc = dswx_body_table_host(reinterpret_cast<const uint32_t*>(label.p), n_cats ? value.p : nullptr, &spec, T, H, W,
                                        extra ? stride : 0, &out);
    if (rc != DSWX_OK) {
        std::fprintf(stderr, "dswx_body_table_host failed (%d): %s\n", rc, last_error);
        return 1;
    }
    int bad = 0;
    for (int64_t t = 0; t < T; ++t) {
        const uint32_t* l = lab.data() + t * n;
        std::vector<uint32_t> rank((size_t)n, 0u);                       // at a root: 1 + its rank
        uint32_t k = 0;
        for (int64_t p = 0; p < n; ++p)
            if (l[p] == (uint32_t)p + 1u) rank[(size_t)p] = ++k;
        std::vector<Row> table((size_t)k);
        uint64_t good = 0, malformed = 0, edges = 0;
        for (int64_t p = 0; p < n; ++p) {
            const uint32_t L = l[p];
            const bool ok = L != 0 && (uint64_t)L <= (uint64_t)p + 1u && l[L - 1u] == L;
            const uint32_t d = ok ? rank[L - 1u] : 0u;
            bad += get_u32(dense.p, (size_t)(t * n + p)) != d;
            malformed += L != 0 && !ok;
            if (!ok) continue;
            ++good;
            const int64_t y = p / W, x = p % W;
            const unsigned e = (x == 0 || l[p - 1] != L) + (x == W - 1 || l[p + 1] != L) + (y == 0 || l[p - W] != L) + (y == H - 1 || l[p + W] != L);
            edges += e;
            Row& r = table[d - 1u];
            if (!r.area) r = Row{L, 0, (uint32_t)x, (uint32_t)x, (uint32_t)y, (uint32_t)y, 0, 0, 0, {0, 0, 0, 0}};
            ++r.area;
            if ((uint32_t)x < r.x_min) r.x_min = (uint32_t)x;
            if ((uint32_t)x > r.x_max) r.x_max = (uint32_t)x;
            if ((uint32_t)y > r.y_max) r.y_max = (uint32_t)y;
            r.perimeter += e, r.sum_x += (uint64_t)x, r.sum_y += (uint64_t)y;
            const unsigned c = spec.cat_of_byte[value.p[t * stride + p]];
            if (n_cats && c < (unsigned)n_cats) ++r.count[c];
        }
        if (want >= 1) {
            const uint64_t h[8] = {k, k < (uint64_t)R ? k : (uint64_t)R, good, malformed, edges, 0, 0, 0};
            for (int w = 0; w < 8; ++w) bad += get_u64(head.p, (size_t)(t * 64 + w * 8)) != h[w];
        }
        if (out.rows)
            for (int64_t j = 0; j < R; ++j) {
                Row r;
                std::memset(&r, 0, sizeof r);
                if (j < (int64_t)k) r = table[(size_t)j];
                const uint8_t* g = rows.p + 64 * (size_t)(t * R + j);
                const uint32_t w32[6] = {r.label, r.area, r.x_min, r.x_max, r.y_min, r.y_max};
                for (int w = 0; w < 6; ++w) bad += get_u32(g, (size_t)w) != w32[w];
                bad += get_u64(g, 24) != r.perimeter;
                bad += get_u64(g, 32) != r.sum_x;
                bad += get_u64(g, 40) != r.sum_y;
                for (int c = 0; c < 4; ++c) bad += get_u32(g, (size_t)(12 + c)) != r.count[c];
            }
    }
    // the outputs that were not wanted
    if (want < 1)
        for (size_t i = 0; i < head.n; ++i) bad += head.p[i] != 0xEE;
    if (!out.rows)
        for (size_t i = 0; i < rows.n; ++i) bad += rows.p[i] != 0xEE;
    if (bad)
        std::fprintf(stderr, "%lld x %lld x %lld, connectivity %d, n_cats %d, max_rows %lld, wild %d: %d values differ\n", (long long)T,
                     (long long)H, (long long)W, conn, n_cats, (long long)R, (int)wild, bad);
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
                failures += run_case(T, s[0], s[1], cases % 2 ? 8 : 4, d, cases % 5, cases % 3 ? 3 : 0, (size_t)(cases % 4), cases % 3,
                                     (cases / 3) % 3, cases % 3 == 2 ? (cases / 3) % 2 == 0 : cases % 7 == 0);
                ++cases;
            }
    // refusals read and write nothing: NULL or wild buffers would fault if they did
    dswx_body_spec_t spec;
    std::memset(&spec, 0, sizeof spec);
    dswx_body_out_t out;
    std::memset(&out, 0, sizeof out);
    out.dense = reinterpret_cast<uint32_t*>(16);
    const uint32_t* wild_label = reinterpret_cast<const uint32_t*>(16);
    const uint8_t* wild_value = reinterpret_cast<const uint8_t*>(16);
    failures += dswx_body_table_host(wild_label, nullptr, &spec, 1, 1 << 16, (1 << 15) + 1, 0, &out) != DSWX_ERR_ARG;
    failures += dswx_body_table_host(wild_label, nullptr, &spec, 1, 10, 10, 99, &out) != DSWX_ERR_ARG;
    failures += dswx_body_table_host(wild_label, wild_value, &spec, 1, 10, 10, 0, &out) != DSWX_ERR_ARG;                 // value with n_cats 0
    spec.n_cats = 2;
    failures += dswx_body_table_host(wild_label, nullptr, &spec, 1, 10, 10, 0, &out) != DSWX_ERR_ARG;                    // none with n_cats 2
    spec.n_cats = 5;
    failures += dswx_body_table_host(wild_label, wild_value, &spec, 1, 10, 10, 0, &out) != DSWX_ERR_ARG;
    spec.n_cats = 0;
    spec.max_rows = 3;
    failures += dswx_body_table_host(wild_label, nullptr, &spec, 1, 10, 10, 0, &out) != DSWX_ERR_ARG;                    // no rows
    spec.max_rows = 0;
    failures += dswx_body_table_host(nullptr, nullptr, &spec, 0, 10, 10, 0, &out) != DSWX_OK;
    std::printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
    return failures ? 1 : 0;
}
