// dswx_burn_rule.h -- what the device kernels and the host statement of the burn (dswx_burn.hip; include/dswx_hip.h "burn")
// share: the constants the tests build their shapes around, which records are malformed, which rows an edge crosses, and the
// exact column of a crossing as quotient and remainder.  Integer arithmetic only.
#pragma once

#include <cstdint>

#define BURN_HD __host__ __device__ __forceinline__

namespace {

// An edge of at most this many rows is finished by the thread that loaded it; a longer one is shared out over the 64 lanes
// of its wave.  (An outline's edges cross 0 or 1 row.)
#define DSWX_BURN_THREAD_ROWS 4
// The pixels of a row that one wave of the scan launch takes per step: 64 lanes of 16 bytes of `acc`.
#define DSWX_BURN_SCAN_STEP 256

enum { BURN_HEAD_RECORDS, BURN_HEAD_MALFORMED, BURN_HEAD_EDGES, BURN_HEAD_TOGGLES, BURN_HEAD_DROPPED, BURN_HEAD_CLAMPED, BURN_HEAD_INSIDE };

// the records of tile t: zero for a table that decreases there or is negative
BURN_HD int64_t burn_count(int64_t first, int64_t behind) { return first >= 0 && behind > first ? behind - first : 0; }

BURN_HD bool burn_legal(int32_t v) { return v >= -(1 << 30) && v <= (1 << 30); }

// An edge oriented downward, and the rows [r0, r1) of a raster of `height` rows whose centre line it crosses:
// y0 <= 256 r + 128 < y1, that is ceil((y0 - 128) / 256) <= r < ceil((y1 - 128) / 256).
struct BurnEdge {
    int64_t x0, y0, x1, y1;
    int64_t r0, r1;
};
BURN_HD bool burn_edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, int64_t height, BurnEdge* e) {
    if (ay == by) return false;
    const bool down = ay < by;
    e->x0 = down ? ax : bx, e->y0 = down ? ay : by, e->x1 = down ? bx : ax, e->y1 = down ? by : ay;
    const int64_t lo = (e->y0 + 127) >> 8, hi = (e->y1 + 127) >> 8;      // (>> of a negative value floors)
    e->r0 = lo > 0 ? lo : 0;
    e->r1 = hi < height ? hi : height;
    return e->r0 < e->r1;
}

// The crossing of row r as a fraction: numerator / den = q + rem / den with 0 <= rem < den; the column is q + (rem > 0).
// |numerator| < 2^63 for legal coordinates: |x1 - x0| <= 2^31 times 0 <= yc - y0 < y1 - y0 <= 2^31, plus |x0 - 128| < 2^30 + 2^7
// times y1 - y0.
struct BurnCross {
    int64_t q, rem;
};
BURN_HD int64_t burn_den(const BurnEdge& e) { return 256 * (e.y1 - e.y0); }
BURN_HD BurnCross burn_floor_div(int64_t num, int64_t den) {
    BurnCross c = {num / den, num % den};
    if (c.rem < 0) c.rem += den, --c.q;
    return c;
}
BURN_HD BurnCross burn_cross(const BurnEdge& e, int64_t r) {
    const int64_t yc = 256 * r + 128;
    return burn_floor_div((e.x1 - e.x0) * (yc - e.y0) + (e.x0 - 128) * (e.y1 - e.y0), burn_den(e));
}
// What `rows` rows further down add to the fraction: rows * 256 * (x1 - x0) over the same denominator.
BURN_HD BurnCross burn_step(const BurnEdge& e, int64_t rows) {
    const BurnCross s = burn_floor_div(rows * (e.x1 - e.x0), e.y1 - e.y0);
    return {s.q, 256 * s.rem};
}
BURN_HD void burn_advance(BurnCross* c, const BurnCross& s, int64_t den) {
    c->q += s.q;
    c->rem += s.rem;
    if (c->rem >= den) c->rem -= den, ++c->q;
}
// the column before the clamp to 0
BURN_HD int64_t burn_column(const BurnCross& c) { return c.q + (c.rem > 0); }

}  // namespace
