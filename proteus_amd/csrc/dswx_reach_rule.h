// dswx_reach_rule.h -- what the device kernels and the host statement of the reach (dswx_reach.hip; include/dswx_hip.h
// "reach") share: the exact predicate "the centre of pixel (c, r) lies within `radius` of the closed segment A -> B", and the
// ONE interval of columns that it holds on along a row.  The records, their legality and the count of a tile are the burn's
// (dswx_burn_rule.h: burn_count, burn_legal), stated there once.
//
// The predicate in integers, with d = B - A, u = P - A, D = d.d, t = u.d, R = radius:
//     D == 0 or t <= 0:  u.u <= R^2          t >= D:  |P - B|^2 <= R^2          otherwise:  (u x d)^2 <= R^2 D
// Widths.  |d| <= 2^31 per axis, so D <= 2^63 (uint64); |u| < 2^39 per axis (a pixel centre is below 2^38 + 2^7, a coordinate
// at most 2^30), so t and u x d reach 2^71: both are __int128.  R^2 D <= 2^103, and (u x d)^2 <= R^2 D iff |u x d| <= K with
// K = isqrt(R^2 D) < 2^52, once per edge: nothing is ever squared past 128 bits.  A disc needs u.u only where |ux|, |uy| <= R
// <= 2^20, which fits 64 bits.
//
// The interval of a row.  The capsule of an edge is convex, so the reached centres of a row are one run of columns: the hull
// of three pieces -- the discs of the two endpoints and the slab 0 <= t <= D, |u x d| <= K between them (on t == 0 and t == D
// the slab's test IS the disc's: u is perpendicular to d there).  A disc is exact as it stands: h = isqrt(R^2 - uy^2), columns
// ceil((ax - h - 128) / 256) .. floor((ax + h - 128) / 256).  The slab is two strips that are linear in the column; their ends
// are ESTIMATED in double, widened by REACH_SLACK, and then moved with the exact slab predicate until it flips -- inward while
// the end is not in the slab, outward while the column behind it still is.  The estimate decides nothing: a poor one only costs
// steps.  (The estimate is good to well below one unit on every row that an edge is given: there |uy| <= |dy| + R, and the
// rounding of uy * dx, at most 2^-53 (|dy| + R) |dx|, is divided by |dy|.)  Everything is clipped to the columns -1 .. width:
// the two columns beside the raster say whether the interval was cut there.
#pragma once

#include <cmath>
#include <cstdint>

#include "dswx_burn_rule.h"

#define REACH_HD __host__ __device__ __forceinline__

namespace {

// An edge of at most this many rows is finished by the thread that loaded it; a longer one is shared out over the 64 lanes of
// its wave.  (Every edge has at least 2 R / 256 rows: only radii below two pixels stay with their thread.)
#define DSWX_REACH_THREAD_ROWS 4
// The pixels of a row that one wave of the scan launch takes per step: 64 lanes of 16 bytes of `acc`.
#define DSWX_REACH_SCAN_STEP 256
#define REACH_MAX_RADIUS (1u << 20)
#define REACH_SLACK 4.0                                  // units of 1/256 pixel by which the estimated slab is widened

enum { REACH_HEAD_RECORDS, REACH_HEAD_MALFORMED, REACH_HEAD_EDGES, REACH_HEAD_INTERVALS, REACH_HEAD_CUT_LEFT, REACH_HEAD_CUT_RIGHT, REACH_HEAD_REACHED };

typedef __int128 reach_i128;
typedef unsigned __int128 reach_u128;

// floor(sqrt(a)) for a < 2^104: the double square root, then the exact correction
REACH_HD uint64_t reach_isqrt(reach_u128 a) {
    uint64_t k = (uint64_t)sqrt((double)a);
    while ((reach_u128)k * k > a) --k;
    while ((reach_u128)(k + 1) * (k + 1) <= a) ++k;
    return k;
}

// A well-formed edge with what a row needs of it, and the rows [r0, r1) of a raster of `height` rows that it can reach:
// min(ay, by) - R <= 256 r + 128 <= max(ay, by) + R.
struct ReachEdge {
    int64_t ax, ay, dx, dy;
    int64_t R;
    uint64_t D, K;                                       // d.d and isqrt(R^2 D)
    int64_t r0, r1;
};
REACH_HD bool reach_rows(int32_t ay, int32_t by, uint32_t radius, int64_t height, int64_t* r0, int64_t* r1) {
    const int64_t ylo = (int64_t)(ay < by ? ay : by) - (int64_t)radius, yhi = (int64_t)(ay < by ? by : ay) + (int64_t)radius;
    const int64_t lo = (ylo + 127) >> 8, hi = ((yhi - 128) >> 8) + 1;     // (>> of a negative value floors)
    *r0 = lo > 0 ? lo : 0;
    *r1 = hi < height ? hi : height;
    return *r0 < *r1;
}
REACH_HD bool reach_edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, uint32_t radius, int64_t height, ReachEdge* e) {
    e->ax = ax, e->ay = ay, e->dx = (int64_t)bx - ax, e->dy = (int64_t)by - ay;
    e->R = (int64_t)radius;
    e->D = (uint64_t)(e->dx * e->dx) + (uint64_t)(e->dy * e->dy);
    e->K = reach_isqrt((reach_u128)((uint64_t)e->R * (uint64_t)e->R) * e->D);
    return reach_rows(ay, by, radius, height, &e->r0, &e->r1);
}

REACH_HD reach_i128 reach_abs(reach_i128 v) { return v < 0 ? -v : v; }

// |(ux, uy)|^2 <= R^2
REACH_HD bool reach_disc(int64_t ux, int64_t uy, int64_t R) {
    if (ux > R || ux < -R || uy > R || uy < -R) return false;
    return ux * ux + uy * uy <= R * R;
}

// THE PREDICATE: is the point (px, py) within R of the closed segment of e
REACH_HD bool reach_point(const ReachEdge& e, int64_t px, int64_t py) {
    const int64_t ux = px - e.ax, uy = py - e.ay;
    const reach_i128 t = (reach_i128)ux * e.dx + (reach_i128)uy * e.dy;
    if (e.D == 0 || t <= 0) return reach_disc(ux, uy, e.R);
    if (t >= (reach_i128)e.D) return reach_disc(ux - e.dx, uy - e.dy, e.R);
    return reach_abs((reach_i128)ux * e.dy - (reach_i128)uy * e.dx) <= (reach_i128)e.K;
}

// the slab alone, for the column c of the row with uy = yc - ay: 0 <= t <= D and |u x d| <= K
REACH_HD bool reach_slab(const ReachEdge& e, int64_t uy, int64_t c) {
    const int64_t ux = 256 * c + 128 - e.ax;
    const reach_i128 t = (reach_i128)ux * e.dx + (reach_i128)uy * e.dy;
    if (t < 0 || t > (reach_i128)e.D) return false;
    return reach_abs((reach_i128)ux * e.dy - (reach_i128)uy * e.dx) <= (reach_i128)e.K;
}

// The columns of a row that an edge reaches, clipped to -1 .. width: empty iff lo > hi.
struct ReachRun {
    int64_t lo, hi;
};
REACH_HD void reach_join(ReachRun* run, int64_t lo, int64_t hi, int64_t width) {
    if (lo < -1) lo = -1;
    if (hi > width) hi = width;
    if (lo > hi) return;
    if (run->lo > run->hi) {
        run->lo = lo, run->hi = hi;
        return;
    }
    if (lo < run->lo) run->lo = lo;
    if (hi > run->hi) run->hi = hi;
}
// the disc around (cx, .) on a row at the vertical distance uy
REACH_HD void reach_join_disc(ReachRun* run, int64_t cx, int64_t uy, int64_t R, int64_t width) {
    if (uy > R || uy < -R) return;
    const int64_t h = (int64_t)reach_isqrt((reach_u128)(uint64_t)(R * R - uy * uy));
    reach_join(run, (cx - h + 127) >> 8, (cx + h - 128) >> 8, width);
}
REACH_HD ReachRun reach_row(const ReachEdge& e, int64_t r, int64_t width) {
    ReachRun run = {0, -1};
    const int64_t uy = 256 * r + 128 - e.ay;
    reach_join_disc(&run, e.ax, uy, e.R, width);
    if (e.D == 0) return run;
    reach_join_disc(&run, e.ax + e.dx, uy - e.dy, e.R, width);
    // the slab: X = ux of a centre.  t = X dx + uy dy in [0, D] and u x d = X dy - uy dx in [-K, K], estimated in double
    const double fdx = (double)e.dx, fdy = (double)e.dy, fuy = (double)uy, fD = (double)e.D, fK = (double)e.K, fR = (double)e.R;
    double xlo = (e.dx < 0 ? fdx : 0.0) - fR, xhi = (e.dx > 0 ? fdx : 0.0) + fR;          // the capsule itself lies between these
    // (with dx == 0 or dy == 0 that strip holds every column of the row or none, decided exactly here)
    if (e.dx != 0) {
        const double s = -fuy * fdy, a = s / fdx, b = (s + fD) / fdx;
        xlo = fmax(xlo, fmin(a, b)), xhi = fmin(xhi, fmax(a, b));
    } else {
        const reach_i128 t = (reach_i128)uy * e.dy;
        if (t < 0 || t > (reach_i128)e.D) return run;
    }
    if (e.dy != 0) {
        const double q = fuy * fdx, a = (q - fK) / fdy, b = (q + fK) / fdy;
        xlo = fmax(xlo, fmin(a, b)), xhi = fmin(xhi, fmax(a, b));
    } else if (reach_abs((reach_i128)uy * e.dx) > (reach_i128)e.K)
        return run;
    if (!(xlo - REACH_SLACK <= xhi + REACH_SLACK)) return run;
    const double fax = (double)e.ax;
    double clo = ceil((fax + xlo - REACH_SLACK - 128.0) / 256.0), chi = floor((fax + xhi + REACH_SLACK - 128.0) / 256.0);
    clo = fmax(clo, -1.0), chi = fmin(chi, (double)width);
    if (!(clo <= chi)) return run;
    int64_t lo = (int64_t)clo, hi = (int64_t)chi;
    while (lo <= hi && !reach_slab(e, uy, lo)) ++lo;
    while (hi >= lo && !reach_slab(e, uy, hi)) --hi;
    if (lo > hi) return run;
    while (lo > -1 && reach_slab(e, uy, lo - 1)) --lo;
    while (hi < width && reach_slab(e, uy, hi + 1)) ++hi;
    reach_join(&run, lo, hi, width);
    return run;
}

}  // namespace
