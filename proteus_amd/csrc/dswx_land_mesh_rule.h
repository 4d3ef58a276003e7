// dswx_land_mesh_rule.h -- the ONE statement of the LAND rule: the class tests of a WorldCover byte, the class hierarchy with
// the uint8 wrap of the two developed classes, the 256-bit set of CGLS forest classes, and the LAND value of an HLS pixel whose
// nine WorldCover taps and one CGLS tap are read through coordinate meshes (include/dswx_hip.h "land mesh").  Host and device:
// dswx_layers.hip (dswx_landcover_mask_*: maps already on their grids), dswx_land_mesh.hip (kernel and host entry) and
// tests/native/land_mesh_host_san.cpp execute it.  Positions are mesh_position of dswx_mesh_rule.h and nothing else.
#pragma once

#include <cstdint>

#include "dswx_mesh_rule.h"

namespace {

// What the hierarchy needs; dswx_layers.hip's LandArgs carries the same fields under the same names.
struct LandRule {
    uint32_t forest_bits[8];     // 256-bit set of CGLS forest classes
    int thr_tree, thr_low, thr_high, thr_water;
    int low_class, high_class;   // year_offset, 100 + year_offset (as uint8)
};

// The class tests of one WorldCover byte as water | urban << 4 | tree << 8: the sum of nine codes IS the three 3 x 3 counts
// (each <= 9 fits its 4-bit field).
MESH_HD uint32_t land_code(int v) {
    return (uint32_t)((((v == 80) | (v == 90) | (v == 95)) ? 1 : 0) | (v == 50 ? 16 : 0) | (v == 10 ? 256 : 0));
}

// `is_forest`: the CGLS class of the pixel is one of forest_mask_landcover_classes
template <class A> MESH_HD int land_class(const A& a, int water, int urban, int tree, bool is_forest) {
    if (!is_forest) tree = 0;
    int v = 255;
    if (tree >= a.thr_tree) v = 201;
    if (urban >= a.thr_low) v = a.low_class;
    if (urban >= a.thr_high) v = a.high_class;
    if (water >= a.thr_water) v = 200;
    return v;
}

template <class A> MESH_HD bool land_is_forest(const A& a, int c) { return ((a.forest_bits[(c & 255) >> 5] >> (c & 31)) & 1u) != 0; }

// The forest set (classes outside 0 .. 255 name no byte), the thresholds and the two developed classes of a request.
// numpy stores the class through a uint8 array: values wrap modulo 256 (the reference's pinned numpy 1.23.5 wraps;
// numpy 2 raises OverflowError instead).  Unsigned sums: 100 + INT32_MAX must wrap, not overflow.
template <class A> inline void land_resolve(A* a, const int32_t* forest_classes, int32_t n_forest_classes, const int32_t thresholds[4],
                                            int32_t year_offset) {
    for (int k = 0; k < 8; ++k) a->forest_bits[k] = 0;
    for (int i = 0; i < n_forest_classes; ++i) {
        const int c = forest_classes[i];
        if (c >= 0 && c <= 255) a->forest_bits[c >> 5] |= 1u << (c & 31);
    }
    a->thr_tree = thresholds[0]; a->thr_low = thresholds[1]; a->thr_high = thresholds[2]; a->thr_water = thresholds[3];
    a->low_class = (int)(uint8_t)(0u + (uint32_t)year_offset);
    a->high_class = (int)(uint8_t)(100u + (uint32_t)year_offset);
}

// The nearest source pixel (c, r) of pixel (X, Y) of a lattice read through a mesh: dswx_warp_*'s, by mesh_position.
template <class Node> MESH_HD void land_tap(Node node, int s, int64_t mesh_w, int64_t X, int64_t Y, int64_t* c, int64_t* r) {
    int64_t sx, sy;
    mesh_position(node, s, mesh_w, X, Y, &sx, &sy);
    *c = sx >> 8;
    *r = sy >> 8;
}
MESH_HD bool land_inside(int64_t c, int64_t r, int64_t height, int64_t width) { return c >= 0 && c < width && r >= 0 && r < height; }

// The nine fine pixels of HLS pixel (X, Y), row-major: fine pixel (3 X + k, 3 Y + i) is number 3 i + k.  Every one evaluates
// mesh_position for itself, so a 3 x 3 block that straddles mesh cells is no special case.  (The per-cell linear form of
// dswx_mesh_rule.h per fine row was measured and bought nothing -- the kernel is not bound by this arithmetic, DESIGN.md
// section 5 -- so it is not used: one form, the definition's.)
template <class Node> MESH_HD void land_fine_taps(Node node, int s, int64_t mesh_w, int64_t X, int64_t Y, int64_t c[9], int64_t r[9]) {
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) land_tap(node, s, mesh_w, 3 * X + k, 3 * Y + i, &c[3 * i + k], &r[3 * i + k]);
}

// What one HLS pixel adds to the head of its tile, beside its LAND value.
struct LandMeshPixel {
    int land;          // 0 .. 255
    int wc_inside;     // 0 .. 9
    int cg_inside;     // 0 or 1
};

// LAND of HLS pixel (X, Y) of a height x width tile.  node_wc / node_cg return int32 number k of the tile's two meshes;
// wc(c, r) / cg(c, r) return the byte of a source pixel that IS inside its raster.
template <class A, class NodeW, class NodeC, class TapW, class TapC>
MESH_HD LandMeshPixel land_mesh_pixel(const A& rule, NodeW node_wc, int shift_wc, int64_t mesh_wc_w, int64_t wc_h, int64_t wc_w, int outside_wc, TapW wc,
                                      NodeC node_cg, int shift_cg, int64_t mesh_cg_w, int64_t cg_h, int64_t cg_w, int outside_cg, TapC cg,
                                      int64_t X, int64_t Y) {
    int64_t c[9], r[9];
    land_fine_taps(node_wc, shift_wc, mesh_wc_w, X, Y, c, r);
    LandMeshPixel px = {255, 0, 0};
    uint32_t cnt = 0;
    for (int k = 0; k < 9; ++k) {
        const bool in = land_inside(c[k], r[k], wc_h, wc_w);
        px.wc_inside += in;
        cnt += land_code(in ? (int)wc(c[k], r[k]) : outside_wc);
    }
    int64_t cc, rr;
    land_tap(node_cg, shift_cg, mesh_cg_w, X, Y, &cc, &rr);
    px.cg_inside = land_inside(cc, rr, cg_h, cg_w);
    const int cls = px.cg_inside ? (int)cg(cc, rr) : outside_cg;
    px.land = land_class(rule, (int)(cnt & 15u), (int)((cnt >> 4) & 15u), (int)(cnt >> 8), land_is_forest(rule, cls));
    return px;
}

}  // namespace
