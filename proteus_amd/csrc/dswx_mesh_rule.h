// dswx_mesh_rule.h -- the ONE statement of the coordinate mesh that the warp and the resample entries read a plane through
// (dswx_warp.hip, dswx_resample.hip; include/dswx_hip.h "warp", POSITION): how many nodes a destination has, the position of a
// destination pixel from the four nodes of its cell, and the per-cell linear form of the same numerator that the warp kernel
// advances along a row.  Integers only.  tests/native/mesh_host_san.cpp executes both forms on the host and holds them equal.
#pragma once

#include <cstdint>

#define MESH_HD __host__ __device__ __forceinline__

namespace {

// Nodes along one side of the mesh of a destination of `dst` pixels: one every 1 << shift pixels and one past the end.
MESH_HD int64_t mesh_dims(int64_t dst, int shift) {
    const int64_t step = (int64_t)1 << shift;
    return ((dst + step - 1) >> shift) + 1;
}

// One coordinate of the position of destination pixel (X, Y) from the four nodes of its cell, in 1/256 source pixel: the
// numerator over step * step, and its rounding.  fx, fy < step = 1 << s, |v| <= 2^31, so |num| < 2^48.
MESH_HD int64_t mesh_numerator(int64_t v00, int64_t v01, int64_t v10, int64_t v11, int64_t fx, int64_t fy, int s) {
    const int64_t step = (int64_t)1 << s;
    return (step - fy) * ((step - fx) * v00 + fx * v01) + fy * ((step - fx) * v10 + fx * v11);
}
MESH_HD int64_t mesh_round(int64_t num, int s) { return s ? (num + ((int64_t)1 << (2 * s - 1))) >> (2 * s) : num; }
MESH_HD int64_t mesh_coord(int64_t v00, int64_t v01, int64_t v10, int64_t v11, int64_t fx, int64_t fy, int s) {
    return mesh_round(mesh_numerator(v00, v01, v10, v11, fx, fy, s), s);
}

// The position (sx, sy); node(k) returns int32 number k of the mesh of this tile (a device load, dswx_load of dswx_host.h on the host).
template <class Node> MESH_HD void mesh_position(Node node, int s, int64_t mesh_w, int64_t X, int64_t Y, int64_t* sx, int64_t* sy) {
    const int64_t step = (int64_t)1 << s;
    const int64_t i = Y >> s, fy = Y & (step - 1), j = X >> s, fx = X & (step - 1);
    const int64_t n00 = 2 * (i * mesh_w + j), n10 = n00 + 2 * mesh_w;
    *sx = mesh_coord(node(n00), node(n00 + 2), node(n10), node(n10 + 2), fx, fy, s);
    *sy = mesh_coord(node(n00 + 1), node(n00 + 3), node(n10 + 1), node(n10 + 3), fx, fy, s);
}

// Within one cell and one destination row the numerator of mesh_coord is linear in fx: num = a + fx * b, with gy = step - fy
// and hy = fy.  The same exact integers as the definition's products in another order: 32 x 32 -> 64 bit products (the weights
// are at most 256, the nodes int32) and a multiplication by the power of two `step`, |a|, |fx * b| < 2^48.
MESH_HD void mesh_cell_linear(int v00, int v01, int v10, int v11, int gy, int hy, int s, long long& a, long long& b) {
    a = ((long long)gy * v00 + (long long)hy * v10) * (1LL << s);
    b = (long long)gy * v01 - (long long)gy * v00 + (long long)hy * v11 - (long long)hy * v10;
}

}  // namespace
