// dswx_body_rule.h -- what the kernels and the host entry of dswx_body_table.hip both state about a body table
// (include/dswx_hip.h "body table"): compiled for both sides, so the two cannot differ.
#pragma once
#include <cstdint>

#include "dswx_hip.h"

namespace {

// The elements of a tile that one workgroup scans (256 threads of 16): the prefix sum over the roots has a seam at every
// multiple of it.  Published so that tests can build shapes around the seams; proteus_amd/_capi.py mirrors it.
constexpr int DSWX_BODY_CHUNK = 4096;
// The per-chunk root counts that the scan launch handles in one step of its loop (one per thread of its workgroup).
constexpr int DSWX_BODY_SCAN_STEP = 256;

// The rectangle of pixels whose contributions one workgroup of the last launch combines in LDS before it touches a row.
constexpr int DSWX_BODY_RECT_H = 32;
constexpr int DSWX_BODY_RECT_W = 128;

// the words of a row
constexpr int BODY_LABEL = 0, BODY_AREA = 1, BODY_X_MIN = 2, BODY_X_MAX = 3, BODY_Y_MIN = 4, BODY_Y_MAX = 5, BODY_PERIMETER = 6,
              BODY_SUM_X = 8, BODY_SUM_Y = 10, BODY_COUNT = 12;
// the words of the head
constexpr int BODY_HEAD_K = 0, BODY_HEAD_ROWS = 1, BODY_HEAD_MEMBERS = 2, BODY_HEAD_MALFORMED = 3, BODY_HEAD_PERIMETER = 4;
constexpr unsigned BODY_NOT_COUNTED = 4;                 // the category of a byte that is not counted (DSWX_BODY_MAX_CATS)

// A root: the pixel whose label names itself.
__host__ __device__ __forceinline__ bool body_is_root(uint32_t label, uint64_t idx) { return (uint64_t)label == idx + 1u; }
// The bound that comes BEFORE the dependent load of label[L - 1]: a label that names a pixel behind this one (or behind the
// tile: idx + 1 <= height * width) is malformed without anything being read.
__host__ __device__ __forceinline__ bool body_in_reach(uint32_t label, uint64_t idx) { return label != 0u && (uint64_t)label <= idx + 1u; }
// The category of a byte: cat_of_byte's entry where it is below n_cats, else "not counted".
__host__ __device__ __forceinline__ unsigned body_cat(unsigned entry, int n_cats) {
    return entry < (unsigned)n_cats ? entry : BODY_NOT_COUNTED;
}

}  // namespace
