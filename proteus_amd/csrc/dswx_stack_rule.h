// dswx_stack_rule.h -- the per-byte and per-pixel rule of a stack (include/dswx_hip.h "stack"), the ONE definition that the
// kernel and the host entry of dswx_stack.hip share: compiled for both sides, so the two cannot differ.
#pragma once
#include <cstdint>

#include "dswx_hip.h"

namespace {

// What one byte adds to the packed counters of a pixel: four uint16 fields in one uint64, field k = count[k].  A byte whose
// category is not below n_cats adds nothing -- and "adds nothing" IS "not an observation".  The fields cannot carry into each
// other: a field grows by at most one per tile and n_tiles <= DSWX_STACK_MAX_TILES = 65535.
__host__ __device__ __forceinline__ uint64_t stack_increment(const uint8_t* cat_of_byte, int n_cats, unsigned byte) {
    const unsigned c = cat_of_byte[byte & 0xffu];
    return c < (unsigned)n_cats ? 1ull << (16u * c) : 0ull;
}

// The latest observation of a pixel in one word: tile index << 8 | byte.  Before any observation it is NONE << 8 | fill.
__host__ __device__ __forceinline__ uint32_t stack_latest_none(int fill) {
    return ((uint32_t)DSWX_STACK_NONE << 8) | ((uint32_t)fill & 0xffu);
}

// tile t shows `byte` at a pixel whose state is (acc, latest); `inc` = stack_increment of the byte
__host__ __device__ __forceinline__ void stack_step(uint64_t& acc, uint32_t& latest, uint64_t inc, uint32_t t, unsigned byte) {
    acc += inc;
    if (inc) latest = (t << 8) | (byte & 0xffu);
}

__host__ __device__ __forceinline__ unsigned stack_count(uint64_t acc, int k) { return (unsigned)(acc >> (16 * k)) & 0xffffu; }
__host__ __device__ __forceinline__ unsigned stack_last(uint32_t latest) { return latest & 0xffu; }
__host__ __device__ __forceinline__ unsigned stack_last_index(uint32_t latest) { return latest >> 8; }
// (100 * count[0]) / n_obs; the fields of the categories that do not exist are zero, so n_obs is the sum of all four
__host__ __device__ __forceinline__ unsigned stack_share(uint64_t acc) {
    const unsigned n_obs = stack_count(acc, 0) + stack_count(acc, 1) + stack_count(acc, 2) + stack_count(acc, 3);
    return n_obs ? (100u * stack_count(acc, 0)) / n_obs : (unsigned)DSWX_STACK_NO_SHARE;
}

}  // namespace
