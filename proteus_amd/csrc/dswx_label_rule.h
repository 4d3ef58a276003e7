// dswx_label_rule.h -- the per-pixel and per-body rule of a labelling (include/dswx_hip.h "label"), the ONE definition that
// the kernels and the host entry of dswx_label.hip share: compiled for both sides, so the two cannot differ.
#pragma once
#include <cstdint>

#include "dswx_hip.h"

namespace {

// The rectangle of pixels that one workgroup labels in LDS (dswx_label.hip, launch 1); seams between rectangles are united
// on the global plane (launch 2).  Published so that tests can build shapes around the seams; proteus_amd/_capi.py mirrors it.
constexpr int DSWX_LABEL_RECT_H = 32;
constexpr int DSWX_LABEL_RECT_W = 128;

// member_of_byte folded into 256 bits: bit (b & 31) of word (b >> 5).  The kernels keep the eight words in LDS: word w lies
// in bank w, so no two lanes of a wave ever collide (equal bytes read by broadcast).
__host__ __device__ __forceinline__ void label_member_bits(const uint8_t* member_of_byte, uint32_t (&bits)[8]) {
    for (int w = 0; w < 8; ++w) {
        uint32_t v = 0;
        for (int b = 0; b < 32; ++b) v |= (member_of_byte[w * 32 + b] != 0 ? 1u : 0u) << b;
        bits[w] = v;
    }
}
__host__ __device__ __forceinline__ bool label_is_member(const uint32_t* bits, unsigned byte) {
    return (bits[(byte & 0xffu) >> 5] >> (byte & 31u)) & 1u;
}

// sieved: a member whose body is smaller than min_size becomes `replace`; every other byte is copied
__host__ __device__ __forceinline__ unsigned label_sieve(unsigned byte, bool member, uint32_t size, uint32_t min_size, unsigned replace) {
    return member && size < min_size ? replace : byte;
}

// summary word 8 + b counts the bodies with floor(log2(size)) == b; size >= 1
__host__ __device__ __forceinline__ int label_size_bin(uint32_t size) {
    int b = 0;
    while (size >>= 1) ++b;                              // (at most 31 shifts: size loses a bit every time)
    return b;
}

// The largest body and, on a tie, the smallest label, as ONE key whose maximum is order-independent: words 2 and 3 of the
// summary are label_key_size / label_key_label of the maximum over the bodies; key 0 = no body (a label is at least 1).
__host__ __device__ __forceinline__ uint64_t label_key(uint32_t size, uint32_t label) {
    return ((uint64_t)size << 32) | (uint64_t)(0xFFFFFFFFu - label);
}
__host__ __device__ __forceinline__ uint64_t label_key_size(uint64_t key) { return key >> 32; }
__host__ __device__ __forceinline__ uint64_t label_key_label(uint64_t key) { return key ? (uint64_t)(0xFFFFFFFFu - (uint32_t)key) : 0u; }

}  // namespace
