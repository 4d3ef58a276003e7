// dswx_hist_bin.h -- the bin of an element (include/dswx_hip.h "histogram"), the ONE definition that dswx_histogram.hip and
// dswx_crosstab.hip share: compiled for the kernels and for the host entries of both, so none of the four can differ.
#pragma once
#include <cstdint>

#include "dswx_hip.h"

namespace {

// THE BIN of an element (include/dswx_hip.h "histogram"): `raw` holds the element's bits in its low 8 / 16 bits; -1 = not
// counted.  One function for the kernels and for the host entries.
template <int KIND> __host__ __device__ __forceinline__ int hist_bin(unsigned raw, int lo, int shift) {
    if constexpr (KIND == DSWX_HIST_U8) {
        return (int)(raw & 0xffu);
    } else if constexpr (KIND == DSWX_HIST_DIAG) {
        // The saved DIAG form writes test bit k as decimal digit k.  Taking 10^4 .. 10^1 off once each where they fit leaves
        // 0 or 1 exactly when every decimal digit of v is 0 or 1 (digits of at most 1 never carry, so v then IS the sum that
        // was taken off; a digit of 2 or more, or a value above 11111, leaves more than 1): no division.
        unsigned v = raw & 0xffffu;
        if (v == 65535u) return 32;
        int bin = 0;
        if (v >= 10000u) { v -= 10000u; bin |= 16; }
        if (v >= 1000u) { v -= 1000u; bin |= 8; }
        if (v >= 100u) { v -= 100u; bin |= 4; }
        if (v >= 10u) { v -= 10u; bin |= 2; }
        return v <= 1u ? (bin | (int)v) : 33;
    } else {
        // d = v - lo as an integer lies in (-2^32, 2^32) (|v| < 2^16, lo an int32), and the counted range [0, 256 << shift) is
        // inside [0, 2^16]: modulo 2^32 a negative d lands at or above 2^31 - 2^15 and a d past the range stays itself, so the
        // ONE unsigned compare decides exactly what the definition's two signed ones do, without 64-bit arithmetic.
        const int v = KIND == DSWX_HIST_I16 ? (int)(int16_t)(uint16_t)(raw & 0xffffu) : (int)(raw & 0xffffu);
        const unsigned d = (unsigned)v - (unsigned)lo;
        return d < (256u << shift) ? (int)(d >> shift) : -1;
    }
}

template <int KIND> struct HistElem { static constexpr int BYTES = KIND == DSWX_HIST_U8 ? 1 : 2; };

}  // namespace
