// Device helpers shared by the units that make class maps from network outputs (segmap.hip, queries.hip): the widening of an
// output's element (GSX_F32 / F16 / BF16) and the nearest-neighbour index rules.  Both units are built with -ffp-contract=off.
// (The element codes of a class map as an argument, GSX_SEG_*, are seg_dtype.hpp's.)
#pragma once
#include <hip/hip_fp16.h>

#include "gsx_ctx.hpp"

namespace gsx {

template <int DT>
struct SegBits { using type = uint16_t; };
template <>
struct SegBits<GSX_F32> { using type = uint32_t; };

// the value of an element as fp32: exact for all three formats, so comparing the results compares the elements
template <int DT>
__device__ __forceinline__ float seg_val(unsigned bits) {
    if (DT == GSX_F32) return __uint_as_float(bits);
    if (DT == GSX_F16) return __half2float(__ushort_as_half((unsigned short)bits));
    return __uint_as_float(bits << 16);
}

// ---- nearest resize, source index of destination index d, S source pixels ----------------------------------------------------------
// OpenCV's resizeNN: s(d) = min(floor(d * inv), S - 1) with inv = 1.0 / ((double)D / S) from the host
__device__ __forceinline__ int seg_src(int d, double inv, int S) {
    const int s = (int)floor((double)d * inv);
    return s < S - 1 ? s : S - 1;
}

// torch's 'nearest': s(d) = min((int)floorf(d * scale), S - 1) with scale = (float)S / D from the host, one fp32 product
__device__ __forceinline__ int seg_src_torch(int d, float scale, int S) {
    const float f = floorf((float)d * scale);               // >= 0
    const int s = f < 2147483648.f ? (int)f : S - 1;        // the conversion never overflows
    return s < S - 1 ? s : S - 1;
}

}  // namespace gsx
