// A class map as an argument: everything that depends on its element code GSX_SEG_* (include/gsx.h), for the units that take
// one - handover.hip, lift.hip, assoc.hip, iou.hip.  (segmap_device.hpp is about the dtypes of network outputs, GSX_F32 ...)
#pragma once
#include <type_traits>

#include "gsx_ctx.hpp"

namespace gsx {

// bytes per element of a map handed over as GSX_SEG_*
constexpr size_t seg_elem_size(int seg_dtype) { return seg_dtype == GSX_SEG_I32 ? 4 : seg_dtype == GSX_SEG_I64 ? 8 : 1; }
constexpr bool seg_dtype_known(int seg_dtype) {
    return seg_dtype == GSX_SEG_I32 || seg_dtype == GSX_SEG_I64 || seg_dtype == GSX_SEG_U8 || seg_dtype == GSX_SEG_U8_LABELS;
}

// the element a map of code DT stores, and what turns a stored value into its bin = label + 1 (a packed u8 map holds the bin itself)
template <int DT>
struct SegElem { using type = uint8_t; static constexpr int add = DT == GSX_SEG_U8 ? 0 : 1; };
template <>
struct SegElem<GSX_SEG_I32> { using type = int32_t; static constexpr int add = 1; };
template <>
struct SegElem<GSX_SEG_I64> { using type = long long; static constexpr int add = 1; };

// Instantiation by code: calls f(std::integral_constant<int, DT>{}) for dt and returns what it returns (the same type for every
// DT).  Callers have validated dt (seg_dtype_known): anything else goes the way of GSX_SEG_U8_LABELS.
template <class F>
static inline auto with_seg_dtype(int dt, F&& f) {
    switch (dt) {
        case GSX_SEG_I32: return f(std::integral_constant<int, GSX_SEG_I32>{});
        case GSX_SEG_I64: return f(std::integral_constant<int, GSX_SEG_I64>{});
        case GSX_SEG_U8: return f(std::integral_constant<int, GSX_SEG_U8>{});
        default: return f(std::integral_constant<int, GSX_SEG_U8_LABELS>{});
    }
}

// bin = value + 1 as an unsigned number (a packed uint8 map holds the bin itself): for n classes or segments, anything outside
// [-1, n - 1] - a value below -1 included - comes out above n
template <int DT>
__device__ __forceinline__ unsigned long long seg_bin(const void* p, long long i) {
    if (DT == GSX_SEG_I32) return (unsigned long long)((unsigned)reinterpret_cast<const int*>(p)[i] + 1u);
    if (DT == GSX_SEG_I64) return (unsigned long long)reinterpret_cast<const long long*>(p)[i] + 1ull;
    if (DT == GSX_SEG_U8) return reinterpret_cast<const uint8_t*>(p)[i];
    return (unsigned long long)reinterpret_cast<const uint8_t*>(p)[i] + 1ull;
}

// four consecutive values of one lane, as one 16-byte load (two for int64, four bytes for uint8) where the pointer allows it:
// p aligned to the load and all four inside the map; otherwise one by one, ~0 past the end
template <int DT>
__device__ __forceinline__ void seg_bins4(const void* p, long long i, long long npix, unsigned long long b[4]) {
    constexpr int B = DT == GSX_SEG_I32 ? 4 : (DT == GSX_SEG_I64 ? 8 : 1);
    const bool vec = (reinterpret_cast<uintptr_t>(p) & (B == 1 ? 3 : 15)) == 0 && i + 4 <= npix;
    if (vec) {
        if (DT == GSX_SEG_I32) {
            const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const int*>(p) + i);
            b[0] = (unsigned long long)(v.x + 1u), b[1] = (unsigned long long)(v.y + 1u);
            b[2] = (unsigned long long)(v.z + 1u), b[3] = (unsigned long long)(v.w + 1u);
        } else if (DT == GSX_SEG_I64) {
            const ulonglong2 v0 = *reinterpret_cast<const ulonglong2*>(reinterpret_cast<const long long*>(p) + i);
            const ulonglong2 v1 = *reinterpret_cast<const ulonglong2*>(reinterpret_cast<const long long*>(p) + i + 2);
            b[0] = v0.x + 1ull, b[1] = v0.y + 1ull, b[2] = v1.x + 1ull, b[3] = v1.y + 1ull;
        } else {
            const unsigned v = *reinterpret_cast<const unsigned*>(reinterpret_cast<const uint8_t*>(p) + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = (unsigned long long)((v >> (8 * j)) & 255u) + (DT == GSX_SEG_U8 ? 0ull : 1ull);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = i + j < npix ? seg_bin<DT>(p, i + j) : ~0ull;
    }
}

}  // namespace gsx
