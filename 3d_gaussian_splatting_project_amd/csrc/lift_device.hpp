// lift_device.hpp - what the kernels that walk a frame's blend for its weights share (lift.hip: weights onto the splats;
// labelmap.hip: weights onto the pixels; depthmap.hip: weights times depth keys onto the pixels): the fixed-point unit, the tile
// and chunk geometry and the fragment arithmetic.  All three units are compiled with -ffp-contract=off, like blend.hip whose
// operation order lift_fragment keeps.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsx {

static constexpr int kLiftShift = 20;
static constexpr int kLiftOne = 1 << kLiftShift;  // GSX_LIFT_ONE: the fixed-point weight 1.0
static constexpr int kLiftTile = 16;
static constexpr int kLiftThreads = kLiftTile * kLiftTile;
static constexpr int kLiftChunk = 256;   // records staged through LDS at a time, and between two opacity votes (blend_kernel's)
static constexpr int kLiftMaxBins = 256;
static_assert(kLiftThreads == 256 && kLiftChunk == kLiftThreads, "one staged record per thread; four waves");

// blend_one's alpha channel, operation for operation: -> the fragment's weight (0: discarded), dst.a updated
__device__ __forceinline__ float lift_fragment(float& a, float fxp, float fyp, const float4 r0, const float4 r1, float alpha) {
    const float dx = fxp - r0.x;
    const float dy = fyp - r0.y;
    const float vx = dx * r0.z + dy * r0.w;
    const float vy = dx * r1.x + dy * r1.y;
    const float A = -(vx * vx + vy * vy);
    float w = 0.0f;
    if (!(A < -4.0f)) {  // `if (A < -4.0) discard;`
        const float B = __expf(A) * alpha;
        const float om = 1.0f - a;  // ONE_MINUS_DST_ALPHA, ONE
        w = om * B;
        a = __builtin_fmaf(om, B, a);
    }
    return w;
}

// rank of bit v among the set bits of the 256-bit mask pw
__device__ __forceinline__ uint32_t rank256(const uint32_t pw[8], uint32_t v) {
    uint32_t r = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t m = j < (v >> 5) ? 0xffffffffu : j == (v >> 5) ? ((1u << (v & 31u)) - 1u) : 0u;
        r += (uint32_t)__popc(pw[j] & m);
    }
    return r;
}

}  // namespace gsx
