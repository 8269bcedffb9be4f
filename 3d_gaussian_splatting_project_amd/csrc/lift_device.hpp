// lift_device.hpp - what the kernels that walk a frame's blend for its weights share (lift.hip: weights onto the splats;
// labelmap.hip: weights onto the pixels; depthmap.hip: weights times depth keys onto the pixels): the fixed-point unit, the tile
// and chunk geometry, and the pieces of a tile's walk - a lane's pixel (lift_pixel), the staging of a record (lift_stage), a
// fragment's quantised weight (lift_weight over lift_fragment), the opacity vote (lift_tile_opaque) and the statistics slot
// (lift_stats_slot).  Each kernel keeps its own loop - rounds with barriers inside, windows around the walk, a second vote - and
// builds it from these, so the three sum the same integers by construction.  All three units are compiled with
// -ffp-contract=off, like blend.hip whose operation order lift_fragment keeps.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gsx_ctx.hpp"

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

// a lane's pixel in its tile: one pixel per lane, 16 lanes per row.  pix is meant only where inside.
struct LiftPixel {
    int px, py;
    bool inside;
    size_t pix;
    float fxp, fyp;  // the pixel centre in GL window coordinates
};

__device__ __forceinline__ LiftPixel lift_pixel(int tile, int tiles_x, int W, int H, int tid) {
    LiftPixel p;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    p.px = tx * kLiftTile + (tid & (kLiftTile - 1));
    p.py = ty * kLiftTile + (tid >> 4);
    p.inside = p.px < W && p.py < H;
    p.pix = (size_t)p.py * (size_t)W + (size_t)p.px;
    p.fxp = (float)p.px + 0.5f;
    p.fyp = (float)H - ((float)p.py + 0.5f);  // window y is up; image row py counts from the top
    return p;
}

// record `id` into slot tid of the staged chunk: its two float4 and the alpha its third one holds in .y
__device__ __forceinline__ void lift_stage(float4* s0, float4* s1, float* sa, const float4* rec, uint32_t id, int tid) {
    s0[tid] = rec[3 * (size_t)id];
    s1[tid] = rec[3 * (size_t)id + 1];
    sa[tid] = reinterpret_cast<const float2*>(rec + 3 * (size_t)id + 2)->y;
}

// the fragment's weight in units of 1 / 2^20, <= 2^20 as w <= 1; a pixel outside the frame gets 0.  dst.a updated
__device__ __forceinline__ uint32_t lift_weight(float& a, const LiftPixel& p, const float4 r0, const float4 r1, float alpha) {
    const float w = lift_fragment(a, p.fxp, p.fyp, r0, r1, alpha);
    return p.inside && w > 0.0f ? (uint32_t)rintf(w * (float)kLiftOne) : 0u;
}

// The opacity vote (a barrier: every lane of the workgroup takes it).  Every further fragment is weighted by (1 - dst.a): the
// frame's rule, a tile stops once that is < 1e-5 on all of it; pixels outside the frame count as opaque.
__device__ __forceinline__ bool lift_tile_opaque(const LiftPixel& p, const float& a) {
    return __syncthreads_and(!p.inside || a > 1.0f - 1.0e-5f);
}

// the workgroup's statistics slot: spread over kConsumedSlots lines like the blend kernels' (slot[0]: records staged)
__device__ __forceinline__ unsigned long long* lift_stats_slot(unsigned long long* consumed) {
    return consumed + (blockIdx.x & (kConsumedSlots - 1)) * 16;
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
