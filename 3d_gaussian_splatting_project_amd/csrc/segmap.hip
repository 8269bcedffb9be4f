// Class maps from a segmentation network's output, on the device: the step between the network and the vote
// (the reference's deep_learning_segmentation.py, "dls.py": 85-124 YOLO instances composited into a map, 142-144 SegFormer
// logits -> arg-max -> nearest resize).  Both paths first build the map at the network's own resolution - a few tens of
// thousands of pixels, which stay in L2 - and then gather it to the image size; a nearest resize only copies pixels, so
// compositing before the resize gives what dls.py:120-121 gives by resizing every mask first.
// Nothing here rounds: floats are only compared, and the one multiplication of the resize rule is a single fp64 product
// (this file is built with -ffp-contract=off like its siblings).  The gather kernel also serves queries.hip, with torch's
// nearest rule (one fp32 product) instead of OpenCV's; the two producers here keep OpenCV's.
#include <climits>

#include "segmap_device.hpp"

namespace gsx {

// ---- the units the kernels are built on (gsx_debug_segmap_constants hands them to the tests) --------------------------------------
static constexpr int kSegVec = 2;                        // consecutive pixels of one lane: one load of 8 bytes (fp32) or 4 (fp16, bf16)
static constexpr int kSegSlices = 16;                    // waves of a workgroup; wave s walks the channel steps s, s + 16, ..
static constexpr int kSegStep = 8;                       // channels (instances) a wave loads before it compares them
static constexpr int kSegPixWg = 64 * kSegVec;           // pixels per workgroup of the arg-max and the instance kernel
static constexpr int kSegBlock = 64 * kSegSlices;
static constexpr int kSegResizeVec = 4;                  // consecutive output pixels of one lane of the resize kernel: one 16-byte store
static constexpr int kSegResizeBlock = 256;

// pixels [i, i + kSegVec) of a plane of n pixels, as one load where the address allows it; pixels past the end read as 0
template <int DT>
__device__ __forceinline__ void seg_load(const typename SegBits<DT>::type* __restrict__ p, long long i, long long n, float v[kSegVec]) {
    using U = typename SegBits<DT>::type;
    static_assert(kSegVec == 2, "the vector forms below load two elements");
    if (i + kSegVec <= n && (reinterpret_cast<uintptr_t>(p + i) & (uintptr_t)(kSegVec * sizeof(U) - 1)) == 0) {
        if (sizeof(U) == 4) {
            const uint2 r = *reinterpret_cast<const uint2*>(p + i);
            v[0] = seg_val<DT>(r.x), v[1] = seg_val<DT>(r.y);
        } else {
            const unsigned r = *reinterpret_cast<const unsigned*>(p + i);
            v[0] = seg_val<DT>(r & 0xffffu), v[1] = seg_val<DT>(r >> 16);
        }
    } else {  // a volume aligned to its element only, an odd plane size, and the ragged end
#pragma unroll
        for (int j = 0; j < kSegVec; ++j) v[j] = i + j < n ? seg_val<DT>(p[i + j]) : 0.f;
    }
}

// torch.argmax's order (dls.py:142) as a relation that does not depend on who is compared first: a NaN is the maximum, equal
// values (-0.0 == +0.0) and two NaNs go to the lower index.  (-inf, INT_MAX) is "no channel seen": it loses to every channel.
__device__ __forceinline__ bool seg_better(float va, int ia, float vb, int ib) {
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return na && (!nb || ia < ib);
    return va > vb || (va == vb && ia < ib);
}

// ---- arg-max over the channels: low[img][p] = argmax_c logits[img][c][p] ----------------------------------------------------------------
// A workgroup owns kSegPixWg pixels of one volume; each of its kSegSlices waves walks every kSegSlices-th step of kSegStep
// channels (kSegStep independent loads in flight per lane), and the slices meet in LDS.
template <int DT>
__global__ __launch_bounds__(kSegBlock) void segmap_argmax_kernel(const void* __restrict__ logits, int C, long long hw, unsigned tiles,
                                                                  int* __restrict__ low) {
    using U = typename SegBits<DT>::type;
    __shared__ float s_val[kSegSlices][kSegPixWg];
    __shared__ int s_idx[kSegSlices][kSegPixWg];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned img = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const long long px0 = (long long)tile * kSegPixWg + lane * kSegVec;
    const U* __restrict__ vol = reinterpret_cast<const U*>(logits) + (long long)img * C * hw;
    float bv[kSegVec];
    int bi[kSegVec];
#pragma unroll
    for (int e = 0; e < kSegVec; ++e) bv[e] = -INFINITY, bi[e] = INT_MAX;
    if (px0 < hw) {
        for (int c0 = wave * kSegStep; c0 < C; c0 += kSegSlices * kSegStep) {
            float v[kSegStep][kSegVec];
#pragma unroll
            for (int j = 0; j < kSegStep; ++j)
                if (c0 + j < C) seg_load<DT>(vol + (long long)(c0 + j) * hw, px0, hw, v[j]);
#pragma unroll
            for (int j = 0; j < kSegStep; ++j)
                if (c0 + j < C) {
#pragma unroll
                    for (int e = 0; e < kSegVec; ++e)
                        if (seg_better(v[j][e], c0 + j, bv[e], bi[e])) bv[e] = v[j][e], bi[e] = c0 + j;
                }
        }
    }
#pragma unroll
    for (int e = 0; e < kSegVec; ++e) s_val[wave][lane * kSegVec + e] = bv[e], s_idx[wave][lane * kSegVec + e] = bi[e];
    __syncthreads();
    if (threadIdx.x < kSegPixWg) {
        const long long p = (long long)tile * kSegPixWg + threadIdx.x;
        if (p < hw) {
            float v = s_val[0][threadIdx.x];
            int i = s_idx[0][threadIdx.x];
#pragma unroll
            for (int s = 1; s < kSegSlices; ++s) {
                const float vs = s_val[s][threadIdx.x];
                const int is = s_idx[s][threadIdx.x];
                if (seg_better(vs, is, v, i)) v = vs, i = is;
            }
            low[(long long)img * hw + p] = i;  // channel 0 always competes, so i < C
        }
    }
}

// ---- instances: low[p] = (int)cls[k] of the highest accepted k whose mask is > 0.5 at p, or -1 (dls.py:113-122) ------------------------
// "later instances overwrite earlier ones" is "the highest index wins", which no order of looking can change: wave s walks the
// steps of kSegStep instances n - 1 - s, n - 1 - s - 16, .. downwards, stops once every pixel of the wave has a hit, and the
// slices meet in LDS by maximum.  conf is read on the device (wave-uniform): conf > 0.5 in fp32, so 0.5 and NaN are left out.
template <int DT>
__global__ __launch_bounds__(kSegBlock) void segmap_masks_kernel(const void* __restrict__ masks, int K, long long hw, const float* __restrict__ cls,
                                                                 const float* __restrict__ conf, int* __restrict__ low) {
    using U = typename SegBits<DT>::type;
    __shared__ int s_top[kSegSlices][kSegPixWg];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long px0 = (long long)blockIdx.x * kSegPixWg + lane * kSegVec;
    const bool in = px0 < hw;
    const U* __restrict__ base = reinterpret_cast<const U*>(masks);
    int top[kSegVec];
#pragma unroll
    for (int e = 0; e < kSegVec; ++e) top[e] = -1;
    const int nsteps = (K + kSegStep - 1) / kSegStep;
    for (int g = nsteps - 1 - wave; g >= 0; g -= kSegSlices) {  // wave-uniform bounds: every lane meets the ballot below
        float v[kSegStep][kSegVec];
        bool acc[kSegStep];
#pragma unroll
        for (int j = 0; j < kSegStep; ++j) {
            const int k = g * kSegStep + j;
            acc[j] = k < K && conf[k] > 0.5f;
#pragma unroll
            for (int e = 0; e < kSegVec; ++e) v[j][e] = 0.f;
            if (acc[j] && in) seg_load<DT>(base + (long long)k * hw, px0, hw, v[j]);
        }
#pragma unroll
        for (int j = kSegStep - 1; j >= 0; --j)
            if (acc[j]) {
#pragma unroll
                for (int e = 0; e < kSegVec; ++e)
                    if (top[e] < 0 && v[j][e] > 0.5f) top[e] = g * kSegStep + j;
            }
        bool open = false;
#pragma unroll
        for (int e = 0; e < kSegVec; ++e) open = open || (top[e] < 0 && px0 + e < hw);
        if (__ballot(open) == 0ull) break;
    }
#pragma unroll
    for (int e = 0; e < kSegVec; ++e) s_top[wave][lane * kSegVec + e] = top[e];
    __syncthreads();
    if (threadIdx.x < kSegPixWg) {
        const long long p = (long long)blockIdx.x * kSegPixWg + threadIdx.x;
        if (p < hw) {
            int t = s_top[0][threadIdx.x];
#pragma unroll
            for (int s = 1; s < kSegSlices; ++s) t = max(t, s_top[s][threadIdx.x]);
            low[p] = t >= 0 ? (int)cls[t] : -1;  // the final astype(np.int32) of dls.py:124 truncates
        }
    }
}

// ---- nearest resize: OpenCV's rule for the two producers here, torch's for the queries (segmap_device.hpp) -----------------------------
// inv: OpenCV's 1.0 / ((double)D / S), or torch's (float)S / D widened (exactly) to a double
template <bool TORCH>
__device__ __forceinline__ int seg_src_rule(int d, double inv, int S) {
    return TORCH ? seg_src_torch(d, (float)inv, S) : seg_src(d, inv, S);
}

// out[img][y][x] = low[img][sy(y)][sx(x)]; a lane owns kSegResizeVec consecutive pixels of one output row
template <bool TORCH>
__global__ __launch_bounds__(kSegResizeBlock) void segmap_resize_kernel(const int* __restrict__ low, int w, int h, int W, int H, int qpr,
                                                                        long long nquads, double inv_x, double inv_y, int* __restrict__ out) {
    const long long q = (long long)blockIdx.x * kSegResizeBlock + threadIdx.x;
    if (q >= nquads) return;
    const long long row = q / qpr;
    const int x0 = (int)(q - row * qpr) * kSegResizeVec;
    const long long img = row / H;
    const int y = (int)(row - img * H);
    const int* __restrict__ src = low + img * ((long long)h * w) + (long long)seg_src_rule<TORCH>(y, inv_y, h) * w;
    int* dst = out + row * W + x0;
    int v[kSegResizeVec];
#pragma unroll
    for (int j = 0; j < kSegResizeVec; ++j) v[j] = x0 + j < W ? src[seg_src_rule<TORCH>(x0 + j, inv_x, w)] : 0;
    static_assert(kSegResizeVec == 4, "the vector store below writes four pixels");
    if (x0 + kSegResizeVec <= W && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<int4*>(dst) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kSegResizeVec; ++j)
            if (x0 + j < W) dst[j] = v[j];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
int seg_elem_bytes(int dtype) {
    switch (dtype) {
        case GSX_F32: return 4;
        case GSX_F16: case GSX_BF16: return 2;
    }
    return 0;
}

bool seg_misaligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) != 0; }

int seg_launch_resize(Ctx* c, int n, int w, int h, int W, int H, int32_t* out, bool torch_rule) {
    const int qpr = (W + kSegResizeVec - 1) / kSegResizeVec;
    const long long nquads = (long long)n * H * qpr;
    const dim3 grid((unsigned)((nquads + kSegResizeBlock - 1) / kSegResizeBlock));
    ProfScope ps(c, "segmap_resize");
    if (torch_rule) {
        const double sx = (double)((float)w / (float)W), sy = (double)((float)h / (float)H);
        hipLaunchKernelGGL(segmap_resize_kernel<true>, grid, dim3(kSegResizeBlock), 0, c->stream, c->seg_low.as<int>(), w, h, W, H, qpr, nquads,
                           sx, sy, out);
    } else {
        const double inv_x = 1.0 / ((double)W / (double)w), inv_y = 1.0 / ((double)H / (double)h);
        hipLaunchKernelGGL(segmap_resize_kernel<false>, grid, dim3(kSegResizeBlock), 0, c->stream, c->seg_low.as<int>(), w, h, W, H, qpr, nquads,
                           inv_x, inv_y, out);
    }
    return GSX_OK;
}

int segmap_from_logits(Ctx* c, const void* logits, int dtype, int n, int C, int h, int w, int out_w, int out_h, int32_t* maps) {
    const char* who = "segmap_from_logits";
    if (!logits || !maps) return fail(c, GSX_E_INVALID, "%s: NULL argument", who);
    if (n <= 0 || C <= 0 || h <= 0 || w <= 0 || out_w <= 0 || out_h <= 0)
        return fail(c, GSX_E_INVALID, "%s: every size must be positive (got n %d, C %d, %d x %d -> %d x %d)", who, n, C, h, w, out_h, out_w);
    const int eb = seg_elem_bytes(dtype);
    if (!eb) return fail(c, GSX_E_INVALID, "%s: unknown dtype %d", who, dtype);
    if (seg_misaligned(logits, eb) || seg_misaligned(maps, 4))
        return fail(c, GSX_E_INVALID, "%s: a pointer is not aligned to its element", who);
    const long long hw = (long long)h * w, HW = (long long)out_h * out_w;
    if (C > 65535) return fail(c, GSX_E_UNSUPPORTED, "%s: %d channels: at most 65535", who, C);
    if (hw >= (1ll << 31) || HW >= (1ll << 31) || (long long)n * HW >= (1ll << 31))
        return fail(c, GSX_E_UNSUPPORTED, "%s: h * w, out_h * out_w and n * out_h * out_w must stay below 2^31 (n %d, %d x %d -> %d x %d)", who,
                    n, h, w, out_h, out_w);
    const long long tiles = (hw + kSegPixWg - 1) / kSegPixWg;
    if ((long long)n * tiles >= (1ll << 31))
        return fail(c, GSX_E_UNSUPPORTED, "%s: %d volumes of %d x %d are more workgroups than one launch holds", who, n, h, w);
    GSX_HIP(c, hipSetDevice(c->device));
    GSX_HIP(c, c->seg_low.ensure((size_t)n * (size_t)hw * sizeof(int)));
    {
        const dim3 grid((unsigned)(n * tiles));
        ProfScope ps(c, "segmap_argmax");
#define GSX_SEG_ARGMAX(DT) \
    hipLaunchKernelGGL((segmap_argmax_kernel<DT>), grid, dim3(kSegBlock), 0, c->stream, logits, C, hw, (unsigned)tiles, c->seg_low.as<int>())
        switch (dtype) {
            case GSX_F32: GSX_SEG_ARGMAX(GSX_F32); break;
            case GSX_F16: GSX_SEG_ARGMAX(GSX_F16); break;
            default: GSX_SEG_ARGMAX(GSX_BF16); break;
        }
#undef GSX_SEG_ARGMAX
    }
    GSX_HIP(c, hipGetLastError());
    seg_launch_resize(c, n, w, h, out_w, out_h, maps);
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

int segmap_from_masks(Ctx* c, const void* masks, int dtype, int K, int mh, int mw, const float* cls, const float* conf, int out_w, int out_h,
                      int32_t* map) {
    const char* who = "segmap_from_masks";
    if (!map) return fail(c, GSX_E_INVALID, "%s: map_dev is NULL", who);
    if (K < 0) return fail(c, GSX_E_INVALID, "%s: K must not be negative (got %d)", who, K);
    if (K > 0 && (!masks || !cls || !conf)) return fail(c, GSX_E_INVALID, "%s: masks_dev, cls_dev and conf_dev may be NULL only when K == 0", who);
    if (mh <= 0 || mw <= 0 || out_w <= 0 || out_h <= 0)
        return fail(c, GSX_E_INVALID, "%s: every size must be positive (got %d x %d -> %d x %d)", who, mh, mw, out_h, out_w);
    const int eb = seg_elem_bytes(dtype);
    if (!eb) return fail(c, GSX_E_INVALID, "%s: unknown dtype %d", who, dtype);
    if (seg_misaligned(map, 4) || (K > 0 && (seg_misaligned(masks, eb) || seg_misaligned(cls, 4) || seg_misaligned(conf, 4))))
        return fail(c, GSX_E_INVALID, "%s: a pointer is not aligned to its element", who);
    const long long hw = (long long)mh * mw, HW = (long long)out_h * out_w;
    if (hw >= (1ll << 31) || HW >= (1ll << 31))
        return fail(c, GSX_E_UNSUPPORTED, "%s: mh * mw and out_h * out_w must stay below 2^31 (%d x %d -> %d x %d)", who, mh, mw, out_h, out_w);
    GSX_HIP(c, hipSetDevice(c->device));
    GSX_HIP(c, c->seg_low.ensure((size_t)hw * sizeof(int)));
    {
        const dim3 grid((unsigned)((hw + kSegPixWg - 1) / kSegPixWg));
        ProfScope ps(c, "segmap_masks");
#define GSX_SEG_MASKS(DT) \
    hipLaunchKernelGGL((segmap_masks_kernel<DT>), grid, dim3(kSegBlock), 0, c->stream, masks, K, hw, cls, conf, c->seg_low.as<int>())
        switch (dtype) {
            case GSX_F32: GSX_SEG_MASKS(GSX_F32); break;
            case GSX_F16: GSX_SEG_MASKS(GSX_F16); break;
            default: GSX_SEG_MASKS(GSX_BF16); break;
        }
#undef GSX_SEG_MASKS
    }
    GSX_HIP(c, hipGetLastError());
    seg_launch_resize(c, 1, mw, mh, out_w, out_h, map);
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

void segmap_constants(int32_t out[8]) {
    out[0] = kSegPixWg;
    out[1] = kSegSlices;
    out[2] = kSegStep;
    out[3] = kSegVec;
    out[4] = kSegResizeVec;
    out[5] = kSegResizeBlock;
    out[6] = kSegBlock;
    out[7] = 0;
}

}  // namespace gsx
