// Class maps from Mask2Former's query outputs, on the device: transformers' post_process_instance_segmentation as the reference
// calls it (deep_learning_segmentation.py "dls.py":156-158), from the K slots its softmax / top-k selected to the map of segment
// ids (or class ids) at the image size.  tests/queries_model.py is the specification; include/gsx.h states the semantics.
//   queries_sampled   which mid-grid columns and rows the target grid's nearest resize reads, as bit words
//   queries_mask      bilinear to the mid grid, one ballot word of "v > 0" per wave and row, integer counts, fixed-order sigmoid sum
//   queries_accept    per slot: score, acceptance, segment id (an exclusive scan over the slots)
//   queries_compose   per mid-grid pixel: the highest accepted slot whose bit is set
//   segmap_resize     the gather of segmap.hip, with torch's nearest rule
// The bilinear step rounds every product and sum to fp32 as the model does: this file is built with -ffp-contract=off.  No
// floating-point atomics: every sum has one fixed order, so two runs give identical bits.
#include <cmath>

#include "segmap_device.hpp"

namespace gsx {

// ---- the units the kernels are built on (gsx_debug_queries_constants hands them to the tests) ------------------------------------
static constexpr int kQCols = 64;                          // mid-grid columns of a wave: one ballot word
static constexpr int kQWaves = 4;                          // waves of a workgroup of the mask kernel
static constexpr int kQRowsWave = 4;                       // consecutive mid-grid rows a wave walks
static constexpr int kQRowsWg = kQWaves * kQRowsWave;      // rows per workgroup: one partial sum
static constexpr int kQBlock = 64 * kQWaves;
static constexpr int kQMaxSlots = 1024;                    // slots of a call: one thread each in the scan of the accept kernel
static constexpr int kQAcceptWaves = kQMaxSlots / 64;      // wave s reduces the slots s, s + 16, ..
static constexpr int kQScanWord = 64;                      // slots per ballot word of that scan
static constexpr int kQComposeWaves = 4;

using u64 = unsigned long long;

struct QPart {      // what one workgroup of the mask kernel knows about its rows of one slot
    double sum;     // sum of sigmoid(v) over the set pixels, fp64, fixed order
    int count;      // set pixels
    int sampled;    // set pixels on columns and rows the target grid reads
    int nan;        // some v is a NaN
    int pad;
};

// torch's align_corners=False source coordinate in fp32: (i0, i1, l0, l1) of destination index d, S source pixels
__device__ __forceinline__ void q_axis(int d, float scale, int S, int& i0, int& i1, float& l0, float& l1) {
    const float src = fmaxf(scale * ((float)d + 0.5f) - 0.5f, 0.f);
    i0 = min((int)src, S - 1);  // (int)src < S for every d < D; the clamp keeps lanes past the end of a row in bounds
    i1 = i0 + (i0 < S - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

// ---- sampled columns and rows: word j < wpr holds the columns 64 j .., word wpr + j the rows 64 j .. -----------------------------------
// seg_src_torch is monotone in d, so "some destination reads source i" is a lower bound away
__global__ __launch_bounds__(64) void queries_sampled_kernel(int mid_w, int mid_h, int out_w, int out_h, float scale_x, float scale_y, int wpr,
                                                             u64* __restrict__ samp) {
    const bool col = (int)blockIdx.x < wpr;
    const int i = ((int)blockIdx.x - (col ? 0 : wpr)) * 64 + (int)threadIdx.x;
    const int S = col ? mid_w : mid_h, D = col ? out_w : out_h;
    const float scale = col ? scale_x : scale_y;
    bool hit = false;
    if (i < S) {
        int lo = 0, hi = D;
        while (lo < hi) {
            const int m = lo + (hi - lo) / 2;
            if (seg_src_torch(m, scale, S) < i) lo = m + 1; else hi = m;
        }
        hit = lo < D && seg_src_torch(lo, scale, S) == i;
    }
    const u64 word = __ballot(hit);
    if (threadIdx.x == 0) samp[blockIdx.x] = word;
}

// ---- bilinear to the mid grid, threshold, statistics ---------------------------------------------------------------------------------
// grid (wpr * row groups, K): workgroup (wc, rg) of slot k owns the columns [64 wc, 64 wc + 64) of the rows [16 rg, 16 rg + 16);
// wave s walks the rows 16 rg + 4 s .. + 3.  The source (Q planes of h x w) stays in L2.  A slot whose query is outside [0, Q)
// reads and writes nothing: the accept kernel rejects it without looking at its partials.
template <int DT>
__global__ __launch_bounds__(kQBlock) void queries_mask_kernel(const void* __restrict__ masks, int Q, int h, int w,
                                                               const int* __restrict__ slot_query, int mid_w, int mid_h, int wpr, float scale_x,
                                                               float scale_y, const u64* __restrict__ samp, u64* __restrict__ bits,
                                                               QPart* __restrict__ parts) {
    using U = typename SegBits<DT>::type;
    __shared__ double s_sum[kQWaves];
    __shared__ int s_cnt[kQWaves], s_smp[kQWaves], s_nan[kQWaves];
    const int k = blockIdx.y;
    const int q = slot_query[k];
    if (q < 0 || q >= Q) return;  // the whole workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wc = (int)(blockIdx.x % (unsigned)wpr), rg = (int)(blockIdx.x / (unsigned)wpr);
    const int c = wc * kQCols + lane;
    const bool in = c < mid_w;
    int x0, x1;
    float lx0, lx1;
    q_axis(c, scale_x, w, x0, x1, lx0, lx1);
    const U* __restrict__ plane = reinterpret_cast<const U*>(masks) + (long long)q * h * w;
    const u64 col_word = samp[wc];
    double acc = 0.0;
    int cnt = 0, smp = 0, nan = 0;
    for (int i = 0; i < kQRowsWave; ++i) {
        const int r = rg * kQRowsWg + wave * kQRowsWave + i;
        if (r >= mid_h) break;  // wave-uniform
        int y0, y1;
        float ly0, ly1;
        q_axis(r, scale_y, h, y0, y1, ly0, ly1);
        float v = 0.f;
        if (in) {
            const float a00 = seg_val<DT>(plane[(long long)y0 * w + x0]), a01 = seg_val<DT>(plane[(long long)y0 * w + x1]);
            const float a10 = seg_val<DT>(plane[(long long)y1 * w + x0]), a11 = seg_val<DT>(plane[(long long)y1 * w + x1]);
            v = ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11);
        }
        const bool set = v > 0.f;  // 0 and NaN are not set
        const u64 word = __ballot(set);
        if (lane == 0) bits[((long long)k * mid_h + r) * wpr + wc] = word;
        cnt += __popcll(word);
        if ((samp[wpr + (r >> 6)] >> (r & 63)) & 1ull) smp += __popcll(word & col_word);
        nan |= __ballot(v != v) != 0ull;
        if (set) acc += (double)(1.f / (1.f + expf(-v)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);  // a + b == b + a: every lane holds the same bits
    if (lane == 0) s_sum[wave] = acc, s_cnt[wave] = cnt, s_smp[wave] = smp, s_nan[wave] = nan;
    __syncthreads();
    if (threadIdx.x == 0) {
        QPart p{0.0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < kQWaves; ++s) p.sum += s_sum[s], p.count += s_cnt[s], p.sampled += s_smp[s], p.nan |= s_nan[s];
        parts[(long long)k * gridDim.x + blockIdx.x] = p;
    }
}

// ---- score, acceptance, segment ids --------------------------------------------------------------------------------------------------
// One workgroup.  Wave s reduces the partials of the slots s, s + 16, .. (lane l takes the partials l, l + 64, .., then the
// same butterfly), forms pred = score * ((float)sum / ((float)count + 1e-6f)) and the acceptance; then thread k scans.
__global__ __launch_bounds__(kQMaxSlots) void queries_accept_kernel(int K, int Q, int G, const int* __restrict__ slot_query,
                                                                    const float* __restrict__ slot_score, const int* __restrict__ slot_label,
                                                                    const QPart* __restrict__ parts, double threshold, int mode,
                                                                    int* __restrict__ q_seg, int* __restrict__ q_val,
                                                                    int* __restrict__ slot_segment, float* __restrict__ slot_pred) {
    __shared__ float s_pred[kQMaxSlots];
    __shared__ int s_acc[kQMaxSlots];
    __shared__ int s_wave[kQAcceptWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = wave; k < K; k += kQAcceptWaves) {
        const int q = slot_query[k];
        const bool valid = q >= 0 && q < Q;
        double sum = 0.0;
        long long cnt = 0, smp = 0;
        int nan = 0;
        if (valid)
            for (int g = lane; g < G; g += 64) {
                const QPart p = parts[(long long)k * G + g];
                sum += p.sum, cnt += p.count, smp += p.sampled, nan |= p.nan;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o), cnt += __shfl_xor(cnt, o), smp += __shfl_xor(smp, o);
        nan = __ballot(nan != 0) != 0ull;
        if (lane == 0) {
            float pred = 0.f;  // a slot that reads nothing scores 0
            bool acc = false;
            if (valid) {
                const float total = nan ? NAN : (float)sum;  // torch's NaN * 0: one NaN anywhere in the mask poisons the sum
                pred = slot_score[k] * (total / ((float)cnt + 1e-6f));
                acc = smp > 0 && (double)pred >= threshold;
            }
            s_pred[k] = pred, s_acc[k] = acc;
        }
    }
    __syncthreads();
    const int k = threadIdx.x;
    const bool acc = k < K && s_acc[k] != 0;
    const u64 word = __ballot(acc);
    if (lane == 0) s_wave[wave] = __popcll(word);
    __syncthreads();
    int id = __popcll(word & ((1ull << lane) - 1ull));
    for (int s = 0; s < wave; ++s) id += s_wave[s];
    if (k < K) {
        q_seg[k] = acc ? id : -1;
        q_val[k] = acc ? (mode == GSX_QUERIES_LABELS ? slot_label[k] : id) : -1;
        if (slot_segment) slot_segment[k] = acc ? id : -1;
        if (slot_pred) slot_pred[k] = s_pred[k];
    }
}

// ---- composition at the mid resolution: low[r][c] = value of the highest accepted slot whose bit is set, or -1 ------------------------------
// A wave owns one bit word: 64 columns of one row.  It walks the slots downwards and stops once every lane has a hit.
__global__ __launch_bounds__(64 * kQComposeWaves) void queries_compose_kernel(int K, int mid_w, int mid_h, int wpr, const int* __restrict__ q_seg,
                                                                              const int* __restrict__ q_val, const u64* __restrict__ bits,
                                                                              int* __restrict__ low) {
    const int lane = threadIdx.x & 63;
    const long long gw = (long long)blockIdx.x * kQComposeWaves + (threadIdx.x >> 6);
    if (gw >= (long long)mid_h * wpr) return;  // the whole wave
    const int r = (int)(gw / wpr), wc = (int)(gw % wpr);
    const int c = wc * kQCols + lane;
    const bool in = c < mid_w;
    int top = -1;
    bool open = in;
    for (int k = K - 1; k >= 0; --k) {
        if (q_seg[k] < 0) continue;
        const u64 word = bits[((long long)k * mid_h + r) * wpr + wc];
        if (open && ((word >> lane) & 1ull)) top = q_val[k], open = false;
        if (__ballot(open) == 0ull) break;
    }
    if (in) low[(long long)r * mid_w + c] = top;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
int segmap_from_queries(Ctx* c, const void* masks, int dtype, int Q, int h, int w, int K, const int32_t* slot_query, const float* slot_score,
                        const int32_t* slot_label, int mid_w, int mid_h, double threshold, int mode, int out_w, int out_h, int32_t* map,
                        int32_t* slot_segment, float* slot_pred_score) {
    const char* who = "segmap_from_queries";
    if (!masks || !map) return fail(c, GSX_E_INVALID, "%s: masks_dev or map_dev is NULL", who);
    if (K < 0) return fail(c, GSX_E_INVALID, "%s: K must not be negative (got %d)", who, K);
    if (mode != GSX_QUERIES_SEGMENTS && mode != GSX_QUERIES_LABELS) return fail(c, GSX_E_INVALID, "%s: unknown mode %d", who, mode);
    if (K > 0 && (!slot_query || !slot_score || (mode == GSX_QUERIES_LABELS && !slot_label)))
        return fail(c, GSX_E_INVALID, "%s: the slot arrays may be NULL only when K == 0 (slot_label_dev also in segment mode)", who);
    if (Q <= 0 || h <= 0 || w <= 0 || mid_w <= 0 || mid_h <= 0 || out_w <= 0 || out_h <= 0)
        return fail(c, GSX_E_INVALID, "%s: every size must be positive (got Q %d, %d x %d -> %d x %d -> %d x %d)", who, Q, h, w, mid_h, mid_w,
                    out_h, out_w);
    const int eb = seg_elem_bytes(dtype);
    if (!eb) return fail(c, GSX_E_INVALID, "%s: unknown dtype %d", who, dtype);
    if (!std::isfinite(threshold)) return fail(c, GSX_E_INVALID, "%s: the threshold must be finite", who);
    if (seg_misaligned(masks, eb) || seg_misaligned(map, 4) || seg_misaligned(slot_query, 4) || seg_misaligned(slot_score, 4) ||
        seg_misaligned(slot_label, 4) || seg_misaligned(slot_segment, 4) || seg_misaligned(slot_pred_score, 4))
        return fail(c, GSX_E_INVALID, "%s: a pointer is not aligned to its element", who);
    if (K > kQMaxSlots) return fail(c, GSX_E_UNSUPPORTED, "%s: %d slots: at most %d", who, K, kQMaxSlots);
    const long long lim = 1ll << 31;
    const long long wpr = (mid_w + kQCols - 1) / kQCols, rgs = (mid_h + kQRowsWg - 1) / kQRowsWg, row_words = (mid_h + 63) / 64;
    const long long words = (long long)K * mid_h * wpr;
    if ((long long)Q * h * w >= lim || (long long)mid_h * mid_w >= lim || (long long)out_h * out_w >= lim || words >= lim)
        return fail(c, GSX_E_UNSUPPORTED,
                    "%s: Q * h * w, mid_h * mid_w, out_h * out_w and K * mid_h * ceil(mid_w / 64) must stay below 2^31 (Q %d, K %d, %d x %d -> "
                    "%d x %d -> %d x %d)", who, Q, K, h, w, mid_h, mid_w, out_h, out_w);
    GSX_HIP(c, hipSetDevice(c->device));
    const long long G = wpr * rgs;  // workgroups, and partials, per slot
    GSX_HIP(c, c->seg_low.ensure((size_t)mid_h * mid_w * sizeof(int)));
    GSX_HIP(c, c->q_bits.ensure((size_t)words * sizeof(u64)));
    GSX_HIP(c, c->q_parts.ensure((size_t)K * G * sizeof(QPart)));
    const size_t tab_ints = ((size_t)2 * K + 1) & ~(size_t)1;  // the words behind the two tables stay 8-byte aligned
    GSX_HIP(c, c->q_tab.ensure(tab_ints * sizeof(int) + (size_t)(wpr + row_words) * sizeof(u64)));
    int* q_seg = c->q_tab.as<int>();
    int* q_val = q_seg + K;
    u64* samp = reinterpret_cast<u64*>(q_seg + tab_ints);
    if (K > 0) {
        {
            ProfScope ps(c, "queries_sampled");
            hipLaunchKernelGGL(queries_sampled_kernel, dim3((unsigned)(wpr + row_words)), dim3(64), 0, c->stream, mid_w, mid_h, out_w, out_h,
                               (float)mid_w / (float)out_w, (float)mid_h / (float)out_h, (int)wpr, samp);
        }
        GSX_HIP(c, hipGetLastError());
        {
            const dim3 grid((unsigned)G, (unsigned)K);
            const float sx = (float)w / (float)mid_w, sy = (float)h / (float)mid_h;
            ProfScope ps(c, "queries_mask");
#define GSX_Q_MASK(DT)                                                                                                                   \
    hipLaunchKernelGGL((queries_mask_kernel<DT>), grid, dim3(kQBlock), 0, c->stream, masks, Q, h, w, slot_query, mid_w, mid_h, (int)wpr, sx, sy, \
                       samp, c->q_bits.as<u64>(), c->q_parts.as<QPart>())
            switch (dtype) {
                case GSX_F32: GSX_Q_MASK(GSX_F32); break;
                case GSX_F16: GSX_Q_MASK(GSX_F16); break;
                default: GSX_Q_MASK(GSX_BF16); break;
            }
#undef GSX_Q_MASK
        }
        GSX_HIP(c, hipGetLastError());
        {
            ProfScope ps(c, "queries_accept");
            hipLaunchKernelGGL(queries_accept_kernel, dim3(1), dim3(kQMaxSlots), 0, c->stream, K, Q, (int)G, slot_query, slot_score, slot_label,
                               c->q_parts.as<QPart>(), threshold, mode, q_seg, q_val, slot_segment, slot_pred_score);
        }
        GSX_HIP(c, hipGetLastError());
    }
    {
        const long long waves = (long long)mid_h * wpr;
        ProfScope ps(c, "queries_compose");
        hipLaunchKernelGGL(queries_compose_kernel, dim3((unsigned)((waves + kQComposeWaves - 1) / kQComposeWaves)), dim3(64 * kQComposeWaves), 0,
                           c->stream, K, mid_w, mid_h, (int)wpr, q_seg, q_val, c->q_bits.as<u64>(), c->seg_low.as<int>());
    }
    GSX_HIP(c, hipGetLastError());
    seg_launch_resize(c, 1, mid_w, mid_h, out_w, out_h, map, true);
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

void queries_constants(int32_t out[8]) {
    out[0] = kQCols;
    out[1] = kQRowsWg;
    out[2] = kQRowsWave;
    out[3] = kQScanWord;
    out[4] = kQAcceptWaves;
    out[5] = kQMaxSlots;
    out[6] = kQBlock;
    out[7] = 0;
}

}  // namespace gsx
