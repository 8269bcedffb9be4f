// IoU evaluation of 2-D segmentations (the reference's Image_Segmentation/evaluation.py, "ev.py"): mask pairs as a binary GEMM
// over bit planes, label-map pairs as contingency tables, and the "last mask wins" index map of generate_segmentation_map.
// Every sum is an integer, so the atomics below are exact and order-free; the one division of IoU (ev.py:35) happens on the
// host (iou_host.cpp).  A pixel is SET iff value != 0 (ev.py:29-30): the kernels look at the element's bits - any non-zero
// integer; for floats anything but +0.0 and -0.0, i.e. NaN, infinities and denormals are set whatever the float mode is.
#include <algorithm>
#include <cstring>

#include "seg_dtype.hpp"

namespace gsx {

// ---- the units the kernels are built on (gsx_debug_iou_constants hands them to the tests) ----------------------------------------
static constexpr int kIouLoadBytes = 16;                  // one lane's vector load in the pack kernel, for every dtype
static constexpr int kIouWordBits = 64;                   // pixels per plane word
static constexpr int kIouWaveTile = 64 * kIouWordBits;    // pixels per wave of the pack kernel: 64 words, one per lane
static constexpr int kIouPackBlock = 256;
static constexpr int kIouBlockTile = (kIouPackBlock / 64) * kIouWaveTile;  // pixels per workgroup of the pack kernel
static constexpr int kIouPairTile = 16;                   // a workgroup of the pair kernel owns 16 x 16 (mask, gt) pairs ...
static constexpr int kIouPairChunk = 64;                  // ... and walks its slice of the words in chunks of 64 (slice = a multiple)
static constexpr int kIouPairWgs = 512;                   // workgroups the slices are sized for (two per CU)
static constexpr int kIouTableLdsMax = 40000;             // table entries up to which a workgroup keeps a u32 copy in LDS (160 000 B)
static constexpr int kIouTableBlock = 512;
static constexpr int kIouTableRun = 4;                    // consecutive pixels a lane run-length-merges

static constexpr long long kIouPlaneBytesMax = 1ll << 30;
static constexpr int kIouListMax = 65535;

// ---- pack: masks -> bit planes ----------------------------------------------------------------------------------------------------
template <int B>
struct IouWord;
template <>
struct IouWord<1> { using type = uint8_t; };
template <>
struct IouWord<4> { using type = uint32_t; };
template <>
struct IouWord<8> { using type = unsigned long long; };

template <int B, bool F>
__device__ __forceinline__ unsigned iou_set(typename IouWord<B>::type v) {
    if (F) v &= (typename IouWord<B>::type)((~0ull >> 1) >> (64 - 8 * B));  // drop the sign: -0.0 is not set, everything else non-zero is
    return v != 0 ? 1u : 0u;
}

// plane[mask][k] bit i = pixel 64 k + i; the unused bits of the last word are zero.  A wave owns kIouWaveTile pixels: in each of
// 64 / E steps (E = elements per 16 bytes) every lane loads 16 bytes, the 64 / E lanes of a word OR their E-bit pieces together,
// and lane L keeps word L of the tile, so that the wave stores 64 consecutive words at once.  ptrs == NULL: the one mask `single`.
template <int B, bool F>
__global__ __launch_bounds__(kIouPackBlock) void iou_pack_kernel(const void* const* __restrict__ ptrs, const void* single, long long npix,
                                                                 long long nwords, unsigned long long* __restrict__ planes,
                                                                 unsigned long long* __restrict__ areas) {
    using U = typename IouWord<B>::type;
    constexpr int E = kIouLoadBytes / B;  // 16, 4, 2
    constexpr int G = 64 / E;             // lanes per word = steps per tile: 4, 16, 32
    const int mask = blockIdx.y;
    const U* __restrict__ p = reinterpret_cast<const U*>(ptrs ? ptrs[mask] : single);
    const bool vec = (reinterpret_cast<uintptr_t>(p) & (kIouLoadBytes - 1)) == 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile0 = ((long long)blockIdx.x * (kIouPackBlock / 64) + wave) * kIouWaveTile;
    unsigned long long mine = 0;
    if (tile0 < npix) {  // wave-uniform
        for (int s = 0; s < G; ++s) {
            const long long e0 = tile0 + (long long)s * (64 * E) + (long long)lane * E;
            unsigned m = 0;
            if (vec && e0 + E <= npix) {
                const uint4 v = *reinterpret_cast<const uint4*>(p + e0);
                const unsigned w4[4] = {v.x, v.y, v.z, v.w};
                if (B == 1) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) m |= iou_set<1, false>((uint8_t)(w4[j >> 2] >> (8 * (j & 3)))) << j;
                } else if (B == 4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) m |= iou_set<4, F>(w4[j]) << j;
                } else {
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        m |= iou_set<8, F>((unsigned long long)w4[2 * j] | ((unsigned long long)w4[2 * j + 1] << 32)) << j;
                }
            } else {  // a pointer that is aligned to its element only, and the ragged end
#pragma unroll
                for (int j = 0; j < E; ++j)
                    if (e0 + j < npix) m |= iou_set<B, F>(p[e0 + j]) << j;
            }
            unsigned long long w = (unsigned long long)m << ((lane % G) * E);
#pragma unroll
            for (int d = 1; d < G; d <<= 1) w |= __shfl_xor(w, d, 64);
            // every lane of group g = lane / G now holds word s * E + g of the tile; lane L wants word L
            const unsigned long long got = __shfl(w, (lane % E) * G, 64);
            if (lane / E == s) mine = got;
        }
    }
    const long long wi = tile0 / kIouWordBits + lane;
    if (wi < nwords) planes[(long long)mask * nwords + wi] = mine;
    // area = popcount, reduced per workgroup: one atomic per workgroup
    unsigned cnt = (unsigned)__popcll(mine);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_down(cnt, d, 64);
    __shared__ unsigned s_cnt[kIouPackBlock / 64];
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned tot = 0;
#pragma unroll
        for (int i = 0; i < kIouPackBlock / 64; ++i) tot += s_cnt[i];
        if (tot) atomicAdd(&areas[mask], (unsigned long long)tot);
    }
}

// ---- pairs: inter[m][g] = sum_k popc(P[m][k] & Q[g][k]) ---------------------------------------------------------------------------
// A workgroup owns a 16 x 16 tile of pairs and the words [blockIdx.z * slice, + slice).  Thread t = (kg, pg, pm): a 4 x 4 register
// block of pairs (rows 4 pm.., columns 4 pg..) for the words kg, kg + 16, .. of each staged chunk: 8 LDS reads feed 16 popcounts.
__global__ __launch_bounds__(256) void iou_pairs_kernel(const unsigned long long* __restrict__ P, const unsigned long long* __restrict__ Q,
                                                        int nm, int ng, long long nwords, long long slice,
                                                        unsigned long long* __restrict__ inter) {
    __shared__ unsigned long long sp[kIouPairTile][kIouPairChunk + 1], sq[kIouPairTile][kIouPairChunk + 1];
    __shared__ unsigned red[16][kIouPairTile * kIouPairTile];
    const int t = threadIdx.x;
    const int pm = t & 3, pg = (t >> 2) & 3, kg = t >> 4;
    const int m0 = blockIdx.x * kIouPairTile, g0 = blockIdx.y * kIouPairTile;
    const long long k0 = (long long)blockIdx.z * slice;
    const long long k1 = k0 + slice < nwords ? k0 + slice : nwords;
    unsigned acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[i][l] = 0;
    for (long long kc = k0; kc < k1; kc += kIouPairChunk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (t >> 6) + 4 * i, col = t & 63;
            const long long k = kc + col;
            sp[row][col] = (m0 + row < nm && k < k1) ? P[(long long)(m0 + row) * nwords + k] : 0ull;
            sq[row][col] = (g0 + row < ng && k < k1) ? Q[(long long)(g0 + row) * nwords + k] : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kIouPairChunk / 16; ++j) {
            const int k = kg + 16 * j;
            unsigned long long a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = sp[4 * pm + i][k];
                b[i] = sq[4 * pg + i][k];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int l = 0; l < 4; ++l) acc[i][l] += (unsigned)__popcll(a[i] & b[l]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int l = 0; l < 4; ++l) red[kg][(4 * pm + i) * kIouPairTile + 4 * pg + l] = acc[i][l];
    __syncthreads();
    unsigned long long s = 0;  // 32-bit sums inside the slice (< 2^31 pixels), 64 bits on the way out
#pragma unroll
    for (int q = 0; q < 16; ++q) s += red[q][t];
    const int mi = m0 + (t >> 4), gi = g0 + (t & 15);
    if (mi < nm && gi < ng && s) atomicAdd(&inter[(long long)mi * ng + gi], s);  // at most one per pair and workgroup
}

// ---- top index: the highest list index whose mask is set at a pixel, or -1 (ev.py:65-67: the last mask drawn owns the pixel) ------
__global__ __launch_bounds__(256) void iou_top_index_kernel(const unsigned long long* __restrict__ planes, int n, long long nwords,
                                                            long long npix, int* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (i - lane >= npix) return;  // wave-uniform: a wave is one plane word
    const long long wi = i >> 6;
    const bool in = i < npix;
    int best = -1;
    for (int m = n - 1; m >= 0; --m) {
        const unsigned long long wd = planes[(long long)m * nwords + wi];
        if (best < 0 && ((wd >> lane) & 1ull)) best = m;
        if (__ballot(in && best < 0) == 0ull) break;
    }
    if (in) out[i] = best;
}

// ---- table: contingency table of two label maps (the maps are read through seg_dtype.hpp's seg_bins4) -------------------------------
// the lanes that hold the first active lane's (key, count) add once, with count x the popcount of their ballot (the device of
// normals.hip's radix-select histogram); two rounds, then whoever is left adds on its own
template <bool LDS>
__device__ __forceinline__ void iou_table_add(bool act, unsigned packed, int lane, unsigned* ltab, unsigned long long* gtab) {
    unsigned long long pend = __ballot(act);
#pragma unroll 1
    for (int r = 0; r < 2 && pend; ++r) {
        const int first = __ffsll((long long)pend) - 1;
        const unsigned p0 = (unsigned)__shfl((int)packed, first, 64);
        const unsigned long long same = __ballot(act && packed == p0);
        if (lane == first) {
            const unsigned add = (unsigned)__popcll(same) * (p0 & 7u);
            if (LDS) atomicAdd(&ltab[p0 >> 3], add);
            else atomicAdd(&gtab[p0 >> 3], (unsigned long long)add);
        }
        if (packed == p0) act = false;
        pend &= ~same;
    }
    if (act) {
        if (LDS) atomicAdd(&ltab[packed >> 3], packed & 7u);
        else atomicAdd(&gtab[packed >> 3], (unsigned long long)(packed & 7u));
    }
}

// table[pair0 + blockIdx.y][a][b] += pixels with pred bin a and gt bin b; a pixel with a bin out of range is left out and its flat
// index goes into err[pair] by atomicMin (the call then fails: the table is not handed out).  LDS: a u32 table per workgroup
// (a workgroup sees < 2^31 pixels), flushed with one 64-bit atomic per non-zero entry; otherwise straight onto the u64 table.
template <int DP, int DG, bool LDS>
__global__ __launch_bounds__(kIouTableBlock) void iou_table_kernel(const void* const* __restrict__ preds, const void* const* __restrict__ gts,
                                                                   int pair0, long long npix, int np1, int ng1,
                                                                   unsigned long long* __restrict__ table, unsigned* __restrict__ err) {
    extern __shared__ unsigned iou_ltab[];
    const int t = threadIdx.x, lane = t & 63;
    const int entries = np1 * ng1;
    const void* pp = preds[blockIdx.y];
    const void* pg = gts[blockIdx.y];
    unsigned long long* gtab = table + (long long)(pair0 + blockIdx.y) * entries;
    if (LDS) {
        for (int i = t; i < entries; i += kIouTableBlock) iou_ltab[i] = 0;
        __syncthreads();
    }
    const long long nquads = (npix + kIouTableRun - 1) / kIouTableRun;
    const long long nquads_pad = (nquads + 63) / 64 * 64;  // whole waves stay in the loop together: the ballots need every lane
    unsigned bad = 0xffffffffu;
    for (long long q = (long long)blockIdx.x * kIouTableBlock + t; q < nquads_pad; q += (long long)gridDim.x * kIouTableBlock) {
        const long long i0 = q * kIouTableRun;
        unsigned long long a[4], b[4];
        if (i0 < npix) {
            seg_bins4<DP>(pp, i0, npix, a);
            seg_bins4<DG>(pg, i0, npix, b);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = b[j] = ~0ull;
        }
        unsigned key[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = i0 + j < npix;
            const bool ok = in && a[j] < (unsigned long long)np1 && b[j] < (unsigned long long)ng1;
            key[j] = ok ? (unsigned)a[j] * (unsigned)ng1 + (unsigned)b[j] : 0xffffffffu;
            if (in && !ok) bad = min(bad, (unsigned)(i0 + j));
        }
        // run lengths: cnt[j] = pixels of the run that starts at j (an invalid pixel ends a run and starts none)
        unsigned cnt[4];
        cnt[3] = 1;
#pragma unroll
        for (int j = 2; j >= 0; --j) cnt[j] = 1 + (key[j + 1] == key[j] ? cnt[j + 1] : 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool start = key[j] != 0xffffffffu && (j == 0 || key[j] != key[j - 1]);
            iou_table_add<LDS>(start, (key[j] << 3) | cnt[j], lane, iou_ltab, gtab);
        }
    }
    if (bad != 0xffffffffu) atomicMin(&err[pair0 + blockIdx.y], bad);
    if (LDS) {
        __syncthreads();
        for (int i = t; i < entries; i += kIouTableBlock) {
            const unsigned v = iou_ltab[i];
            if (v) atomicAdd(&gtab[i], (unsigned long long)v);
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static int iou_elem_bytes(int mask_dtype) {
    switch (mask_dtype) {
        case GSX_MASK_U8: return 1;
        case GSX_MASK_I32: case GSX_MASK_F32: return 4;
        case GSX_MASK_I64: case GSX_MASK_F64: return 8;
    }
    return 0;
}

// the pinned staging pair and the two raw device buffers behind it: room for `bytes` per slot
static int iou_stage_reserve(Ctx* c, size_t bytes) {
    for (int s = 0; s < 2; ++s) {
        if (c->iou_pin[s].p && c->iou_pin[s].cap < bytes) GSX_HIP(c, hipStreamSynchronize(c->stream));  // a copy may still read the old block
        GSX_HIP(c, c->iou_pin[s].ensure(bytes));
        c->iou_ev[s].pending = false;  // (every call ends with a stream synchronise: the previous call's copies are done)
        GSX_HIP(c, c->iou_raw[s].ensure(bytes));
    }
    return GSX_OK;
}

// host arrays a (and b, at byte off_b) -> pinned slot -> raw device slot, queued on the ctx stream
static int iou_stage(Ctx* c, int slot, const void* a, size_t na, const void* b, size_t nb, size_t off_b) {
    GSX_HIP(c, c->iou_ev[slot].wait());  // the slot's previous copy has to have left the pinned buffer
    char* pin = c->iou_pin[slot].as<char>();
    std::memcpy(pin, a, na);
    size_t total = na;
    if (b) {
        std::memcpy(pin + off_b, b, nb);
        total = off_b + nb;
    }
    GSX_HIP(c, hipMemcpyAsync(c->iou_raw[slot].p, pin, total, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, c->iou_ev[slot].record(c->stream));
    return GSX_OK;
}

static void iou_launch_pack(Ctx* c, int dtype, const void* const* ptrs_dev, const void* single, int count, long long npix, long long nwords,
                            unsigned long long* planes, unsigned long long* areas) {
    const dim3 grid((unsigned)((npix + kIouBlockTile - 1) / kIouBlockTile), (unsigned)count);
    ProfScope ps(c, "iou_pack");
#define GSX_IOU_PACK(B, F) \
    hipLaunchKernelGGL((iou_pack_kernel<B, F>), grid, dim3(kIouPackBlock), 0, c->stream, ptrs_dev, single, npix, nwords, planes, areas)
    switch (dtype) {
        case GSX_MASK_U8: GSX_IOU_PACK(1, false); break;
        case GSX_MASK_I32: GSX_IOU_PACK(4, false); break;
        case GSX_MASK_I64: GSX_IOU_PACK(8, false); break;
        case GSX_MASK_F32: GSX_IOU_PACK(4, true); break;
        default: GSX_IOU_PACK(8, true); break;
    }
#undef GSX_IOU_PACK
}

// one list of masks -> planes[first .. first + n) and areas[first ..)
static int iou_pack_list(Ctx* c, bool device, int n, const void* const* list, int dtype, long long npix, long long nwords,
                         unsigned long long* planes, unsigned long long* areas, const void* const* ptrs_dev) {
    if (device) {
        iou_launch_pack(c, dtype, ptrs_dev, nullptr, n, npix, nwords, planes, areas);
        GSX_HIP(c, hipGetLastError());
        return GSX_OK;
    }
    const size_t bytes = (size_t)npix * iou_elem_bytes(dtype);
    for (int i = 0; i < n; ++i) {  // one raw mask at a time: copied up through the pinned pair, packed behind its copy
        const int slot = c->iou_slot;
        c->iou_slot ^= 1;
        const int rc = iou_stage(c, slot, list[i], bytes, nullptr, 0, 0);
        if (rc) return rc;
        iou_launch_pack(c, dtype, nullptr, c->iou_raw[slot].p, 1, npix, nwords, planes + (long long)i * nwords, areas + i);
        GSX_HIP(c, hipGetLastError());
    }
    return GSX_OK;
}

// the arguments of one list that can be judged without reading the list ...
static int iou_check_list(Ctx* c, const char* who, const char* what, int n, const void* const* list, int dtype) {
    if (n <= 0) return fail(c, GSX_E_INVALID, "%s: the number of %s must be positive (got %d)", who, what, n);
    if (!list) return fail(c, GSX_E_INVALID, "%s: the %s array is NULL", who, what);
    if (!iou_elem_bytes(dtype)) return fail(c, GSX_E_INVALID, "%s: unknown dtype %d of the %s", who, dtype, what);
    return GSX_OK;
}
// ... and its entries (once n is known to be a sane count)
static int iou_check_entries(Ctx* c, const char* who, const char* what, int n, const void* const* list, int dtype, bool device) {
    const int eb = iou_elem_bytes(dtype);
    for (int i = 0; i < n; ++i) {
        if (!list[i]) return fail(c, GSX_E_INVALID, "%s: %s[%d] is NULL", who, what, i);
        if (device && (reinterpret_cast<uintptr_t>(list[i]) & (uintptr_t)(eb - 1)))
            return fail(c, GSX_E_INVALID, "%s: %s[%d] is not aligned to its %d-byte element", who, what, i, eb);
    }
    return GSX_OK;
}

int iou_masks(Ctx* c, bool device, int n_masks, const void* const* masks, int mask_dtype, int n_gt, const void* const* gts, int gt_dtype,
              int h, int w, int64_t* inter_out, int64_t* area_masks_out, int64_t* area_gt_out, double* iou_out) {
    const char* who = device ? "iou_masks_device" : "iou_masks";
    if (h <= 0 || w <= 0) return fail(c, GSX_E_INVALID, "%s: h and w must be positive (got %d x %d)", who, h, w);
    int rc = iou_check_list(c, who, "masks", n_masks, masks, mask_dtype);
    if (rc) return rc;
    rc = iou_check_list(c, who, "ground truths", n_gt, gts, gt_dtype);
    if (rc) return rc;
    const long long npix = (long long)h * w;
    if (npix >= (1ll << 31)) return fail(c, GSX_E_UNSUPPORTED, "%s: %d x %d pixels: h * w must stay below 2^31", who, h, w);
    if (n_masks > kIouListMax || n_gt > kIouListMax)
        return fail(c, GSX_E_UNSUPPORTED, "%s: %d masks x %d ground truths: at most %d of either", who, n_masks, n_gt, kIouListMax);
    rc = iou_check_entries(c, who, "masks", n_masks, masks, mask_dtype, device);
    if (rc) return rc;
    rc = iou_check_entries(c, who, "ground truths", n_gt, gts, gt_dtype, device);
    if (rc) return rc;
    const long long nwords = (npix + kIouWordBits - 1) / kIouWordBits;
    const long long nlist = (long long)n_masks + n_gt;
    if (nlist * nwords * 8 > kIouPlaneBytesMax)
        return fail(c, GSX_E_UNSUPPORTED, "%s: %lld bit planes of %lld bytes exceed 1 GiB", who, nlist, nwords * 8);
    GSX_HIP(c, hipSetDevice(c->device));
    const long long ncnt = nlist + (long long)n_masks * n_gt;
    GSX_HIP(c, c->iou_planes.ensure((size_t)(nlist * nwords * 8)));
    GSX_HIP(c, c->iou_cnt.ensure((size_t)ncnt * 8));
    unsigned long long* planes = c->iou_planes.as<unsigned long long>();
    unsigned long long* cnt = c->iou_cnt.as<unsigned long long>();  // areas of the masks, of the ground truths, then inter[m][g]
    const void* const* ptrs_dev = nullptr;
    std::vector<const void*> ptrs;
    if (device) {
        GSX_HIP(c, c->iou_ptrs.ensure((size_t)nlist * sizeof(void*)));
        ptrs.assign(masks, masks + n_masks);
        ptrs.insert(ptrs.end(), gts, gts + n_gt);
        GSX_HIP(c, hipMemcpyAsync(c->iou_ptrs.p, ptrs.data(), (size_t)nlist * sizeof(void*), hipMemcpyHostToDevice, c->stream));
        ptrs_dev = c->iou_ptrs.as<const void*>();
    } else {
        const size_t raw = (size_t)npix * std::max(iou_elem_bytes(mask_dtype), iou_elem_bytes(gt_dtype));
        rc = iou_stage_reserve(c, raw);
        if (rc) return rc;
    }
    GSX_HIP(c, hipMemsetAsync(cnt, 0, (size_t)ncnt * 8, c->stream));
    rc = iou_pack_list(c, device, n_masks, masks, mask_dtype, npix, nwords, planes, cnt, ptrs_dev);
    if (rc) return rc;
    rc = iou_pack_list(c, device, n_gt, gts, gt_dtype, npix, nwords, planes + (long long)n_masks * nwords, cnt + n_masks,
                       ptrs_dev ? ptrs_dev + n_masks : nullptr);
    if (rc) return rc;
    {
        const int tm = (n_masks + kIouPairTile - 1) / kIouPairTile, tg = (n_gt + kIouPairTile - 1) / kIouPairTile;
        const long long chunks = (nwords + kIouPairChunk - 1) / kIouPairChunk;
        long long ns = (kIouPairWgs + (long long)tm * tg - 1) / ((long long)tm * tg);  // slices that fill the chip with this many tiles
        ns = std::max(1ll, std::min(ns, chunks));
        const long long slice = (chunks + ns - 1) / ns * kIouPairChunk;
        ns = (nwords + slice - 1) / slice;
        ProfScope ps(c, "iou_pairs");
        hipLaunchKernelGGL(iou_pairs_kernel, dim3((unsigned)tm, (unsigned)tg, (unsigned)ns), dim3(256), 0, c->stream, planes,
                           planes + (long long)n_masks * nwords, n_masks, n_gt, nwords, slice, cnt + nlist);
    }
    GSX_HIP(c, hipGetLastError());
    std::vector<int64_t> host((size_t)ncnt);
    GSX_HIP(c, hipMemcpyAsync(host.data(), cnt, (size_t)ncnt * 8, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    const int64_t* am = host.data();
    const int64_t* ag = host.data() + n_masks;
    const int64_t* in = host.data() + nlist;
    if (area_masks_out) std::memcpy(area_masks_out, am, sizeof(int64_t) * n_masks);
    if (area_gt_out) std::memcpy(area_gt_out, ag, sizeof(int64_t) * n_gt);
    if (inter_out) std::memcpy(inter_out, in, sizeof(int64_t) * (size_t)n_masks * n_gt);
    if (iou_out) {
        std::vector<int64_t> row((size_t)n_gt);
        for (int m = 0; m < n_masks; ++m) {
            std::fill(row.begin(), row.end(), am[m]);
            gsx_iou_from_counts(n_gt, in + (size_t)m * n_gt, row.data(), ag, iou_out + (size_t)m * n_gt);
        }
    }
    return GSX_OK;
}

int masks_top_index(Ctx* c, int n_masks, const void* const* masks, int mask_dtype, int h, int w, int32_t* index_out) {
    const char* who = "masks_top_index";
    if (h <= 0 || w <= 0) return fail(c, GSX_E_INVALID, "%s: h and w must be positive (got %d x %d)", who, h, w);
    if (!index_out) return fail(c, GSX_E_INVALID, "%s: index_out is NULL", who);
    int rc = iou_check_list(c, who, "masks", n_masks, masks, mask_dtype);
    if (rc) return rc;
    const long long npix = (long long)h * w;
    if (npix >= (1ll << 31)) return fail(c, GSX_E_UNSUPPORTED, "%s: %d x %d pixels: h * w must stay below 2^31", who, h, w);
    if (n_masks > kIouListMax) return fail(c, GSX_E_UNSUPPORTED, "%s: %d masks: at most %d", who, n_masks, kIouListMax);
    rc = iou_check_entries(c, who, "masks", n_masks, masks, mask_dtype, false);
    if (rc) return rc;
    const long long nwords = (npix + kIouWordBits - 1) / kIouWordBits;
    if ((long long)n_masks * nwords * 8 > kIouPlaneBytesMax)
        return fail(c, GSX_E_UNSUPPORTED, "%s: %d bit planes of %lld bytes exceed 1 GiB", who, n_masks, nwords * 8);
    GSX_HIP(c, hipSetDevice(c->device));
    GSX_HIP(c, c->iou_planes.ensure((size_t)n_masks * nwords * 8));
    GSX_HIP(c, c->iou_cnt.ensure((size_t)n_masks * 8));
    GSX_HIP(c, c->iou_top.ensure((size_t)npix * sizeof(int)));
    rc = iou_stage_reserve(c, (size_t)npix * iou_elem_bytes(mask_dtype));
    if (rc) return rc;
    GSX_HIP(c, hipMemsetAsync(c->iou_cnt.p, 0, (size_t)n_masks * 8, c->stream));
    rc = iou_pack_list(c, false, n_masks, masks, mask_dtype, npix, nwords, c->iou_planes.as<unsigned long long>(),
                       c->iou_cnt.as<unsigned long long>(), nullptr);
    if (rc) return rc;
    {
        ProfScope ps(c, "iou_top_index");
        hipLaunchKernelGGL(iou_top_index_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, c->stream,
                           c->iou_planes.as<unsigned long long>(), n_masks, nwords, npix, c->iou_top.as<int>());
    }
    GSX_HIP(c, hipGetLastError());
    GSX_HIP(c, hipMemcpyAsync(index_out, c->iou_top.p, (size_t)npix * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

template <int DP, int DG>
static int iou_launch_table2(Ctx* c, bool lds, dim3 grid, size_t lds_bytes, const void* const* preds, const void* const* gts, int pair0,
                             long long npix, int np1, int ng1, unsigned long long* table, unsigned* err) {
    if (lds) {
        if (lds_bytes > 64 * 1024)
            GSX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(iou_table_kernel<DP, DG, true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        hipLaunchKernelGGL((iou_table_kernel<DP, DG, true>), grid, dim3(kIouTableBlock), lds_bytes, c->stream, preds, gts, pair0, npix, np1,
                           ng1, table, err);
    } else {
        hipLaunchKernelGGL((iou_table_kernel<DP, DG, false>), grid, dim3(kIouTableBlock), 0, c->stream, preds, gts, pair0, npix, np1, ng1,
                           table, err);
    }
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

static int iou_launch_table(Ctx* c, int pdt, int gdt, bool lds, int pairs, const void* const* preds, const void* const* gts, int pair0,
                            long long npix, int np1, int ng1, unsigned long long* table, unsigned* err) {
    const long long nquads = (npix + kIouTableRun - 1) / kIouTableRun;
    long long gx = (nquads + kIouTableBlock - 1) / kIouTableBlock;
    gx = std::max(1ll, std::min(gx, (long long)std::max(1, 512 / pairs)));  // two workgroups per CU over all pairs of the launch
    const dim3 grid((unsigned)gx, (unsigned)pairs);
    const size_t lds_bytes = lds ? sizeof(unsigned) * (size_t)np1 * ng1 : 0;
    ProfScope ps(c, "iou_table");
    return with_seg_dtype(pdt, [&](auto dp) {
        return with_seg_dtype(gdt, [&](auto dg) {
            return iou_launch_table2<decltype(dp)::value, decltype(dg)::value>(c, lds, grid, lds_bytes, preds, gts, pair0, npix, np1, ng1, table,
                                                                               err);
        });
    });
}

int iou_label_maps(Ctx* c, bool device, int n_pairs, const void* const* pred, int pred_dtype, int n_pred_classes, const void* const* gt,
                   int gt_dtype, int n_gt_classes, int h, int w, int64_t* table_out) {
    const char* who = device ? "iou_label_maps_device" : "iou_label_maps";
    if (h <= 0 || w <= 0) return fail(c, GSX_E_INVALID, "%s: h and w must be positive (got %d x %d)", who, h, w);
    if (n_pairs <= 0) return fail(c, GSX_E_INVALID, "%s: n_pairs must be positive (got %d)", who, n_pairs);
    if (!pred || !gt || !table_out) return fail(c, GSX_E_INVALID, "%s: NULL argument", who);
    if (!seg_dtype_known(pred_dtype) || !seg_dtype_known(gt_dtype))
        return fail(c, GSX_E_INVALID, "%s: unknown seg dtype (%d, %d)", who, pred_dtype, gt_dtype);
    const int pb = (int)seg_elem_size(pred_dtype), gb = (int)seg_elem_size(gt_dtype);
    if (n_pred_classes < 1 || n_pred_classes > 255 || n_gt_classes < 1 || n_gt_classes > 255)
        return fail(c, GSX_E_INVALID, "%s: class counts must lie in [1, 255] (got %d, %d)", who, n_pred_classes, n_gt_classes);
    const long long npix = (long long)h * w;
    if (npix >= (1ll << 31)) return fail(c, GSX_E_UNSUPPORTED, "%s: %d x %d pixels: h * w must stay below 2^31", who, h, w);
    const int np1 = n_pred_classes + 1, ng1 = n_gt_classes + 1;
    const long long entries = (long long)np1 * ng1;
    if (n_pairs > kIouListMax || (long long)n_pairs * entries * 8 > kIouPlaneBytesMax)
        return fail(c, GSX_E_UNSUPPORTED, "%s: %d pairs of %lld table entries: at most %d pairs and 1 GiB of tables", who, n_pairs, entries,
                    kIouListMax);
    for (int i = 0; i < n_pairs; ++i) {
        if (!pred[i] || !gt[i]) return fail(c, GSX_E_INVALID, "%s: a map of pair %d is NULL", who, i);
        if (device && (seg_misaligned(pred[i], pb) || seg_misaligned(gt[i], gb)))
            return fail(c, GSX_E_INVALID, "%s: a map of pair %d is not aligned to its element", who, i);
    }
    GSX_HIP(c, hipSetDevice(c->device));
    const bool lds = c->opt_iou_table_lds && entries <= kIouTableLdsMax;
    const size_t tbytes = (size_t)n_pairs * entries * 8, ebytes = (size_t)n_pairs * sizeof(unsigned);
    GSX_HIP(c, c->iou_table.ensure(tbytes + ebytes));
    unsigned long long* table = c->iou_table.as<unsigned long long>();
    unsigned* err = reinterpret_cast<unsigned*>(c->iou_table.as<char>() + tbytes);
    GSX_HIP(c, hipMemsetAsync(table, 0, tbytes, c->stream));
    GSX_HIP(c, hipMemsetAsync(err, 0xff, ebytes, c->stream));
    std::vector<const void*> ptrs;
    int rc;
    if (device) {
        GSX_HIP(c, c->iou_ptrs.ensure((size_t)2 * n_pairs * sizeof(void*)));
        ptrs.assign(pred, pred + n_pairs);
        ptrs.insert(ptrs.end(), gt, gt + n_pairs);
        GSX_HIP(c, hipMemcpyAsync(c->iou_ptrs.p, ptrs.data(), ptrs.size() * sizeof(void*), hipMemcpyHostToDevice, c->stream));
        rc = iou_launch_table(c, pred_dtype, gt_dtype, lds, n_pairs, c->iou_ptrs.as<const void*>(), c->iou_ptrs.as<const void*>() + n_pairs, 0,
                              npix, np1, ng1, table, err);
        if (rc) return rc;
    } else {
        // a pair's two maps share a slot of the pinned pair: pred at 0, gt at the next multiple of 16 bytes
        const size_t nb_p = (size_t)npix * pb, nb_g = (size_t)npix * gb, off_g = (nb_p + 15) / 16 * 16;
        rc = iou_stage_reserve(c, off_g + nb_g);
        if (rc) return rc;
        GSX_HIP(c, c->iou_ptrs.ensure(4 * sizeof(void*)));
        ptrs = {c->iou_raw[0].p, c->iou_raw[1].p, c->iou_raw[0].as<char>() + off_g, c->iou_raw[1].as<char>() + off_g};
        GSX_HIP(c, hipMemcpyAsync(c->iou_ptrs.p, ptrs.data(), 4 * sizeof(void*), hipMemcpyHostToDevice, c->stream));
        for (int i = 0; i < n_pairs; ++i) {
            const int slot = c->iou_slot;
            c->iou_slot ^= 1;
            rc = iou_stage(c, slot, pred[i], nb_p, gt[i], nb_g, off_g);
            if (rc) return rc;
            rc = iou_launch_table(c, pred_dtype, gt_dtype, lds, 1, c->iou_ptrs.as<const void*>() + slot, c->iou_ptrs.as<const void*>() + 2 + slot,
                                  i, npix, np1, ng1, table, err);
            if (rc) return rc;
        }
    }
    std::vector<unsigned> herr((size_t)n_pairs);
    GSX_HIP(c, hipMemcpyAsync(herr.data(), err, ebytes, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n_pairs; ++i)
        if (herr[i] != 0xffffffffu)
            return fail(c, GSX_E_RANGE, "%s: pair %d: the label at flat index %u (row %u, column %u) is outside [-1, %d] (pred) / [-1, %d] (gt)",
                        who, i, herr[i], herr[i] / (unsigned)w, herr[i] % (unsigned)w, n_pred_classes - 1, n_gt_classes - 1);
    GSX_HIP(c, hipMemcpy(table_out, table, tbytes, hipMemcpyDeviceToHost));
    return GSX_OK;
}

void iou_constants(int32_t out[8]) {
    out[0] = kIouLoadBytes;
    out[1] = kIouWordBits;
    out[2] = kIouWaveTile;
    out[3] = kIouBlockTile;
    out[4] = kIouPairTile;
    out[5] = kIouPairChunk;
    out[6] = kIouTableLdsMax;
    out[7] = kIouTableRun;
}

}  // namespace gsx
