// vote.hip — majority-vote labeler kernels for gfx950 (MI355X) and their host drivers.
//
// Replaces the double loop of assign_labels (deep_learning_segmentation.py:255-295) and its arg-max
// (:297-308); project() (vote_device.hpp) restates project_gaussian (:43-82) operation for operation in fp64.
// This translation unit MUST be compiled with -ffp-contract=off: every fma below is explicit and
// every other product/sum must round separately, exactly as the reference's Python floats do.
// How the segmentation maps get into the seg pool: handover.hip.
//
// Data layout in HBM
//   positions      SoA  x[n], y[n], z[n] f32                      (coalesced 4 B/lane loads)
//   views          ViewDesc[V], 256 B each (176 hot), wave-uniform -> four scalar loads, operands live in SGPRs
//   seg pool       u8 maps, value = label+1 (bin index), in strips of 16 pixel columns (handover.hip); 1 B gathers
//   planes        cnt[slab][bins][sn], fv[slab][bins][sn]  u8 or u16 (16 bit only for the all-reduce
//                  protocol with > 255 views in total): bin-major so that a wave's 64 Gaussians touch 64
//                  consecutive elements of a row; slab = one rank's share in the all-to-all protocols
//                  (a single slab is plain [bins][n_pad])
//   keys, labels   int32[n_pad]; cand u32[8][sn]; codes u16[n_pad] (exchange protocol v3)
//
// Kernels
//   vote_fused_labels_kernel   single GPU: all staged views in one launch, labels straight out
//   vote_fused_planes_kernel   multi-GPU v1/v2 (and > 255 views): count + first-view planes
//   vote_fused_counts_kernel   multi-GPU v3: count plane only; vote_slab_totals / vote_tie / vote_tie_resolve
//   vote_keys / vote_labels / vote_slab_reduce / unpermute_labels   the rank-local ends of the protocols
//
// Kernel design (Gaussian-major, all staged views in one launch)
//   one thread = one Gaussian; it walks the views in REVERSE order and keeps its private vote
//   histogram in LDS (row stride an odd number of dwords: a wave that votes one label hits 32
//   different banks).  Reverse order makes the reference's tie rule an online rule: a label that
//   reaches a count >= the best count so far takes over; the label whose FIRST vote (in forward
//   order) is earliest among the max-count labels is the last one to do so.  See DESIGN.md §3.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "gsx_ctx.hpp"
#include "vote_device.hpp"

namespace gsx {

template <int DIV>
__global__ __launch_bounds__(kBlock) void project_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ z, long long n,
                                                         const ViewDesc* __restrict__ vd,
                                                         const uint32_t* __restrict__ perm, int* __restrict__ ox,
                                                         int* __restrict__ oy, float filt_h) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i < n;  // (no early return: the flat forms ballot over the whole wave)
    int xi, yi;
    const ViewRegs vr = load_view(vd);
    const double X = valid ? (double)x[i] : __builtin_nan(""), Y = valid ? (double)y[i] : 0.0, Z = valid ? (double)z[i] : 0.0;
    const bool vis = DIV == kDivFiltCoarse ? project_filtered(vr, filt_h, X, Y, Z, xi, yi) : project<DIV>(vr, X, Y, Z, xi, yi);
    if (!valid) return;
    const long long o = perm ? (long long)perm[i] : i;  // back to the caller's order
    ox[o] = vis ? xi : -1;
    oy[o] = vis ? yi : -1;
}

// -------------------------------------------------------------------------------------------------
// fused vote, single GPU / single batch: labels straight out of the kernel
// -------------------------------------------------------------------------------------------------
struct FusedParams {
    const float* x;
    const float* y;
    const float* z;
    long long n;
    const ViewDesc* views;  // the batch's views
    int nviews;             // <= kMaxBatch
    const uint8_t* pool;
    int bins;
    int stride_dw;         // LDS row stride in dwords (odd)
    int xcd_swizzle;       // see logical_block()
    const uint32_t* perm;  // sorted slot -> caller's index, or nullptr
    const double* cull;    // culling planes of the batch's views, [25][cull_pitch] (nullptr: no culling)
    int cull_pitch;
    unsigned long long* cull_tally;  // [0] += (wave, view) pairs skipped
    float filt_h;                    // kDivFiltCoarse: 0.5 - E of project_filtered() for the largest frame among the staged views
};

static inline int odd_dwords(int bytes) {
    int dw = (bytes + 3) / 4;
    return dw | 1;
}
// 0.5 - E of project_filtered() for the staged views (E grows with the frame: the largest one decides)
static float filter_half_width(const Ctx* c) {
    int dim = 64;
    for (const ViewDesc& v : c->run.views) dim = std::max(dim, std::max(v.cam_w, v.cam_h));
    return (float)(0.5 - kFilterK * (double)dim * 5.9604644775390625e-08);
}
// The parameters of a walk over ALL staged views of the whole scene (host side; call after sync_views()).  Every launch starts
// from these and overrides what differs: the views and culling planes of a batch, the Gaussians of a range.
static FusedParams fused_params(Ctx* c, int stride_bytes_per_bin) {
    FusedParams p{};
    p.x = c->x.as<float>();
    p.y = c->y.as<float>();
    p.z = c->z.as<float>();
    p.n = c->n;
    p.views = c->run.d_views.as<ViewDesc>();
    p.nviews = (int)c->run.views.size();
    p.pool = c->run.segpool.as<uint8_t>();
    p.bins = c->run.bins;
    p.xcd_swizzle = c->vopt.xcd_swizzle;
    p.perm = c->sorted ? c->perm.as<uint32_t>() : nullptr;
    p.stride_dw = odd_dwords(c->run.bins * stride_bytes_per_bin);
    p.cull = c->vopt.wave_cull ? c->run.d_cull.as<double>() : nullptr;
    p.cull_pitch = c->run.cull_pitch;
    p.cull_tally = c->run.d_cull_tally.as<unsigned long long>();
    p.filt_h = filter_half_width(c);
    return p;
}

// ---- wave-level view culling ------------------------------------------------------------------------------------
// 40 % of the (Gaussian, view) pairs of an ordinary capture are invisible, and in Morton order they come in whole
// waves.  Each wave bounds its 64 Gaussians by a sphere (c, r) once; then LANE l tests view l against the five
// world-space planes the host derived from that view's frustum (gsx::cull_planes): a plane is stored as a unit normal
// A, an offset B and a margin slope M, and `A.c + B > r + M (|c|_1 + r)` proves that every point of the sphere fails the reference's visibility test (dls.py:72, :80) by more than a million times the rounding error of
// the fp64 projection.  One ballot turns 64 such tests into a 64-bit mask; a culled view costs two scalar
// instructions instead of ~50 fp64 ones, and no descriptor load.  Bits are indexed by the REVERSE view index
// (nviews-1-v), so that the U views of a chunk are U adjacent bits.  Pairs that are not provably invisible take
// the exact path as before: the result is unchanged, bit for bit.
static constexpr int kCullPlanes = 5;
static constexpr unsigned kTallySlots = 1024, kTallyStride = 16;  // u64 counters, one per 128-B line
struct CullMasks {
    unsigned long long m[4];  // kMaxBatch <= 256 views
};

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// X is NaN on lanes past the end of the scene: fmin / fmax ignore them (and NaN positions, which never vote).
__device__ __forceinline__ CullMasks wave_cull_masks(const double* __restrict__ cull, int pitch, int nviews, double X,
                                                     double Y, double Z, unsigned long long* __restrict__ tally) {
    CullMasks k;
    k.m[0] = k.m[1] = k.m[2] = k.m[3] = 0;
    if (!cull) return k;  // wave-uniform
    const double big = 1.7e308;
    const double lx = wave_min(X == X ? X : big), hx = wave_max(X == X ? X : -big);
    const double ly = wave_min(X == X ? Y : big), hy = wave_max(X == X ? Y : -big);
    const double lz = wave_min(X == X ? Z : big), hz = wave_max(X == X ? Z : -big);
    const double cx = 0.5 * lx + 0.5 * hx, cy = 0.5 * ly + 0.5 * hy, cz = 0.5 * lz + 0.5 * hz;
    const double dx = X - cx, dy = Y - cy, dz = Z - cz;
    // r >= the distance of every member from c; the factor covers the rounding of the distance itself.
    // An infinite coordinate makes c or r non-finite and every test below false: such a wave is never culled.
    const double r = wave_max(sqrt(dx * dx + dy * dy + dz * dz)) * (1.0 + 1e-12);
    const double reach = fabs(cx) + fabs(cy) + fabs(cz) + r;  // >= |p| for every member: scales the rounding margin
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (64 * j < nviews) {  // wave-uniform
            const int ri = 64 * j + lane;  // reverse view index
            bool out = false;
            if (ri < nviews) {
                const double* q = cull + (nviews - 1 - ri);
#pragma unroll
                for (int pl = 0; pl < kCullPlanes; ++pl) {
                    const double a0 = q[(5 * pl + 0) * pitch], a1 = q[(5 * pl + 1) * pitch], a2 = q[(5 * pl + 2) * pitch];
                    const double b = q[(5 * pl + 3) * pitch], m = q[(5 * pl + 4) * pitch];
                    out = out | (a0 * cx + a1 * cy + a2 * cz + b > r + m * reach);
                }
            }
            k.m[j] = __builtin_amdgcn_ballot_w64(out);
        }
    }
    if (tally && lane == 0) {  // statistics for gsx_vote_culled(): one atomic per wave, spread over kTallySlots cache lines -
                               // 47 k atomics on ONE address keep an L2 channel busy for ~0.4 ms, longer than a short kernel runs
        const unsigned slot = (blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kTallySlots - 1);
        atomicAdd(tally + slot * kTallyStride, (unsigned long long)(__popcll(k.m[0]) + __popcll(k.m[1]) + __popcll(k.m[2]) + __popcll(k.m[3])));
    }
    return k;
}

// the U bits of the chunk that starts `done` views into the (reverse) walk; 64 % U == 0, so they share a word
template <int U>
__device__ __forceinline__ unsigned cull_bits(const CullMasks& k, int done) {
    const int w = done >> 6;
    const unsigned long long word = w == 0 ? k.m[0] : w == 1 ? k.m[1] : w == 2 ? k.m[2] : k.m[3];
    return (unsigned)(word >> (done & 63)) & ((1u << U) - 1u);
}

// One chunk of U views (vb-1, vb-2, ..): bin[u] = the vote of this lane's Gaussian in view vb-1-u, or -1.
// FULL: all U views exist (no index test).  culled: bit u set = the whole wave provably misses view vb-1-u.
typedef const __attribute__((address_space(1))) uint8_t* global_u8_ptr;

template <int U, int DIV, bool FULL>
__device__ __forceinline__ void gather_chunk(const ViewDesc* __restrict__ views, const uint8_t* __restrict__ pool, int vb,
                                             double X, double Y, double Z, unsigned culled, int (&bin)[U], float filt_h) {
    if (DIV == kDivFlatCoarse || DIV == kDivFiltCoarse) {
        // Two-level lookup.  Every map carries a 4x4-coarsened copy whose cell holds the label shared by its 16
        // pixels, or 255 where they differ.  The patch of pixels a wave gathers is ~30 px wide and costs ~16 L2
        // requests per view in the full-resolution map (one per 128-B line = 16x8 pixels; the L2 request rate, not
        // HBM, is what the kernel waits for) but ~3 in the coarse one (a line = 64x32 pixels).  Phase A gathers
        // the coarse cells of all U views; phase B re-reads the exact pixel only for lanes that hit a mixed cell
        // (segment boundaries).  A uniform cell IS the pixel's label, so results do not change.
        unsigned pixel[U];  // xi | yi << 16 (both < 65536): the full-resolution offset is only worked out if needed
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int v = vb - 1 - u;
            bin[u] = -1;  // (pixel[u] is only read where bin[u] == 255, i.e. where it was set below)
            if (((culled >> u) & 1u) || !(FULL || v >= 0)) continue;  // wave-uniform
            const ViewRegs vd = load_view(views + v);
            int xi, yi;
            if (DIV == kDivFiltCoarse ? project_filtered(vd, filt_h, X, Y, Z, xi, yi) : project<kDivFlatSimple>(vd, X, Y, Z, xi, yi)) {
                pixel[u] = (unsigned)xi | ((unsigned)yi << 16);
                const unsigned cx = (unsigned)xi >> 2, cy = (unsigned)yi >> 2;
                const unsigned coff = __umul24(cx >> 4, (unsigned)vd.coarse_row_bytes) + (cx & 15u) + (cy << 4);
                bin[u] = ((global_u8_ptr)((unsigned long long)vd.seg_off + vd.coarse_delta))[coff];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool mixed = bin[u] == 255;
            if (__builtin_amdgcn_ballot_w64(mixed) != 0) {  // wave-uniform; rare away from segment boundaries
                const ViewDesc* __restrict__ vp = views + (vb - 1 - u);
                const global_u8_ptr base = (global_u8_ptr)(unsigned long long)vp->seg_off;
                const unsigned xi = pixel[u] & 0xffffu, yi = pixel[u] >> 16;
                if (mixed) bin[u] = base[__umul24(xi >> 4, (unsigned)vp->seg_row_bytes) + (xi & 15u) + (yi << 4)];
            }
        }
        return;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int v = vb - 1 - u;  // `v >= 0` is wave-uniform
        if ((culled >> u) & 1u) {  // wave-uniform
            bin[u] = -1;
            continue;
        }
        bin[u] = (FULL || v >= 0) ? seg_bin<DIV>(views + v, pool, X, Y, Z) : -1;
    }
}

// (The last stage's LDS layout - a wave's histograms as [bin][64 lanes] bytes - was measured here too, round 3: 1.052 ms against
// 1.036-1.043 for the row per thread, profiles/r03/lds_layout_and_replay_ab.txt; removed again.)
template <int U, int DIV>
__global__ __launch_bounds__(kBlock) void vote_fused_labels_kernel(FusedParams p, const ViewDesc* __restrict__ views,
                                                                   int* __restrict__ labels) {
    extern __shared__ uint32_t lds[];
    uint32_t* row = lds + threadIdx.x * p.stride_dw;
    uint8_t* h = reinterpret_cast<uint8_t*>(row);

    for (int k = 0; k < p.stride_dw; ++k) row[k] = 0;  // thread-private: no barrier needed
    const long long i = (long long)logical_block(blockIdx.x, gridDim.x, p.xcd_swizzle) * kBlock + threadIdx.x;
    const bool valid = i < p.n;
    // lanes past the end carry NaN: every comparison in project() fails, they never vote
    const double X = valid ? (double)p.x[i] : __builtin_nan("");
    const double Y = valid ? (double)p.y[i] : 0.0;
    const double Z = valid ? (double)p.z[i] : 0.0;
    const uint8_t* __restrict__ pool = p.pool;

    int best = -1;  // bin of the current winner
    int bestc = 0;
    const CullMasks cmask = wave_cull_masks(p.cull, p.cull_pitch, p.nviews, X, Y, Z, p.cull_tally);
    // views vb-1, vb-2, .. (reverse order); only the last, ragged chunk tests its view indices
    auto chunk = [&](auto full, int vb) {
        constexpr bool kFull = decltype(full)::value;
        int bin[U];
        gather_chunk<U, DIV, kFull>(views, pool, vb, X, Y, Z, cull_bits<U>(cmask, p.nviews - vb), bin, p.filt_h);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (bin[u] >= 0) {
                const int c = h[bin[u]] + 1;  // dls.py:295
                h[bin[u]] = (uint8_t)c;
                if (c >= bestc) {  // reverse-order tie rule == first-inserted wins (dls.py:303)
                    bestc = c;
                    best = bin[u];
                }
            }
        }
        };
    int vb = p.nviews;
    for (; vb >= U; vb -= U) chunk(std::true_type{}, vb);
    if (vb > 0) chunk(std::false_type{}, vb);
    if (valid) {
        const long long o = p.perm ? (long long)p.perm[i] : i;
        labels[o] = best - 1 + (best < 0);  // bin b -> label b-1; no vote -> -1 (dls.py:306)
    }
}

// -------------------------------------------------------------------------------------------------
// early vote, last stage (host side: early_vote_stage / vote_finalize).  While the host is still handing over the last
// maps of a run, vote_fused_planes_kernel has already voted the views [0, E) on a second stream and left their
// count plane cntA and first-view plane fvA (u8, wave-major [wave][bin][64]; code = 255 - view index, 0 = no vote).  This kernel is
// what remains between the last map and the labels: the walk of vote_fused_labels_kernel over the views [E, V) only,
// on a histogram that STARTS from cntA, and one pass over fvA.
// The reference's winner (dls.py:303) is the bin with the largest total whose first vote is earliest.  A bin with
// votes in [0, E) has its first vote there (fvA); among such bins the pass below maximises (total, fvA).  The reverse
// walk's online rule maximises (total, earliest vote inside [E, V)) over the bins voted in [E, V); if that bin has
// no vote in [0, E) it beats every other bin of its kind, and it wins only with a strictly larger total than the best
// bin that was voted earlier.  If it has votes in [0, E) it is covered by the pass.
// The planes are read as dwords by a transposed lane mapping (lane (g, t) = bins g, g+4, .. of Gaussians 4t .. 4t+3,
// as the planes kernel stores them): 256 B per wave instruction instead of 64 single bytes.
// -------------------------------------------------------------------------------------------------
// ---- early vote by RECORD and REPLAY (option "early_replay") -----------------------------------------------------------------
// The early stage only RECORDS the vote of every Gaussian in every early view (bin + 1, 0 = none; [wave][view][64 lanes]
// bytes): projection, gather, store - no histogram, no LDS, twice the waves per CU.  The last stage is the one-piece kernel
// with one difference: behind its reverse walk over the views [E, V) it does not project the views E-1 .. 0, it reads their
// votes back from the record, in the same reverse order.  Every update of the histogram and of (best, best_count) is the
// one the one-piece kernel would have made: the labels are identical by construction.
template <int U, int DIV>
__global__ __launch_bounds__(kBlock) void vote_record_kernel(FusedParams p, const ViewDesc* __restrict__ views,
                                                             uint8_t* __restrict__ rec) {
    const long long i = (long long)logical_block(blockIdx.x, gridDim.x, p.xcd_swizzle) * kBlock + threadIdx.x;
    const bool valid = i < p.n;
    const long long ic = valid ? i : 0;
    const float xf = p.x[ic], yf = p.y[ic], zf = p.z[ic];
    const double X = valid ? (double)xf : __builtin_nan("");  // lanes past the end never vote
    const double Y = valid ? (double)yf : 0.0;
    const double Z = valid ? (double)zf : 0.0;
    const uint8_t* __restrict__ pool = p.pool;
    const int lane = threadIdx.x & 63;
    uint8_t* r = rec + (i - lane) * p.nviews + lane;
    const CullMasks cmask = wave_cull_masks(p.cull, p.cull_pitch, p.nviews, X, Y, Z, p.cull_tally);
    auto chunk = [&](auto full, int vb) {
        constexpr bool kFull = decltype(full)::value;
        int bin[U];
        gather_chunk<U, DIV, kFull>(views, pool, vb, X, Y, Z, cull_bits<U>(cmask, p.nviews - vb), bin, p.filt_h);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (kFull || vb - 1 - u >= 0) r[(vb - 1 - u) * 64] = (uint8_t)(bin[u] + 1);
    };
    int vb = p.nviews;
    for (; vb >= U; vb -= U) chunk(std::true_type{}, vb);
    if (vb > 0) chunk(std::false_type{}, vb);
}

template <int U, int DIV>
__global__ __launch_bounds__(kBlock) void vote_fused_replay_kernel(FusedParams p, const ViewDesc* __restrict__ views,
                                                                   const uint8_t* __restrict__ rec, int E,
                                                                   int* __restrict__ labels) {
    extern __shared__ uint32_t lds[];
    uint32_t* row = lds + threadIdx.x * p.stride_dw;
    uint8_t* h = reinterpret_cast<uint8_t*>(row);
    for (int k = 0; k < p.stride_dw; ++k) row[k] = 0;  // thread-private: no barrier needed
    const long long i = (long long)logical_block(blockIdx.x, gridDim.x, p.xcd_swizzle) * kBlock + threadIdx.x;
    const bool valid = i < p.n;
    const long long ic = valid ? i : 0;
    const float xf = p.x[ic], yf = p.y[ic], zf = p.z[ic];
    const double X = valid ? (double)xf : __builtin_nan("");
    const double Y = valid ? (double)yf : 0.0;
    const double Z = valid ? (double)zf : 0.0;
    const uint8_t* __restrict__ pool = p.pool;
    int best = -1, bestc = 0;
    auto vote = [&](int b) {  // dls.py:295, :303 in reverse view order, as in vote_fused_labels_kernel
        const int c = h[b] + 1;
        h[b] = (uint8_t)c;
        if (c >= bestc) {
            bestc = c;
            best = b;
        }
    };
    const CullMasks cmask = wave_cull_masks(p.cull, p.cull_pitch, p.nviews, X, Y, Z, p.cull_tally);
    auto chunk = [&](auto full, int vb) {
        constexpr bool kFull = decltype(full)::value;
        int bin[U];
        gather_chunk<U, DIV, kFull>(views, pool, vb, X, Y, Z, cull_bits<U>(cmask, p.nviews - vb), bin, p.filt_h);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (bin[u] >= 0) vote(bin[u]);
    };
    int vb = p.nviews;
    for (; vb >= U; vb -= U) chunk(std::true_type{}, vb);
    if (vb > 0) chunk(std::false_type{}, vb);
    // the views E-1 .. 0 from the record, kReplay bytes of it in flight per lane
    constexpr int kReplay = 16;
    const int lane = threadIdx.x & 63;
    const uint8_t* __restrict__ r = rec + (i - lane) * E + lane;
    for (int v0 = E; v0 > 0; v0 -= kReplay) {
        unsigned b[kReplay];
#pragma unroll
        for (int j = 0; j < kReplay; ++j) {
            const int v = v0 - 1 - j;
            const unsigned got = r[max(v, 0) * 64];  // unconditional load + select
            b[j] = v >= 0 ? got : 0u;
        }
        // (Applying the replayed votes eight per LDS round trip - counters read first, repeats of a bin resolved in registers -
        // was measured, round 3: the last stage took 0.495 ms instead of 0.426; the 28 compares per batch cost more than the
        // dependent read-modify-writes they replace.  Removed, like lds_batch in the walk.)
#pragma unroll
        for (int j = 0; j < kReplay; ++j)
            if (b[j]) vote((int)b[j] - 1);
    }
    if (valid) {
        const long long o = p.perm ? (long long)p.perm[i] : i;
        labels[o] = best - 1 + (best < 0);  // bin b -> label b-1; no vote -> -1 (dls.py:306)
    }
}

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {  // v_pk_max_u16
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

template <int U, int DIV, int NQ>
__global__ __launch_bounds__(kBlock, 4) void vote_fused_final_kernel(FusedParams p, const ViewDesc* __restrict__ views,
                                                                     const uint8_t* __restrict__ cntA,
                                                                     const uint8_t* __restrict__ fvA,
                                                                     const uint8_t* __restrict__ recA, int E,
                                                                     int* __restrict__ labels, int ablate_arg) {
#ifdef GSX_EXPERIMENTS
    const int ablate = ablate_arg;  // timing experiments (tools/early_probe.py), results invalid
#else
    constexpr int ablate = 0;       // product build: every branch on it folds away
#endif
    extern __shared__ uint32_t lds[];
    const long long i = (long long)logical_block(blockIdx.x, gridDim.x, p.xcd_swizzle) * kBlock + threadIdx.x;
    const bool valid = i < p.n;
    const long long ic = valid ? i : 0;  // unconditional loads: all three in flight together with the planes' rows
    const float xf = p.x[ic], yf = p.y[ic], zf = p.z[ic];
    const double X = valid ? (double)xf : __builtin_nan("");  // lanes past the end never vote
    const double Y = valid ? (double)yf : 0.0;
    const double Z = valid ? (double)zf : 0.0;
    const uint8_t* __restrict__ pool = p.pool;
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4;
    // The wave's histogram block in LDS has the layout of its block in the planes, [bin][64 lanes] bytes (rows padded to
    // a multiple of four bins): the counts of the views [0, E) arrive by a plain coalesced copy, and dword q * 64 + lane
    // of either holds bin 4q + g of the Gaussians 4t .. 4t+3 (g = lane / 16, t = lane % 16) - what the pass over the
    // first-view plane below needs side by side.  Bank behaviour of the walk is that of the row-per-thread layout: lanes
    // voting one bin touch 16 consecutive dwords, lanes voting different bins collide now and then.
    const int nq = (p.bins + 3) >> 2;
    uint32_t* wl = lds + (threadIdx.x >> 6) * (nq * 64);  // nq * 256 bytes per wave
    uint8_t* hw = reinterpret_cast<uint8_t*>(wl) + lane;   // hw[bin * 64]: this lane's counter of a bin
    const long long wave_at = (ablate & 1) ? 0 : (i - lane) * p.bins;  // (ablate: timing experiments only, tools/early_probe.py)
    const uint32_t* __restrict__ csrc = reinterpret_cast<const uint32_t*>(cntA + wave_at) + lane;
    const uint32_t* __restrict__ fsrc = reinterpret_cast<const uint32_t*>(fvA + wave_at) + lane;
    // unconditional load + select (a conditional load costs a branch per row; the rows past the last bin lie in the next
    // wave's block or in the slack behind the planes, kEarlySlack)
    auto plane_dword = [&](const uint32_t* __restrict__ src, int q) {
        const uint32_t v = src[q * 64];
        return 4 * q + g < p.bins ? v : 0u;
    };
    // A wave lives through a chain of memory round trips and only 16 waves fit a CU (the histograms): the fewer round
    // trips, the shorter the kernel.  NQ > 0 (bins <= 4 NQ): the first-view rows are fetched right behind the counts and
    // wait in NQ registers until the walk is over; NQ == 0: any bin count, planes in rounds of kRound rows.
    constexpr int kRound = 13;
    uint32_t fd[NQ > 0 ? NQ : 1];
    if (NQ > 0) {
        uint32_t w[NQ > 0 ? NQ : 1];
#pragma unroll
        for (int q = 0; q < NQ; ++q) w[q] = plane_dword(csrc, q);
#pragma unroll
        for (int q = 0; q < NQ; ++q) fd[q] = plane_dword(fsrc, q);  // right behind the counts: ONE round trip for both planes
        __builtin_amdgcn_sched_barrier(0);                          // (keep all 2 NQ loads ahead of the first LDS write)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (q < nq) wl[q * 64 + lane] = w[q];
    } else {
        for (int q0 = 0; q0 < nq; q0 += kRound) {
            uint32_t w[kRound];
#pragma unroll
            for (int j = 0; j < kRound; ++j) w[j] = plane_dword(csrc, q0 + j);
#pragma unroll
            for (int j = 0; j < kRound; ++j)
                if (q0 + j < nq) wl[(q0 + j) * 64 + lane] = w[j];
        }
    }
    __builtin_amdgcn_wave_barrier();  // the block is written and read by the lanes of ONE wave: LDS keeps a wave's order

    int best = -1, bestc = 0;
    const CullMasks cmask = wave_cull_masks((ablate & 32) ? nullptr : p.cull, p.cull_pitch, p.nviews, X, Y, Z, p.cull_tally);
    auto chunk = [&](auto full, int vb) {
        constexpr bool kFull = decltype(full)::value;
        int bin[U];
        gather_chunk<U, DIV, kFull>(views, pool, vb, X, Y, Z, cull_bits<U>(cmask, p.nviews - vb), bin, p.filt_h);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (bin[u] >= 0) {
                const int c = hw[bin[u] * 64] + 1;  // dls.py:295
                hw[bin[u] * 64] = (uint8_t)c;
                if (c >= bestc) {  // reverse order: the bin whose earliest vote in [E, V) comes first survives a tie
                    bestc = c;
                    best = bin[u];
                }
            }
        }
    };
    int vb = p.nviews;
    for (; vb >= U; vb -= U) chunk(std::true_type{}, vb);
    if (vb > 0) chunk(std::false_type{}, vb);
    __builtin_amdgcn_wave_barrier();

    // Largest 16-bit key total << 8 | first-view code over ALL bins, per Gaussian: two packed maxima per lane for its four
    // Gaussians, v_perm_b32 pairs a dword of totals with a dword of codes.  A bin without a vote in [0, E) has code 0 and
    // loses against an equal total with one: the order the tie rule asks for.
    uint32_t m01 = 0u, m23 = 0u;
    auto fold = [&](uint32_t f4, int q) {
        const uint32_t hd = wl[q * 64 + lane];
        m01 = pk_max_u16(m01, __builtin_amdgcn_perm(hd, f4, 0x05010400u));  // [T1 f1 T0 f0]
        m23 = pk_max_u16(m23, __builtin_amdgcn_perm(hd, f4, 0x07030602u));  // [T3 f3 T2 f2]
    };
    if (ablate & 4) {  // timing experiment: no pass over the first-view rows (they are still fetched)
#pragma unroll
        for (int q = 0; q < (NQ > 0 ? NQ : 1); ++q) m01 |= fd[q] & 1u;
    } else if (NQ > 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (q < nq) fold(fd[q], q);
    } else {
        for (int q0 = 0; q0 < nq; q0 += kRound) {
            uint32_t f[kRound];
#pragma unroll
            for (int j = 0; j < kRound; ++j) f[j] = plane_dword(fsrc, q0 + j);
#pragma unroll
            for (int j = 0; j < kRound; ++j)
                if (q0 + j < nq) fold(f[j], q0 + j);
        }
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {  // the four lanes (0..3, t) share their Gaussians
        m01 = pk_max_u16(m01, (uint32_t)__shfl_xor((int)m01, o));
        m23 = pk_max_u16(m23, (uint32_t)__shfl_xor((int)m23, o));
    }
    // Gaussian `lane` = 4 t' + k' is key k' of the lanes with t = t'
    const uint32_t s01 = (uint32_t)__shfl((int)m01, lane >> 2), s23 = (uint32_t)__shfl((int)m23, lane >> 2);
    const uint32_t pair = (lane & 2) ? s23 : s01;
    const unsigned mine = (lane & 1) ? pair >> 16 : pair & 0xffffu;
    if (valid) {
        // code 0: no bin was voted in [0, E) and reached the total of the walk's winner -> the walk's winner (-1: no vote at
        // all).  Otherwise the winner is the bin this Gaussian voted in view 255 - code: the early stage kept that record.
        int win = best;
        const unsigned code = mine & 0xffu;
        if (code && !(ablate & 8)) win = (int)recA[(i - lane) * E + (255 - (int)code) * 64 + lane] - 1;
        const long long o = (p.perm && !(ablate & 16)) ? (long long)p.perm[i] : i;
        labels[o] = win - 1 + (win < 0);  // bin b -> label b-1; no vote -> -1 (dls.py:306)
    }
}

// -------------------------------------------------------------------------------------------------
// exchange protocol v3, rank-local part 1: the same walk as the labels kernel (u8 counters, 16 waves/CU)
// but the only output is this rank's COUNT plane, u8 [slab][bins][sn].  No first-view plane: ties are
// resolved later, for the tied Gaussians only, by vote_tie_kernel.
// -------------------------------------------------------------------------------------------------
template <int U, int DIV>
__global__ __launch_bounds__(kBlock) void vote_fused_counts_kernel(FusedParams p, const ViewDesc* __restrict__ views,
                                                                   uint8_t* __restrict__ cnt, long long sn) {
    extern __shared__ uint32_t lds[];
    uint32_t* row = lds + threadIdx.x * p.stride_dw;
    for (int k = 0; k < p.stride_dw; ++k) row[k] = 0;
    uint8_t* h = reinterpret_cast<uint8_t*>(row);
    const long long i = (long long)logical_block(blockIdx.x, gridDim.x, p.xcd_swizzle) * kBlock + threadIdx.x;
    const bool valid = i < p.n;
    const double X = valid ? (double)p.x[i] : __builtin_nan("");
    const double Y = valid ? (double)p.y[i] : 0.0;
    const double Z = valid ? (double)p.z[i] : 0.0;
    const uint8_t* __restrict__ pool = p.pool;
    const CullMasks cmask = wave_cull_masks(p.cull, p.cull_pitch, p.nviews, X, Y, Z, p.cull_tally);
    // views vb-1, vb-2, .. (reverse order); only the last, ragged chunk tests its view indices
    auto chunk = [&](auto full, int vb) {
        constexpr bool kFull = decltype(full)::value;
        int bin[U];
        gather_chunk<U, DIV, kFull>(views, pool, vb, X, Y, Z, cull_bits<U>(cmask, p.nviews - vb), bin, p.filt_h);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (bin[u] >= 0) h[bin[u]] = (uint8_t)(h[bin[u]] + 1);
        };
    int vb = p.nviews;
    for (; vb >= U; vb -= U) chunk(std::true_type{}, vb);
    if (vb > 0) chunk(std::false_type{}, vb);
    // transposed store (see vote_fused_planes_kernel): lane (g, t) packs bin 4*it+g of Gaussians 4t..4t+3
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    const long long i0 = i - lane;
    const long long slab = i0 / sn;
    const long long base = slab * p.bins * sn + (i0 - slab * sn) + 4 * t;
    const uint32_t* wrow = lds + (threadIdx.x - lane + 4 * t) * p.stride_dw;
    for (int b = g; b < p.bins; b += 4) {
        uint32_t pc = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) pc |= (uint32_t)reinterpret_cast<const uint8_t*>(wrow + k * p.stride_dw)[b] << (8 * k);
        *reinterpret_cast<uint32_t*>(cnt + base + (long long)b * sn) = pc;
    }
}

// v3, slab owner: sum the S ranks' counters per bin; a unique maximum is the label, otherwise the Gaussian is
// TIED (label -2 for now) and the set of max-count bins goes out as a bit mask, cand[word][sn], 8 words.
static constexpr int kCandWords = 8;  // bins <= 256
// One thread owns 4 consecutive Gaussians: every plane row is read as coalesced dwords (256 B per wave
// instruction instead of 64 single bytes).  (Two passes - maximum, then masks - read the slab twice: 0.37 ms;
// parking the totals in LDS instead was 2x slower still, 77 KB per wave leaves 2 waves per CU.)
__device__ __forceinline__ void slab_totals4(const uint8_t* __restrict__ rcnt, int S, int bins, long long sn, long long i4, int b,
                                             unsigned t[4]) {
    t[0] = t[1] = t[2] = t[3] = 0;
    for (int r = 0; r < S; ++r) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(rcnt + ((long long)r * bins + b) * sn + i4);
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] += (w >> (8 * k)) & 0xffu;
    }
}

__global__ __launch_bounds__(kBlock) void vote_slab_totals_kernel(const uint8_t* __restrict__ rcnt, int S, int bins,
                                                                  long long sn, int* __restrict__ slab_labels,
                                                                  uint32_t* __restrict__ cand) {
    const long long i4 = ((long long)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (i4 >= sn) return;
    // ONE pass over the planes: the mask of max-count bins is built against the running maximum; a word of 32 bins
    // remembers the maximum its bits refer to, and only the words whose maximum is the final one survive.
    unsigned M[4] = {0, 0, 0, 0};
    uint32_t word[kCandWords][4];
    unsigned wmax[kCandWords][4];
#pragma unroll
    for (int w = 0; w < kCandWords; ++w) {
#pragma unroll
        for (int k = 0; k < 4; ++k) word[w][k] = 0, wmax[w][k] = 0;
        if (w * 32 < bins) {  // wave-uniform
            const int nb = min(32, bins - w * 32);
#pragma unroll 4
            for (int bb = 0; bb < nb; ++bb) {
                unsigned t[4];
                slab_totals4(rcnt, S, bins, sn, i4, w * 32 + bb, t);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (t[k] > M[k]) {  // a new maximum: the bits gathered so far in this word are void
                        M[k] = t[k];
                        word[w][k] = 0;
                    }
                    if (t[k] == M[k]) word[w][k] |= 1u << bb;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) wmax[w][k] = M[k];
        }
    }
    int n_max[4] = {0, 0, 0, 0}, first_bin[4] = {-1, -1, -1, -1};
#pragma unroll
    for (int w = 0; w < kCandWords; ++w) {
        uint32_t out[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            out[k] = (M[k] > 0 && wmax[w][k] == M[k]) ? word[w][k] : 0u;
            if (out[k] && n_max[k] == 0) first_bin[k] = w * 32 + __ffs(out[k]) - 1;
            n_max[k] += __popc(out[k]);
        }
        *reinterpret_cast<uint4*>(cand + (long long)w * sn + i4) = make_uint4(out[0], out[1], out[2], out[3]);
    }
    int lab[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) lab[k] = n_max[k] == 0 ? -1 : (n_max[k] == 1 ? first_bin[k] - 1 : -2);
    *reinterpret_cast<int4*>(slab_labels + i4) = make_int4(lab[0], lab[1], lab[2], lab[3]);
}

// (A wave-ballot compaction of the tied Gaussians in front of this kernel was measured: 0.90 ms vs 0.59 ms —
// the atomically ordered list loses the Morton locality of the gathers; not kept.)
// v3, every rank: for each TIED Gaussian (two or more candidate bins) walk this rank's views in FORWARD order
// and stop at the first one that votes a candidate: code = (255 - local view index) << 8 | bin, 0 if none.
// cand_all: [S][kCandWords][sn] (all-gathered masks); codes: u16 [S][sn], slab-major.
// earlier: codes of n_earlier batches that come BEFORE this one in view order and were walked before it (one GPU playing the
// ranks one after the other): a Gaussian one of them has resolved is not walked again - the earliest batch wins anyway.
__global__ __launch_bounds__(kBlock) void vote_tie_kernel(FusedParams p, const ViewDesc* __restrict__ views,
                                                          const uint32_t* __restrict__ cand_all, long long sn,
                                                          uint16_t* __restrict__ codes, const uint16_t* __restrict__ earlier,
                                                          int n_earlier) {
    const long long i = (long long)logical_block(blockIdx.x, gridDim.x, p.xcd_swizzle) * kBlock + threadIdx.x;
    if (i >= p.n) return;
    for (int e = 0; e < n_earlier; ++e)
        if (earlier[(long long)e * sn + i]) {  // (single slab: codes are [batch][sn])
            codes[i] = 0;
            return;
        }
    const long long slab = i / sn, j = i - slab * sn;
    uint32_t mask[kCandWords];
    int pop = 0;
#pragma unroll
    for (int w = 0; w < kCandWords; ++w) {
        mask[w] = cand_all[(slab * kCandWords + w) * sn + j];
        pop += __popc(mask[w]);
    }
    unsigned code = 0;
    if (pop >= 2) {
        const double X = (double)p.x[i], Y = (double)p.y[i], Z = (double)p.z[i];
        for (int v = 0; v < p.nviews; ++v) {
            const int sb = seg_bin<kDivFlat>(views + v, p.pool, X, Y, Z);
            if (sb < 0) continue;
            const unsigned b = (unsigned)sb;
            uint32_t word = 0;
#pragma unroll
            for (int w = 0; w < kCandWords; ++w) word = (b >> 5) == (unsigned)w ? mask[w] : word;
            if ((word >> (b & 31u)) & 1u) {
                code = ((unsigned)(255 - v) << 8) | b;
                break;
            }
        }
    }
    codes[i] = (uint16_t)code;  // == codes[slab][j]: n_pad = S * sn
}

// v3, slab owner: a tied Gaussian takes the candidate first voted by the LOWEST rank that voted one (ranks own
// contiguous rank-ordered view blocks), i.e. the globally earliest view.  rcodes: u16 [S(src)][sn].
__global__ __launch_bounds__(kBlock) void vote_tie_resolve_kernel(const uint16_t* __restrict__ rcodes, int S, long long sn,
                                                                  int* __restrict__ slab_labels) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= sn || slab_labels[i] != -2) return;
    int label = -1;
    for (int r = 0; r < S; ++r) {
        const unsigned c = rcodes[(long long)r * sn + i];
        if (c) {
            label = (int)(c & 0xffu) - 1;
            break;
        }
    }
    slab_labels[i] = label;
}

// -------------------------------------------------------------------------------------------------
// fused vote, planes mode (multi-GPU exchange, or more than kMaxBatch views): the batch's votes
// are merged into the global planes cnt[bins][n_pad] / fv[bins][n_pad].
// LDS word per bin: count << 8 | local index of the earliest view that voted it.
// fv code = FVMAX - global view index of the first vote (larger = earlier; 0 = no vote).
// -------------------------------------------------------------------------------------------------
template <int U, typename PT, int DIV>
__global__ __launch_bounds__(kBlock) void vote_fused_planes_kernel(FusedParams p, const ViewDesc* __restrict__ views,
                                                                   PT* __restrict__ cnt,
                                                                   PT* __restrict__ fv, long long sn,
                                                                   int view_base, int fresh, int local_codes,
                                                                   uint8_t* __restrict__ rec) {
    constexpr int FVMAX = sizeof(PT) == 1 ? 255 : 65535;
    extern __shared__ uint32_t lds[];
    uint32_t* row = lds + threadIdx.x * p.stride_dw;
    for (int k = 0; k < p.stride_dw; ++k) row[k] = 0;
    uint16_t* h = reinterpret_cast<uint16_t*>(row);

    const long long i = (long long)logical_block(blockIdx.x, gridDim.x, p.xcd_swizzle) * kBlock + threadIdx.x;
    const bool valid = i < p.n;
    const double X = valid ? (double)p.x[i] : __builtin_nan("");
    const double Y = valid ? (double)p.y[i] : 0.0;
    const double Z = valid ? (double)p.z[i] : 0.0;
    const uint8_t* __restrict__ pool = p.pool;

    const CullMasks cmask = wave_cull_masks(p.cull, p.cull_pitch, p.nviews, X, Y, Z, p.cull_tally);
    // views vb-1, vb-2, .. (reverse order); only the last, ragged chunk tests its view indices
    auto chunk = [&](auto full, int vb) {
        constexpr bool kFull = decltype(full)::value;
        int bin[U];
        gather_chunk<U, DIV, kFull>(views, pool, vb, X, Y, Z, cull_bits<U>(cmask, p.nviews - vb), bin, p.filt_h);
        if (rec) {  // early vote: the record of every vote, [wave][view][64 lanes] bytes (bin + 1, 0 = none) - the last stage
                    // looks the winner's bin up by the view of its first vote
            uint8_t* r = rec + (i - (threadIdx.x & 63)) * p.nviews + (threadIdx.x & 63);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (kFull || vb - 1 - u >= 0) r[(vb - 1 - u) * 64] = (uint8_t)(bin[u] + 1);
        }
        unsigned old[U];  // one LDS round trip per chunk, repeats of a bin resolved in registers
#pragma unroll
        for (int u = 0; u < U; ++u) old[u] = bin[u] >= 0 ? (unsigned)h[bin[u]] : 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (bin[u] >= 0) {
                const int v = vb - 1 - u;
                unsigned cnt = (old[u] >> 8) + 1u;
#pragma unroll
                for (int w = 0; w < u; ++w) cnt += (bin[w] == bin[u]) ? 1u : 0u;
                h[bin[u]] = (uint16_t)((cnt << 8) | (unsigned)v);  // reverse order: the last store = the earliest view
            }
        }
        };
    int vb = p.nviews;
    for (; vb >= U; vb -= U) chunk(std::true_type{}, vb);
    if (vb > 0) chunk(std::false_type{}, vb);
    // planes are slab-major: [slab][bin][sn] with slab = i / sn (one slab = one rank's share in the
    // all-to-all exchange; a single slab is the plain [bin][n_pad] layout).  sn is a multiple of the block
    // size, so a workgroup never straddles two slabs.
    const int vb0 = local_codes ? 0 : view_base;  // local codes: 255 - index inside this rank's batch
    if (sizeof(PT) == 1 && fresh) {
        // Transposed store through the wave's own LDS rows: lane (g, t) = (lane / 16, lane % 16) packs bin
        // 4*it + g of Gaussians 4t .. 4t+3 into one dword per plane, so a wave writes 4 bins x 64 B per
        // instruction pair instead of 1 bin x 64 single bytes.  Rows of lanes past n hold zeros.
        const int lane = threadIdx.x & 63;
        const int g = lane >> 4, t = lane & 15;
        const long long i0 = i - lane;  // first Gaussian of this wave
        const long long slab = i0 / sn;
        const long long base = slab * p.bins * sn + (i0 - slab * sn) + 4 * t;
        const uint32_t* wrow = lds + (threadIdx.x - lane + 4 * t) * p.stride_dw;
        for (int b = g; b < p.bins; b += 4) {
            uint32_t pc = 0, pf = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned w = reinterpret_cast<const uint16_t*>(wrow + k * p.stride_dw)[b];
                const unsigned c = w >> 8;
                const unsigned code = c ? (unsigned)(FVMAX - (vb0 + (int)(w & 0xffu))) : 0u;
                pc |= c << (8 * k);
                pf |= code << (8 * k);
            }
            const long long at = base + (long long)b * sn;
            *reinterpret_cast<uint32_t*>(cnt + at) = pc;
            *reinterpret_cast<uint32_t*>(fv + at) = pf;
        }
        return;
    }
    if (!valid) return;
    const long long slab = i / sn;
    const long long base = slab * p.bins * sn + (i - slab * sn);
    for (int b = 0; b < p.bins; ++b) {
        const unsigned w = h[b];
        const unsigned c = w >> 8;
        const unsigned code = c ? (unsigned)(FVMAX - (vb0 + (int)(w & 0xffu))) : 0u;
        const long long at = base + (long long)b * sn;
        if (fresh) {
            cnt[at] = (PT)c;
            fv[at] = (PT)code;
        } else if (c) {
            cnt[at] = (PT)(cnt[at] + c);
            const unsigned old = fv[at];
            if (code > old) fv[at] = (PT)code;
        }
    }
}

// per Gaussian: among the bins holding the (global) maximum count, the one this rank saw first
template <typename PT>
__global__ __launch_bounds__(kBlock) void vote_keys_kernel(const PT* __restrict__ cnt, const PT* __restrict__ fv,
                                                           long long n, long long sn, int bins,
                                                           int* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const long long slab = i / sn;
    const long long base = slab * bins * sn + (i - slab * sn);
    unsigned M = 0;
    int key = 0;
    for (int b = 0; b < bins; ++b) {
        const unsigned c = cnt[base + (long long)b * sn];
        if (c == 0 || c < M) continue;
        const unsigned f = fv[base + (long long)b * sn];
        const int k = f ? (int)((f << 8) | (unsigned)b) : 0;
        if (c > M) {
            M = c;
            key = k;
        } else if (k > key) {
            key = k;
        }
    }
    keys[i] = key;
}

// ---- exchange v2: after the all-to-all this rank holds, for ITS slab of Gaussians, every rank's u8 count and
// first-view planes: recv[r][bin][sn].  Sum the counts, and among the bins holding the maximum pick the one
// whose first vote is globally earliest: ranks own contiguous, rank-ordered view blocks, so that is the
// lowest rank that voted it, then its local view code (255 - local index; larger = earlier).
__global__ __launch_bounds__(kBlock) void vote_slab_reduce_kernel(const uint8_t* __restrict__ rcnt,
                                                                  const uint8_t* __restrict__ rfv, int S, int bins,
                                                                  long long sn, int* __restrict__ slab_labels) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= sn) return;
    unsigned M = 0;
    int best_bin = -1;
    unsigned best_key = 0;  // (S - r) << 8 | code : larger = earlier
    for (int b = 0; b < bins; ++b) {
        unsigned total = 0;
        unsigned key = 0;
        for (int r = 0; r < S; ++r) {
            const long long at = ((long long)r * bins + b) * sn + i;
            const unsigned c = rcnt[at];
            total += c;
            if (c && key == 0) key = ((unsigned)(S - r) << 8) | (unsigned)rfv[at];
        }
        if (total == 0 || total < M) continue;
        if (total > M || key > best_key) {
            M = total;
            best_key = key;
            best_bin = b;
        }
    }
    slab_labels[i] = best_bin - 1 + (best_bin < 0);  // bin b -> label b-1; never visible -> -1
}

__global__ __launch_bounds__(kBlock) void unpermute_labels_kernel(const int* __restrict__ sorted, long long n,
                                                                  const uint32_t* __restrict__ perm,
                                                                  int* __restrict__ labels) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) labels[perm ? (long long)perm[i] : i] = sorted[i];
}

__global__ __launch_bounds__(kBlock) void vote_labels_kernel(const int* __restrict__ keys, long long n,
                                                             const uint32_t* __restrict__ perm,
                                                             int* __restrict__ labels) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int k = keys[i];
    labels[perm ? (long long)perm[i] : i] = k ? (k & 0xff) - 1 : -1;
}

// -------------------------------------------------------------------------------------------------
// host side
// -------------------------------------------------------------------------------------------------
void fill_view_desc(ViewDesc& vd, const gsx_camera* cam, int seg_w, int seg_h, int img_w, int img_h) {
    std::memset(&vd, 0, sizeof vd);
    double nR[9];
    for (int k = 0; k < 9; ++k) {
        vd.R[k] = cam->R[k];
        nR[k] = -cam->R[k];  // t = -R @ p: unary minus first (dls.py:66)
    }
    for (int r = 0; r < 3; ++r)
        vd.t[r] = std::fma(nR[3 * r + 2], cam->p[2], std::fma(nR[3 * r + 0], cam->p[0], nR[3 * r + 1] * cam->p[1]));
    vd.fx = cam->fx;
    vd.fy = cam->fy;
    vd.half_w = (double)cam->width / 2.0;
    vd.half_h = (double)cam->height / 2.0;
    vd.width = (double)cam->width;
    vd.height = (double)cam->height;
    vd.cam_w = cam->width;
    vd.cam_h = cam->height;
    vd.hw32 = (float)vd.half_w;  // exact for frames up to 2^24 pixels a side
    vd.hh32 = (float)vd.half_h;
    vd.wscale = (double)seg_w / (double)img_w;
    vd.hscale = (double)seg_h / (double)img_h;
    vd.seg_w = seg_w;
    vd.seg_h = seg_h;
    // int(x*1.0) == x; the clamp (dls.py:285-286) is a no-op only if the camera frame fits the map
    vd.unit_scale = (vd.wscale == 1.0 && vd.hscale == 1.0 && cam->width <= seg_w && cam->height <= seg_h) ? 1 : 0;
}

// The branchless projection variant a set of views allows under this context's options.  simple: every view has unit scale and
// a tiled map; coarse: ... and a coarse level.
static inline int flat_div_mode(const Ctx* c, bool simple, bool coarse) {
    if (!simple) return kDivFlat;
    return coarse && c->vopt.seg_coarse ? (c->vopt.filter_project ? kDivFiltCoarse : kDivFlatCoarse) : kDivFlatSimple;
}
// call after sync_views(): views_simple describes the staged batch
static inline int div_mode(const Ctx* c) {
    return c->vopt.flat_project ? flat_div_mode(c, c->run.views_simple, c->run.views_coarse) : kDivExact;
}
// Kernel selection: calls f(std::integral_constant<int, DIV>{}) for the projection variant dm and returns what it returns
// (the same type for every DIV: a kernel pointer).  FLAT_ONLY: f is instantiated for the four branchless variants only -
// the early-vote kernels exist for no other, and their stages never run without "flat_project".
template <bool FLAT_ONLY = false, class F>
static inline auto with_div(int dm, F&& f) {
    switch (dm) {
        case kDivFiltCoarse: return f(std::integral_constant<int, kDivFiltCoarse>{});
        case kDivFlatCoarse: return f(std::integral_constant<int, kDivFlatCoarse>{});
        case kDivFlatSimple: return f(std::integral_constant<int, kDivFlatSimple>{});
        case kDivFlat: return f(std::integral_constant<int, kDivFlat>{});
        default: return f(std::integral_constant<int, FLAT_ONLY ? kDivFlat : kDivExact>{});
    }
}

int project_all(Ctx* c, const gsx_camera* cam, const float* dx, const float* dy, const float* dz, int64_t n,
                int32_t* x_host, int32_t* y_host, const uint32_t* perm) {
    if (n <= 0) return GSX_OK;
    GSX_HIP(c, hipSetDevice(c->device));
    ViewDesc vd;
    fill_view_desc(vd, cam, 1, 1, 1, 1);
    DevBuf dvd, ox, oy;
    GSX_HIP(c, dvd.ensure(sizeof vd));
    GSX_HIP(c, ox.ensure(sizeof(int) * n));
    GSX_HIP(c, oy.ensure(sizeof(int) * n));
    int rc = GSX_OK;
    hipError_t e = hipMemcpyAsync(dvd.p, &vd, sizeof vd, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        ProfScope ps(c, "project");
        // the filtered form is the vote kernels' (kDivFiltCoarse): frames up to 65535 pixels a side (hw32 exact, E < 1/64)
        const int dim = std::max(cam->width, cam->height);
        const float filt_h = (float)(0.5 - kFilterK * (double)std::max(dim, 64) * 5.9604644775390625e-08);
        const bool filtered = c->vopt.flat_project && c->vopt.filter_project && dim <= 65535;
        auto k = filtered ? project_kernel<kDivFiltCoarse> : c->vopt.flat_project ? project_kernel<kDivFlat> : project_kernel<kDivExact>;
        hipLaunchKernelGGL(k, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, dx, dy, dz, (long long)n, dvd.as<ViewDesc>(), perm, ox.as<int>(),
                           oy.as<int>(), filtered ? filt_h : 0.f);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(x_host, ox.p, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(y_host, oy.p, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, GSX_E_HIP, "project_all: %s", hipGetErrorString(e));
    dvd.release();
    ox.release();
    oy.release();
    return rc;
}

// Orders c->stream behind whatever the second stream was last asked to do.  Needed wherever an early stage's buffers (ecnt,
// efv, erec, bcnt) or the pool it reads are touched again: by the last stage that uses its result, and just as much by every
// path that DROPS the result (fewer views than announced, rewind, a new run) and is about to overwrite those buffers.
int early_join(Ctx* c) {
    if (!c->early.inflight) return GSX_OK;
    GSX_HIP(c, c->early.done_ev.stream_wait(c->stream));
    c->early.inflight = false;
    return GSX_OK;
}

int vote_begin(Ctx* c, int n_classes, int first_view, int total_views) {
    if (n_classes < 1 || n_classes > 255)
        return fail(c, GSX_E_UNSUPPORTED, "vote_begin: n_classes=%d outside [1,255] (u8 seg maps)", n_classes);
    if (first_view < 0 || total_views < 1 || total_views > 65535 || first_view >= total_views)
        return fail(c, GSX_E_INVALID, "vote_begin: first_view=%d total_views=%d (need 0 <= first < total <= 65535)",
                    first_view, total_views);
    GSX_HIP(c, hipSetDevice(c->device));
    c->run.begin_run(c->vopt, c->n, n_classes, first_view, total_views);
    c->ho.begin_run();
    c->planes.begin_run();
    if (const int rc = early_join(c)) return rc;  // an abandoned run's early stage may still be running: this run reuses its buffers
    c->early.begin_run();
    GSX_HIP(c, c->run.errflag.ensure(sizeof(int)));
    GSX_HIP(c, hipMemsetAsync(c->run.errflag.p, 0x7f, sizeof(int), c->stream));  // kNoBadView
    c->run.begun = true;
    return GSX_OK;
}

// Five world-space planes per view for wave_cull_masks().  With pc = R p + t (camera space) the reference rejects a
// Gaussian when pc_z <= 0 (dls.py:72) or when px = fx pc_x / pc_z + w/2 leaves [0, w) (:80), i.e. for pc_z > 0 when
// h(pc) >= 0 for one of
//      h = -pc_z,   fx pc_x - (w/2) pc_z,   -fx pc_x - (w/2) pc_z,   fy pc_y - (h/2) pc_z,   -fy pc_y - (h/2) pc_z .
// Each h = alpha . pc = (R^T alpha) . p + alpha . t is linear in the world position p; over a sphere (c, r) its minimum
// is a.c + b - r |a|.  The floating-point projection of a point p can deviate from real arithmetic by at most a few
// ulp of |alpha|_1 (|R|_F |p| + |t|), so the test demands h >= delta with delta = 1e-9 times that quantity (a million
// times the worst case) for the largest |p| of the sphere: stored are A = a/|a|, B = (b - 1e-9 |alpha|_1 |t|)/|a|
// and M = 1e-9 |alpha|_1 |R|_F / |a|, and the device tests  A.c + B > r + M (|c|_1 + r).
// Views with non-finite or extreme parameters (outside 1e-30 .. 1e30) get planes that never fire.
static constexpr int kCullStride = 5;  // doubles per plane
static void cull_planes(const ViewDesc& v, double out[kCullStride * kCullPlanes]) {
    for (int k = 0; k < kCullPlanes; ++k) {  // "never": 0.c - 1 > r + 0 is false for every r >= 0
        for (int j = 0; j < kCullStride; ++j) out[kCullStride * k + j] = 0.0;
        out[kCullStride * k + 3] = -1.0;
    }
    double rf = 0.0, tn = 0.0;
    for (int k = 0; k < 9; ++k) rf += v.R[k] * v.R[k];
    for (int k = 0; k < 3; ++k) tn += v.t[k] * v.t[k];
    rf = std::sqrt(rf);
    tn = std::sqrt(tn);
    auto sane = [](double x, double lo) { return std::isfinite(x) && std::fabs(x) >= lo && std::fabs(x) <= 1e30; };
    if (!(sane(rf, 1e-10) && sane(tn, 0.0) && sane(v.fx, 1e-30) && sane(v.fy, 1e-30) && sane(v.half_w, 1e-30) &&
          sane(v.half_h, 1e-30) && rf <= 1e10))
        return;
    const double alpha[kCullPlanes][3] = {{0.0, 0.0, -1.0},
                                          {v.fx, 0.0, -v.half_w},
                                          {-v.fx, 0.0, -v.half_w},
                                          {0.0, v.fy, -v.half_h},
                                          {0.0, -v.fy, -v.half_h}};
    for (int k = 0; k < kCullPlanes; ++k) {
        const double* al = alpha[k];
        double a[3], b = 0.0, l1 = 0.0;
        for (int j = 0; j < 3; ++j) {
            a[j] = v.R[0 + j] * al[0] + v.R[3 + j] * al[1] + v.R[6 + j] * al[2];  // (R^T alpha)_j
            b += al[j] * v.t[j];
            l1 += std::fabs(al[j]);
        }
        const double na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        if (!(std::isfinite(na) && na > 1e-200 && std::isfinite(b))) continue;
        double pl[kCullStride] = {a[0] / na, a[1] / na, a[2] / na, (b - 1e-9 * l1 * tn - 1e-280) / na, 1e-9 * l1 * rf / na};
        bool ok = true;
        for (int j = 0; j < kCullStride; ++j) ok = ok && std::isfinite(pl[j]);
        if (ok)
            for (int j = 0; j < kCullStride; ++j) out[kCullStride * k + j] = pl[j];
    }
}

static constexpr size_t kTallyBytes = sizeof(unsigned long long) * kTallySlots * kTallyStride;
static int ensure_tally(Ctx* c) {
    if (c->run.d_cull_tally.p) return GSX_OK;
    GSX_HIP(c, c->run.d_cull_tally.ensure(kTallyBytes));
    GSX_HIP(c, hipMemsetAsync(c->run.d_cull_tally.p, 0, kTallyBytes, c->stream));
    return GSX_OK;
}

int vote_culled(Ctx* c, int64_t* out, bool reset) {
    unsigned long long h = 0;
    if (c->run.d_cull_tally.p) {
        GSX_HIP(c, hipSetDevice(c->device));
        std::vector<unsigned long long> slots(kTallySlots * kTallyStride);
        GSX_HIP(c, hipMemcpyAsync(slots.data(), c->run.d_cull_tally.p, kTallyBytes, hipMemcpyDeviceToHost, c->stream));
        if (reset) GSX_HIP(c, hipMemsetAsync(c->run.d_cull_tally.p, 0, kTallyBytes, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
        for (unsigned k = 0; k < kTallySlots; ++k) h += slots[(size_t)k * kTallyStride];
    }
    *out = (int64_t)h;
    return GSX_OK;
}

// ---- what project_filtered()'s proof assumes about the hardware, measured on the device -------------------------------
// Exhaustive: v_rcp_f32 on EVERY float in [2^-41, 2^41] against the exact reciprocal (r * z in double is exact, so
// |r z - 1| is the relative error of r); and the special cases of v_fract_f32 / v_cvt_flr_i32_f32 the filter meets.
__global__ __launch_bounds__(kBlock) void filter_check_kernel(unsigned lo_bits, unsigned hi_bits, unsigned long long* worst) {
    double m = 0.0;
    for (unsigned long long b = (unsigned long long)lo_bits + (unsigned long long)blockIdx.x * kBlock + threadIdx.x; b <= hi_bits;
         b += (unsigned long long)gridDim.x * kBlock) {
        const float z = __builtin_bit_cast(float, (unsigned)b);
        const float r = __builtin_amdgcn_rcpf(z);
        m = fmax(m, fabs((double)r * (double)z - 1.0));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(worst, (unsigned long long)__double_as_longlong(m));  // non-negative doubles order as integers
}
__global__ void filter_special_kernel(double* out) {
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    volatile float in[8] = {inf, -inf, -1e-10f, nan, 1920.5f, -0.25f, 3.0e38f, -3.0e38f};
    for (int k = 0; k < 8; ++k) {
        const float v = in[k];
        out[k] = (double)__builtin_amdgcn_fractf(v);
        out[8 + k] = (double)cvt_floor_i32(v);
    }
}

int filter_check(Ctx* c, double* out) {
    GSX_HIP(c, hipSetDevice(c->device));
    DevBuf buf;
    GSX_HIP(c, buf.ensure(8 + 16 * sizeof(double)));
    GSX_HIP(c, hipMemsetAsync(buf.p, 0, 8 + 16 * sizeof(double), c->stream));
    const unsigned lo = 0x2B000000u /* 2^-41 */, hi = 0x54000000u /* 2^41 */;
    hipLaunchKernelGGL(filter_check_kernel, dim3(4096), dim3(kBlock), 0, c->stream, lo, hi, buf.as<unsigned long long>());
    hipLaunchKernelGGL(filter_special_kernel, dim3(1), dim3(1), 0, c->stream, reinterpret_cast<double*>(buf.as<char>() + 8));
    GSX_HIP(c, hipGetLastError());
    unsigned long long w = 0;
    GSX_HIP(c, hipMemcpyAsync(&w, buf.p, 8, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(out + 1, buf.as<char>() + 8, 16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    double m;
    std::memcpy(&m, &w, 8);
    out[0] = m / 5.9604644775390625e-08;  // in units of u = 2^-24
    buf.release();
    return GSX_OK;
}

void debug_cull_planes(const gsx_camera* cam, double* out) {
    ViewDesc vd;
    fill_view_desc(vd, cam, cam->width > 0 ? cam->width : 1, cam->height > 0 ? cam->height : 1, 1, 1);
    cull_planes(vd, out);
}

// The device form of the views [lo, hi) into dev[0 .. hi - lo): the host descriptor with the map's absolute address (seg_off +
// pool_base; one scalar add less per view and wave); their culling planes into planes[k * pitch + (i - lo)], plane-component-
// major so that lane l reads view l with unit stride.  Returns what the projection variants ask of a batch (flat_div_mode).
struct ViewKinds {
    bool simple, coarse;  // every view: unit scale + tiled map; ... and a coarse level
};
static ViewKinds stage_views(const Ctx* c, int lo, int hi, const void* pool_base, ViewDesc* dev, double* planes, size_t pitch) {
    const long long base = (long long)reinterpret_cast<uintptr_t>(pool_base);
    ViewKinds kinds{true, true};
    for (int i = lo; i < hi; ++i) {
        ViewDesc& v = dev[i - lo];
        v = c->run.views[i];
        v.seg_off += base;
        kinds.simple = kinds.simple && v.unit_scale && v.seg_row_bytes;
        kinds.coarse = kinds.coarse && v.coarse_row_bytes;
        double pl[kCullStride * kCullPlanes];
        cull_planes(v, pl);
        for (int k = 0; k < kCullStride * kCullPlanes; ++k) planes[(size_t)k * pitch + (i - lo)] = pl[k];
    }
    return kinds;
}

// Host descriptors -> device: the map's absolute address goes into the device copy (one scalar add less per view
// and wave), the culling planes are derived here.  Staged through pinned memory owned by the ctx and guarded by an
// event, so nothing waits for the stream: the maps that vote_view queued keep flowing while this is prepared.
static int sync_views(Ctx* c) {
    if (const int rc = vote_flush_pending(c)) return rc;  // every consumer of the views comes through here
    if (!c->run.views_dirty) return GSX_OK;
    const size_t nv = c->run.views.size();
    const size_t bytes = sizeof(ViewDesc) * (nv ? nv : 1);
    GSX_HIP(c, c->run.d_views.ensure(bytes));
    c->run.views_simple = c->run.views_coarse = false;  // no views: nothing to be simple about
    if (nv) {
        const int pitch = (int)((nv + 63) / 64 * 64);
        const size_t plane_doubles = (size_t)kCullStride * kCullPlanes * pitch;
        const size_t need = bytes + sizeof(double) * plane_doubles;
        GSX_HIP(c, c->hstage.views_ev.wait());  // the previous upload has left the buffer
        GSX_HIP(c, c->hstage.views.ensure(need, need * 2));
        ViewDesc* dev = c->hstage.views.as<ViewDesc>();
        double* planes = reinterpret_cast<double*>(c->hstage.views.as<char>() + bytes);
        std::memset(planes, 0, sizeof(double) * plane_doubles);
        const ViewKinds kinds = stage_views(c, 0, (int)nv, c->run.pool_base ? c->run.pool_base : c->run.segpool.p, dev, planes, (size_t)pitch);
        c->run.views_simple = kinds.simple;
        c->run.views_coarse = kinds.coarse;
        GSX_HIP(c, c->run.d_cull.ensure(sizeof(double) * plane_doubles));
        GSX_HIP(c, hipMemcpyAsync(c->run.d_views.p, dev, bytes, hipMemcpyHostToDevice, c->stream));
        GSX_HIP(c, hipMemcpyAsync(c->run.d_cull.p, planes, sizeof(double) * plane_doubles, hipMemcpyHostToDevice, c->stream));
        GSX_HIP(c, c->hstage.views_ev.record(c->stream));
        c->run.cull_pitch = pitch;
        if (const int rc = ensure_tally(c)) return rc;
    }
    c->run.views_dirty = false;
    return GSX_OK;
}

static int ensure_planes(Ctx* c) {
    const size_t esz = c->run.wide ? 2 : 1;
    const size_t bytes = (size_t)c->run.bins * (size_t)c->run.n_pad * esz;
    const bool grew = bytes > c->planes.cnt.cap || bytes > c->planes.fv.cap;
    c->planes.counts = PlaneLayout{};  // cnt is about to hold planes of this layout: the next vote_flush_counts clears its pad entries again
    GSX_HIP(c, c->planes.cnt.ensure(bytes ? bytes : 4));
    GSX_HIP(c, c->planes.fv.ensure(bytes ? bytes : 4));
    if (grew || !c->planes.holds()) {
        GSX_HIP(c, hipMemsetAsync(c->planes.cnt.p, 0, bytes, c->stream));
        GSX_HIP(c, hipMemsetAsync(c->planes.fv.p, 0, bytes, c->stream));
        c->planes.state = PlaneState::Zero;
    }
    return GSX_OK;
}

// After a rewind the planes still hold the previous run's votes ("stale"): the next flush overwrites every
// element of every Gaussian with its first batch, so nothing is cleared up front (2 x 453 MB of memset per
// step at C3).  Anything that reads the planes before such a flush clears them here.
static int clear_stale_planes(Ctx* c) {
    if (c->planes.state != PlaneState::Stale) return GSX_OK;
    const size_t bytes = (size_t)c->run.bins * (size_t)c->run.n_pad * (c->run.wide ? 2 : 1);
    GSX_HIP(c, hipMemsetAsync(c->planes.cnt.p, 0, bytes, c->stream));
    GSX_HIP(c, hipMemsetAsync(c->planes.fv.p, 0, bytes, c->stream));
    c->planes.state = PlaneState::Zero;
    return GSX_OK;
}

int vote_rewind(Ctx* c) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_rewind before vote_begin");
    GSX_HIP(c, hipSetDevice(c->device));
    c->run.n_flushed = 0;
    c->run.labels_valid = false;
    c->early.drop();  // a rewound run is voted in one piece (its views are all there)
    if (const int rc = early_join(c)) return rc;  // ... behind whatever the early stage is still doing to bcnt / ecnt / erec
    if (c->planes.state == PlaneState::Votes) c->planes.state = PlaneState::Stale;  // cleared lazily, see clear_stale_planes
    return GSX_OK;
}

template <class K>
static int set_lds(Ctx* c, K kernel, size_t bytes) {
    if (bytes > 160 * 1024) return fail(c, GSX_E_UNSUPPORTED, "vote: %zu B of LDS per workgroup exceeds 160 KiB", bytes);
    GSX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)bytes));
    return GSX_OK;
}

static constexpr int kUnroll = 8;

// One launch of a kernel that walks p's views over n Gaussians with a histogram row of p.stride_dw dwords per thread in LDS:
// k(p, p.views, args...) on stream st, timed as `name` when profiling is on.
template <class K, class... Args>
static int launch_walk(Ctx* c, const char* name, hipStream_t st, K k, long long n, const FusedParams& p, Args... args) {
    const size_t lds = (size_t)kBlock * p.stride_dw * 4;
    const int rc = set_lds(c, k, lds);
    if (rc) return rc;
    ProfScope ps(c, name, st);
    hipLaunchKernelGGL(k, dim3(grid_for(n)), dim3(kBlock), lds, st, p, p.views, args...);
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}
// bytes of keys / labels: int32 [n_pad], never an empty buffer
static inline size_t label_bytes(const Ctx* c) { return sizeof(int) * (size_t)(c->run.n_pad ? c->run.n_pad : 1); }

// ---- early vote ---------------------------------------------------------------------------------------------------
// A run is the hand-over of its maps (the host pass over them, ~37 us per 1080p map) followed by the vote over all of
// them (~1.2 ms for 3 M Gaussians x 200 views) with the GPU idle during the first and the host during the second.
// When enough of the announced views are staged (`early_vote_at` permille, or a split chosen from the hand-over rate), their
// vote starts on a second stream (vote_fused_planes_kernel into ecnt / efv: counts and first-view codes per bin, plus the
// record of every vote) while the host goes on packing; what vote_finalize still has to do behind the last map is the walk
// over the remaining views plus one pass over the two planes (vote_fused_final_kernel).  Same labels, bit for bit: the
// planes keep everything the tie rule needs.  (Option early_replay: record only + replay, see vote_record_kernel.)
// More than 255 announced views: early_batch_stage starts the batches' count kernels one by one.
// Only where it pays and is simple: one rank holds all views of the run, they arrive one by one through gsx_vote_view, the
// branchless projection is on.  Anything else (rewind, flush, exchange protocols, a pool that had to move) ignores the
// early results and votes all views in one piece as before.
static constexpr int kEarlyPitch = 256;                    // views per block of culling planes (>= kMaxBatch)
static constexpr long long kEarlyMinGaussians = 1 << 18;   // below this the vote is too short to be worth a second stream
static constexpr int kEarlyMinViews = 32;
static constexpr double kEarlyUsPerGaussianView = 4.4e-6;  // early stage on MI355X: 1.6 ms for 3 M Gaussians x 140 views, + 15 %
static constexpr double kRecordUsPerGaussianView = 1.7e-6;  // record-only stage (early_replay): 0.62 ms for the same, + 15 %
static constexpr size_t kEarlySlack = 64 * 260;           // the last stage reads whole groups of four rows, up to row 4 * kRegRows - 1, whatever the bin count
static constexpr size_t kEarlyCullDoubles = (size_t)kCullStride * kCullPlanes * kEarlyPitch;

static bool early_common(const Ctx* c) {
    return c->vopt.early_vote && c->run.first_view == 0 && !c->run.local_codes && c->run.slabs == 1 && c->run.n_flushed == 0 && !c->run.pool_base &&
           c->vopt.flat_project && c->n > 0 && c->run.bins <= 255 &&
           (c->vopt.early_vote == 2 || (c->n >= kEarlyMinGaussians && c->run.total_views >= kEarlyMinViews));
}
static bool early_possible(const Ctx* c) { return early_common(c) && c->run.total_views <= kMaxBatch && !c->run.wide; }
// more than 255 announced views: the batches of labels_batched() (cut by the ANNOUNCED number of views) start their count
// kernels on the second stream as soon as their views are staged; only the last batch, the totals and the tie walk are
// left behind the last map
static bool early_batched_possible(const Ctx* c) { return early_common(c) && c->run.total_views > kMaxBatch && c->vopt.batched_counts; }
// The early batches: a short LAST batch (its count kernel is what stays behind the last map) after balanced ones of <= 255
// views.  Any cut of the view order into consecutive batches gives the same labels (the earliest batch wins a tie).
static int early_batch_count(int total) {
    const int tail = std::min(std::max(total / 16, 16), 64), body = total - tail;
    return (body + kMaxBatch - 1) / kMaxBatch + 1;
}
static void early_batch_bounds(int total, int s, int& lo, int& hi) {
    const int tail = std::min(std::max(total / 16, 16), 64), body = total - tail;
    const int Sb = (body + kMaxBatch - 1) / kMaxBatch;
    if (s >= Sb) {
        lo = body;
        hi = total;
    } else {
        lo = (int)((long long)body * s / Sb);
        hi = (int)((long long)body * (s + 1) / Sb);
    }
}

// Descriptors and culling planes of the views [lo, hi) -> e_views[lo..hi), culling block `block` of e_cull, on stream st.
// dm: the projection variant these views allow.
static int early_upload(Ctx* c, int lo, int hi, int block, int blocks, hipStream_t st, int* dm) {
    const size_t vbytes = sizeof(ViewDesc) * kEarlyPitch, cbytes = sizeof(double) * kEarlyCullDoubles;
    GSX_HIP(c, c->early.h_stage.ensure(vbytes + cbytes));
    // sized for the whole run at its first stage: a later stage must find the earlier ones' descriptors and planes in place
    GSX_HIP(c, c->early.e_views.ensure(sizeof(ViewDesc) * (size_t)std::max(kEarlyPitch, c->run.total_views)));
    GSX_HIP(c, c->early.e_cull.ensure(cbytes * (size_t)std::max(2, blocks)));
    GSX_HIP(c, c->early.up_ev.wait());  // the previous upload has left the staging buffer
    ViewDesc* hv = c->early.h_stage.as<ViewDesc>();  // the stage's views, at most kEarlyPitch
    double* planes = reinterpret_cast<double*>(c->early.h_stage.as<char>() + vbytes);
    std::memset(planes, 0, cbytes);
    const ViewKinds kinds = stage_views(c, lo, hi, c->run.segpool.p, hv, planes, kEarlyPitch);  // (early_common: no imported pool)
    *dm = flat_div_mode(c, kinds.simple, kinds.coarse);
    if (hi > lo) GSX_HIP(c, hipMemcpyAsync(c->early.e_views.as<ViewDesc>() + lo, hv, sizeof(ViewDesc) * (size_t)(hi - lo), hipMemcpyHostToDevice, st));
    GSX_HIP(c, hipMemcpyAsync(c->early.e_cull.as<double>() + (size_t)block * kEarlyCullDoubles, planes, cbytes, hipMemcpyHostToDevice, st));
    GSX_HIP(c, c->early.up_ev.record(st));
    return GSX_OK;
}

static FusedParams early_params(Ctx* c, int lo, int hi, int block, int stride_bytes_per_bin) {
    FusedParams p = fused_params(c, stride_bytes_per_bin);
    p.views = c->early.e_views.as<ViewDesc>() + lo;
    p.nviews = hi - lo;
    p.cull = c->vopt.wave_cull ? c->early.e_cull.as<double>() + (size_t)block * kEarlyCullDoubles : nullptr;
    p.cull_pitch = kEarlyPitch;
    return p;
}

// The context's SECOND stream: the early vote's, and the stream of the first extra frame of gsx_render_views (render.hip borrows
// it: a context never labels and renders at the same time, and a process should not hold more streams than the hardware has
// queues - two streams that share a queue serialise even when the GPU has room).
int second_stream(Ctx* c) {
    if (c->stream2) return GSX_OK;
    // lowest priority: the kernels that expand the maps still arriving (c->stream) get the CUs the stage's waves free first
    int least = 0, greatest = 0;
    GSX_HIP(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
    GSX_HIP(c, hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, least));
    return GSX_OK;
}

// pool_reserve (handover.hip) is about to free the pool an early stage may still be reading: wait for it, and vote this run in one
// piece
int early_pool_moves(Ctx* c) {
    if (c->early.phase == EarlyPhase::Started || c->early.batches > 0) {
        GSX_HIP(c, hipStreamSynchronize(c->stream2));
        c->early.inflight = false;
        c->early.drop();
    }
    return GSX_OK;
}

static int early_batch_stage(Ctx* c) {
    const int nv = (int)c->run.views.size();
    const int S = early_batch_count(c->run.total_views);
    const int s = c->early.batches;
    if (s >= S - 1) return GSX_OK;  // the last batch ends with the last view: vote_finalize launches it
    int lo, hi;
    early_batch_bounds(c->run.total_views, s, lo, hi);
    if (nv != hi) return GSX_OK;
    int rc = vote_flush_pending(c);
    if (rc) return rc;
    if ((rc = second_stream(c))) return rc;
    const size_t plane = (size_t)c->run.bins * (size_t)c->run.n_pad;
    GSX_HIP(c, c->planes.bcnt.ensure(plane * S));  // all batches at the first stage: a later one must find the earlier planes in place
    if ((rc = ensure_tally(c))) return rc;
    GSX_HIP(c, c->early.maps_ev.record(c->stream));
    GSX_HIP(c, c->early.maps_ev.stream_wait(c->stream2));
    int dm = kDivFlat;
    if ((rc = early_upload(c, lo, hi, s, S, c->stream2, &dm))) return rc;
    const FusedParams p = early_params(c, lo, hi, s, 1);
    auto k = with_div<true>(dm, [](auto d) { return vote_fused_counts_kernel<kUnroll, decltype(d)::value>; });
    if ((rc = launch_walk(c, "vote_early_counts", c->stream2, k, c->n, p, c->planes.bcnt.as<uint8_t>() + plane * s, (long long)c->run.n_pad))) return rc;
    GSX_HIP(c, c->early.done_ev.record(c->stream2));
    c->early.inflight = true;
    c->early.batches = s + 1;
    c->early.done = hi;
    return GSX_OK;
}

static int early_vote_stage(Ctx* c) {
    if (c->early.phase == EarlyPhase::Idle && early_batched_possible(c)) return early_batch_stage(c);
    if (c->early.phase != EarlyPhase::Idle || !early_possible(c)) return GSX_OK;
    const int nv = (int)c->run.views.size();
    int at;
    if (c->vopt.early_at > 0) {
        at = std::max(1, (int)(((long long)c->run.total_views * c->vopt.early_at + 999) / 1000));
        if (nv != at) return GSX_OK;
    } else {
        // The split that lets the stage finish just as the last map arrives: it walks a view in about kEarlyUsPerGaussianView * n
        // microseconds, the caller hands over a map every t_map (measured on this run's own calls) - so E / V = t_map / (t_map +
        // that).  Kept between one half and 88 % of the announced views; the stage starts at the first call past it.
        const auto now = std::chrono::steady_clock::now();
        if (nv == 1) c->early.t0 = now;
        if (nv < std::max(8, c->run.total_views / 4)) return GSX_OK;
        const double t_map = std::chrono::duration<double, std::micro>(now - c->early.t0).count() / (double)(nv - 1);
        const double t_view = (c->vopt.early_replay ? kRecordUsPerGaussianView : kEarlyUsPerGaussianView) * (double)c->n;
        const int lo = (c->run.total_views + 1) / 2, hi = (int)(((long long)c->run.total_views * 880) / 1000);
        const int want = std::min(std::max((int)std::ceil(c->run.total_views * t_map / (t_map + t_view)), lo), std::max(lo, hi));
        if (nv < want) return GSX_OK;
        at = nv;
    }
    if (at >= c->run.total_views) return GSX_OK;
    int rc = vote_flush_pending(c);  // the maps of these views are on their way on c->stream
    if (rc) return rc;
    if ((rc = second_stream(c))) return rc;
    const size_t plane = (size_t)c->run.bins * (size_t)c->run.n_pad;
    if (!c->vopt.early_replay) {
        GSX_HIP(c, c->early.ecnt.ensure(plane + kEarlySlack));
        GSX_HIP(c, c->early.efv.ensure(plane + kEarlySlack));
    }
    GSX_HIP(c, c->early.erec.ensure((size_t)c->run.n_pad * (size_t)at));
    if ((rc = ensure_tally(c))) return rc;
    GSX_HIP(c, c->early.maps_ev.record(c->stream));
    GSX_HIP(c, c->early.maps_ev.stream_wait(c->stream2));
    int dm = kDivFlat;
    if ((rc = early_upload(c, 0, at, 0, 2, c->stream2, &dm))) return rc;
    c->early.replayed = c->vopt.early_replay != 0;  // (read once early.phase says that a stage has started)
    if (c->early.replayed) {  // record only (no LDS): the last stage replays it
        const FusedParams p = early_params(c, 0, at, 0, 1);
        auto kr = with_div<true>(dm, [](auto d) { return vote_record_kernel<kUnroll, decltype(d)::value>; });
        ProfScope ps(c, "vote_early_record", c->stream2);
        hipLaunchKernelGGL(kr, dim3(grid_for(c->n)), dim3(kBlock), 0, c->stream2, p, p.views, c->early.erec.as<uint8_t>());
        GSX_HIP(c, hipGetLastError());
    } else {
        const FusedParams p = early_params(c, 0, at, 0, 2);
        auto k = with_div<true>(dm, [](auto d) { return vote_fused_planes_kernel<kUnroll, uint8_t, decltype(d)::value>; });
        // fresh planes, one "slab" per wave (sn = 64: the wave-major layout the last stage streams), global view codes 255 - v
        if ((rc = launch_walk(c, "vote_early_planes", c->stream2, k, c->n, p, c->early.ecnt.as<uint8_t>(), c->early.efv.as<uint8_t>(), 64LL, 0, 1, 0,
                              c->early.erec.as<uint8_t>())))
            return rc;
    }
    GSX_HIP(c, c->early.done_ev.record(c->stream2));
    c->early.inflight = true;
    c->early.done = at;
    c->early.phase = EarlyPhase::Started;
    return GSX_OK;
}

int vote_view(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, int seg_w, int seg_h, int img_w, int img_h) {
    const int rc = vote_view_host(c, cam, seg, seg_dtype, seg_w, seg_h, img_w, img_h);
    return rc ? rc : early_vote_stage(c);  // enough of the run staged: its first views are voted while the rest is handed over
}

// vote_finalize behind an early stage: the views [early_done, nv) on top of the early planes -> c->planes.labels
static int early_vote_finish(Ctx* c) {
    const int nv = (int)c->run.views.size();
    int rc = vote_flush_pending(c);
    if (rc) return rc;
    int dm = kDivFlat;
    if ((rc = early_upload(c, c->early.done, nv, 1, 2, c->stream, &dm))) return rc;
    GSX_HIP(c, c->planes.labels.ensure(label_bytes(c)));
    if (c->early.replayed) {
        FusedParams pr = early_params(c, c->early.done, nv, 1, 1);
        auto kr = with_div<true>(dm, [](auto d) { return vote_fused_replay_kernel<kUnroll, decltype(d)::value>; });
        if ((rc = early_join(c))) return rc;
        if ((c->vopt.ablate >> 4) & 2) pr.nviews = 0;  // timing experiment (tools/early_probe.py)
        return launch_walk(c, "vote_fused_replay", c->stream, kr, c->n, pr, c->early.erec.as<uint8_t>(), c->early.done, c->planes.labels.as<int>());
    }
    FusedParams p = early_params(c, c->early.done, nv, 1, 1);
    const size_t lds = (size_t)(kBlock / 64) * ((c->run.bins + 3) / 4) * 256;  // per wave: [bin][64] bytes, rows padded to a multiple of four
    constexpr int kRegRows = 38;  // bins <= 152 (the 150 ADE20K classes + unlabelled): the first-view rows wait in registers
    const bool regs = c->run.bins <= 4 * kRegRows;
    auto k = with_div<true>(dm, [&](auto d) {
        constexpr int kDiv = decltype(d)::value;
        return regs ? vote_fused_final_kernel<kUnroll, kDiv, kRegRows> : vote_fused_final_kernel<kUnroll, kDiv, 0>;
    });
    if ((rc = set_lds(c, k, lds))) return rc;
    if ((rc = early_join(c))) return rc;
    // timing experiments (results invalid), option "ablate": 16 every wave reads the planes of wave 0; 32 no views behind the
    // early ones; 64 no pass over the first-view rows; 128 no look-up in the vote record; 256 labels stored in Morton order;
    // 512 no wave-level culling
    const int ablate = (c->vopt.ablate >> 4) & 63;
    if (ablate & 2) p.nviews = 0;
    ProfScope ps(c, "vote_fused_final");
    hipLaunchKernelGGL(k, dim3(grid_for(c->n)), dim3(kBlock), lds, c->stream, p, p.views, c->early.ecnt.as<uint8_t>(), c->early.efv.as<uint8_t>(),
                       c->early.erec.as<uint8_t>(), c->early.done, c->planes.labels.as<int>(), ablate);
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

// merge views [n_flushed, size) into the planes, kMaxBatch at a time
int vote_flush(Ctx* c) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_flush before vote_begin");
    GSX_HIP(c, hipSetDevice(c->device));
    int rc = early_join(c);
    if (rc) return rc;
    if ((rc = sync_views(c))) return rc;
    if ((rc = ensure_planes(c))) return rc;
    const int nv = (int)c->run.views.size();
    if (c->n <= 0 || c->run.n_flushed >= nv) {
        c->run.n_flushed = nv;
        return clear_stale_planes(c);  // nothing will overwrite them
    }
    const FusedParams all = fused_params(c, 2);
    while (c->run.n_flushed < nv) {
        const int batch = std::min(kMaxBatch, nv - c->run.n_flushed);
        FusedParams p = all;
        p.views = all.views + c->run.n_flushed;
        p.nviews = batch;
        if (p.cull) p.cull = all.cull + c->run.n_flushed;
        const int view_base = c->run.first_view + c->run.n_flushed;
        const int fresh = (c->planes.state == PlaneState::Zero || c->planes.state == PlaneState::Stale) ? 1 : 0;
        auto planes = [&](auto t) {  // PT = the planes' element: u16 only when `wide` (then never local codes, vote_begin)
            using PT = decltype(t);
            auto k = with_div(div_mode(c), [](auto d) { return vote_fused_planes_kernel<kUnroll, PT, decltype(d)::value>; });
            return launch_walk(c, "vote_fused_planes", c->stream, k, c->n, p, c->planes.cnt.as<PT>(), c->planes.fv.as<PT>(), (long long)c->run.sn, view_base,
                               fresh, c->run.local_codes ? 1 : 0, (uint8_t*)nullptr);
        };
        if ((rc = c->run.wide ? planes(uint16_t{}) : planes(uint8_t{}))) return rc;
        c->planes.state = PlaneState::Votes;
        c->run.n_flushed += batch;
    }
    return GSX_OK;
}

int vote_tiebreak_keys(Ctx* c) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_tiebreak_keys before vote_begin");
    GSX_HIP(c, hipSetDevice(c->device));
    int rc = ensure_planes(c);
    if (rc) return rc;
    if ((rc = clear_stale_planes(c))) return rc;
    GSX_HIP(c, c->planes.keys.ensure(label_bytes(c)));
    GSX_HIP(c, hipMemsetAsync(c->planes.keys.p, 0, sizeof(int) * (size_t)c->run.n_pad, c->stream));
    if (c->n <= 0) return GSX_OK;
    ProfScope ps(c, "vote_keys");
    auto keys = [&](auto t) {
        using PT = decltype(t);
        hipLaunchKernelGGL(vote_keys_kernel<PT>, dim3(grid_for(c->n)), dim3(kBlock), 0, c->stream, c->planes.cnt.as<PT>(), c->planes.fv.as<PT>(),
                           (long long)c->n, (long long)c->run.sn, c->run.bins, c->planes.keys.as<int>());
    };
    c->run.wide ? keys(uint16_t{}) : keys(uint8_t{});
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

// Last step of every protocol: the labels (and the device-side range flag) to the host.  A label is -1 .. 254, so it
// crosses PCIe as ONE byte (bin = label + 1; labels_narrow_kernel, 3 MB instead of 12 MB for 3 M Gaussians: the D2H is
// on the critical path of every run) into pinned memory, in kLabelChunks pieces; the worker threads widen piece i into
// the caller's (pageable) int32 array while piece i+1 is still on the link.  A map that gsx_vote_view_device packed
// with a label out of range fails the call here.
static constexpr int kBadLabelWord = -2;  // errflag value: c->planes.labels held something that is not a label (never a view index)
__global__ __launch_bounds__(kBlock) void labels_narrow_kernel(const int* __restrict__ labels, long long n, uint8_t* __restrict__ out,
                                                               int* __restrict__ errflag) {
    const long long i4 = ((long long)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (i4 >= n) return;
    unsigned b[4];
    if (i4 + 4 <= n) {
        const int4 v = *reinterpret_cast<const int4*>(labels + i4);
        b[0] = (unsigned)v.x + 1u, b[1] = (unsigned)v.y + 1u, b[2] = (unsigned)v.z + 1u, b[3] = (unsigned)v.w + 1u;
        if ((b[0] | b[1] | b[2] | b[3]) > 255u) atomicMin(errflag, kBadLabelWord);
        *reinterpret_cast<uint32_t*>(out + i4) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    } else {
        for (long long i = i4; i < n; ++i) {
            const unsigned bb = (unsigned)labels[i] + 1u;
            if (bb > 255u) atomicMin(errflag, kBadLabelWord);
            out[i] = (uint8_t)bb;
        }
    }
}

static int labels_to_host(Ctx* c, int32_t* labels_out) {
    c->run.labels_valid = true;
    const size_t n = labels_out && c->n > 0 ? (size_t)c->n : 0;
    const size_t esz = c->vopt.labels_u8 ? 1 : sizeof(int);  // bytes per label on the link ("labels_u8" = 0: the A/B of DESIGN.md)
    const size_t nbytes = n * esz;
    const size_t flag_off = (nbytes + 63) / 64 * 64;
    const size_t need = flag_off + 64;
    GSX_HIP(c, c->hstage.labels.ensure(need, need + need / 8));
    char* land = c->hstage.labels.as<char>();
    int* flag = reinterpret_cast<int*>(land + flag_off);
    const char* src = c->planes.labels.as<char>();
    if (n && c->vopt.labels_u8) {
        GSX_HIP(c, c->planes.labels8.ensure(align256(n)));
        ProfScope ps(c, "labels_narrow");
        hipLaunchKernelGGL(labels_narrow_kernel, dim3(grid_for((long long)(n + 3) / 4)), dim3(kBlock), 0, c->stream, c->planes.labels.as<int>(),
                           (long long)n, c->planes.labels8.as<uint8_t>(), c->run.errflag.as<int>());
        GSX_HIP(c, hipGetLastError());
        src = c->planes.labels8.as<char>();
    }
    GSX_HIP(c, hipMemcpyAsync(flag, c->run.errflag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (n) {
        const int chunks = nbytes >= ((size_t)1 << 20) ? kLabelChunks : 1;
        const size_t per = ((n + chunks - 1) / chunks + 4095) / 4096 * 4096;  // labels per chunk
        for (int k = 0; k < chunks; ++k) {
            const size_t lo = std::min(n, per * k), hi = std::min(n, per * (k + 1));
            if (lo < hi) GSX_HIP(c, hipMemcpyAsync(land + lo * esz, src + lo * esz, (hi - lo) * esz, hipMemcpyDeviceToHost, c->stream));
            GSX_HIP(c, c->hstage.labels_ev[k].record(c->stream));
        }
        Workers* w = host_workers(c);
        for (int k = 0; k < chunks; ++k) {
            const size_t lo = std::min(n, per * k), hi = std::min(n, per * (k + 1));
            GSX_HIP(c, c->hstage.labels_ev[k].wait());
            if (lo >= hi) continue;
            if (c->vopt.labels_u8) host_widen_labels(w, labels_out + lo, reinterpret_cast<const uint8_t*>(land) + lo, hi - lo);
            else host_copy(w, labels_out + lo, land + lo * esz, (hi - lo) * esz);
        }
    }
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    if (*flag != kNoBadView) {
        const int view = *flag;
        GSX_HIP(c, hipMemsetAsync(c->run.errflag.p, 0x7f, sizeof(int), c->stream));
        if (view == kBadLabelWord)
            return fail(c, GSX_E_STATE, "the label buffer holds a value outside [-1, 254] (a corrupt exchange buffer?)");
        return fail(c, GSX_E_RANGE, "the segmentation map of view %d (gsx_vote_view_device) holds a label outside [-1, %d]", view,
                    c->run.n_classes - 1);
    }
    return GSX_OK;
}

void vote_release_host(Ctx* c) {  // gsx_destroy: the second stream goes before the first
    if (!c->stream2) return;
    (void)hipStreamSynchronize(c->stream2);
    (void)hipStreamDestroy(c->stream2);
    c->stream2 = nullptr;
}

int vote_labels_from_keys(Ctx* c, int32_t* labels_out) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_labels_from_keys before vote_begin");
    if (c->planes.keys.cap < sizeof(int) * (size_t)c->run.n_pad) return fail(c, GSX_E_STATE, "vote_labels_from_keys before vote_tiebreak_keys");
    GSX_HIP(c, hipSetDevice(c->device));
    GSX_HIP(c, c->planes.labels.ensure(label_bytes(c)));
    if (c->n > 0) {
        ProfScope ps(c, "vote_labels");
        hipLaunchKernelGGL(vote_labels_kernel, dim3(grid_for(c->n)), dim3(kBlock), 0, c->stream, c->planes.keys.as<int>(),
                           (long long)c->n, c->sorted ? c->perm.as<uint32_t>() : nullptr, c->planes.labels.as<int>());
        GSX_HIP(c, hipGetLastError());
    }
    return labels_to_host(c, labels_out);
}

// A contiguous range of the Gaussians in upload (Morton) order: the whole scene for a single GPU, one rank's slab in
// exchange protocol v4.
struct VoteRange {
    long long i0, n;
};
static FusedParams range_params(Ctx* c, const VoteRange& r, int stride_bytes_per_bin) {
    FusedParams p = fused_params(c, stride_bytes_per_bin);
    p.x += r.i0;
    p.y += r.i0;
    p.z += r.i0;
    p.n = r.n;
    p.perm = nullptr;
    return p;
}

// <= 255 staged views: labels straight out of the fused kernel.  perm == nullptr: out[i] = label of Gaussian i0 + i
// (Morton order); otherwise out[perm[i0 + i]] (the caller's order).
static int labels_one_batch(Ctx* c, const VoteRange& r, const uint32_t* perm, int* out) {
    if (r.n <= 0) return GSX_OK;
    FusedParams p = range_params(c, r, 1);
    p.perm = perm ? perm + r.i0 : nullptr;
    // kernel variants: unroll U in {2,4,8} x division mode
    using K = void (*)(FusedParams, const ViewDesc*, int*);
    const int ui = c->vopt.vote_unroll == 2 ? 0 : c->vopt.vote_unroll == 4 ? 1 : 2;
    K k = with_div(div_mode(c), [ui](auto d) {
        constexpr int kDiv = decltype(d)::value;
        static const K by_unroll[3] = {vote_fused_labels_kernel<2, kDiv>, vote_fused_labels_kernel<4, kDiv>, vote_fused_labels_kernel<8, kDiv>};
        return by_unroll[ui];
    });
    return launch_walk(c, "vote_fused_labels", c->stream, k, r.n, p, out);
}

// More than 255 views on one GPU (the reference's own cameras.json holds 311): the views are cut into S balanced
// batches of <= 255 that play the ranks of exchange protocol v3 on a single device.  Every batch is one launch of the
// fast u8-histogram walk (vote_fused_counts_kernel) into its own count plane; vote_slab_totals_kernel sums the S
// planes per bin (unique maximum -> label, else a candidate mask); vote_tie_kernel walks each batch forward for the
// tied Gaussians and vote_tie_resolve_kernel takes the earliest batch that voted a candidate = the earliest view,
// which is the reference's first-inserted rule (dls.py:303).  Replaces the 16-bit count + first-view planes of
// vote_flush() for this case (1.9 ms per 200 views at C3 sizes against 1.1 ms).
// Leaves the range's labels in Morton order at c->planes.keys[0 .. r.n).
static int labels_batched(Ctx* c, const VoteRange& r) {
    const int nv = (int)c->run.views.size();
    // batches whose count kernels already ran on the second stream while the run's later maps were handed over (early_batch_stage:
    // same batches - the run brought exactly the announced views -, same planes, the whole scene)
    const bool early = c->early.batches > 0 && c->early.phase == EarlyPhase::Idle && early_batched_possible(c) && nv == c->run.total_views && r.i0 == 0 &&
                       r.n == c->n;
    const int S = early ? early_batch_count(nv) : (nv + kMaxBatch - 1) / kMaxBatch;
    const long long npad = (r.n + 255) / 256 * 256;
    const size_t plane = (size_t)c->run.bins * (size_t)npad;
    GSX_HIP(c, c->planes.bcnt.ensure(plane * S));
    GSX_HIP(c, c->planes.cand.ensure(sizeof(uint32_t) * kCandWords * (size_t)npad));
    GSX_HIP(c, c->planes.bcodes.ensure(sizeof(uint16_t) * (size_t)npad * S));
    if (r.n <= 0) return GSX_OK;
    auto k = with_div(div_mode(c), [](auto d) { return vote_fused_counts_kernel<kUnroll, decltype(d)::value>; });
    const FusedParams base = range_params(c, r, 1);
    auto batch = [&](int s, FusedParams& p) {  // views [lo, hi) of batch s: balanced (sizes differ by at most one), or the early cut
        int lo = (int)((long long)nv * s / S), hi = (int)((long long)nv * (s + 1) / S);
        if (early) early_batch_bounds(nv, s, lo, hi);
        p = base;
        p.views = base.views + lo;
        p.nviews = hi - lo;
        if (p.cull) p.cull = base.cull + lo;
    };
    const int s0 = early ? c->early.batches : 0;
    for (int s = s0; s < S; ++s) {
        FusedParams p;
        batch(s, p);
        const int rc = launch_walk(c, "vote_fused_counts", c->stream, k, r.n, p, c->planes.bcnt.as<uint8_t>() + plane * s, npad);
        if (rc) return rc;
    }
    {
        ProfScope ps(c, "vote_slab_totals");
        hipLaunchKernelGGL(vote_slab_totals_kernel, dim3(grid_for(npad / 4)), dim3(kBlock), 0, c->stream, c->planes.bcnt.as<uint8_t>(), S,
                           c->run.bins, npad, c->planes.keys.as<int>(), c->planes.cand.as<uint32_t>());
    }
    for (int s = 0; s < S; ++s) {
        FusedParams p;
        batch(s, p);
        ProfScope ps(c, "vote_tie");
        hipLaunchKernelGGL(vote_tie_kernel, dim3(grid_for(r.n)), dim3(kBlock), 0, c->stream, p, p.views, c->planes.cand.as<uint32_t>(), npad,
                           c->planes.bcodes.as<uint16_t>() + (size_t)npad * s, c->planes.bcodes.as<uint16_t>(), s);
    }
    {
        ProfScope ps(c, "vote_tie_resolve");
        hipLaunchKernelGGL(vote_tie_resolve_kernel, dim3(grid_for(npad)), dim3(kBlock), 0, c->stream, c->planes.bcodes.as<uint16_t>(), S, npad,
                           c->planes.keys.as<int>());
    }
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

// labels of a range of Gaussians over ALL staged views, whatever their number.  to_sorted: leave them in Morton order
// at c->planes.keys[0 .. r.n) (protocol v4); otherwise write c->planes.labels in the caller's order (needs r = the whole scene).
static int labels_for_range(Ctx* c, const VoteRange& r, bool to_sorted) {
    // early or not: an early batch may still be writing its plane of bcnt on the second stream (a run that stopped short of the
    // announced views, a rewind) - the buffers are (re)sized and the kernels launched behind it
    int rc = early_join(c);
    if (rc) return rc;
    if ((rc = sync_views(c))) return rc;
    GSX_HIP(c, c->planes.keys.ensure(label_bytes(c)));
    GSX_HIP(c, c->planes.labels.ensure(label_bytes(c)));
    const uint32_t* perm = c->sorted ? c->perm.as<uint32_t>() : nullptr;
    if ((int)c->run.views.size() <= kMaxBatch)
        return labels_one_batch(c, r, to_sorted ? nullptr : perm, to_sorted ? c->planes.keys.as<int>() : c->planes.labels.as<int>());
    if ((rc = labels_batched(c, r))) return rc;
    if (!to_sorted && r.n > 0) {
        ProfScope ps(c, "vote_labels");
        hipLaunchKernelGGL(unpermute_labels_kernel, dim3(grid_for(r.n)), dim3(kBlock), 0, c->stream, c->planes.keys.as<int>(), r.n, perm,
                           c->planes.labels.as<int>());
        GSX_HIP(c, hipGetLastError());
    }
    return GSX_OK;
}

int vote_finalize(Ctx* c, int32_t* labels_out) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_finalize before vote_begin");
    GSX_HIP(c, hipSetDevice(c->device));
    const int nv = (int)c->run.views.size();
    const bool batched_ok = !c->run.local_codes && c->vopt.batched_counts;
    if (c->early.phase == EarlyPhase::Started && early_possible(c) && nv >= c->early.done && nv <= kMaxBatch) {
        // the first views were voted while the rest was handed over: only the views behind them are left
        int rc = early_vote_finish(c);
        if (rc) return rc;
        return labels_to_host(c, labels_out);
    }
    if (c->run.n_flushed == 0 && (nv <= kMaxBatch || batched_ok)) {
        // nothing in the planes yet: labels come straight out of the fused kernel(s)
        int rc = labels_for_range(c, VoteRange{0, c->n}, false);
        if (rc) return rc;
        return labels_to_host(c, labels_out);
    }
    int rc = vote_flush(c);
    if (rc) return rc;
    if ((rc = vote_tiebreak_keys(c))) return rc;
    return vote_labels_from_keys(c, labels_out);
}

int vote_slab_labels(Ctx* c, int slab, int slabs, int64_t* slab_size) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_slab_labels before vote_begin");
    if (slabs < 1 || slab < 0 || slab >= slabs) return fail(c, GSX_E_INVALID, "vote_slab_labels: slab %d of %d", slab, slabs);
    GSX_HIP(c, hipSetDevice(c->device));
    long long sn = ((c->n + slabs - 1) / slabs + 255) / 256 * 256;
    if (sn == 0) sn = 256;
    if (slab_size) *slab_size = sn;
    const long long i0 = std::min<long long>(c->n, sn * slab);
    const long long cnt = std::min<long long>(c->n - i0, sn);
    if ((long long)sn > c->run.n_pad) {  // tiny scenes: the key buffer must hold one whole slab for the all-gather
        GSX_HIP(c, c->planes.keys.ensure(sizeof(int) * (size_t)sn));
    }
    return labels_for_range(c, VoteRange{i0, cnt}, true);
}

// ---- exchange v3 host side ------------------------------------------------------------------------------------
int vote_flush_counts(Ctx* c) {
    if (!c->run.begun || !c->run.local_codes) return fail(c, GSX_E_STATE, "vote_flush_counts needs vote_begin with the 'exchange_local' option");
    GSX_HIP(c, hipSetDevice(c->device));
    int rc = sync_views(c);
    if (rc) return rc;
    const size_t bytes = (size_t)c->run.bins * (size_t)c->run.n_pad;
    // pad Gaussians stay zero as long as the plane keeps its layout: a context that comes back with another scene, bin count or
    // slab count (or whose buffer held vote_flush's planes in between) would otherwise show the earlier run's counters there
    const PlaneLayout layout{c->n, c->run.n_pad, c->run.sn, c->run.bins};
    if (bytes > c->planes.cnt.cap || !(c->planes.counts == layout)) {
        GSX_HIP(c, c->planes.cnt.ensure(bytes));
        GSX_HIP(c, hipMemsetAsync(c->planes.cnt.p, 0, bytes, c->stream));
        c->planes.counts = layout;
    }
    if (c->n > 0) {
        auto k = with_div(div_mode(c), [](auto d) { return vote_fused_counts_kernel<kUnroll, decltype(d)::value>; });
        if ((rc = launch_walk(c, "vote_fused_counts", c->stream, k, c->n, fused_params(c, 1), c->planes.cnt.as<uint8_t>(), (long long)c->run.sn))) return rc;
    }
    c->run.n_flushed = (int)c->run.views.size();
    return GSX_OK;
}

int vote_slab_totals(Ctx* c, const void* recv_cnt) {
    if (!c->run.begun || !c->run.local_codes) return fail(c, GSX_E_STATE, "vote_slab_totals needs the 'exchange_local' option");
    if (!recv_cnt) return fail(c, GSX_E_INVALID, "vote_slab_totals: NULL argument");
    GSX_HIP(c, hipSetDevice(c->device));
    GSX_HIP(c, c->planes.keys.ensure(sizeof(int) * (size_t)c->run.n_pad));
    GSX_HIP(c, c->planes.cand.ensure(sizeof(uint32_t) * kCandWords * (size_t)c->run.sn));
    ProfScope ps(c, "vote_slab_totals");
    hipLaunchKernelGGL(vote_slab_totals_kernel, dim3(grid_for(c->run.sn / 4)), dim3(kBlock), 0, c->stream, (const uint8_t*)recv_cnt,
                       c->run.slabs, c->run.bins, (long long)c->run.sn, c->planes.keys.as<int>(), c->planes.cand.as<uint32_t>());
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;  // ordered by the ctx stream; nothing waits on the host
}

int vote_tie_codes(Ctx* c, const void* cand_all) {
    if (!c->run.begun || !c->run.local_codes) return fail(c, GSX_E_STATE, "vote_tie_codes needs the 'exchange_local' option");
    if (!cand_all) return fail(c, GSX_E_INVALID, "vote_tie_codes: NULL argument");
    GSX_HIP(c, hipSetDevice(c->device));
    const size_t bytes = sizeof(uint16_t) * (size_t)c->run.n_pad;
    const PlaneLayout layout{c->n, c->run.n_pad};
    if (bytes > c->planes.codes.cap || !(c->planes.tie_codes == layout)) {  // pad entries are zero: see vote_flush_counts
        GSX_HIP(c, c->planes.codes.ensure(bytes));
        GSX_HIP(c, hipMemsetAsync(c->planes.codes.p, 0, bytes, c->stream));
        c->planes.tie_codes = layout;
    }
    if (c->n > 0) {
        FusedParams p = fused_params(c, 1);
        ProfScope ps(c, "vote_tie");
        hipLaunchKernelGGL(vote_tie_kernel, dim3(grid_for(c->n)), dim3(kBlock), 0, c->stream, p, p.views,
                           (const uint32_t*)cand_all, (long long)c->run.sn, c->planes.codes.as<uint16_t>(), (const uint16_t*)nullptr, 0);
        GSX_HIP(c, hipGetLastError());
    }
    return GSX_OK;  // ordered by the ctx stream; nothing waits on the host
}

int vote_tie_resolve(Ctx* c, const void* recv_codes) {
    if (!c->run.begun || !c->run.local_codes) return fail(c, GSX_E_STATE, "vote_tie_resolve needs the 'exchange_local' option");
    if (!recv_codes) return fail(c, GSX_E_INVALID, "vote_tie_resolve: NULL argument");
    GSX_HIP(c, hipSetDevice(c->device));
    ProfScope ps(c, "vote_tie_resolve");
    hipLaunchKernelGGL(vote_tie_resolve_kernel, dim3(grid_for(c->run.sn)), dim3(kBlock), 0, c->stream, (const uint16_t*)recv_codes,
                       c->run.slabs, (long long)c->run.sn, c->planes.keys.as<int>());
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;  // ordered by the ctx stream; nothing waits on the host
}

int vote_slab_reduce(Ctx* c, const void* recv_cnt, const void* recv_fv) {
    if (!c->run.begun || !c->run.local_codes) return fail(c, GSX_E_STATE, "vote_slab_reduce needs vote_begin with the 'exchange_local' option");
    if (!recv_cnt || !recv_fv) return fail(c, GSX_E_INVALID, "vote_slab_reduce: NULL argument");
    GSX_HIP(c, hipSetDevice(c->device));
    GSX_HIP(c, c->planes.keys.ensure(sizeof(int) * (size_t)c->run.n_pad));
    ProfScope ps(c, "vote_slab_reduce");
    hipLaunchKernelGGL(vote_slab_reduce_kernel, dim3(grid_for(c->run.sn)), dim3(kBlock), 0, c->stream, (const uint8_t*)recv_cnt,
                       (const uint8_t*)recv_fv, c->run.slabs, c->run.bins, (long long)c->run.sn, c->planes.keys.as<int>());
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;  // ordered by the ctx stream; nothing waits on the host
}

int vote_labels_from_sorted(Ctx* c, const void* sorted_labels_dev, int32_t* labels_out) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_labels_from_sorted before vote_begin");
    if (!sorted_labels_dev) return fail(c, GSX_E_INVALID, "vote_labels_from_sorted: NULL argument");
    GSX_HIP(c, hipSetDevice(c->device));
    GSX_HIP(c, c->planes.labels.ensure(label_bytes(c)));
    if (c->n > 0) {
        ProfScope ps(c, "vote_labels");
        hipLaunchKernelGGL(unpermute_labels_kernel, dim3(grid_for(c->n)), dim3(kBlock), 0, c->stream,
                           (const int*)sorted_labels_dev, (long long)c->n, c->sorted ? c->perm.as<uint32_t>() : nullptr,
                           c->planes.labels.as<int>());
        GSX_HIP(c, hipGetLastError());
    }
    return labels_to_host(c, labels_out);
}

int vote_debug_planes(Ctx* c, uint16_t* counts_out, uint16_t* first_out) {
    if (!c->run.begun || !c->planes.holds()) return fail(c, GSX_E_STATE, "vote_debug_planes: no planes");
    if (const int rc = clear_stale_planes(c)) return rc;
    if (!counts_out || !first_out) return fail(c, GSX_E_INVALID, "vote_debug_planes: NULL argument");
    GSX_HIP(c, hipSetDevice(c->device));
    const size_t esz = c->run.wide ? 2 : 1;
    const size_t elems = (size_t)c->run.bins * (size_t)c->run.n_pad;
    std::vector<uint8_t> tmp(elems * esz);
    std::vector<uint32_t> perm;
    if (c->sorted && c->n > 0) {
        perm.resize((size_t)c->n);
        GSX_HIP(c, hipMemcpy(perm.data(), c->perm.p, sizeof(uint32_t) * (size_t)c->n, hipMemcpyDeviceToHost));
    }
    for (int which = 0; which < 2; ++which) {
        GSX_HIP(c, hipMemcpyAsync(tmp.data(), which ? c->planes.fv.p : c->planes.cnt.p, elems * esz, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
        uint16_t* out = which ? first_out : counts_out;
        for (int b = 0; b < c->run.bins; ++b)
            for (int64_t i = 0; i < c->n; ++i) {
                const size_t slab = (size_t)i / (size_t)c->run.sn;
                const size_t at = (slab * c->run.bins + b) * (size_t)c->run.sn + ((size_t)i - slab * (size_t)c->run.sn);
                out[(size_t)b * c->n + (perm.empty() ? (size_t)i : (size_t)perm[i])] = c->run.wide ? reinterpret_cast<uint16_t*>(tmp.data())[at] : tmp[at];
            }
    }
    return GSX_OK;
}

}  // namespace gsx
