// render.hip - the frame of the tile-based forward rasterizer for gfx950, bit-faithful to the reference viewer's data path.
//
// Restates Web_Viewer_Gaussians_Selection/gaussians_selection.js ("gs.js"):
//   render_scene.hip                processPlyBuffer, generateTexture, performHitTesting: once per scene
//   render_pre.hip                  runSort's depth keys and buckets, the vertex shader: once per splat per view
//   bin / sort / ranges (here)      the global stable counting sort (gs.js:450-457) becomes two stable
//                                   radix sorts: splats by bucket, then (tile, splat) pairs by tile
//   blend.hip                       fragment shader + blend unit gs.js:782-799, 1036-1038
// Compiled with -ffp-contract=off like the other three (bin_kernel's exact test is tile_test.hpp's, shared with the blend).
//
// HBM layout (per frame in flight: RenderFrame)
//   keys/vals  u32[P]      (tile, splat) pairs emitted in depth order, P = sum of tiles touched
//   ranges     int2[tiles] [start, end) into the sorted pairs
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <thread>

#include "gsx_ctx.hpp"
#include "render_device.hpp"
#include "tile_test.hpp"

namespace gsx {

// ---- exclusive scan of u32 (2 launches: tile sums; downsweep, every workgroup adding up the sums before its own) -----
static constexpr int kScanItems = 16;
static constexpr int kScanTile = kRB * kScanItems;

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wsum /*[4]*/, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t off = 0;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return off + inc - v;
}

__global__ __launch_bounds__(kRB) void scan_sums_kernel(const uint32_t* __restrict__ in, long long n,
                                                         uint32_t* __restrict__ sums) {
    __shared__ uint32_t wsum[4];
    const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) s += in[base + k];
    uint32_t total;
    (void)block_exclusive_scan(s, wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums: one u32 per workgroup (a few hundred): each workgroup re-adds the ones before it instead of a third launch.
// The last workgroup also writes the grand total in 64 bits (the pair count of a close-up view can pass 2^32).  It is exact
// as long as every 4096-entry tile's OWN sum stays below 2^32 (`sums` keeps one u32 per tile; they are added up in 64 bits);
// the offsets are the exclusive sums mod 2^32.
__global__ __launch_bounds__(kRB) void scan_down_kernel(const uint32_t* __restrict__ in, long long n,
                                                         const uint32_t* __restrict__ sums, uint32_t* __restrict__ out,
                                                         unsigned long long* __restrict__ grand) {
    __shared__ uint32_t wsum[4];
    __shared__ unsigned long long wbase[4];
    unsigned long long before = 0;
    for (int t = threadIdx.x; t < (int)blockIdx.x; t += kRB) before += sums[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    if ((threadIdx.x & 63) == 0) wbase[threadIdx.x >> 6] = before;
    __syncthreads();
    const unsigned long long block_base = wbase[0] + wbase[1] + wbase[2] + wbase[3];
    const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    uint32_t v[kScanItems];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = base + k < n ? in[base + k] : 0u;
        s += v[k];
    }
    uint32_t total;
    uint32_t run = (uint32_t)block_base + block_exclusive_scan(s, wsum, total);  // offsets are only used when the total fits 31 bits
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *grand = block_base + total;
}

// ---- binning ---------------------------------------------------------------------------------------------------------
// The reference orders ALL splats by (bucket, index) (stable counting sort, gs.js:450-457).  Level 1 sorts the n splats
// by bucket (16 bits, stable); level 2 emits their (tile, splat) pairs in that order and sorts the pairs by tile only
// (stable): inside a tile the pairs keep the (bucket, index) order.
//
// Wave-cooperative binning.  The 64 splats of a wave (consecutive in depth order) span a list of CANDIDATE tiles: the
// concatenation of their tile rectangles.  The lanes walk that list 64 candidates at a time: a lane finds the splat that
// owns its candidate by a binary search over the wave's candidate offsets (shuffles), derives the tile from the
// candidate's rank inside the rectangle and tests it -
//    * exact: the ellipse |vPosition| <= 2 really reaches the tile (tile_touches), not just its bounding box;
//    * skip:  the tile is not yet opaque (`sat`, written by the blend kernel of the previous depth phase) -
// and one ballot turns the 64 verdicts into a mask from which every splat counts its kept tiles (COUNT) or every kept
// candidate derives its slot in the pair arrays (EMIT: splat's offset + kept candidates of the same splat before it).
// No lane ever loops over a rectangle on its own: a splat covering 4000 tiles costs the wave 63 rounds, not one lane
// 4000, which is what made the exact test a net loss when every thread walked its own rectangle.
// COUNT and EMIT run the same tests on the same data (sat is not written in between), so the slots are exact.
//
// BIN32 (option render_bin32): the candidates are 32x32-pixel BINS (2x2 tiles) instead of tiles.  A pair's key is the bin,
// its value carries in bits 28-31 the mask of the bin's tiles (bit = 2 * (ty & 1) + (tx & 1)) that the splat's rectangle
// covers and that are not opaque yet; the blend kernel of a tile walks its bin's list and takes the entries whose mask names
// it - in list order, so a tile blends exactly the splats, in exactly the order, of the per-tile lists.  A splat's rectangle
// spans about half as many bins as tiles: half the pairs to emit, sort and range.  `tiles_x` is then the bins per row and
// `sat` holds four bytes per bin (bin * 4 + bit), read as one word.
template <bool EMIT, bool BIN32>
__global__ __launch_bounds__(kRB) void bin_kernel(const unsigned long long* __restrict__ nvis_dev, long long div0, long long div1,
                                                   long long m_cap, const uint32_t* __restrict__ by_depth,
                                                   const uint32_t* __restrict__ tile_rect, const float4* __restrict__ rec,
                                                   float H, int tiles_x, int exact,
                                                   const uint8_t* __restrict__ sat, uint32_t* __restrict__ count_out,
                                                   const uint32_t* __restrict__ offset, uint32_t* __restrict__ keys,
                                                   uint32_t* __restrict__ vals, const unsigned long long* __restrict__ total_dev,
                                                   unsigned long long cap, uint32_t* __restrict__ rect_seq) {
    if (EMIT && *total_dev > cap) return;  // the phase does not fit the pair buffers: the host redoes the frame with larger ones
    // the phase's splats: [nvis / div0, nvis / div1) of the depth order, nvis = the splats the level-1 sort kept (on the device:
    // the host never waits for it; the launch covers m_cap >= the phase's length, and COUNT writes every slot of it)
    const long long nvis = (long long)*nvis_dev;
    const long long j0 = div0 ? nvis / div0 : 0, j1 = nvis / div1;
    const long long rel = (long long)blockIdx.x * kRB + threadIdx.x;
    const long long j = j0 + rel;
    const int lane = threadIdx.x & 63;
    const bool live = j < j1;
    const bool slot = rel < m_cap;
    const uint32_t i = live ? by_depth[j] : 0u;
    // COUNT gathers the splat's rectangle (a 4-byte read that costs a whole line) and leaves it in the phase's own order for
    // EMIT (count_out / offset and rect_seq are per-phase arrays of m_cap slots)
    const uint32_t rect = live ? (EMIT ? rect_seq[rel] : tile_rect[i]) : kEmptyRect;
    if (!EMIT && slot) rect_seq[rel] = rect;
    const uint32_t tx0 = rect & 255u, tx1 = (rect >> 8) & 255u, ty0 = (rect >> 16) & 255u, ty1 = rect >> 24;
    constexpr uint32_t kSh = BIN32 ? 1u : 0u;  // candidate = bin: the rectangle in bin units
    const uint32_t w = tx1 >= tx0 ? (tx1 >> kSh) - (tx0 >> kSh) + 1u : 0u;
    const uint32_t area = w * (ty1 >= ty0 ? (ty1 >> kSh) - (ty0 >> kSh) + 1u : 0u);
    // candidate offsets inside the wave: exclusive scan of the areas
    uint32_t inc = area;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    const uint32_t total = __shfl(inc, 63);
    if (total == 0) {  // wave-uniform
        if (!EMIT && slot) count_out[rel] = 0u;
        return;
    }
    const uint32_t cstart = inc - area;
    if (!EMIT && !exact && !sat) {  // wave-uniform: nothing to test, every tile of the rectangle is kept
        if (slot) count_out[rel] = area;  // (a slot past the phase's end: area 0)
        return;
    }
    const bool test = exact && area > 1u;  // a one-tile rectangle holds the centre's tile or touches it by construction
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
    if (test) {
        r0 = rec[3 * (size_t)i];
        r1 = rec[3 * (size_t)i + 1];
    }
    const uint32_t my_off = EMIT && live ? offset[rel] : 0u;
    uint32_t kept_run = 0;  // kept candidates of MY splat in the rounds so far
    // every lane runs every round: the shuffles read registers of ALL lanes; only the stores are predicated
    for (uint32_t base = 0; base < total; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        const bool valid = e < total;
        const uint32_t target = valid ? e : total - 1u;
        int lo = 0, hi = 63;  // the LAST lane whose candidates start at or before `target` (empty splats share their
                              // start with the next non-empty one, which is the later lane)
#pragma unroll
        for (int step = 0; step < 6; ++step) {
            const int mid = (lo + hi + 1) >> 1;
            const uint32_t om = __shfl(cstart, mid);
            if (om <= target) lo = mid;
            else hi = mid - 1;
        }
        const uint32_t s_start = __shfl(cstart, lo);
        const uint32_t s_rect = __shfl(rect, lo);
        const uint32_t s_tx0 = s_rect & 255u, s_tx1 = (s_rect >> 8) & 255u, s_ty0 = (s_rect >> 16) & 255u;
        const uint32_t s_w = (s_tx1 >> kSh) - (s_tx0 >> kSh) + 1u;
        const uint32_t local = target - s_start;
        const uint32_t ry = local / s_w, rx = local - ry * s_w;
        const uint32_t tx = (s_tx0 >> kSh) + rx, ty = (s_ty0 >> kSh) + ry;
        const uint32_t tile = ty * (uint32_t)tiles_x + tx;
        bool keep = valid;
        uint32_t tag = 0u;  // BIN32: the mask of the bin's tiles, in the value's top four bits
        if (BIN32) {
            const uint32_t s_ty1 = s_rect >> 24;
            const uint32_t cx = 2u * tx, cy = 2u * ty;
            const uint32_t xb = (cx >= s_tx0 && cx <= s_tx1 ? 1u : 0u) | (cx + 1u >= s_tx0 && cx + 1u <= s_tx1 ? 2u : 0u);
            uint32_t m = (cy >= s_ty0 && cy <= s_ty1 ? xb : 0u) | (cy + 1u >= s_ty0 && cy + 1u <= s_ty1 ? xb << 2 : 0u);
            if (sat && keep) {
                const uint32_t sw = reinterpret_cast<const uint32_t*>(sat)[tile];
                m &= ~((sw & 0xffu ? 1u : 0u) | (sw & 0xff00u ? 2u : 0u) | (sw & 0xff0000u ? 4u : 0u) | (sw & 0xff000000u ? 8u : 0u));
            }
            keep = keep && m != 0u;
            tag = m << 28;
        }
        if (exact) {  // wave-uniform
            const int s_test = __shfl((int)test, lo);
            const float a0 = __shfl(r0.x, lo), a1 = __shfl(r0.y, lo), a2 = __shfl(r0.z, lo), a3 = __shfl(r0.w, lo);
            const float b0 = __shfl(r1.x, lo), b1 = __shfl(r1.y, lo);
            if (keep && s_test) keep = tile_touches(a0, a1, a2, a3, b0, b1, H, tx, ty);
        }
        if (!BIN32 && sat && keep) keep = sat[tile] == 0;
        if (EMIT && !exact && !sat) {  // wave-uniform fast path: slot = the splat's offset + the candidate's rank in its rectangle
            const uint32_t pos = __shfl(my_off, lo) + local;  // shuffles outside the predicate: every lane must take part
            const uint32_t s_i = __shfl(i, lo);
            if (keep) {
                keys[pos] = tile;
                vals[pos] = s_i | tag;
            }
            continue;
        }
        const unsigned long long verdict = __ballot(keep);
        // bits of this round that belong to my splat: candidates [cstart, cstart + area) shifted by base
        const long long mlo = (long long)cstart - (long long)base, mhi = mlo + (long long)area;
        const int blo = (int)(mlo < 0 ? 0 : (mlo > 64 ? 64 : mlo)), bhi = (int)(mhi < 0 ? 0 : (mhi > 64 ? 64 : mhi));
        const unsigned long long below_hi = bhi >= 64 ? ~0ull : ((1ull << bhi) - 1ull);
        const unsigned long long below_lo = blo >= 64 ? ~0ull : ((1ull << blo) - 1ull);
        const uint32_t mine = (uint32_t)__popcll(verdict & below_hi & ~below_lo);
        if (EMIT) {
            const uint32_t s_prior = __shfl(kept_run, lo);   // kept candidates of the owner in earlier rounds
            const uint32_t s_off = __shfl(my_off, lo);
            const uint32_t s_i = __shfl(i, lo);
            const long long slo = (long long)s_start - (long long)base;
            const int sblo = (int)(slo < 0 ? 0 : slo);        // first bit of the owner in this round (<= lane)
            const unsigned long long upto = (1ull << lane) - 1ull;
            const unsigned long long from = sblo >= 64 ? ~0ull : ((1ull << sblo) - 1ull);
            const uint32_t rank = s_prior + (uint32_t)__popcll(verdict & upto & ~from);
            if (keep) {
                keys[s_off + rank] = tile;
                vals[s_off + rank] = s_i | tag;
            }
        }
        kept_run += mine;
    }
    if (!EMIT && slot) count_out[rel] = kept_run;
}

__global__ __launch_bounds__(kRB) void ranges_kernel(const uint32_t* __restrict__ keys, const unsigned long long* __restrict__ total,
                                                      unsigned long long cap, int ntiles, int2* __restrict__ ranges) {
    const unsigned long long tot = *total;
    const long long P = tot > cap ? 0 : (long long)tot;
    const long long p = (long long)blockIdx.x * kRB + threadIdx.x;
    if (p >= P) return;
    const uint32_t t = keys[p];
    if (t >= (uint32_t)ntiles) return;  // defensive: a key outside the frame must never index the table
    if (p == 0 || keys[p - 1] != t) ranges[t].x = (int)p;
    if (p == P - 1 || keys[p + 1] != t) ranges[t].y = (int)(p + 1);
}

static int exclusive_scan_u32(Ctx* c, const uint32_t* in, uint32_t* out, long long n, unsigned long long* grand_dev) {
    const int m = (int)((n + kScanTile - 1) / kScanTile);
    GSX_HIP(c, c->frame.scan.ensure(sizeof(uint32_t) * (size_t)(m + 1)));
    uint32_t* sums = c->frame.scan.as<uint32_t>();
    {
        ProfScope ps(c, "scan");
        hipLaunchKernelGGL(scan_sums_kernel, dim3(m), dim3(kRB), 0, c->stream, in, n, sums);
        hipLaunchKernelGGL(scan_down_kernel, dim3(m), dim3(kRB), 0, c->stream, in, n, sums, out, grand_dev);
    }
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

// test hooks (gsx_debug_exclusive_scan, gsx_debug_ranges): the scan and the ranges launched as a frame launches them
int debug_exclusive_scan(Ctx* c, const uint32_t* in, uint32_t* out, long long n, unsigned long long* grand_dev) {
    return exclusive_scan_u32(c, in, out, n, grand_dev);
}

int debug_ranges(Ctx* c, const uint32_t* keys, const unsigned long long* total_dev, long long cap, int nlists, int2* ranges) {
    GSX_HIP(c, hipMemsetAsync(ranges, 0, sizeof(int2) * (size_t)nlists, c->stream));
    hipLaunchKernelGGL(ranges_kernel, dim3(grid_for(cap)), dim3(kRB), 0, c->stream, keys, total_dev, (unsigned long long)cap, nlists, ranges);
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

// One depth phase's COUNT -> scan -> EMIT: the ONE place these are launched, for render_view and for the test hook alike
static int launch_bin_phase(Ctx* c, const BinPhaseArgs& a) {
    const int lists_x = a.bin32 ? (a.tiles_x + 1) / 2 : a.tiles_x;
    const auto count_k = a.bin32 ? bin_kernel<false, true> : bin_kernel<false, false>;
    const auto emit_k = a.bin32 ? bin_kernel<true, true> : bin_kernel<true, false>;
    const long long m = a.m_cap;
    {
        ProfScope ps(c, "render_bin_count");
        hipLaunchKernelGGL(count_k, dim3(grid_for(m)), dim3(kRB), 0, c->stream,
                           a.nvis_dev, a.div0, a.div1, m, a.by_depth, a.tile_rect, a.rec, (float)a.H, lists_x,
                           a.exact, a.sat, a.count, (const uint32_t*)nullptr,
                           (uint32_t*)nullptr, (uint32_t*)nullptr, (const unsigned long long*)nullptr, 0ull, a.rect_seq);
    }
    GSX_HIP(c, hipGetLastError());
    const int rc = exclusive_scan_u32(c, a.count, a.offset, m, a.total_dev);
    if (rc) return rc;
    {
        ProfScope ps(c, "render_bin_emit");
        hipLaunchKernelGGL(emit_k, dim3(grid_for(m)), dim3(kRB), 0, c->stream,
                           a.nvis_dev, a.div0, a.div1, m, a.by_depth, a.tile_rect, a.rec, (float)a.H, lists_x,
                           a.exact, a.sat, (uint32_t*)nullptr, a.offset,
                           a.keys, a.vals, a.total_dev, a.pair_cap, a.rect_seq);
    }
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

// test hook (gsx_debug_bin): a depth phase as a frame launches it, in the caller's buffers
int debug_bin(Ctx* c, const BinPhaseArgs& a) { return launch_bin_phase(c, a); }

// One frame.  Per view: pre_kernel (depth keys, vertex shader, colours, tile rectangles), bucket_kernel, the level-1
// sort of the splats by depth bucket; then the splats are rasterized FRONT TO BACK IN DEPTH PHASES (the nearest
// n/r^(K-1) splats, the next ones up to n/r^(K-2), .., the rest): each phase bins its splats into the tiles that are not
// opaque yet (bin_kernel COUNT -> scan -> EMIT), sorts its (tile, splat) pairs by tile, and blends them on top of the
// image, marking the tiles whose every pixel has reached 1 - alpha < 1e-5.  A dense scene sorts a few times the pairs
// the blend really consumes instead of all of them (3 M splats at 1080p: 22 M pairs bounded by the boxes, 2.2 M
// consumed); what is skipped could not have changed any channel by more than 1e-5 (the remaining transmittance bounds
// the sum of everything behind it).
// The host never waits inside a frame: the pair count of a phase stays on the device, the sort / ranges kernels are
// launched for the CAPACITY of the pair buffers and read the count themselves.  Only the end-of-frame read-back tells
// the host whether a phase overflowed the buffers; then they are enlarged and the frame is redone (first frame of a
// scene, or a much closer view).  (render_view is below its three steps.)
//
// The front of a frame, shared with the lift frame (lift.hip), in three steps.  frame_plan: the frame's geometry, the forms the
// options select and the per-frame buffers (allow_bin32 = false, phases = 1: per-tile lists of ALL pairs, what lift_kernel walks).
int frame_plan(Ctx* c, int W, int H, bool allow_bin32, int phases, FramePlan& fp) {
    const int tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16;
    RenderFrame& f = c->frame;
    const RenderOpts& o = c->ropt;
    const int ntiles = tiles_x * tiles_y;
    const long long n = c->scene.rn;
    // 32x32-pixel bins (see bin_kernel): the one-wave blend kernel reads the masks; a value's top four bits are the mask
    const bool bin32 = allow_bin32 && o.bin32 && o.blend_pk2 == 2 && !o.exact_cull && n < (1ll << 28);
    f.bin32 = bin32;
    const int bins_x = (tiles_x + 1) / 2, bins_y = (tiles_y + 1) / 2;
    const int nlists = bin32 ? bins_x * bins_y : ntiles;          // lists the pairs are sorted into
    const size_t sat_bytes = bin32 ? 4 * (size_t)nlists : (size_t)ntiles;
    fp.W = W, fp.H = H, fp.tiles_x = tiles_x, fp.tiles_y = tiles_y, fp.ntiles = ntiles, fp.nlists = nlists;
    fp.bin32 = bin32, fp.sat_bytes = sat_bytes, fp.n = n;
    GSX_HIP(c, f.ranges.ensure(sizeof(int2) * (size_t)nlists));
    GSX_HIP(c, f.sat.ensure(sat_bytes));
    GSX_HIP(c, f.small.ensure(sizeof(FrameCounters)));
    f.P = 0;
    f.consumed = 0;
    if (n <= 0) return GSX_OK;  // no splats at all: nothing else is needed
    const size_t n4 = 4 * (size_t)n;
    fp.ext_pre = f.pre_ext >= 0;  // gsx_render_views ran this frame's pre pass (pre_multi_kernel) into one of the rotating sets
    f.cur = &f.sets[fp.ext_pre ? f.pre_ext : 0];  // a frame on its own uses set 0
    int rc = ensure_pre_set(c, *f.cur, n);
    if (rc) return rc;
    GSX_HIP(c, f.bucket.ensure(n4));
    GSX_HIP(c, f.count.ensure(n4));
    GSX_HIP(c, f.offset.ensure(n4));
    GSX_HIP(c, f.d0.ensure(n4));
    GSX_HIP(c, f.d1.ensure(n4));
    GSX_HIP(c, f.d2.ensure(n4));
    GSX_HIP(c, f.d3.ensure(n4));
    GSX_HIP(c, f.rects.ensure(n4));
    // depth phases: boundaries nvis / r^(K-1), nvis / r^(K-2), .., nvis / r, nvis of the depth order, nvis = the splats the
    // level-1 sort keeps (on the device); the host sizes a phase's launches for n instead
    const int K = std::max(1, std::min(phases, kMaxPhases));
    const long long ratio = std::max(2, std::min(o.phase_ratio, 64));
    long long* divs = fp.divs;  // phase p = [nvis / divs[p], nvis / divs[p + 1]); divs[0] = 0 stands for the start
    divs[0] = 0;
    for (int p = 1; p <= K; ++p) {
        long long div = 1;
        for (int q = p; q < K; ++q) div = std::min<long long>(div * ratio, (long long)1 << 40);
        divs[p] = div;
    }
    int tile_bits = 1;
    while ((1 << tile_bits) < nlists) ++tile_bits;
    // the pair sorts in one pass (2040 bins at 1080p; 4K: 8160, two passes) - for a frame on its own: 6 % less kernel time; with
    // several frames in flight its scattered stores cost the other streams more than the saved launches give (option value 2: always)
    const bool wide = tile_bits <= 11 && (o.wide_sort == 2 || (o.wide_sort == 1 && !f.in_flight));
    if (f.pair_cap == 0) f.pair_cap = std::max<size_t>((size_t)1 << 20, 2 * (size_t)n);
    fp.K = K, fp.tile_bits = tile_bits, fp.wide = wide;
    return GSX_OK;
}

// frame_depth_order, once per attempt at a frame: the pair buffers at their current capacity, the opacity bytes and the counters
// zeroed, the pre pass (unless gsx_render_views ran it), the depth buckets and the level-1 sort.  -> fp.by_depth
int frame_depth_order(Ctx* c, const gsx_camera* cam, FramePlan& fp) {
    RenderFrame& f = c->frame;
    const RenderOpts& o = c->ropt;
    FrameCounters* fc = f.small.as<FrameCounters>();
    const long long n = fp.n;
    int rc;
    const size_t cap = f.pair_cap;
    GSX_HIP(c, f.keys0.ensure(4 * cap));
    GSX_HIP(c, f.keys1.ensure(4 * cap));
    GSX_HIP(c, f.vals0.ensure(4 * cap));
    GSX_HIP(c, f.vals1.ensure(4 * cap));
    GSX_HIP(c, hipMemsetAsync(f.sat.p, 0, fp.sat_bytes, c->stream));
    GSX_HIP(c, hipMemsetAsync(fc, 0, sizeof(FrameCounters), c->stream));
    // (a frame that is redone because a phase overflowed the pair buffers keeps an external pre pass's records)
    if (!fp.ext_pre && (rc = launch_pre(c, cam, fp.W, fp.H, *f.cur))) return rc;
    launch_bucket(c, *f.cur, f.bucket.as<uint32_t>(), f.d0.as<uint32_t>(), f.d1.as<uint32_t>(), &fc->dropped, o.compact);
    GSX_HIP(c, hipGetLastError());
    // level 1: splats by depth bucket (stable)
    int dwhere = 0;
    // (its first pass leaves out the splats bucket_kernel marked: fc->nvis = the ones that remain, sorted, in front)
    rc = radix_sort_pairs_drop(c, f.d0.as<uint32_t>(), f.d1.as<uint32_t>(), f.d2.as<uint32_t>(), f.d3.as<uint32_t>(), n, nullptr, 16,
                               &dwhere, &fc->nvis);
    if (rc) return rc;
    fp.by_depth = dwhere ? f.d3.as<uint32_t>() : f.d1.as<uint32_t>();
    return GSX_OK;
}

// frame_phase_lists, once per depth phase: bin the phase's splats (COUNT -> scan -> EMIT), sort the pairs by list, write the
// lists' ranges.  *vals_sorted: the sorted list entries f.ranges indexes.  The caller has checked that the phase is due
// (n / divs[p + 1] > 0 or the last phase).
int frame_phase_lists(Ctx* c, const FramePlan& fp, int p, int first_phase, const uint32_t** vals_sorted) {
    RenderFrame& f = c->frame;
    const RenderOpts& o = c->ropt;
    FrameCounters* fc = f.small.as<FrameCounters>();
    const size_t cap = f.pair_cap;
    const int nlists = fp.nlists;
    const bool wide = fp.wide;
    int rc;
    const long long m = fp.n / fp.divs[p + 1];  // >= the phase's length nvis / divs[p + 1] - nvis / divs[p]
    unsigned long long* pairs_dev = &fc->pairs[p];
    int where = 0;
    if (m > 0) {
        const BinPhaseArgs bin = {&fc->nvis, fp.divs[p], fp.divs[p + 1], m, fp.by_depth, f.cur->rect.as<uint32_t>(), f.cur->rec.as<float4>(),
                                  fp.H, fp.tiles_x, fp.bin32, o.exact_cull, first_phase ? nullptr : f.sat.as<uint8_t>(),
                                  f.count.as<uint32_t>(), f.offset.as<uint32_t>(), f.rects.as<uint32_t>(), f.keys0.as<uint32_t>(),
                                  f.vals0.as<uint32_t>(), pairs_dev, (unsigned long long)cap};
        if ((rc = launch_bin_phase(c, bin))) return rc;
        if (wide) {  // one pass over the whole key; the digits' bases are the lists' ranges (sort.hip)
            rc = radix_sort_values_wide(c, f.keys0.as<uint32_t>(), f.vals0.as<uint32_t>(), f.vals1.as<uint32_t>(), (long long)cap,
                                        pairs_dev, fp.tile_bits, f.ranges.as<int2>(), nlists);
            where = 1;
        } else {
            rc = radix_sort_pairs_dev(c, f.keys0.as<uint32_t>(), f.vals0.as<uint32_t>(), f.keys1.as<uint32_t>(), f.vals1.as<uint32_t>(),
                                      (long long)cap, pairs_dev, fp.tile_bits, &where);
        }
        if (rc) return rc;
    }
    if (!(wide && m > 0)) GSX_HIP(c, hipMemsetAsync(f.ranges.p, 0, sizeof(int2) * (size_t)nlists, c->stream));
    if (m > 0 && !wide) {
        ProfScope ps(c, "render_ranges");
        hipLaunchKernelGGL(ranges_kernel, dim3(grid_for((long long)cap)), dim3(kRB), 0, c->stream,
                           where ? f.keys1.as<uint32_t>() : f.keys0.as<uint32_t>(), pairs_dev, (unsigned long long)cap, nlists,
                           f.ranges.as<int2>());
        GSX_HIP(c, hipGetLastError());
    }
    *vals_sorted = where ? f.vals1.as<uint32_t>() : f.vals0.as<uint32_t>();
    return GSX_OK;
}

// ---- a walked frame ---------------------------------------------------------------------------------------------------------
// A view that walks a frame's per-tile lists for the fragments' weights (lift_view, label_view, depth_view) is frame_walk_guard
// + frame_lists_that_fit + a kernel built from the pieces of lift_device.hpp + the statistics pair below.  The guard: the state
// a walked frame needs and the sizes it takes, in one order for all of them.  `what`: the noun of the edit-state message.
int frame_walk_guard(Ctx* c, const gsx_camera* cam, int W, int H, const char* who, const char* what) {
    if (c->scene.edits_on)
        return fail(c, GSX_E_STATE, "%s: a render edit state is set (gsx_render_set_edits): %s through an edited frame is not defined", who, what);
    if (c->frame.pre_ext >= 0 || c->frame.in_flight) return fail(c, GSX_E_STATE, "%s: gsx_render_views is running on this context", who);
    if (!cam || W < 1 || H < 1) return fail(c, GSX_E_INVALID, "%s: bad arguments (camera, width %d, height %d)", who, W, H);
    if (W > 4096 || H > 4096) return fail(c, GSX_E_UNSUPPORTED, "%s: %dx%d exceeds 4096 pixels per side", who, W, H);
    return GSX_OK;
}

// The frame's front is render_view's; what differs is WHEN the host learns the pair count.  render_view reads it at the end of
// the frame and redoes a frame whose lists overflowed the pair buffers - a walk must never count a frame twice or count a
// truncated list, so the counters are read back once the lists stand (one host wait); until they fit, the buffers grow and the
// lists are rebuilt.  -> per-tile lists of all pairs (one depth phase) that fit, nothing walked yet.
int frame_lists_that_fit(Ctx* c, const gsx_camera* cam, int W, int H, const char* who, FramePlan& fp, const uint32_t** vals) {
    RenderFrame& f = c->frame;
    int rc = frame_plan(c, W, H, false, 1, fp);
    if (rc) return rc;
    for (int attempt = 0;; ++attempt) {
        const size_t cap = f.pair_cap;
        if ((rc = frame_depth_order(c, cam, fp))) return rc;
        if ((rc = frame_phase_lists(c, fp, 0, 1, vals))) return rc;
        FrameCounters stats;
        GSX_HIP(c, hipMemcpyAsync(&stats, f.small.p, sizeof stats, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
        const unsigned long long P = stats.pairs[0];
        if (P > 0x7fffffffull)
            return fail(c, GSX_E_RANGE, "%s: %llu (tile, splat) pairs exceed 2^31-1 (a close-up of a very large scene)", who, P);
        if (P <= cap) {
            f.P = P;
            return GSX_OK;
        }
        // EMIT wrote nothing and the ranges are empty: grow, rebuild the lists
        if (attempt >= 2) return fail(c, GSX_E_STATE, "%s: pair buffers overflowed three times in a row", who);
        f.pair_cap = (size_t)(P + P / 4 + 4096);
    }
}

// The end of a walked view: the kernel's statistics are queued for `stats` behind it (no wait), and once the caller has waited
// for the stream, summed: f.consumed, and the kernel's own two counters of FrameCounters::Slot.
int frame_walk_stats_queue(Ctx* c, FrameCounters& stats) {
    GSX_HIP(c, hipMemcpyAsync(&stats, c->frame.small.p, sizeof stats, hipMemcpyDeviceToHost, c->stream));
    return GSX_OK;
}

void frame_walk_stats_sum(Ctx* c, const FrameCounters& stats, unsigned long long* atomics, unsigned long long* single) {
    c->frame.consumed = *atomics = 0;
    if (single) *single = 0;
    for (const FrameCounters::Slot& slot : stats.consumed) {
        c->frame.consumed += slot.n;
        *atomics += slot.atomics;
        if (single) *single += slot.single;
    }
}

int render_view(Ctx* c, const gsx_camera* cam, int W, int H, float* rgba_out) {
    GSX_HIP(c, hipSetDevice(c->device));
    if (!cam || W < 1 || H < 1) return fail(c, GSX_E_INVALID, "render_view: bad arguments");
    const int tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16;
    if (tiles_x > 256 || tiles_y > 256)
        return fail(c, GSX_E_UNSUPPORTED, "render_view: %dx%d exceeds 4096 pixels per side", W, H);
    RenderFrame& f = c->frame;
    const size_t img_bytes = sizeof(float) * 4 * (size_t)W * H;
    GSX_HIP(c, f.image.ensure(img_bytes));
    FramePlan fp;
    int rc = frame_plan(c, W, H, true, c->ropt.phases, fp);
    if (rc) return rc;
    FrameCounters* fc = f.small.as<FrameCounters>();
    const long long n = fp.n;
    if (n <= 0) {  // no splats at all: the cleared canvas
        GSX_HIP(c, hipMemsetAsync(f.image.p, 0, img_bytes, c->stream));
        if (rgba_out) GSX_HIP(c, hipMemcpyAsync(rgba_out, f.image.p, img_bytes, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
        return GSX_OK;
    }
    const int K = fp.K;

    for (int attempt = 0;; ++attempt) {
        const size_t cap = f.pair_cap;
        if ((rc = frame_depth_order(c, cam, fp))) return rc;
        int first_phase = 1;
        for (int p = 0; p < K; ++p) {
            const bool last = p == K - 1;
            if (n / fp.divs[p + 1] <= 0 && !last) continue;
            const uint32_t* vals = nullptr;
            if ((rc = frame_phase_lists(c, fp, p, first_phase, &vals))) return rc;
            rc = launch_blend(c, vals, W, H, tiles_x, tiles_y, &fc->dropped,
                              &fc->consumed[0].n, f.sat.as<uint8_t>(), first_phase, last ? 1 : 0);
            if (rc) return rc;
            first_phase = 0;
        }
        // end of frame: the only host wait.  Did every phase fit the pair buffers?
        FrameCounters stats;
        GSX_HIP(c, hipMemcpyAsync(&stats, fc, sizeof stats, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
        unsigned long long maxP = 0, sumP = 0;
        for (int p = 0; p < K; ++p) {
            maxP = std::max(maxP, stats.pairs[p]);
            sumP += stats.pairs[p];
        }
        if (maxP > 0x7fffffffull)  // offsets are 32 bit (and the scan's partial sums would have wrapped beyond 2^32)
            return fail(c, GSX_E_RANGE, "render_view: %llu (tile, splat) pairs in one depth phase exceed 2^31-1 "
                                        "(a close-up of a very large scene): raise the option \"render_phases\"", maxP);
        if (maxP > cap) {
            if (attempt >= 2) return fail(c, GSX_E_STATE, "render_view: pair buffers overflowed three times in a row");
            f.pair_cap = (size_t)(maxP + maxP / 4 + 4096);
            continue;
        }
        f.P = sumP;
        f.consumed = 0;
        for (const FrameCounters::Slot& slot : stats.consumed) f.consumed += slot.n;
        break;
    }
    if (rgba_out) {
        GSX_HIP(c, hipMemcpyAsync(rgba_out, f.image.p, img_bytes, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
    }
    return GSX_OK;
}

// ---- several views: a few frames in flight ------------------------------------------------------------------------------
// A frame is a chain of dependent kernels: memory-bound per-splat passes and sorts first, then the VALU-bound blend with
// its tail of long tiles.  Frames on separate HIP streams fill each other's gaps (measured 916 -> 1221 views/s with two at
// 3 M splats / 1080p / SH 3).  The context therefore keeps TWINS: further streams with their own per-frame buffers that
// alias this context's scene (texel pairs, SH planes: nothing is duplicated), each driven by a host thread of its own; frame
// k is rendered by stream k % F (option "render_frames").
static int twin_sync_scene(Ctx* c, int k) {
    if (!c->twins[k]) {
        c->twins[k] = new (std::nothrow) Ctx();
        if (!c->twins[k]) return fail(c, GSX_E_INVALID, "render_views: out of host memory");
        c->twins[k]->device = c->device;
        hipError_t e = hipSuccess;
        if (k == 0 && c->ropt.share_stream) {
            // the first extra frame runs on the context's second stream (the early vote's): with a stream of its own a process
            // that has labelled before holds six streams for four hardware queues, and frames that share a queue serialise
            // (bench.py's render leg: 1160-1200 views/s against 1335-1400 in a process that never labelled)
            if (second_stream(c) != GSX_OK) e = hipErrorUnknown;
            c->twins[k]->stream = c->stream2;
            c->twins[k]->stream_borrowed = true;
        } else {
            e = hipStreamCreateWithFlags(&c->twins[k]->stream, hipStreamNonBlocking);
        }
        if (e != hipSuccess) {
            c->twins[k]->stream = nullptr;
            delete c->twins[k];
            c->twins[k] = nullptr;
            return fail(c, GSX_E_HIP, "render_views: hipStreamCreate failed: %s", hipGetErrorString(e));
        }
    }
    Ctx* t = c->twins[k];
    t->scene.alias(c->scene);  // every frame in flight draws the same scene and edit state ..
    t->ropt = c->ropt;         // .. with the same options
    if (t->frame.pair_cap < c->frame.pair_cap) t->frame.pair_cap = c->frame.pair_cap;
    return GSX_OK;
}

void render_release_twin(Ctx* c) {
    for (Ctx*& t : c->twins) {
        if (!t) continue;
        (void)hipStreamSynchronize(t->stream);
        if (!t->stream_borrowed) (void)hipStreamDestroy(t->stream);
        t->stream = nullptr;
        delete t;
        t = nullptr;
    }
}

int render_views(Ctx* c, int n, const gsx_camera* cams, int W, int H, float* const* rgba_out) {
    if (n < 0 || (n > 0 && !cams)) return fail(c, GSX_E_INVALID, "render_views: bad arguments");
    if (n == 0) return GSX_OK;
    const int F = std::max(1, std::min({c->ropt.frames, kMaxFrames, n}));
    if (F == 1 || c->prof_on)  // the per-kernel events belong to one stream: profiled runs render one frame at a time
    {
        unsigned long long P = 0, used = 0;
        for (int k = 0; k < n; ++k) {
            const int rc = render_view(c, cams + k, W, H, rgba_out ? rgba_out[k] : nullptr);
            if (rc) return rc;
            P += c->frame.P;
            used += c->frame.consumed;
        }
        c->frame.P = P;
        c->frame.consumed = used;
        return GSX_OK;
    }
    int rc = GSX_OK;
    for (int f = 1; f < F; ++f)
        if ((rc = twin_sync_scene(c, f - 1))) return rc;
    // frame k is rendered by stream k % F: stream 0 is the context's own (this thread), the others have a host thread each.
    // Group g = the frames g * F .. g * F + F - 1.  With the option render_multi_pre the pre pass of a whole group is ONE launch
    // (pre_multi_kernel) on stream 0, issued by this thread ahead of its own frame of the previous group, into record set
    // g % 3 of every frame's context; the other frames wait for it through an event.  Host-side ordering (an event must have
    // been recorded before another thread may wait for it, a set must not be rewritten while a frame still reads it) goes
    // through two counters: pre_issued (groups whose pass has been launched) and done[f] (frames context f has completed -
    // render_view returns only after its end-of-frame synchronisation).
    int rcs[kMaxFrames] = {};  // GSX_OK == 0
    unsigned long long P[kMaxFrames] = {}, used[kMaxFrames] = {};
    const bool multi = c->ropt.multi_pre != 0 && c->scene.rn > 0;
    const int groups = (n + F - 1) / F;
    std::atomic<int> pre_issued{0}, done[kMaxFrames];
    std::atomic<bool> failed{false};
    for (auto& d : done) d.store(0);
    Ctx* ctxs[kMaxFrames] = {c};
    for (int f = 1; f < F; ++f) ctxs[f] = c->twins[f - 1];
    if (multi) {
        for (int f = 0; f < F; ++f)
            for (PreSet& ps : ctxs[f]->frame.sets)
                if ((rc = ensure_pre_set(c, ps, c->scene.rn))) return rc;
    }
    auto issue_pre = [&](int g) -> int {  // this thread only; stream 0
        // set g % 3 was last read by the frames of group g - 3: every context must have completed them
        for (int f = 0; f < F; ++f)
            while (done[f].load(std::memory_order_acquire) < std::min(g - 2, (n - 1 - f) / F + 1) && !failed.load()) std::this_thread::yield();
        if (failed.load()) return GSX_OK;
        const int set = g % kPreSets;
        const int nv = std::min(F, n - g * F);
        PreSet* sets[kMaxFrames];
        for (int v = 0; v < nv; ++v) sets[v] = &ctxs[v]->frame.sets[set];
        const int rcp = launch_pre_multi(c, nv, cams + g * F, W, H, sets, set);  // (argument slot = record set)
        if (rcp) return rcp;
        GSX_HIP(c, c->r_pre_ev[set].record(c->stream));
        pre_issued.store(g + 1, std::memory_order_release);
        return GSX_OK;
    };
    auto frames_of = [&](Ctx* t, int f) {
        t->frame.in_flight = true;  // (other frames run next to this context's: render_view picks the forms that share the GPU best)
        int g = 0;
        for (int k = f; k < n && rcs[f] == GSX_OK; k += F, ++g) {
            if (multi) {
                if (f == 0) {  // this thread: the pass of the NEXT group goes out before this group's frame (group 0's before the threads start)
                    if (g + 1 < groups && (rcs[f] = issue_pre(g + 1))) break;
                    if (failed.load()) break;  // (a pass that was not issued leaves no records to render from)
                } else {
                    while (pre_issued.load(std::memory_order_acquire) < g + 1 && !failed.load()) std::this_thread::yield();
                    if (failed.load()) break;
                    const hipError_t e = c->r_pre_ev[g % kPreSets].stream_wait(t->stream);
                    if (e != hipSuccess) {
                        rcs[f] = fail(t, GSX_E_HIP, "render_views: hipStreamWaitEvent: %s", hipGetErrorString(e));
                        break;
                    }
                }
                t->frame.pre_ext = g % kPreSets;
            }
            rcs[f] = render_view(t, cams + k, W, H, rgba_out ? rgba_out[k] : nullptr);
            t->frame.pre_ext = -1;
            P[f] += t->frame.P;
            used[f] += t->frame.consumed;
            done[f].store(g + 1, std::memory_order_release);
        }
        t->frame.pre_ext = -1;
        t->frame.in_flight = false;
        if (rcs[f] != GSX_OK) failed.store(true);  // nobody waits for a pass or a frame that will not come
    };
    if (multi && (rc = issue_pre(0))) return rc;
    std::thread others[kMaxFrames - 1];
    int started = 0;
    try {
        for (int f = 1; f < F; ++f) {
            Ctx* t = c->twins[f - 1];
            others[f - 1] = std::thread([&, t, f] {
                try {  // nothing may escape a thread's entry function
                    (void)hipSetDevice(t->device);
                    frames_of(t, f);
                } catch (...) {
                    rcs[f] = fail(t, GSX_E_INVALID, "render_views: a stream's host thread failed (out of host memory?)");
                    failed.store(true);
                }
            });
            ++started;
        }
        frames_of(c, 0);
    } catch (...) {
        failed.store(true);
        for (int f = 0; f < started; ++f) others[f].join();  // never leave a joinable thread behind
        throw;
    }
    for (int f = 0; f < started; ++f) others[f].join();
    for (int f = 0; f < F; ++f) ctxs[f]->frame.in_flight = false;
    rc = rcs[0];
    for (int f = 1; f < F && rc == GSX_OK; ++f)
        if (rcs[f] != GSX_OK) {
            c->err = c->twins[f - 1]->err;
            rc = rcs[f];
        }
    c->frame.P = 0;
    c->frame.consumed = 0;
    for (int f = 0; f < F; ++f) {
        c->frame.P += P[f];
        c->frame.consumed += used[f];
    }
    return rc;
}

}  // namespace gsx
