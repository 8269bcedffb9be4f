// lift.hip - the lifting labeler: 2-D class maps lifted onto the splats through the rasterizer's own blend.
//
// For a view (cam, W, H) and an H x W class map the frame is walked exactly as gsx_render_view walks it - the same pre pass,
// depth order and per-tile lists (render.hip: frame_plan / frame_depth_order / frame_phase_lists, one depth phase, 16x16 tiles),
// the same `discard` rule and ONE_MINUS_DST_ALPHA, ONE blend (blend.hip: blend_one, whose operation order lift_fragment keeps;
// compiled with -ffp-contract=off like it).  The k-th fragment at pixel p, made by splat i, raises the frame's alpha by
//     w = (1 - dst.a) * B,   B = exp(A) * alpha
// and the view adds q = rint(w * 2^20) to table[i][map[p] + 1].  The table is u64 [n][n_classes + 1]; integer sums do not
// depend on the order in which they arrive, so a table is reproducible bit for bit and two views accumulated together are the
// sum of their tables (float atomics give neither: a float sum depends on the order of arrival).
//
// On-chip reduction.  A record (one splat in one tile's list) would cost up to 256 atomics, one per pixel.  lift_kernel sums a
// record's q over the tile's pixels per class first - a wave reduction, then LDS adds across the four waves - and issues at
// most ONE 64-bit global atomic per (record, class present in the tile), none for a zero sum.  The classes present in the tile
// are found once per tile; a wave whose 64 pixels share a class (the common case of a real segmentation) takes one full-wave
// reduction per record and no per-class loop.  The rate of 64-bit integer atomics on this GPU is not measured anywhere we know
// of (published figures are for float atomics); tools/lift_bench.py reports how many a view issues next to its time.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "lift_device.hpp"
#include "render_device.hpp"
#include "seg_dtype.hpp"

namespace gsx {

static constexpr int kLiftCells = 2048;  // LDS accumulators: (records of a round) x (classes present in the tile)
static constexpr int kLiftLoopMax = 4;   // a mixed wave with up to this many classes reduces per class; with more, its lanes add to LDS
static_assert(kLiftCells >= kLiftMaxBins && kLiftCells % kLiftThreads == 0, "a round holds at least one record");

void lift_constants(int32_t out[8]) {
    const int32_t v[8] = {kLiftOne, kLiftShift, kLiftTile, kLiftChunk, kLiftCells, kLiftLoopMax, kLiftMaxBins - 1, 0};
    for (int k = 0; k < 8; ++k) out[k] = v[k];
}

// ---- the view's map as one u8 bin per pixel ---------------------------------------------------------------------------------
// bin = label + 1 (0 = label -1).  A label outside [-1, n_classes - 1] becomes bin 0 and records the view in *flag (host maps
// are checked before anything is launched and never get here with one).
// The stored value v is compared with the range of stored values itself, [lo - off, n_classes - off], and the bin v + off is
// formed only for a value inside it: no sum that could leave 64 bits (v + 1 at 2^63 - 1), nothing narrowed before the test.
template <int DT>
__host__ __device__ __forceinline__ bool lift_value_ok(long long v, int n_classes) {
    const long long off = SegElem<DT>::add;  // a packed u8 map holds the bin itself
    const long long lo = DT == GSX_SEG_U8_LABELS ? 1 : 0;  // u8 labels cannot say -1
    return v >= lo - off && v <= (long long)n_classes - off;
}

template <int DT>
__global__ __launch_bounds__(kRB) void lift_narrow_kernel(const typename SegElem<DT>::type* __restrict__ seg, long long npix, int n_classes,
                                                           int view, uint8_t* __restrict__ bins, int* __restrict__ flag) {
    const long long p = (long long)blockIdx.x * kRB + threadIdx.x;
    if (p >= npix) return;
    const long long v = (long long)seg[p];
    const bool ok = lift_value_ok<DT>(v, n_classes);
    bins[p] = ok ? (uint8_t)(v + SegElem<DT>::add) : (uint8_t)0;
    if (!ok) atomicMin(flag, view);
}

template <int DT>
static long long host_first_bad(const void* seg, long long npix, int n_classes) {
    const auto* s = static_cast<const typename SegElem<DT>::type*>(seg);
    for (long long p = 0; p < npix; ++p)
        if (!lift_value_ok<DT>((long long)s[p], n_classes)) return p;
    return -1;
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One workgroup per 16x16 tile, modelled on blend_kernel: 256 records staged through LDS at a time, every pixel walks them
// carrying only dst.a; the opacity vote falls after every staged chunk.  The walk's pieces - pixel, staging, weight, vote,
// statistics slot - and rank256 live in lift_device.hpp: labelmap.hip and depthmap.hip walk the same fragments with them.
// Pixels outside the frame contribute 0 and count as opaque.  A chunk is walked in ROUNDS of `sub` records, sub * (classes in the tile) <= kLiftCells accumulators: up to 8
// classes in a tile a round is the whole chunk; the worst case (255 classes in 256 pixels) walks 8 records per round - correct,
// slow.  No lane leaves before the last barrier: a tile without a list returns as a whole, before the first one.
__global__ __launch_bounds__(kLiftThreads) void lift_kernel(const int2* __restrict__ ranges, const uint32_t* __restrict__ vals,
                                                            const float4* __restrict__ rec, const uint8_t* __restrict__ bins,
                                                            int W, int H, int tiles_x, int nbins,
                                                            unsigned long long* __restrict__ table,
                                                            unsigned long long* __restrict__ consumed) {
    __shared__ float4 s0[kLiftChunk];
    __shared__ float4 s1[kLiftChunk];
    __shared__ float sa[kLiftChunk];
    __shared__ uint32_t sid[kLiftChunk];
    __shared__ uint32_t cells[kLiftCells];
    __shared__ uint32_t present[8];
    __shared__ uint8_t tile_bin[kLiftMaxBins];  // class index in the tile -> bin
    __shared__ uint8_t wlist[4][64];            // a mixed wave's class indices
    __shared__ uint32_t natom;
    const int tile = (int)blockIdx.x;
    const int2 range = ranges[tile];
    if (range.y <= range.x) return;  // (workgroup-uniform)
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LiftPixel p = lift_pixel(tile, tiles_x, W, H, tid);
    const bool inside = p.inside;
    if (tid < 8) present[tid] = 0u;
    if (tid == 0) natom = 0u;
    for (int i = tid; i < kLiftCells; i += kLiftThreads) cells[i] = 0u;
    __syncthreads();
    // the tile's classes, once: a 256-bit mask of the bins present, a pixel's class index = the rank of its bin
    const uint32_t b = inside ? (uint32_t)bins[p.pix] : 0u;
    if (inside) atomicOr(&present[b >> 5], 1u << (b & 31u));
    __syncthreads();
    uint32_t pw[8];
    int D = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        pw[j] = present[j];
        D += __popc(pw[j]);
    }
    if ((present[tid >> 5] >> (tid & 31)) & 1u) tile_bin[rank256(pw, (uint32_t)tid)] = (uint8_t)tid;
    // the wave's classes, once: lanes outside the frame never add anything and take the class of the wave's first pixel inside
    uint32_t ci = inside ? rank256(pw, b) : 0u;
    const unsigned long long in_mask = __ballot(inside);
    const uint32_t wc = in_mask ? (uint32_t)__shfl((int)ci, __ffsll((long long)in_mask) - 1) : 0u;
    if (!inside) ci = wc;
    const bool uniform = __all(ci == wc) != 0;
    int wcount = 1;
    if (!uniform) {  // (wave-uniform)
        wcount = 0;
        unsigned long long left = ~0ull;
        while (left) {
            const uint32_t d = (uint32_t)__shfl((int)ci, __ffsll((long long)left) - 1);
            left &= ~__ballot(ci == d);
            if (lane == 0) wlist[wave][wcount] = (uint8_t)d;
            ++wcount;
        }
    }
    const int sub = min(kLiftChunk, kLiftCells / D);  // D >= 1: the tile has a pixel inside the frame
    float a = 0.0f;                                   // gl.clear to (0,0,0,0): only dst.a is carried
    uint32_t my_atoms = 0u;
    int staged = 0;
    for (int base = range.x; base < range.y; base += kLiftChunk) {
        const int cnt = min(kLiftChunk, range.y - base);
        __syncthreads();
        if (tid < cnt) {
            const uint32_t id = vals[base + tid];
            lift_stage(s0, s1, sa, rec, id, tid);
            sid[tid] = id;
        }
        __syncthreads();
        for (int r0 = 0; r0 < cnt; r0 += sub) {
            const int r1 = min(cnt, r0 + sub);
            for (int k = r0; k < r1; ++k) {
                const uint32_t q = lift_weight(a, p, s0[k], s1[k], sa[k]);
                if (__ballot(q != 0u) == 0ull) continue;  // (wave-uniform) the record puts nothing on this wave's pixels
                uint32_t* row = cells + (k - r0) * D;
                if (uniform) {
                    const uint32_t s = wave_sum_u32(q);  // <= 2^26 per wave, <= 2^28 per cell
                    if (lane == 0) atomicAdd(&row[wc], s);
                } else if (wcount <= kLiftLoopMax) {
                    for (int j = 0; j < wcount; ++j) {
                        const uint32_t d = wlist[wave][j];
                        const uint32_t s = wave_sum_u32(ci == d ? q : 0u);
                        if (lane == 0 && s) atomicAdd(&row[d], s);
                    }
                } else if (q) {
                    atomicAdd(&row[ci], q);
                }
            }
            __syncthreads();
            // the round's sums leave the chip: one atomic per (record, class) that got anything
            const int ncell = (r1 - r0) * D;
            for (int i = tid; i < ncell; i += kLiftThreads) {
                const uint32_t v = cells[i];
                if (v) {
                    cells[i] = 0u;
                    const int r = i / D, d = i - r * D;
                    atomicAdd(&table[(size_t)sid[r0 + r] * (size_t)nbins + tile_bin[d]], (unsigned long long)v);
                    ++my_atoms;
                }
            }
            __syncthreads();
        }
        staged += cnt;
        if (lift_tile_opaque(p, a)) break;
    }
    // statistics: records staged, global atomics issued
    if (my_atoms) atomicAdd(&natom, my_atoms);
    __syncthreads();
    if (tid == 0) {
        unsigned long long* slot = lift_stats_slot(consumed);
        atomicAdd(slot, (unsigned long long)staged);
        if (natom) atomicAdd(slot + 1, (unsigned long long)natom);
    }
}

// ---- the arg-max --------------------------------------------------------------------------------------------------------------
// Per splat: total < threshold -> -1; else the largest bin, the lowest on a tie (bin 0 = label -1 can win).  Integers only; the
// share is one fp64 division.  Row j of the table is importance-order slot j, order[j] its index in the upload.
__global__ __launch_bounds__(kRB) void lift_argmax_kernel(const unsigned long long* __restrict__ table, const uint32_t* __restrict__ order,
                                                           long long n, int nbins, unsigned long long threshold,
                                                           int32_t* __restrict__ labels, double* __restrict__ share) {
    const long long j = (long long)blockIdx.x * kRB + threadIdx.x;
    if (j >= n) return;
    const unsigned long long* row = table + (size_t)j * nbins;
    unsigned long long total = 0, best = 0;
    int arg = 0;
    for (int k = 0; k < nbins; ++k) {
        const unsigned long long v = row[k];
        total += v;
        if (v > best) best = v, arg = k;
    }
    const uint32_t i = order[j];
    labels[i] = total < threshold ? -1 : arg - 1;
    share[i] = total ? (double)best / (double)total : 0.0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
void lift_end(Ctx* c) {
    c->lift.begun = false;
    c->lift.views = 0;
}

int lift_begin(Ctx* c, int n_classes) {
    GSX_HIP(c, hipSetDevice(c->device));
    if (n_classes < 1 || n_classes > kLiftMaxBins - 1)
        return fail(c, GSX_E_INVALID, "lift_begin: n_classes = %d must be in [1, %d]", n_classes, kLiftMaxBins - 1);
    if (c->scene.rn <= 0) return fail(c, GSX_E_STATE, "lift_begin: no splats uploaded (gsx_upload_splats)");
    LiftState& L = c->lift;
    lift_end(c);
    const size_t bytes = sizeof(unsigned long long) * (size_t)c->scene.rn * (size_t)(n_classes + 1);
    if (L.table.ensure(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, GSX_E_HIP, "lift_begin: could not allocate %zu bytes for the table of %lld splats x %d bins", bytes,
                    (long long)c->scene.rn, n_classes + 1);
    }
    GSX_HIP(c, L.flag.ensure(sizeof(int)));
    GSX_HIP(c, hipMemsetAsync(L.table.p, 0, bytes, c->stream));
    GSX_HIP(c, hipMemsetAsync(L.flag.p, 0x7f, sizeof(int), c->stream));  // kNoBadView
    L.n_classes = n_classes;
    L.atomics = 0;
    L.begun = true;
    return GSX_OK;
}

static int lift_narrow(Ctx* c, const void* seg_dev, int seg_dtype, long long npix) {
    LiftState& L = c->lift;
    uint8_t* bins = L.bins.as<uint8_t>();
    int* flag = L.flag.as<int>();
    const dim3 grid(grid_for(npix)), block(kRB);
    ProfScope ps(c, "lift_narrow");
    with_seg_dtype(seg_dtype, [&](auto d) {
        constexpr int DT = decltype(d)::value;
        hipLaunchKernelGGL(lift_narrow_kernel<DT>, grid, block, 0, c->stream, static_cast<const typename SegElem<DT>::type*>(seg_dev), npix,
                           L.n_classes, L.views, bins, flag);
    });
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

// One view: a walked frame (render.hip: frame_walk_guard, frame_lists_that_fit - lift_kernel only runs on lists that fit, so no
// frame is counted twice and no truncated list is counted).  A second read at the end fetches the statistics.
int lift_view(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, int W, int H, bool device) {
    GSX_HIP(c, hipSetDevice(c->device));
    LiftState& L = c->lift;
    const char* who = device ? "lift_view_device" : "lift_view";
    if (!L.begun) return fail(c, GSX_E_STATE, "%s: call gsx_lift_begin first", who);
    int rc = frame_walk_guard(c, cam, W, H, who, "lifting");
    if (rc) return rc;
    if (!seg) return fail(c, GSX_E_INVALID, "%s: bad arguments (the map is NULL)", who);
    if (!seg_dtype_known(seg_dtype)) return fail(c, GSX_E_INVALID, "%s: unknown seg_dtype %d", who, seg_dtype);
    const size_t elem = seg_elem_size(seg_dtype);
    if (seg_misaligned(seg, (int)elem)) return fail(c, GSX_E_INVALID, "%s: the map is not aligned to its element", who);
    const long long npix = (long long)W * H;
    if (!device) {  // the label range, before anything is launched
        const long long bad = with_seg_dtype(seg_dtype, [&](auto d) { return host_first_bad<decltype(d)::value>(seg, npix, L.n_classes); });
        if (bad >= 0)
            return fail(c, GSX_E_RANGE, "%s: view %d: the label at row %lld, column %lld is outside [-1, %d]", who, L.views, bad / W, bad % W,
                        L.n_classes - 1);
    }
    GSX_HIP(c, L.bins.ensure((size_t)npix));
    const void* seg_dev = seg;
    if (!device) {
        GSX_HIP(c, L.raw.ensure(elem * (size_t)npix));
        GSX_HIP(c, hipMemcpyAsync(L.raw.p, seg, elem * (size_t)npix, hipMemcpyHostToDevice, c->stream));
        seg_dev = L.raw.p;
    }
    if ((rc = lift_narrow(c, seg_dev, seg_dtype, npix))) return rc;
    if (!device) GSX_HIP(c, hipStreamSynchronize(c->stream));  // the caller's map has been read when the call returns
    RenderFrame& f = c->frame;
    FramePlan fp;
    const uint32_t* vals = nullptr;
    if ((rc = frame_lists_that_fit(c, cam, W, H, who, fp, &vals))) return rc;
    {
        ProfScope ps(c, "lift");
        hipLaunchKernelGGL(lift_kernel, dim3(fp.ntiles), dim3(kLiftThreads), 0, c->stream, f.ranges.as<int2>(), vals,
                           f.cur->rec.as<float4>(), L.bins.as<uint8_t>(), W, H, fp.tiles_x, L.n_classes + 1,
                           L.table.as<unsigned long long>(), &f.small.as<FrameCounters>()->consumed[0].n);
    }
    GSX_HIP(c, hipGetLastError());
    FrameCounters stats;
    if ((rc = frame_walk_stats_queue(c, stats))) return rc;
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    frame_walk_stats_sum(c, stats, &L.atomics, nullptr);
    ++L.views;
    return GSX_OK;
}

static int lift_check_maps(Ctx* c, const char* who) {
    int flag = kNoBadView;
    GSX_HIP(c, hipMemcpyAsync(&flag, c->lift.flag.p, sizeof flag, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    if (flag != kNoBadView)
        return fail(c, GSX_E_RANGE, "%s: the device map of view %d held a label outside [-1, %d]", who, flag, c->lift.n_classes - 1);
    return GSX_OK;
}

unsigned long long lift_threshold(double min_weight) {
    const double scaled = std::ceil(min_weight * (double)kLiftOne);
    return scaled >= 18446744073709551615.0 ? ~0ull : (unsigned long long)scaled;
}

int lift_finalize(Ctx* c, double min_weight, int32_t* labels_out, double* share_out) {
    GSX_HIP(c, hipSetDevice(c->device));
    LiftState& L = c->lift;
    if (!L.begun) return fail(c, GSX_E_STATE, "lift_finalize: call gsx_lift_begin first");
    if (!labels_out) return fail(c, GSX_E_INVALID, "lift_finalize: labels_out is NULL");
    if (!(min_weight >= 0.0) || !(min_weight <= 1.0e300)) return fail(c, GSX_E_INVALID, "lift_finalize: min_weight must be finite and >= 0");
    int rc = lift_check_maps(c, "lift_finalize");
    if (rc) return rc;
    const unsigned long long threshold = lift_threshold(min_weight);
    const size_t n = (size_t)c->scene.rn;
    GSX_HIP(c, L.out.ensure(12 * n + 8));
    double* share = L.out.as<double>();
    int32_t* labels = reinterpret_cast<int32_t*>(share + n);
    {
        ProfScope ps(c, "lift_argmax");
        hipLaunchKernelGGL(lift_argmax_kernel, dim3(grid_for((long long)n)), dim3(kRB), 0, c->stream, L.table.as<unsigned long long>(),
                           c->scene.order.as<uint32_t>(), (long long)n, L.n_classes + 1, threshold, labels, share);
    }
    GSX_HIP(c, hipGetLastError());
    GSX_HIP(c, hipMemcpyAsync(labels_out, labels, 4 * n, hipMemcpyDeviceToHost, c->stream));
    if (share_out) GSX_HIP(c, hipMemcpyAsync(share_out, share, 8 * n, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

int lift_table(Ctx* c, uint64_t* table_out) {
    GSX_HIP(c, hipSetDevice(c->device));
    LiftState& L = c->lift;
    if (!L.begun) return fail(c, GSX_E_STATE, "lift_table: call gsx_lift_begin first");
    if (!table_out) return fail(c, GSX_E_INVALID, "lift_table: table_out is NULL");
    int rc = lift_check_maps(c, "lift_table");
    if (rc) return rc;
    const size_t n = (size_t)c->scene.rn, nb = (size_t)L.n_classes + 1;
    std::vector<uint32_t> order(n);
    std::vector<uint64_t> rows(n * nb);  // importance order, as on the device
    GSX_HIP(c, hipMemcpyAsync(order.data(), c->scene.order.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(rows.data(), L.table.p, 8 * n * nb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t j = 0; j < n; ++j) {
        if (order[j] >= n) return fail(c, GSX_E_STATE, "lift_table: the scene's permutation is damaged");
        std::copy(rows.begin() + j * nb, rows.begin() + (j + 1) * nb, table_out + (size_t)order[j] * nb);
    }
    return GSX_OK;
}

}  // namespace gsx
