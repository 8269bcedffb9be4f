// labelmap.hip - label frames: the splats' labels as the class map of a view, the transpose of the lifting labeler.
//
// lift.hip adds, per fragment, the blend weight q = rint(w * 2^20) to table[splat][class of the pixel]; this unit adds the same
// q to plane[label of the splat][pixel] and takes the arg-max per pixel.  The frame is walked exactly as lift_view walks it: the
// same pre pass, depth order and per-tile lists (render.hip: frame_plan / frame_depth_order / frame_phase_lists, one depth
// phase, 16x16 tiles), the same fragment arithmetic (lift_device.hpp: lift_fragment, -ffp-contract=off) and the same opacity
// vote after every staged chunk of 256 records.  Both kernels therefore sum the same integers, and
//     sum over {p: seg[p] = c} of plane[b][p]  ==  sum over {i: label[i] = b} of lift_table[i][c + 1]
// holds bit for bit (tests/test_labelmap_gpu.py).
//
// A pixel belongs to one lane, so its sums need no reduction and no atomics between lanes: the accumulators are acc[slot][pixel]
// uint32 in LDS - the 64 lanes of a wave hit 64 consecutive words, no bank conflict - one slot per label bin present in the
// tile's list (a 256-bit presence mask, a bin's slot = its rank in the mask).  The LDS holds a window of kLabelWindow slots; a
// tile whose list carries more bins walks its list once per window - the identical walk, same dst.a sequence, same votes -
// and adds only the window's bins.  A real labelling puts a handful of labels into a tile: one walk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "gsx_ctx.hpp"
#include "lift_device.hpp"
#include "render_device.hpp"

namespace gsx {

// Labels per window.  LDS per workgroup: 9 KiB of staged records (two float4 and one float per record), 256 B of their slots,
// 1 KiB per label of the window, under 1 KiB of masks and tables.  16 labels: 26 656 B, six workgroups (24 waves) per CU of
// 160 KiB; 32 labels would leave three, 8 labels eight - and a tile on an object border rarely sees more than 16.
static constexpr int kLabelWindow = 16;
static constexpr int kLabelMaxPlanes = 256;
static constexpr uint32_t kNoSlot = 0xffffu;

void labelmap_constants(int32_t out[8]) {
    const int32_t v[8] = {kLiftOne, kLiftShift, kLiftTile, kLiftChunk, kLabelWindow, kLiftMaxBins - 1, 0, 0};
    for (int k = 0; k < 8; ++k) out[k] = v[k];
}

// ---- the labels as one byte per splat, importance order ------------------------------------------------------------------------
// bin = label + 1 (0 = label -1).  A label outside [-1, n_classes - 1] records the lowest upload row that holds one.
__global__ __launch_bounds__(kRB) void label_bins_kernel(const int* __restrict__ labels, const uint32_t* __restrict__ order, long long n,
                                                          int n_classes, uint8_t* __restrict__ bins8, uint32_t* __restrict__ bad) {
    const long long j = (long long)blockIdx.x * kRB + threadIdx.x;
    if (j >= n) return;
    const int v = labels[j];
    const bool ok = v >= -1 && v < n_classes;
    bins8[j] = ok ? (uint8_t)(v + 1) : (uint8_t)0;
    if (!ok) atomicMin(bad, order[j]);
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------------
// One workgroup per 16x16 tile, one pixel per lane, built from the pieces of lift_device.hpp that lift_kernel walks with: 256
// records staged through LDS at a time, every pixel walks them carrying only dst.a, the opacity vote falls after every staged
// chunk.  Pixels outside the frame contribute
// 0, count as opaque and write nothing.  A tile without a list writes label -1 and zeros and returns as a whole; in every other
// tile no lane leaves before the last barrier.
__global__ __launch_bounds__(kLiftThreads) void label_kernel(const int2* __restrict__ ranges, const uint32_t* __restrict__ vals,
                                                             const float4* __restrict__ rec, const uint8_t* __restrict__ bins8, int W,
                                                             int H, int tiles_x, unsigned long long threshold, int n_planes,
                                                             const uint8_t* __restrict__ plane_bins, int32_t* __restrict__ label_out,
                                                             uint32_t* __restrict__ weight_out, uint32_t* __restrict__ total_out,
                                                             uint32_t* __restrict__ planes_out, unsigned long long* __restrict__ consumed) {
    __shared__ float4 s0[kLiftChunk];
    __shared__ float4 s1[kLiftChunk];
    __shared__ float sa[kLiftChunk];
    __shared__ uint8_t sslot[kLiftChunk];                // a staged record's slot
    __shared__ uint32_t acc[kLabelWindow * kLiftThreads];  // [slot of the window][pixel]
    __shared__ uint32_t present[8];
    __shared__ uint8_t tile_bin[kLiftMaxBins];           // slot -> bin
    __shared__ uint16_t plane_slot[kLabelMaxPlanes];     // plane -> slot of its bin, kNoSlot: the bin is not in the tile's list
    const int tile = (int)blockIdx.x;
    const int2 range = ranges[tile];
    const int tid = (int)threadIdx.x;
    const LiftPixel p = lift_pixel(tile, tiles_x, W, H, tid);
    const bool inside = p.inside;
    const size_t npix = (size_t)W * (size_t)H, pix = p.pix;
    if (range.y <= range.x) {  // (workgroup-uniform) nothing reaches this tile
        if (inside) {
            label_out[pix] = -1;
            if (weight_out) weight_out[pix] = 0u;
            if (total_out) total_out[pix] = 0u;
            for (int k = 0; k < n_planes; ++k) planes_out[(size_t)k * npix + pix] = 0u;
        }
        return;
    }
    if (tid < 8) present[tid] = 0u;
    __syncthreads();
    // the bins of the tile's list, once: a 256-bit mask, a bin's slot = its rank
    for (int i = range.x + tid; i < range.y; i += kLiftThreads) {
        const uint32_t b = bins8[vals[i]];
        atomicOr(&present[b >> 5], 1u << (b & 31u));
    }
    __syncthreads();
    uint32_t pw[8];
    int D = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        pw[j] = present[j];
        D += __popc(pw[j]);
    }
    if ((pw[tid >> 5] >> (tid & 31)) & 1u) tile_bin[rank256(pw, (uint32_t)tid)] = (uint8_t)tid;
    if (tid < n_planes) {
        const uint32_t b = plane_bins[tid];
        plane_slot[tid] = (uint16_t)(((pw[b >> 5] >> (b & 31u)) & 1u) ? rank256(pw, b) : kNoSlot);
    }
    // (both tables are read after the walk's barriers)
    const int nwin = (D + kLabelWindow - 1) / kLabelWindow;  // D >= 1: the list is not empty
    uint32_t total = 0u, best = 0u;
    int arg = 0;
    int staged = 0;
    for (int win = 0; win < nwin; ++win) {
        const int lo = win * kLabelWindow;
        const int nslot = min(kLabelWindow, D - lo);
        for (int s = 0; s < nslot; ++s) acc[s * kLiftThreads + tid] = 0u;  // a lane's own column: no barrier
        float a = 0.0f;  // gl.clear to (0,0,0,0): only dst.a is carried
        for (int base = range.x; base < range.y; base += kLiftChunk) {
            const int cnt = min(kLiftChunk, range.y - base);
            __syncthreads();
            if (tid < cnt) {
                const uint32_t id = vals[base + tid];
                lift_stage(s0, s1, sa, rec, id, tid);
                sslot[tid] = (uint8_t)rank256(pw, (uint32_t)bins8[id]);
            }
            __syncthreads();
            for (int k = 0; k < cnt; ++k) {
                const uint32_t q = lift_weight(a, p, s0[k], s1[k], sa[k]);
                const uint32_t s =(uint32_t)sslot[k] - (uint32_t)lo;  // (workgroup-uniform)
                if (s < (uint32_t)kLabelWindow && q) atomicAdd(&acc[s * kLiftThreads + tid], q);  // no result used: one LDS add
            }
            if (win == 0) staged += cnt;
            if (lift_tile_opaque(p, a)) break;
        }
        // the window's sums: bins ascend with the slots, so a strict > keeps the lowest bin on a tie
        for (int s = 0; s < nslot; ++s) {
            const uint32_t v = acc[s * kLiftThreads + tid];
            total += v;
            if (v > best) best = v, arg = (int)tile_bin[lo + s];
        }
        if (inside) {
            for (int k = 0; k < n_planes; ++k) {
                const uint32_t ps = plane_slot[k];
                if (ps == kNoSlot) {
                    if (win == 0) planes_out[(size_t)k * npix + pix] = 0u;
                } else if (ps >= (uint32_t)lo && ps < (uint32_t)(lo + nslot)) {
                    planes_out[(size_t)k * npix + pix] = acc[(ps - (uint32_t)lo) * kLiftThreads + tid];
                }
            }
        }
    }
    if (inside) {
        const bool keep = (unsigned long long)total >= threshold;
        label_out[pix] = keep ? arg - 1 : -1;
        if (weight_out) weight_out[pix] = keep ? best : 0u;
        if (total_out) total_out[pix] = total;
    }
    // statistics: records staged by the first walk, walks, one-label tiles
    if (tid == 0) {
        unsigned long long* slot = lift_stats_slot(consumed);
        atomicAdd(slot, (unsigned long long)staged);
        atomicAdd(slot + 1, (unsigned long long)nwin);
        if (D == 1) atomicAdd(slot + 2, 1ull);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
void label_new_upload(Ctx* c, bool has_labels) {
    c->labelmap.has_labels = has_labels;
    c->labelmap.checked_classes = 0;
}

// the upload's labels against [-1, n_classes - 1], and as bytes: one kernel over the n labels, once per upload and n_classes
static int label_check(Ctx* c, int n_classes) {
    LabelMapState& S = c->labelmap;
    if (S.checked_classes == n_classes) return GSX_OK;
    S.checked_classes = 0;
    const long long n = (long long)c->scene.rn;
    GSX_HIP(c, S.bins8.ensure((size_t)n));
    GSX_HIP(c, S.bad.ensure(sizeof(uint32_t)));
    GSX_HIP(c, hipMemsetAsync(S.bad.p, 0xff, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(label_bins_kernel, dim3(grid_for(n)), dim3(kRB), 0, c->stream, c->scene.labels.as<int>(),
                       c->scene.order.as<uint32_t>(), n, n_classes, S.bins8.as<uint8_t>(), S.bad.as<uint32_t>());
    GSX_HIP(c, hipGetLastError());
    uint32_t bad = 0;
    GSX_HIP(c, hipMemcpyAsync(&bad, S.bad.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    if (bad != ~0u)
        return fail(c, GSX_E_RANGE, "label_view: the label of upload row %u is outside [-1, %d]", bad, n_classes - 1);
    S.checked_classes = n_classes;
    return GSX_OK;
}

// One view: a walked frame (render.hip: frame_walk_guard, frame_lists_that_fit), label_kernel walks lists that fit.
int label_view(Ctx* c, const gsx_camera* cam, int W, int H, const LabelViewArgs& a) {
    GSX_HIP(c, hipSetDevice(c->device));
    LabelMapState& S = c->labelmap;
    const char* who = "label_view";
    if (c->scene.rn <= 0) return fail(c, GSX_E_STATE, "%s: no splats uploaded (gsx_upload_splats)", who);
    if (!S.has_labels) return fail(c, GSX_E_STATE, "%s: the splats were uploaded without labels", who);
    int rc = frame_walk_guard(c, cam, W, H, who, "a label frame");
    if (rc) return rc;
    if (a.n_classes < 1 || a.n_classes > kLiftMaxBins - 1)
        return fail(c, GSX_E_INVALID, "%s: n_classes = %d must be in [1, %d]", who, a.n_classes, kLiftMaxBins - 1);
    if (!(a.min_weight >= 0.0) || !(a.min_weight <= 1.0e300)) return fail(c, GSX_E_INVALID, "%s: min_weight must be finite and >= 0", who);
    if (a.n_planes < 0 || a.n_planes > kLabelMaxPlanes)
        return fail(c, GSX_E_INVALID, "%s: n_planes = %d must be in [0, %d]", who, a.n_planes, kLabelMaxPlanes);
    if (a.n_planes > 0 && !a.plane_labels) return fail(c, GSX_E_INVALID, "%s: %d planes without plane_labels", who, a.n_planes);
    uint8_t pb[kLabelMaxPlanes] = {};  // alive until the call's last wait: the copy below may read it late
    for (int k = 0; k < a.n_planes; ++k) {
        const int v = a.plane_labels[k];
        if (v < -1 || v >= a.n_classes)
            return fail(c, GSX_E_INVALID, "%s: plane %d asks for label %d, outside [-1, %d]", who, k, v, a.n_classes - 1);
        pb[k] = (uint8_t)(v + 1);
    }
    if ((rc = label_check(c, a.n_classes))) return rc;
    const size_t npix = (size_t)W * (size_t)H;
    const int n_planes = a.planes_out ? a.n_planes : 0;
    GSX_HIP(c, S.map.ensure(4 * npix));
    if (a.weight_out) GSX_HIP(c, S.weight.ensure(4 * npix));
    if (a.total_out) GSX_HIP(c, S.total.ensure(4 * npix));
    if (n_planes) {
        GSX_HIP(c, S.plane_bins.ensure(kLabelMaxPlanes));
        GSX_HIP(c, hipMemcpyAsync(S.plane_bins.p, pb, kLabelMaxPlanes, hipMemcpyHostToDevice, c->stream));
        if (S.planes.ensure(4 * npix * (size_t)n_planes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, GSX_E_HIP, "%s: could not allocate %zu bytes for %d planes of %dx%d", who, 4 * npix * (size_t)n_planes, n_planes, W, H);
        }
    }
    const unsigned long long threshold = std::max(1ull, lift_threshold(a.min_weight));
    RenderFrame& f = c->frame;
    FramePlan fp;
    const uint32_t* vals = nullptr;
    if ((rc = frame_lists_that_fit(c, cam, W, H, who, fp, &vals))) return rc;
    {
        ProfScope ps(c, "label");
        hipLaunchKernelGGL(label_kernel, dim3(fp.ntiles), dim3(kLiftThreads), 0, c->stream, f.ranges.as<int2>(), vals,
                           f.cur->rec.as<float4>(), S.bins8.as<uint8_t>(), W, H, fp.tiles_x, threshold, n_planes,
                           S.plane_bins.as<uint8_t>(), S.map.as<int32_t>(),
                           a.weight_out ? S.weight.as<uint32_t>() : nullptr, a.total_out ? S.total.as<uint32_t>() : nullptr,
                           n_planes ? S.planes.as<uint32_t>() : nullptr, &f.small.as<FrameCounters>()->consumed[0].n);
    }
    GSX_HIP(c, hipGetLastError());
    FrameCounters stats;
    if ((rc = frame_walk_stats_queue(c, stats))) return rc;
    if (a.label_out) GSX_HIP(c, hipMemcpyAsync(a.label_out, S.map.p, 4 * npix, hipMemcpyDeviceToHost, c->stream));
    if (a.weight_out) GSX_HIP(c, hipMemcpyAsync(a.weight_out, S.weight.p, 4 * npix, hipMemcpyDeviceToHost, c->stream));
    if (a.total_out) GSX_HIP(c, hipMemcpyAsync(a.total_out, S.total.p, 4 * npix, hipMemcpyDeviceToHost, c->stream));
    if (n_planes) GSX_HIP(c, hipMemcpyAsync(a.planes_out, S.planes.p, 4 * npix * (size_t)n_planes, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    frame_walk_stats_sum(c, stats, &S.passes, &S.single);
    return GSX_OK;
}

}  // namespace gsx
