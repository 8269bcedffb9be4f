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
// One workgroup per 16x16 tile, one pixel per lane, modelled on lift_kernel: 256 records staged through LDS at a time, every
// pixel walks them carrying only dst.a, the opacity vote falls after every staged chunk.  Pixels outside the frame contribute
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
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int px = tx * kLiftTile + (tid & (kLiftTile - 1));
    const int py = ty * kLiftTile + (tid >> 4);
    const bool inside = px < W && py < H;
    const size_t npix = (size_t)W * (size_t)H;
    const size_t pix = (size_t)py * (size_t)W + (size_t)px;  // used only where inside
    if (range.y <= range.x) {  // (workgroup-uniform) nothing reaches this tile
        if (inside) {
            label_out[pix] = -1;
            if (weight_out) weight_out[pix] = 0u;
            if (total_out) total_out[pix] = 0u;
            for (int k = 0; k < n_planes; ++k) planes_out[(size_t)k * npix + pix] = 0u;
        }
        return;
    }
    const float fxp = (float)px + 0.5f;               // pixel centre, GL window coordinates
    const float fyp = (float)H - ((float)py + 0.5f);  // window y is up; image row py counts from the top
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
                s0[tid] = rec[3 * (size_t)id];
                s1[tid] = rec[3 * (size_t)id + 1];
                sa[tid] = reinterpret_cast<const float2*>(rec + 3 * (size_t)id + 2)->y;
                sslot[tid] = (uint8_t)rank256(pw, (uint32_t)bins8[id]);
            }
            __syncthreads();
            for (int k = 0; k < cnt; ++k) {
                const float w = lift_fragment(a, fxp, fyp, s0[k], s1[k], sa[k]);
                const uint32_t q = inside && w > 0.0f ? (uint32_t)rintf(w * (float)kLiftOne) : 0u;  // <= 2^20: w <= 1
                const uint32_t s = (uint32_t)sslot[k] - (uint32_t)lo;  // (workgroup-uniform)
                if (s < (uint32_t)kLabelWindow && q) atomicAdd(&acc[s * kLiftThreads + tid], q);  // no result used: one LDS add
            }
            if (win == 0) staged += cnt;
            // every further fragment is weighted by (1 - dst.a): the frame's rule, a tile stops once that is < 1e-5 on all of it
            if (__syncthreads_and(!inside || a > 1.0f - 1.0e-5f)) break;
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
    // statistics, spread over kConsumedSlots lines like the blend kernels': records staged by the first walk, walks, one-label tiles
    if (tid == 0) {
        unsigned long long* slot = consumed + (blockIdx.x & (kConsumedSlots - 1)) * 16;
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

// One view.  The frame's front and the handling of the pair count are lift_view's: the counters are read back once the lists
// stand, the buffers grow and the lists are rebuilt until they fit, and only then label_kernel walks them.
int label_view(Ctx* c, const gsx_camera* cam, int W, int H, const LabelViewArgs& a) {
    GSX_HIP(c, hipSetDevice(c->device));
    LabelMapState& S = c->labelmap;
    const char* who = "label_view";
    if (c->scene.rn <= 0) return fail(c, GSX_E_STATE, "%s: no splats uploaded (gsx_upload_splats)", who);
    if (!S.has_labels) return fail(c, GSX_E_STATE, "%s: the splats were uploaded without labels", who);
    if (c->scene.edits_on)
        return fail(c, GSX_E_STATE, "%s: a render edit state is set (gsx_render_set_edits): a label frame through an edited frame is not defined", who);
    if (c->frame.pre_ext >= 0 || c->frame.in_flight) return fail(c, GSX_E_STATE, "%s: gsx_render_views is running on this context", who);
    if (!cam || W < 1 || H < 1) return fail(c, GSX_E_INVALID, "%s: bad arguments (camera, width %d, height %d)", who, W, H);
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
    const int tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16;
    if (tiles_x > 256 || tiles_y > 256) return fail(c, GSX_E_UNSUPPORTED, "%s: %dx%d exceeds 4096 pixels per side", who, W, H);
    int rc = label_check(c, a.n_classes);
    if (rc) return rc;
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
    const double scaled = std::ceil(a.min_weight * (double)kLiftOne);
    const unsigned long long threshold =
        scaled >= 18446744073709551615.0 ? ~0ull : std::max(1ull, (unsigned long long)scaled);
    RenderFrame& f = c->frame;
    FramePlan fp;
    if ((rc = frame_plan(c, W, H, false, 1, fp))) return rc;
    FrameCounters* fc = f.small.as<FrameCounters>();
    FrameCounters stats;
    for (int attempt = 0;; ++attempt) {
        const size_t cap = f.pair_cap;
        if ((rc = frame_depth_order(c, cam, fp))) return rc;
        const uint32_t* vals = nullptr;
        if ((rc = frame_phase_lists(c, fp, 0, 1, &vals))) return rc;
        GSX_HIP(c, hipMemcpyAsync(&stats, fc, sizeof stats, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
        const unsigned long long P = stats.pairs[0];
        if (P > 0x7fffffffull)
            return fail(c, GSX_E_RANGE, "%s: %llu (tile, splat) pairs exceed 2^31-1 (a close-up of a very large scene)", who, P);
        if (P > cap) {  // EMIT wrote nothing and the ranges are empty: grow, rebuild the lists
            if (attempt >= 2) return fail(c, GSX_E_STATE, "%s: pair buffers overflowed three times in a row", who);
            f.pair_cap = (size_t)(P + P / 4 + 4096);
            continue;
        }
        f.P = P;
        {
            ProfScope ps(c, "label");
            hipLaunchKernelGGL(label_kernel, dim3(fp.ntiles), dim3(kLiftThreads), 0, c->stream, f.ranges.as<int2>(), vals,
                               f.cur->rec.as<float4>(), S.bins8.as<uint8_t>(), W, H, tiles_x, threshold, n_planes,
                               S.plane_bins.as<uint8_t>(), S.map.as<int32_t>(),
                               a.weight_out ? S.weight.as<uint32_t>() : nullptr, a.total_out ? S.total.as<uint32_t>() : nullptr,
                               n_planes ? S.planes.as<uint32_t>() : nullptr, &fc->consumed[0].n);
        }
        GSX_HIP(c, hipGetLastError());
        break;
    }
    GSX_HIP(c, hipMemcpyAsync(&stats, fc, sizeof stats, hipMemcpyDeviceToHost, c->stream));
    if (a.label_out) GSX_HIP(c, hipMemcpyAsync(a.label_out, S.map.p, 4 * npix, hipMemcpyDeviceToHost, c->stream));
    if (a.weight_out) GSX_HIP(c, hipMemcpyAsync(a.weight_out, S.weight.p, 4 * npix, hipMemcpyDeviceToHost, c->stream));
    if (a.total_out) GSX_HIP(c, hipMemcpyAsync(a.total_out, S.total.p, 4 * npix, hipMemcpyDeviceToHost, c->stream));
    if (n_planes) GSX_HIP(c, hipMemcpyAsync(a.planes_out, S.planes.p, 4 * npix * (size_t)n_planes, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    f.consumed = 0;
    S.passes = S.single = 0;
    for (const FrameCounters::Slot& slot : stats.consumed) {
        f.consumed += slot.n;
        S.passes += slot.atomics;
        S.single += slot.single;
    }
    return GSX_OK;
}

}  // namespace gsx
