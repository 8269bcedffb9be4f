// depthmap.hip - depth frames: per pixel the blend's expected depth, the depth at which the accumulated alpha crosses a
// quantile, and the splat that crosses it.
//
// The frame is walked exactly as label_view and lift_view walk it (render.hip: frame_plan / frame_depth_order /
// frame_phase_lists, one depth phase, 16x16 tiles; lift_device.hpp: lift_fragment, -ffp-contract=off; the opacity vote after
// every staged chunk of 256 records).  A fragment's weight is the lift's q = rint(w * 2^20), a splat's depth is runSort's int32
// key as the pre pass wrote it for this view (render_pre.hip: PreGeom::depth).  Per pixel, over its fragments in walk order:
//     total   = sum of q                         (uint32, the number label_kernel writes to total_out)
//     moment  = sum of q * key                   (int64)
//     surface = the first fragment at which the running sum of q reaches cut = max(1, ceil(quantile * 2^20))
// All of it is integer arithmetic on integers two pinned kernels already form: no floating-point depth exists in this unit.
// key / 4096 = proj[10] * (z_view - view[14]), so the way back to scene units is one fp64 multiply-add on the host
// (depth_key_to_z).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "gsx_ctx.hpp"
#include "lift_device.hpp"
#include "render_device.hpp"

namespace gsx {

void depth_constants(int32_t out[8]) {
    const int32_t v[8] = {kLiftOne, kLiftShift, kLiftTile, kLiftChunk, 0, 0, 0, 0};
    for (int k = 0; k < 8; ++k) out[k] = v[k];
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------------
// One workgroup per 16x16 tile, one pixel per lane, built from the pieces of lift_device.hpp that lift_kernel and label_kernel
// walk with: 256 records staged through LDS at a time, next to s0 / s1 / sa their depth key and upload row, so that the walk
// reads LDS broadcasts only.  A lane carries dst.a, total, moment and its surface in registers: no LDS accumulators, no
// atomics, no presence pass, one walk.  total is the running sum itself: the surface is the fragment that takes it from below
// the cut to the cut or beyond (such a fragment has q > 0, as cut >= 1).
// Pixels outside the frame contribute 0, count as opaque and write nothing.  A tile without a list writes 0, 0, 0, -1 and
// returns as a whole; in every other tile no lane leaves before the last barrier.
//
// full = 0 (surface-only): neither total nor moment is wanted, and a tile may also stop once every pixel of the frame has its
// surface.  It must still stop where the full walk stops - at the opacity vote - or a pixel the full walk leaves without a
// surface could find one further down the list; and a pixel that is opaque but below the cut may not excuse the tile on its
// own, since the full walk goes on while any other pixel is open and may still give it a surface (fragments of q <= 10 each;
// it happens with quantile = 1).  So the second condition is a vote of its own, taken only where the first one fails.
__global__ __launch_bounds__(kLiftThreads) void depth_kernel(const int2* __restrict__ ranges, const uint32_t* __restrict__ vals,
                                                             const float4* __restrict__ rec, const int* __restrict__ depth,
                                                             const uint32_t* __restrict__ order, int W, int H, int tiles_x, uint32_t cut,
                                                             int full, uint32_t* __restrict__ total_out, long long* __restrict__ moment_out,
                                                             int32_t* __restrict__ key_out, int32_t* __restrict__ index_out,
                                                             unsigned long long* __restrict__ consumed) {
    __shared__ float4 s0[kLiftChunk];
    __shared__ float4 s1[kLiftChunk];
    __shared__ float sa[kLiftChunk];
    __shared__ int skey[kLiftChunk];  // a staged record's depth key in this view
    __shared__ int srow[kLiftChunk];  // ... and its upload row
    const int tile = (int)blockIdx.x;
    const int2 range = ranges[tile];
    const int tid = (int)threadIdx.x;
    const LiftPixel p = lift_pixel(tile, tiles_x, W, H, tid);
    const bool inside = p.inside;
    const size_t pix = p.pix;
    if (range.y <= range.x) {  // (workgroup-uniform) nothing reaches this tile
        if (inside) {
            if (total_out) total_out[pix] = 0u;
            if (moment_out) moment_out[pix] = 0ll;
            key_out[pix] = 0;
            index_out[pix] = -1;
        }
        return;
    }
    float a = 0.0f;  // gl.clear to (0,0,0,0): only dst.a is carried
    uint32_t total = 0u;
    long long moment = 0ll;
    int surf_key = 0, surf_row = -1;
    int staged = 0;
    for (int base = range.x; base < range.y; base += kLiftChunk) {
        const int cnt = min(kLiftChunk, range.y - base);
        __syncthreads();
        if (tid < cnt) {
            const uint32_t id = vals[base + tid];
            lift_stage(s0, s1, sa, rec, id, tid);
            skey[tid] = depth[id];
            srow[tid] = (int)order[id];
        }
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const uint32_t q = lift_weight(a, p, s0[k], s1[k], sa[k]);
            const uint32_t run = total + q;
            if (total < cut && run >= cut) surf_key = skey[k], surf_row = srow[k];
            total = run;
            if (full) moment += (long long)(int)q * (long long)skey[k];  // (workgroup-uniform)
        }
        staged += cnt;
        if (lift_tile_opaque(p, a)) break;
        if (!full && __syncthreads_and(!inside || total >= cut)) break;
    }
    if (inside) {
        if (total_out) total_out[pix] = total;
        if (moment_out) moment_out[pix] = moment;
        key_out[pix] = surf_key;
        index_out[pix] = surf_row;
    }
    // statistics: records staged, pixels with a surface
    const int surfaces = __syncthreads_count(inside && surf_row >= 0);
    if (tid == 0) {
        unsigned long long* slot = lift_stats_slot(consumed);
        atomicAdd(slot, (unsigned long long)staged);
        atomicAdd(slot + 1, (unsigned long long)surfaces);
    }
}

// the upload's exact labels by upload row (scene.labels keeps them in importance order): what depth_pick reports
__global__ __launch_bounds__(kRB) void depth_labels_kernel(const int* __restrict__ labels, const uint32_t* __restrict__ order, long long n,
                                                            int* __restrict__ by_row) {
    const long long j = (long long)blockIdx.x * kRB + threadIdx.x;
    if (j < n) by_row[order[j]] = labels[j];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
void depth_new_upload(Ctx* c) {
    c->depthmap.valid = false;
    c->depthmap.labels_ready = false;
}

// z_view = key * scale + offset.  With the viewer's matrices row 2 of proj * view is proj[10] * (view[2], view[6], view[10])
// (view[3] = 0), so key / 4096 = proj[10] * (z_view - view[14]) up to the key's truncation.
int depth_key_to_z(const gsx_camera* cam, int W, int H, double* scale, double* offset) {
    if (!cam || W < 1 || H < 1 || !scale || !offset) return fail(nullptr, GSX_E_INVALID, "depth_key_to_z: bad arguments");
    double view[16], proj[16];
    js_view_matrix(cam, view);
    js_proj_matrix(cam->fx, cam->fy, (double)W, (double)H, proj);
    *scale = 1.0 / (4096.0 * proj[10]);
    *offset = view[14];
    return GSX_OK;
}

// One view: a walked frame (render.hip: frame_walk_guard, frame_lists_that_fit), depth_kernel walks lists that fit.
int depth_view(Ctx* c, const gsx_camera* cam, int W, int H, const DepthViewArgs& a) {
    GSX_HIP(c, hipSetDevice(c->device));
    DepthMapState& S = c->depthmap;
    const char* who = "depth_view";
    if (c->scene.rn <= 0) return fail(c, GSX_E_STATE, "%s: no splats uploaded (gsx_upload_splats)", who);
    int rc = frame_walk_guard(c, cam, W, H, who, "a depth frame");
    if (rc) return rc;
    if (!(a.quantile > 0.0) || !(a.quantile <= 1.0)) return fail(c, GSX_E_INVALID, "%s: quantile = %g must be in (0, 1]", who, a.quantile);
    const size_t npix = (size_t)W * (size_t)H;
    const bool full = a.total_out || a.moment_out;
    if (4 * npix > S.index.cap || 4 * npix > S.key.cap) S.valid = false;  // the maps are about to move: the last view goes with them
    GSX_HIP(c, S.index.ensure(4 * npix));
    GSX_HIP(c, S.key.ensure(4 * npix));
    if (a.total_out) GSX_HIP(c, S.total.ensure(4 * npix));
    if (a.moment_out) GSX_HIP(c, S.moment.ensure(8 * npix));
    const uint32_t cut = (uint32_t)std::max(1.0, std::ceil(a.quantile * (double)kLiftOne));  // <= 2^20
    RenderFrame& f = c->frame;
    FramePlan fp;
    const uint32_t* vals = nullptr;
    if ((rc = frame_lists_that_fit(c, cam, W, H, who, fp, &vals))) return rc;
    S.valid = false;  // from here on the maps are this view's, and it stands once its results have arrived
    {
        ProfScope ps(c, "depth");
        hipLaunchKernelGGL(depth_kernel, dim3(fp.ntiles), dim3(kLiftThreads), 0, c->stream, f.ranges.as<int2>(), vals,
                           f.cur->rec.as<float4>(), f.cur->depth.as<int>(), c->scene.order.as<uint32_t>(), W, H, fp.tiles_x, cut,
                           full ? 1 : 0, a.total_out ? S.total.as<uint32_t>() : nullptr,
                           a.moment_out ? S.moment.as<long long>() : nullptr, S.key.as<int32_t>(), S.index.as<int32_t>(),
                           &f.small.as<FrameCounters>()->consumed[0].n);
    }
    GSX_HIP(c, hipGetLastError());
    FrameCounters stats;
    if ((rc = frame_walk_stats_queue(c, stats))) return rc;
    if (a.total_out) GSX_HIP(c, hipMemcpyAsync(a.total_out, S.total.p, 4 * npix, hipMemcpyDeviceToHost, c->stream));
    if (a.moment_out) GSX_HIP(c, hipMemcpyAsync(a.moment_out, S.moment.p, 8 * npix, hipMemcpyDeviceToHost, c->stream));
    if (a.key_out) GSX_HIP(c, hipMemcpyAsync(a.key_out, S.key.p, 4 * npix, hipMemcpyDeviceToHost, c->stream));
    if (a.index_out) GSX_HIP(c, hipMemcpyAsync(a.index_out, S.index.p, 4 * npix, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    frame_walk_stats_sum(c, stats, &S.surfaces, nullptr);
    S.W = W, S.H = H;
    (void)depth_key_to_z(cam, W, H, &S.scale, &S.offset);
    S.valid = true;
    return GSX_OK;
}

// The surface under a canvas point of the last depth view: a few bytes out of its maps, nothing is rendered.
int depth_pick(Ctx* c, double x, double y, int32_t* label_out, int64_t* index_out, double* z_out) {
    GSX_HIP(c, hipSetDevice(c->device));
    DepthMapState& S = c->depthmap;
    if (!S.valid) return fail(c, GSX_E_STATE, "depth_pick: no depth view since the last upload (gsx_depth_view)");
    int32_t label = -999999, row = -1, key = 0;  // NO_SELECTION, gs.js:6
    double z = std::nan("");
    const double col = std::floor(x), up = std::floor(y);
    if (col >= 0.0 && col < (double)S.W && up >= 0.0 && up < (double)S.H) {  // (false for a NaN)
        const size_t pix = (size_t)(S.H - 1 - (int)up) * (size_t)S.W + (size_t)(int)col;
        GSX_HIP(c, hipMemcpyAsync(&row, S.index.as<int32_t>() + pix, 4, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipMemcpyAsync(&key, S.key.as<int32_t>() + pix, 4, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
        if (row >= 0) {
            if (!S.labels_ready) {  // once per upload
                const long long n = (long long)c->scene.rn;
                GSX_HIP(c, S.labels.ensure(4 * (size_t)n));
                hipLaunchKernelGGL(depth_labels_kernel, dim3(grid_for(n)), dim3(kRB), 0, c->stream, c->scene.labels.as<int>(),
                                   c->scene.order.as<uint32_t>(), n, S.labels.as<int>());
                GSX_HIP(c, hipGetLastError());
                S.labels_ready = true;
            }
            GSX_HIP(c, hipMemcpyAsync(&label, S.labels.as<int32_t>() + row, 4, hipMemcpyDeviceToHost, c->stream));
            GSX_HIP(c, hipStreamSynchronize(c->stream));
            z = (double)key * S.scale + S.offset;
        }
    }
    if (label_out) *label_out = label;
    if (index_out) *index_out = (int64_t)row;
    if (z_out) *z_out = z;
    return GSX_OK;
}

}  // namespace gsx
