// handover.hip — segmentation maps into the seg pool that the labeler kernels of vote.hip gather from, and the pool and its
// descriptors between ranks (gsx_vote_export / gsx_vote_import*).  Votes nothing: the early vote that runs behind a hand-over is
// vote.hip's (vote_view), and the one thing this unit tells it is that the pool is about to move (early_pool_moves).
//
//   seg pool       u8 maps, value = label+1 (bin index), one after another on 256-byte boundaries, each stored as strips of
//                  16 pixel columns (rows of a strip back to back, 16 B each; 8 rows = one 128-B L2 line): the pixels a wave
//                  gathers are a compact patch, so they fall into few lines; behind the strips a 4x4-coarsened level in the
//                  same strip form (host_pack.hpp: MapLayout).  Every byte of a map's stride is written by whoever puts it there.
//
// A host map (gsx_vote_view -> vote_view_host) takes one of three transfer forms:
//   compact ring     the workers pack the coarse level + one 16-byte block per mixed cell into a pinned ring, a group of records
//                    goes up in one DMA and seg_expand_kernel rebuilds the pool form            (hand_over_compact; the default)
//   pool-form ring   the workers pack the pool form itself, a group of maps is one DMA straight into the pool
//                    (hand_over_pool_form: maps without a coarse level or strips, option host_compact = 0)
//   raw copy + pack  the map crosses PCIe as it is and seg_pack_fused_kernel packs it        (hand_over_raw: host_pack = 0)
// vote_flush_pending queues the DMA of what waits in a ring.  Device maps (gsx_vote_views_device) go through the pack kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "seg_dtype.hpp"
#include "vote_device.hpp"

namespace gsx {

// -------------------------------------------------------------------------------------------------
// seg-map packing on the device (gsx_vote_view_device / gsx_vote_views_device): ONE pass over the int32 / int64 /
// u8 map writes both levels of the library's form — the u8 bins (label + 1) in strips of 16 pixel columns and the
// 4x4-coarsened level (a cell = the bin its 16 pixels share, 255 where they differ or the cell sticks out of the
// map) — and validates the label range.  One thread = one 4x4 cell: four 16-byte loads (int32), four u32 stores
// (the four lanes of a strip write 64 contiguous bytes) and one coarse byte.  Up to kPackBatch maps of one geometry
// per launch (blockIdx.y): a 1080p map is 8 MB, i.e. ~2 us of HBM time, less than a launch.
// Every byte of the map's pool stride is written, as seg_expand_kernel and the host packer's zeroed ring do: the threads
// cover the PADDED cell grid (whole strips and bands of the coarse level, which contain those of the full-resolution
// level), cells and rows past the map are 0 in both levels, and the first workgroup of a map clears the alignment gaps.
// The pool is reused from run to run, so a byte left out would carry the previous run's data into what vote_export ships.
// -------------------------------------------------------------------------------------------------
static constexpr int kPackBatch = 16;
static constexpr int kStripCols = 16, kBandRows = 8;    // pixel columns per strip, pixel rows per band (full-resolution level)
static constexpr int kCStripCells = 16, kCBandRows = 8;  // cells per coarse strip, cell rows per coarse band
struct PackArgs {
    const void* src[kPackBatch];
    uint8_t* dst[kPackBatch];
    int view[kPackBatch];  // index reported through `err` when the map holds a label outside [-1, bins-2]
    int w, h, strip_bytes, cstrip_bytes, cw, ch, bins;
    int pw, ph;            // cells per row / column of the full-resolution level including its padding (row-major: cw, ch)
    int gw, gh;            // the cell grid the threads cover: the coarse level including its padding (no coarse level: pw, ph)
    unsigned gap_lo, coarse_off, map_bytes, stride;  // [gap_lo, coarse_off) and [map_bytes, stride) belong to no cell: zeroed
    int* err;              // atomicMin of the offending view indices (INT_MAX = none)
};

static void pack_geometry(PackArgs& a, const MapLayout& L, int bins, int* err) {
    a.w = L.w, a.h = L.h, a.strip_bytes = L.strip_bytes, a.cstrip_bytes = L.cstrip_bytes, a.cw = L.cw, a.ch = L.ch;
    a.bins = bins;
    a.pw = L.strip_bytes ? (L.w + kStripCols - 1) / kStripCols * (kStripCols / 4) : L.cw;
    a.ph = L.strip_bytes ? (L.h + kBandRows - 1) / kBandRows * (kBandRows / 4) : L.ch;
    a.gw = L.cstrip_bytes ? (L.cw + kCStripCells - 1) / kCStripCells * kCStripCells : a.pw;
    a.gh = L.cstrip_bytes ? (L.ch + kCBandRows - 1) / kCBandRows * kCBandRows : a.ph;
    a.gap_lo = (unsigned)(L.strip_bytes ? L.fine_bytes : (size_t)L.w * (size_t)L.h);  // row-major: the four tail bytes too
    a.coarse_off = (unsigned)L.coarse_off;  // no coarse level: the end of the stride
    a.map_bytes = (unsigned)L.map_bytes;
    a.stride = (unsigned)align256(L.map_bytes);
    a.err = err;
}

template <typename T, int ADD, bool VEC>
__global__ __launch_bounds__(kBlock) void seg_pack_fused_kernel(PackArgs a) {
    const int job = blockIdx.y;
    const T* __restrict__ in = static_cast<const T*>(a.src[job]);
    uint8_t* __restrict__ out = a.dst[job];
    if (blockIdx.x == 0) {  // the two alignment gaps, each shorter than 256 bytes
        for (unsigned j = a.gap_lo + threadIdx.x; j < a.coarse_off; j += kBlock) out[j] = 0;
        for (unsigned j = a.map_bytes + threadIdx.x; j < a.stride; j += kBlock) out[j] = 0;
    }
    const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int cy = (int)(q / a.gw), cx = (int)(q % a.gw);
    if (cy >= a.gh) return;
    const int x0 = cx * 4, y0 = cy * 4;
    const unsigned bins = (unsigned)a.bins;
    const bool fine_pad = a.strip_bytes && cx < a.pw && cy < a.ph;  // a cell of a strip, in the map or in its padding
    unsigned bad = 0;
    uint32_t rows[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = y0 + r;
        uint32_t packed = 0;
        if (y >= a.h || cx >= a.cw) {  // rows below the map, cells right of it: bin 0 in the strips' padding
            if (fine_pad) *reinterpret_cast<uint32_t*>(out + (long long)(x0 >> 4) * a.strip_bytes + ((long long)y << 4) + (x0 & 15)) = 0u;
        } else {
            const T* row = in + (long long)y * a.w + x0;
            T v[4];
            bool have[4];
            if (VEC) {  // host checked: w % 4 == 0 and a 16-byte aligned base, so x0 + 4 <= w and the vector is aligned
                typedef T vec4 __attribute__((ext_vector_type(4)));
                const vec4 t = *reinterpret_cast<const vec4*>(row);
                v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
                have[0] = have[1] = have[2] = have[3] = true;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    have[k] = x0 + k < a.w;
                    v[k] = have[k] ? row[k] : (T)0;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long b = (unsigned long long)(long long)v[k] + (unsigned)ADD;  // label -2 wraps far above bins
                bad |= (unsigned)(have[k] & (b >= bins));
                packed |= (have[k] ? (uint32_t)(b & 0xffu) : 0u) << (8 * k);  // columns past the edge: bin 0
            }
            if (a.strip_bytes) {
                *reinterpret_cast<uint32_t*>(out + (long long)(x0 >> 4) * a.strip_bytes + ((long long)y << 4) + (x0 & 15)) = packed;
            } else {
                const long long o = (long long)y * a.w + x0;
                if (VEC) *reinterpret_cast<uint32_t*>(out + o) = packed;
                else
                    for (int k = 0; k < 4 && x0 + k < a.w; ++k) out[o + k] = (uint8_t)(packed >> (8 * k));
            }
        }
        rows[r] = packed;
    }
    if (a.cstrip_bytes) {
        const uint32_t same = (rows[0] & 0xffu) * 0x01010101u;
        const bool uniform = x0 + 4 <= a.w && y0 + 4 <= a.h && rows[0] == same && rows[1] == same && rows[2] == same && rows[3] == same;
        const bool cell = cx < a.cw && cy < a.ch;  // else the coarse strips' padding: 0
        out[a.coarse_off + (long long)(cx >> 4) * a.cstrip_bytes + (cx & 15) + ((long long)cy << 4)] =
            uniform ? (uint8_t)(rows[0] & 0xffu) : cell ? (uint8_t)255 : (uint8_t)0;
    }
    if (bad) atomicMin(a.err, a.view[job]);
}

// -------------------------------------------------------------------------------------------------
// Host maps arrive in the COMPACT form of host_pack.hpp (coarse level + one 16-byte block per mixed 4x4 cell: the PCIe
// link, not the host pass, is what a run's hand-over waits for, and a segmentation map is mostly uniform cells).  This
// kernel, queued behind the DMA of a group of maps on a GPU that has nothing else to do while maps are handed over,
// rebuilds the pool form: one workgroup = one band of 8 pixel rows (two cell rows) of one map; a thread takes the cells of a
// cell row in the stream's order (by cell column), a ballot scan ranks the mixed ones, and every cell is written
// as four 4-byte rows - its block, or its coarse byte four times over.  The coarse level is copied as it is; every
// byte of the map's pool stride is written (cells and rows past the map, alignment gaps: 0), so a pool map stays a pure
// function of the map, which exchange protocol v4 ships.
// -------------------------------------------------------------------------------------------------
struct ExpandArgs {
    const uint8_t* rec[kCompactBatch];  // compact records in the device staging buffer
    uint8_t* map[kCompactBatch];        // their places in the pool
    int w, h, strip_bytes, cstrip_bytes, cw, ch, strips;
    unsigned table_bytes, stream_off, coarse_off, fine_bytes, map_bytes, stride;
    unsigned max_block;  // last block a cell row of this geometry can hold, counted from its first
};

__global__ __launch_bounds__(kBlock) void seg_expand_kernel(ExpandArgs a) {
    __shared__ unsigned wave_total[kBlock / 64];
    const uint8_t* __restrict__ rec = a.rec[blockIdx.y];
    uint8_t* __restrict__ map = a.map[blockIdx.y];
    const int band = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint8_t* __restrict__ coarse = rec + a.table_bytes;
    const uint32_t* __restrict__ table = reinterpret_cast<const uint32_t*>(rec);
    const uint4* __restrict__ stream = reinterpret_cast<const uint4*>(rec + a.stream_off);
    const int per = a.strips * 4;  // cells per cell row (padded to whole strips)
    for (int cyl = 0; cyl < 2; ++cyl) {  // the band's two cell rows: each has its own run of blocks in the stream
        const int cy = band * 2 + cyl;
        const unsigned first = table[2 * band + cyl];
        unsigned running = 0;  // mixed cells of this cell row before the current round
        for (int i0 = 0; i0 < per; i0 += kBlock) {
            const int cx = i0 + tid;
            const bool valid = cx < per;
            const int s = cx >> 2, cc = cx & 3;
            const bool cell = valid && cy < a.ch && cx < a.cw;
            const unsigned cb = cell ? coarse[(size_t)(cx >> 4) * a.cstrip_bytes + (cx & 15) + ((size_t)cy << 4)] : 0u;
            const bool mixed = cell && cb == 255u;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(mixed);
            const unsigned below = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            __syncthreads();  // the previous round's totals have been read
            if (lane == 0) wave_total[wv] = (unsigned)__popcll(m);
            __syncthreads();
            unsigned before = running;
#pragma unroll
            for (int k = 0; k < kBlock / 64; ++k) {
                before += k < wv ? wave_total[k] : 0u;
                running += wave_total[k];
            }
            if (valid) {
                uint32_t r0, r1, r2, r3;
                if (mixed) {
                    const uint4 b = stream[first + min(before + below, a.max_block)];  // (a record is the library's own: the clamp never acts)
                    r0 = b.x, r1 = b.y, r2 = b.z, r3 = b.w;
                } else {
                    r0 = r1 = r2 = r3 = cb * 0x01010101u;  // a uniform cell; 0 for the cells and rows past the map
                }
                uint8_t* o = map + (size_t)s * a.strip_bytes + ((size_t)(band * 8 + cyl * 4) << 4) + cc * 4;
                *reinterpret_cast<uint32_t*>(o) = r0;
                *reinterpret_cast<uint32_t*>(o + 16) = r1;
                *reinterpret_cast<uint32_t*>(o + 32) = r2;
                *reinterpret_cast<uint32_t*>(o + 48) = r3;
            }
        }
    }
    // the coarse level, verbatim (16-byte pieces dealt over the bands), and the alignment gaps
    const unsigned cbytes = a.map_bytes - a.coarse_off;  // a multiple of 128
    for (unsigned j = (unsigned)band * kBlock + tid; j < cbytes / 16; j += gridDim.x * kBlock)
        reinterpret_cast<uint4*>(map + a.coarse_off)[j] = reinterpret_cast<const uint4*>(coarse)[j];
    if (band == 0) {
        for (unsigned j = a.fine_bytes + tid; j < a.coarse_off; j += kBlock) map[j] = 0;
        for (unsigned j = a.map_bytes + tid; j < a.stride; j += kBlock) map[j] = 0;
    }
}

// -------------------------------------------------------------------------------------------------
// host side: the pool
// -------------------------------------------------------------------------------------------------
static int pool_reserve(Ctx* c, size_t need) {
    if (need <= c->run.segpool.cap) return GSX_OK;
    int rc = vote_flush_pending(c);  // the pool is about to move: maps still waiting in the pinned ring go up first
    if (rc) return rc;
    if ((rc = early_pool_moves(c))) return rc;  // ... and an early stage may be reading the pool that is about to be freed
    size_t cap = c->run.segpool.cap ? c->run.segpool.cap : ((size_t)64 << 20);
    while (cap < need) cap *= 2;
    void* np = nullptr;
    GSX_HIP(c, hipMalloc(&np, cap));
    if (c->run.seg_used) {
        hipError_t e = hipMemcpyAsync(np, c->run.segpool.p, c->run.seg_used, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            (void)hipFree(np);
            return fail(c, GSX_E_HIP, "seg pool growth copy failed: %s", hipGetErrorString(e));
        }
    }
    c->run.segpool.release();
    c->run.segpool.p = np;
    c->run.segpool.cap = cap;
    return GSX_OK;
}

// ---- seg-map hand-over ------------------------------------------------------------------------------------------
// Common front part of gsx_vote_view / gsx_vote_views_device: argument checks, the map's layout, room in the pool.
static int view_prologue(Ctx* c, const char* who, const void* cams, const void* seg, int n, int seg_dtype, int seg_w, int seg_h,
                         int img_w, int img_h, MapLayout& L) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "%s before vote_begin", who);
    if (c->run.pool_base) return fail(c, GSX_E_STATE, "%s after gsx_vote_import: the run's views are final; start the next one with gsx_vote_begin", who);
    if (!cams || !seg) return fail(c, GSX_E_INVALID, "%s: NULL argument", who);
    if (seg_w < 1 || seg_h < 1 || img_w < 1 || img_h < 1)
        return fail(c, GSX_E_INVALID, "%s: sizes must be positive (seg %dx%d, image %dx%d)", who, seg_w, seg_h, img_w, img_h);
    if (seg_w > 65535 || seg_h > 65535)  // in-map byte offsets are 32-bit, row products use 24-bit multiplies
        return fail(c, GSX_E_RANGE, "%s: segmentation map %dx%d exceeds 65535 pixels a side", who, seg_w, seg_h);
    if (!seg_dtype_known(seg_dtype)) return fail(c, GSX_E_INVALID, "%s: unknown seg_dtype %d", who, seg_dtype);
    if (c->run.first_view + (int)c->run.views.size() + n > c->run.total_views)
        return fail(c, GSX_E_RANGE, "%s: more views than total_views=%d announced at vote_begin", who, c->run.total_views);
    if (c->run.local_codes && (int)c->run.views.size() + n > kMaxBatch)
        return fail(c, GSX_E_RANGE, "%s: the all-to-all exchange keeps 8-bit per-rank counters: at most %d views per rank", who,
                    kMaxBatch);
    GSX_HIP(c, hipSetDevice(c->device));
    // bin 255 must be free to mean "mixed" in the coarse level
    L = map_layout(seg_w, seg_h, c->vopt.seg_tiled != 0, c->vopt.seg_coarse && c->run.bins <= 255);
    if (L.map_bytes > 0xffffffffull) return fail(c, GSX_E_RANGE, "%s: segmentation map %dx%d exceeds 4 GiB", who, seg_w, seg_h);
    const size_t stride = align256(L.map_bytes);  // 256-B aligned maps
    const size_t off = align256(c->run.seg_used);
    size_t need = off + stride * (size_t)n;
    if (c->run.views.empty()) {
        // first view of a run: room for all announced views of this geometry at once (capped), so that the pool is
        // not re-allocated and copied while maps stream in
        const size_t all = stride * (size_t)(c->run.total_views - c->run.first_view);
        need = std::max(need, std::min(all, (size_t)32 << 30));
    }
    return pool_reserve(c, need);
}

// The host descriptor of a view whose map of layout L lies `off` bytes into the pool
static void map_view_desc(ViewDesc& vd, const gsx_camera* cam, const MapLayout& L, unsigned long long off, int img_w, int img_h) {
    fill_view_desc(vd, cam, L.w, L.h, img_w, img_h);
    vd.seg_off = (long long)off;
    vd.seg_row_bytes = L.strip_bytes;
    vd.coarse_row_bytes = L.cstrip_bytes;
    vd.coarse_delta = (unsigned)L.coarse_off;
}

static void push_view(Ctx* c, const gsx_camera* cam, const MapLayout& L, size_t off, int img_w, int img_h) {
    ViewDesc vd;
    map_view_desc(vd, cam, L, off, img_w, img_h);
    c->run.views.push_back(vd);
    c->run.views_dirty = true;
    c->run.seg_used = off + L.map_bytes;
    c->run.labels_valid = false;
}

static void launch_pack(Ctx* c, const PackArgs& a, int jobs, int seg_dtype, bool vec) {
    using K = void (*)(PackArgs);
    static const K table[4][2] = {{seg_pack_fused_kernel<int32_t, 1, false>, seg_pack_fused_kernel<int32_t, 1, true>},
                                  {seg_pack_fused_kernel<int64_t, 1, false>, seg_pack_fused_kernel<int64_t, 1, true>},
                                  {seg_pack_fused_kernel<uint8_t, 0, false>, seg_pack_fused_kernel<uint8_t, 0, true>},
                                  {seg_pack_fused_kernel<uint8_t, 1, false>, seg_pack_fused_kernel<uint8_t, 1, true>}};
    ProfScope ps(c, "seg_pack");
    hipLaunchKernelGGL(table[seg_dtype][vec ? 1 : 0], dim3(grid_for((long long)a.gw * a.gh), jobs), dim3(kBlock), 0, c->stream, a);
}

void segpack_constants(int32_t out[8]) {
    out[0] = kBlock;
    out[1] = kPackBatch;
    out[2] = kStripCols;
    out[3] = kBandRows;
    out[4] = kCStripCells;
    out[5] = kCBandRows;
    out[6] = kDmaBatch;
    out[7] = kCompactBatch;
}

// near: a buffer the pool is about to read (the first map of a run): the workers are placed on its NUMA node
Workers* host_workers(Ctx* c, const void* near) {
    if (!c->ho.workers) {
        try {
            c->ho.workers.reset(new Workers(c->vopt.host_threads > 0 ? c->vopt.host_threads : default_host_threads(), numa_node_of(near)));
        } catch (...) {  // out of memory (a thread that cannot be started is handled inside: the pool then has one thread)
        }
    }
    return c->ho.workers.get();  // nullptr: single-threaded packing on the calling thread
}

// ---- host maps (gsx_vote_view): the three transfer forms ------------------------------------------------------------------
// The two ring forms: the worker threads narrow the map into the pinned ring (u8 strips + coarse level, range checked on the
// way: an out-of-range label fails THIS call), one asynchronous DMA per group moves the packed maps up.  No synchronisation;
// the call returns as soon as the caller's buffer has been read.
static constexpr int kRingSlots = kDmaBatch * kDmaGroups;

// First map, or a new geometry or form: re-lay the ring as kRingSlots slots of slot_bytes.
static int relay_ring(Ctx* c, size_t slot_bytes, bool compact) {
    int rc = vote_flush_pending(c);
    if (rc) return rc;
    for (Event& ev : c->ho.hring_ev) GSX_HIP(c, ev.wait());
    GSX_HIP(c, c->ho.hring.ensure(slot_bytes * kRingSlots));
    if (!compact) std::memset(c->ho.hring.p, 0, slot_bytes * kRingSlots);  // the bytes between a map's end and its stride travel too
    c->ho.hring_slot = slot_bytes;
    c->ho.hring_compact = compact;
    c->ho.hring_next = 0;
    c->ho.cgrp = 0;
    c->ho.grp_recs = 0;
    return GSX_OK;
}

// The last views of the run (as announced to vote_begin) go up one by one: a group waiting for more maps would put its DMA
// between the last hand-over and the vote.
static bool run_tail(const Ctx* c) { return c->run.total_views - c->run.first_view - (int)c->run.views.size() < kDmaBatch; }

// Compact ring: records of a group lie back to back (a record is as long as its map has mixed cells): one DMA per group moves
// exactly the bytes in use, and a group takes as many records as fit (at most kCompactBatch).
static int hand_over_compact(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, const MapLayout& L, const CompactLayout& CL,
                             size_t slot_bytes, int img_w, int img_h) {
    int rc = GSX_OK;
    const size_t off = align256(c->run.seg_used);
    const size_t gcap = (size_t)kDmaBatch * slot_bytes;
    if (c->ho.grp_recs == 0) {
        GSX_HIP(c, c->ho.hring_ev[c->ho.cgrp].wait());  // the group's previous DMA must have left the buffer
        c->ho.grp_used = 0;
    }
    if (c->ho.h_scratch_cap < L.fine_bytes) {
        c->ho.h_scratch.reset();  // the old block goes before the new one comes
        c->ho.h_scratch_cap = 0;
        const size_t cap = (L.fine_bytes + 4095) / 4096 * 4096;
        c->ho.h_scratch.reset(static_cast<uint8_t*>(std::aligned_alloc(4096, cap)));
        if (!c->ho.h_scratch) return fail(c, GSX_E_HIP, "vote_view: out of host memory");
        c->ho.h_scratch_cap = cap;
    }
    uint8_t* rec = c->ho.hring.as<uint8_t>() + (size_t)c->ho.cgrp * gcap + c->ho.grp_used;
    size_t blocks = 0;
    if (!(c->vopt.ablate & 2) &&  // timing experiment only: the DMA stream without the host pass; results invalid
        host_pack_map_compact(host_workers(c, seg), seg, seg_dtype, L, c->run.bins, c->ho.h_scratch.get(), rec, &blocks))
        return fail(c, GSX_E_RANGE, "vote_view: segmentation map holds a label outside [-1, %d]", c->run.n_classes - 1);
    if (c->ho.pend_count && (L.w != c->ho.pend_L.w || L.h != c->ho.pend_L.h)) {  // one expansion launch = one geometry
        if ((rc = vote_flush_pending(c))) return rc;
    }
    if (!c->ho.pend_count) {
        c->ho.pend_group = c->ho.cgrp;
        c->ho.pend_lo = c->ho.grp_used;
        c->ho.pend_L = L;
    }
    c->ho.pend_rec[c->ho.pend_count] = c->ho.grp_used;
    c->ho.pend_map[c->ho.pend_count] = off;
    ++c->ho.pend_count;
    ++c->ho.grp_recs;
    c->ho.grp_used += align256(CL.stream_off + blocks * 16);
    c->ho.compact_bytes += CL.stream_off + blocks * 16;
    push_view(c, cam, L, off, img_w, img_h);
    const bool full = c->ho.grp_recs == kCompactBatch || c->ho.grp_used + slot_bytes > gcap;  // no room for a worst-case record
    const bool tail = run_tail(c);
    if (tail || full) rc = vote_flush_pending(c);
    if (full) {
        c->ho.cgrp = (c->ho.cgrp + 1) % kDmaGroups;
        c->ho.grp_recs = 0;
    }
    return rc;
}

// Pool-form ring: a slot = the pool stride of the geometry, so consecutive packed maps are consecutive in the ring and in the pool.
static int hand_over_pool_form(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, const MapLayout& L, size_t stride, int img_w,
                               int img_h) {
    int rc = GSX_OK;
    const size_t off = align256(c->run.seg_used);
    const int s = c->ho.hring_next, g = s / kDmaBatch;
    if (s % kDmaBatch == 0) GSX_HIP(c, c->ho.hring_ev[g].wait());  // the group's previous DMA must have left the buffer
    uint8_t* slot = c->ho.hring.as<uint8_t>() + (size_t)s * stride;
    if (!(c->vopt.ablate & 2) && host_pack_map(host_workers(c, seg), seg, seg_dtype, L, c->run.bins, slot))
        return fail(c, GSX_E_RANGE, "vote_view: segmentation map holds a label outside [-1, %d]", c->run.n_classes - 1);
    if (c->ho.pend_count && off != c->ho.pend_dst + (size_t)c->ho.pend_count * stride) {  // the pool moved on (device maps in between)
        if ((rc = vote_flush_pending(c))) return rc;
    }
    if (!c->ho.pend_count) {
        c->ho.pend_first = s;
        c->ho.pend_dst = off;
    }
    ++c->ho.pend_count;
    c->ho.compact_bytes += stride;
    push_view(c, cam, L, off, img_w, img_h);
    c->ho.hring_next = (s + 1) % kRingSlots;
    const bool tail = run_tail(c);
    if (tail || c->ho.pend_count == kDmaBatch || c->ho.hring_next % kDmaBatch == 0) return vote_flush_pending(c);
    return GSX_OK;
}

// Raw copy + GPU pack.  The alternative this library does NOT default to (kept for hosts short of cores, and as the A/B of
// DESIGN.md §3): the raw map crosses PCIe (8.3 MB instead of 2.2 MB per 1080p int32 map) and the fused kernel packs it on the
// GPU.  The range check is then the device-side one (reported with the labels).
static int hand_over_raw(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, const MapLayout& L, int img_w, int img_h) {
    PinSlot& slot = c->ho.ring[c->ho.ring_next];
    GSX_HIP(c, slot.ev.wait());
    const size_t raw = seg_elem_size(seg_dtype) * (size_t)L.w * (size_t)L.h;
    // room for the raw map and for its packed form, whichever is larger; a slot that grows gets the packed form's MiB at least
    GSX_HIP(c, slot.buf.ensure(std::max(L.map_bytes, raw), (L.map_bytes + ((size_t)1 << 20) - 1) >> 20 << 20));
    DevBuf& land = c->ho.dstage[c->ho.ring_next];
    GSX_HIP(c, land.ensure(raw));
    host_copy(host_workers(c, seg), slot.buf.p, seg, raw);
    GSX_HIP(c, hipMemcpyAsync(land.p, slot.buf.p, raw, hipMemcpyHostToDevice, c->stream));
    const size_t off = align256(c->run.seg_used);
    PackArgs a{};
    a.src[0] = land.p;
    a.dst[0] = c->run.segpool.as<uint8_t>() + off;
    a.view[0] = c->run.first_view + (int)c->run.views.size();
    pack_geometry(a, L, c->run.bins, c->run.errflag.as<int>());
    launch_pack(c, a, 1, seg_dtype, L.w % 4 == 0);
    GSX_HIP(c, hipGetLastError());
    GSX_HIP(c, slot.ev.record(c->stream));  // after the kernel: it is the last reader of this slot's landing zone
    c->ho.ring_next = (c->ho.ring_next + 1) % kPinSlots;
    push_view(c, cam, L, off, img_w, img_h);
    return GSX_OK;
}

int vote_view_host(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, int seg_w, int seg_h, int img_w, int img_h) {
    MapLayout L;
    int rc = view_prologue(c, "vote_view", cam, seg, 1, seg_dtype, seg_w, seg_h, img_w, img_h, L);
    if (rc) return rc;
    if (!c->vopt.host_pack) return hand_over_raw(c, cam, seg, seg_dtype, L, img_w, img_h);
    const size_t stride = align256(L.map_bytes);
    // compact transfer form (host_pack.hpp) whenever the pool form has both levels; else the pool form itself
    const bool compact = c->vopt.host_compact && L.strip_bytes && L.cstrip_bytes;
    const CompactLayout CL = compact ? compact_layout(L) : CompactLayout{};
    const size_t slot_bytes = compact ? align256(CL.capacity) : stride;
    if (c->ho.hring_slot != slot_bytes || !c->ho.hring.p || c->ho.hring_compact != compact) {
        if ((rc = relay_ring(c, slot_bytes, compact))) return rc;
    }
    return compact ? hand_over_compact(c, cam, seg, seg_dtype, L, CL, slot_bytes, img_w, img_h)
                   : hand_over_pool_form(c, cam, seg, seg_dtype, L, stride, img_w, img_h);
}

// Device maps (all of one geometry and dtype): kPackBatch maps per launch of the fused pack kernel.  Nothing is
// read back: a label out of range is recorded on the device and reported by the call that hands out the labels.
int vote_views_device(Ctx* c, int n, const gsx_camera* cams, const void* const* segs, int seg_dtype, int seg_w, int seg_h,
                      int img_w, int img_h) {
    if (n <= 0) return n == 0 ? GSX_OK : fail(c, GSX_E_INVALID, "vote_views_device: n < 0");
    MapLayout L;
    int rc = view_prologue(c, "vote_views_device", cams, segs, n, seg_dtype, seg_w, seg_h, img_w, img_h, L);
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (!segs[i]) return fail(c, GSX_E_INVALID, "vote_views_device: map %d is NULL", i);
    const size_t esz = seg_elem_size(seg_dtype);
    for (int i0 = 0; i0 < n; i0 += kPackBatch) {
        const int m = std::min(kPackBatch, n - i0);
        PackArgs a{};
        bool vec = seg_w % 4 == 0;
        size_t off = 0;
        for (int k = 0; k < m; ++k) {
            off = align256(c->run.seg_used);
            a.src[k] = segs[i0 + k];
            a.dst[k] = c->run.segpool.as<uint8_t>() + off;
            a.view[k] = c->run.first_view + (int)c->run.views.size();
            vec = vec && reinterpret_cast<uintptr_t>(segs[i0 + k]) % (4 * esz) == 0;
            push_view(c, cams + i0 + k, L, off, img_w, img_h);
        }
        pack_geometry(a, L, c->run.bins, c->run.errflag.as<int>());
        launch_pack(c, a, m, seg_dtype, vec);
        GSX_HIP(c, hipGetLastError());
    }
    return GSX_OK;
}

// One DMA for the packed maps that wait in the filling group of the pinned ring (up to kDmaBatch consecutive slots =
// consecutive pool offsets).  Called when the group is full, for each of the last maps of a run, and by everything that
// needs the maps on the device.
int vote_flush_pending(Ctx* c) {
    if (!c->ho.pend_count) return GSX_OK;
    GSX_HIP(c, hipSetDevice(c->device));
    if (c->ho.hring_compact) {
        const int g = c->ho.pend_group;
        const size_t gcap = (size_t)kDmaBatch * c->ho.hring_slot;
        GSX_HIP(c, c->ho.cstage.ensure(gcap));
        const uint8_t* src = c->ho.hring.as<uint8_t>() + (size_t)g * gcap;
        if (!(c->vopt.ablate & 1))  // timing experiment only (tools/tail_probe.py): the host pass without its DMA; results invalid
            GSX_HIP(c, hipMemcpyAsync(c->ho.cstage.as<uint8_t>() + c->ho.pend_lo, src + c->ho.pend_lo, c->ho.grp_used - c->ho.pend_lo, hipMemcpyHostToDevice,
                                      c->stream));
        GSX_HIP(c, c->ho.hring_ev[g].record(c->stream));
        const MapLayout& L = c->ho.pend_L;
        const CompactLayout CL = compact_layout(L);
        ExpandArgs a{};
        for (int k = 0; k < c->ho.pend_count; ++k) {
            a.rec[k] = c->ho.cstage.as<uint8_t>() + c->ho.pend_rec[k];
            a.map[k] = c->run.segpool.as<uint8_t>() + c->ho.pend_map[k];
        }
        a.w = L.w, a.h = L.h, a.strip_bytes = L.strip_bytes, a.cstrip_bytes = L.cstrip_bytes, a.cw = L.cw, a.ch = L.ch;
        a.strips = (L.w + 15) / 16;
        a.table_bytes = (unsigned)CL.table_bytes, a.stream_off = (unsigned)CL.stream_off, a.coarse_off = (unsigned)L.coarse_off;
        a.fine_bytes = (unsigned)L.fine_bytes, a.map_bytes = (unsigned)L.map_bytes, a.stride = (unsigned)align256(L.map_bytes);
        a.max_block = (unsigned)(L.cw - 1);
        if (!(c->vopt.ablate & 3)) {  // (an ablation of the hand-over leaves no valid record to expand)
            ProfScope ps(c, "seg_expand");
            hipLaunchKernelGGL(seg_expand_kernel, dim3((unsigned)CL.bands, (unsigned)c->ho.pend_count), dim3(kBlock), 0, c->stream, a);
            GSX_HIP(c, hipGetLastError());
        }
        c->ho.pend_count = 0;
        return GSX_OK;
    }
    const int g = c->ho.pend_first / kDmaBatch;
    const size_t bytes = (size_t)c->ho.pend_count * c->ho.hring_slot;
    if (!(c->vopt.ablate & 1))
        GSX_HIP(c, hipMemcpyAsync(c->run.segpool.as<uint8_t>() + c->ho.pend_dst, c->ho.hring.as<uint8_t>() + (size_t)c->ho.pend_first * c->ho.hring_slot,
                                  bytes, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, c->ho.hring_ev[g].record(c->stream));
    c->ho.pend_count = 0;
    // a group that was flushed before it was full keeps filling: its later slots are not in flight, and the event (recorded
    // again by the next flush) always stands for the group's LAST copy, which is what the next lap waits for
    return GSX_OK;
}

int host_threads(Ctx* c) {
    Workers* w = host_workers(c);
    return w ? w->threads() : 1;
}

// test hook, host only: the packed form of one map exactly as gsx_vote_view stages it
int debug_host_pack(const void* seg, int seg_dtype, int w, int h, int n_classes, int tiled, int coarse, int threads,
                    uint8_t* out, int64_t out_cap, int64_t* bytes, int64_t* coarse_off, int32_t* bad) {
    if (!seg || w < 1 || h < 1 || w > 65535 || h > 65535 || n_classes < 1 || n_classes > 255 || !seg_dtype_known(seg_dtype))
        return fail(nullptr, GSX_E_INVALID, "debug_host_pack: bad arguments");
    const MapLayout L = map_layout(w, h, tiled != 0, coarse != 0 && n_classes + 1 <= 255);
    if (bytes) *bytes = (int64_t)L.map_bytes;
    if (coarse_off) *coarse_off = L.cstrip_bytes ? (int64_t)L.coarse_off : -1;
    if (!out) return GSX_OK;
    if (out_cap < (int64_t)L.map_bytes) return fail(nullptr, GSX_E_INVALID, "debug_host_pack: output buffer too small");
    Workers pool(threads > 0 ? threads : 1);
    const int b = host_pack_map(&pool, seg, seg_dtype, L, n_classes + 1, out);
    if (bad) *bad = b;
    return GSX_OK;
}

// test hook, host only: the compact transfer form of one map (host_pack.hpp), as gsx_vote_view writes it into the pinned ring
int debug_host_pack_compact(const void* seg, int seg_dtype, int w, int h, int n_classes, int threads, uint8_t* out, int64_t out_cap,
                            int64_t* bytes, int64_t* table_bytes, int64_t* stream_off, int32_t* bad) {
    if (!seg || w < 1 || h < 1 || w > 65535 || h > 65535 || n_classes < 1 || n_classes > 254 || !seg_dtype_known(seg_dtype) || !bytes)
        return fail(nullptr, GSX_E_INVALID, "debug_host_pack_compact: bad arguments");
    const MapLayout L = map_layout(w, h, true, true);
    const CompactLayout CL = compact_layout(L);
    if (table_bytes) *table_bytes = (int64_t)CL.table_bytes;
    if (stream_off) *stream_off = (int64_t)CL.stream_off;
    *bytes = (int64_t)CL.capacity;
    if (!out) return GSX_OK;
    if (out_cap < (int64_t)CL.capacity) return fail(nullptr, GSX_E_INVALID, "debug_host_pack_compact: output buffer too small");
    void* scratch = std::aligned_alloc(4096, (L.fine_bytes + 4095) / 4096 * 4096);
    if (!scratch) return fail(nullptr, GSX_E_HIP, "debug_host_pack_compact: out of memory");
    Workers pool(threads > 0 ? threads : 1);
    size_t blocks = 0;
    const int b = host_pack_map_compact(&pool, seg, seg_dtype, L, n_classes + 1, static_cast<uint8_t*>(scratch), out, &blocks);
    std::free(scratch);
    if (bad) *bad = b;
    *bytes = (int64_t)(CL.stream_off + blocks * 16);
    return GSX_OK;
}

// ---- exchange v4 host side: views sharded for the hand-over, Gaussians sharded for the vote ------------------------
// The packed maps of 200 1080p views are 0.44 GB; the dense vote histogram of 3 M Gaussians is 0.45 GB PER RANK.  So
// the maps travel (one all-gather), not the votes: afterwards every rank holds every view, votes its own slab of
// the Gaussians with the single-GPU kernel, and only 4 bytes per Gaussian (the labels) are gathered.  No histogram,
// no tie-break exchange: a slab sees all views in order, the tie rule is the single-GPU one.
int vote_export(Ctx* c, int64_t reserve_bytes, void* blobs_out, void** pool_dev, int64_t* pool_bytes) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_export before vote_begin");
    if (c->run.pool_base) return fail(c, GSX_E_STATE, "vote_export after vote_import");
    GSX_HIP(c, hipSetDevice(c->device));
    if (reserve_bytes < 0) return fail(c, GSX_E_INVALID, "vote_export: negative size");
    if (const int rc = vote_flush_pending(c)) return rc;  // the caller is about to read the pool (all-gather)
    const size_t used = align256(c->run.seg_used);
    int rc = pool_reserve(c, std::max<size_t>(std::max<size_t>((size_t)reserve_bytes, used), 256));
    if (rc) return rc;
    c->run.views_dirty = true;  // the pool may have moved
    static_assert(sizeof(ViewDesc) == GSX_VIEW_BLOB_BYTES, "view blob size is part of the ABI");
    if (blobs_out && !c->run.views.empty()) std::memcpy(blobs_out, c->run.views.data(), sizeof(ViewDesc) * c->run.views.size());
    if (pool_dev) *pool_dev = c->run.segpool.p;
    if (pool_bytes) *pool_bytes = (int64_t)used;
    return GSX_OK;
}

// The imported views replace the rank's own; those are kept aside so that gsx_vote_import_undo can put them back (a protocol
// that imports optimistically and then learns that a peer's pool was not what the schedule assumed falls back to the plain
// exchange, which starts from the rank's own views again).
static void import_commit(Ctx* c, std::vector<ViewDesc>& all, const void* pool_all_dev) {
    if (!c->run.pool_base) {  // (a second import on top of an import keeps the first one's saved state)
        c->run.own_views.swap(c->run.views);
        c->run.own_first_view = c->run.first_view;
    }
    c->run.views.swap(all);
    c->run.views_dirty = true;
    c->run.pool_base = pool_all_dev;
    c->run.first_view = 0;
    c->run.n_flushed = 0;
    c->run.labels_valid = false;
}

int vote_import_undo(Ctx* c) {
    if (!c->run.begun || !c->run.pool_base) return fail(c, GSX_E_STATE, "vote_import_undo without a gsx_vote_import");
    c->run.views.swap(c->run.own_views);
    c->run.own_views.clear();
    c->run.first_view = c->run.own_first_view;
    c->run.pool_base = nullptr;
    c->run.views_dirty = true;
    c->run.n_flushed = 0;
    c->run.labels_valid = false;
    return GSX_OK;
}

int vote_import(Ctx* c, int n_parts, const int32_t* part_views, const int64_t* part_offsets, const void* blobs,
                const void* pool_all_dev, int64_t pool_all_bytes) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_import before vote_begin");
    if (n_parts < 1 || !part_views || !part_offsets || !pool_all_dev || pool_all_bytes < 0)
        return fail(c, GSX_E_INVALID, "vote_import: bad arguments");
    long long total = 0;
    for (int r = 0; r < n_parts; ++r) {
        if (part_views[r] < 0 || part_offsets[r] < 0) return fail(c, GSX_E_INVALID, "vote_import: negative count or offset");
        total += part_views[r];
    }
    if (total > 65535) return fail(c, GSX_E_RANGE, "vote_import: %lld views exceed 65535", total);
    if (total > 0 && !blobs) return fail(c, GSX_E_INVALID, "vote_import: blobs is NULL");
    std::vector<ViewDesc> all((size_t)total);
    if (total) std::memcpy(all.data(), blobs, sizeof(ViewDesc) * (size_t)total);
    size_t k = 0;
    for (int r = 0; r < n_parts; ++r)
        for (int v = 0; v < part_views[r]; ++v, ++k) {
            ViewDesc& d = all[k];
            // the blob comes from another process: check what the kernels rely on before any address is formed from it
            const MapLayout L = map_layout(d.seg_w, d.seg_h, d.seg_row_bytes != 0, d.coarse_row_bytes != 0);
            const bool ok = d.seg_w >= 1 && d.seg_h >= 1 && d.seg_w <= 65535 && d.seg_h <= 65535 && d.seg_off >= 0 &&
                            d.seg_row_bytes == L.strip_bytes && d.coarse_row_bytes == L.cstrip_bytes &&
                            (!d.coarse_row_bytes || d.coarse_delta == (unsigned)L.coarse_off) &&
                            (unsigned long long)d.seg_off + (unsigned long long)part_offsets[r] + L.map_bytes <= (unsigned long long)pool_all_bytes;
            if (!ok) return fail(c, GSX_E_INVALID, "vote_import: descriptor %zu (part %d) is inconsistent with the gathered pool", k, r);
            d.seg_off += part_offsets[r];
            d.hw32 = (float)d.half_w;  // (never trusted from the blob: the filter's proof needs exactly these)
            d.hh32 = (float)d.half_h;
        }
    import_commit(c, all, pool_all_dev);
    return GSX_OK;
}

// gsx_vote_import without the blobs: every rank of a run holds the whole camera list (cameras.json) and, when all maps of the
// run share ONE geometry, knows where view k of part r lies in the gathered buffer - part_offsets[r] + k * stride, the stride
// gsx_vote_view gives a map of that geometry under this context's options (all ranks run the same build with the same
// options).  So the descriptors are derived here, the same way gsx_vote_view derives them (fill_view_desc + map_layout),
// and the header exchange of the blobs and its host wait disappear from the protocol.
static MapLayout uniform_layout(const Ctx* c, int seg_w, int seg_h) {
    return map_layout(seg_w, seg_h, c->vopt.seg_tiled != 0, c->vopt.seg_coarse && c->run.bins <= 255);  // as view_prologue
}
// a staged view has the map geometry that (L, image size) derive: everything of a descriptor that does not come from the camera
static bool same_geometry(const ViewDesc& d, const MapLayout& L, int img_w, int img_h) {
    return d.seg_w == L.w && d.seg_h == L.h && d.wscale == (double)L.w / (double)img_w && d.hscale == (double)L.h / (double)img_h &&
           d.seg_row_bytes == L.strip_bytes && d.coarse_row_bytes == L.cstrip_bytes && d.coarse_delta == (unsigned)L.coarse_off;
}

int vote_map_stride(Ctx* c, int seg_w, int seg_h, int64_t* stride) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_map_stride before vote_begin (the layout depends on the number of classes)");
    if (!stride) return fail(c, GSX_E_INVALID, "vote_map_stride: NULL argument");
    if (seg_w < 1 || seg_h < 1 || seg_w > 65535 || seg_h > 65535) return fail(c, GSX_E_INVALID, "vote_map_stride: map %dx%d", seg_w, seg_h);
    const MapLayout L = uniform_layout(c, seg_w, seg_h);
    *stride = (int64_t)align256(L.map_bytes);
    return GSX_OK;
}

// Are this context's own views exactly views [0, n) of a uniform run as gsx_vote_import_uniform would derive them: n of them, view i
// from cams[i] with this map and image size, at byte i * stride of the pool?  A rank asks before it votes on a schedule that assumes so.
int vote_views_match_uniform(Ctx* c, int n, const gsx_camera* cams, int seg_w, int seg_h, int img_w, int img_h, int32_t* match) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_views_match_uniform before vote_begin");
    if (c->run.pool_base) return fail(c, GSX_E_STATE, "vote_views_match_uniform after gsx_vote_import: the context holds imported views");
    if (n < 0 || (n > 0 && !cams) || !match) return fail(c, GSX_E_INVALID, "vote_views_match_uniform: bad arguments");
    if (seg_w < 1 || seg_h < 1 || img_w < 1 || img_h < 1 || seg_w > 65535 || seg_h > 65535)
        return fail(c, GSX_E_INVALID, "vote_views_match_uniform: map %dx%d, image %dx%d", seg_w, seg_h, img_w, img_h);
    const MapLayout L = uniform_layout(c, seg_w, seg_h);
    const size_t stride = align256(L.map_bytes);
    *match = 0;
    if ((size_t)n != c->run.views.size()) return GSX_OK;
    for (int i = 0; i < n; ++i) {
        ViewDesc d;
        map_view_desc(d, &cams[i], L, (size_t)i * stride, img_w, img_h);
        if (std::memcmp(&d, &c->run.views[(size_t)i], sizeof d) != 0) return GSX_OK;  // (fill_view_desc zeroes the padding)
    }
    *match = 1;
    return GSX_OK;
}

int vote_import_uniform(Ctx* c, int n_parts, const int32_t* part_views, const int64_t* part_offsets, const gsx_camera* cams,
                        int seg_w, int seg_h, int img_w, int img_h, const void* pool_all_dev, int64_t pool_all_bytes) {
    if (!c->run.begun) return fail(c, GSX_E_STATE, "vote_import_uniform before vote_begin");
    if (n_parts < 1 || !part_views || !part_offsets || !pool_all_dev || pool_all_bytes < 0)
        return fail(c, GSX_E_INVALID, "vote_import_uniform: bad arguments");
    if (seg_w < 1 || seg_h < 1 || img_w < 1 || img_h < 1 || seg_w > 65535 || seg_h > 65535)
        return fail(c, GSX_E_INVALID, "vote_import_uniform: map %dx%d, image %dx%d", seg_w, seg_h, img_w, img_h);
    long long total = 0;
    for (int r = 0; r < n_parts; ++r) {
        if (part_views[r] < 0 || part_offsets[r] < 0) return fail(c, GSX_E_INVALID, "vote_import_uniform: negative count or offset");
        total += part_views[r];
    }
    if (total > 65535) return fail(c, GSX_E_RANGE, "vote_import_uniform: %lld views exceed 65535", total);
    if (total > 0 && !cams) return fail(c, GSX_E_INVALID, "vote_import_uniform: cams is NULL");
    const MapLayout L = uniform_layout(c, seg_w, seg_h);
    const size_t stride = align256(L.map_bytes);
    // the caller laid the parts out with a stride of its own: parts that overlap at THIS stride were sized for another geometry
    std::vector<std::pair<unsigned long long, unsigned long long>> spans;  // (first byte, bytes) of the parts that hold views
    for (int r = 0; r < n_parts; ++r)
        if (part_views[r] > 0) spans.emplace_back((unsigned long long)part_offsets[r], (unsigned long long)part_views[r] * stride);
    std::sort(spans.begin(), spans.end());
    for (size_t s = 0; s + 1 < spans.size(); ++s)
        if (spans[s].first + spans[s].second > spans[s + 1].first)
            return fail(c, GSX_E_INVALID, "vote_import_uniform: the part offsets leave less than %llu bytes a view, the stride of a %dx%d map",
                        (unsigned long long)stride, seg_w, seg_h);
    // what this context staged itself is part of the run: its geometry must be the one the descriptors are derived for
    for (const ViewDesc& o : c->run.pool_base ? c->run.own_views : c->run.views)
        if (!same_geometry(o, L, img_w, img_h))
            return fail(c, GSX_E_INVALID, "vote_import_uniform: map %dx%d / image %dx%d, but gsx_vote_view staged a %dx%d map (scales %g, %g)",
                        seg_w, seg_h, img_w, img_h, o.seg_w, o.seg_h, o.wscale, o.hscale);
    std::vector<ViewDesc> all((size_t)total);
    size_t k = 0;
    for (int r = 0; r < n_parts; ++r)
        for (int v = 0; v < part_views[r]; ++v, ++k) {
            const unsigned long long off = (unsigned long long)part_offsets[r] + (unsigned long long)v * stride;
            if (off + L.map_bytes > (unsigned long long)pool_all_bytes)
                return fail(c, GSX_E_INVALID, "vote_import_uniform: view %zu (part %d) lies outside the gathered pool", k, r);
            map_view_desc(all[k], &cams[k], L, off, img_w, img_h);
        }
    import_commit(c, all, pool_all_dev);
    return GSX_OK;
}

}  // namespace gsx
