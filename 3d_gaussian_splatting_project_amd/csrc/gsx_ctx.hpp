// Internal (non-ABI) state of libgsx.so.  Everything here is private to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <cstddef>
#include <string>
#include <vector>

#include "../../include/gsx.h"
#include "host_pack.hpp"

namespace gsx {

// ---- error plumbing ----------------------------------------------------------------------------
void set_global_error(const char* fmt, ...);
struct Ctx;
int fail(Ctx* c, int code, const char* fmt, ...);

#define GSX_HIP(ctx, call)                                                                         \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return gsx::fail((ctx), GSX_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                             __FILE__, __LINE__);                                                  \
    } while (0)

// ---- device buffer: grows, never shrinks ---------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool owned = true;  // false: an alias of another context's buffer (gsx_render_views' twin): never freed or regrown here
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), owned(o.owned) { o.p = nullptr; o.cap = 0; o.owned = true; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            cap = o.cap;
            owned = o.owned;
            o.p = nullptr;
            o.cap = 0;
            o.owned = true;
        }
        return *this;
    }
    void alias(const DevBuf& o) {  // view of o's memory; o must outlive this
        release();
        p = o.p;
        cap = o.cap;
        owned = false;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes) {  // contents are NOT preserved on growth
        if (bytes <= cap) return hipSuccess;
        if (!owned) return hipErrorInvalidValue;  // an alias cannot grow
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release() {
        if (p && owned) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        owned = true;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// ---- pinned host buffer: grows, never shrinks ------------------------------------------------------
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            cap = o.cap;
            o.p = nullptr;
            o.cap = 0;
        }
        return *this;
    }
    ~PinBuf() { release(); }
    // contents are NOT preserved on growth; reserve: the caller's growth rule (what a buffer that has to grow is given, at least need).
    // Nothing may still be copying out of or into the old block: the caller waits for the event that guards it first.
    hipError_t ensure(size_t need, size_t reserve = 0) {
        if (need <= cap) return hipSuccess;
        release();
        const size_t bytes = need > reserve ? need : reserve;
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes;
        else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// ---- event without timing, created at its first record ----------------------------------------------
struct Event {
    hipEvent_t e = nullptr;
    bool pending = false;  // recorded, and the host has not waited for it since
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e(o.e), pending(o.pending) { o.e = nullptr; o.pending = false; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            destroy();
            e = o.e;
            pending = o.pending;
            o.e = nullptr;
            o.pending = false;
        }
        return *this;
    }
    ~Event() { destroy(); }
    hipError_t record(hipStream_t stream) {
        if (!e) {
            const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (r != hipSuccess) {
                e = nullptr;
                return r;
            }
        }
        const hipError_t r = hipEventRecord(e, stream);
        if (r == hipSuccess) pending = true;
        return r;
    }
    hipError_t wait() {  // the host waits for the last record, once
        if (!pending) return hipSuccess;
        const hipError_t r = hipEventSynchronize(e);
        if (r == hipSuccess) pending = false;
        return r;
    }
    hipError_t stream_wait(hipStream_t stream) const { return hipStreamWaitEvent(stream, e, 0); }  // after a record only
    void destroy() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
        pending = false;
    }
};

// ---- per-view descriptor read by the kernels through scalar (wave-uniform) loads ------------------
struct alignas(64) ViewDesc {
    // ---- core, 128 B = two s_load_dwordx16: everything that differs from view to view in an ordinary capture ----
    double R[9];        // cameras.json rotation, row-major                         (dls.py:60)
    double t[3];        // (-R) @ p in the dgemv association of the oracle           (dls.py:66)
    double fx, fy;      //                                                           (dls.py:54-55)
    long long seg_off;  // host copy: byte offset of this view's u8 map in the seg pool; device copy
                        // (sync_views): the map's absolute address
    int seg_row_bytes;  // bytes per strip of 16 pixel columns (0: row-major map)
    int unit_scale;     // both scales are exactly 1.0 and the camera frame fits the map: skip scale + clamp
    // ---- frame, 48 B: identical for all views when the cameras share one resolution (then kernel constants) ----
    double half_w, half_h;  // width/2, height/2                                    (dls.py:76-77)
    double width, height;   // bounds of the visibility test                        (dls.py:80)
    int seg_w, seg_h;
    int cam_w, cam_h;   // camera width / height as integers (visibility test of the filtered projection)
    int coarse_row_bytes;   // bytes per strip of 16 coarse cells (0: this view has no coarse level)
    unsigned coarse_delta;  // byte offset of the coarse level from the map's own start
    float hw32, hh32;       // half_w, half_h as floats (exact: the frame is <= 65535 pixels a side): the fp32 filter of the projection
    // ---- cold part: only read on the scale + clamp path (dls.py:270-286) ----
    double wscale, hscale;  // seg_w/img_w, seg_h/img_h                             (dls.py:270-271)
};
static_assert(sizeof(ViewDesc) == 256 && offsetof(ViewDesc, wscale) == 192, "ViewDesc layout");

// one slot of the pinned staging ring of gsx_vote_view (host maps): packed by the host workers, DMA'd to the pool
struct PinSlot {
    PinBuf buf;
    Event ev;  // recorded after the slot's H2D copy
};
static constexpr int kPinSlots = 4;
static constexpr int kDmaBatch = 4;    // packed host maps per H2D copy (one hipMemcpyAsync + event record costs ~6 us of host time)
static constexpr int kCompactBatch = 16;  // compact records per H2D copy and expansion launch (as many as fit into a group's part of the ring)
static constexpr int kDmaGroups = 3;   // ring = kDmaGroups groups of kDmaBatch slots: one filling, one or two in flight
static constexpr int kLabelChunks = 4;
static constexpr int kConsumedSlots = 64;  // rasterizer statistics: the blend kernels' "pairs staged" counter, one slot per 128-B line
static constexpr int kNoBadView = 0x7f7f7f7f;  // errflag value meaning "every device-side map was in range"

// A frame's counters (RenderFrame::small), zeroed when the frame starts and read back when it ends.  The kernels get pointers
// into it; the layout is what it has always been.
constexpr int kMaxPhases = 8;
struct FrameCounters {
    int unused0[2];
    int dropped;                          // bucket_kernel: splats outside the 16-bit bucket range (the blend's epilogue draws them)
    int unused1[3];
    unsigned long long pairs[kMaxPhases]; // the scan's grand total of phase p: its (list, splat) pairs
    unsigned long long unused2;
    unsigned long long nvis;              // splats the level-1 sort kept (those with a rectangle in this view)
    unsigned long long unused3[19];
    struct alignas(128) Slot {
        unsigned long long n;
        unsigned long long atomics;       // lift_kernel: global atomics it issued (same line, same spreading); label_kernel: list walks;
                                          // depth_kernel: pixels with a surface
        unsigned long long single;        // label_kernel: tiles whose list holds one label bin
    } consumed[kConsumedSlots];           // pairs the blend kernels staged: one counter per 128-B line (summed at the end of the frame)
};
static_assert(offsetof(FrameCounters, dropped) == 8 && offsetof(FrameCounters, pairs) == 24 && offsetof(FrameCounters, nvis) == 96 &&
                  offsetof(FrameCounters, consumed) == 256 && sizeof(FrameCounters::Slot) == 128 &&
                  sizeof(FrameCounters) == 256 + (size_t)kConsumedSlots * 128,
              "FrameCounters layout");

struct ProfEvent {
    int name_id;
    hipEvent_t start, stop;
};

// ---- small expressions with one spelling -----------------------------------------------------------------------------
// maps, records and staging areas start on 256-byte boundaries
constexpr size_t align256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// State of the segmentation-map hand-over (handover.hip): worker pool, the pinned rings of the three transfer forms and the
// packed maps that wait for their DMA.  Plain data; only handover.hip (and the option "host_threads") writes it.
struct HandOver {
    std::unique_ptr<Workers> workers;  // created at first use (host_workers), dropped by the option "host_threads"
    DevBuf dstage[kPinSlots];  // host_pack = 0: device-side landing zone of the raw map of each ring slot
    PinSlot ring[kPinSlots];   // host_pack = 0: raw maps
    int ring_next = 0;
    // host_pack = 1: ONE pinned buffer of kDmaGroups * kDmaBatch slots, a slot = the pool stride of the map geometry, so that
    // consecutive packed maps are consecutive both here and in the pool and a whole group goes up in one DMA
    PinBuf hring;
    size_t hring_slot = 0;
    Event hring_ev[kDmaGroups];  // recorded behind a group's DMA; pending: the group's slots may not be rewritten yet
    int hring_next = 0;
    int pend_first = 0, pend_count = 0;  // packed maps of the filling group whose DMA has not been queued yet
    size_t pend_dst = 0;
    // compact transfer form: the records of a group lie back to back in its part of the ring
    bool hring_compact = false;
    size_t grp_used = 0;                 // bytes of the filling group in use
    size_t pend_lo = 0;                  // where the pending records start in the group
    size_t pend_rec[kCompactBatch] = {}; // their offsets in the group
    size_t pend_map[kCompactBatch] = {}; // their maps' offsets in the pool
    int cgrp = 0, grp_recs = 0;          // the filling group and the records it holds
    int pend_group = 0;                  // group of the pending records
    MapLayout pend_L;                    // their geometry (one expansion launch = one geometry)
    DevBuf cstage;                       // device staging of one group of records
    struct Free {
        void operator()(void* p) const { std::free(p); }
    };
    std::unique_ptr<uint8_t, Free> h_scratch;  // host: the narrowed strips of the map being packed (ordinary memory, page aligned)
    size_t h_scratch_cap = 0;
    long long compact_bytes = 0;         // statistics: bytes of host maps sent over PCIe since vote_begin (compact records or pool form)
    void begin_run() {  // vote_begin: packed maps of an abandoned run that never went up are forgotten with it
        pend_count = 0;
        compact_bytes = 0;
    }
};

// ---- state of the vote: plain data, members of Ctx ---------------------------------------------------------------------------
// The options the vote, the hand-over and the early stage read (gsx_set_option writes them, nothing else does).
struct VoteOpts {
    int spatial_sort = 1;    // Morton-order the Gaussians at upload (results do not depend on it)
    int xcd_swizzle = 32;    // 0: off, 1: contiguous eighths of the Morton curve per XCD, C: chunks of C workgroups round-robin
    int vote_unroll = 8;     // views whose seg gathers are in flight together: 1, 2, 4 or 8
    int slabs = 1;           // see VoteRun::slabs (takes effect at the next vote_begin)
    int local_codes = 0;     // see VoteRun::local_codes
    int seg_tiled = 1;       // store seg maps as 16x8-pixel tiles of 128 B
    int batched_counts = 1;  // > 255 views on one GPU: per-batch count planes + sparse tie pass instead of 16-bit planes
    int seg_coarse = 1;      // keep a 4x4-coarsened level of every tiled map (views staged after the call)
    int flat_project = 1;    // branchless projection block (exact divisions, one predicate at the end)
    int wave_cull = 1;       // skip (wave, view) pairs whose 64 Gaussians provably all miss the frame
    int filter_project = 1;  // fp32 filter in front of the two fp64 divisions of the projection (vote.hip: project_filtered); exact by construction
    int host_threads = 0;    // 0: default_host_threads()
    int host_compact = 1;    // host maps cross PCIe in the compact form (coarse level + the mixed cells' blocks), expanded on the GPU
    int labels_u8 = 1;       // 1: the labels cross PCIe as one byte each (bin = label + 1) and are widened by the workers; 0: as int32
    int host_pack = 1;       // 1: host maps are narrowed to u8 by the workers (2.2 MB/map over PCIe); 0: raw copy + GPU pack kernel (8.3 MB/map)
    int early_vote = 1;      // 0: off, 1: for runs worth it (one rank holds all <= 255 views, a large scene), 2: whenever possible (tests)
    int early_at = 0;        // the stage starts when this many permille of the announced views are staged; 0: chosen from the run's own hand-over rate
    int early_replay = 1;    // 1 (default since round 3): the early stage only records the votes, the last stage replays them (vote_record_kernel / vote_fused_replay_kernel); 0: count + first-view planes and the fold
#ifdef GSX_EXPERIMENTS  // `make experiments` only (libgsx_experiments.so, used by tools/): timing-only switches, results invalid
    int ablate = 0;          // 1 = host maps are packed but not copied, 2 = copied but not packed (handover.hip); << 4: last-stage ablations (vote.hip)
#else
    static constexpr int ablate = 0;  // the product library has no such option: every branch on it folds away
#endif
};

// One run, gsx_vote_begin .. the next one.
struct VoteRun {
    // fixed by vote_begin (begin_run)
    bool begun = false;
    int n_classes = 0, bins = 0;
    int first_view = 0, total_views = 0;
    bool wide = false;         // 16-bit plane counters (total_views > 255)
    bool local_codes = false;  // planes hold per-rank u8 counters and LOCAL first-view codes (all-to-all exchange)
    int slabs = 1;             // planes are [slab][bins][sn]; one slab per rank of the all-to-all exchange
    int64_t sn = 0;            // Gaussians per slab (multiple of 256)
    int64_t n_pad = 0;         // slabs * sn: row pitch of the vote planes (after an upload: n rounded up to 256)
    // filled by the hand-over (handover.hip); sync_views (vote.hip) derives the device copies from it
    std::vector<ViewDesc> views;
    bool views_dirty = true;    // host views newer than d_views
    bool views_simple = false;  // every staged view: unit scale + tiled map (set by sync_views)
    bool views_coarse = false;  // ... and a coarse level (set by sync_views)
    size_t seg_used = 0;
    const void* pool_base = nullptr;  // gsx_vote_import: the maps live in a caller-owned gathered pool, not in segpool
    std::vector<ViewDesc> own_views;  // gsx_vote_import: this rank's own views, for gsx_vote_import_undo
    int own_first_view = 0;
    int n_flushed = 0;          // views [0, n_flushed) are already in the planes
    bool labels_valid = false;
    // on the device
    DevBuf d_views;
    DevBuf d_cull;              // double[25][cull_pitch]: five world-space culling planes per staged view
    int cull_pitch = 0;
    DevBuf d_cull_tally;        // u64: (wave, view) pairs skipped by the culling since the last reset
    DevBuf segpool;
    DevBuf errflag;             // int: smallest view index whose device-side map held a label out of range (kNoBadView: none)
    void begin_run(const VoteOpts& o, int64_t n, int classes, int first, int total) {
        n_classes = classes;
        bins = classes + 1;
        first_view = first;
        total_views = total;
        local_codes = o.local_codes != 0;
        wide = total > 255 && !local_codes;
        slabs = o.slabs > 0 ? o.slabs : 1;
        sn = ((n + slabs - 1) / slabs + 255) / 256 * 256;
        if (sn == 0) sn = 256;
        n_pad = sn * slabs;
        views.clear();
        views_dirty = true;
        pool_base = nullptr;
        seg_used = 0;
        n_flushed = 0;
        labels_valid = false;
    }
};

// What cnt / fv hold.  Stale: a rewound run's votes; the next fresh flush overwrites them (vote.hip: clear_stale_planes)
enum class PlaneState { None, Zero, Votes, Stale };
// The layout gsx_vote_flush_counts / gsx_vote_tie_codes last wrote into cnt / codes: their kernels write the Gaussians (whole
// workgroups of them) only, so the pad entries behind them are zero as long as the layout is still this one.  Default: none.
struct PlaneLayout {
    long long n = -1, npad = -1, sn = -1;
    int bins = -1;
    bool operator==(const PlaneLayout& o) const { return n == o.n && npad == o.npad && sn == o.sn && bins == o.bins; }
};
struct VotePlanes {
    DevBuf cnt, fv;             // [bins][n_pad] counters / first-view codes (u8 or u16)
    DevBuf keys, labels;        // [n_pad] int32
    DevBuf labels8;             // [n] u8: bin = label + 1, what labels_to_host sends over PCIe
    DevBuf bcnt, bcodes;        // > 255 views on one GPU: per-batch u8 count planes [S][bins][n_pad], tie codes u16 [S][n_pad]
    DevBuf cand, codes;         // exchange v3: candidate masks u32[8][sn] of this slab; tie codes u16[n_pad]
    PlaneState state = PlaneState::None;
    PlaneLayout counts, tie_codes;  // of cnt and of codes (u16 [n_pad]: neither slabs nor bins shape them, so only n and npad are set)
    bool holds() const { return state != PlaneState::None; }  // cnt / fv are allocated for this run and defined
    void begin_run() { state = PlaneState::None; }
};

// Early vote (vote.hip: early_vote_stage): the views [0, done) are voted on the second stream while the host is still handing
// over the rest of the run; vote_finalize then only walks the views behind them.
enum class EarlyPhase { Idle, Started, Off };  // not started in this run; started; not available any more (rewind, pool moved)
struct EarlyVote {
    EarlyPhase phase = EarlyPhase::Idle;
    int done = 0;               // views [0, done) are in ecnt / efv (or, > 255 announced views, in the first `batches` planes of bcnt)
    int batches = 0;            // > 255 announced views: batches of labels_batched() whose count kernels already ran on stream2
    bool replayed = false;      // this run's early stage was a record-only one
    bool inflight = false;      // done_ev was recorded on stream2 and the context's stream has not been ordered behind it yet (early_join)
    std::chrono::steady_clock::time_point t0;  // first gsx_vote_view of the run
    Event maps_ev, done_ev, up_ev;  // stream2 behind the maps; the stage's end; the staging buffer's last upload
    DevBuf ecnt, efv;           // u8 [wave][bin][64]: counts / first-view codes of the early views
    DevBuf erec;                // u8 [wave][view][64]: bin + 1 voted by each Gaussian in each early view
    DevBuf e_views, e_cull;     // descriptors and culling planes (pitch kEarlyPitch) of the run's views, filled stage by stage
    PinBuf h_stage;             // pinned staging of both
    void begin_run() {
        phase = EarlyPhase::Idle;
        done = 0;
        batches = 0;
    }
    void drop() {  // this run is voted in one piece
        phase = EarlyPhase::Off;
        batches = 0;
    }
};

// Pinned staging between the vote and the host (vote.hip): each buffer is guarded by the events recorded behind its copies.
struct VoteStaging {
    PinBuf labels;  // n u8 bins (label + 1) + one int (the error flag) land here before the caller's array (labels_to_host)
    Event labels_ev[kLabelChunks];
    PinBuf views;   // view descriptors + culling planes on their way to d_views / d_cull (sync_views)
    Event views_ev;
};

// ---- state of the rasterizer: plain data, three members of Ctx ------------------------------------------------------------
// What exists once per scene: written by the upload (render_scene.hip) or by gsx_render_set_edits, only read by a frame.
struct RenderScene {
    int64_t rn = 0;             // splats uploaded
    DevBuf order, buffer, tex;  // importance permutation, .splat rows, texel pairs
    DevBuf fdc, shc;            // f_dc (source order); SH coefficients coef[k][c][i] (importance order)
    bool sh_on = false;
    int sh_deg = 0;
    // label edits (gsx_render_set_edits): the exact int32 labels in importance order (kept from the upload), and per state a
    // 16-bit code per splat, the tables (render_device.hpp: EditTables) and the sorted hidden labels
    DevBuf labels, edit_code, edit_tab, edit_hidden;
    bool edits_on = false;
    int64_t edit_hidden_n = 0;  // splats the state hides
    // a twin's view of its parent's scene: EVERY buffer aliased, every scalar copied (o must outlive this)
    void alias(const RenderScene& o) {
        rn = o.rn;
        order.alias(o.order), buffer.alias(o.buffer), tex.alias(o.tex);
        fdc.alias(o.fdc), shc.alias(o.shc);
        sh_on = o.sh_on, sh_deg = o.sh_deg;
        labels.alias(o.labels), edit_code.alias(o.edit_code), edit_tab.alias(o.edit_tab), edit_hidden.alias(o.edit_hidden);
        edits_on = o.edits_on, edit_hidden_n = o.edit_hidden_n;
    }
};

// The rasterizer's options (gsx_set_option); a twin gets them with `=`.
struct RenderOpts {
    int blend_pk2 = 2;     // 0 = one pixel per thread, 1 = two (packed fp32), 2 = four, one wave per tile (default since round 3)
    int exact_cull = 0;    // keep only the tiles the splat's ellipse really reaches (pairs -23 %; the test costs more than the sort saves)
    int tile_lpt = 0;      // launch the tiles with the longest lists first (blend -3 %, but net 0)
    int phases = 2;        // depth phases per frame (1 = bin and sort every pair at once)
    int phase_ratio = 6;   // phase p ends at nvis / ratio^(K-1-p) splats (front to back; nvis = the splats with a rectangle in the view; 4 until the level-1 sort left the others out)
    int bin32 = 1;         // bin, sort and range the splats by 32x32-pixel BINS (2x2 tiles); a pair carries the mask of the bin's tiles
                           // the splat's rectangle covers (one-wave blend kernel, no exact_cull, < 2^28 splats; else 16x16)
    int compact = 1;       // the level-1 sort leaves out the splats without a rectangle in the view (its first pass is the partition)
    int wide_sort = 1;     // the pair sorts in ONE pass when the list index fits 11 bits (sort.hip: radix_sort_values_wide; the ranges come with it):
                           // 0 never, 1 for a frame on its own (gsx_render_view), 2 also with several frames in flight
    int frames = 4;        // frames in flight in gsx_render_views (1 .. kMaxFrames): 935 / 1252 / 1359 / 1396 views/s with 1 / 2 / 3 / 4
    int multi_pre = 1;     // gsx_render_views: one pre pass per group of frames in flight (0: every frame its own)
    int share_stream = 1;  // gsx_render_views: the first extra frame runs on the context's second stream instead of one more stream
};
static constexpr int kMaxFrames = 6;

// gsx_render_views with several frames in flight: ONE pre pass per group of frames (pre_multi_kernel) writes the per-view
// records of all of them; a frame's records live in one of three rotating sets so that the pass for group g + 1 can run
// while the frames of group g (and stragglers of g - 1) still read theirs
struct PreSet {
    DevBuf depth, rect, rec;
    DevBuf pre;  // int[4]: min depth, max depth, splat 0's tile rectangle (written by the pre pass)
};
static constexpr int kPreSets = 3;

// What one frame in flight owns (the context's own frame and every twin's).
struct RenderFrame {
    DevBuf image;                      // float4[H][W] of the last view
    DevBuf ranges, small, scan, bucket, count, offset;
    DevBuf d0, d1, d2, d3;             // level-1 sort ping-pong (bucket, splat)
    DevBuf keys0, keys1, vals0, vals1;
    DevBuf rects;                      // the tile rectangles of a phase's splats in the phase's order (bin COUNT -> EMIT)
    DevBuf sat;                        // u8 per tile: every pixel is opaque (1 - alpha < 1e-5): later depth phases skip it
    DevBuf tile_order;                 // blend launch order (longest list first)
    PreSet sets[kPreSets];
    PreSet* cur = nullptr;             // the set the frame being rendered reads (set by render_view: sets[0] for a frame on its own)
    size_t pair_cap = 0;               // capacity (pairs) of keys* / vals*: grown when a phase overflows it, the frame is redone
    unsigned long long P = 0;          // (tile, splat) pairs of the last view (all phases)
    unsigned long long consumed = 0;   // pairs the blend kernel actually staged (early-out leaves the rest unread)
    int bin32 = 0;                     // the frame being rendered uses bins (set by render_view, read by launch_blend)
    bool in_flight = false;            // this context renders one of several frames in flight (set by render_views for the call)
    int pre_ext = -1;                  // >= 0: this frame's pre pass has been run for it into sets[pre_ext] (render_view skips its own)
};

// A frame up to and including its per-list ranges (render.hip: frame_plan / frame_depth_order / frame_phase_lists): what
// gsx_render_view and a lift frame (lift.hip) share.  Plain data, filled by frame_plan.
struct FramePlan {
    int W = 0, H = 0, tiles_x = 0, tiles_y = 0, ntiles = 0;
    int nlists = 0;                    // lists the pairs are sorted into: tiles, or 32x32-pixel bins
    int tile_bits = 1, K = 1;          // key bits of a list index; depth phases
    bool bin32 = false, wide = false, ext_pre = false;
    size_t sat_bytes = 0;
    long long n = 0;
    long long divs[kMaxPhases + 1] = {};  // phase p = [nvis / divs[p], nvis / divs[p + 1]); divs[0] = 0 stands for the start
    const uint32_t* by_depth = nullptr;   // the splats front to back (frame_depth_order)
};

// State of a lift run (lift.hip): gsx_lift_begin .. the next gsx_upload_splats
struct LiftState {
    bool begun = false;
    int n_classes = 0, views = 0;
    DevBuf table;                      // u64 [n][n_classes + 1], rows in importance order
    DevBuf bins;                       // u8 [H][W]: the view's map, bin = label + 1
    DevBuf raw;                        // a host map on its way to the narrowing kernel
    DevBuf flag;                       // int: smallest view whose device map held a label out of range (kNoBadView: none)
    DevBuf out;                        // finalize: int32 labels [n] | double shares [n], upload order
    unsigned long long atomics = 0;    // global atomics lift_kernel issued for the last view
};

// State of the label frames (labelmap.hip): what gsx_label_view keeps between calls
struct LabelMapState {
    bool has_labels = false;           // the last gsx_upload_splats came with labels
    int checked_classes = 0;           // bins8 holds the upload's labels, all within [-1, checked_classes - 1] (0: not checked yet)
    DevBuf bins8;                      // u8 [n], importance order: bin = label + 1
    DevBuf bad;                        // u32: the lowest upload row whose label is out of range (~0: none)
    DevBuf map;                        // int32 [H][W]: the last view's map (gsx_label_map_device)
    DevBuf weight, total;              // u32 [H][W]: the winner's sum and the pixel's total, when asked for
    DevBuf planes;                     // u32 [n_planes][H][W]
    DevBuf plane_bins;                 // u8 [256]: the bins of the planes asked for
    unsigned long long passes = 0;     // list walks summed over the tiles of the last view
    unsigned long long single = 0;     // tiles of the last view whose list held one label bin
};

// State of the depth frames (depthmap.hip): what gsx_depth_view keeps between calls
struct DepthMapState {
    bool valid = false;                // index / key hold a view of the current upload (gsx_depth_pick, the device maps)
    int W = 0, H = 0;                  // ... of this size
    double scale = 0.0, offset = 0.0;  // ... whose camera gives z_view = key * scale + offset
    DevBuf index, key;                 // int32 [H][W]: the surface's upload row (-1: none) and depth key
    DevBuf total;                      // u32 [H][W], when asked for
    DevBuf moment;                     // i64 [H][W], when asked for
    DevBuf labels;                     // int32 [n]: the upload's exact labels by upload row (gsx_depth_pick)
    bool labels_ready = false;         // ... filled since the last upload
    unsigned long long surfaces = 0;   // pixels of the last view with a surface
};

// State of an association run (assoc.hip): gsx_assoc_begin .. the next gsx_upload_positions
struct AssocState {
    bool begun = false;
    int max_segments = 0, max_instances = 0;  // S, M: the view's table is (S + 1) x (M + 1)
    unsigned long long q = 0;          // ceil(min_overlap * 2^20)
    long long min_size = 1;
    int views = 0, instances = 0;      // views associated; G, the global instances so far
    long long dropped = 0;             // segments that found no instance with G == M
    DevBuf gid;                        // int32 [n], Morton order: the instance a Gaussian was first given, -1 = none yet
    DevBuf bins;                       // u8 [n], Morton order: the view's bin (segment + 1) under the Gaussian, 255 = invisible
    DevBuf table;                      // u32 [(S + 1) (M + 1)], then u32: the lowest flat map index out of range (~0: none)
    DevBuf remap, view, raw, ids;      // int32 [S]; the ViewDesc; a host map on its way to the kernels; int32 [n] upload order
    PinBuf up;                         // pinned, host -> device: ViewDesc (256 B) | remap int32 [S] (1024 B) | the raw host map
    PinBuf down;                       // pinned, device -> host: the table and the range word behind it
    Event up_ev, down_ev;              // recorded behind the copies out of `up` / into `down`
    std::vector<uint32_t> last;        // the last view's table (gsx_assoc_table)
};

struct Ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    std::string err;

    // scene
    int64_t n = 0;
    DevBuf x, y, z;     // SoA f32 positions (Morton order when `sorted`)
    DevBuf perm;        // u32[n]: original index of slot i (valid when `sorted`)
    bool sorted = false;
    DevBuf sort_hist;   // radix-sort scratch

    // the vote (vote.hip, handover.hip): options, the run since vote_begin, the planes, the early stage, the host staging
    VoteOpts vopt;
    VoteRun run;
    HandOver ho;
    VotePlanes planes;
    hipStream_t stream2 = nullptr;  // the early vote's stream (vote.hip: second_stream); gsx_render_views borrows it
    bool stream_borrowed = false;   // (a twin of gsx_render_views) `stream` is the parent context's second stream: not this context's to destroy
    EarlyVote early;
    VoteStaging hstage;

    // rasterizer (render_scene.hip / render_pre.hip / render.hip / blend.hip)
    RenderScene scene;
    RenderOpts ropt;
    RenderFrame frame;
    LiftState lift;
    LabelMapState labelmap;
    DepthMapState depthmap;
    AssocState assoc;
    // gsx_render_views: further streams + per-frame buffers.  A twin is a whole Ctx because sort.hip, ProfScope and fail take
    // one; what it uses of it is stream, sort_hist, err, scene (aliases of this context's), ropt (a copy) and frame
    Ctx* twins[kMaxFrames - 1] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // ... with ONE pre pass per group of frames (pre_multi_kernel), issued by this context for all of them
    DevBuf r_pre_args;                   // pre_multi_kernel's per-view arguments, one slot per record set
    std::vector<unsigned long long> r_pre_args_host;  // ... and their host copies (8-byte aligned; alive while the H2D copies run)
    Event r_pre_ev[kPreSets];            // recorded behind the pre pass that filled set s

    // nearest-neighbour search (normals.hip)
    int opt_nn_brute = 0;                // 1: a 1 x 1 x 1 grid, i.e. every query visits every point (the search the grid is tested against)
    DevBuf nn_index;                     // int32[n][k]: the lists of the last gsx_knn
    int64_t nn_index_rows = 0;           // 0: none
    int nn_index_k = 0;                  // ... and their k
    DevBuf nn_pts, nn_cs;                // float4[n] (x, y, z, index) in cell order; u32[cells + 1]
    DevBuf nn_out, nn_flag;              // double normals[3n] | residuals[n] | moments[9n] (before the search: the raw points of the finite check); int

    // label filter (smooth.hip)
    int opt_smooth_search = 0;           // 1: the search form also for k <= 64 (the form the lists are tested against)
    DevBuf sm_lab[2];                    // the round's input and output: int32[n] labels (list form) or u16[n] class ids (search form)
    DevBuf sm_sup, sm_changed;           // int32[n] support; u64: labels the round changed
    DevBuf sm_lists;                     // int32[n][k]: lists handed over by the caller (gsx_smooth_labels_lists)

    // label split (split.hip): buffers only grow
    DevBuf sp_lab, sp_parent, sp_rep;    // int32[n]: the labels (in the end the instance ids); the union-find forest; rep, -1 = ignored
    DevBuf sp_size, sp_id, sp_kept;      // u32[n] points per root; int32[n] rep -> instance id, -1 = none; int32[M] the kept reps by rank
    DevBuf sp_trip, sp_cnt;              // int32[3][n] (rep, size, label) of the roots that reach min_size; u32[2]: triples, roots
    DevBuf sp_pts, sp_lists;             // float[n][3] in the caller's order (finite max_dist only); int32[n][k] lists handed over by the caller

    // IoU evaluation (iou.hip): buffers only grow
    int opt_iou_table_lds = 1;           // label-map tables of up to 40000 entries are counted in LDS per workgroup (0: on the global table)
    DevBuf iou_planes;                   // u64 [masks + ground truths][ceil(h w / 64)]: the bit planes
    DevBuf iou_cnt;                      // u64: areas of the masks, of the ground truths, then inter[m][g]
    DevBuf iou_ptrs;                     // the device copy of a call's pointer arrays
    DevBuf iou_table;                    // u64 [pair][P + 1][G + 1], then u32 [pair]: lowest flat index out of range
    DevBuf iou_top;                      // int32 [h w]
    DevBuf iou_raw[2];                   // host inputs: the two raw masks (or pairs of label maps) in flight ...
    PinBuf iou_pin[2];                   // ... and the pinned staging pair they come through
    Event iou_ev[2];                     // recorded behind a slot's H2D copy
    int iou_slot = 0;

    // class maps from network outputs (segmap.hip)
    DevBuf seg_low;                      // int32 [n][h w]: the maps at the network's resolution, between the two kernels of a call
    // Mask2Former queries (queries.hip): everything between the kernels of one call
    DevBuf q_bits;                       // u64 [K][mid_h][ceil(mid_w / 64)]: the slot-major bit planes of "v > 0"
    DevBuf q_parts;                      // QPart [K][workgroups per slot]: sigmoid sum, set count, sampled count, NaN flag
    DevBuf q_tab;                        // int32 [2][K]: segment id and map value per slot, then the u64 words of the sampled columns and rows

    // profiling
    bool prof_on = false;
    std::vector<std::string> prof_names;
    std::vector<ProfEvent> prof_events;
    std::vector<hipEvent_t> event_pool;
    std::map<std::string, std::pair<int64_t, double>> prof_acc;
};

// RAII: brackets one kernel launch with events when profiling is on
struct ProfScope {
    Ctx* c;
    ProfEvent ev{};
    bool active = false;
    hipStream_t st = nullptr;
    ProfScope(Ctx* ctx, const char* name, hipStream_t on = nullptr);  // on: the stream the kernel is launched on (default: ctx->stream)
    ~ProfScope();
};

// vote.hip
int vote_begin(Ctx* c, int n_classes, int first_view, int total_views);
int vote_view(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, int seg_w, int seg_h, int img_w, int img_h);
int early_pool_moves(Ctx* c);    // the seg pool is about to be re-allocated: wait for the early vote that reads it, drop its result
void vote_release_host(Ctx* c);  // the second stream (gsx_destroy)
int vote_slab_labels(Ctx* c, int slab, int slabs, int64_t* slab_size);
// handover.hip: segmentation maps into the seg pool, descriptors between ranks
int vote_view_host(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, int seg_w, int seg_h, int img_w, int img_h);
int vote_views_device(Ctx* c, int n, const gsx_camera* cams, const void* const* segs, int seg_dtype, int seg_w, int seg_h,
                      int img_w, int img_h);
int vote_export(Ctx* c, int64_t reserve_bytes, void* blobs_out, void** pool_dev, int64_t* pool_bytes);
int vote_import(Ctx* c, int n_parts, const int32_t* part_views, const int64_t* part_offsets, const void* blobs,
                const void* pool_all_dev, int64_t pool_all_bytes);
int vote_import_uniform(Ctx* c, int n_parts, const int32_t* part_views, const int64_t* part_offsets, const gsx_camera* cams,
                        int seg_w, int seg_h, int img_w, int img_h, const void* pool_all_dev, int64_t pool_all_bytes);
int vote_import_undo(Ctx* c);
int vote_map_stride(Ctx* c, int seg_w, int seg_h, int64_t* stride);
int vote_views_match_uniform(Ctx* c, int n, const gsx_camera* cams, int seg_w, int seg_h, int img_w, int img_h, int32_t* match);
Workers* host_workers(Ctx* c, const void* near = nullptr);  // the context's pool, created at first use (nullptr: pack on the caller)
int host_threads(Ctx* c);
int vote_flush_pending(Ctx* c);  // queue the DMA of packed host maps that are still waiting for their group to fill
void segpack_constants(int32_t out[8]);
int debug_host_pack(const void* seg, int seg_dtype, int w, int h, int n_classes, int tiled, int coarse, int threads,
                    uint8_t* out, int64_t out_cap, int64_t* bytes, int64_t* coarse_off, int32_t* bad);
int debug_host_pack_compact(const void* seg, int seg_dtype, int w, int h, int n_classes, int threads, uint8_t* out, int64_t out_cap,
                            int64_t* bytes, int64_t* table_bytes, int64_t* stream_off, int32_t* bad);
// vote.hip
int vote_rewind(Ctx* c);
int vote_finalize(Ctx* c, int32_t* labels_out);
int vote_flush(Ctx* c);
int vote_tiebreak_keys(Ctx* c);
int vote_labels_from_keys(Ctx* c, int32_t* labels_out);
int vote_debug_planes(Ctx* c, uint16_t* counts_out, uint16_t* first_out);
int vote_slab_reduce(Ctx* c, const void* recv_cnt, const void* recv_fv);
int vote_flush_counts(Ctx* c);
int vote_slab_totals(Ctx* c, const void* recv_cnt);
int vote_tie_codes(Ctx* c, const void* cand_all);
int vote_tie_resolve(Ctx* c, const void* recv_codes);
int vote_labels_from_sorted(Ctx* c, const void* sorted_labels_dev, int32_t* labels_out);
int project_all(Ctx* c, const gsx_camera* cam, const float* dx, const float* dy, const float* dz, int64_t n,
                int32_t* x_host, int32_t* y_host, const uint32_t* perm);
// sort.hip
int radix_sort_pairs(Ctx* c, uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, long long n, int bits,
                     int* result_in);
int radix_sort_pairs_dev(Ctx* c, uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, long long n,
                         const unsigned long long* n_dev, int bits, int* result_in);
int radix_sort_pairs_drop(Ctx* c, uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, long long n,
                          const unsigned long long* n_dev, int bits, int* result_in, unsigned long long* n_kept);  // elements with key 0xffffffff are left out
int radix_sort_values_wide(Ctx* c, const uint32_t* k0, const uint32_t* v0, uint32_t* v1, long long n, const unsigned long long* n_dev,
                           int bits, int2* ranges, int nranges);  // one pass over <= 11 key bits; ranges[d] = slots of key d
int spatial_sort_positions(Ctx* c);
int vote_culled(Ctx* c, int64_t* out, bool reset);
int second_stream(Ctx* c);
int filter_check(Ctx* c, double* out);
int kmeans(Ctx* c, int64_t n, const float* points, const float* colors, int k, const int64_t* init_index, int max_iter,
           double tol, int32_t* labels_out, float* centroids_out, int32_t* iterations_out, int32_t* converged_out);
void debug_cull_planes(const gsx_camera* cam, double* out);
// normals.hip
int normals(Ctx* c, int64_t n, const float* points, int64_t k, double* normals_out, double* residuals_out, double* moments_out = nullptr,
            bool checked = false);
int knn(Ctx* c, int64_t n, const float* points, int k, int32_t* index_out, bool checked = false);
int knn_lists(Ctx* c, const char* who, int64_t n, const float* points, int k, int32_t* index_out, bool checked);  // knn without its argument checks, k >= 1
int debug_nn_grid(int64_t n, const float* points, int64_t k, int brute, double* origin_out, double* h_out, int32_t* dims_out,
                  uint32_t* cell_start_out, int32_t* order_out);  // test hook: the grid and the counting sort, host only
int region_growing(Ctx* c, int64_t n, const float* points, int64_t k_normals, int k, double residual_threshold, double angle_threshold,
                   int32_t* labels_out, double* normals_out, double* residuals_out, int32_t* n_regions_out);
// smooth.hip: the k-nearest-neighbour majority filter over a label field
struct SmoothArgs {
    int32_t rounds, min_votes, ignore_label, flags;
    int32_t *labels_out, *support_out;
    int64_t* changed_out;
    int32_t* rounds_done_out;
};
int smooth_labels(Ctx* c, int64_t n, const float* points, const int32_t* labels, int64_t k, const SmoothArgs& a);
int smooth_labels_lists(Ctx* c, int64_t n, int32_t k, const int32_t* knn, const int32_t* labels, const SmoothArgs& a);
void smooth_constants(int32_t out[8]);
// split.hip: connected components of every label over the k-nearest-neighbour graph
struct SplitArgs {
    double max_dist;
    int64_t min_size;
    int32_t max_instances, ignore_label, flags;
    int32_t *labels_out, *component_out, *instance_label_out;
    int64_t* instance_size_out;
    int32_t *instance_rep_out, *n_instances_out;
    int64_t* n_components_out;
};
int split_labels(Ctx* c, int64_t n, const float* points, const int32_t* labels, int32_t k, const SplitArgs& a);
int split_labels_lists(Ctx* c, int64_t n, int32_t k, const int32_t* knn, const float* points, const int32_t* labels, const SplitArgs& a);
// render_scene.hip: what exists once per scene
int upload_splats(Ctx* c, int64_t n, const float* xyz, const float* scale, const float* rot, const float* opacity,
                  const float* f_dc, const int32_t* labels);
int upload_sh(Ctx* c, const float* f_rest, int deg);
int render_set_edits(Ctx* c, const gsx_render_edits* edits);
int hit_test(Ctx* c, const gsx_camera* cam, int W, int H, double x, double y, int32_t* label_out, int64_t* index_out);
int render_debug(Ctx* c, uint8_t* buffer_out, uint32_t* order_out, uint32_t* tex_out, uint32_t* bucket_out);
int debug_render_scene(Ctx* c, int32_t* labels_out, float* sh_out, int32_t* sh_degree_out);
// render_pre.hip: the per-view per-splat pass.  ONE place for its launches (gsx_render_view, gsx_render_views and the test hook
// gsx_debug_render_pre), so that what the hook observes is the product's launch (grid cap, arguments, initial pre[])
int ensure_pre_set(Ctx* c, PreSet& ps, long long n);
int launch_pre(Ctx* c, const gsx_camera* cam, int W, int H, const PreSet& to);  // one view: pre[] reset, then pre_kernel
int launch_pre_multi(Ctx* c, int nv, const gsx_camera* cams, int W, int H, PreSet* const* sets, int slot);  // view v into *sets[v]; arguments in slot `slot`
void launch_bucket(Ctx* c, const PreSet& ps, uint32_t* bucket, uint32_t* key, uint32_t* idx, int* dropped, int compact);
int debug_render_pre(Ctx* c, int nv, const gsx_camera* cams, int W, int H, int multi, int compact, const gsx_debug_pre_view* out);
// render.hip: the frame
int render_view(Ctx* c, const gsx_camera* cam, int W, int H, float* rgba_out);
int render_views(Ctx* c, int n, const gsx_camera* cams, int W, int H, float* const* rgba_out);
void render_release_twin(Ctx* c);
// the frame's shared front: geometry + buffers; then per attempt the pre pass, buckets and level-1 sort; then per depth phase
// bin COUNT -> scan -> EMIT, the pair sort and the ranges (*vals_sorted: the list entries the ranges index)
int frame_plan(Ctx* c, int W, int H, bool allow_bin32, int phases, FramePlan& fp);
int frame_depth_order(Ctx* c, const gsx_camera* cam, FramePlan& fp);
int frame_phase_lists(Ctx* c, const FramePlan& fp, int p, int first_phase, const uint32_t** vals_sorted);
// a walked frame (lift_view, label_view, depth_view): the frame-state and size checks; plan + lists of one depth phase, rebuilt
// until they fit the pair buffers (nothing walked yet); the kernel's statistics, queued without a wait, summed after the caller's
int frame_walk_guard(Ctx* c, const gsx_camera* cam, int W, int H, const char* who, const char* what);
int frame_lists_that_fit(Ctx* c, const gsx_camera* cam, int W, int H, const char* who, FramePlan& fp, const uint32_t** vals);
int frame_walk_stats_queue(Ctx* c, FrameCounters& stats);
void frame_walk_stats_sum(Ctx* c, const FrameCounters& stats, unsigned long long* atomics, unsigned long long* single);  // -> c->frame.consumed too
int debug_exclusive_scan(Ctx* c, const uint32_t* in, uint32_t* out, long long n, unsigned long long* grand_dev);  // test hook: exclusive_scan_u32
int debug_ranges(Ctx* c, const uint32_t* keys, const unsigned long long* total_dev, long long cap, int nlists, int2* ranges);  // test hook: ranges_kernel as a frame launches it
// bin_kernel COUNT -> exclusive_scan_u32 -> bin_kernel EMIT of one depth phase (device pointers): what render_view launches per
// phase and, through the test hook debug_bin, gsx_debug_bin in the caller's buffers
struct BinPhaseArgs {
    const unsigned long long* nvis_dev;
    long long div0, div1, m_cap;
    const uint32_t* by_depth;
    const uint32_t* tile_rect;
    const float4* rec;
    int H, tiles_x, bin32, exact;
    const uint8_t* sat;
    uint32_t *count, *offset, *rect_seq, *keys, *vals;
    unsigned long long* total_dev;
    unsigned long long pair_cap;
};
int debug_bin(Ctx* c, const BinPhaseArgs& a);
// blend.hip
int launch_blend(Ctx* c, const uint32_t* vals, int W, int H, int tiles_x, int tiles_y, const int* dropped_dev,
                 unsigned long long* consumed_dev, uint8_t* sat, int first_phase, int last_phase);
// lift.hip: per-splat, per-class blend weights of class maps, and their arg-max
int lift_begin(Ctx* c, int n_classes);
int lift_view(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, int W, int H, bool device);
int lift_finalize(Ctx* c, double min_weight, int32_t* labels_out, double* share_out);
int lift_table(Ctx* c, uint64_t* table_out);
void lift_end(Ctx* c);             // a new upload ends the run
void lift_constants(int32_t out[8]);
unsigned long long lift_threshold(double min_weight);  // ceil(min_weight * 2^20), saturating at 2^64 - 1
// labelmap.hip: the splats' labels as the class map of a view (the transpose of the lift)
struct LabelViewArgs {
    int32_t n_classes;
    double min_weight;
    int32_t n_planes;
    const int32_t* plane_labels;
    int32_t* label_out;
    uint32_t *weight_out, *total_out, *planes_out;
};
int label_view(Ctx* c, const gsx_camera* cam, int W, int H, const LabelViewArgs& a);
void label_new_upload(Ctx* c, bool has_labels);  // a new upload: the checked one-byte labels go away with the old splats
void labelmap_constants(int32_t out[8]);
// depthmap.hip: per-pixel depth sums, the surface splat and the pick on it
struct DepthViewArgs {
    double quantile;
    uint32_t* total_out;
    int64_t* moment_out;
    int32_t *key_out, *index_out;
};
int depth_view(Ctx* c, const gsx_camera* cam, int W, int H, const DepthViewArgs& a);
int depth_pick(Ctx* c, double x, double y, int32_t* label_out, int64_t* index_out, double* z_out);
int depth_key_to_z(const gsx_camera* cam, int W, int H, double* scale, double* offset);  // host only
void depth_new_upload(Ctx* c);     // a new upload invalidates the last view
void depth_constants(int32_t out[8]);
// assoc.hip: per-view segment ids -> global instance ids through the Gaussians
int assoc_begin(Ctx* c, int max_segments, int max_instances, double min_overlap, int min_size);
int assoc_view(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, int seg_w, int seg_h, int img_w, int img_h,
               int32_t* remap_out, void* map_out_dev, bool device);
int assoc_ids(Ctx* c, int32_t* gid_out);
int assoc_table(Ctx* c, uint32_t* table_out);
void assoc_end(Ctx* c);            // a new upload ends the run
void assoc_constants(int32_t out[8]);
// iou.hip
int iou_masks(Ctx* c, bool device, int n_masks, const void* const* masks, int mask_dtype, int n_gt, const void* const* gts, int gt_dtype,
              int h, int w, int64_t* inter_out, int64_t* area_masks_out, int64_t* area_gt_out, double* iou_out);
int iou_label_maps(Ctx* c, bool device, int n_pairs, const void* const* pred, int pred_dtype, int n_pred_classes, const void* const* gt,
                   int gt_dtype, int n_gt_classes, int h, int w, int64_t* table_out);
int masks_top_index(Ctx* c, int n_masks, const void* const* masks, int mask_dtype, int h, int w, int32_t* index_out);
void iou_constants(int32_t out[8]);
// segmap.hip
int segmap_from_logits(Ctx* c, const void* logits, int dtype, int n, int C, int h, int w, int out_w, int out_h, int32_t* maps);
int segmap_from_masks(Ctx* c, const void* masks, int dtype, int K, int mh, int mw, const float* cls, const float* conf, int out_w, int out_h,
                      int32_t* map);
void segmap_constants(int32_t out[8]);
int seg_elem_bytes(int dtype);                    // 0: not a gsx_float_dtype
bool seg_misaligned(const void* p, int bytes);
// seg_low (n, h, w) -> out (n, H, W) on the ctx stream; torch_rule: torch's float32 nearest rule instead of OpenCV's
int seg_launch_resize(Ctx* c, int n, int w, int h, int W, int H, int32_t* out, bool torch_rule = false);
// queries.hip
int segmap_from_queries(Ctx* c, const void* masks, int dtype, int Q, int h, int w, int K, const int32_t* slot_query, const float* slot_score,
                        const int32_t* slot_label, int mid_w, int mid_h, double threshold, int mode, int out_w, int out_h, int32_t* map,
                        int32_t* slot_segment, float* slot_pred_score);
void queries_constants(int32_t out[8]);
// vote.hip
void fill_view_desc(ViewDesc& vd, const gsx_camera* cam, int seg_w, int seg_h, int img_w, int img_h);

}  // namespace gsx
