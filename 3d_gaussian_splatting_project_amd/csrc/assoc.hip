// Instance association: a Mask2Former map numbers its segments per image, so segment 3 of one view and segment 7 of the next may
// be the same chair.  A run makes the ids mean the same object in every view, view by view, through the Gaussians: each
// Gaussian remembers the global instance it was first given, and a view's segment takes the instance most of its Gaussians
// already carry, or opens a new one (include/gsx.h has the rule; tests/assoc_model.py is its numpy statement).  Every number
// is an integer: the table is exact whatever order the atomics arrive in, and the decision runs on the host over the table.
// The sample is the vote's: project() of vote_device.hpp, then the scale, truncation and clamp of seg_bin_regs().
#include <algorithm>
#include <cmath>
#include <cstring>

#include "seg_dtype.hpp"
#include "vote_device.hpp"

namespace gsx {

// ---- the units (gsx_debug_assoc_constants hands them to the tests) ------------------------------------------------------------------
static constexpr int kAssocShift = 20;                    // min_overlap is compared in units of 2^-20
static constexpr int kAssocOne = 1 << kAssocShift;
static constexpr int kAssocBlock = kBlock;                // threads per workgroup of the assign, relabel and ids kernels
static constexpr int kAssocMaxSegments = 254;             // a bin (segment + 1) is a byte and 255 stands for "invisible"
static constexpr int kAssocMaxInstances = 255;            // the relabelled maps are class maps of the vote: n_classes <= 255
static constexpr int kAssocTableBlock = 1024;             // Gaussians per step of a workgroup of the table kernel: a CU holds one or two
                                                          // copies of the table, and each has to feed 16 waves
static constexpr int kAssocMaxChunks = 63;                // steps per workgroup: 63 * 1024 < 2^16 Gaussians keep its 16-bit counters exact
static constexpr int kAssocLdsEntries = (kAssocMaxSegments + 1) * (kAssocMaxInstances + 1);  // 65 280 counters = 130 560 B of the 160 KB
static constexpr int kAssocRun = 4;                       // consecutive pixels per thread of the relabel kernel
static constexpr unsigned kAssocNoBad = 0xffffffffu;
static constexpr size_t kAssocUpView = 0, kAssocUpRemap = 256, kAssocUpMap = 256 + 1024;  // byte offsets inside AssocState::up

// iou.hip's iou_table_add with a count of one, onto 16-bit counters packed in pairs: the lanes that hold the first active lane's
// key add once, with the popcount of their ballot; two rounds (in Morton order most waves hold one or two keys), then whoever
// is left adds on its own.  No half can carry into the other: a workgroup sees fewer than 2^16 Gaussians.
// (Kept apart from iou_table_add on purpose: counter width, packing and LDS-only against LDS-or-global differ.)
__device__ __forceinline__ void assoc_lds_add(unsigned* ltab, unsigned key, unsigned count) { atomicAdd(&ltab[key >> 1], count << (16 * (key & 1u))); }
__device__ __forceinline__ void assoc_table_add(bool act, unsigned key, int lane, unsigned* ltab) {
    unsigned long long pend = __ballot(act);
#pragma unroll 1
    for (int r = 0; r < 2 && pend; ++r) {
        const int first = __ffsll((long long)pend) - 1;
        const unsigned k0 = (unsigned)__shfl((int)key, first, 64);
        const unsigned long long same = __ballot(act && key == k0);
        if (lane == first) assoc_lds_add(ltab, k0, (unsigned)__popcll(same));
        if (key == k0) act = false;
        pend &= ~same;
    }
    if (act) assoc_lds_add(ltab, key, 1u);
}

// One thread per Gaussian and step, in the context's order (Morton order after a sorted upload; gid and bins are kept in it).
// bins[i] = the bin under Gaussian i's projection, 255 where the view does not see it; table[bin][gid[i] + 1] += 1.
// A workgroup owns `chunks` consecutive steps of 1024 Gaussians and counts into a copy of the table's live part in LDS: rows of
// G1 = G + 1 columns (no Gaussian carries an instance this view has yet to open), 16-bit counters, so that even 255 x 256 of
// them fit.  At the end it adds its non-zero counters onto the global u32 table, one atomic each; a compact piece of the Morton
// curve sees few segments, so few leave the workgroup.  (Every add straight onto the global table, one workgroup per 256
// Gaussians, was measured at 5.8 times this kernel's time: DESIGN.md.)
// Every thread then looks at its share of the map's pixels: the lowest flat index whose value is outside [-1, S - 1] goes into
// *err by atomicMin (the call then fails and nothing is kept).  A Gaussian over such a pixel counts as invisible.
template <int DT>
__global__ __launch_bounds__(kAssocTableBlock) void assoc_table_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                       const float* __restrict__ z, long long n, int chunks,
                                                                       const ViewDesc* __restrict__ vp, const void* __restrict__ seg,
                                                                       long long npix, int S, int M1, int G1, const int* __restrict__ gid,
                                                                       uint8_t* __restrict__ bins, unsigned* __restrict__ table,
                                                                       unsigned* __restrict__ err) {
    constexpr int B = kAssocTableBlock;
    extern __shared__ unsigned assoc_ltab[];
    const int t = threadIdx.x, lane = t & 63;
    const int lentries = (S + 1) * G1, lwords = (lentries + 1) >> 1;
    for (int w = t; w < lwords; w += B) assoc_ltab[w] = 0;
    __syncthreads();
    const ViewRegs vr = load_view(vp);
    for (int k = 0; k < chunks; ++k) {  // (no early exit of a lane: the projection and the table add ballot over the whole wave)
        const long long i = ((long long)blockIdx.x * chunks + k) * B + t;
        const bool valid = i < n;
        const double X = valid ? (double)x[i] : __builtin_nan(""), Y = valid ? (double)y[i] : 0.0, Z = valid ? (double)z[i] : 0.0;
        int xi, yi;
        const bool vis = project<kDivFlat>(vr, X, Y, Z, xi, yi) && valid;
        bool act = false;
        unsigned key = 0, b8 = 255;
        if (vis) {
            if (!vr.unit_scale) {
                const double xs = trunc((double)xi * vp->wscale);  // dls.py:281
                const double ys = trunc((double)yi * vp->hscale);  // :282
                const int seg_h = vp->seg_h;
                xi = xs > (double)(vr.seg_w - 1) ? vr.seg_w - 1 : (int)xs;  // :285 (xs >= 0 always)
                yi = ys > (double)(seg_h - 1) ? seg_h - 1 : (int)ys;        // :286
            }
            const unsigned long long b = seg_bin<DT>(seg, (long long)yi * vr.seg_w + xi);
            if (b <= (unsigned long long)S) {
                b8 = (unsigned)b;
                key = (unsigned)b * (unsigned)G1 + (unsigned)(gid[i] + 1);
                act = true;
            }
        }
        if (valid) bins[i] = (uint8_t)b8;
        assoc_table_add(act, key, lane, assoc_ltab);
    }
    unsigned bad = kAssocNoBad;
    const long long stride = (long long)gridDim.x * B;
    for (long long p = (long long)blockIdx.x * B + t; p < npix; p += stride)
        if (seg_bin<DT>(seg, p) > (unsigned long long)S) bad = min(bad, (unsigned)p);
    if (bad != kAssocNoBad) atomicMin(err, bad);
    __syncthreads();
    for (int w = t; w < lwords; w += B) {
        const unsigned v = assoc_ltab[w];
        if (!v) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned cnt = (v >> (16 * h)) & 0xffffu;
            const int e = 2 * w + h;  // (the odd half past the last entry is never written)
            if (cnt) atomicAdd(&table[(e / G1) * M1 + e % G1], cnt);
        }
    }
}

// rule 4: a visible Gaussian without an instance takes its segment's; the first assignment stays
__global__ __launch_bounds__(kAssocBlock) void assoc_assign_kernel(const uint8_t* __restrict__ bins, const int* __restrict__ remap,
                                                                   long long n, int* __restrict__ gid) {
    const long long i = (long long)blockIdx.x * kAssocBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned b = bins[i];
    if (b == 0 || b == 255u) return;
    const int g = remap[b - 1];
    if (g >= 0 && gid[i] < 0) gid[i] = g;
}

// rule 5: out[p] = map[p] >= 0 ? remap[map[p]] : -1, four pixels per thread; the remap sits in LDS as a table over the bins
template <int DT>
__global__ __launch_bounds__(kAssocBlock) void assoc_relabel_kernel(const void* __restrict__ seg, long long npix, int S,
                                                                    const int* __restrict__ remap, int* __restrict__ out) {
    __shared__ int s_remap[kAssocBlock];
    const int t = threadIdx.x;
    s_remap[t] = t >= 1 && t <= S ? remap[t - 1] : -1;
    __syncthreads();
    const long long i0 = ((long long)blockIdx.x * kAssocBlock + t) * kAssocRun;
    if (i0 >= npix) return;
    unsigned long long b[4];
    seg_bins4<DT>(seg, i0, npix, b);
    int r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = b[j] <= (unsigned long long)S ? s_remap[(int)b[j]] : -1;
    if ((reinterpret_cast<uintptr_t>(out) & 15) == 0 && i0 + 4 <= npix) {
        *reinterpret_cast<int4*>(out + i0) = make_int4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < npix) out[i0 + j] = r[j];
    }
}

// gid in the context's order -> the caller's order
__global__ __launch_bounds__(kAssocBlock) void assoc_ids_kernel(const int* __restrict__ gid, const uint32_t* __restrict__ perm, long long n,
                                                                int* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kAssocBlock + threadIdx.x;
    if (i >= n) return;
    out[perm ? (long long)perm[i] : i] = gid[i];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// With profiling on, the host's own shares of a view are accumulated next to the kernels' (gsx_profile_get): wall time since t0
static void assoc_host_ms(Ctx* c, const char* name, std::chrono::steady_clock::time_point t0) {
    if (!c->prof_on) return;
    if (std::find(c->prof_names.begin(), c->prof_names.end(), name) == c->prof_names.end()) c->prof_names.emplace_back(name);
    auto& acc = c->prof_acc[name];
    acc.first += 1;
    acc.second += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void assoc_end(Ctx* c) {
    AssocState& A = c->assoc;
    A.begun = false;
    A.views = A.instances = 0;
    A.dropped = 0;
    A.last.clear();
}

int assoc_begin(Ctx* c, int max_segments, int max_instances, double min_overlap, int min_size) {
    GSX_HIP(c, hipSetDevice(c->device));
    if (max_segments < 1 || max_segments > kAssocMaxSegments)
        return fail(c, GSX_E_INVALID, "assoc_begin: max_segments = %d must be in [1, %d]", max_segments, kAssocMaxSegments);
    if (max_instances < 1 || max_instances > kAssocMaxInstances)
        return fail(c, GSX_E_INVALID, "assoc_begin: max_instances = %d must be in [1, %d]", max_instances, kAssocMaxInstances);
    if (!(min_overlap >= 0.0) || !(min_overlap <= 1.0)) return fail(c, GSX_E_INVALID, "assoc_begin: min_overlap must lie in [0, 1]");
    if (min_size < 1) return fail(c, GSX_E_INVALID, "assoc_begin: min_size = %d must be at least 1", min_size);
    if (c->n <= 0) return fail(c, GSX_E_STATE, "assoc_begin: no positions uploaded (gsx_upload_positions)");
    AssocState& A = c->assoc;
    assoc_end(c);
    const size_t n = (size_t)c->n, entries = (size_t)(max_segments + 1) * (size_t)(max_instances + 1);
    GSX_HIP(c, A.gid.ensure(n * sizeof(int)));
    GSX_HIP(c, A.bins.ensure(n));
    GSX_HIP(c, A.table.ensure((entries + 1) * sizeof(unsigned)));
    GSX_HIP(c, A.remap.ensure(kAssocMaxSegments * sizeof(int)));
    GSX_HIP(c, A.view.ensure(sizeof(ViewDesc)));
    GSX_HIP(c, A.up_ev.wait());
    GSX_HIP(c, A.up.ensure(kAssocUpMap));
    GSX_HIP(c, A.down_ev.wait());
    GSX_HIP(c, A.down.ensure((entries + 1) * sizeof(unsigned)));
    GSX_HIP(c, hipMemsetAsync(A.gid.p, 0xff, n * sizeof(int), c->stream));  // -1: no instance yet
    A.max_segments = max_segments;
    A.max_instances = max_instances;
    A.q = (unsigned long long)std::ceil(min_overlap * (double)kAssocOne);
    A.min_size = min_size;
    A.last.assign(entries, 0u);
    A.begun = true;
    return GSX_OK;
}

// Rule 3 on the host, over the view's table: remap[S], and the run's G and dropped counter move on
static void assoc_decide(AssocState& A, const uint32_t* table, int32_t* remap) {
    const int S = A.max_segments, M = A.max_instances, M1 = M + 1;
    std::vector<unsigned long long> size((size_t)S + 1, 0);
    std::vector<int> rows;
    for (int b = 1; b <= S; ++b) {
        for (int k = 0; k < M1; ++k) size[b] += table[(size_t)b * M1 + k];
        remap[b - 1] = -1;
        if (size[b] >= (unsigned long long)A.min_size) rows.push_back(b);  // min_size >= 1: an empty row stays -1
    }
    std::stable_sort(rows.begin(), rows.end(), [&](int a, int b) { return size[a] > size[b]; });  // of equal sizes the lower b first
    std::vector<char> taken((size_t)M, 0);
    for (const int b : rows) {
        const uint32_t* row = table + (size_t)b * M1;
        unsigned long long best = 0;
        int g = -1;
        for (int k = 0; k < A.instances; ++k)
            if (!taken[k] && row[k + 1] > best) best = row[k + 1], g = k;  // the largest count, the lowest g of equal counts
        if (g >= 0 && (best << kAssocShift) >= A.q * size[b]) {
            remap[b - 1] = g;
            taken[g] = 1;
        } else if (A.instances < M) {
            remap[b - 1] = A.instances;
            taken[A.instances++] = 1;
        } else {
            ++A.dropped;
        }
    }
}

// The table kernel of one view.  The LDS copy holds (S + 1) x (G + 1) 16-bit counters, G = the instances before this view; one
// or two workgroups per CU, as that allows, each on a contiguous piece of the Morton curve of fewer than 2^16 Gaussians.
template <int DT>
static int assoc_launch(Ctx* c, const void* seg_dev, long long npix) {
    AssocState& A = c->assoc;
    const int S = A.max_segments, M1 = A.max_instances + 1, G1 = A.instances + 1;
    const size_t entries = (size_t)(S + 1) * (size_t)M1, lentries = (size_t)(S + 1) * (size_t)G1;
    const size_t lds_bytes = (lentries + 1) / 2 * sizeof(unsigned);
    unsigned* table = A.table.as<unsigned>();
    if (lds_bytes > 64 * 1024)
        GSX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(assoc_table_kernel<DT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds_bytes));
    const long long nchunks = (c->n + kAssocTableBlock - 1) / kAssocTableBlock;
    long long wgs = std::min(nchunks, 256ll * (lds_bytes * 2 <= 160 * 1024 ? 2 : 1));
    wgs = std::max(wgs, (nchunks + kAssocMaxChunks - 1) / kAssocMaxChunks);
    const int chunks = (int)((nchunks + wgs - 1) / wgs);
    ProfScope ps(c, "assoc_table");
    hipLaunchKernelGGL((assoc_table_kernel<DT>), dim3((unsigned)((nchunks + chunks - 1) / chunks)), dim3(kAssocTableBlock), lds_bytes, c->stream,
                       c->x.as<float>(), c->y.as<float>(), c->z.as<float>(), (long long)c->n, chunks, A.view.as<ViewDesc>(), seg_dev, npix, S,
                       M1, G1, A.gid.as<int>(), A.bins.as<uint8_t>(), table, table + entries);
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

template <int DT>
static void assoc_launch_relabel(Ctx* c, const void* seg_dev, long long npix, int* out) {
    AssocState& A = c->assoc;
    const long long threads = (npix + kAssocRun - 1) / kAssocRun;
    ProfScope ps(c, "assoc_relabel");
    hipLaunchKernelGGL((assoc_relabel_kernel<DT>), dim3(grid_for(threads)), dim3(kAssocBlock), 0, c->stream, seg_dev, npix, A.max_segments,
                       A.remap.as<int>(), out);
}

int assoc_view(Ctx* c, const gsx_camera* cam, const void* seg, int seg_dtype, int seg_w, int seg_h, int img_w, int img_h,
               int32_t* remap_out, void* map_out_dev, bool device) {
    GSX_HIP(c, hipSetDevice(c->device));
    AssocState& A = c->assoc;
    const char* who = device ? "assoc_view_device" : "assoc_view";
    if (!A.begun) return fail(c, GSX_E_STATE, "%s: call gsx_assoc_begin first", who);
    if (!cam || !seg) return fail(c, GSX_E_INVALID, "%s: NULL argument", who);
    if (seg_w < 1 || seg_h < 1 || img_w < 1 || img_h < 1 || seg_w > 65535 || seg_h > 65535)
        return fail(c, GSX_E_INVALID, "%s: map %d x %d, image %d x %d: sizes must be positive and a map at most 65535 a side", who, seg_w,
                    seg_h, img_w, img_h);
    if (!seg_dtype_known(seg_dtype)) return fail(c, GSX_E_INVALID, "%s: unknown seg_dtype %d", who, seg_dtype);
    const size_t elem = seg_elem_size(seg_dtype);
    if (seg_misaligned(seg, (int)elem)) return fail(c, GSX_E_INVALID, "%s: the map is not aligned to its element", who);
    if (reinterpret_cast<uintptr_t>(map_out_dev) & 3u) return fail(c, GSX_E_INVALID, "%s: map_out_dev is not aligned to int32", who);
    const long long npix = (long long)seg_w * seg_h;
    if (npix >= (1ll << 31)) return fail(c, GSX_E_UNSUPPORTED, "%s: %d x %d pixels: seg_w * seg_h must stay below 2^31", who, seg_w, seg_h);
    const int S = A.max_segments;
    const size_t entries = (size_t)(S + 1) * (size_t)(A.max_instances + 1), tbytes = (entries + 1) * sizeof(unsigned);
    const size_t map_bytes = device ? 0 : elem * (size_t)npix;
    const auto t_call = std::chrono::steady_clock::now();
    // the view's descriptor (and a host map behind it) go up through the pinned buffer
    GSX_HIP(c, A.up_ev.wait());
    GSX_HIP(c, A.up.ensure(kAssocUpMap + map_bytes));
    char* up = A.up.as<char>();
    ViewDesc vd;
    fill_view_desc(vd, cam, seg_w, seg_h, img_w, img_h);
    std::memcpy(up + kAssocUpView, &vd, sizeof vd);
    GSX_HIP(c, hipMemcpyAsync(A.view.p, up + kAssocUpView, sizeof vd, hipMemcpyHostToDevice, c->stream));
    const void* seg_dev = seg;
    if (!device) {
        GSX_HIP(c, A.raw.ensure(map_bytes));
        std::memcpy(up + kAssocUpMap, seg, map_bytes);
        GSX_HIP(c, hipMemcpyAsync(A.raw.p, up + kAssocUpMap, map_bytes, hipMemcpyHostToDevice, c->stream));
        seg_dev = A.raw.p;
    }
    GSX_HIP(c, hipMemsetAsync(A.table.p, 0, entries * sizeof(unsigned), c->stream));
    GSX_HIP(c, hipMemsetAsync(A.table.as<unsigned>() + entries, 0xff, sizeof(unsigned), c->stream));
    const int rc = with_seg_dtype(seg_dtype, [&](auto d) { return assoc_launch<decltype(d)::value>(c, seg_dev, npix); });
    if (rc) return rc;
    // the table comes back; the decision needs it, and so does the range check
    GSX_HIP(c, hipMemcpyAsync(A.down.p, A.table.p, tbytes, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, A.down_ev.record(c->stream));
    GSX_HIP(c, A.down_ev.wait());
    assoc_host_ms(c, "assoc_host_until_table", t_call);  // staging, the table kernel, the copy down and the wait
    const auto t_decide = std::chrono::steady_clock::now();
    const uint32_t* table = A.down.as<uint32_t>();
    const unsigned bad = table[entries];
    if (bad != kAssocNoBad)  // nothing of the run has changed: gid, G, the counters and the last table are the previous view's
        return fail(c, GSX_E_RANGE, "%s: view %d: the value at row %u, column %u is outside [-1, %d]", who, A.views, bad / (unsigned)seg_w,
                    bad % (unsigned)seg_w, S - 1);
    int32_t* remap = reinterpret_cast<int32_t*>(up + kAssocUpRemap);
    assoc_decide(A, table, remap);
    A.last.assign(table, table + entries);
    assoc_host_ms(c, "assoc_host_decide", t_decide);
    const auto t_tail = std::chrono::steady_clock::now();
    GSX_HIP(c, hipMemcpyAsync(A.remap.p, remap, (size_t)S * sizeof(int), hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, "assoc_assign");
        hipLaunchKernelGGL(assoc_assign_kernel, dim3(grid_for(c->n)), dim3(kAssocBlock), 0, c->stream, A.bins.as<uint8_t>(), A.remap.as<int>(),
                           (long long)c->n, A.gid.as<int>());
    }
    GSX_HIP(c, hipGetLastError());
    if (map_out_dev) {
        int* out = static_cast<int*>(map_out_dev);
        with_seg_dtype(seg_dtype, [&](auto d) { assoc_launch_relabel<decltype(d)::value>(c, seg_dev, npix, out); });
        GSX_HIP(c, hipGetLastError());
    }
    GSX_HIP(c, A.up_ev.record(c->stream));
    ++A.views;
    if (remap_out) std::memcpy(remap_out, remap, (size_t)S * sizeof(int));
    // the caller's map and map_out_dev belong to the caller again when the call returns
    GSX_HIP(c, A.up_ev.wait());
    assoc_host_ms(c, "assoc_host_after_decide", t_tail);  // the remap's way up, assign, relabel and the wait for them
    return GSX_OK;
}

int assoc_ids(Ctx* c, int32_t* gid_out) {
    GSX_HIP(c, hipSetDevice(c->device));
    AssocState& A = c->assoc;
    if (!A.begun) return fail(c, GSX_E_STATE, "assoc_ids: call gsx_assoc_begin first");
    if (!gid_out) return fail(c, GSX_E_INVALID, "assoc_ids: gid_out is NULL");
    const size_t bytes = (size_t)c->n * sizeof(int);
    GSX_HIP(c, A.ids.ensure(bytes));
    hipLaunchKernelGGL(assoc_ids_kernel, dim3(grid_for(c->n)), dim3(kAssocBlock), 0, c->stream, A.gid.as<int>(),
                       c->sorted ? c->perm.as<uint32_t>() : nullptr, (long long)c->n, A.ids.as<int>());
    GSX_HIP(c, hipGetLastError());
    GSX_HIP(c, hipMemcpyAsync(gid_out, A.ids.p, bytes, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

int assoc_table(Ctx* c, uint32_t* table_out) {
    AssocState& A = c->assoc;
    if (!A.begun) return fail(c, GSX_E_STATE, "assoc_table: call gsx_assoc_begin first");
    if (!table_out) return fail(c, GSX_E_INVALID, "assoc_table: table_out is NULL");
    std::memcpy(table_out, A.last.data(), A.last.size() * sizeof(uint32_t));
    return GSX_OK;
}

void assoc_constants(int32_t out[8]) {
    out[0] = kAssocOne;
    out[1] = kAssocShift;
    out[2] = kAssocTableBlock;
    out[3] = kAssocMaxSegments;
    out[4] = kAssocMaxInstances;
    out[5] = kAssocLdsEntries;
    out[6] = kAssocMaxChunks;
    out[7] = 0;
}

}  // namespace gsx
