// smooth.hip - label clean-up: a majority filter over the k nearest neighbours of every point, with hole filling
// (gsx_smooth_labels, gsx_smooth_labels_lists; include/gsx.h states the rule).  All integers: a round reads the labels L of
// its start and writes a second buffer (Jacobi), counts for every point i the labels of its neighbour set N(i), and takes
// the most frequent one - L[i] itself if it is among the most frequent, else the smallest value among them.
//
// N(i) is the set gsx_knn / gsx_normals select (nn_device.hpp): the k nearest by the key (bits of d2, index).  Two forms of a
// round, the same result bit for bit:
//   list form (k <= 64)   the lists int32[n][k] are on the device (built once by nn_knn_kernel, or handed over by the
//                         caller).  g = the power of two >= k lanes serve a query, 64 / g queries share a wave.  A lane
//                         gathers one neighbour's raw int32 label; the counts are taken in registers by k shuffles inside the
//                         group, so there is no class table and no limit on the distinct labels.  Rows are indexed in 64 bits.
//   search form (any k)   no list is stored: one wave per query runs nn_threshold and then ONE nn_visit pass that adds the
//                         selected neighbours' classes into a per-wave LDS table of u16 counters (k <= 65535), two to a
//                         dword.  The host ranks the distinct labels ascending (<= 4096 of them, 8 KiB per wave), so the
//                         smallest class id is the smallest label.  A wave serves one query, so the table is cleared once per
//                         wave, whole - that is, the ceil(C / 2) dwords the C classes of the call use, which are also all the
//                         winner scan reads.  Clearing only what was touched would take a second nn_visit pass with its fp64
//                         distances; the whole clear costs C / 128 LDS stores per lane.
// Gathers: the list form gathers labels by the original index the lists hold.  The search form visits the points in cell
// order, but nn_visit hands its callback the point, not its sorted position, so the classes stay in the caller's order and are
// gathered by the original index carried in p.w (u16 each: 2n bytes, which stay in the caches at any n this runs at).
// Bytes per list round: n k 4 of lists + n k label gathers of 4 bytes + 8 n (own label read, new label written).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "gsx_ctx.hpp"
#include "nn_device.hpp"

namespace gsx {

static constexpr int kSmMaxK = 64;            // list form
static constexpr int kSmMaxClasses = 4096;    // search form: u16 counters, two to a dword
static constexpr unsigned kSmNoClass = ~0u;   // search form: the ignore label is not among the data's labels

// One round over lists.  shift: log2 of the lanes per query, g = 1 << shift >= k.  No lane leaves before the end: the
// ballots and shuffles below want the whole wave.
__global__ __launch_bounds__(kNnBlock) void smooth_list_kernel(const int32_t* __restrict__ lists, long long n, int k, int shift,
                                                               const int32_t* __restrict__ lab, int32_t* __restrict__ out,
                                                               int32_t* __restrict__ support, unsigned long long* __restrict__ changed,
                                                               int32_t ignore_label, int vote_ignore, int fill_only, unsigned min_votes) {
    const int lane = threadIdx.x & 63;
    const int g = 1 << shift;
    const int j = lane & (g - 1), base = lane - j;  // this lane's neighbour; first lane of its query
    const long long q = ((long long)blockIdx.x * kNnBlock + threadIdx.x) >> shift;
    const bool row = q < n;
    int32_t mine = 0;
    bool votes = false;
    if (row && j < k) {  // never past row q's k entries
        mine = lab[lists[(size_t)q * (size_t)k + (size_t)j]];
        votes = !(vote_ignore && mine == ignore_label);
    }
    const int32_t own = row ? lab[q] : 0;
    const unsigned long long gm = g == 64 ? ~0ull : ((1ull << g) - 1ull) << base;
    const unsigned long long vm = __ballot(votes);
    unsigned cnt = 0;  // voters of my query with my label
    for (int u = 0; u < k; ++u) {
        const int32_t other = __shfl(mine, base + u, 64);
        cnt += (((vm >> (base + u)) & 1ull) && other == mine) ? 1u : 0u;
    }
    if (!votes) cnt = 0;
    unsigned m = cnt;
    for (int s = 1; s < g; s <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, s, 64));
    const bool cand = votes && cnt == m;
    int32_t w = cand ? mine : INT32_MAX;  // the smallest label that reaches m (m >= 1: some lane is a candidate)
    for (int s = 1; s < g; s <<= 1) w = min(w, __shfl_xor(w, s, 64));
    const bool own_wins = (__ballot(cand && mine == own) & gm) != 0;
    int32_t fin = own;
    if (m >= 1 && m >= min_votes) fin = own_wins ? own : w;
    if (fill_only && own != ignore_label) fin = own;
    const unsigned sup = (unsigned)__popcll(__ballot(votes && mine == fin) & gm);
    if (row && j == 0) {
        out[q] = fin;
        if (support) support[q] = (int32_t)sup;
    }
    const unsigned long long ch = __ballot(row && j == 0 && fin != own);
    if (lane == 0 && ch) atomicAdd(changed, (unsigned long long)__popcll(ch));
}

// One round without lists: a wave per query, queries in cell order.  cls / out: class ids by ORIGINAL index; words: dwords of
// the count table the call's classes use.
__global__ __launch_bounds__(kNnBlock) void smooth_search_kernel(NnGrid G, const uint32_t* __restrict__ cs, const float4* __restrict__ pts,
                                                                 long long n, unsigned k, const uint16_t* __restrict__ cls,
                                                                 uint16_t* __restrict__ out, int32_t* __restrict__ support,
                                                                 unsigned long long* __restrict__ changed, unsigned words,
                                                                 unsigned ignore_id, int vote_ignore, int fill_only, unsigned min_votes) {
    __shared__ unsigned hist_all[kNnWaves][256];
    __shared__ unsigned count_all[kNnWaves][kSmMaxClasses / 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * kNnWaves + wave;
    if (q >= n) return;  // wave-uniform; no workgroup barrier below
    const float4 me = pts[q];
    const double qx = me.x, qy = me.y, qz = me.z;
    const NnThreshold T = nn_threshold(G, cs, pts, qx, qy, qz, k, lane, hist_all[wave]);
    unsigned* count = count_all[wave];
    for (unsigned d = lane; d < words; d += 64) count[d] = 0;
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    nn_visit(G, cs, pts, T.cube, lane, [&](const float4& p, bool act) {
        double dx, dy, dz;
        const double d2 = nn_d2(p, qx, qy, qz, dx, dy, dz);
        const uint32_t id = __float_as_uint(p.w);
        if (act && nn_selected(T, d2, id)) {
            const unsigned c = cls[id];
            if (!(vote_ignore && c == ignore_id)) atomicAdd(&count[c >> 1], 1u << (16 * (c & 1u)));  // <= k <= 65535: no carry
        }
    });
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    // the largest count, the smallest class among equals: a lane walks its dwords in ascending class order
    unsigned bc = 0, bi = 0;
    for (unsigned d = lane; d < words; d += 64) {
        const unsigned v = count[d], lo = v & 0xffffu, hi = v >> 16;
        if (lo > bc) {
            bc = lo;
            bi = 2 * d;
        }
        if (hi > bc) {
            bc = hi;
            bi = 2 * d + 1;
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned oc = (unsigned)__shfl_xor((int)bc, s, 64), oi = (unsigned)__shfl_xor((int)bi, s, 64);
        if (oc > bc || (oc == bc && oi < bi)) {
            bc = oc;
            bi = oi;
        }
    }
    if (lane == 0) {
        const uint32_t o = __float_as_uint(me.w);
        const unsigned own = cls[o];
        // an ignored class was never added, so its count is 0 and it is never among the winners (bc >= 1 there)
        const unsigned own_cnt = (count[own >> 1] >> (16 * (own & 1u))) & 0xffffu;
        unsigned fin = own;
        if (bc >= 1 && bc >= min_votes) fin = own_cnt == bc ? own : bi;
        if (fill_only && own != ignore_id) fin = own;
        out[o] = (uint16_t)fin;
        if (support) support[o] = (int32_t)((count[fin >> 1] >> (16 * (fin & 1u))) & 0xffffu);
        if (fin != own) atomicAdd(changed, 1ull);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host
static int smooth_check(Ctx* c, const char* who, int64_t n, int64_t k, const int32_t* labels, const SmoothArgs& a) {
    if (!labels || !a.labels_out) return fail(c, GSX_E_INVALID, "%s: labels or labels_out is NULL", who);
    if (n < 1 || k < 1 || k > n) return fail(c, GSX_E_INVALID, "%s: n < 1 or k outside [1, n]", who);
    if (a.rounds < 1 || a.min_votes < 1) return fail(c, GSX_E_INVALID, "%s: rounds < 1 or min_votes < 1", who);
    if (a.flags & ~(GSX_SMOOTH_IGNORE | GSX_SMOOTH_FILL_ONLY)) return fail(c, GSX_E_INVALID, "%s: unknown flag bits 0x%x", who, (unsigned)a.flags);
    return GSX_OK;
}

// The rounds of a run: round r reads sm_lab[r & 1] and writes the other buffer (launch(r & 1) does); the changed counter comes
// back once per round, and a round that changed nothing is the last.  The result is in sm_lab[done & 1].
template <class Launch>
static int smooth_rounds(Ctx* c, const SmoothArgs& a, int& done, Launch launch) {
    GSX_HIP(c, c->sm_changed.ensure(sizeof(unsigned long long)));
    if (a.changed_out) std::fill(a.changed_out, a.changed_out + a.rounds, (int64_t)0);
    done = 0;
    for (int r = 0; r < a.rounds; ++r) {
        GSX_HIP(c, hipMemsetAsync(c->sm_changed.p, 0, sizeof(unsigned long long), c->stream));
        launch(r & 1);
        GSX_HIP(c, hipGetLastError());
        unsigned long long ch = 0;
        GSX_HIP(c, hipMemcpyAsync(&ch, c->sm_changed.p, sizeof(ch), hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
        done = r + 1;
        if (a.changed_out) a.changed_out[r] = (int64_t)ch;
        if (!ch) break;
    }
    if (a.rounds_done_out) *a.rounds_done_out = done;
    return GSX_OK;
}

// list form over the device lists `lists` (int32[n][k], every index in [0, n))
static int smooth_run_lists(Ctx* c, int64_t n, int k, const int32_t* lists, const int32_t* labels, const SmoothArgs& a) {
    const size_t nn = (size_t)n;
    for (DevBuf& b : c->sm_lab) GSX_HIP(c, b.ensure(sizeof(int32_t) * nn));
    if (a.support_out) GSX_HIP(c, c->sm_sup.ensure(sizeof(int32_t) * nn));
    GSX_HIP(c, hipMemcpyAsync(c->sm_lab[0].p, labels, sizeof(int32_t) * nn, hipMemcpyHostToDevice, c->stream));
    int shift = 0;
    while ((1 << shift) < k) ++shift;
    const long long blocks = (((long long)n << shift) + kNnBlock - 1) / kNnBlock;  // n < 2^31, shift <= 6
    int done = 0;
    int rc = smooth_rounds(c, a, done, [&](int in) {
        ProfScope ps(c, "smooth_list");
        hipLaunchKernelGGL(smooth_list_kernel, dim3((unsigned)blocks), dim3(kNnBlock), 0, c->stream, lists, (long long)n, k, shift,
                           c->sm_lab[in].as<int32_t>(), c->sm_lab[in ^ 1].as<int32_t>(), a.support_out ? c->sm_sup.as<int32_t>() : nullptr,
                           c->sm_changed.as<unsigned long long>(), a.ignore_label, (a.flags & GSX_SMOOTH_IGNORE) != 0,
                           (a.flags & GSX_SMOOTH_FILL_ONLY) != 0, (unsigned)a.min_votes);
    });
    if (rc) return rc;
    GSX_HIP(c, hipMemcpyAsync(a.labels_out, c->sm_lab[done & 1].p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, c->stream));
    if (a.support_out) GSX_HIP(c, hipMemcpyAsync(a.support_out, c->sm_sup.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

int smooth_labels(Ctx* c, int64_t n, const float* points, const int32_t* labels, int64_t k, const SmoothArgs& a) {
    if (!points) return fail(c, GSX_E_INVALID, "smooth_labels: points is NULL");
    int rc = smooth_check(c, "smooth_labels", n, k, labels, a);
    if (rc) return rc;
    if (n > ((int64_t)1 << 31) - 1) return fail(c, GSX_E_UNSUPPORTED, "smooth_labels: n > 2^31-1");
    for (int64_t i = 0; i < 3 * n; ++i)  // on the host: no error of this call comes after a launch
        if (!std::isfinite(points[i])) return fail(c, GSX_E_INVALID, "smooth_labels: a coordinate is not finite");
    const bool search = k > kSmMaxK || c->opt_smooth_search;
    std::vector<int32_t> uniq;
    if (search) {
        if (k > 65535) return fail(c, GSX_E_UNSUPPORTED, "smooth_labels: k > 65535 (the search form counts in 16 bits)");
        uniq.assign(labels, labels + n);
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        if (uniq.size() > (size_t)kSmMaxClasses)
            return fail(c, GSX_E_UNSUPPORTED, "smooth_labels: %zu distinct labels, the search form (k > 64) holds %d", uniq.size(), kSmMaxClasses);
    }
    GSX_HIP(c, hipSetDevice(c->device));
    if (!search) {
        rc = knn_lists(c, "smooth_labels", n, points, (int)k, nullptr, true);
        if (rc) return rc;
        return smooth_run_lists(c, n, (int)k, c->nn_index.as<int32_t>(), labels, a);
    }
    // class ids in ascending label order: "smallest id" is "smallest label"
    const size_t nn = (size_t)n;
    std::vector<uint16_t> ids(nn);
    for (size_t i = 0; i < nn; ++i) ids[i] = (uint16_t)(std::lower_bound(uniq.begin(), uniq.end(), labels[i]) - uniq.begin());
    const auto ig = std::lower_bound(uniq.begin(), uniq.end(), a.ignore_label);
    const unsigned ignore_id = ig != uniq.end() && *ig == a.ignore_label ? (unsigned)(ig - uniq.begin()) : kSmNoClass;
    NnScene S;
    rc = nn_prepare(c, "smooth_labels", n, points, k, S, true);
    if (rc) return rc;
    for (DevBuf& b : c->sm_lab) GSX_HIP(c, b.ensure(sizeof(uint16_t) * nn));
    if (a.support_out) GSX_HIP(c, c->sm_sup.ensure(sizeof(int32_t) * nn));
    GSX_HIP(c, hipMemcpyAsync(c->sm_lab[0].p, ids.data(), sizeof(uint16_t) * nn, hipMemcpyHostToDevice, c->stream));
    const unsigned words = (unsigned)((uniq.size() + 1) / 2);
    int done = 0;
    rc = smooth_rounds(c, a, done, [&](int in) {
        ProfScope ps(c, "smooth_search");
        hipLaunchKernelGGL(smooth_search_kernel, dim3((unsigned)((n + kNnWaves - 1) / kNnWaves)), dim3(kNnBlock), 0, c->stream, S.G,
                           c->nn_cs.as<uint32_t>(), c->nn_pts.as<float4>(), (long long)n, (unsigned)k, c->sm_lab[in].as<uint16_t>(),
                           c->sm_lab[in ^ 1].as<uint16_t>(), a.support_out ? c->sm_sup.as<int32_t>() : nullptr,
                           c->sm_changed.as<unsigned long long>(), words, ignore_id, (a.flags & GSX_SMOOTH_IGNORE) != 0,
                           (a.flags & GSX_SMOOTH_FILL_ONLY) != 0, (unsigned)a.min_votes);
    });
    if (rc) return rc;
    GSX_HIP(c, hipMemcpyAsync(ids.data(), c->sm_lab[done & 1].p, sizeof(uint16_t) * nn, hipMemcpyDeviceToHost, c->stream));
    if (a.support_out) GSX_HIP(c, hipMemcpyAsync(a.support_out, c->sm_sup.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < nn; ++i) a.labels_out[i] = uniq[ids[i]];
    return GSX_OK;
}

int smooth_labels_lists(Ctx* c, int64_t n, int32_t k, const int32_t* knn, const int32_t* labels, const SmoothArgs& a) {
    int rc = smooth_check(c, "smooth_labels_lists", n, k, labels, a);
    if (rc) return rc;
    if (k > kSmMaxK) return fail(c, GSX_E_INVALID, "smooth_labels_lists: k > 64");
    if (n > ((int64_t)1 << 31) - 1) return fail(c, GSX_E_UNSUPPORTED, "smooth_labels_lists: n > 2^31-1");
    const size_t nk = (size_t)n * (size_t)k;
    if (knn) {
        for (size_t t = 0; t < nk; ++t)
            if (knn[t] < 0 || knn[t] >= n)
                return fail(c, GSX_E_INVALID, "smooth_labels_lists: index %d outside [0, n) in row %zu, column %zu", knn[t], t / (size_t)k, t % (size_t)k);
    } else if (c->nn_index_rows != n || c->nn_index_k != k) {
        return fail(c, GSX_E_STATE, "smooth_labels_lists: knn is NULL and the context holds no lists of this n and k (gsx_knn first)");
    }
    GSX_HIP(c, hipSetDevice(c->device));
    const int32_t* lists = c->nn_index.as<int32_t>();
    if (knn) {
        GSX_HIP(c, c->sm_lists.ensure(sizeof(int32_t) * nk));
        GSX_HIP(c, hipMemcpyAsync(c->sm_lists.p, knn, sizeof(int32_t) * nk, hipMemcpyHostToDevice, c->stream));
        lists = c->sm_lists.as<int32_t>();
    }
    return smooth_run_lists(c, n, k, lists, labels, a);
}

void smooth_constants(int32_t out[8]) {
    out[0] = kSmMaxK;
    out[1] = kSmMaxClasses;
    out[2] = 16;  // bits of a counter of the search form's table, two counters to a dword
    out[3] = 64;  // lanes of the winner scan: lane l reads the dwords l, l + 64, ..
    out[4] = kNnWaves;
    out[5] = out[6] = out[7] = 0;
}

}  // namespace gsx
