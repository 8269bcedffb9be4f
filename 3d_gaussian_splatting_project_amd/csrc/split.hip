// split.hip - class labels into object instances: connected components of every label over the k-nearest-neighbour graph
// (gsx_split_labels, gsx_split_labels_lists; include/gsx.h states the rule).  Points i and j are joined when one of them
// lists the other, both carry the same non-ignored label and d2(i, j) <= r2; a component is an object, the largest
// components get the smallest ids, components below min_size become -1.
//
// A lock-free union-find on parent[n], in a fixed number of launches whatever the graph (a wall is one component thousands
// of hops across: iterating a min-label propagation from the host would take that many rounds):
//   init      parent[i] = i
//   hook      the lane layout of smooth_list_kernel: g = the power of two >= k lanes per point, 64 / g points per wave, the
//             list read coalesced.  A lane takes one entry j of row i, gathers labels[j] (and the coordinates when a distance
//             is given), drops self, label-mismatch, ignored and too-far entries and unites i and j.
//   flatten   rep[i] = find(i), -1 for an ignored point
//   sizes     size[rep[i]] += 1, one add per distinct rep in a wave, gathered per workgroup in LDS; then the roots with
//             size >= min_size are compacted as (rep, size, label) triples through a wave-aggregated counter, in whatever order
//   (host)    one wait for M; sorts the triples by (-size, rep), cuts at max_instances, uploads the kept reps in rank order
//   relabel   id_of[rep of rank m] = m over an id_of preset to -1; labels_out[i] = rep[i] >= 0 ? id_of[rep[i]] : -1
//
// The union.  Invariant: parent[x] <= x at all times, so every root is the smallest index its tree holds and there is no
// cycle.  find walks up with path halving; unite takes the two roots hi > lo and tries atomicCAS(&parent[hi], hi, lo).  A
// failed CAS returns what parent[hi] holds now, which is below hi: the walk continues from there.  Every retry strictly lowers
// a value, so a lane always makes progress on its own and never waits for another lane to write something.
// Stale reads are harmless: the loads are relaxed and may return an older value of parent[x], but every value parent[x] ever
// held is an ancestor of x, and x's set only grows - so "both walks ended at the same node" proves one set, a walk that ends
// at a node which is no root any more makes the CAS fail (or hangs hi under a lower member of the other set, which joins the
// sets just as well), and a halving store that puts back an older ancestor keeps parent[x] < x inside x's set.  A halving
// store never meets a CAS on the same word: it writes parent[x] only after x was seen with another parent, and such an x is
// never a root again, while the CAS changes only words that still hold their own index.  The atomics are ordinary vector
// global atomics at device scope.
// The result does not depend on the order of the joins: the partition is the graph's, rep is its smallest index, sizes are
// integer counts, and the host's sort key (-size, rep) is total.
// Bytes: lists n k 4 + label gathers n k 4 (+ coordinate gathers n k 12 with a distance) + the parent traffic: 4 n of init,
// two finds per kept entry (a few dwords each once halving has flattened the trees), 4 n of flatten reads + 4 n of rep.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "gsx_ctx.hpp"

namespace gsx {

static constexpr int kSpMaxK = 64;
static constexpr int kSpBlock = 256;
static constexpr int kSpCountPer = 16;              // split_count_kernel: points per thread ...
static constexpr int kSpSlotBits = 9;               // ... and its LDS table: 512 (rep, count) slots, 4 KiB
static constexpr int kSpSlots = 1 << kSpSlotBits;
static constexpr int kSpProbes = 8;

__device__ inline int32_t sp_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as far as this lane can see, halving the path on the way (parent[x] <- its grandparent)
__device__ inline int32_t sp_find(int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = sp_load(parent + x);
        if (p == x) return x;
        const int32_t gp = sp_load(parent + p);
        if (gp == p) return p;
        __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = gp;
    }
}

__device__ inline void sp_unite(int32_t* parent, int32_t a, int32_t b) {
    a = sp_find(parent, a);
    b = sp_find(parent, b);
    while (a != b) {  // a == b: one set already, no CAS
        const int32_t hi = max(a, b), lo = min(a, b);
        const int32_t seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;
        a = sp_find(parent, seen);  // seen < hi: hi has been hung under it meanwhile
        b = lo;
    }
}

__global__ __launch_bounds__(kSpBlock) void split_init_kernel(long long n, int32_t* __restrict__ parent) {
    const long long i = (long long)blockIdx.x * kSpBlock + threadIdx.x;
    if (i < n) parent[i] = (int32_t)i;
}

// pts: float[n][3] in the caller's order, or NULL when no distance is given.  No wave-wide operation: a lane leaves as soon
// as its entry is no edge.
__global__ __launch_bounds__(kSpBlock) void split_hook_kernel(const int32_t* __restrict__ lists, long long n, int k, int shift,
                                                              const int32_t* __restrict__ lab, const float* __restrict__ pts, double r2,
                                                              int32_t ignore_label, int use_ignore, int32_t* parent) {
    const int j = threadIdx.x & ((1 << shift) - 1);
    const long long q = ((long long)blockIdx.x * kSpBlock + threadIdx.x) >> shift;
    if (q >= n || j >= k) return;  // never past row q's k entries
    const int32_t o = lists[(size_t)q * (size_t)k + (size_t)j];
    if (o == (int32_t)q) return;  // a self loop is no edge
    const int32_t mine = lab[q];
    if (lab[o] != mine || (use_ignore && mine == ignore_label)) return;
    if (pts) {
        const float* a = pts + 3 * (size_t)q;
        const float* b = pts + 3 * (size_t)o;
        const double dx = (double)b[0] - (double)a[0], dy = (double)b[1] - (double)a[1], dz = (double)b[2] - (double)a[2];
        if (!((dx * dx + dy * dy) + dz * dz <= r2)) return;  // nn_d2's expression; this unit is built without contraction
    }
    sp_unite(parent, (int32_t)q, o);
}

__global__ __launch_bounds__(kSpBlock) void split_flatten_kernel(long long n, const int32_t* __restrict__ lab, int32_t ignore_label,
                                                                 int use_ignore, int32_t* parent, int32_t* __restrict__ rep) {
    const long long i = (long long)blockIdx.x * kSpBlock + threadIdx.x;
    if (i >= n) return;
    rep[i] = (use_ignore && lab[i] == ignore_label) ? -1 : sp_find(parent, (int32_t)i);
}

// size[r] = points with rep r.  Two levels of aggregation before a global add.  In a wave, the lanes that hold the same rep
// add once: the first live lane's value is broadcast, the lanes that share it are counted by ballot and retire (the trick of
// nn_threshold's histogram, repeated until no lane is left).  In a workgroup, which walks kSpCountPer * 256 consecutive points,
// those per-wave sums go into an LDS table keyed by rep (open addressing, a few probes, else straight to memory) that is
// flushed once.  The reps of the large components are small indices, so their counters share a few cache lines, and with
// the wave level alone 3 M points in ~100 components are about 2.3 M adds on those lines; this form adds once per component and
// workgroup.
__global__ __launch_bounds__(kSpBlock) void split_count_kernel(long long n, const int32_t* __restrict__ rep, unsigned* __restrict__ size) {
    __shared__ int32_t key[kSpSlots];
    __shared__ unsigned num[kSpSlots];
    for (int s = threadIdx.x; s < kSpSlots; s += kSpBlock) {
        key[s] = -1;
        num[s] = 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long base = (long long)blockIdx.x * (kSpBlock * kSpCountPer);
    for (int it = 0; it < kSpCountPer; ++it) {  // uniform over the workgroup: every lane reaches the barrier below
        const long long i = base + (long long)it * kSpBlock + threadIdx.x;
        const int32_t r = i < n ? rep[i] : -1;
        bool live = r >= 0;
        unsigned long long m = __ballot(live);
        while (m) {
            const int first = __ffsll((long long)m) - 1;
            const int32_t v = __shfl(r, first, 64);
            const unsigned long long same = __ballot(live && r == v);
            if (lane == first) {
                const unsigned c = (unsigned)__popcll(same);
                unsigned s = ((unsigned)v * 2654435761u) >> (32 - kSpSlotBits);
                bool placed = false;
                for (int p = 0; p < kSpProbes && !placed; ++p, s = (s + 1) & (kSpSlots - 1)) {
                    const int32_t seen = atomicCAS(&key[s], -1, v);
                    if (seen == -1 || seen == v) {
                        atomicAdd(&num[s], c);
                        placed = true;
                    }
                }
                if (!placed) atomicAdd(&size[v], c);
            }
            if (r == v) live = false;
            m &= ~same;
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kSpSlots; s += kSpBlock)
        if (key[s] >= 0) atomicAdd(&size[key[s]], num[s]);
}

// the roots with size >= min_size as triples, any order; cnt[0] = triples written, cnt[1] = roots (components)
__global__ __launch_bounds__(kSpBlock) void split_compact_kernel(long long n, const int32_t* __restrict__ rep, const unsigned* __restrict__ size,
                                                                 const int32_t* __restrict__ lab, long long min_size, unsigned* __restrict__ cnt,
                                                                 int32_t* __restrict__ t_rep, int32_t* __restrict__ t_size,
                                                                 int32_t* __restrict__ t_lab) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * kSpBlock + threadIdx.x;
    const bool root = i < n && rep[i] == (int32_t)i;
    const unsigned sz = root ? size[i] : 0u;
    const bool keep = root && (long long)sz >= min_size;
    const unsigned long long rm = __ballot(root), km = __ballot(keep);
    if (!rm) return;  // wave-uniform
    unsigned base = 0;
    if (lane == 0) {
        atomicAdd(&cnt[1], (unsigned)__popcll(rm));
        if (km) base = atomicAdd(&cnt[0], (unsigned)__popcll(km));
    }
    base = (unsigned)__shfl((int)base, 0, 64);
    if (keep) {
        const unsigned at = base + (unsigned)__popcll(km & ((1ull << lane) - 1ull));  // < n: at most one triple per point
        t_rep[at] = (int32_t)i;
        t_size[at] = (int32_t)sz;
        t_lab[at] = lab[i];
    }
}

__global__ __launch_bounds__(kSpBlock) void split_scatter_kernel(int m, const int32_t* __restrict__ kept, int32_t* __restrict__ id_of) {
    const long long t = (long long)blockIdx.x * kSpBlock + threadIdx.x;
    if (t < m) id_of[kept[t]] = (int32_t)t;  // kept[t] is a root of this run: in [0, n)
}

__global__ __launch_bounds__(kSpBlock) void split_relabel_kernel(long long n, const int32_t* __restrict__ rep, const int32_t* __restrict__ id_of,
                                                                 int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kSpBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t r = rep[i];
    out[i] = r >= 0 ? id_of[r] : -1;
}

// ---------------------------------------------------------------------------------------------------------------
// host
static int split_check(Ctx* c, const char* who, int64_t n, int64_t k, int64_t k_min, const int32_t* labels, const SplitArgs& a) {
    if (!labels || !a.labels_out) return fail(c, GSX_E_INVALID, "%s: labels or labels_out is NULL", who);
    if (n < 1 || k < k_min || k > kSpMaxK || k > n) return fail(c, GSX_E_INVALID, "%s: n < 1 or k outside [%d, min(64, n)]", who, (int)k_min);
    if (a.min_size < 1 || a.max_instances < 0) return fail(c, GSX_E_INVALID, "%s: min_size < 1 or max_instances < 0", who);
    if (!(a.max_dist > 0)) return fail(c, GSX_E_INVALID, "%s: max_dist is NaN or <= 0 (+inf: no cut)", who);
    if (a.flags & ~GSX_SPLIT_IGNORE) return fail(c, GSX_E_INVALID, "%s: unknown flag bits 0x%x", who, (unsigned)a.flags);
    if (n > ((int64_t)1 << 31) - 1) return fail(c, GSX_E_UNSUPPORTED, "%s: n > 2^31-1", who);
    return GSX_OK;
}

static int split_check_points(Ctx* c, const char* who, int64_t n, const float* points) {
    for (int64_t i = 0; i < 3 * n; ++i)  // on the host: no error of this call comes after a launch
        if (!std::isfinite(points[i])) return fail(c, GSX_E_INVALID, "%s: a coordinate is not finite", who);
    return GSX_OK;
}

// over the device lists `lists` (int32[n][k], every index in [0, n)); points: host, used iff max_dist is finite
static int split_run(Ctx* c, int64_t n, int k, const int32_t* lists, const float* points, const int32_t* labels, const SplitArgs& a) {
    const size_t nn = (size_t)n;
    const bool cut = std::isfinite(a.max_dist);
    const double r2 = a.max_dist * a.max_dist;  // the one fp64 product of the rule (+inf for a huge max_dist: no cut either)
    const int use_ignore = (a.flags & GSX_SPLIT_IGNORE) != 0;
    for (DevBuf* b : {&c->sp_lab, &c->sp_parent, &c->sp_rep, &c->sp_size, &c->sp_id, &c->sp_kept}) GSX_HIP(c, b->ensure(sizeof(int32_t) * nn));
    GSX_HIP(c, c->sp_trip.ensure(sizeof(int32_t) * 3 * nn));
    GSX_HIP(c, c->sp_cnt.ensure(2 * sizeof(unsigned)));
    if (cut) GSX_HIP(c, c->sp_pts.ensure(sizeof(float) * 3 * nn));
    int32_t *lab = c->sp_lab.as<int32_t>(), *parent = c->sp_parent.as<int32_t>(), *rep = c->sp_rep.as<int32_t>(), *id_of = c->sp_id.as<int32_t>();
    int32_t *t_rep = c->sp_trip.as<int32_t>(), *t_size = t_rep + nn, *t_lab = t_size + nn;
    unsigned *size = c->sp_size.as<unsigned>(), *cnt = c->sp_cnt.as<unsigned>();
    GSX_HIP(c, hipMemcpyAsync(lab, labels, sizeof(int32_t) * nn, hipMemcpyHostToDevice, c->stream));
    if (cut) GSX_HIP(c, hipMemcpyAsync(c->sp_pts.p, points, sizeof(float) * 3 * nn, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemsetAsync(size, 0, sizeof(unsigned) * nn, c->stream));
    GSX_HIP(c, hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned), c->stream));
    GSX_HIP(c, hipMemsetAsync(id_of, 0xff, sizeof(int32_t) * nn, c->stream));  // -1
    int shift = 0;
    while ((1 << shift) < k) ++shift;
    const dim3 per_point((unsigned)((n + kSpBlock - 1) / kSpBlock)), block(kSpBlock);
    const dim3 per_entry((unsigned)((((long long)n << shift) + kSpBlock - 1) / kSpBlock));  // n < 2^31, shift <= 6
    {
        ProfScope ps(c, "split_hook");
        hipLaunchKernelGGL(split_init_kernel, per_point, block, 0, c->stream, (long long)n, parent);
    }
    {
        ProfScope ps(c, "split_hook");
        hipLaunchKernelGGL(split_hook_kernel, per_entry, block, 0, c->stream, lists, (long long)n, k, shift, lab,
                           cut ? c->sp_pts.as<float>() : nullptr, r2, a.ignore_label, use_ignore, parent);
    }
    {
        ProfScope ps(c, "split_flatten");
        hipLaunchKernelGGL(split_flatten_kernel, per_point, block, 0, c->stream, (long long)n, lab, a.ignore_label, use_ignore, parent, rep);
    }
    {
        ProfScope ps(c, "split_sizes");
        const long long per = (long long)kSpBlock * kSpCountPer;
        hipLaunchKernelGGL(split_count_kernel, dim3((unsigned)((n + per - 1) / per)), block, 0, c->stream, (long long)n, rep, size);
    }
    {
        ProfScope ps(c, "split_sizes");
        hipLaunchKernelGGL(split_compact_kernel, per_point, block, 0, c->stream, (long long)n, rep, size, lab, (long long)a.min_size, cnt, t_rep,
                           t_size, t_lab);
    }
    GSX_HIP(c, hipGetLastError());
    unsigned counts[2] = {0, 0};
    GSX_HIP(c, hipMemcpyAsync(counts, cnt, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));  // the one wait in the middle: M
    const size_t found = counts[0];
    std::vector<int32_t> trip(3 * found);
    if (found) {  // plain copies: the stream is idle, and no queued copy may outlive `trip` on an early return
        GSX_HIP(c, hipMemcpy(trip.data(), t_rep, sizeof(int32_t) * found, hipMemcpyDeviceToHost));
        GSX_HIP(c, hipMemcpy(trip.data() + found, t_size, sizeof(int32_t) * found, hipMemcpyDeviceToHost));
        GSX_HIP(c, hipMemcpy(trip.data() + 2 * found, t_lab, sizeof(int32_t) * found, hipMemcpyDeviceToHost));
    }
    const int32_t *h_rep = trip.data(), *h_size = h_rep + found, *h_lab = h_size + found;
    std::vector<uint32_t> order(found);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return h_size[x] != h_size[y] ? h_size[x] > h_size[y] : h_rep[x] < h_rep[y]; });
    const size_t m = a.max_instances > 0 ? std::min(found, (size_t)a.max_instances) : found;
    std::vector<int32_t> kept(std::max<size_t>(m, 1));
    for (size_t t = 0; t < m; ++t) kept[t] = h_rep[order[t]];
    if (m) GSX_HIP(c, hipMemcpy(c->sp_kept.p, kept.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));  // done before `kept` can go
    {
        ProfScope ps(c, "split_relabel");
        hipLaunchKernelGGL(split_scatter_kernel, dim3((unsigned)((std::max<size_t>(m, 1) + kSpBlock - 1) / kSpBlock)), block, 0, c->stream, (int)m,
                           c->sp_kept.as<int32_t>(), id_of);
    }
    {
        ProfScope ps(c, "split_relabel");
        hipLaunchKernelGGL(split_relabel_kernel, per_point, block, 0, c->stream, (long long)n, rep, id_of, lab);  // lab is read no more
    }
    GSX_HIP(c, hipGetLastError());
    GSX_HIP(c, hipMemcpyAsync(a.labels_out, lab, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, c->stream));
    if (a.component_out) GSX_HIP(c, hipMemcpyAsync(a.component_out, rep, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t t = 0; t < m; ++t) {
        if (a.instance_label_out) a.instance_label_out[t] = h_lab[order[t]];
        if (a.instance_size_out) a.instance_size_out[t] = h_size[order[t]];
        if (a.instance_rep_out) a.instance_rep_out[t] = h_rep[order[t]];
    }
    if (a.n_instances_out) *a.n_instances_out = (int32_t)m;
    if (a.n_components_out) *a.n_components_out = (int64_t)counts[1];
    return GSX_OK;
}

int split_labels(Ctx* c, int64_t n, const float* points, const int32_t* labels, int32_t k, const SplitArgs& a) {
    if (!points) return fail(c, GSX_E_INVALID, "split_labels: points is NULL");
    int rc = split_check(c, "split_labels", n, k, 2, labels, a);
    if (rc) return rc;
    rc = split_check_points(c, "split_labels", n, points);
    if (rc) return rc;
    GSX_HIP(c, hipSetDevice(c->device));
    rc = knn_lists(c, "split_labels", n, points, k, nullptr, true);
    if (rc) return rc;
    return split_run(c, n, k, c->nn_index.as<int32_t>(), points, labels, a);
}

int split_labels_lists(Ctx* c, int64_t n, int32_t k, const int32_t* knn, const float* points, const int32_t* labels, const SplitArgs& a) {
    int rc = split_check(c, "split_labels_lists", n, k, 1, labels, a);
    if (rc) return rc;
    if (!points && std::isfinite(a.max_dist)) return fail(c, GSX_E_INVALID, "split_labels_lists: a finite max_dist needs points");
    if (points) {
        rc = split_check_points(c, "split_labels_lists", n, points);
        if (rc) return rc;
    }
    const size_t nk = (size_t)n * (size_t)k;
    if (knn) {
        for (size_t t = 0; t < nk; ++t)
            if (knn[t] < 0 || knn[t] >= n)
                return fail(c, GSX_E_INVALID, "split_labels_lists: index %d outside [0, n) in row %zu, column %zu", knn[t], t / (size_t)k, t % (size_t)k);
    } else if (c->nn_index_rows != n || c->nn_index_k != k) {
        return fail(c, GSX_E_STATE, "split_labels_lists: knn is NULL and the context holds no lists of this n and k (gsx_knn first)");
    }
    GSX_HIP(c, hipSetDevice(c->device));
    const int32_t* lists = c->nn_index.as<int32_t>();
    if (knn) {
        GSX_HIP(c, c->sp_lists.ensure(sizeof(int32_t) * nk));
        GSX_HIP(c, hipMemcpyAsync(c->sp_lists.p, knn, sizeof(int32_t) * nk, hipMemcpyHostToDevice, c->stream));
        lists = c->sp_lists.as<int32_t>();
    }
    return split_run(c, n, k, lists, points, labels, a);
}

}  // namespace gsx
