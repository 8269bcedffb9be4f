// nn_device.hpp - the exact k-nearest-neighbour search that normals.hip (normals, residuals, lists) and smooth.hip (the label
// filter's search form) share: the uniform grid, the ring, the radix select over the composite key (bits of d2, index), the
// visit of a cube of cells, and the host side that sizes the grid, bins the points and uploads them.  normals.hip's header
// comment describes the search.  Every unit that includes it is compiled with -ffp-contract=off: the distance is
// (dx*dx + dy*dy) + dz*dz without FMA.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "gsx_ctx.hpp"

namespace gsx {

static constexpr int kNnBlock = 256;
static constexpr int kNnWaves = kNnBlock / 64;
static constexpr int kNnMaxDim = 1024;      // cells per axis
static constexpr double kNnMargin = 1e-5;   // of a cell edge: covers the rounding of floor((p - o) * inv_h), < 1e-12

struct NnGrid {
    double o[3], h, inv_h;
    int g[3];
};

static __global__ void nn_finite_kernel(const float* __restrict__ p, long long n3, int* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3 && !isfinite(p[i])) atomicOr(flag, 1);
}

__device__ inline unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}
__device__ inline double wave_sum_f64(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

struct NnCube {
    int x0, x1, y0, y1, z0, z1;
};

// f(point, active) for every point of the cube's cells; the loop is wave-uniform, `active` masks the tail
template <class F>
__device__ inline void nn_visit(const NnGrid& G, const uint32_t* __restrict__ cs, const float4* __restrict__ pts, const NnCube& q,
                                int lane, F f) {
    for (int z = q.z0; z <= q.z1; ++z)
        for (int y = q.y0; y <= q.y1; ++y) {
            const size_t row = ((size_t)z * G.g[1] + y) * G.g[0];
            const uint32_t b = cs[row + q.x0], e = cs[row + q.x1 + 1];
            for (uint32_t j0 = b; j0 < e; j0 += 64) {
                const uint32_t j = j0 + lane;
                const bool act = j < e;
                const float4 p = pts[act ? j : b];
                f(p, act);
            }
        }
}

__device__ inline double nn_d2(const float4& p, double qx, double qy, double qz, double& dx, double& dy, double& dz) {
    dx = (double)p.x - qx;
    dy = (double)p.y - qy;
    dz = (double)p.z - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

struct NnThreshold {
    NnCube cube;
    double R2;                 // candidates are the cube's points with d2 <= R2
    unsigned long long tk;     // selected: key < tk, or key == tk and index <= ti
    uint32_t ti;
};

__device__ inline bool nn_selected(const NnThreshold& T, double d2, uint32_t idx) {
    const unsigned long long key = (unsigned long long)__double_as_longlong(d2);
    return d2 <= T.R2 && (key < T.tk || (key == T.tk && idx <= T.ti));
}

// steps 1 and 2 of normals.hip's header comment for the query (qx, qy, qz); hist: 256 LDS counters of this wave
__device__ inline NnThreshold nn_threshold(const NnGrid& G, const uint32_t* __restrict__ cs, const float4* __restrict__ pts, double qx,
                                           double qy, double qz, unsigned k, int lane, unsigned* hist) {
    NnThreshold T;
    const double qq[3] = {qx, qy, qz};
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double t = floor((qq[a] - G.o[a]) * G.inv_h);
        c[a] = t < 0.0 ? 0 : (t > (double)(G.g[a] - 1) ? G.g[a] - 1 : (int)t);
    }
    // ---- 1. ring ----
    for (int r = 0;; ) {
        int lo[3], hi[3];
        double R = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = max(c[a] - r, 0);
            hi[a] = min(c[a] + r, G.g[a] - 1);
            if (lo[a] > 0) R = fmin(R, qq[a] - (G.o[a] + (double)lo[a] * G.h));
            if (hi[a] < G.g[a] - 1) R = fmin(R, (G.o[a] + (double)(hi[a] + 1) * G.h) - qq[a]);
        }
        T.cube = NnCube{lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]};
        if (R == INFINITY) {  // the cube is the whole grid
            T.R2 = INFINITY;
            break;
        }
        R -= kNnMargin * G.h;
        unsigned cnt = 0;
        if (R > 0.0) {
            const double R2 = R * R;
            unsigned mine = 0;
            nn_visit(G, cs, pts, T.cube, lane, [&](const float4& p, bool act) {
                double dx, dy, dz;
                const double d2 = nn_d2(p, qx, qy, qz, dx, dy, dz);
                mine += (act && d2 <= R2) ? 1u : 0u;
            });
            cnt = wave_sum_u32(mine);
            if (cnt >= k) {
                T.R2 = R2;
                break;
            }
        }
        r = (cnt < k / 8) ? 2 * r + 1 : r + 1;  // nearly empty: double the ring
    }
    // ---- 2. radix select of the k-th composite key ----
    unsigned long long pk = 0;  // digits fixed so far
    uint32_t pi = 0;
    unsigned need = k;
    T.tk = ~0ull;
    T.ti = ~0u;
    for (int t = 0; t < 12; ++t) {
        for (int b = lane; b < 256; b += 64) hist[b] = 0;
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
        nn_visit(G, cs, pts, T.cube, lane, [&](const float4& p, bool act) {
            double dx, dy, dz;
            const double d2 = nn_d2(p, qx, qy, qz, dx, dy, dz);
            const unsigned long long key = (unsigned long long)__double_as_longlong(d2);
            const uint32_t idx = __float_as_uint(p.w);
            bool in = act && d2 <= T.R2;
            unsigned digit;
            if (t < 8) {
                if (t > 0) in = in && (key >> (64 - 8 * t)) == (pk >> (64 - 8 * t));
                digit = (unsigned)(key >> (56 - 8 * t)) & 255u;
            } else {
                in = in && key == pk;
                if (t > 8) in = in && (idx >> (32 - 8 * (t - 8))) == (pi >> (32 - 8 * (t - 8)));
                digit = (idx >> (24 - 8 * (t - 8))) & 255u;
            }
            const unsigned long long m = __ballot(in);
            if (m) {  // lanes that share the first one's digit add once (the top digits are the same for all)
                const int first = __ffsll((long long)m) - 1;
                const unsigned d0 = (unsigned)__shfl((int)digit, first, 64);
                const unsigned long long same = __ballot(in && digit == d0);
                if (lane == first) atomicAdd(&hist[d0], (unsigned)__popcll(same));
                if (in && digit != d0) atomicAdd(&hist[digit], 1u);
            }
        });
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
        // lane l owns the counters 4l .. 4l+3
        unsigned h4[4];
        unsigned s = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            h4[b] = hist[4 * lane + b];
            s += h4[b];
        }
        unsigned incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        unsigned cum = incl - s, digit = 0, before = 0, inside = 0;
        bool found = false;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (!found && need > cum && need <= cum + h4[b]) {
                found = true;
                digit = 4 * lane + b;
                before = cum;
                inside = h4[b];
            }
            cum += h4[b];
        }
        const unsigned long long fm = __ballot(found);
        const int src = fm ? __ffsll((long long)fm) - 1 : 0;  // fm != 0: the candidates hold >= k points
        digit = (unsigned)__shfl((int)digit, src, 64);
        before = (unsigned)__shfl((int)before, src, 64);
        inside = (unsigned)__shfl((int)inside, src, 64);
        if (t < 8) pk |= (unsigned long long)digit << (56 - 8 * t);
        else pi |= digit << (24 - 8 * (t - 8));
        if (need == before + inside || t == 11) {  // the bucket is taken whole: everything at or below its upper end
            if (t < 8) {
                T.tk = pk | (t < 7 ? (~0ull >> (8 * (t + 1))) : 0ull);
                T.ti = ~0u;
            } else {
                T.tk = pk;
                T.ti = pi | (t < 11 ? (~0u >> (8 * (t - 8 + 1))) : 0u);
            }
            break;
        }
        need -= before;
    }
    return T;
}

// ---------------------------------------------------------------------------------------------------------------
// host: validation, grid, upload
struct NnScene {
    NnGrid G;
};

// grid sizing and counting sort: host arithmetic only, no context and no HIP call (gsx_debug_nn_grid shows it to the tests).
// start: cells + 1 offsets into sorted, cells in x-fastest order; sorted: (x, y, z, bits of the original index)
static void nn_grid_sort(int64_t n, const float* points, int64_t k, bool brute, NnGrid& G, std::vector<uint32_t>& start,
                         std::vector<float4>& sorted) {
    // robust bounding box
    double ext[3];
    for (int a = 0; a < 3; ++a) {
        double lo, hi;
        if (n <= 4096) {
            lo = hi = points[a];
            for (int64_t i = 1; i < n; ++i) {
                lo = std::min(lo, (double)points[i * 3 + a]);
                hi = std::max(hi, (double)points[i * 3 + a]);
            }
        } else {
            const int64_t m = std::min<int64_t>(n, 65536), step = n / m;
            std::vector<float> sm((size_t)m);
            for (int64_t i = 0; i < m; ++i) sm[(size_t)i] = points[i * step * 3 + a];
            const size_t cut = (size_t)(m / 200);
            std::nth_element(sm.begin(), sm.begin() + cut, sm.end());
            lo = sm[cut];
            std::nth_element(sm.begin(), sm.end() - 1 - cut, sm.end());
            hi = sm[sm.size() - 1 - cut];
        }
        G.o[a] = lo;
        ext[a] = hi - lo;
    }
    int dims = 0;
    double vol = 1.0;
    for (int a = 0; a < 3; ++a)
        if (ext[a] > 0.0) {
            ++dims;
            vol *= ext[a];
        }
    G.g[0] = G.g[1] = G.g[2] = 1;
    G.h = 1.0;
    if (dims > 0 && !brute) {
        // about 3 cells of ring radius for k neighbours: k = (4 pi / 3) 27 occupancy
        const double occupancy = std::max(2.0, (double)k / 113.0);
        const double cells = std::max(1.0, (double)n / occupancy);
        G.h = std::pow(vol / cells, 1.0 / dims);
        if (!(G.h > 0.0) || !std::isfinite(G.h)) G.h = 1.0;
        for (;;) {  // the cells cover the whole box: the edge grows until both caps hold
            double total = 1.0;
            bool fits = true;
            for (int a = 0; a < 3; ++a) {
                const double ga = std::floor(ext[a] / G.h) + 1.0;
                fits = fits && ga <= (double)kNnMaxDim;
                G.g[a] = (int)std::min((double)kNnMaxDim, ga);
                total *= G.g[a];
            }
            if (fits && total <= 4.0 * (double)n + 64.0) break;
            G.h *= 1.26;
        }
    }
    G.inv_h = 1.0 / G.h;
    const size_t ncells = (size_t)G.g[0] * G.g[1] * G.g[2];
    // counting sort by cell, x fastest; stable, so a cell's points stay in index order
    std::vector<uint32_t> cell((size_t)n);
    start.assign(ncells + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        size_t id = 0;
        for (int a = 2; a >= 0; --a) {
            const double t = std::floor(((double)points[i * 3 + a] - G.o[a]) * G.inv_h);  // the kernels' expression
            const int ca = t < 0.0 ? 0 : (t > (double)(G.g[a] - 1) ? G.g[a] - 1 : (int)t);
            id = id * G.g[a] + ca;
        }
        cell[(size_t)i] = (uint32_t)id;
        ++start[id + 1];
    }
    for (size_t j = 0; j < ncells; ++j) start[j + 1] += start[j];
    sorted.resize((size_t)n);
    {
        std::vector<uint32_t> at(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < n; ++i) {
            float4 v;
            v.x = points[i * 3];
            v.y = points[i * 3 + 1];
            v.z = points[i * 3 + 2];
            const uint32_t u = (uint32_t)i;
            std::memcpy(&v.w, &u, 4);
            sorted[at[cell[(size_t)i]]++] = v;
        }
    }
}

// the buffers live in the context (nn_*), as every other path's do: nothing is allocated once they have grown.
// checked: the caller has already had these points through the finite check (the second search of gsx_region_growing)
static int nn_prepare(Ctx* c, const char* who, int64_t n, const float* points, int64_t k, NnScene& S, bool checked = false) {
    GSX_HIP(c, hipSetDevice(c->device));
    // non-finite coordinates are found on the device, before anything is derived from them
    if (!checked) {
        DevBuf& raw = c->nn_out;  // the output buffer is free until the search has run
        DevBuf& flag = c->nn_flag;
        GSX_HIP(c, raw.ensure(sizeof(float) * 3 * (size_t)n));
        GSX_HIP(c, flag.ensure(sizeof(int)));
        GSX_HIP(c, hipMemcpyAsync(raw.p, points, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        GSX_HIP(c, hipMemsetAsync(flag.p, 0, sizeof(int), c->stream));
        const long long n3 = 3 * (long long)n;
        hipLaunchKernelGGL(nn_finite_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, c->stream, raw.as<float>(), n3, flag.as<int>());
        GSX_HIP(c, hipGetLastError());
        int bad = 0;
        GSX_HIP(c, hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
        if (bad) return fail(c, GSX_E_INVALID, "%s: a coordinate is not finite", who);
    }
    std::vector<uint32_t> start;
    std::vector<float4> sorted;
    nn_grid_sort(n, points, k, c->opt_nn_brute != 0, S.G, start, sorted);
    const size_t ncells = start.size() - 1;
    GSX_HIP(c, c->nn_pts.ensure(sizeof(float4) * (size_t)n));
    GSX_HIP(c, c->nn_cs.ensure(sizeof(uint32_t) * (ncells + 1)));
    GSX_HIP(c, hipMemcpyAsync(c->nn_pts.p, sorted.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemcpyAsync(c->nn_cs.p, start.data(), sizeof(uint32_t) * (ncells + 1), hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
    return GSX_OK;
}

}  // namespace gsx
