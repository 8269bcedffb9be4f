// normals.hip - the geometric front of the reference's third labeler, 3D_clustering/region_growing.py ("rg.py"):
// exact k nearest neighbours, PCA normals and plane residuals as HIP kernels for gfx950.
//
//   gsx_normals   rg.py:78-129 compute_normals + rg.py:132-163 compute_residuals in one pass (same neighbour set, same
//                 centroid): covariance of the k nearest points (the point itself included, as kd_tree.query includes
//                 it), eigenvector of the smallest eigenvalue, flipped when dot(normal, p - centroid) > 0 (:120-121),
//                 normalised (:126); residual |dot(normal, p - centroid)| (:161).  All fp64.
//   gsx_knn       rg.py:205 kd_tree.query(points[seed], k)[1]: the k nearest in ascending distance.
//
// Distances are fp64 of the widened float32 coordinates, (dx*dx + dy*dy) + dz*dz without FMA (this file is compiled
// with -ffp-contract=off), so that a host model evaluating the same expression agrees bit for bit.  Order: nearer
// first, then lower index - the composite key (bits of d2, index) is unique per point, which makes every selection
// below deterministic even among duplicated positions.
//
// Search structure: a uniform grid over the robust bounding box (0.5 % .. 99.5 % per axis; what lies outside is
// clamped into the border cells, which therefore reach to infinity).  The host bins the points with a counting sort
// (O(n), cells in x-fastest order, index order kept inside a cell) and uploads float4 (x, y, z, original index).
// ONE WAVE PER QUERY, queries in cell order so that the four waves of a workgroup walk the same cells:
//   1. ring: the cube of cells [c - r, c + r]^3 is widened until the sphere inscribed in it (radius = distance from the
//      query to the nearest cube face that is not a grid border, less a margin for the rounding of the cell
//      assignment) holds >= k points: every point outside the cube is then farther than the k-th neighbour.
//   2. select: radix select over the composite key, 8 bits per pass, most significant first, a 256-counter LDS
//      histogram per wave (lanes that share a digit with the wave's first lane add once).  A pass ends the
//      selection as soon as the chosen bucket is needed whole, which with distinct distances happens after the
//      bucket has thinned out to one point: 5 - 6 passes instead of 12.
//   3. gsx_normals: one more pass adds up the moments of (p_j - p_i) over the points at or below the threshold (shifted
//      by the query, so S2 - k m m^T does not cancel), a wave reduction, and lane 0 solves the 3x3 symmetric
//      eigenproblem by cyclic Jacobi.  No neighbour list is ever stored.
//      gsx_knn (k <= 64): the k points at or below the threshold go to LDS and are ranked by their keys.
// A row of cells along x is one contiguous range of the sorted points, so a cube is (2r+1)^2 coalesced ranges.
// With a 1 x 1 x 1 grid (option "nn_brute") the same kernels visit every point for every query: the brute-force
// search the grid is tested against (the same lists bit for bit; the moments are added up in another order).
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

__global__ void nn_finite_kernel(const float* __restrict__ p, long long n3, int* __restrict__ flag) {
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

// steps 1 and 2 of the header comment for the query (qx, qy, qz); hist: 256 LDS counters of this wave
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

// cyclic Jacobi on the symmetric 3x3 matrix a (upper triangle used); returns the unit eigenvector of the smallest eigenvalue
__device__ inline void nn_smallest_eigvec(double a00, double a01, double a02, double a11, double a12, double a22, double n[3]) {
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 12; ++sweep) {
        // Jacobi converges quadratically: the rotations are repeated until the off-diagonal has underflowed (or is NaN)
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (!(off > 1e-300)) break;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
            for (int i = 0; i < 3; ++i) {  // A <- A J
                const double aip = A[i][p], aiq = A[i][q];
                A[i][p] = cs * aip - sn * aiq;
                A[i][q] = sn * aip + cs * aiq;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {  // A <- J^T A
                const double api = A[p][i], aqi = A[q][i];
                A[p][i] = cs * api - sn * aqi;
                A[q][i] = sn * api + cs * aqi;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double vip = V[i][p], viq = V[i][q];
                V[i][p] = cs * vip - sn * viq;
                V[i][q] = sn * vip + cs * viq;
            }
        }
    }
    // column of the smallest eigenvalue (the first among equals), by selects: no run-time index, no scratch
    double lmin = A[0][0], x = V[0][0], y = V[1][0], z = V[2][0];
    if (A[1][1] < lmin) {
        lmin = A[1][1]; x = V[0][1]; y = V[1][1]; z = V[2][1];
    }
    if (A[2][2] < lmin) {
        lmin = A[2][2]; x = V[0][2]; y = V[1][2]; z = V[2][2];
    }
    const double len = sqrt(x * x + y * y + z * z);
    if (!(len > 0.0) || !isfinite(len)) {  // never NaN: an undefined normal is still a unit vector
        x = 0.0; y = 0.0; z = 1.0;
    } else {
        x /= len; y /= len; z /= len;
    }
    n[0] = x; n[1] = y; n[2] = z;
}

// kMoments: the test hook's instantiation also writes centroid and covariance; the product one carries no such code
template <bool kMoments>
__global__ __launch_bounds__(kNnBlock) void nn_normals_kernel(NnGrid G, const uint32_t* __restrict__ cs, const float4* __restrict__ pts,
                                                              long long n, unsigned k, double* __restrict__ normals,
                                                              double* __restrict__ residuals, double* __restrict__ moments) {
    __shared__ unsigned hist_all[kNnWaves][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * kNnWaves + wave;
    if (q >= n) return;  // wave-uniform; no workgroup barrier below
    const float4 me = pts[q];
    const double qx = me.x, qy = me.y, qz = me.z;
    const NnThreshold T = nn_threshold(G, cs, pts, qx, qy, qz, k, lane, hist_all[wave]);
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0, s8 = 0;
    nn_visit(G, cs, pts, T.cube, lane, [&](const float4& p, bool act) {
        double dx, dy, dz;
        const double d2 = nn_d2(p, qx, qy, qz, dx, dy, dz);
        if (act && nn_selected(T, d2, __float_as_uint(p.w))) {
            s0 += dx; s1 += dy; s2 += dz;
            s3 += dx * dx; s4 += dx * dy; s5 += dx * dz;
            s6 += dy * dy; s7 += dy * dz; s8 += dz * dz;
        }
    });
    const double s[9] = {wave_sum_f64(s0), wave_sum_f64(s1), wave_sum_f64(s2), wave_sum_f64(s3), wave_sum_f64(s4),
                         wave_sum_f64(s5), wave_sum_f64(s6), wave_sum_f64(s7), wave_sum_f64(s8)};
    if (lane == 0) {
        const double kd = (double)k;
        const double mx = s[0] / kd, my = s[1] / kd, mz = s[2] / kd;  // centroid - p
        double nv[3];
        nn_smallest_eigvec(s[3] - kd * mx * mx, s[4] - kd * mx * my, s[5] - kd * mx * mz, s[6] - kd * my * my, s[7] - kd * my * mz,
                           s[8] - kd * mz * mz, nv);
        double dot = -(nv[0] * mx + nv[1] * my + nv[2] * mz);  // dot(normal, p - centroid)
        if (dot > 0.0) {                                        // rg.py:120-121
            nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2];
            dot = -dot;
        }
        const size_t o = (size_t)__float_as_uint(me.w);
        if (kMoments) {  // test hook: centroid and the upper triangle of the covariance the normal was taken from
            double* mo = moments + o * 9;
            mo[0] = qx + mx; mo[1] = qy + my; mo[2] = qz + mz;
            mo[3] = s[3] - kd * mx * mx; mo[4] = s[4] - kd * mx * my; mo[5] = s[5] - kd * mx * mz;
            mo[6] = s[6] - kd * my * my; mo[7] = s[7] - kd * my * mz; mo[8] = s[8] - kd * mz * mz;
        }
        if (normals) {
            normals[o * 3 + 0] = nv[0];
            normals[o * 3 + 1] = nv[1];
            normals[o * 3 + 2] = nv[2];
        }
        if (residuals) residuals[o] = fabs(dot);  // rg.py:161
    }
}

__global__ __launch_bounds__(kNnBlock) void nn_knn_kernel(NnGrid G, const uint32_t* __restrict__ cs, const float4* __restrict__ pts,
                                                          long long n, unsigned k, int32_t* __restrict__ index) {
    __shared__ unsigned hist_all[kNnWaves][256];
    __shared__ unsigned long long keys_all[kNnWaves][64];
    __shared__ uint32_t idx_all[kNnWaves][64];
    __shared__ unsigned fill_all[kNnWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * kNnWaves + wave;
    if (q >= n) return;
    const float4 me = pts[q];
    const double qx = me.x, qy = me.y, qz = me.z;
    const NnThreshold T = nn_threshold(G, cs, pts, qx, qy, qz, k, lane, hist_all[wave]);
    unsigned long long* keys = keys_all[wave];
    uint32_t* idx = idx_all[wave];
    if (lane == 0) fill_all[wave] = 0;
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    nn_visit(G, cs, pts, T.cube, lane, [&](const float4& p, bool act) {
        double dx, dy, dz;
        const double d2 = nn_d2(p, qx, qy, qz, dx, dy, dz);
        const uint32_t id = __float_as_uint(p.w);
        if (act && nn_selected(T, d2, id)) {
            const unsigned slot = atomicAdd(&fill_all[wave], 1u);
            if (slot < 64) {  // exactly k <= 64 points are selected: the keys are unique
                keys[slot] = (unsigned long long)__double_as_longlong(d2);
                idx[slot] = id;
            }
        }
    });
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    if ((unsigned)lane < k) {
        const unsigned long long mk = keys[lane];
        const uint32_t mi = idx[lane];
        unsigned rank = 0;
        for (unsigned j = 0; j < k; ++j) rank += (keys[j] < mk || (keys[j] == mk && idx[j] < mi)) ? 1u : 0u;
        index[(size_t)__float_as_uint(me.w) * k + rank] = (int32_t)mi;
    }
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

int normals(Ctx* c, int64_t n, const float* points, int64_t k, double* normals_out, double* residuals_out, double* moments_out,
            bool checked) {
    if (!points || n < 1) return fail(c, GSX_E_INVALID, "normals: points is NULL or n < 1");
    if (k < 3 || k > n) return fail(c, GSX_E_INVALID, "normals: k must be in [3, n]");
    if (n > ((int64_t)1 << 31) - 1) return fail(c, GSX_E_UNSUPPORTED, "normals: n > 2^31-1");
    NnScene S;
    int rc = nn_prepare(c, "normals", n, points, k, S, checked);
    if (rc) return rc;
    const size_t nn = (size_t)n;
    GSX_HIP(c, c->nn_out.ensure(sizeof(double) * nn * (moments_out ? 13 : 4)));  // normals 3n | residuals n | moments 9n
    double* dn = c->nn_out.as<double>();
    double* dr = dn + 3 * nn;
    double* dm = moments_out ? dr + nn : nullptr;
    {
        ProfScope ps(c, "nn_normals");
        hipLaunchKernelGGL(moments_out ? nn_normals_kernel<true> : nn_normals_kernel<false>, dim3((unsigned)((n + kNnWaves - 1) / kNnWaves)),
                           dim3(kNnBlock), 0, c->stream, S.G,
                           c->nn_cs.as<uint32_t>(), c->nn_pts.as<float4>(), (long long)n, (unsigned)k, normals_out ? dn : nullptr,
                           residuals_out ? dr : nullptr, dm);
        GSX_HIP(c, hipGetLastError());
    }
    if (normals_out) GSX_HIP(c, hipMemcpyAsync(normals_out, dn, sizeof(double) * 3 * nn, hipMemcpyDeviceToHost, c->stream));
    if (residuals_out) GSX_HIP(c, hipMemcpyAsync(residuals_out, dr, sizeof(double) * nn, hipMemcpyDeviceToHost, c->stream));
    if (moments_out) GSX_HIP(c, hipMemcpyAsync(moments_out, dm, sizeof(double) * 9 * nn, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

int knn(Ctx* c, int64_t n, const float* points, int k, int32_t* index_out, bool checked) {
    if (!points || n < 1) return fail(c, GSX_E_INVALID, "knn: points is NULL or n < 1");
    if (k < 2 || k > 64 || k > n) return fail(c, GSX_E_INVALID, "knn: k must be in [2, min(64, n)]");
    if (n > ((int64_t)1 << 31) - 1) return fail(c, GSX_E_UNSUPPORTED, "knn: n > 2^31-1");
    c->nn_index_rows = 0;
    NnScene S;
    int rc = nn_prepare(c, "knn", n, points, k, S, checked);
    if (rc) return rc;
    GSX_HIP(c, c->nn_index.ensure(sizeof(int32_t) * (size_t)n * k));
    {
        ProfScope ps(c, "nn_knn");
        hipLaunchKernelGGL(nn_knn_kernel, dim3((unsigned)((n + kNnWaves - 1) / kNnWaves)), dim3(kNnBlock), 0, c->stream, S.G,
                           c->nn_cs.as<uint32_t>(), c->nn_pts.as<float4>(), (long long)n, (unsigned)k, c->nn_index.as<int32_t>());
        GSX_HIP(c, hipGetLastError());
    }
    if (index_out) GSX_HIP(c, hipMemcpyAsync(index_out, c->nn_index.p, sizeof(int32_t) * (size_t)n * k, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    c->nn_index_rows = n;
    return GSX_OK;
}

int region_growing(Ctx* c, int64_t n, const float* points, int64_t k_normals, int k, double residual_threshold, double angle_threshold,
                   int32_t* labels_out, double* normals_out, double* residuals_out, int32_t* n_regions_out) {
    if (!labels_out) return fail(c, GSX_E_INVALID, "region_growing: labels_out is NULL");
    if (n < 1) return fail(c, GSX_E_INVALID, "region_growing: n < 1");
    std::vector<double> nv, rv;
    if (!normals_out) {
        nv.resize((size_t)n * 3);
        normals_out = nv.data();
    }
    if (!residuals_out) {
        rv.resize((size_t)n);
        residuals_out = rv.data();
    }
    int rc = normals(c, n, points, k_normals, normals_out, residuals_out, nullptr, false);
    if (rc) return rc;
    std::vector<int32_t> nb((size_t)n * (size_t)std::max(k, 1));
    rc = knn(c, n, points, k, nb.data(), true);  // the same points: checked and found finite a moment ago
    if (rc) return rc;
    rc = gsx_region_grow(n, normals_out, residuals_out, nb.data(), k, residual_threshold, angle_threshold, labels_out, n_regions_out);
    if (rc) return fail(c, rc, "region_growing: %s", gsx_last_error(nullptr));
    return GSX_OK;
}

int debug_nn_grid(int64_t n, const float* points, int64_t k, int brute, double* origin_out, double* h_out, int32_t* dims_out,
                  uint32_t* cell_start_out, int32_t* order_out) {
    if (!points || n < 1 || k < 1) return fail(nullptr, GSX_E_INVALID, "debug_nn_grid: points is NULL, n < 1 or k < 1");
    if (n > ((int64_t)1 << 31) - 1) return fail(nullptr, GSX_E_UNSUPPORTED, "debug_nn_grid: n > 2^31-1");
    if (!origin_out || !h_out || !dims_out) return fail(nullptr, GSX_E_INVALID, "debug_nn_grid: origin_out, h_out or dims_out is NULL");
    for (int64_t i = 0; i < 3 * n; ++i)  // the product finds these on the device (nn_finite_kernel)
        if (!std::isfinite(points[i])) return fail(nullptr, GSX_E_INVALID, "debug_nn_grid: a coordinate is not finite");
    NnGrid G;
    std::vector<uint32_t> start;
    std::vector<float4> sorted;
    nn_grid_sort(n, points, k, brute != 0, G, start, sorted);
    for (int a = 0; a < 3; ++a) {
        origin_out[a] = G.o[a];
        dims_out[a] = G.g[a];
    }
    *h_out = G.h;
    if (cell_start_out) std::memcpy(cell_start_out, start.data(), sizeof(uint32_t) * start.size());
    if (order_out)
        for (int64_t j = 0; j < n; ++j) {
            uint32_t u;
            std::memcpy(&u, &sorted[(size_t)j].w, 4);
            order_out[j] = (int32_t)u;
        }
    return GSX_OK;
}

}  // namespace gsx
