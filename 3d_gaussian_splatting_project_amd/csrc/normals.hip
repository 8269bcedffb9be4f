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
// Steps 1 and 2, the visit and the host side of the grid live in nn_device.hpp, which smooth.hip shares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "gsx_ctx.hpp"
#include "nn_device.hpp"

namespace gsx {

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

// the lists of gsx_knn into the context's nn_index, 1 <= k <= min(64, n) (the caller has checked the arguments); also what
// smooth.hip's list form runs on
int knn_lists(Ctx* c, const char* who, int64_t n, const float* points, int k, int32_t* index_out, bool checked) {
    c->nn_index_rows = 0;
    NnScene S;
    int rc = nn_prepare(c, who, n, points, k, S, checked);
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
    c->nn_index_k = k;
    return GSX_OK;
}

int knn(Ctx* c, int64_t n, const float* points, int k, int32_t* index_out, bool checked) {
    if (!points || n < 1) return fail(c, GSX_E_INVALID, "knn: points is NULL or n < 1");
    if (k < 2 || k > 64 || k > n) return fail(c, GSX_E_INVALID, "knn: k must be in [2, min(64, n)]");
    if (n > ((int64_t)1 << 31) - 1) return fail(c, GSX_E_UNSUPPORTED, "knn: n > 2^31-1");
    return knn_lists(c, "knn", n, points, k, index_out, checked);
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
