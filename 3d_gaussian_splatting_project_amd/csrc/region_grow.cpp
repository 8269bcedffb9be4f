// region_grow.cpp - smoothness-constrained region growing, 3D_clustering/region_growing.py:166-226 segmentation_3D, on
// the host.  The algorithm is sequential by definition: a point belongs to the first region whose front reaches it
// and is tested against the normal of the seed that reached it.  Needs no context and no GPU.
//
//   next region   the available point of smallest residual (:194), lowest index among equals: one presorted order
//                 walked once instead of the reference's O(n) scan per region
//   front         FIFO (:199-203); neighbours in list order; accept iff |dot(normal[seed], normal[nb])| >
//                 cos(angle_threshold) (:209-211); an accepted neighbour joins the front iff its residual <
//                 residual_threshold (:216-218)
//   labels        rank of the point's region by size, largest first, creation order among equals (:224)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/gsx.h"

namespace gsx {
void set_global_error(const char* fmt, ...);
}

extern "C" int gsx_region_grow(int64_t n, const double* normals, const double* residuals, const int32_t* knn, int32_t k,
                               double residual_threshold, double angle_threshold, int32_t* labels_out, int32_t* n_regions_out) {
    if (n < 1 || !normals || !residuals || !knn || !labels_out) {
        gsx::set_global_error("region_grow: NULL argument or n < 1");
        return GSX_E_INVALID;
    }
    if (k < 1 || n > INT32_MAX) {
        gsx::set_global_error("region_grow: k < 1 or n > 2^31-1");
        return GSX_E_INVALID;
    }
    if (std::isnan(residual_threshold) || std::isnan(angle_threshold)) {
        gsx::set_global_error("region_grow: a threshold is NaN");
        return GSX_E_INVALID;
    }
    try {
        for (int64_t i = 0; i < n; ++i)
            if (std::isnan(residuals[i])) {
                gsx::set_global_error("region_grow: residual %lld is NaN", (long long)i);
                return GSX_E_INVALID;
            }
        for (int64_t t = 0; t < n * k; ++t)
            if (knn[t] < 0 || knn[t] >= n) {
                gsx::set_global_error("region_grow: neighbour index %d of point %lld is out of range", (int)knn[t], (long long)(t / k));
                return GSX_E_INVALID;
            }
        std::vector<int32_t> order((size_t)n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return residuals[a] < residuals[b]; });
        const double cos_thr = std::cos(angle_threshold);
        std::vector<int32_t> region((size_t)n, -1), queue, sizes;
        queue.reserve((size_t)n);
        size_t next = 0;
        for (;;) {
            while (next < (size_t)n && region[order[next]] >= 0) ++next;
            if (next == (size_t)n) break;
            const int32_t id = (int32_t)sizes.size();
            int32_t size = 1;
            queue.clear();
            queue.push_back(order[next]);
            region[order[next]] = id;
            for (size_t head = 0; head < queue.size(); ++head) {
                const int32_t seed = queue[head];
                const double* ns = normals + (size_t)seed * 3;
                const int32_t* nb = knn + (size_t)seed * k;
                for (int32_t j = 0; j < k; ++j) {
                    const int32_t v = nb[j];
                    if (region[v] >= 0) continue;
                    const double* nv = normals + (size_t)v * 3;
                    const double cos_angle = std::fabs(ns[0] * nv[0] + ns[1] * nv[1] + ns[2] * nv[2]);
                    if (cos_angle > cos_thr) {
                        region[v] = id;
                        ++size;
                        if (residuals[v] < residual_threshold) queue.push_back(v);
                    }
                }
            }
            sizes.push_back(size);
        }
        std::vector<int32_t> by_size(sizes.size()), rank(sizes.size());
        std::iota(by_size.begin(), by_size.end(), 0);
        std::stable_sort(by_size.begin(), by_size.end(), [&](int32_t a, int32_t b) { return sizes[a] > sizes[b]; });
        for (size_t r = 0; r < by_size.size(); ++r) rank[by_size[r]] = (int32_t)r;
        for (int64_t i = 0; i < n; ++i) labels_out[i] = rank[region[i]];
        if (n_regions_out) *n_regions_out = (int32_t)sizes.size();
        return GSX_OK;
    } catch (...) {
        gsx::set_global_error("region_grow: out of host memory");
        return GSX_E_INVALID;
    }
}
