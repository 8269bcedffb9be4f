// Host-only part of the IoU evaluation (the reference's Image_Segmentation/evaluation.py, "ev.py"): the quotient of ev.py:35 and
// the best-match rule of ev.py:44-54.  No ctx, no GPU; errors go to gsx_last_error(NULL).
#include <cstdint>

#include "../../include/gsx.h"

namespace gsx {
void set_global_error(const char* fmt, ...);
}

extern "C" {

// np.sum(intersection) / np.sum(union) (ev.py:35): two int64 sums, numpy's true division = one IEEE double division of the
// converted operands; union = |a| + |b| - |a & b|.  0 / 0 is NaN, as in the reference (which also warns).
int gsx_iou_from_counts(int64_t n, const int64_t* inter, const int64_t* area_a, const int64_t* area_b, double* iou_out) {
    if (n < 0 || (n > 0 && (!inter || !area_a || !area_b || !iou_out))) {
        gsx::set_global_error("iou_from_counts: NULL argument or negative n");
        return GSX_E_INVALID;
    }
    for (int64_t i = 0; i < n; ++i) {
        const double num = (double)inter[i];
        const double den = (double)(area_a[i] + area_b[i] - inter[i]);
        iou_out[i] = num / den;
    }
    return GSX_OK;
}

// ev.py:44-54 per mask: max_iou = 0, gt_idx = 0; a ground truth takes over only if iou > max_iou - so the first of equal maxima
// wins, NaN never wins, and a mask without a positive IoU reports (0, 0).
int gsx_iou_best(int32_t n_masks, int32_t n_gt, const double* iou, double* best_iou_out, int32_t* best_gt_out) {
    if (n_masks < 0 || n_gt < 0 || (n_masks > 0 && (!best_iou_out || !best_gt_out)) || (n_masks > 0 && n_gt > 0 && !iou)) {
        gsx::set_global_error("iou_best: NULL argument or negative size");
        return GSX_E_INVALID;
    }
    for (int32_t m = 0; m < n_masks; ++m) {
        double best = 0.0;
        int32_t idx = 0;
        for (int32_t g = 0; g < n_gt; ++g) {
            const double v = iou[(int64_t)m * n_gt + g];
            if (v > best) {
                best = v;
                idx = g;
            }
        }
        best_iou_out[m] = best;
        best_gt_out[m] = idx;
    }
    return GSX_OK;
}

}  // extern "C"
