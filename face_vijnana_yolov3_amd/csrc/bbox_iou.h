// bbox_iou of the accuracy metrics (reference yd.py:165-194) on float64 corners, shared by bbox_iou_pairs_kernel (postproc.hip)
// and the matching kernel of det_metric.hip: the reference's branch structure and operation order, every operation one IEEE
// double operation (the library is built with -ffp-contract=off), so the result is bit-identical to the Python floats.  A zero
// union gives nan (0/0) or +-inf, as NumPy's division does.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double interval_overlap_f64(double x1, double x2, double x3, double x4) {
    if (x3 < x1) {
        if (x4 < x1) return 0.0;
        return fmin(x2, x4) - x1;
    } else {
        if (x2 < x3) return 0.0;
        return fmin(x2, x4) - x3;
    }
}

__device__ __forceinline__ double bbox_iou_f64(double ax0, double ay0, double ax1, double ay1, double bx0, double by0, double bx1,
                                               double by1) {
    const double iw = interval_overlap_f64(ax0, ax1, bx0, bx1), ih = interval_overlap_f64(ay0, ay1, by0, by1);
    const double inter = iw * ih;
    const double uni = (ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0) - inter;
    return inter / uni;
}
