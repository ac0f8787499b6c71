/* The three-scale head's selection step on the device: the candidate list fv_yolo_decode_nms_batch leaves per image becomes the
 * layout fv_decode_nms leaves (boxes [n][K][4], score [n][K], count [n]), which fv_det_rows_from_nms and the pinned-copy code of
 * the single-scale path read (yolo_select.hip).  Part of the C ABI of libfv_hotpath; the declaration moves
 * into include/fv_hotpath.h together with its row in the stream-order table (DESIGN.md section 30 says why such declarations are
 * not there yet).  Additive: fv_abi_version() is unchanged. */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/fv_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FV_YOLO_SELECT_MAX_K 512          /* fv_decode_nms' num_cands bound */
#define FV_YOLO_SELECT_MAX_CAPACITY 8192  /* fv_yolo_decode_nms_batch's capacity bound: the keys of one image are sorted in LDS */

/* boxes [nimg][capacity][4] int32, objness [nimg][capacity] float32, classes [nimg][capacity][nclass] float32 (suppressed entries
 * zeroed), count [nimg] int32: what fv_yolo_decode_nms_batch left for nimg images.  The tail of the reference's detect()
 * (BoundBox.get_score() > 0, ascending stable argsort, the first num_cands) per image:
 *
 * Image b has n = clamp(count[b], 0, capacity) rows.  Row r < n has score = min(m, 1.0f), m the value of the row's arg-max class as
 * np.argmax finds it: the maximum, and NaN when any class of the row is a NaN (the first NaN wins there).  A row is kept when
 * score > 0: a NaN is not, +0.0 and -0.0 are not, a positive denormal is (the comparison is made on the bit pattern and does not
 * depend on the denormal mode).  The kept rows are ordered by ascending score, equal scores by the smaller r (np.argsort,
 * kind='stable'); the first min(kept, num_cands) of them are the result, in that order:
 *   out_boxes [nimg][num_cands][4] int32 and out_obj [nimg][num_cands] float32: the row's box and objectness, copied;
 *   out_src [nimg][num_cands] int32: r, the row's index in the candidate list;  out_score [nimg][num_cands] float32: the capped
 *   score;  out_classes [nimg][num_cands][nclass] float32: the row's classes, copied (may be NULL: not written);
 *   out_count [nimg] int32: their number.
 * Slots past out_count[b] are -1 (boxes, src) and 0 (floats), as fv_decode_nms fills them.
 *
 * An image with count[b] >= refuse_at gets out_count[b] = -1, its slots filled like unused slots, and none of its rows is read;
 * the other images are served.  Callers pass refuse_at = capacity where capacity is smaller than the grid's slot count (the list
 * may have been cut short) and INT_MAX otherwise.
 *
 * One workgroup per image; every output value is a copy of an input or a minimum with 1; no float atomics; nothing waits for the
 * stream.  FV_ERR_INVALID with nothing enqueued and the outputs untouched for: nimg < 1, capacity outside
 * 1..FV_YOLO_SELECT_MAX_CAPACITY, nclass < 1 (or beyond INT_MAX / FV_YOLO_SELECT_MAX_K), num_cands outside
 * 1..FV_YOLO_SELECT_MAX_K, refuse_at < 1, a NULL pointer other than out_classes. */
int fv_yolo_select_cands(fv_ctx* ctx, const int32_t* boxes, const float* objness, const float* classes, const int32_t* count, int nimg,
                         int capacity, int nclass, int refuse_at, int num_cands, int32_t* out_boxes, int32_t* out_src, float* out_obj,
                         float* out_score, float* out_classes, int32_t* out_count);

#ifdef __cplusplus
}
#endif
