/* Tiled (sliced) inference, the step in the middle: every tile view's detections projected into frame coordinates and one
 * cross-tile greedy NMS per frame, on the device (tile_merge.hip).  Part of the C ABI of libfv_hotpath;
 * the two declarations move into include/fv_hotpath.h together with their row in the stream-order table (DESIGN.md says why
 * they are not there yet).  Additive: fv_abi_version() is unchanged. */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/fv_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FV_TILE_MAX_CANDS 4096 /* candidates per frame the merge kernel ranks in LDS */
#define FV_TILE_MAX_K 512      /* slots per view (fv_decode_nms' num_cands bound) */
#define FV_TILE_METRIC_IOS 0   /* intersection over the smaller area */
#define FV_TILE_METRIC_IOU 1   /* bbox_iou */

/* Bytes of device workspace fv_tile_merge needs for n_frames frames (0 for n_frames < 1). */
size_t fv_tile_merge_workspace_bytes(int n_frames);

/* boxes [n_views][num_cands][4] int32, score [n_views][num_cands] float32, count [n_views] int32: what fv_decode_nms left for
 * n_views letterboxed views (network pixels at image_size).  tiles [n_views][5] int32 = (frame, y0, x0, th, tw): the source
 * rectangle of each view in its frame.  frame_off [n_frames + 1] int32: frame f owns the views frame_off[f] .. frame_off[f + 1].
 *
 * A candidate is slot k < clamp(count[t], 0, num_cands) of view t with score > 0 (a NaN is not).  Its frame box is the network box
 * put through FaceDetector._project_back's float64 operations in their order (both w >= h branches) for (h, w) = (th, tw) and the
 * padding of letterbox_geometry(th, tw, image_size), then x0 added to the x values and y0 to the y values.  The candidates of a
 * frame are ranked by descending float32 score, equal scores by the smaller view, then the smaller slot.  Walking the ranking, a
 * candidate still alive is kept and kills every later candidate whose overlap with it is >= merge_th (a NaN never is, +inf is):
 * bbox_iou for FV_TILE_METRIC_IOU, inter / fmin(area_kept, area_later) for FV_TILE_METRIC_IOS.  The first FV_DET_ROWS kept
 * candidates are the result, in that order:
 *   corners [n_frames][FV_DET_ROWS][4] float64 xmin, ymin, xmax, ymax;  rows [n_frames][FV_DET_ROWS][5] float64 x, y,
 *   w = xmax - xmin, h = ymax - ymin, conf = (double)min(score, 1) (what fv_det_match_rows reads);  nrows [n_frames] int32;
 *   src [n_frames][FV_DET_ROWS] int32 = view * num_cands + slot.  Slots past nrows[f] are zeros (src: -1).
 * A frame whose view range is not inside [0, n_views] or that holds more than FV_TILE_MAX_CANDS candidates gets nrows = -1, zeros
 * everywhere else, and none of its boxes is read.
 *
 * One workgroup per frame; every operation on a coordinate is a single IEEE double operation; no float atomics; nothing waits for
 * the stream.  workspace: device memory of at least fv_tile_merge_workspace_bytes(n_frames) bytes, 8-byte aligned; its contents
 * on entry are ignored.  FV_ERR_INVALID with nothing enqueued for: n_views, n_frames or num_cands < 1, num_cands > FV_TILE_MAX_K,
 * n_views * num_cands beyond int32, image_size < 1, a metric other than the two, merge_th outside (0, 1], a NULL pointer, a
 * workspace that is too small or misaligned. */
int fv_tile_merge(fv_ctx* ctx, const int32_t* boxes, const float* score, const int32_t* count, const int32_t* tiles,
                  const int32_t* frame_off, int n_views, int n_frames, int num_cands, int image_size, int metric, double merge_th,
                  void* workspace, size_t workspace_bytes, double* corners, double* rows, int32_t* nrows, int32_t* src);

#ifdef __cplusplus
}
#endif
