// YOLOv3 detection loss of the three-scale head (yolo_det_loss.hip): launcher shared by the operator
// fv_yolo_det_loss_grad and the training step fv_yolov3_train_step_det.
#pragma once
#include "../../include/fv_hotpath.h"
#include "common.h"

// argument checks of both entry points (FV_ERR_INVALID with a message, nothing launched)
int fv_det_check(fv_ctx* ctx, const char* who, const fv_yolo_det_conf* conf, int batch, int image_size, int ncls, int c_pad,
                 const void* scratch, size_t scratch_bytes, const double* stats);
// gather + loss + finish on ctx->stream.  y_s dense [B g_s^2][3*(5+ncls)], t_s likewise, dy_s [B g_s^2][c_pad]; arguments checked
// by the caller (fv_det_check)
int fv_det_loss_launch(fv_ctx* ctx, const float* const* y3, const float* const* t3, int batch, int image_size, int ncls, int c_pad,
                       const fv_yolo_det_conf* conf, double loss_weight, void* scratch, float* loss, float* const* dy3, double* stats);
