/*
 * fv_hotpath.h -- C ABI of the MI355X-native FaceDetector hot path.
 *
 * The reference (tonandr/face_vijnana_yolov3) is pure Python on Keras/TensorFlow and exposes
 * no C ABI of its own; the seam this library sits behind is the handful of Keras `Model`
 * methods and NumPy helpers that `FaceDetector` calls.  Every entry point below names the
 * reference interface it replaces (paths relative to /root/reference/src/space; fd.py =
 * face_detection.py, yd.py = yolov3_detect.py).  A ctypes binding is shown in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error; fv_last_error(ctx) returns a message
 *    owned by the context (fv_last_error(NULL): message of the last failed fv_create).
 *  - the CALLER owns all device memory (plain pointers + explicit sizes; in this project
 *    torch-ROCm tensors provide the storage).  The library allocates nothing persistent.
 *  - one context per GPU / rank / host thread; all work is enqueued on the context's HIP
 *    stream and is asynchronous with respect to the host unless stated otherwise.
 *  - activations are NHWC float32; conv kernels inside the flat parameter vector are stored
 *    OHWI ([cout][kh][kw][cin]); see fv_layer_desc for offsets.
 */
#ifndef FV_HOTPATH_H
#define FV_HOTPATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fv_ctx fv_ctx;

#define FV_OK 0
#define FV_ERR_INVALID (-1)   /* bad argument / unsupported shape */
#define FV_ERR_HIP (-2)       /* a HIP runtime call failed */
#define FV_ERR_WORKSPACE (-3) /* caller workspace too small */

/* ------------------------------------------------------------------ context */
int fv_abi_version(void);
/* stream: a hipStream_t (may be NULL = default stream).  Replaces the implicit TF session
 * that Keras creates behind FaceDetector.__init__ (fd.py:312-382). */
int fv_create(int device, void* stream, fv_ctx** out);
/* (The context owns a low-priority side stream for the backward overlap.  The HIP runtime multiplexes a process's streams onto
 * a fixed number of hardware queues, 4 by default: a context created AFTER an RCCL communicator has existed in the process can find
 * its side stream sharing a hardware queue with the compute stream, which serialises the overlap -- 30 - 40 % on a training step.
 * Create contexts before communicators.
 * DESIGN 6.) */
void fv_destroy(fv_ctx* ctx);
const char* fv_last_error(const fv_ctx* ctx);
/* Rebinds the context to another hipStream_t (NULL = the default stream); a host setter, nothing is enqueued.  The stream
 * contract: every launch, memset and table upload of the calls that follow goes to this stream in call order, so an entry point
 * reads its inputs and writes its outputs in stream order; the only calls that wait for the host are fv_fid_pair_dists,
 * fv_fid_mine_negatives and fv_profile_collect.  Work already enqueued stays where it is: the caller orders the old stream and the
 * new one itself, and zero-fills what a call accumulates into (dw, statistics slots) on the stream the context is bound to.
 * tests/test_stream_order_gpu.py runs every entry point on a delayed non-default stream. */
int fv_set_stream(fv_ctx* ctx, void* stream);
/* Where fv_bucket_fn fires.  Default (0): after the context's stream has been made to wait for the range's weight-gradient --
 * work the callback enqueues on the context's stream sees the finished range.  on = 1 (with the overlap on): as soon as the
 * range's weight-gradient kernels are in the SIDE stream's queue -- the callback must enqueue its work (the all-reduce of the
 * bucket) on fv_side_stream(ctx), where it is ordered behind them and runs beside the data-gradient chain without an event
 * between the context's stream and the communication.  Before fv_train_step returns, the context's stream has been made to wait
 * for every weight-gradient kernel on the side stream (the event is recorded before the callback fires); what the callback itself
 * enqueued on the side stream is NOT joined by the library: the caller joins it (once, before fv_adam_step). */
int fv_set_bucket_on_side(fv_ctx* ctx, int on);
void* fv_side_stream(fv_ctx* ctx);   /* the hipStream_t of the internal side stream */
/* Update rule of the BatchNormalization moving mean / variance in every training-mode BN launch that follows (reference
 * yd.py:212 `BatchNormalization(epsilon=0.001)`; the update itself is third-party: Keras 2.2.4 `K.moving_average_update` ->
 * TF 1.x `assign_moving_average(..., zero_debias=True)`).  step = 0 (default): plain EMA, moving <- m moving + (1 - m) batch.
 * step = t >= 1: the t-th zero-debiased update since the model was built, moving_t = b_t / (1 - m^t) with the zero-initialised
 * b_t = m b_{t-1} + (1 - m) batch_t -- the first update REPLACES the stored value (so loaded Darknet statistics are forgotten
 * at the first training step, as in the reference's stack).  The setting is consumed by the NEXT fv_train_step /
 * fv_yolov3_train_step (which resets it to 0 when it returns) or by the per-operator fv_bn_finalize / fv_bn_act_slots calls that
 * follow; the caller sets t before every training step.  Parity unpinned (neither Keras nor TF is importable here). */
int fv_set_bn_zero_debias_step(fv_ctx* ctx, long long step);
/* ------------------------------------------------------------------ tuning
 * Schedule / kernel-selection switches with no counterpart in the reference.  None of them changes WHAT is computed: every
 * value gives results that are bit-identical or differ only in fp32 summation order (stated per key); all default to 1 (the
 * fastest measured configuration) and exist for A/B measurements and for the tests that compare the specialised
 * kernels with the generic ones.  key (value != 0 = on):
 *   "overlap"           fv_train_step runs the weight-gradient kernels on an internal side stream, concurrently with the
 *                       data-gradient / BN-backward chain on the context's stream (independent given dz); all side-stream work is
 *                       joined back before a gradient range is reported (fv_bucket_fn) and before the call returns.  0 serialises
 *                       everything on the context's stream.
 *   "tail_split"        when the 128x128 output tiles of a conv launch do not fill whole rounds of the 512 resident workgroup
 *                       slots, the tiles of the last partial round are cut into K slices whose partial tiles a fix-up kernel sums
 *                       in fixed slice order.  Deterministic; changes the summation order of those tiles.
 *   "conv_waves8"       128- / 64-wide conv tiles as 512-thread workgroups (8 waves of 64x32 / 32x32: four waves per SIMD) instead
 *                       of 256 threads (4 waves of 64x64).  Bit-identical.
 *   "conv1x1_persist"   1x1 stride-1 launches with more than 512 tiles (forward and data-gradient of the 1x1 layers at batch >= ~16)
 *                       run as a persistent GEMM whose workgroups walk several tiles with the next tile's operands in flight
 *                       during the epilogue (conv1x1_mfma.hip) instead of one workgroup per tile.  Bit-identical.
 *   "conv_small"        small-M inference (batch 1): a layer whose launch fits one workgroup per CU (<= 256 tiles of 64 x 64, 64 x 32
 *                       or 32 x 32) runs with the K dimension split INSIDE each 512-thread workgroup (four wave pairs or eight waves
 *                       multiply 1/4 or 1/8 of the K steps each, the sums are formed in group order) instead of K slices of one
 *                       workgroup each + a finish launch.  Deterministic; another fp32 summation order.
 *   "conv_bm64"         small-M inference (fewer than 192 tiles of 128 x 128: batch 1): 64-row tiles where they leave fewer padded rows
 *                       than 128-row ones (13x13, 26x26, 52x52 pixels) -- less padding to multiply, fewer K slices to sum.  Changes the
 *                       K-split plan of those launches, i.e. their fp32 summation order.
 *   "conv_halo"         the 3x3 layers with 32 -> 64 channels (conv_1, conv_3): training forward and stride-2 data-gradient from
 *                       an LDS halo tile with resident weights (conv9_mfma.hip, dgrad9s2_mfma.hip).  z / dx bit-identical, the
 *                       statistics are the same sums in another (fp64) order.
 *   "conv0_direct"      first layer (3 -> 32 channels) as a direct vector-FMA kernel when W % 32 == 0 and H % 8 == 0 instead of
 *                       the matrix-core gather kernel.  Bit-identical.
 *   "early_bn_fused"    the BN passes of the first layers folded into their halo-kernel consumers: conv_1 / conv_3 (forward and
 *                       weight-gradient) read z(0) / z(2) and apply scale/shift + LeakyReLU while staging, so a(0) / a(2) are not
 *                       written; the first layer's weight-gradient forms dz(0) from g(0) and z(0) while staging, so dz(0) is not
 *                       written either.  Needs "conv_halo" / "wgrad_fused_taps" (otherwise the passes run as before).  Same bits
 *                       per element; d-beta / d-gamma of layer 0 are made on the side stream.  0 off, 1 on; for A/B runs of one
 *                       part an even value selects parts: 2 forward on load, 4 weight-gradient on load, 8 dz(0), or their sums.
 *   "bn_in_1x1"         the normalise pass (BN + LeakyReLU + residual add) of the layer in front of a residual block's first 1x1
 *                       conv runs inside that conv (conv1x1_mfma.hip): the kernel sums the statistics slots, publishes the
 *                       layer's vectors, forms the activation while staging z as its operand and writes it once.  Same bits
 *                       per element as the separate pass.  Needs "conv1x1_persist".  0 off, 1 on for the shape classes that
 *                       measured faster than the two launches, 2 on for every launch the kernel takes.
 *   "wgrad_fused_taps"  weight-gradients of conv_0 / conv_1 / conv_2 / conv_3 from halo tiles / streaming units (wgrad0, wgrad1,
 *                       wgrad9) instead of the generic kernel.  Same products, other float-atomic summation order.
 * Unknown keys return FV_ERR_INVALID.  The environment variable FV_OPTIONS="key=0,key=1" sets initial values at fv_create. */
int fv_set_option(fv_ctx* ctx, const char* key, long long value);
int fv_get_option(fv_ctx* ctx, const char* key, long long* value);
/* The per-operator conv entry points (fv_conv2d_forward / fv_conv2d_dgrad) have no workspace
 * argument; a caller that wants the tail split there lends device scratch here (NULL, 0 = none;
 * 64 MiB covers every Darknet-53 shape at batch 40).  The buffer must stay valid until the calls that
 * use it have completed on the stream.  fv_train_step / fv_forward_infer use their own workspace. */
int fv_set_conv_scratch(fv_ctx* ctx, void* buf, size_t bytes);

/* ------------------------------------------------------------------ per-kernel timing
 * Measurement aid with no counterpart in the reference (it has no profiler hooks):
 * when enabled, every kernel launch of this library is bracketed by a HIP event pair on the
 * context's stream; fv_profile_collect synchronises and returns one aggregate per kernel with
 * the ALGORITHMIC flops / bytes of the launches (what bench.py's `roofline` is computed from).
 * on = 2: the records of the matrix kernels additionally carry the launch's problem shape in the name ("conv_kernel<128,2,4,false>
 * M108160 N256 K1152 r": rows, output channels, taps x input channels; s2 = stride-2 data-gradient, ks = K split, r = fused
 * BN-backward reduction), i.e. one aggregate per kernel AND shape (names are cut at 63 characters). */
typedef struct fv_profile_rec {
    char name[64];
    int64_t launches;
    double ms_total, flops_total, bytes_total;
} fv_profile_rec;
int fv_profile_enable(fv_ctx* ctx, int on);
int fv_profile_collect(fv_ctx* ctx, fv_profile_rec* out, int max_recs, int* n_out);

/* ------------------------------------------------------------------ detect post-processing
 * Replaces the NumPy/Python tail of FaceDetector.detect (fd.py:900-947): float32 sigmoid,
 * threshold, per-cell box decode, do_nms_v2 (yd.py:446-458, IoU yd.py:165-194), score>0
 * filter, ASCENDING argsort and first num_cands.  One workgroup per image.
 *   head   [nimg][grid][grid][6] float32 raw head outputs (device)
 *   boxes  [nimg][num_cands][4] int32 xmin,ymin,xmax,ymax   cell [nimg][num_cands] int32
 *   obj, score [nimg][num_cands] float32                     count [nimg] int32
 * Unused slots are filled with -1 / 0.  grid <= 22 (ncell <= 512), 1 <= num_cands <= 512.
 * Ties between exactly equal scores (undefined in the reference) break toward the lower
 * row-major cell index. */
int fv_decode_nms(fv_ctx* ctx, const float* head, int nimg, int grid, int image_size,
                  double conf_th, double iou_th, int num_cands, int32_t* boxes, int32_t* cell,
                  float* obj, float* score, int32_t* count);


/* Batched bbox_iou (yd.py:183-194) for the accuracy metric cal_mAP_fd (evaluate.py:46-75):
 * boxes_a, boxes_b [npairs][4] float64 xmin,ymin,xmax,ymax (device) -> iou [npairs] float64, bit-identical to
 * the reference's Python-float arithmetic (nan / inf for a zero union, as NumPy division gives). */
int fv_bbox_iou_pairs(fv_ctx* ctx, const double* boxes_a, const double* boxes_b, int64_t npairs, double* iou);

/* ------------------------------------------------------------------ detection metric on the device (FaceDetector.validate)
 * cal_mAP_fd (evaluate.py:27-127) without the csv round trip: DESIGN.md section 28.  Every buffer is on the device unless it says
 * host; no call waits for the stream; no float atomics, so the same inputs give the same bytes whatever the launch geometry.
 *
 * fv_det_rows_from_nms: fv_decode_nms's result -> the rows FaceDetector.evaluate would have written.  boxes [nimg][num_cands][4],
 * score [nimg][num_cands], count [nimg] as fv_decode_nms leaves them; geom [nimg][6] int32 (h, w, pad_t, pad_b, pad_l, pad_r), the
 * letterbox geometry of fv_letterbox_batch.  Image i keeps its first min(count[i], FV_DET_ROWS) detections in that order
 * (_write_rows' boxes[:60]), undoes the letterbox with _project_back's float64 operations in its order (int -> double, subtract,
 * max, multiply, divide, min; both w >= h branches) and writes rows [nimg][FV_DET_ROWS][5] float64 = x, y, w = xmax - xmin,
 * h = ymax - ymin, conf = (double)min(score, 1) -- the doubles float() reads back from the csv fields -- and nrows [nimg].  Rows
 * past nrows[i] are written as zeros. */
#define FV_DET_ROWS 60
#define FV_DET_MAX_GT 4096
#define FV_DET_MAX_TH 16
int fv_det_rows_from_nms(fv_ctx* ctx, const int32_t* boxes, const float* score, const int32_t* count, const int32_t* geom, int nimg,
                         int num_cands, int image_size, double* rows, int32_t* nrows);
/* The greedy assignment of cal_mAP_fd per image (evaluate.py:46-95), one workgroup per image: rows / nrows as above (nrows is
 * clamped to [0, FV_DET_ROWS]); gt [total][4] float64 x, y, w, h and gt_off [nimg + 1] int64, image i's boxes being
 * gt[gt_off[i] .. gt_off[i + 1]).  IoUs are fv_bbox_iou_pairs' on the corners (x, y, x + w, y + h).  Pairs with IoU > 0 are taken
 * in descending IoU order, equal IoUs by the smaller ground-truth index, then the smaller detection index, each box and each
 * detection at most once; nan is never > 0, +inf is.  iou [nimg][FV_DET_ROWS]: a detection's assigned IoU, -1.0 without one (and
 * past nrows); flag [nimg]: 1 when some pair overlapped, 0 when none did (the reference then drops the image's detections).
 * max_gt is the caller's bound on gt_off[i + 1] - gt_off[i]; more than FV_DET_MAX_GT is FV_ERR_INVALID and nothing is enqueued.  An
 * image the device finds outside [0, FV_DET_MAX_GT] all the same gets flag -1 and no box of it is read. */
int fv_det_match_rows(fv_ctx* ctx, const double* rows, const int32_t* nrows, const double* gt, const int64_t* gt_off, int nimg,
                      int max_gt, double* iou, int32_t* flag);
/* Ranking and precision / recall sweep (evaluate.py:104-125) over n_img images' rows, iou and flag as the two calls above leave
 * them.  The detections of images with flag > 0, in image order then row order, are the N (conf, iou) pairs; they are ranked by
 * descending conf, equal confidences by the earlier position (np.argsort(-conf, kind='stable'); conf must not be nan); per
 * threshold t (host, 1 <= n_th <= FV_DET_MAX_TH) tp_k = the inclusive running count of iou >= thresholds[t] along the ranking, and
 *   result[t]            = sum_{k=1}^{N-1} (r_k - r_{k-1}) * (p_k + p_{k-1}) / 2,  p_k = tp_k / (k + 1),  r_k = tp_k / gt_count
 *                          (float64; the exact integral of the linear interpolant the reference hands to quad; 0 for N < 2),
 *   result[n_th + t]     = p_{N-1},   result[2 * n_th + t] = r_{N-1}   (0 for N == 0),
 * n_det [1] int32 = N.  order (may be NULL) [n_img * FV_DET_ROWS] int32 receives the ranking in its first N entries, counts (may be
 * NULL) [n_th][n_img * FV_DET_ROWS] int32 tp_k in the first N entries of each row.  gt_count >= 1.  workspace:
 * fv_det_ap_sweep_workspace_bytes(n_img) bytes, 8-byte aligned; its contents on entry are ignored. */
size_t fv_det_ap_sweep_workspace_bytes(int n_img);
int fv_det_ap_sweep(fv_ctx* ctx, const double* rows, const int32_t* nrows, const double* iou, const int32_t* flag, int n_img,
                    const double* thresholds, int n_th, int64_t gt_count, void* workspace, size_t workspace_bytes, double* result,
                    int32_t* n_det, int32_t* order, int32_t* counts);

/* ------------------------------------------------------------------ network description
 * The FaceDetector network: the first 52 conv+BN+LeakyReLU(0.1) layers / 23 residual adds of
 * make_yolov3_model (yd.py:221-267) as re-wired by FaceDetector.YOLOV3Base (fd.py:404-593), plus
 * the Conv2D(6, 3x3, 'same', linear, bias) head (fd.py:348-352).  Parameters live in ONE flat
 * float32 vector owned by the caller (so Adam and the gradient all-reduce are single ranges):
 *   per base layer: kernel OHWI [cout][k][k][cin] at w_off, gamma[cout] at gamma_off, beta[cout]
 *   at beta_off;  head: kernel at w_off, bias[6] at beta_off (gamma_off = -1).
 * BatchNorm moving statistics live in a second flat vector: mean at mean_off, var at var_off. */
typedef struct fv_layer_desc {
    int32_t darknet_index; /* conv_<i> / bnorm_<i> of yd.py; -1 for the head ('output') */
    int32_t ksize, stride, cin, cout;
    int32_t has_bn;        /* 1: BN(eps 1e-3)+LeakyReLU(0.1) follow; 0: linear + bias (head) */
    int32_t role;          /* 0 plain, 1 first conv of a residual block (its input is the skip),
                              2 second conv of a residual block (add(skip, x) follows), 3 head */
    int32_t in_div, out_div; /* spatial size = image_size / div */
    int64_t w_off, gamma_off, beta_off; /* offsets (floats) into the parameter vector */
    int64_t mean_off, var_off;          /* offsets into the BN-state vector (-1 for the head) */
} fv_layer_desc;

int fv_num_layers(void);                       /* 53 */
int fv_layer(int i, fv_layer_desc* out);
int64_t fv_param_count(void);                  /* 40 640 230 trainable floats */
int64_t fv_state_count(void);                  /* 35 712 BN moving mean/var floats */
/* bytes of caller-provided device workspace for a batch; training != 0 keeps every layer's
 * pre-BN and activated output for the backward pass.  The contents of the workspace on entry are ignored, and nothing outside
 * [workspace, workspace + bytes) is written: this holds for every entry point that takes a workspace or a scratch buffer
 * (tests/test_workspace_contract_gpu.py runs each of them on a poisoned workspace between guards). */
size_t fv_workspace_bytes(int batch, int image_size, int training);

/* ------------------------------------------------------------------ hot path: network level */
/* Replaces self.model.predict(image) (fd.py:899): BN in inference mode (moving statistics folded
 * into the conv epilogue), x [batch][S][S][3] float32 NHWC in [0,1], y [batch][S/32][S/32][6].
 * Every tensor is addressed through one 2 GiB buffer descriptor: batch * S * S * 32 (the first layer's output) must stay below
 * 2^29 floats -- 96 images at 416, 45 at 608; beyond that the call returns FV_ERR_INVALID ("... reaches 2^29 elements (2 GiB buffer
 * descriptor) ...") before any convolution is launched, and the caller splits the batch (inference is per image; the Python host does). The
 * same bound holds for fv_forward_base, fv_train_step and the fv_yolov3_* entry points. */
int fv_forward_infer(fv_ctx* ctx, const float* params, const float* bn_state, const float* x, int batch,
                     int image_size, void* workspace, size_t workspace_bytes, float* y);
/* The model `FaceDetector.YOLOV3Base` returns (fd.py:384-600): the Darknet-53 base alone, input -> the output of the last
 * residual add (add_23), feat [batch][S/32][S/32][1024] float32 -- the tensor the head conv reads (fd.py:344-352) and the
 * backbone output FaceIdentifier builds on (face_identification.py:323, 397-614; fv_fid_extract).  Same kernels, same arithmetic and the same
 * workspace as fv_forward_infer; y (may be NULL) additionally receives the head output of the same pass. */
int fv_forward_base(fv_ctx* ctx, const float* params, const float* bn_state, const float* x, int batch,
                    int image_size, void* workspace, size_t workspace_bytes, float* feat, float* y);

/* Called (on the host, in enqueue order) when the gradient range [offset, offset+count) of the
 * flat gradient vector has been fully enqueued on the context's stream -- the hook a data-parallel
 * host uses to start the RCCL all-reduce of that bucket while the backward pass continues. */
typedef void (*fv_bucket_fn)(void* user, int64_t offset, int64_t count);

/* One optimisation step's forward + loss + backward; replaces the TF graph that
 * model.fit_generator runs per batch (fd.py:621-627) with loss='mse' (fd.py:381): training-mode BN
 * (batch statistics, moving statistics updated in bn_state), mean-squared error over every element
 * of [batch][G][G][6], gradients of all 40 640 230 parameters written to `grads` (overwritten).
 * loss: one float (device).  Follow with fv_adam_step.
 * loss_weight: 1 for a single-GPU step.  Data parallel (keras.utils.multi_gpu_model, fd.py:358-371: ONE loss over the
 * concatenated tower outputs): the share n_rank / n_total of the merged batch this call's slice holds -- it scales dL/dy in the
 * loss kernel, so every gradient of the step arrives pre-scaled and the SUM all-reduce over the ranks yields the gradient of
 * the merged-batch mean without a separate scaling pass over the 162 MB vector; `loss` stays this slice's own mean.
 * Reproducibility: kernel gradients are accumulated with float atomics and the BN statistics with fp64
 * atomics, so two runs agree to rounding (dW ~3e-6 relative, statistics in the last float bit at most),
 * not bit for bit; fv_forward_infer is bit-reproducible. */
int fv_train_step(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const float* y_true,
                  int batch, int image_size, void* workspace, size_t workspace_bytes, float* grads,
                  float* loss, double loss_weight, fv_bucket_fn on_bucket, void* user);

/* Introspection of the training workspace after fv_train_step (test aid; Keras keeps these tensors
 * inside the TF graph): where layer `layer` (0..51) keeps which = 0 pre-BN output z, 1 activated output a
 * ([batch][S/div][S/div][cout] each), 2 batch mean, 3 1/sqrt(var+eps), 4 scale, 5 shift ([cout] each).
 * offset_bytes is relative to the workspace pointer given to fv_train_step with the same batch /
 * image_size.  The parity tests read z / scale / shift back to learn which LeakyReLU slope the GPU took
 * for every element, so that the float64 oracle can be evaluated on the same side of each kink. */
/* With option "early_bn_fused" (the default) the step does not write a of layers 0 and 2 where their readers -- forward and
 * weight-gradient of conv_1 / conv_3 -- apply the BN on load: the two tensors keep their place in the workspace (its layout does
 * not depend on the context) but hold no data; z, mean, invstd, scale and shift of those layers are published as ever. */
int fv_train_workspace_tensor(int batch, int image_size, int layer, int which, size_t* offset_bytes,
                              int64_t* count);

/* keras.optimizers.Adam(lr, beta_1, beta_2, decay) update (fd.py:376-379), Keras 2.2.4 formula:
 * t = iteration+1; lr_t = lr/(1+decay*iteration) * sqrt(1-b2^t)/(1-b1^t);
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr_t m / (sqrt(v) + eps)  (eps = 1e-7). */
int fv_adam_step(fv_ctx* ctx, float* params, const float* grads, float* m, float* v, int64_t n,
                 int64_t iteration, double lr, double beta_1, double beta_2, double eps, double decay);
/* v[i] *= alpha over n floats on the context's stream.  The data-parallel host uses it for the one small vector whose mean over
 * the ranks is not a gradient: the 35 712 BN moving statistics after their SUM all-reduce (the reference's towers race on
 * shared variables, fd.py:369 -- SURVEY 8e; the build keeps the ranks identical by averaging). */
int fv_scale(fv_ctx* ctx, float* v, int64_t n, double alpha);

/* ------------------------------------------------------------------ hot path: single operators
 * (what the network-level calls are built from; exported for unit parity tests) */
/* ZeroPadding2D(1)+Conv2D(k=3,'valid',strides=stride) or Conv2D(k=1) of yd.py:205-211.
 * x [B][H][W][cin], w OHWI [cout][k][k][cin] (cin % 32 == 0; for the cin=3 first layer pass the
 * [cout][32] form made by fv_pack_first_layer), out [B][H/stride][W/stride][cout].
 * out = acc*scale[c]+shift[c] (either may be NULL), then LeakyReLU(leaky) if leaky >= 0, then
 * + addend (may be NULL).  If psum != NULL the raw result is stored instead and psum/psq receive
 * per-tile column sums / sums of squares, [fv_conv2d_stat_rows(M)][cout] each. */
int fv_conv2d_forward(fv_ctx* ctx, const float* x, const float* w, int B, int H, int W, int cin, int cout,
                      int ksize, int stride, const float* scale, const float* shift, float leaky,
                      const float* addend, float* out, float* psum, float* psq);
int fv_conv2d_stat_rows(int64_t out_pixels);
/* gradient w.r.t. the conv input.  dy [B][H/stride][W/stride][cout_pad], w_t [cin][k*k][cout_pad]
 * (fv_transpose_weights), dx [B][H][W][cin] = dgrad (+ addend if not NULL). */
int fv_conv2d_dgrad(fv_ctx* ctx, const float* dy, const float* w_t, int B, int H, int W, int cin,
                    int cout_pad, int ksize, int stride, const float* addend, float* dx);
/* gradient w.r.t. the kernel, ACCUMULATED into dw OHWI [cout][k][k][cin] (zero it first).
 * dy has dy_stride >= cout channels per pixel. */
int fv_conv2d_wgrad(fv_ctx* ctx, const float* x, const float* dy, int B, int H, int W, int cin, int cout,
                    int dy_stride, int ksize, int stride, float* dw);
int fv_transpose_weights(fv_ctx* ctx, const float* w, int cout, int taps, int cin, int cout_pad, float* w_t);
int fv_pack_first_layer(fv_ctx* ctx, const float* w, int cout, int k_elems, float* w_packed /*[cout][32]*/);
/* training-mode BatchNormalization(eps) statistics from the conv partials: mean, 1/sqrt(var+eps),
 * scale = gamma*invstd, shift = beta-mean*scale; moving stats updated in place when not NULL
 * (Keras: moving = momentum*moving + (1-momentum)*batch, variance scaled by n/(n-(1+eps))). */
int fv_bn_finalize(fv_ctx* ctx, const float* psum, const float* psq, int stat_rows, int C, int64_t count,
                   const float* gamma, const float* beta, float eps, float momentum, float* mean,
                   float* invstd, float* scale, float* shift, float* moving_mean, float* moving_var);
/* out = LeakyReLU(z*scale+shift) (+ skip) over [rows][C] */
int fv_bn_act(fv_ctx* ctx, const float* z, const float* scale, const float* shift, const float* skip,
              float* out, int64_t rows, int C, float leaky);
/* backward of BN(train)+LeakyReLU: dz, dgamma[C], dbeta[C] from g = dL/d(activated output).
 * scratch: 2 * fv_bn_bwd_scratch_floats(rows, C) floats. */
int64_t fv_bn_bwd_scratch_floats(int64_t rows, int C);
int fv_bn_bwd(fv_ctx* ctx, const float* g, const float* z, const float* scale, const float* shift,
              const float* mean, const float* invstd, int64_t rows, int C, float leaky, float* scratch,
              float* dbeta, float* dgamma, float* dz);
/* ---- the fused forms fv_train_step actually runs (same Keras semantics, yd.py:212-215; exported so
 * that each is checked against float64 on its own).  "Slots": [nslot][2][C] float64 accumulators the
 * CALLER zeroes; producers ADD per-tile column sums with fp64 atomics (slot = tile % nslot), the
 * consumer sums the slots in fixed order.  nslot = fv_bn_stat_slots(C); C % 4 == 0, C <= 1024 and C
 * divides or is divided by 256. */
int fv_bn_stat_slots(int C);
/* conv forward storing the raw result z and ADDING the column sums of z and z^2 to `slots`. */
int fv_conv2d_forward_slots(fv_ctx* ctx, const float* x, const float* w, int B, int H, int W, int cin, int cout,
                            int ksize, int stride, float* z, double* slots, int nslot);
/* training-mode BN + LeakyReLU (+ skip) fed by the slots: sums them, publishes mean / invstd / scale /
 * shift, updates the moving statistics (may be NULL), writes out = leaky(z*scale+shift) (+ skip). */
int fv_bn_act_slots(fv_ctx* ctx, const float* z, const double* slots, int nslot, int64_t rows, int C,
                    const float* gamma, const float* beta, float eps, float momentum, float* mean, float* invstd,
                    float* scale, float* shift, float* moving_mean, float* moving_var, const float* skip,
                    float* out, float leaky);
/* fv_conv2d_dgrad whose epilogue also reduces d-beta / d-gamma of the BN+LeakyReLU layer that PRODUCED
 * the conv input: with that layer's pre-BN tensor bn_z [B][H][W][cin] and its mean / invstd / scale /
 * shift, gy = dx * leaky'(bn_z*scale+shift) and the column sums of gy and gy*(bn_z-mean)*invstd are
 * ADDED to `slots`.  cin % 4 == 0.  With scratch lent (fv_set_conv_scratch) the launch may take the
 * tail split, whose fix-up kernel then does the same reduction. */
int fv_conv2d_dgrad_bnred(fv_ctx* ctx, const float* dy, const float* w_t, int B, int H, int W, int cin,
                          int cout_pad, int ksize, int stride, const float* addend, float* dx,
                          const float* bn_z, const float* scale, const float* shift, const float* mean,
                          const float* invstd, float leaky, double* slots, int nslot);
/* backward of BN(train)+LeakyReLU through the slots.  reduced = 0: this call first adds the column
 * sums to `slots` (its own reduction pass); reduced = 1: they are already there (fv_conv2d_dgrad_bnred).
 * Then: d-beta, d-gamma = slot sums (as float), dz = scale*(gy - dbeta/rows - xhat*dgamma/rows). */
int fv_bn_bwd_slots(fv_ctx* ctx, const float* g, const float* z, const float* scale, const float* shift,
                    const float* mean, const float* invstd, int64_t rows, int C, float leaky, double* slots,
                    int nslot, int reduced, float* dbeta, float* dgamma, float* dz);
/* ---- the BN passes folded into halo kernels (option "early_bn_fused"), as single operators.  Each returns FV_ERR_INVALID when
 * the halo kernel that has the mode does not take the shape: there is no other implementation to fall back to.
 * fv_conv2d_forward_slots whose input is LeakyReLU(z_in*in_scale+in_shift), formed while z_in [B][H][W][cin] is staged (zero
 * padding stays zero): 3x3, 32 -> 64 channels, stride 1 or 2.  z is bit-identical to fv_bn_act + fv_conv2d_forward_slots. */
int fv_conv2d_forward_slots_bn_in(fv_ctx* ctx, const float* z_in, const float* in_scale, const float* in_shift, float leaky,
                                  const float* w, int B, int H, int W, int cin, int cout, int ksize, int stride, float* z,
                                  double* slots, int nslot);
/* fv_bn_act_slots of the producing layer + fv_conv2d_forward_slots of a 1x1 stride-1 conv in one kernel (option "bn_in_1x1"):
 * z_in [B][H][W][cin] is the producing layer's raw conv output with its statistics in in_slots [in_nslot][2][cin]; the kernel
 * publishes mean / invstd / scale / shift [cin] (+ the moving statistics when given), writes a_out = LeakyReLU(z_in*scale+shift)
 * (+ skip when given) and z = conv(a_out, w) with its column sums added to slots.  cin % 32 == 0, cin <= 512, cout % 4 == 0,
 * cout > 32.  a_out, z and the vectors are bit-identical to the two calls. */
int fv_conv2d_forward_slots_bn_stats_in(fv_ctx* ctx, const float* z_in, const double* in_slots, int in_nslot, const float* gamma,
                                        const float* beta, float eps, float momentum, float* mean, float* invstd, float* scale,
                                        float* shift, float* moving_mean, float* moving_var, const float* skip, float* a_out,
                                        float leaky, const float* w, int B, int H, int W, int cin, int cout, float* z,
                                        double* slots, int nslot);
/* Which normalise passes of a training step run inside the next layer's 1x1 conv under option value `option` (and
 * "conv1x1_persist" on): folded[l] = 1 when layer l's pass is folded into layer l + 1's forward, else 0, for the n =
 * fv_num_layers() / fv_yolov3_num_layers() layers.  Needs no device. */
int fv_train_bn_in_1x1_plan(int option, int batch, int image_size, int32_t* folded, int n);
int fv_yolov3_train_bn_in_1x1_plan(int option, int batch, int image_size, int out_channels, int32_t* folded, int n);
/* fv_conv2d_wgrad with the same input transform (same shapes). */
int fv_conv2d_wgrad_bn_in(fv_ctx* ctx, const float* z_in, const float* in_scale, const float* in_shift, float leaky,
                          const float* dy, int B, int H, int W, int cin, int cout, int dy_stride, int ksize, int stride,
                          float* dw);
/* fv_bn_bwd_slots(reduced = 1) + fv_conv2d_wgrad of the first layer (3x3 stride 1, 3 -> 32 channels) in one kernel: dz is formed
 * from g and z [B][H][W][cout] while they are staged and never stored; d-beta / d-gamma = slot sums, stored or (accumulate != 0)
 * added to what dbeta / dgamma hold.  dw is ACCUMULATED (zero it first). */
int fv_conv2d_wgrad_bn_bwd(fv_ctx* ctx, const float* x, const float* g, const float* z, const float* scale, const float* shift,
                           const float* mean, const float* invstd, float leaky, const double* slots, int nslot, int B, int H,
                           int W, int cin, int cout, int ksize, int stride, int accumulate, float* dbeta, float* dgamma,
                           float* dw);
/* loss = mean((yp-yt)^2) over [rows][C]; dy [rows][c_pad] = 2(yp-yt)/(rows*C) zero padded;
 * dbias[C] = column sums of dy (may be NULL). */
int fv_mse_loss_grad(fv_ctx* ctx, const float* yp, const float* yt, int rows, int C, int c_pad,
                     float* loss, float* dy, float* dbias);
/* ---- the helpers of fv_yolov3_train_step as single operators (exported so that each is checked against float64 on its own, at
 * the production row counts the small whole-step tests never reach).  Each call forwards to the launcher the step calls and sizes
 * its partial buffer with the step's own helper; an additive part of ABI version 4 (no existing entry point changed).
 * UpSampling2D(2) (nearest) of src [B][Hs][Ws][C1] concatenated in front of skip [B][2Hs][2Ws][C2] (yd.py:282-283, 298-299)
 * -> out [B][2Hs][2Ws][C1+C2]; a pure copy.  C1 % 4 == 0 and C2 % 4 == 0, FV_ERR_INVALID otherwise (nothing is written). */
int fv_upsample_concat(fv_ctx* ctx, const float* src, const float* skip, float* out, int B, int Hs, int Ws, int C1, int C2);
/* its backward: g [B][2Hs][2Ws][C1+C2] -> g_up [B][Hs][Ws][C1] = (p + q) + (r + t) of the 2x2 block of the first C1 channels
 * (p, q the upper row left to right, r, t the lower; fp32, this order), g_skip [B][2Hs][2Ws][C2] = a copy of the other C2. */
int fv_upsample_concat_bwd(fv_ctx* ctx, const float* g, float* g_up, float* g_skip, int B, int Hs, int Ws, int C1, int C2);
/* out[C] = column sums of dy [rows][c_pad] over its first C columns (the bias gradient of a detection conv): fp64 sums in a
 * fixed order, rounded to float once; columns >= C are never read.  partial: fv_colsum_partial_doubles(rows, C) doubles. */
int64_t fv_colsum_partial_doubles(int64_t rows, int C);
int fv_colsum(fv_ctx* ctx, const float* dy, int64_t rows, int C, int c_pad, double* partial, float* out);
/* The detection loss of fv_yolov3_train_step and its gradient.  yp3 / yt3 / dy3: HOST arrays of three DEVICE pointers (scale 0
 * first): logits and targets [cells3[s]][A][5+ncls], dy [cells3[s]][c_pad] = grad_weight * dL/d(logit), columns >= A*(5+ncls)
 * zeroed.  loss (device float) = sum over the scales of the mean over (cell, anchor) of the per-box term stated at
 * fv_yolov3_train_step, unweighted.  grad_weight finite and > 0, c_pad >= A*(5+ncls); partial:
 * fv_yolo_loss_partial_doubles(cells3, A) doubles, laid out as in the step.  Deterministic (fp64 sums in a fixed order). */
int64_t fv_yolo_loss_partial_doubles(const int64_t* cells3, int A);
int fv_yolo_loss_grad(fv_ctx* ctx, const float* const* yp3, const float* const* yt3, const int64_t* cells3, int ncls, int A,
                      int c_pad, double grad_weight, double* partial, float* loss, float* const* dy3);
/* Letterbox preprocessing (SURVEY 8f "next" row 1): replaces image/255 -> cv2.resize(INTER_CUBIC)
 * -> cv2.copyMakeBorder(zeros) of fd.py:112-147 / 656-694 / 798-835.  src: uint8 [h][w][3] (device),
 * dst: float32 [S][S][3]; geom (host, may be NULL) receives w_p, h_p, pad_t, pad_b, pad_l, pad_r.
 * Geometry is exact; pixels follow OpenCV's bicubic (a=-0.75) in fp32 (parity unpinned vs cv2). */
int fv_letterbox(fv_ctx* ctx, const uint8_t* src, int h, int w, int image_size, float* dst, int32_t* geom);
/* The same for a whole training batch in one launch (fd.py:98-147, the body of
 * TrainingSequence.__getitem__): the n decoded images lie back to back in `packed` (device; one
 * host-to-device copy per batch), image i at byte offsets[i] with hw[2i] rows and hw[2i+1] columns
 * (offsets, hw, geom: HOST arrays; geom [n][6] may be NULL).  dst [n][S][S][3].  Pixels identical to
 * n calls of fv_letterbox. */
int fv_letterbox_batch(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                       int image_size, float* dst, int32_t* geom);
/* Crop + letterbox of many face rectangles in one call (FaceIdentifier.test, fi.py:1061-1101: `image_o[(t-1):(b-1), (l-1):(r-1)]`,
 * /255, cv.resize(INTER_CUBIC), cv.copyMakeBorder).  packed / offsets / hw: the batch's n_img decoded images as for
 * fv_letterbox_batch.  crops: HOST int32 [n][5] records (image index, y0, x0, h, w), each inside its image.  dst [n][S][S][3].
 * Crop c is letterboxed as fv_letterbox would letterbox a contiguous copy of those h x w pixels -- same geometry, same bicubic
 * weights, same fp64 source coordinates, the border replicated at the crop's edges: bit-identical to that call.  Any number of
 * crops (chunked inside the call).  A crop outside its image, or one whose letterboxed side rounds to 0, is FV_ERR_INVALID and
 * nothing is enqueued. */
int fv_letterbox_crops(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img,
                       const int32_t* crops, int n, int image_size, float* dst);
/* fv_letterbox_batch with a per-image placement and colour distortion, for FaceDetector.train with hps['augment'] (not in the
 * reference; data.draw_augment draws the parameters).  packed / offsets / hw: the n images as for fv_letterbox_batch.  place: HOST
 * int32 [n][8] records (cy0, cx0, ch, cw, T, oy, ox, flip): the ch x cw crop at (cy0, cx0) of image i is letterboxed as
 * fv_letterbox_crops letterboxes it at image_size T -- bit-identical to that call -- into the T x T box at row oy, column ox of
 * the otherwise zero S x S canvas; flip = 1 then mirrors the finished canvas, padding included (x -> S - 1 - x).  colour: HOST float
 * [n][3] records (dh, sat, exp), or NULL for none; a record that is exactly (0, 1, 1) leaves its image's pixels as resampled.
 * Otherwise each content pixel is clamped to [0, 1], converted to HSV (v = max, s = (max - min) / max or 0 for black; h in turns
 * from the usual six-sector form, 0 for grey), h = frac(h + dh), s *= sat, v *= exp, converted back and clamped to [0, 1], all in
 * float32 (Darknet's distort_image); padding stays 0.  dst: DEVICE float32 [n][S][S][3], 16-byte aligned; image_size a multiple
 * of 4.  One kernel, one pass, chunks of 64 images per launch, on the context's stream; no atomics: the same call gives the same
 * bits.  Every record is checked before anything is enqueued -- crop inside its image, 1 <= T <= S, 0 <= oy, ox <= S - T, a
 * letterboxed side of at least 1, flip 0 or 1, finite colour values -- and a bad one is FV_ERR_INVALID with dst untouched. */
int fv_letterbox_augment_batch(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int image_size,
                               const int32_t* place, const float* colour, float* dst);
/* Mosaic: canvases made of up to four tiles, for FaceDetector.train with hps['mosaic'] (not in the reference; data.draw_mosaic
 * draws the tables).  packed / offsets / hw: the n_img images as for fv_letterbox_batch.  tiles: HOST int32 [n_tiles][14] records
 * (canvas, image, cy0, cx0, ch, cw, T, oy, ox, flip, wy0, wx0, wy1, wx1), sorted by canvas, 1 to 4 for every canvas 0 .. n_out - 1:
 * the ch x cw crop at (cy0, cx0) of `image` is letterboxed as fv_letterbox_crops letterboxes it at image_size T into a T x T box
 * whose corner lies at row oy, column ox of the S x S canvas -- oy, ox may be negative and the box may reach beyond the canvas --
 * flip = 1 mirrors the BOX in place, padding included (local column c -> T - 1 - c), and only the WINDOW rows [wy0, wy1) x columns
 * [wx0, wx1) of the canvas shows the tile.  colour: HOST float [n_tiles][3] records (dh, sat, exp) per tile, or NULL.  An output
 * pixel inside a tile's window and inside its placed content rectangle holds fv_letterbox_crops's bits for that crop at image
 * size T at the (mirrored) local position, then fv_letterbox_augment_batch's colour stage when the tile's record is not exactly
 * (0, 1, 1); every other pixel is +0.  One tile whose window is the whole canvas is fv_letterbox_augment_batch's sample (its flip
 * restated for the box: ox' = S - T - ox).  dst: DEVICE float32 [n_out][S][S][3], 16-byte aligned; image_size a multiple of 4.
 * One kernel, one pass, whole canvases of up to 48 tiles together per launch, on the context's stream; no atomics: the same call
 * gives the same bits.  Every record is checked before anything is enqueued -- canvas in range and non-decreasing, 1 to 4 tiles
 * for every canvas, image in range, crop inside its image, 1 <= T <= 4 S, -T <= oy, ox <= S, a letterboxed side of at least 1,
 * flip 0 or 1, a non-empty window inside the canvas, the windows of one canvas pairwise disjoint, finite colour values -- and a
 * bad one is FV_ERR_INVALID with dst untouched.  Additive: fv_abi_version() is unchanged. */
int fv_letterbox_mosaic_batch(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img, int image_size,
                              int n_out, const int32_t* tiles, const float* colour, int n_tiles, float* dst);
/* Crop + nearest-neighbour letterbox of many face rectangles on uint8, in one call (create_db_fi / save_extracted_face,
 * fi.py:113-161 and 233-274: the slice, cv.resize(INTER_NEAREST), cv.copyMakeBorder(value 0)).  Images and crop records as for
 * fv_letterbox_crops; dst: device uint8 [n][S][S][3], 16-byte aligned; image_size a multiple of 16, at most 4096.  Geometry as
 * fv_letterbox (int(h / w * S), the odd padding pixel at the bottom / right).  Destination pixel (y, x) of the resized area
 * reads source pixel (min(floor(y * ify), h - 1), min(floor(x * ifx), w - 1)) of the crop, ifx = 1.0 / (w_p / (double)w), ify
 * likewise, in IEEE fp64; the padding is 0.  That index rule is this build's DEFINITION of INTER_NEAREST (OpenCV's resizeNN as
 * published); parity with cv2 itself is unpinned, as for the bicubic path.  A pure gather: exact against that definition.  Any
 * number of crops (chunked inside the call); n == 0 does nothing.  A crop outside its image, h or w below 1, or a letterboxed
 * side that rounds to 0 is FV_ERR_INVALID and nothing is enqueued. */
int fv_crop_nearest_u8(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img,
                       const int32_t* crops, int n, int image_size, uint8_t* dst);
/* Rows of a device-resident store of uint8 images as a float32 batch in [0, 1] (the input of FaceIdentifier.train and of the
 * facial-ID database from crop_store.CropStore; fi.py:1577, `img.astype(np.float32) / 255.0`, without the host).  store: DEVICE
 * array of n_slots slots of elems bytes each; idx: HOST int32 [n]; dst: DEVICE float32 [n][elems]:
 *     dst[j][e] = (float)store[idx[j] * elems + e] / 255.0f,
 * the correctly rounded IEEE float32 quotient -- bit for bit numpy's `x.astype(np.float32) / np.float32(255.0)` for each of the 256
 * byte values, whatever floating-point flags the library is built with (csrc/crop_gather.hip).  Indices may repeat and come in
 * any order.  Stream-ordered; no device allocation and no synchronisation inside the call; the index list travels in the kernel
 * arguments, FV_GATHER_CHUNK indices per launch, chunked inside the call.  Any n; n == 0 does nothing.  All byte offsets are
 * 64-bit (a store of 416 x 416 x 3 crops passes 4 GiB at slot 8 273).  Every argument is checked before the first launch, and
 * before the context is looked at: an index outside [0, n_slots), elems < 16, elems % 16 != 0, elems > 2^36, a store or dst that
 * is not 16-byte aligned, a negative n or n_slots, or a null pointer with n > 0 is FV_ERR_INVALID and nothing is enqueued.  An
 * additive part of ABI version 4. */
#define FV_GATHER_CHUNK 128
int fv_gather_u8_f32(fv_ctx* ctx, const uint8_t* store, int64_t n_slots, int64_t elems, const int32_t* idx, int n, float* dst);
/* Draw onto the packed uint8 RGB images of a batch, in place (FaceIdentifier.evaluate, fi.py:945-992: the rectangles and labels
 * of draw_boxes_v3, yolov3_detect.py:515-530).  packed / offsets / hw: the batch's n_img decoded images as for
 * fv_letterbox_batch.  prims: HOST array of n primitives, applied in order; masks: DEVICE buffer of mask_bytes 8-bit masks.
 *   FV_DRAW_OUTLINE  corners x0, y0, x1, y1 (inclusive) and a width: every pixel with x0 <= x <= x1, y0 <= y <= y1 and
 *                    (x - x0 < width or x1 - x < width or y - y0 < width or y1 - y < width) becomes (r, g, b).  Corners may lie
 *                    outside the image on any side, or be out of order (nothing is drawn then).
 *   FV_DRAW_MASK     top-left x0, y0 (may be negative), mask size x1 = mw, y1 = mh, the mask row-major with mw bytes per row at
 *                    masks + mask_off.  For every mask pixel inside the image and each channel, with m the mask byte:
 *                    t = old * (255 - m) + ink * m + 128; new = ((t >> 8) + t) >> 8 (Pillow's BLEND8, what ImageDraw.text does
 *                    with the rasterised text).  `width` is ignored.
 * The result equals applying the primitives one after another: where two overlap, the later one sees the earlier one's output.
 * Every primitive is clipped to its image; images and pixels no primitive touches keep their bytes.  Stream-ordered; no device
 * allocation and no synchronisation inside the call; the table travels in the kernel arguments, 32 primitives per launch, in
 * order.  Any number of primitives; n == 0 does nothing.  FV_ERR_INVALID, with nothing enqueued, for: an image index outside
 * [0, n_img), an outline width < 1, a negative mask size, a mask that does not lie inside [0, mask_bytes), an unknown kind, an
 * image with fewer than 1 row or column or more than 524 280 rows. */
enum { FV_DRAW_OUTLINE = 0, FV_DRAW_MASK = 1 };
typedef struct fv_draw_prim {
    int32_t kind, image;
    int32_t x0, y0, x1, y1;
    int32_t width;
    uint8_t r, g, b, reserved;
    int64_t mask_off;
} fv_draw_prim;
int fv_draw_prims_u8(fv_ctx* ctx, uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n_img,
                     const fv_draw_prim* prims, int n, const uint8_t* masks, int64_t mask_bytes);

/* ------------------------------------------------------------------ JPEG decode, split host / device
 * (replaces `imread` of fd.py:112, 656, 798 for baseline / extended-sequential Huffman JPEGs with 1 or 3
 * components and 4:4:4 / 4:2:2 / 4:2:0 sampling; anything else -> FV_ERR_INVALID and the caller decodes that file elsewhere).
 * The host part (no context, thread-safe, pure CPU) parses the headers and Huffman-decodes the scan into quantised coefficients:
 * int16, natural (de-zigzagged) order, [64] per block, component after component, each component's block grid padded to whole
 * MCUs in raster order.  The device part dequantises, inverse-transforms (libjpeg's jpeg_idct_islow), upsamples the chroma
 * (libjpeg's "fancy" triangle filters, its replicating ones where there are at most two chroma columns) and converts
 * YCbCr -> RGB for a whole batch in two launches: for every stream the host part ACCEPTS, pixels bit-identical to
 * libjpeg-turbo's default decode (what Pillow / scikit-image return).  The host part refuses (FV_ERR_INVALID) whatever it cannot
 * hold to that: colour spaces other than libjpeg's YCbCr decision, a scan that is cut, lacks or misnumbers an RSTn or lacks its
 * EOI, a block outside the coefficient range in which libjpeg's inverse DCTs agree. */
typedef struct fv_jpeg_info {
    int32_t width, height, ncomp, hmax, vmax, restart_interval;
    int32_t h[3], v[3], blocks_w[3], blocks_h[3];
    int64_t coef_off[3];   /* first coefficient of component c, in int16 units from the image's coefficient array */
    int64_t total_coefs;
    uint16_t qt[3][64];    /* quantisation table of component c, natural order */
} fv_jpeg_info;
typedef struct fv_jpeg_desc {   /* one image of a batch; array in DEVICE memory */
    int32_t width, height, ncomp, hmax, vmax, reserved;
    int32_t blocks_w[3], blocks_h[3];
    int64_t coef_off[3];   /* absolute, int16 units from `coefs` */
    int64_t plane_off[3];  /* absolute, bytes from `planes` (component c needs blocks_w*blocks_h*64 bytes) */
    int64_t rgb_off;       /* bytes from `rgb` (height*width*3 bytes, rows packed) */
    uint16_t qt[3][64];
} fv_jpeg_desc;
int fv_jpeg_parse(const uint8_t* data, size_t nbytes, fv_jpeg_info* info);
int fv_jpeg_entropy_decode(const uint8_t* data, size_t nbytes, int16_t* coefs, int64_t ncoefs);   /* HOST buffers */
int64_t fv_jpeg_plane_bytes(const fv_jpeg_info* info);
/* coefs, descs, planes (scratch), rgb: device; max_blocks / max_pixels: the largest block / pixel count of one image (grid size) */
int fv_jpeg_reconstruct_batch(fv_ctx* ctx, const int16_t* coefs, const fv_jpeg_desc* descs, int n, uint8_t* planes, uint8_t* rgb,
                              int64_t max_blocks, int64_t max_pixels);

/* ------------------------------------------------------------------ JPEG encode, on the device (csrc/jpeg_enc.hip)
 * The entropy-coded scan of what `PIL.Image.fromarray(rgb).save(path)` writes with libjpeg-turbo -- 8-bit RGB, quality 75, 4:2:0,
 * the Annex K Huffman tables, no restart markers; nothing else is offered -- byte for byte, for a batch of n images of any sizes
 * in one pair of calls.  packed / offsets / hw: the images as for fv_letterbox_batch (packed: device, packed_bytes long; offsets,
 * hw: HOST arrays; any order, gaps allowed).  The caller puts the header (SOI .. SOS, which depends on the size alone) in front
 * and EOI behind.  An additive part of ABI version 4.
 *   fv_jpeg_encode_workspace_bytes  bytes of workspace the batch needs (device, 16-byte aligned), -1 for a size outside
 *       1 <= rows, columns <= 65535.  Sized for the longest block the tables admit (1658 bits), so it holds whatever the pixels.
 *   fv_jpeg_encode_coefs    the front end alone: colour conversion, edge replication, 2x2 chroma downsampling, forward DCT
 *       (jpeg_fdct_islow), quantisation.  Leaves int16 coefficients in the workspace at byte *coef_offset_bytes: [64] per block in
 *       ZIGZAG order, the blocks in scan order (MCU after MCU, Y00 Y01 Y10 Y11 Cb Cr), image after image.  Luma blocks beyond
 *       ceil(w/8) x ceil(h/8) are libjpeg's dummy blocks (AC 0, DC of the block before them in the MCU).
 *   fv_jpeg_encode_measure  call 1: the front end, the Huffman bit lengths, their prefix sum, the bits packed, the FF bytes
 *       counted.  counts (DEVICE int64 [n]) receives every scan's length in bytes, stuffing and the 1-bit pad included.
 *   fv_jpeg_encode_emit     call 2, on the same stream, workspace, hw and n: counts is the HOST copy of what call 1 left; the
 *       scans are written back to back in image order, scan i at out + counts[0] + .. + counts[i-1].  out_bytes >= their sum; not a
 *       byte of out beyond that sum is written.
 * Stream-ordered; no allocation and no synchronisation inside (the caller waits once, to read counts).  n == 0 does nothing.
 * Every argument is checked before anything is enqueued: a size outside 1..65535, an image that does not lie inside
 * [0, packed_bytes), a workspace or output too small, a count below 1 is FV_ERR_INVALID with workspace and outputs untouched. */
int64_t fv_jpeg_encode_workspace_bytes(const int32_t* hw, int n);
int fv_jpeg_encode_coefs(fv_ctx* ctx, const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets, const int32_t* hw, int n,
                         void* workspace, size_t workspace_bytes, int64_t* coef_offset_bytes);
int fv_jpeg_encode_measure(fv_ctx* ctx, const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets, const int32_t* hw, int n,
                           void* workspace, size_t workspace_bytes, int64_t* counts);
int fv_jpeg_encode_emit(fv_ctx* ctx, const int32_t* hw, int n, void* workspace, size_t workspace_bytes, const int64_t* counts,
                        uint8_t* out, int64_t out_bytes);

/* ------------------------------------------------------------------ FaceIdentifier (facial IDs, triplet loss)
 * The reference's second model (face_identification.py = fi.py): FaceIdentifier (fi.py:288-376) runs ONE shared Darknet-53 base
 * (the 52 BN layers of fv_layer(0..51), weights as FaceDetector.YOLOV3Base) over three inputs, then Flatten (NHWC row-major,
 * F = (S/32)^2 * 1024 = 173 056 at 416), Dense(64, relu) and K.l2_normalize (x * rsqrt(max(sum x^2, 1e-12)): an all-zero ReLU row
 * stays zero); the facial-ID extractor (_make_fid_extractor, fi.py:378-395) is the same chain for one input with inference BN.
 * Flat parameter layout: the 52 base layers exactly at their fv_layer offsets (first 40 584 928 floats), then the dense kernel
 * [F][64] (Keras layout), then the bias [64] -- 51 660 576 floats at 416.  BN moving statistics: the fv_state_count() vector.
 * dense1_dim is fixed at 64: the reference's loss slices 0:64 / 64:128 / 128:192 (fi.py:72-76). */
int64_t fv_fid_param_count(int image_size);   /* 0 unless image_size is a positive multiple of 32 */
/* training = 0: fv_fid_extract, != 0: fv_fid_train_step / fv_fid_train_step_dp (three towers' kept tensors). */
size_t fv_fid_workspace_bytes(int batch, int image_size, int training);
/* Replaces fid_extractor.predict (fi.py:378-395): x [batch][S][S][3] in [0,1] -> fid [batch][64], inference-mode BN.  Runs
 * fv_forward_base (feature map kept in the workspace), then the dense layer split over F in fixed chunks whose partials are
 * summed in chunk order (no atomics): bit-reproducible, and an image's ID does not depend on the rest of the batch.  Batch bound as
 * fv_forward_infer. */
int fv_fid_extract(fv_ctx* ctx, const float* params, const float* bn_state, const float* x, int batch, int image_size,
                   void* workspace, size_t workspace_bytes, float* fid);
/* One step of model.fit_generator with loss=triplet_loss (fi.py:616-643, 72-76): forward of the towers a, p, n (xa / xp / xn,
 * [batch][S][S][3] each) through the shared base in training-mode BN, each tower normalising with ITS OWN batch statistics; the
 * dense layer and l2_normalize over the 3*batch rows; loss = mean_b max(|ua - up| - |ua - un| + 0.2, 0) (device float); the
 * gradient of every parameter of the fv_fid_param_count layout into `grads` (overwritten).  Follow with fv_adam_step over the
 * whole vector.  This build's definitions where the reference's stack leaves the result open (Keras is not importable here, so
 * they are not pinned against it):
 *  - BN moving statistics: each tower applies its own update (Keras calls the shared base three times), in the order a -> p -> n.
 *    With fv_set_bn_zero_debias_step(ctx, k) before the call, the three updates are the zero-debiased updates k, k + 1, k + 2 of
 *    the model's life (the host passes k = 3 * steps so far + 1); with 0 all three are the plain EMA.
 *  - a distance of exactly 0 contributes gradient 0 (TF's sqrt gradient is NaN there and would poison every weight); the hinge
 *    passes the gradient where its argument is >= 0 (TF's MaximumGrad), ReLU where the pre-activation is > 0 (ReluGrad).
 * Reproducibility as fv_train_step (float atomics in the conv weight-gradients).  The same call as fv_fid_train_step_dp with
 * loss_weight 1 and no callback. */
int fv_fid_train_step(fv_ctx* ctx, const float* params, float* bn_state, const float* xa, const float* xp, const float* xn,
                      int batch, int image_size, void* workspace, size_t workspace_bytes, float* grads, float* loss);
/* The data-parallel form of fv_fid_train_step (the reference wraps the triplet model in keras.utils.multi_gpu_model,
 * fi.py:303-312, 348-361): one process per GPU runs this call on its slice of the merged triplet batch.
 * loss_weight: the slice's share n_rank / n_total, finite and > 0 (FV_ERR_INVALID otherwise, nothing is written).  It scales
 * dL/d(pre-activation) of the 3*batch dense rows and the bias gradient inside the loss kernel, once, where the fp64 values are
 * rounded to float (a power of two scales both exactly); every gradient downstream arrives pre-scaled and the SUM all-reduce over
 * the ranks yields the gradient of the merged-batch mean.  `loss` stays this slice's own unweighted mean.
 * on_bucket (may be NULL): as for fv_train_step / fv_yolov3_train_step -- ranges arrive on the host in enqueue order, with
 * descending offsets, contiguous, covering [0, fv_fid_param_count(image_size)) exactly once; fv_set_bucket_on_side and the
 * "overlap" option mean what they mean there.  All three towers accumulate into the same vector, so a range is reported only when
 * the last tower's contribution to it is in the queue: the dense bias and the dense kernel right after the dense weight-gradient,
 * before any base backward starts (made on the context's stream; with fv_set_bucket_on_side the side stream is made to wait for
 * them first), then the base layers' ranges from the backward pass of the third tower.  `grads` is zeroed on the context's
 * stream at the top of the call: the caller joins the previous step's collectives before that (before fv_adam_step). */
int fv_fid_train_step_dp(fv_ctx* ctx, const float* params, float* bn_state, const float* xa, const float* xp, const float* xn,
                         int batch, int image_size, void* workspace, size_t workspace_bytes, float* grads, float* loss,
                         double loss_weight, fv_bucket_fn on_bucket, void* user);
/* The dense head on its own (operator parity tests): x [rows][F] -> out [rows][64] = l2_normalize(relu(x . w + bias)),
 * w [F][64]; pre (may be NULL) receives x . w + bias.  F % 256 == 0; partial: fv_fid_dense_partial_floats(rows, F) floats. */
int64_t fv_fid_dense_partial_floats(int rows, int64_t F);
int fv_fid_dense_l2(fv_ctx* ctx, const float* x, int rows, int64_t F, const float* w, const float* bias, float* partial,
                    float* pre, float* out);
/* The head kernels of fv_fid_train_step as single operators, over the rows the step builds: row m (0 <= m < M <= 3 * per) lies
 * at tower m / per, row m % per -- three separately allocated [per][F] buffers read (written) in place; a tower that M does not
 * reach may be NULL, one that it reaches may not (FV_ERR_INVALID, as for M > 3 * per and F % 256 != 0; nothing is written).
 * fv_fid_towers_dense_l2: fv_fid_dense_l2 over those rows; partial: fv_fid_dense_partial_floats(M, F) floats.  A row's pre / out
 * bits depend on that row, w and bias alone -- not on M, per or the other rows. */
int fv_fid_towers_dense_l2(fv_ctx* ctx, const float* x0, const float* x1, const float* x2, int per, int M, int64_t F,
                           const float* w, const float* bias, float* partial, float* pre, float* out);
/* Triplet loss over B triplets (rows b, B + b, 2B + b of pre / u [3B][64], u = l2_normalize(relu(pre)) as the dense call returns
 * them): loss (device float) = mean_b max(|ua - up| - |ua - un| + 0.2, 0), unweighted; dE [3B][64] = grad_weight * dL/d pre with
 * the definitions stated at fv_fid_train_step (distance exactly 0: gradient 0; hinge passes at >= 0; ReLU at pre > 0; a row with
 * sum relu(pre)^2 <= 1e-12 is scaled by the constant 1e6); dbias [64] = the column sums of the stored dE (fp64, fixed order).
 * grad_weight finite and > 0. */
int fv_fid_triplet_loss_grad(fv_ctx* ctx, const float* pre, const float* u, int B, double grad_weight, float* loss, float* dE,
                             float* dbias);
/* Batch triplet loss with in-batch mining (FaceNet section 3.2 online mining; Hermans et al., "batch hard"): pre / u [M][64] as the
 * dense call returns them, subjects [M] int32 (device; u 16-byte aligned), 1 <= M <= 1024.  Every row of a known subject is an
 * anchor; its triplet is formed inside the batch.
 *   D(i, r): the distance of fv_fid_match and fv_fid_mine_negatives (sqrt of the fp64 sum, in dimension order, of the squared fp64
 *   differences).  Row r is a positive candidate of anchor i iff r != i and subjects[r] == subjects[i] >= 0, a negative candidate
 *   iff subjects[r] >= 0 and subjects[r] != subjects[i]; a row of subject < 0 is never an anchor, a positive or a negative; a row
 *   whose D(i, r) is NaN belongs to no class.
 *   positive p_i: the candidate with the largest D, the lowest r among equals; dap = D(i, p_i).
 *   negative n_i: mode 0 (batch hard) the minimum of (D, r) over the negative candidates; mode 1 (batch semi-hard) the row that
 *   fv_fid_mine_negatives' mode 0 table picks for (dap, margin) among them (semi-hard nearest, else the mildest violating, else
 *   the nearest easy).  kind: 0 / 1 / 2 by that table's three inequalities, in both modes.
 *   An anchor is valid iff it has both; otherwise pos_index = neg_index = -1, kind = 3, d_ap one quiet NaN (sign and payload
 *   clear), d_an +inf, and it contributes nothing.
 *   loss (device float) = (1 / V) sum over the V valid anchors, in anchor order (fp64), of max(h_i, 0), h_i = dap - dan + margin;
 *   V == 0: loss 0, dE and dbias exactly 0, FV_OK.
 *   gradient, with the definitions stated at fv_fid_train_step: an anchor with h_i >= 0 adds c ((u_i - u_p) / dap - (u_i - u_n) / dan)
 *   to row i, -c (u_i - u_p) / dap to row p_i and c (u_i - u_n) / dan to row n_i, c = 1 / V (a distance of exactly 0: 0).  Row r's
 *   total is one fp64 sum in a fixed order -- its own anchor term, then for i = 0 .. M-1 the positive and then the negative term
 *   anchor i sends to r (gathered by the row's owner: no atomics) -- taken back through l2_normalize and ReLU as in
 *   fv_fid_triplet_loss_grad; loss_weight (finite, > 0) multiplies once where the value is rounded to float.  dE [M][64];
 *   dbias [64] = the column sums of the stored dE in fp64, in row order.
 * The same inputs give the same bits on every call.  Checked before anything is enqueued: a NULL buffer, M outside [1, 1024], a
 * mode other than 0 / 1, a margin or loss_weight that is not finite and > 0 is FV_ERR_INVALID and leaves the outputs untouched. */
int fv_fid_batch_triplet_loss_grad(fv_ctx* ctx, const float* pre, const float* u, const int32_t* subjects, int M, double margin,
                                   int mode, double loss_weight, float* loss, float* dE, float* dbias, int32_t* pos_index,
                                   int32_t* neg_index, int32_t* kind, double* d_ap, double* d_an);
/* One training step on a labelled batch: x [M][S][S][3] and subjects [M] (device) go through ONE tower -- the 52 base layers in
 * training-mode BN over all M images (one set of batch statistics, one update of the moving statistics: with
 * fv_set_bn_zero_debias_step(ctx, k) update k alone), the dense layer and l2_normalize over the M rows,
 * fv_fid_batch_triplet_loss_grad with loss_weight 1, the dense gradients and one backward of the base.  `grads` (the
 * fv_fid_param_count layout) is overwritten; loss and the five selection outputs are device buffers as above.  M: the batch bound
 * of fv_fid_extract and at most 1024, both checked before anything is enqueued.  Reproducibility as fv_fid_train_step. */
size_t fv_fid_batch_workspace_bytes(int M, int image_size);
int fv_fid_batch_train_step(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const int32_t* subjects, int M,
                            int image_size, int mode, double margin, void* workspace, size_t workspace_bytes, float* grads,
                            float* loss, int32_t* pos_index, int32_t* neg_index, int32_t* kind, double* d_ap, double* d_an);
/* Softmax over the subjects with an additive margin (CosFace: Wang et al. 2018; ArcFace: Deng et al. 2019) and its gradients.
 * Device inputs: pre / u [M][64] float as the dense call returns them, labels [M] int32 (a class in [0, C), < 0: an unknown
 * identity), W [C][64] float, the class kernel; u, W and the workspace 16-byte aligned.  1 <= M <= 1024, 1 <= C <= 32768; kind 0
 * CosFace, 1 ArcFace; scale s finite and > 0; margin m finite, 0 < m < 1 (kind 0) or 0 < m < pi / 2 (kind 1); loss_weight finite
 * and > 0.  Device outputs: loss [1], dE [M][64], dbias [64], dW [C][64] float, pred [M] int32, cos_t [M] double.
 * Everything is computed in fp64 and every stored float is rounded once.
 *   w^_c = w_c * 1 / sqrt(max(sum_k w_ck^2, 1e-12)) (the l2_normalize rule; the factor is the constant 1e6 where the sum is <=
 *   1e-12); cos_ic = sum_k u_ik w^_ck; pred[i] = argmax_c cos_ic, the lowest c among equals, for every row.
 *   A row with y = labels[i] >= 0: cos_t[i] = cos_iy; t = clamp(cos_iy, -1, 1), whose derivative is 1 where -1 <= cos_iy <= 1, else 0.
 *   kind 0: psi = t - m, psi' = 1.  kind 1: q = 1 - t^2, sin = sqrt(max(q, 1e-12)); if t > cos(pi - m): psi = t cos m - sin sin m,
 *   psi' = cos m + (q > 1e-12 ? t sin m / sin : 0); otherwise psi = t - m sin(pi - m), psi' = 1 (keeps psi monotone).
 *   logits z_ic = s cos_ic for c != y, z_iy = s psi; row loss = logsumexp_c(z_i) - z_iy (the row maximum subtracted);
 *   loss = (1 / V) sum over the V rows with a label >= 0.  A row with a label < 0: cos_t one quiet NaN, nothing added anywhere.
 *   A label >= C cannot be refused without a sync: the row is treated as label < 0 and pred[i] = -2.
 *   V == 0: loss 0, all gradients exactly 0, FV_OK.
 *   gradients, p the softmax of z_i: g_ic = (p_ic - [c = y]) s / V, times psi' clamp' for c = y; dU_i = sum_c g_ic w^_c;
 *   dE_i = dU_i taken back through l2_normalize and ReLU as in fv_fid_triplet_loss_grad, loss_weight multiplying once where the
 *   value is rounded; dbias = the column sums of the STORED dE rows (fp64); dW^_c = sum_i g_ic u_i; dW_c = inv_c (dW^_c - w^_c
 *   (w^_c . dW^_c)) where sum w^2 > 1e-12, else dW^_c 1e6, times loss_weight.  dW is stored, not accumulated.
 * No atomics: the same inputs give the same bits on every call.  The summation orders over k, c and i are the build's.
 * workspace: fv_fid_margin_workspace_bytes(M, C) bytes (0 for an M or C out of range); it keeps the [M][C] coefficients g.
 * Checked before anything is enqueued: a NULL buffer, M / C / kind / scale / margin / loss_weight out of range or a misaligned
 * buffer is FV_ERR_INVALID, a workspace that is too small FV_ERR_WORKSPACE; the outputs are left untouched. */
size_t fv_fid_margin_workspace_bytes(int M, int C);
int fv_fid_margin_softmax_loss_grad(fv_ctx* ctx, const float* pre, const float* u, const int32_t* labels, int M, const float* W, int C,
                                    int kind, double scale, double margin, double loss_weight, void* workspace,
                                    size_t workspace_bytes, float* loss, float* dE, float* dbias, float* dW, int32_t* pred,
                                    double* cos_t);
/* One training step on a labelled batch with the margin softmax: fv_fid_batch_train_step with the loss exchanged for
 * fv_fid_margin_softmax_loss_grad (loss_weight 1) over class_kernel [C][64] (device, 16-byte aligned).  One tower, one update of
 * the moving statistics.  `grads` (the fv_fid_param_count layout) and class_grads [C][64] are overwritten; loss, pred and cos_t
 * are device buffers as above.  Refusals as both operators', before anything is enqueued. */
size_t fv_fid_cls_workspace_bytes(int M, int C, int image_size);
int fv_fid_cls_train_step(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const int32_t* labels, int M,
                          int image_size, const float* class_kernel, int C, int kind, double scale, double margin, void* workspace,
                          size_t workspace_bytes, float* grads, float* class_grads, float* loss, int32_t* pred, double* cos_t);
/* dX = dE . w^T ([M][64] x [F][64]^T) stored into the towers' rows; each element one fp32 chain over the 64 columns in order. */
int fv_fid_towers_dense_dgrad(fv_ctx* ctx, const float* dE, int M, int64_t F, const float* w, float* dx0, float* dx1, float* dx2,
                              int per);
/* dw [F][64] = X^T . dE over the M rows, stored; each element one fp32 chain over the rows in order. */
int fv_fid_towers_dense_wgrad(fv_ctx* ctx, const float* x0, const float* x1, const float* x2, int per, const float* dE, int M,
                              int64_t F, float* dw);
/* Nearest registered facial ID (FaceIdentifier.test, fi.py:1117-1127: `norm(anchor - reg)` per subject, then np.argmin):
 * queries [n][64] and registry [m][64] float32 (device; registry 16-byte aligned) -> best_index int32 [n] and best_dist
 * float64 [n] (device).  Distance: sqrt of the fp64 sum, in dimension order 0..63, of the squared fp64 differences.  The
 * winner is the lexicographic minimum of (distance, index) -- equal distances go to the lowest index, as np.argmin -- so the
 * result does not depend on n, on the rest of the batch or on how the work is split: any split of the queries gives the same
 * bits.  No atomics.  m == 0 is FV_ERR_INVALID.  The similarity threshold (hps.sim_th) is applied by the caller. */
int fv_fid_match(fv_ctx* ctx, const float* queries, int n, const float* registry, int m, int32_t* best_index, double* best_dist);
/* Face-verification pair distances (evaluate.py:129-194 cal_face_pairs_dists, 196-223 cal_VAL_FAR): one block per subject or
 * subject pair over the rows of ids [n_ids][64] float32 (device, 16-byte aligned).  kind 0: the i < j triangle of rows
 * a0..a0+na-1 (b0 == a0, nb == na; the same-identity pairs of evaluate.py:143-159); kind 1: the na x nb rectangle of rows
 * a0.. and b0.. (the different-identity pairs of evaluate.py:166-187, k's file outer).  A pair's distance goes to
 * dists[out_off + rank] -- rank i*na - i*(i+1)/2 + (j-i-1) in a triangle, i*nb + j in a rectangle: the reference's append order --
 * and is sqrt of the fp64 sum, in dimension order 0..63, of the squared fp64 differences, rounded to float32 (fv_fid_match's
 * numerics), whatever the block order or launch split.  counts [2][n_th] int64 (device, overwritten): counts[kind][t] = pairs of
 * that kind with float32 distance <= thresholds[t] (host, ascending, 1 <= n_th <= 4096; NaN counts nowhere); integer sums, so
 * deterministic.  dists == NULL: counts only (n_dists ignored).  The whole table is checked before anything is enqueued: a row
 * range outside n_ids, a bad kind or triangle shape, out_off + pairs > n_dists or unsorted thresholds is FV_ERR_INVALID and
 * leaves dists and counts untouched.  Returns after the table has been uploaded (the call waits for the stream once). */
typedef struct {
    int64_t a0, na, b0, nb, out_off;
    int32_t kind, pad;
} fv_pair_block;
int fv_fid_pair_dists(fv_ctx* ctx, const float* ids, int64_t n_ids, const fv_pair_block* blocks, int n_blocks,
                      const float* thresholds, int n_th, float* dists, int64_t n_dists, int64_t* counts);
/* Triplet negatives mined from the current facial IDs (semi-hard mining, FaceNet section 3.2; the reference draws its negatives
 * at random, once).  ids [n][64] float32 and subjects [n] int32 (device; ids 16-byte aligned).  The triplets are a group table on
 * the host: anchors [g], pos_off [g + 1] ascending from 0 to t, positives [t]; triplet j of group q is (anchors[q], positives[j])
 * for pos_off[q] <= j < pos_off[q + 1].  Outputs (device, one per triplet): neg_index int32, kind int32, d_ap and d_an float64.
 *   D(i, r) = sqrt of the fp64 sum, in dimension order 0..63, of the squared fp64 differences (fv_fid_match's numerics);
 *   dap = D(a, p);  hi = dap + margin (one fp64 add);  row r is eligible for anchor a iff subjects[r] >= 0 and subjects[r] !=
 *   subjects[a];  a row whose D(a, r) is NaN belongs to no class.
 *   mode 0 (semi-hard): the first class that is not empty --
 *     kind 0  eligible rows with dap < D < hi:  the minimum of (D, r);
 *     kind 1  eligible rows with D <= dap:      the largest D, the lowest r among equals (the mildest violating negative);
 *     kind 2  eligible rows with D >= hi:       the minimum of (D, r);
 *     kind 3  none, or dap is NaN:              neg_index -1, d_an +inf.
 *   mode 1 (hardest): the minimum of (D, r) over the eligible rows whose D is not NaN; kind says by the same three inequalities
 *     where that row fell; kind 3 as above.
 * d_ap is dap (one quiet NaN, sign and payload clear, when it is NaN); d_an is the chosen row's D.  Every choice is an extremum
 * under a total order: a triplet's outputs depend on ids, subjects, a, p, margin and mode alone, not on the grouping, the launch
 * split or the other triplets.  No atomics.  A group longer than FV_MINE_PB positives is served in parts of that many, each part
 * one scan of the rows.  The whole table is checked before anything is enqueued: n < 1, t < 0, an index outside [0, n), offsets
 * that do not ascend from 0 to t, a mode other than 0 / 1 or a margin that is not finite and > 0 is FV_ERR_INVALID and leaves
 * the outputs untouched.  t == 0 writes nothing.  Returns after the table has been uploaded (the call waits for the stream once). */
#define FV_MINE_PB 8
int fv_fid_mine_negatives(fv_ctx* ctx, const float* ids, const int32_t* subjects, int n, const int32_t* anchors,
                          const int32_t* pos_off, int g, const int32_t* positives, int t, double margin, int mode,
                          int32_t* neg_index, int32_t* kind, double* d_ap, double* d_an);

/* ------------------------------------------------------------------ FaceIdentifier: the reconstruction model
 * create_face_reconst_model (fi.py:1155-1488): a facial ID [64] back through the network to an image [S][S][3].
 *   head : u = relu(l2_normalize(ids)) (x * rsqrt(max(sum x^2, 1e-12)));  x = u . K^T + b, K the dense1 kernel [F][64],
 *          b [F];  reshaped to [g][g][1024] NHWC, g = S / 32, F = g^2 * 1024;  skip = x.
 *   stage(l), l a base layer (Cin -> Cout, k, stride):  y = BN_l(l2_normalize_channels(leaky_relu(x, 0.1))) over the Cout
 *          channels of every pixel (same rsqrt(max(., 1e-12)): an all-zero pixel stays zero; BN_l inference-mode with eps 1e-3
 *          and its OWN gamma / beta / mean / variance), then x = Conv2DTranspose(Cin, k, strides, 'same', no bias) of y with layer
 *          l's kernel.  Stride 1: the layer's data-gradient (fv_conv2d_dgrad).  Stride 2: out[h] = sum_{2i + r = h} in[i] w[r],
 *          r = 0..2, the gradient of a 'same'-padded ((0, 1)) stride-2 conv -- NOT the data-gradient of this network's stride-2
 *          layers, which pad (1, 1) (sum_{2i + r - 1 = h}).
 *   order: layers 51 .. 2: a stride-2 layer is one stage, then skip = x; the others come as a residual block's 3x3 then its 1x1:
 *          two stages, then x = x - skip, skip = x.  Then stage(1), stage(0); no activation on the [S][S][3] output.
 * Flat parameter layout: the 52 conv kernels at their fv_layer w_off (the gamma / beta slots between them are unused), then K
 * [F][64], then b [F], then per layer l = 0..51 gamma, beta, moving mean, moving variance of ITS BN ([4][Cout_l], layers in order).
 * Keras itself is not importable in this build's environment: the model is pinned against a float64 restatement of the above. */
int64_t fv_recon_param_count(int image_size);   /* 0 unless image_size is a positive multiple of 32 */
size_t fv_recon_workspace_bytes(int batch, int image_size);
/* ids [batch][64] -> out [batch][S][S][3].  The transposed kernel images and the folded BN scale / shift are made in the workspace
 * on EVERY call (nothing is cached in the context: `params` may change between calls); three rotating activation buffers; the
 * tail-split scratch of the conv launcher is lent out of the workspace for the call.  No atomics: the same call gives the same
 * bits.  Batch bound as fv_forward_infer (batch * S * S * 32 < 2^29). */
int fv_recon_forward(fv_ctx* ctx, const float* params, const float* ids, int batch, int image_size, void* workspace,
                     size_t workspace_bytes, float* out);
/* The model's kernels as single operators (parity tests).
 * fv_recon_dense_head: ids [rows][64] -> u [rows][64] = relu(l2_normalize(ids)) and out [rows][F] = u . w^T + bias, w [F][64],
 *   bias [F], F % 256 == 0; each element one fp32 chain over the 64 columns in order, the bias added last.
 * fv_l2norm_affine: rows pixels of C floats, C one of 32, 64, 128, 256, 512, 1024 (FV_ERR_INVALID otherwise, nothing written):
 *   d = x - skip (skip NULL: d = x), l = leaky_relu(d, leaky), y = l * (1 / sqrt(max(sum_c l^2, 1e-12))) * scale[c] + shift[c].
 *   d_out (may be NULL) receives d and may be x itself; y must be a buffer of its own.  A pixel's bits do not depend on rows.
 * fv_conv2d_transpose: x [B][Hin][Win][cout] -> out [B][Hin*stride][Win*stride][cin] = Conv2DTranspose(cin, ksize, stride, 'same')
 *   with the kernel of a conv layer cin -> cout given as its fv_transpose_weights image w_t [cin][ksize^2][cout]; cout % 32 == 0.
 *   ksize 1 / stride 1 and ksize 3 / stride 1 or 2 (the stride-2 alignment described above).  cin == 3 (needs cout == 32,
 *   ksize 3, stride 1, Hin % 8 == 0, Win % 32 == 0) runs the direct vector-FMA kernel; any other cin the matrix-core tiles. */
int fv_recon_dense_head(fv_ctx* ctx, const float* ids, int rows, int64_t F, const float* w, const float* bias, float* u, float* out);
int fv_l2norm_affine(fv_ctx* ctx, const float* x, const float* skip, float* d_out, const float* scale, const float* shift,
                     float* y, int64_t rows, int C, float leaky);
int fv_conv2d_transpose(fv_ctx* ctx, const float* x, const float* w_t, int B, int Hin, int Win, int cin, int cout, int ksize,
                        int stride, float* out);

/* ------------------------------------------------------------------ secondary: three-scale YOLOv3
 * (SURVEY 8a-17/18).  The reference builds this graph in make_yolov3_model (yd.py:217-311) and
 * runs it only from yolov3_detect.py:_main_ (COCO demo: yd.py:596-598 decode, do_nms); FaceDetector
 * discards it.  Inference only.  Flat layout: the 52 base layers exactly as fv_layer(0..51), then
 * the 23 layers 75..105 (fv_yolov3_layer: role 4 = conv+BN+leaky, role 5 = detection conv with bias
 * at beta_off, linear).  out_channels = 3*(5+classes) (255 for COCO). */
int fv_yolov3_num_layers(void);                                   /* 75 */
int fv_yolov3_layer(int i, int out_channels, fv_layer_desc* out);
int64_t fv_yolov3_param_count(int out_channels);                  /* 61 949 149 at 255 */
int64_t fv_yolov3_state_count(int out_channels);                  /* 52 608 */
size_t fv_yolov3_workspace_bytes(int batch, int image_size, int out_channels);
/* replaces yolov3.predict (yd.py:590): y13/y26/y52 = [batch][S/32|S/16|S/8]^2[out_channels] */
int fv_yolov3_forward(fv_ctx* ctx, const float* params, const float* bn_state, const float* x, int batch,
                      int image_size, int out_channels, void* workspace, size_t workspace_bytes,
                      float* y13, float* y26, float* y52);
/* TRAINING the three-scale graph (SURVEY 8f row 4 -- "three-scale YOLO head + bbox/objectness loss" of the
 * north star; the reference builds this graph for inference only and defines no loss for it, so this is the
 * build's own definition, restated in oracle/net_oracle.py).  One step's forward (training-mode BN in all 72
 * BN layers, moving statistics updated) + loss + backward through the heads, both UpSampling2D+concatenate
 * routes and the base; gradients of every parameter of the fv_yolov3_layer layout into `grads` (overwritten).
 * yt13 / yt26 / yt52: targets shaped like the outputs, [batch][g][g][3][5+classes].  Loss = sum over the
 * three scales of the mean over (cell, anchor) of
 *     ( bce(t4, y4) + mean_{k<4} |t_k - y_k| + mean_c bce(t_{5+c}, y_{5+c}) ) / 3
 * -- the reference's fd_loss (fd.py:59-64) generalised to 3 anchors and `classes` classes, with the
 * cross-entropies on logits: bce(t, y) = max(t,0) - t*y + log1p(exp(-|t|)).  Follow with fv_adam_step.
 * loss_weight: as in fv_train_step (scales the gradient, not the reported loss).
 * on_bucket (may be NULL): as in fv_train_step -- called on the host as the gradient range of a layer completes, in reverse
 * execution order = descending offsets, contiguous, covering every parameter once (data-parallel overlap of the all-reduce). */
size_t fv_yolov3_train_workspace_bytes(int batch, int image_size, int out_channels);
int fv_yolov3_train_step(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const float* yt13,
                         const float* yt26, const float* yt52, int batch, int image_size, int out_channels,
                         void* workspace, size_t workspace_bytes, float* grads, float* loss, double loss_weight,
                         fv_bucket_fn on_bucket, void* user);
/* as fv_train_workspace_tensor, for the workspace of fv_yolov3_train_step (BN layers of fv_yolov3_layer) */
int fv_yolov3_train_workspace_tensor(int batch, int image_size, int out_channels, int layer, int which,
                                     size_t* offset_bytes, int64_t* count);
/* the head tensors either training step leaves in its workspace: which = 0 the raw output y of scale `scale` (0 = the coarsest
 * grid), [batch g^2][out_channels]; which = 1 its gradient dy, [batch g^2][c_pad] with c_pad = out_channels rounded up to 32 */
int fv_yolov3_train_workspace_head(int batch, int image_size, int out_channels, int scale, int which,
                                   size_t* offset_bytes, int64_t* count);
/* ---- YOLOv3 detection loss for the three-scale head (not in the reference, which never trains this graph; an
 * additive part of ABI version 4).  Replaces the loss STAGE of fv_yolov3_train_step: ignore mask, box regression on assigned
 * slots only, box term in keras-yolo3's form or as 1 - GIoU.
 * Tensors: y_s (raw head outputs) and t_s (targets of data.encode_gt_three_scale) are dense [batch][g_s][g_s][3][5+ncls] with
 * g_s = image_size/32 << s, entries [tx, ty, tw, th, obj, cls...]; dy_s is [batch g_s^2][c_pad], c_pad >= 3*(5+ncls), its
 * padding columns written as exactly 0.  cell_s = 32 >> s network pixels; (aw, ah) = anchors[6 s + 2 a], anchors[6 s + 2 a + 1].
 * (a) Gather: per image, the slots with t4 == 1 of all three scales in slot order (scale, row, column, anchor) form a list of
 *     boxes (cx, cy, w, h) = ((col + sigma(t0)) cell, (row + sigma(t1)) cell, aw e^t2, ah e^t3); the first max_boxes are kept,
 *     the true count is recorded.
 * (b) Per slot: the predicted box ((col + sigma(y0)) cell, (row + sigma(y1)) cell, aw e^c2, ah e^c3), c = clamp(y, -20, 20);
 *     best = max IoU with the listed boxes of the same image (0 for an empty list).  With bce(x, z) = max(x,0) - x z +
 *     log1p(e^-|x|) on the logit x:
 *       assigned slot (t4 == 1):  bce(y4, 1) + sum_c bce(y_{5+c}, t_{5+c}) + box_weight * box term against the slot's OWN
 *                                 target box (so a box cut from the list still trains its slot);
 *       unassigned slot:          0 when best > ignore_thresh, else noobj_weight * bce(y4, 0)   (the mask carries no gradient).
 *     box term, box_loss = FV_DET_BOX_L2 (keras-yolo3), s = 2 - w h / image_size^2 of the target box:
 *           s (bce(y0, sigma(t0)) + bce(y1, sigma(t1))) + 0.5 s ((y2 - t2)^2 + (y3 - t3)^2);
 *     box_loss = FV_DET_BOX_GIOU: 1 - GIoU(predicted, target), differentiated through the decode; an entry with |y| >= 20
 *     (at the clamp) gets gradient 0.
 * loss (device float) = the sum over every slot of every scale / batch, unweighted; dy = loss_weight * d loss / d y.
 * stats (12 device doubles): [0..3] the loss parts box (with box_weight), objectness of the assigned slots, no-object (with
 * noobj_weight), class -- each / batch, their sum is the loss; [4] assigned slots; [5] ignored unassigned slots; [6] sum of
 * IoU(predicted, target) over the assigned slots; [7], [8] assigned slots with that IoU > 0.5, > 0.75; [9] the largest
 * per-image box count; [10] boxes dropped by the cap, summed over the images; [11] 0 (spare).
 * fp64 inside; per-workgroup partial sums added in a fixed order: deterministic, two runs are bit-identical.
 * scratch: fv_yolo_det_scratch_bytes(batch, image_size, max_boxes) bytes of device memory, 8-byte aligned, owned by the caller
 * (0 for a bad argument).  FV_ERR_INVALID before any launch for: NULL buffers, ignore_thresh outside (0, 1], box_weight /
 * noobj_weight / loss_weight not finite or <= 0, max_boxes outside [1, 1024], unknown box_loss, anchors not finite or <= 0,
 * c_pad < 3*(5+ncls), image_size not a multiple of 32, a scratch buffer that is too small. */
#define FV_DET_BOX_L2 0
#define FV_DET_BOX_GIOU 1
typedef struct {
    int32_t box_loss;      /* FV_DET_BOX_L2 / FV_DET_BOX_GIOU */
    float ignore_thresh;   /* (0, 1] */
    float box_weight;      /* > 0 */
    float noobj_weight;    /* > 0 */
    int32_t max_boxes;     /* 1 .. 1024 listed boxes per image */
    float anchors[18];     /* network pixels, scale 0 (the coarsest grid) first, (w, h) per anchor */
} fv_yolo_det_conf;
size_t fv_yolo_det_scratch_bytes(int batch, int image_size, int max_boxes);
/* yp3 / yt3 / dy3: HOST arrays of three DEVICE pointers, scale 0 first (as fv_yolo_loss_grad) */
int fv_yolo_det_loss_grad(fv_ctx* ctx, const float* const* yp3, const float* const* yt3, int batch, int image_size, int ncls,
                          int c_pad, const fv_yolo_det_conf* conf, double loss_weight, void* scratch, size_t scratch_bytes,
                          float* loss, float* const* dy3, double* stats);
/* fv_yolov3_train_step with this loss in place of its loss stage: the same forward, backward, workspace
 * (fv_yolov3_train_workspace_bytes) and arguments, plus conf, the scratch buffer above and stats.  The activations and the BN
 * state it leaves are those of fv_yolov3_train_step bit for bit. */
int fv_yolov3_train_step_det(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const float* yt13,
                             const float* yt26, const float* yt52, int batch, int image_size, int out_channels,
                             void* workspace, size_t workspace_bytes, float* grads, float* loss, double loss_weight,
                             fv_bucket_fn on_bucket, void* user, const fv_yolo_det_conf* conf, void* scratch,
                             size_t scratch_bytes, double* stats);
/* replaces decode_netout x3 (yd.py:335-387, with its anchor skip list), correct_yolo_boxes
 * (yd.py:389-404) and do_nms (yd.py:426-444) for ONE image: outputs in the reference's list order;
 * boxes [capacity][4] int32 xmin,ymin,xmax,ymax in image pixels, objness [capacity],
 * classes [capacity][nclass] (suppressed entries zeroed), count (device int).  anchors18: host
 * floats, scale 0 first.  A zero-area pair (ZeroDivisionError in the reference) does not suppress.
 * capacity: 1..8192 rows of the output buffers (the per-class sort of one image runs in the LDS of one
 * workgroup), for ANY grid0; FV_ERR_INVALID outside that range, outputs untouched.  An image has 25 grid0^2
 * candidate slots: 4225 at grid 13, 8100 at 18, 9025 at 19 (608 input).  With more candidates than capacity the
 * first `capacity` of the list are written, count = capacity, and the NMS runs over those rows only; so
 * count == capacity < 25 grid0^2 tells the caller that the list may have been cut.  The Python wrappers pass
 * min(25 grid0^2, 8192) and raise on that condition instead of returning a shortened list. */
int fv_yolo_decode_nms(fv_ctx* ctx, const float* y13, const float* y26, const float* y52, int grid0, int nclass,
                       const float* anchors18, float obj_thresh, double nms_thresh, int net_h, int net_w,
                       int image_h, int image_w, int capacity, int32_t* boxes, float* objness, float* classes,
                       int32_t* count);

/* The same for a BATCH of images of one size (the driver loop of yd.py:596-604 runs the chain image by image): outputs
 * [nimg][g][g][3*(5+nclass)] per scale, boxes [nimg][capacity][4], objness [nimg][capacity], classes [nimg][capacity][nclass],
 * count [nimg] -- one launch pair for the whole batch (workgroup = image in the decode, (class, image) in the NMS). */
int fv_yolo_decode_nms_batch(fv_ctx* ctx, const float* y13, const float* y26, const float* y52, int nimg, int grid0, int nclass,
                             const float* anchors18, float obj_thresh, double nms_thresh, int net_h, int net_w,
                             int image_h, int image_w, int capacity, int32_t* boxes, float* objness, float* classes,
                             int32_t* count);

/* fd_loss (fd.py:59-64) -- DEFINED BUT NEVER USED by the reference (every compile() passes
 * loss='mse', fd.py:335/366/370/381); provided as an operator only, not wired into fv_train_step.
 * yp, yt [cells][6]; per cell (BCE(y0,p0) + mean_{c=1..4} sqrt((y_c-p_c)^2) + BCE(y5,p5))/3 with
 * Keras' probability-space binary_crossentropy (p clipped to [1e-7, 1-1e-7]); loss = mean over
 * cells; dy [cells][c_pad] its gradient (0 outside the clip range and at y_c == p_c). */
int fv_fd_loss_grad(fv_ctx* ctx, const float* yp, const float* yt, int cells, int c_pad, float* loss,
                    float* dy);

#ifdef __cplusplus
}
#endif
#endif /* FV_HOTPATH_H */
