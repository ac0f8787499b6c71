// Network-level schedule: the FaceDetector model (Darknet-53 base as wired by reference
// face_detection.py:404-593 over yolov3_detect.py:221-267, head face_detection.py:348-352),
// inference forward and the training step (forward, MSE, backward) as a fixed sequence of kernel
// launches on one HIP stream.  The layer table (net_plan.h) is derived from the stage structure
// (filters, residual blocks) rather than transcribed.
#include "net_plan.h"

extern "C" {

int fv_num_layers(void) { return (int)net().L.size(); }
int fv_layer(int i, fv_layer_desc* out) {
    if (!out || i < 0 || i >= (int)net().L.size()) return FV_ERR_INVALID;
    *out = net().L[i];
    return FV_OK;
}
int64_t fv_param_count(void) { return net().nparam; }
int64_t fv_state_count(void) { return net().nstate; }

size_t fv_workspace_bytes(int batch, int image_size, int training) {
    if (batch < 1 || image_size < 32 || image_size % 32) return 0;
    return make_plan(nullptr, batch, image_size, training != 0).bytes;
}

int fv_train_workspace_tensor(int batch, int image_size, int layer, int which, size_t* offset_bytes, int64_t* count) {
    if (!offset_bytes || !count || batch < 1 || image_size < 32 || image_size % 32) return FV_ERR_INVALID;
    const Net& N = net();
    if (layer < 0 || layer >= (int)N.L.size() - 1 || which < 0 || which > 5) return FV_ERR_INVALID;
    char* const base = (char*)(uintptr_t)65536;   // any non-null base: only differences are used
    const Plan p = make_plan(base, batch, image_size, true);
    return kept_tensor(p.k, base, N.L[layer], layer, which, batch, image_size, offset_bytes, count);
}

int fv_train_bn_in_1x1_plan(int option, int batch, int image_size, int32_t* folded, int n) {
    const Net& N = net();
    if (!folded || n != (int)N.L.size() || batch < 1 || image_size < 32 || image_size % 32) return FV_ERR_INVALID;
    bn_in_plan(N.L, option, batch, image_size, folded);
    return FV_OK;
}

// inference forward: the 52 base layers (the last one into `feat` when given), then the head into `y` when given
static int forward_impl(fv_ctx* ctx, const char* who, const float* params, const float* bn_state, const float* x, int batch,
                        int image_size, void* workspace, size_t workspace_bytes, float* feat, float* y) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, params && bn_state && x && workspace && (y || feat), "%s: NULL buffer", who);
    if (int rc = check_batch(ctx, who, batch, image_size)) return rc;
    Plan p = make_plan(workspace, batch, image_size, false);
    if (p.bytes > workspace_bytes) return fv_fail(ctx, FV_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, p.bytes);
    TailLend lend(ctx, p.tail, p.tail_floats);
    const Net& N = net();
    const int nb = p.nl - 1;
    if (int rc = fold_bn(ctx, N.L, params, bn_state, p.k.scale[0], p.k.shift[0])) return rc;
    if (int rc = fv_ew_pad_rows(ctx, params + N.L[0].w_off, p.w0p, 32, 27, 32)) return rc;
    const Infer f{ctx, params, batch, image_size, p.w0p, p.k.scale[0], p.k.shift[0], p.slab};
    std::vector<float*> out_at;
    if (feat) { out_at.assign(nb, nullptr); out_at[nb - 1] = feat; }
    const float* cur; int icur;
    if (int rc = base_infer(f, N.L, nb, x, p.G, out_at, &cur, &icur)) return rc;
    return y ? infer_conv(f, N.L[nb], cur, nullptr, y) : FV_OK;
}

int fv_forward_infer(fv_ctx* ctx, const float* params, const float* bn_state, const float* x, int batch, int image_size,
                     void* workspace, size_t workspace_bytes, float* y) {
    if (ctx && !y) return fv_fail(ctx, FV_ERR_INVALID, "forward_infer: NULL buffer");
    return forward_impl(ctx, "forward_infer", params, bn_state, x, batch, image_size, workspace, workspace_bytes, nullptr, y);
}

int fv_forward_base(fv_ctx* ctx, const float* params, const float* bn_state, const float* x, int batch, int image_size,
                    void* workspace, size_t workspace_bytes, float* feat, float* y) {
    if (ctx && !feat) return fv_fail(ctx, FV_ERR_INVALID, "forward_base: NULL buffer");
    return forward_impl(ctx, "forward_base", params, bn_state, x, batch, image_size, workspace, workspace_bytes, feat, y);
}

int fv_train_step(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const float* y_true, int batch,
                  int image_size, void* workspace, size_t workspace_bytes, float* grads, float* loss, double loss_weight,
                  fv_bucket_fn on_bucket, void* user) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, params && bn_state && x && y_true && workspace && grads && loss, "train_step: NULL buffer");
    FV_REQUIRE(ctx, loss_weight > 0.0 && loss_weight <= 1.0, "train_step: loss_weight must be in (0, 1] (the slice's share of the merged batch)");
    if (int rc = check_batch(ctx, "train_step", batch, image_size)) return rc;
    Plan p = make_plan(workspace, batch, image_size, true);
    if (p.bytes > workspace_bytes) return fv_fail(ctx, FV_ERR_WORKSPACE, "train_step: workspace %zu < %zu bytes", workspace_bytes, p.bytes);
    TailLend lend(ctx, p.tail, p.tail_floats);
    EmaReset ema_reset{ctx};
    const Net& N = net();
    const int nb = p.nl - 1;
    const Train t{ctx, N.L, p.k, batch, image_size, params, bn_state, grads};

    if (int rc = train_step_begin(ctx, N.L, params, grads, N.nparam, {&p.k}, p.w0p, HEAD_PAD)) return rc;
    // ---------------- forward (training-mode BN)
    if (int rc = base_train_forward(t, nb, x, p.w0p)) return rc;
    if (int rc = train_bn_forward_end(t)) return rc;
    // the head conv has 6 output channels: K-split like the batch-1 inference path (conv_small and conv_bm64 never take it)
    const auto& h = N.L[nb];
    if (int rc = infer_conv(Infer{ctx, params, batch, image_size, nullptr, nullptr, nullptr, p.head_slab}, h, p.k.a[nb - 1], nullptr, p.yhat)) return rc;
    // ---------------- loss + its gradient (fd.py:381 'mse')
    const int G = image_size / h.in_div;
    if (int rc = fv_ew_mse(ctx, p.yhat, y_true, batch * G * G, HEAD_C, HEAD_PAD, loss, p.dyp, grads + h.beta_off, (double*)p.mse_part,
                          loss_weight)) return rc;

    // ---------------- backward: dz of the layers alternates between G[2] and G[3]
    WgradPipe pipe(t, on_bucket, user, p.G[2], p.G[3]);
    // head: its bias gradient was written by the loss kernel above (compute stream, before ev_dz is recorded)
    if (int rc = linear_layer_backward(pipe, nb, nb - 1, p.dyp, HEAD_PAD, p.G[0])) return rc;
    if (int rc = base_backward(pipe, nb, x, p.G, {})) return rc;
    return pipe.finish();
}

}  // extern "C"
