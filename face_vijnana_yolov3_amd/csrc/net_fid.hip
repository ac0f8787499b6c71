// Network-level schedule of the FaceIdentifier (reference face_identification.py:318-345, 378-395): the Darknet-53 base of the
// FaceDetector (net_plan.h), Flatten, Dense(64, relu), l2_normalize -- facial-ID extraction, and the training steps, all one schedule
// (tower_step) over towers of the shared base in training-mode BN: three (anchor, positive, negative) under the triplet loss, one
// over a labelled batch under the in-batch triplet loss or the margin softmax.
#include "fid.h"
#include "net_plan.h"

#include <cmath>

namespace {

constexpr int NB = 52;   // base layers: conv_0 .. the add_23 block

long long feat_floats(int S) { return (long long)(S / 32) * (S / 32) * 1024; }
int64_t base_param_count() { const auto& d = net().L[NB - 1]; return d.beta_off + d.cout; }

// Carves continue after `off` bytes of an earlier region (base == NULL: size query only).
Carver carver_at(void* base, size_t off) {
    Carver c(base);
    c.off = (off + 255) & ~(size_t)255;
    return c;
}
void* at(void* base, size_t off) { return base ? (char*)base + off : nullptr; }

struct ExtractWs { size_t infer_bytes; float *feat, *part; size_t bytes; };
ExtractWs make_extract(void* base, int B, int S) {
    ExtractWs w{};
    w.infer_bytes = make_plan(nullptr, B, S, false).bytes;   // fv_forward_base's own workspace comes first
    Carver c = carver_at(base, w.infer_bytes);
    w.feat = c.take((size_t)B * feat_floats(S));
    w.part = c.take((size_t)fv_fid_chunks(feat_floats(S)) * B * FID_DIM);
    w.bytes = c.off;
    return w;
}

// The workspace of a training step: one training plan per tower (kept z / a, BN statistics, accumulator slots, gradient buffers of
// its own), each starting at the 256-byte rounded end of the one before; only tower 0's carries the weight images, which the
// others share.  Then the dense layer's towers * rows rows, tower-major.  Three towers of B rows are the anchors, positives and
// negatives of the triplet step; one tower of M rows is a labelled batch.
struct StepWs { int towers, rows; Plan t[3]; float *part, *pre, *u, *dE; size_t bytes; };
StepWs make_step(void* base, int towers, int rows, int S) {
    StepWs w{};
    w.towers = towers; w.rows = rows;
    size_t off = 0;
    for (int i = 0; i < towers; ++i) {
        w.t[i] = make_plan(at(base, off), rows, S, true, i == 0);
        if (i) { w.t[i].w0p = w.t[0].w0p; w.t[i].k.wt = w.t[0].k.wt; }
        off = (off + w.t[i].bytes + 255) & ~(size_t)255;
    }
    Carver c = carver_at(base, off);
    const size_t M = (size_t)towers * rows;
    w.part = c.take((size_t)fv_fid_chunks(feat_floats(S)) * M * FID_DIM);
    w.pre = c.take(M * FID_DIM);
    w.u = c.take(M * FID_DIM);
    w.dE = c.take(M * FID_DIM);
    w.bytes = c.off;
    return w;
}

// One training step over w.towers towers of the shared base, tower i reading x[i]: the forward of each tower in training-mode BN,
// the dense layer and l2_normalize over all rows, `loss_call(w, dbias)` -- which enqueues the loss on w.pre / w.u and writes w.dE
// and the dense bias gradient --, the dense gradients and the backward of each tower into the one gradient vector.
template <class LossCall>
int tower_step(fv_ctx* ctx, const float* params, float* bn_state, const float* const* x, int image_size, StepWs& w, float* grads,
               fv_bucket_fn on_bucket, void* user, LossCall&& loss_call) {
    const int T = w.towers, M = T * w.rows;
    TailLend lend(ctx, w.t[0].tail, w.t[0].tail_floats);   // the towers run one after another: one tail-split scratch serves them all
    const long long step0 = ctx->bn_ema_step;
    EmaReset ema_reset{ctx};
    const Net& N = net();
    const long long F = feat_floats(image_size);
    const int64_t dense_off = base_param_count(), bias_off = dense_off + F * FID_DIM;
    // accumulate_bn: conv weight-gradients accumulate anyway (float atomics), d-beta / d-gamma are added to the zeroed vector
    auto tower = [&](int i) { return Train{ctx, N.L, w.t[i].k, w.rows, image_size, params, bn_state, grads, true}; };
    std::vector<const Kept*> kept;
    FidRows X{{}, w.rows}, dX{{}, w.rows};   // the dense layer reads the towers' top activations in place
    for (int i = 0; i < T; ++i) { kept.push_back(&w.t[i].k); X.p[i] = w.t[i].k.a[NB - 1]; dX.p[i] = w.t[i].G[0]; }

    if (int rc = train_step_begin(ctx, N.L, params, grads, fv_fid_param_count(image_size), kept, w.t[0].w0p, HEAD_PAD)) return rc;
    // ---------------- forward: each tower normalises with its own batch statistics and applies its own update of the moving
    // statistics, in this order (zero-debiased: updates step0, step0 + 1, ..)
    for (int i = 0; i < T; ++i) {
        ctx->bn_ema_step = step0 > 0 ? step0 + i : 0;
        const Train t = tower(i);
        if (int rc = base_train_forward(t, NB, x[i], w.t[0].w0p)) return rc;
        if (int rc = train_bn_forward_end(t)) return rc;
    }
    // ---------------- dense + l2_normalize, loss, dense gradients
    if (int rc = fv_fid_dense_fwd(ctx, X, M, F, params + dense_off, w.part)) return rc;
    if (int rc = fv_fid_dense_finish(ctx, w.part, fv_fid_chunks(F), M, params + bias_off, w.pre, w.u)) return rc;
    if (int rc = loss_call(w, grads + bias_off)) return rc;
    if (int rc = fv_fid_dense_wgrad(ctx, X, w.dE, M, F, grads + dense_off)) return rc;
    // The dense ranges are complete here (no tower adds to them): bias, then kernel, before any base backward starts.  They were
    // made on the context's stream; a callback that works on the side stream (fv_set_bucket_on_side) is ordered behind them by an
    // event first.
    if (on_bucket) {
        if (ctx->overlap && ctx->side && ctx->bucket_on_side) {
            FV_HIP(ctx, hipEventRecord(ctx->ev_dz[0], ctx->stream));
            FV_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_dz[0], 0));
        }
        on_bucket(user, bias_off, FID_DIM);
        on_bucket(user, dense_off, F * FID_DIM);
    }
    // the top layer's BN reduction is not fused into the dense data-gradient: base_backward(.., false) lets its BN-backward reduce
    if (int rc = fv_fid_dense_dgrad(ctx, w.dE, M, F, params + dense_off, dX)) return rc;
    // ---------------- backward of each tower.  A base range is complete only when the LAST tower's share of it is in the queue:
    // that pass alone reports (both streams are in order, so that tower's weight-gradient and BN-backward of a layer lie behind
    // the other towers')
    for (int i = 0; i < T; ++i) {
        const Train t = tower(i);
        WgradPipe pipe(t, i == T - 1 ? on_bucket : nullptr, user, w.t[i].G[2], w.t[i].G[3]);
        if (int rc = base_backward(pipe, NB, x[i], w.t[i].G, {}, false)) return rc;
        if (int rc = pipe.finish()) return rc;
    }
    return FV_OK;
}

}  // namespace

extern "C" {

int64_t fv_fid_param_count(int image_size) {
    if (image_size < 32 || image_size % 32) return 0;
    return base_param_count() + feat_floats(image_size) * FID_DIM + FID_DIM;
}

size_t fv_fid_workspace_bytes(int batch, int image_size, int training) {
    if (batch < 1 || image_size < 32 || image_size % 32) return 0;
    return training ? make_step(nullptr, 3, batch, image_size).bytes : make_extract(nullptr, batch, image_size).bytes;
}

size_t fv_fid_batch_workspace_bytes(int M, int image_size) {
    if (M < 1 || M > FID_BATCH_MAX || image_size < 32 || image_size % 32) return 0;
    return make_step(nullptr, 1, M, image_size).bytes;
}

int64_t fv_fid_dense_partial_floats(int rows, int64_t F) {
    if (rows < 1 || F <= 0 || F % FID_KC) return 0;
    return fv_fid_chunks(F) * rows * FID_DIM;
}

int fv_fid_dense_l2(fv_ctx* ctx, const float* x, int rows, int64_t F, const float* w, const float* bias, float* partial, float* pre,
                    float* out) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, x && w && bias && partial && out && rows >= 1, "fid_dense_l2: NULL buffer");
    const FidRows X{{(float*)x, nullptr, nullptr}, rows};
    if (int rc = fv_fid_dense_fwd(ctx, X, rows, F, w, partial)) return rc;
    return fv_fid_dense_finish(ctx, partial, fv_fid_chunks(F), rows, bias, pre, out);
}

int fv_fid_extract(fv_ctx* ctx, const float* params, const float* bn_state, const float* x, int batch, int image_size, void* workspace,
                   size_t workspace_bytes, float* fid) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, params && bn_state && x && workspace && fid, "fid_extract: NULL buffer");
    if (int rc = check_batch(ctx, "fid_extract", batch, image_size)) return rc;
    const ExtractWs w = make_extract(workspace, batch, image_size);
    if (w.bytes > workspace_bytes) return fv_fail(ctx, FV_ERR_WORKSPACE, "fid_extract: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    const long long F = feat_floats(image_size);
    const float* dense = params + base_param_count();
    if (int rc = fv_forward_base(ctx, params, bn_state, x, batch, image_size, workspace, w.infer_bytes, w.feat, nullptr)) return rc;
    if (int rc = fv_fid_dense_fwd(ctx, FidRows{{w.feat, nullptr, nullptr}, batch}, batch, F, dense, w.part)) return rc;
    return fv_fid_dense_finish(ctx, w.part, fv_fid_chunks(F), batch, dense + F * FID_DIM, nullptr, fid);
}

int fv_fid_train_step(fv_ctx* ctx, const float* params, float* bn_state, const float* xa, const float* xp, const float* xn, int batch,
                      int image_size, void* workspace, size_t workspace_bytes, float* grads, float* loss) {
    return fv_fid_train_step_dp(ctx, params, bn_state, xa, xp, xn, batch, image_size, workspace, workspace_bytes, grads, loss, 1.0,
                                nullptr, nullptr);
}

int fv_fid_train_step_dp(fv_ctx* ctx, const float* params, float* bn_state, const float* xa, const float* xp, const float* xn, int batch,
                         int image_size, void* workspace, size_t workspace_bytes, float* grads, float* loss, double loss_weight,
                         fv_bucket_fn on_bucket, void* user) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, params && bn_state && xa && xp && xn && workspace && grads && loss, "fid_train_step: NULL buffer");
    FV_REQUIRE(ctx, std::isfinite(loss_weight) && loss_weight > 0.0,
               "fid_train_step: loss_weight must be finite and > 0 (the slice's share of the merged batch)");
    if (int rc = check_batch(ctx, "fid_train_step", batch, image_size)) return rc;
    StepWs w = make_step(workspace, 3, batch, image_size);
    if (w.bytes > workspace_bytes) return fv_fail(ctx, FV_ERR_WORKSPACE, "fid_train_step: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    const float* x[3] = {xa, xp, xn};
    return tower_step(ctx, params, bn_state, x, image_size, w, grads, on_bucket, user, [&](StepWs& s, float* dbias) {
        return fv_fid_triplet(ctx, s.pre, s.u, batch, loss, s.dE, dbias, loss_weight);
    });
}

int fv_fid_batch_train_step(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const int32_t* subjects, int M,
                            int image_size, int mode, double margin, void* workspace, size_t workspace_bytes, float* grads, float* loss,
                            int32_t* pos_index, int32_t* neg_index, int32_t* kind, double* d_ap, double* d_an) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, params && bn_state && x && subjects && workspace && grads && loss && pos_index && neg_index && kind && d_ap && d_an,
               "fid_batch_train_step: NULL buffer");
    FV_REQUIRE(ctx, M <= FID_BATCH_MAX, "fid_batch_train_step: M %d beyond the loss's %d rows", M, FID_BATCH_MAX);
    FV_REQUIRE(ctx, mode == 0 || mode == 1, "fid_batch_train_step: mode %d (0 batch hard, 1 batch semi-hard)", mode);
    FV_REQUIRE(ctx, std::isfinite(margin) && margin > 0.0, "fid_batch_train_step: margin %g is not finite and > 0", margin);
    if (int rc = check_batch(ctx, "fid_batch_train_step", M, image_size)) return rc;
    StepWs w = make_step(workspace, 1, M, image_size);
    if (w.bytes > workspace_bytes)
        return fv_fail(ctx, FV_ERR_WORKSPACE, "fid_batch_train_step: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    return tower_step(ctx, params, bn_state, &x, image_size, w, grads, nullptr, nullptr, [&](StepWs& b, float* dbias) {
        return fv_fid_batch_triplet(ctx, b.pre, b.u, subjects, M, margin, mode, 1.0, loss, b.dE, dbias, pos_index, neg_index, kind, d_ap,
                                    d_an);
    });
}

size_t fv_fid_cls_workspace_bytes(int M, int C, int image_size) {
    const size_t loss_bytes = fv_fid_margin_ws_bytes(M, C);
    if (!loss_bytes || image_size < 32 || image_size % 32) return 0;
    return carver_at(nullptr, make_step(nullptr, 1, M, image_size).bytes).off + loss_bytes;
}

int fv_fid_cls_train_step(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const int32_t* labels, int M,
                          int image_size, const float* class_kernel, int C, int kind, double scale, double margin, void* workspace,
                          size_t workspace_bytes, float* grads, float* class_grads, float* loss, int32_t* pred, double* cos_t) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, params && bn_state && x && labels && class_kernel && workspace && grads && class_grads && loss && pred && cos_t,
               "fid_cls_train_step: NULL buffer");
    if (int rc = fv_fid_margin_check(ctx, "fid_cls_train_step", M, C, kind, scale, margin, 1.0)) return rc;
    FV_REQUIRE(ctx, (((uintptr_t)class_kernel | (uintptr_t)workspace) & 15) == 0,
               "fid_cls_train_step: the class kernel and the workspace must be 16-byte aligned");
    if (int rc = check_batch(ctx, "fid_cls_train_step", M, image_size)) return rc;
    StepWs w = make_step(workspace, 1, M, image_size);
    const size_t loss_off = carver_at(nullptr, w.bytes).off, loss_bytes = fv_fid_margin_ws_bytes(M, C);
    if (loss_off + loss_bytes > workspace_bytes)
        return fv_fail(ctx, FV_ERR_WORKSPACE, "fid_cls_train_step: workspace %zu < %zu bytes", workspace_bytes, loss_off + loss_bytes);
    return tower_step(ctx, params, bn_state, &x, image_size, w, grads, nullptr, nullptr, [&](StepWs& b, float* dbias) {
        return fv_fid_margin_softmax(ctx, b.pre, b.u, labels, M, class_kernel, C, kind, scale, margin, 1.0, (char*)workspace + loss_off,
                                     loss_bytes, loss, b.dE, dbias, class_grads, pred, cos_t);
    });
}

}  // extern "C"
