// Network-level schedule of the FaceIdentifier (reference face_identification.py:318-345, 378-395): the Darknet-53 base of the
// FaceDetector (net_plan.h), Flatten, Dense(64, relu), l2_normalize -- facial-ID extraction, and the triplet-loss training step that
// runs the shared base three times (anchor, positive, negative) in training-mode BN.
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

// Three training plans, one per tower (kept z / a, BN statistics, accumulator slots, gradient buffers of its own); only the
// anchor's carries the weight images, which the other two share.  Then the dense layer's rows, tower-major.
struct TrainWs { Plan t[3]; float *part, *pre, *u, *dE; size_t bytes; };
TrainWs make_train(void* base, int B, int S) {
    TrainWs w{};
    size_t off = 0;
    for (int i = 0; i < 3; ++i) {
        w.t[i] = make_plan(at(base, off), B, S, true, i == 0);
        off = (off + w.t[i].bytes + 255) & ~(size_t)255;
    }
    Carver c = carver_at(base, off);
    const size_t rows = (size_t)3 * B;
    w.part = c.take((size_t)fv_fid_chunks(feat_floats(S)) * rows * FID_DIM);
    w.pre = c.take(rows * FID_DIM);
    w.u = c.take(rows * FID_DIM);
    w.dE = c.take(rows * FID_DIM);
    w.bytes = c.off;
    return w;
}

// One training plan over the M images of a labelled batch, then the dense layer's M rows and the loss's selection.
struct BatchWs { Plan t; float *part, *pre, *u, *dE; size_t bytes; };
BatchWs make_batch(void* base, int M, int S) {
    BatchWs w{};
    w.t = make_plan(base, M, S, true);
    Carver c = carver_at(base, w.t.bytes);
    w.part = c.take((size_t)fv_fid_chunks(feat_floats(S)) * M * FID_DIM);
    w.pre = c.take((size_t)M * FID_DIM);
    w.u = c.take((size_t)M * FID_DIM);
    w.dE = c.take((size_t)M * FID_DIM);
    w.bytes = c.off;
    return w;
}

}  // namespace

extern "C" {

int64_t fv_fid_param_count(int image_size) {
    if (image_size < 32 || image_size % 32) return 0;
    return base_param_count() + feat_floats(image_size) * FID_DIM + FID_DIM;
}

size_t fv_fid_workspace_bytes(int batch, int image_size, int training) {
    if (batch < 1 || image_size < 32 || image_size % 32) return 0;
    return training ? make_train(nullptr, batch, image_size).bytes : make_extract(nullptr, batch, image_size).bytes;
}

size_t fv_fid_batch_workspace_bytes(int M, int image_size) {
    if (M < 1 || M > FID_BATCH_MAX || image_size < 32 || image_size % 32) return 0;
    return make_batch(nullptr, M, image_size).bytes;
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
    TrainWs w = make_train(workspace, batch, image_size);
    if (w.bytes > workspace_bytes) return fv_fail(ctx, FV_ERR_WORKSPACE, "fid_train_step: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    Plan& pa = w.t[0];
    TailLend lend(ctx, pa.tail, pa.tail_floats);   // the towers run one after another: one tail-split scratch serves all three
    const long long step0 = ctx->bn_ema_step;
    EmaReset ema_reset{ctx};
    const Net& N = net();
    const long long F = feat_floats(image_size);
    const int64_t dense_off = base_param_count();
    const float* x[3] = {xa, xp, xn};

    FV_HIP(ctx, hipMemsetAsync(grads, 0, (size_t)fv_fid_param_count(image_size) * sizeof(float), ctx->stream));
    for (auto& p : w.t) FV_HIP(ctx, hipMemsetAsync(p.k.slots[0], 0, p.k.slots_bytes, ctx->stream));
    // weight images of this step, made once and shared by the three towers
    if (int rc = fv_ew_pad_rows(ctx, params + N.L[0].w_off, pa.w0p, 32, 27, 32)) return rc;
    if (int rc = transpose_weights(ctx, N.L, params, pa.k.wt, HEAD_PAD)) return rc;
    for (int i = 1; i < 3; ++i) { w.t[i].w0p = pa.w0p; w.t[i].k.wt = pa.k.wt; }

    // ---------------- forward of the towers a, p, n: each normalises with its own batch statistics and applies its own update of
    // the moving statistics, in this order (zero-debiased: updates step0, step0 + 1, step0 + 2)
    for (int i = 0; i < 3; ++i) {
        ctx->bn_ema_step = step0 > 0 ? step0 + i : 0;
        const Train t{ctx, N.L, w.t[i].k, batch, image_size, params, bn_state, grads, true};
        const float* cur = x[i];
        const float* skip = nullptr;
        for (int l = 0; l < NB; ++l) {
            const auto& d = N.L[l];
            if (d.role == 1) skip = cur;
            if (int rc = train_bn_forward(t, l, cur, l == 0 ? pa.w0p : params + d.w_off, d.role == 2 ? skip : nullptr)) return rc;
            cur = w.t[i].k.a[l];
        }
        if (int rc = train_bn_forward_end(t)) return rc;
    }
    // ---------------- dense + l2_normalize over the 3B rows (read in place from the towers' top activations), loss, dense gradients
    const FidRows X{{w.t[0].k.a[NB - 1], w.t[1].k.a[NB - 1], w.t[2].k.a[NB - 1]}, batch};
    const int M = 3 * batch;
    if (int rc = fv_fid_dense_fwd(ctx, X, M, F, params + dense_off, w.part)) return rc;
    if (int rc = fv_fid_dense_finish(ctx, w.part, fv_fid_chunks(F), M, params + dense_off + F * FID_DIM, w.pre, w.u)) return rc;
    if (int rc = fv_fid_triplet(ctx, w.pre, w.u, batch, loss, w.dE, grads + dense_off + F * FID_DIM, loss_weight)) return rc;
    if (int rc = fv_fid_dense_wgrad(ctx, X, w.dE, M, F, grads + dense_off)) return rc;
    // The dense ranges are complete here (no tower adds to them): bias, then kernel, before any base backward starts.  They were
    // made on the context's stream; a callback that works on the side stream (fv_set_bucket_on_side) is ordered behind them by an
    // event first.
    if (on_bucket) {
        if (ctx->overlap && ctx->side && ctx->bucket_on_side) {
            FV_HIP(ctx, hipEventRecord(ctx->ev_dz[0], ctx->stream));
            FV_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_dz[0], 0));
        }
        on_bucket(user, dense_off + F * FID_DIM, FID_DIM);
        on_bucket(user, dense_off, F * FID_DIM);
    }
    if (int rc = fv_fid_dense_dgrad(ctx, w.dE, M, F, params + dense_off, FidRows{{w.t[0].G[0], w.t[1].G[0], w.t[2].G[0]}, batch})) return rc;

    // ---------------- backward of each tower into the same gradient vector: conv weight-gradients accumulate (float atomics), BN
    // d-beta / d-gamma are added (accumulate_bn); the top layer's BN reduction is not fused into the dense data-gradient.  A base
    // range is complete only when the LAST tower's share of it is in the queue: the third pass alone reports (both streams are in
    // order, so that tower's weight-gradient and BN-backward of a layer lie behind the other two towers')
    for (int i = 0; i < 3; ++i) {
        const Train t{ctx, N.L, w.t[i].k, batch, image_size, params, bn_state, grads, true};
        WgradPipe pipe(t, i == 2 ? on_bucket : nullptr, user, w.t[i].G[2], w.t[i].G[3]);
        if (int rc = base_backward(pipe, NB, x[i], w.t[i].G, {}, false)) return rc;
        if (int rc = pipe.finish()) return rc;
    }
    return FV_OK;
}

}  // extern "C"

namespace {

// One tower over the M images of a labelled batch: forward in training-mode BN (one update of the moving statistics: update
// ctx->bn_ema_step, as the caller set it), the dense layer and l2_normalize over the M rows, `loss_call(w, dbias)` -- which
// enqueues the loss on w.pre / w.u and writes w.dE and the dense bias gradient --, the dense gradients and one backward of the base.
template <class LossCall>
int labelled_batch_step(fv_ctx* ctx, const float* params, float* bn_state, const float* x, int M, int image_size, BatchWs& w,
                        float* grads, LossCall&& loss_call) {
    Plan& p = w.t;
    TailLend lend(ctx, p.tail, p.tail_floats);
    EmaReset ema_reset{ctx};
    const Net& N = net();
    const long long F = feat_floats(image_size);
    const int64_t dense_off = base_param_count();

    FV_HIP(ctx, hipMemsetAsync(grads, 0, (size_t)fv_fid_param_count(image_size) * sizeof(float), ctx->stream));
    FV_HIP(ctx, hipMemsetAsync(p.k.slots[0], 0, p.k.slots_bytes, ctx->stream));
    if (int rc = fv_ew_pad_rows(ctx, params + N.L[0].w_off, p.w0p, 32, 27, 32)) return rc;
    if (int rc = transpose_weights(ctx, N.L, params, p.k.wt, HEAD_PAD)) return rc;

    // accumulate_bn as fv_fid_train_step sets it: d-beta / d-gamma are added to the zeroed vector
    const Train t{ctx, N.L, p.k, M, image_size, params, bn_state, grads, true};
    const float* cur = x;
    const float* skip = nullptr;
    for (int l = 0; l < NB; ++l) {
        const auto& d = N.L[l];
        if (d.role == 1) skip = cur;
        if (int rc = train_bn_forward(t, l, cur, l == 0 ? p.w0p : params + d.w_off, d.role == 2 ? skip : nullptr)) return rc;
        cur = p.k.a[l];
    }
    if (int rc = train_bn_forward_end(t)) return rc;
    const FidRows X{{p.k.a[NB - 1], nullptr, nullptr}, M};
    if (int rc = fv_fid_dense_fwd(ctx, X, M, F, params + dense_off, w.part)) return rc;
    if (int rc = fv_fid_dense_finish(ctx, w.part, fv_fid_chunks(F), M, params + dense_off + F * FID_DIM, w.pre, w.u)) return rc;
    if (int rc = loss_call(w, grads + dense_off + F * FID_DIM)) return rc;
    if (int rc = fv_fid_dense_wgrad(ctx, X, w.dE, M, F, grads + dense_off)) return rc;
    if (int rc = fv_fid_dense_dgrad(ctx, w.dE, M, F, params + dense_off, FidRows{{p.G[0], nullptr, nullptr}, M})) return rc;
    WgradPipe pipe(t, nullptr, nullptr, p.G[2], p.G[3]);
    if (int rc = base_backward(pipe, NB, x, p.G, {}, false)) return rc;
    return pipe.finish();
}

}  // namespace

extern "C" {

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
    BatchWs w = make_batch(workspace, M, image_size);
    if (w.bytes > workspace_bytes)
        return fv_fail(ctx, FV_ERR_WORKSPACE, "fid_batch_train_step: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    return labelled_batch_step(ctx, params, bn_state, x, M, image_size, w, grads, [&](BatchWs& b, float* dbias) {
        return fv_fid_batch_triplet(ctx, b.pre, b.u, subjects, M, margin, mode, 1.0, loss, b.dE, dbias, pos_index, neg_index, kind, d_ap,
                                    d_an);
    });
}

size_t fv_fid_cls_workspace_bytes(int M, int C, int image_size) {
    const size_t loss_bytes = fv_fid_margin_ws_bytes(M, C);
    if (!loss_bytes || image_size < 32 || image_size % 32) return 0;
    return carver_at(nullptr, make_batch(nullptr, M, image_size).bytes).off + loss_bytes;
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
    BatchWs w = make_batch(workspace, M, image_size);
    const size_t loss_off = carver_at(nullptr, w.bytes).off, loss_bytes = fv_fid_margin_ws_bytes(M, C);
    if (loss_off + loss_bytes > workspace_bytes)
        return fv_fail(ctx, FV_ERR_WORKSPACE, "fid_cls_train_step: workspace %zu < %zu bytes", workspace_bytes, loss_off + loss_bytes);
    return labelled_batch_step(ctx, params, bn_state, x, M, image_size, w, grads, [&](BatchWs& b, float* dbias) {
        return fv_fid_margin_softmax(ctx, b.pre, b.u, labels, M, class_kernel, C, kind, scale, margin, 1.0, (char*)workspace + loss_off,
                                     loss_bytes, loss, b.dE, dbias, class_grads, pred, cos_t);
    });
}

}  // extern "C"
