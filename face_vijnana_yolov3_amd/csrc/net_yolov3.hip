// Secondary path: the full three-scale YOLOv3 inference graph of the reference's
// make_yolov3_model (yolov3_detect.py:217-311), reached only from yolov3_detect.py:_main_ (COCO
// demo), never by FaceDetector.  Base layers 0..73 are the FaceDetector base (same kernels, same
// flat layout); layers 75..105 add the 13/26/52 heads with two UpSampling2D(2)+concatenate routes.
// Inference only (the reference defines no training loss for it).
#include "schedule.h"
#include "yolo_det_loss.h"

namespace {

enum Src { PREV = 0, BASE, ROUTE79, ROUTE91, CAT61, CAT36 };

struct YNet {
    Layers L;            // role: 0/1/2 as the base; 4 = extra conv+BN+leaky; 5 = detection conv (bias, linear)
    std::vector<int> src;
    int64_t nparam = 0, nstate = 0;
    int nbase = 0;
    explicit YNet(int out_ch) {
        const int nb = fv_num_layers() - 1;   // base layers of the FaceDetector table (head excluded)
        for (int i = 0; i < nb; ++i) {
            fv_layer_desc d{}; fv_layer(i, &d);
            L.push_back(d); src.push_back(PREV);
            nparam = d.beta_off + d.cout; nstate = d.var_off + d.cout;
        }
        nbase = nb;
        auto add = [&](int idx, int k, int cin, int cout, bool bn, int from, int div) {
            fv_layer_desc d{};
            d.darknet_index = idx; d.ksize = k; d.stride = 1; d.cin = cin; d.cout = cout; d.has_bn = bn ? 1 : 0;
            d.role = bn ? 4 : 5; d.in_div = div; d.out_div = div;
            d.w_off = nparam; nparam += (int64_t)cout * k * k * cin;
            if (bn) {
                d.gamma_off = nparam; nparam += cout; d.beta_off = nparam; nparam += cout;
                d.mean_off = nstate; nstate += cout; d.var_off = nstate; nstate += cout;
            } else {
                d.gamma_off = -1; d.beta_off = nparam; nparam += cout; d.mean_off = d.var_off = -1;
            }
            L.push_back(d); src.push_back(from);
        };
        // 13x13 branch: five alternating 1x1/3x3, then 3x3 + detection 1x1 (yd.py:269-278)
        int c = 1024;
        const int b13[5][3] = {{75, 1, 512}, {76, 3, 1024}, {77, 1, 512}, {78, 3, 1024}, {79, 1, 512}};
        for (int i = 0; i < 5; ++i) { add(b13[i][0], b13[i][1], c, b13[i][2], true, i == 0 ? BASE : PREV, 32); c = b13[i][2]; }
        add(80, 3, 512, 1024, true, PREV, 32);
        add(81, 1, 1024, out_ch, false, PREV, 32);
        add(84, 1, 512, 256, true, ROUTE79, 32);          // yd.py:281-283 (+ upsample, concat skip_61)
        c = 768;
        const int b26[5][3] = {{87, 1, 256}, {88, 3, 512}, {89, 1, 256}, {90, 3, 512}, {91, 1, 256}};
        for (int i = 0; i < 5; ++i) { add(b26[i][0], b26[i][1], c, b26[i][2], true, i == 0 ? CAT61 : PREV, 16); c = b26[i][2]; }
        add(92, 3, 256, 512, true, PREV, 16);
        add(93, 1, 512, out_ch, false, PREV, 16);
        add(96, 1, 256, 128, true, ROUTE91, 16);          // yd.py:297-299 (+ upsample, concat skip_36)
        c = 384;
        const int b52[6][3] = {{99, 1, 128}, {100, 3, 256}, {101, 1, 128}, {102, 3, 256}, {103, 1, 128}, {104, 3, 256}};
        for (int i = 0; i < 6; ++i) { add(b52[i][0], b52[i][1], c, b52[i][2], true, i == 0 ? CAT36 : PREV, 8); c = b52[i][2]; }
        add(105, 1, 256, out_ch, false, PREV, 8);
    }
};

const YNet& ynet(int out_ch) {
    static YNet n255(255);
    static std::vector<std::pair<int, YNet*>> others;
    if (out_ch == 255) return n255;
    for (auto& o : others) if (o.first == out_ch) return *o.second;
    others.push_back({out_ch, new YNet(out_ch)});
    return *others.back().second;
}

struct YPlan {
    float *scale, *shift, *w0p, *G[3], *s36, *s61, *r79, *r91, *cat, *slab;
    size_t bytes;
};

YPlan yplan(void* base, const YNet& N, int B, int S) {
    YPlan p{};
    Carver c(base);
    p.scale = c.take((size_t)N.nstate / 2); p.shift = c.take((size_t)N.nstate / 2);
    p.w0p = c.take(32 * 32);
    size_t max_act = 0;
    for (const auto& d : N.L) max_act = std::max(max_act, (size_t)B * (S / d.out_div) * (S / d.out_div) * d.cout);
    for (int i = 0; i < 3; ++i) p.G[i] = c.take(max_act);
    p.s36 = c.take((size_t)B * (S / 8) * (S / 8) * 256);
    p.s61 = c.take((size_t)B * (S / 16) * (S / 16) * 512);
    p.r79 = c.take((size_t)B * (S / 32) * (S / 32) * 512);
    p.r91 = c.take((size_t)B * (S / 16) * (S / 16) * 256);
    p.cat = c.take(std::max((size_t)B * (S / 8) * (S / 8) * 384, (size_t)B * (S / 16) * (S / 16) * 768));
    p.slab = c.take_some(ksplit_slab_floats(N.L, B, S));
    p.bytes = c.off;
    return p;
}

// ---------------------------------------------------------------------------------------------- training plan
// Everything the backward pass needs is kept: per BN layer z (pre-BN) and a (activated), the two concatenated
// tensors, the three raw head outputs and their padded gradients.
struct YTrain {
    Kept k;
    float *w0p, *cat61, *cat36, *y[3], *dy[3], *GA, *GB, *DZ, *DZ2, *gs61, *gs36, *r79, *r91, *loss_part, *colsum_part, *tail;
    size_t tail_floats = 0, bytes = 0;
    int cpad = 0;
};

YTrain ytrain_plan(void* base, const YNet& N, int B, int S, int out_ch) {
    YTrain p{};
    Carver c(base);
    const int nl = (int)N.L.size();
    p.k.resize(nl);
    p.cpad = (out_ch + 31) / 32 * 32;
    size_t max_act = 0;
    for (int l = 0; l < nl; ++l) {
        const auto& d = N.L[l];
        const size_t elems = (size_t)B * (S / d.out_div) * (S / d.out_div) * d.cout;
        if (d.has_bn) {
            p.k.z[l] = c.take(elems); p.k.a[l] = c.take(elems);
            p.k.mean[l] = c.take(d.cout); p.k.invstd[l] = c.take(d.cout); p.k.scale[l] = c.take(d.cout); p.k.shift[l] = c.take(d.cout);
            max_act = std::max(max_act, elems);
        }
        if (l > 0) p.k.wt[l] = c.take((size_t)d.cin * d.ksize * d.ksize * (d.has_bn ? d.cout : p.cpad));
    }
    p.k.carve_slots(c, N.L);
    p.w0p = c.take(32 * 32);
    const size_t cat61 = (size_t)B * (S / 16) * (S / 16) * 768, cat36 = (size_t)B * (S / 8) * (S / 8) * 384;
    p.cat61 = c.take(cat61); p.cat36 = c.take(cat36);
    max_act = std::max({max_act, cat61, cat36});
    for (int s = 0; s < 3; ++s) {
        const size_t rows = (size_t)B * (S / (32 >> s)) * (S / (32 >> s));
        p.y[s] = c.take(rows * out_ch); p.dy[s] = c.take(rows * p.cpad);
    }
    p.GA = c.take(max_act); p.GB = c.take(max_act); p.DZ = c.take(max_act); p.DZ2 = c.take(max_act);
    p.gs61 = c.take((size_t)B * (S / 16) * (S / 16) * 512); p.gs36 = c.take((size_t)B * (S / 8) * (S / 8) * 256);
    p.r79 = c.take((size_t)B * (S / 32) * (S / 32) * 512); p.r91 = c.take((size_t)B * (S / 16) * (S / 16) * 256);
    p.loss_part = c.take(2 * 3 * 1024 + 64);
    p.colsum_part = c.take(2 * 64 * (size_t)p.cpad);
    p.tail_floats = tail_split_floats(N.L, B, S, true, p.cpad);
    p.tail = c.take_some(p.tail_floats);
    p.bytes = c.off;
    return p;
}

int find_base(const YNet& N, int darknet_idx) {
    for (int l = 0; l < N.nbase; ++l) if (N.L[l].darknet_index == darknet_idx) return l;
    return -1;
}

}  // namespace

extern "C" {

int fv_yolov3_num_layers(void) { return (int)ynet(255).L.size(); }
int fv_yolov3_layer(int i, int out_channels, fv_layer_desc* out) {
    const YNet& N = ynet(out_channels);
    if (!out || i < 0 || i >= (int)N.L.size()) return FV_ERR_INVALID;
    *out = N.L[i];
    return FV_OK;
}
int64_t fv_yolov3_param_count(int out_channels) { return ynet(out_channels).nparam; }
int64_t fv_yolov3_state_count(int out_channels) { return ynet(out_channels).nstate; }
size_t fv_yolov3_workspace_bytes(int batch, int image_size, int out_channels) {
    if (batch < 1 || image_size < 32 || image_size % 32 || out_channels < 1) return 0;
    return yplan(nullptr, ynet(out_channels), batch, image_size).bytes;
}

int fv_yolov3_forward(fv_ctx* ctx, const float* params, const float* bn_state, const float* x, int batch, int image_size,
                      int out_channels, void* workspace, size_t workspace_bytes, float* y13, float* y26, float* y52) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, params && bn_state && x && workspace && y13 && y26 && y52, "yolov3_forward: NULL buffer");
    if (int rc = check_batch(ctx, "yolov3_forward", batch, image_size)) return rc;
    FV_REQUIRE(ctx, out_channels >= 1, "yolov3_forward: bad shape");
    const YNet& N = ynet(out_channels);
    const int S = image_size;
    YPlan p = yplan(workspace, N, batch, S);
    if (p.bytes > workspace_bytes) return fv_fail(ctx, FV_ERR_WORKSPACE, "yolov3_forward: workspace %zu < %zu bytes", workspace_bytes, p.bytes);
    if (int rc = fold_bn(ctx, N.L, params, bn_state, p.scale, p.shift)) return rc;
    if (int rc = fv_ew_pad_rows(ctx, params + N.L[0].w_off, p.w0p, 32, 27, 32)) return rc;
    const Infer f{ctx, params, batch, S, p.w0p, p.scale, p.shift, p.slab};

    // ---- base (rotating buffers; the two routed block outputs go to dedicated buffers)
    std::vector<float*> out_at(N.nbase, nullptr);
    out_at[find_base(N, 35)] = p.s36;
    out_at[find_base(N, 60)] = p.s61;
    const float* base_out;
    int ibase;
    if (int rc = base_infer(f, N.L, N.nbase, x, p.G, out_at, &base_out, &ibase)) return rc;
    // ---- heads
    const float* prev = base_out;
    int iprev = ibase;
    for (size_t l = N.nbase; l < N.L.size(); ++l) {
        const auto& d = N.L[l];
        const int src = N.src[l];
        const float* in = prev;
        if (src == BASE) in = base_out;
        else if (src == ROUTE79) in = p.r79;
        else if (src == ROUTE91) in = p.r91;
        else if (src == CAT61 || src == CAT36) {
            // UpSampling2D(2) of the previous 1x1 output, concatenated in front of the routed skip
            const int Hs = S / (src == CAT61 ? 32 : 16), C1 = src == CAT61 ? 256 : 128, C2 = src == CAT61 ? 512 : 256;
            if (int rc = fv_ew_upsample_concat(ctx, prev, src == CAT61 ? p.s61 : p.s36, p.cat, batch, Hs, Hs, C1, C2)) return rc;
            in = p.cat;
        }
        float* out;
        int iout = -1;
        if (d.role == 5) out = d.in_div == 32 ? y13 : (d.in_div == 16 ? y26 : y52);
        else if (d.darknet_index == 79) out = p.r79;
        else if (d.darknet_index == 91) out = p.r91;
        else {
            iout = 0;
            while (iout == iprev || iout == ibase) ++iout;   // keep the base output alive until conv_75 consumed it
            out = p.G[iout];
        }
        if (int rc = infer_conv(f, d, in, nullptr, out)) return rc;
        if (d.role != 5) { prev = out; iprev = iout; }
        else { prev = nullptr; iprev = -1; }
    }
    return FV_OK;
}

size_t fv_yolov3_train_workspace_bytes(int batch, int image_size, int out_channels) {
    if (batch < 1 || image_size < 32 || image_size % 32 || out_channels < 1 || out_channels % 3) return 0;
    return ytrain_plan(nullptr, ynet(out_channels), batch, image_size, out_channels).bytes;
}

int fv_yolov3_train_bn_in_1x1_plan(int option, int batch, int image_size, int out_channels, int32_t* folded, int n) {
    if (!folded || batch < 1 || image_size < 32 || image_size % 32 || out_channels < 18 || out_channels % 3) return FV_ERR_INVALID;
    const YNet& N = ynet(out_channels);
    if (n != (int)N.L.size()) return FV_ERR_INVALID;
    bn_in_plan(N.L, option, batch, image_size, folded);
    return FV_OK;
}

int fv_yolov3_train_workspace_tensor(int batch, int image_size, int out_channels, int layer, int which, size_t* offset_bytes,
                                     int64_t* count) {
    if (!offset_bytes || !count || batch < 1 || image_size < 32 || image_size % 32 || out_channels < 18 || out_channels % 3) return FV_ERR_INVALID;
    const YNet& N = ynet(out_channels);
    if (layer < 0 || layer >= (int)N.L.size() || which < 0 || which > 5 || !N.L[layer].has_bn) return FV_ERR_INVALID;
    char* const base = (char*)(uintptr_t)65536;
    const YTrain p = ytrain_plan(base, N, batch, image_size, out_channels);
    return kept_tensor(p.k, base, N.L[layer], layer, which, batch, image_size, offset_bytes, count);
}

int fv_yolov3_train_workspace_head(int batch, int image_size, int out_channels, int scale, int which, size_t* offset_bytes,
                                   int64_t* count) {
    if (!offset_bytes || !count || batch < 1 || image_size < 32 || image_size % 32 || out_channels < 18 || out_channels % 3) return FV_ERR_INVALID;
    if (scale < 0 || scale > 2 || which < 0 || which > 1) return FV_ERR_INVALID;
    char* const base = (char*)(uintptr_t)65536;
    const YTrain p = ytrain_plan(base, ynet(out_channels), batch, image_size, out_channels);
    const int64_t rows = (int64_t)batch * (image_size / (32 >> scale)) * (image_size / (32 >> scale));
    *offset_bytes = (size_t)((char*)(which ? p.dy[scale] : p.y[scale]) - base);
    *count = rows * (which ? p.cpad : out_channels);
    return FV_OK;
}

// One body for fv_yolov3_train_step (det == nullptr: the fd_loss generalisation) and fv_yolov3_train_step_det (the YOLOv3 detection
// loss of yolo_det_loss.hip): the same forward and backward, only the loss stage differs.
static int yolov3_train_step_body(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const float* yt13, const float* yt26,
                                  const float* yt52, int batch, int image_size, int out_channels, void* workspace, size_t workspace_bytes,
                                  float* grads, float* loss, double loss_weight, fv_bucket_fn on_bucket, void* user,
                                  const fv_yolo_det_conf* det, void* det_scratch, size_t det_scratch_bytes, double* det_stats) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, loss_weight > 0.0 && loss_weight <= 1.0, "yolov3_train_step: loss_weight must be in (0, 1]");
    FV_REQUIRE(ctx, params && bn_state && x && yt13 && yt26 && yt52 && workspace && grads && loss, "yolov3_train_step: NULL buffer");
    if (int rc = check_batch(ctx, "yolov3_train_step", batch, image_size)) return rc;
    FV_REQUIRE(ctx, out_channels >= 18 && out_channels % 3 == 0, "yolov3_train_step: bad shape (out_channels = 3*(5+classes))");
    if (det) {
        if (int rc = fv_det_check(ctx, "yolov3_train_step_det", det, batch, image_size, out_channels / 3 - 5, (out_channels + 31) / 32 * 32,
                                  det_scratch, det_scratch_bytes, det_stats)) return rc;
    }
    const YNet& N = ynet(out_channels);
    const int S = image_size, B = batch, nl = (int)N.L.size(), nb = N.nbase;
    const int ncls = out_channels / 3 - 5;
    YTrain p = ytrain_plan(workspace, N, B, S, out_channels);
    if (p.bytes > workspace_bytes) return fv_fail(ctx, FV_ERR_WORKSPACE, "yolov3_train_step: workspace %zu < %zu bytes", workspace_bytes, p.bytes);
    TailLend lend(ctx, p.tail, p.tail_floats);
    EmaReset ema_reset{ctx};
    const Train t{ctx, N.L, p.k, B, S, params, bn_state, grads};

    if (int rc = train_step_begin(ctx, N.L, params, grads, N.nparam, {&p.k}, p.w0p, p.cpad)) return rc;
    const int l35 = find_base(N, 35), l60 = find_base(N, 60);
    const int P79 = nb + 4, P80 = nb + 5, D13 = nb + 6, P84 = nb + 7, P87 = nb + 8, P91 = nb + 12, P92 = nb + 13, D26 = nb + 14, P96 = nb + 15,
              P99 = nb + 16, P104 = nb + 21, D52 = nb + 22;
    FV_REQUIRE(ctx, l35 >= 0 && l60 >= 0 && D52 == nl - 1 && N.L[P79].darknet_index == 79 && N.L[P91].darknet_index == 91 &&
                        N.L[P84].darknet_index == 84 && N.L[P96].darknet_index == 96 && N.L[P104].darknet_index == 104,
               "yolov3_train_step: unexpected layer table");

    // ------------------------------------------------------------------ forward (training-mode BN everywhere)
    auto input_of = [&](int l) -> const float* {
        if (l == 0) return x;
        switch (N.src[l]) {
            case BASE: return p.k.a[nb - 1];
            case ROUTE79: return p.k.a[P79];
            case ROUTE91: return p.k.a[P91];
            case CAT61: return p.cat61;
            case CAT36: return p.cat36;
            default: return p.k.a[l - 1];
        }
    };
    const float* skip = nullptr;
    for (int l = 0; l < nl; ++l) {
        const auto& d = N.L[l];
        const int H = S / d.in_div;
        if (N.src[l] == CAT61) { if (int rc = fv_ew_upsample_concat(ctx, p.k.a[P84], p.k.a[l60], p.cat61, B, S / 32, S / 32, 256, 512)) return rc; }
        if (N.src[l] == CAT36) { if (int rc = fv_ew_upsample_concat(ctx, p.k.a[P96], p.k.a[l35], p.cat36, B, S / 16, S / 16, 128, 256)) return rc; }
        const float* in = input_of(l);
        if (d.role == 1) skip = in;
        const float* w = l == 0 ? p.w0p : params + d.w_off;
        if (d.has_bn) {
            if (int rc = train_bn_forward(t, l, in, w, d.role == 2 ? skip : nullptr)) return rc;
        } else {
            const int sidx = d.in_div == 32 ? 0 : (d.in_div == 16 ? 1 : 2);
            if (int rc = fv_op_conv_forward(ctx, in, w, B, H, H, d.cin, d.cout, d.ksize, d.stride, FV_EPI_AFFINE, nullptr, params + d.beta_off,
                                            0.f, nullptr, p.y[sidx], nullptr, nullptr)) return rc;
        }
    }
    if (int rc = train_bn_forward_end(t)) return rc;
    // ------------------------------------------------------------------ loss of the three scales, its gradient, bias gradients
    const float* yt[3] = {yt13, yt26, yt52};
    const int dconv[3] = {D13, D26, D52};
    long long cells[3];
    double* lpart = (double*)p.loss_part;
    for (int s = 0; s < 3; ++s) cells[s] = (long long)B * (S / (32 >> s)) * (S / (32 >> s));
    if (det) {
        if (int rc = fv_det_loss_launch(ctx, p.y, yt, B, S, ncls, p.cpad, det, loss_weight, det_scratch, loss, p.dy, det_stats)) return rc;
        for (int s = 0; s < 3; ++s)
            if (int rc = fv_ew_colsum(ctx, p.dy[s], cells[s], out_channels, p.cpad, (double*)p.colsum_part, grads + N.L[dconv[s]].beta_off)) return rc;
    } else {
        int off = 0;
        for (int s = 0; s < 3; ++s) {
            if (int rc = fv_ew_yolo_loss_part(ctx, p.y[s], yt[s], cells[s], ncls, 3, p.cpad, p.dy[s], lpart + off, loss_weight)) return rc;
            off += fv_ew_yolo_loss_blocks(cells[s] * 3);
            if (int rc = fv_ew_colsum(ctx, p.dy[s], cells[s], out_channels, p.cpad, (double*)p.colsum_part, grads + N.L[dconv[s]].beta_off)) return rc;
        }
        if (int rc = fv_ew_yolo_loss_finish(ctx, lpart, cells, 3, loss)) return rc;
    }
    // ------------------------------------------------------------------ backward
    // bn_layer_backward(pipe, l, g, reduced, xin, g_out, addend, lred): lred = -1 where the gradient of l's input is not complete
    // yet or is a concatenation's
    WgradPipe pipe(t, on_bucket, user, p.DZ, p.DZ2);
    const auto& a = p.k.a;
    float *ga = p.GA, *gb = p.GB;
    auto bn_chain = [&](int hi, int lo) -> int {   // layers hi .. lo+1 of a head branch, each reading its predecessor's output
        for (int l = hi; l > lo; --l) {
            if (int rc = bn_layer_backward(pipe, l, ga, true, a[l - 1], gb, nullptr, l - 1)) return rc;
            std::swap(ga, gb);
        }
        return FV_OK;
    };
    // 52x52 head
    if (int rc = linear_layer_backward(pipe, D52, P104, p.dy[2], p.cpad, ga)) return rc;
    if (int rc = bn_chain(P104, P99)) return rc;
    if (int rc = bn_layer_backward(pipe, P99, ga, true, p.cat36, gb, nullptr, -1)) return rc;
    if (int rc = fv_ew_upsample_concat_bwd(ctx, gb, ga, p.gs36, B, S / 16, S / 16, 128, 256)) return rc;       // ga = g(a96), gs36 = g(skip_36) part
    if (int rc = bn_layer_backward(pipe, P96, ga, false, a[P91], p.r91, nullptr, -1)) return rc;
    // 26x26 head
    if (int rc = linear_layer_backward(pipe, D26, P92, p.dy[1], p.cpad, ga)) return rc;
    if (int rc = bn_layer_backward(pipe, P92, ga, true, a[P91], gb, p.r91, P91)) return rc;
    std::swap(ga, gb);
    if (int rc = bn_chain(P91, P87)) return rc;
    if (int rc = bn_layer_backward(pipe, P87, ga, true, p.cat61, gb, nullptr, -1)) return rc;
    if (int rc = fv_ew_upsample_concat_bwd(ctx, gb, ga, p.gs61, B, S / 32, S / 32, 256, 512)) return rc;
    if (int rc = bn_layer_backward(pipe, P84, ga, false, a[P79], p.r79, nullptr, -1)) return rc;
    // 13x13 head
    if (int rc = linear_layer_backward(pipe, D13, P80, p.dy[0], p.cpad, ga)) return rc;
    if (int rc = bn_layer_backward(pipe, P80, ga, true, a[P79], gb, p.r79, P79)) return rc;
    std::swap(ga, gb);
    if (int rc = bn_chain(P79, nb - 1)) return rc;     // down to conv_75, which reads the base output
    // base, with the two routed gradients joining where the forward pass branched off: conv_37 / conv_62 read the tensors that
    // were also routed to the 52x52 / 26x26 heads
    std::vector<const float*> addend_at(nb, nullptr);
    addend_at[l35] = p.gs36;
    addend_at[l60] = p.gs61;
    float* const g[2] = {ga, gb};
    if (int rc = base_backward(pipe, nb, x, g, addend_at)) return rc;
    return pipe.finish();
}

int fv_yolov3_train_step(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const float* yt13, const float* yt26,
                         const float* yt52, int batch, int image_size, int out_channels, void* workspace, size_t workspace_bytes,
                         float* grads, float* loss, double loss_weight, fv_bucket_fn on_bucket, void* user) {
    return yolov3_train_step_body(ctx, params, bn_state, x, yt13, yt26, yt52, batch, image_size, out_channels, workspace, workspace_bytes,
                                  grads, loss, loss_weight, on_bucket, user, nullptr, nullptr, 0, nullptr);
}

int fv_yolov3_train_step_det(fv_ctx* ctx, const float* params, float* bn_state, const float* x, const float* yt13, const float* yt26,
                             const float* yt52, int batch, int image_size, int out_channels, void* workspace, size_t workspace_bytes,
                             float* grads, float* loss, double loss_weight, fv_bucket_fn on_bucket, void* user,
                             const fv_yolo_det_conf* conf, void* scratch, size_t scratch_bytes, double* stats) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, conf && scratch && stats, "yolov3_train_step_det: NULL conf, scratch or stats");
    return yolov3_train_step_body(ctx, params, bn_state, x, yt13, yt26, yt52, batch, image_size, out_channels, workspace, workspace_bytes,
                                  grads, loss, loss_weight, on_bucket, user, conf, scratch, scratch_bytes, stats);
}

}  // extern "C"
