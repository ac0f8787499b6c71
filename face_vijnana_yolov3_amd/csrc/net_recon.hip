// Network-level schedule of the FaceIdentifier's reconstruction model (reference face_identification.py:1155-1488,
// create_face_reconst_model): a facial ID through the transposed dense1 layer and then through the 52 Darknet-53 base layers in
// reverse, each as a Conv2DTranspose that carries the layer's own kernel -- the layer's data-gradient launcher -- behind a
// LeakyReLU / l2_normalize / BatchNorm stage (recon.hip), every residual add turned into a subtract.  Inference only.
#include "fid.h"
#include "net_plan.h"
#include "recon.h"

namespace {

constexpr int NB = 52;   // base layers: conv_0 .. the add_23 block

long long feat_floats(int S) { return (long long)(S / 32) * (S / 32) * 1024; }
int64_t base_param_count() { const auto& d = net().L[NB - 1]; return d.beta_off + d.cout; }
int64_t bn_channels() { return net().nstate / 2; }   // the 52 BN layers' channels: layer l's begin at mean_off / 2

// offsets in the fv_recon_param_count layout
struct Layout { int64_t dense, bias, bn, count; };
Layout layout(int S) {
    Layout o{};
    o.dense = base_param_count();
    o.bias = o.dense + feat_floats(S) * FID_DIM;
    o.bn = o.bias + feat_floats(S);
    o.count = o.bn + 4 * bn_channels();
    return o;
}

// The stride-1 transposed convs are whole-lattice launches: the conv launcher may cut their tail tiles into K slices.
size_t recon_tail_floats(const Layers& L, int B, int S) {
    long long need = 0;
    for (int l = 1; l < NB; ++l) {
        const auto& d = L[l];
        if (d.stride != 1) continue;
        const int Hi = S / d.in_div;
        int tf, full; long long n;
        fv_conv_tail_plan(B * Hi * Hi, d.cin, d.ksize * d.ksize * d.cout / 32, &tf, &full, &n);
        need = std::max(need, n);
    }
    return (size_t)need;
}

struct ReconWs {
    float *scale, *shift, *u, *act[3], *tail;
    std::vector<float*> wt;   // wt[l]: [cin][taps][cout] of layer l
    size_t tail_floats, bytes;
};
ReconWs make_ws(void* base, int B, int S) {
    const Net& N = net();
    ReconWs w{};
    Carver c(base);
    w.scale = c.take((size_t)bn_channels());
    w.shift = c.take((size_t)bn_channels());
    w.u = c.take((size_t)B * FID_DIM);
    w.wt.resize(NB);
    for (int l = 0; l < NB; ++l) {
        const auto& d = N.L[l];
        w.wt[l] = c.take((size_t)d.cin * d.ksize * d.ksize * d.cout);
    }
    // the largest activation is the input of the last stage: batch * S * S * 32 floats (the head's batch * F is smaller)
    for (auto& a : w.act) a = c.take((size_t)B * S * S * 32);
    w.tail_floats = recon_tail_floats(N.L, B, S);
    w.tail = c.take_some(w.tail_floats);
    w.bytes = c.off;
    return w;
}

}  // namespace

extern "C" {

int64_t fv_recon_param_count(int image_size) {
    if (image_size < 32 || image_size % 32) return 0;
    return layout(image_size).count;
}

size_t fv_recon_workspace_bytes(int batch, int image_size) {
    if (batch < 1 || image_size < 32 || image_size % 32) return 0;
    return make_ws(nullptr, batch, image_size).bytes;
}

int fv_recon_dense_head(fv_ctx* ctx, const float* ids, int rows, int64_t F, const float* w, const float* bias, float* u, float* out) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_fid_recon_head(ctx, ids, rows, F, w, bias, u, out);
}

int fv_l2norm_affine(fv_ctx* ctx, const float* x, const float* skip, float* d_out, const float* scale, const float* shift, float* y,
                     int64_t rows, int C, float leaky) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_recon_l2norm_affine(ctx, x, skip, d_out, scale, shift, y, rows, C, leaky);
}

int fv_conv2d_transpose(fv_ctx* ctx, const float* x, const float* w_t, int B, int Hin, int Win, int cin, int cout, int ksize, int stride,
                        float* out) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, x && w_t && out, "conv2d_transpose: NULL buffer");
    FV_REQUIRE(ctx, B >= 1 && Hin >= 1 && Win >= 1 && cin >= 1 && cout >= 1, "conv2d_transpose: bad problem size");
    FV_REQUIRE(ctx, (long long)B * Hin * stride * Win * stride * std::max(cin, 4) < (1ll << 31), "conv2d_transpose: output reaches 2^31 elements");
    if (cin == 3) {
        FV_REQUIRE(ctx, cout == 32 && ksize == 3 && stride == 1, "conv2d_transpose: cin = 3 is served for the 32 -> 3 channel 3x3 stride-1 layer only");
        return fv_recon_convt_last(ctx, x, w_t, B, Hin, Win, out);
    }
    return fv_op_conv_dgrad(ctx, x, w_t, B, Hin * stride, Win * stride, cin, cout, ksize, stride, nullptr, out, nullptr, 0);
}

int fv_recon_forward(fv_ctx* ctx, const float* params, const float* ids, int batch, int image_size, void* workspace, size_t workspace_bytes,
                     float* out) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, params && ids && workspace && out, "recon_forward: NULL buffer");
    if (int rc = check_batch(ctx, "recon_forward", batch, image_size)) return rc;
    const int S = image_size;
    FV_REQUIRE(ctx, fv_recon_convt_last_ok(S, S), "recon_forward: image_size %d", S);
    const ReconWs w = make_ws(workspace, batch, S);
    if (w.bytes > workspace_bytes) return fv_fail(ctx, FV_ERR_WORKSPACE, "recon_forward: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    const Layout o = layout(S);
    FV_REQUIRE(ctx, o.count < (1ll << 31), "recon_forward: parameter vector reaches 2^31 floats");
    TailLend lend(ctx, w.tail, w.tail_floats);
    const Net& N = net();
    const Layers L(N.L.begin(), N.L.begin() + NB);

    // ---------------- this call's images of the parameters: BN folded into scale / shift, kernels transposed
    {
        int chb[64]; long long go[64], bo[64], mo[64], vo[64];
        for (int l = 0; l < NB; ++l) {
            const long long c0 = L[l].mean_off / 2, at = o.bn + 4 * c0;
            chb[l] = (int)c0; go[l] = at; bo[l] = at + L[l].cout; mo[l] = at + 2 * L[l].cout; vo[l] = at + 3 * L[l].cout;
        }
        if (int rc = fv_ew_bn_fold_all(ctx, params, params, NB, chb, go, bo, mo, vo, BN_EPS, (int)bn_channels(), w.scale, w.shift)) return rc;
    }
    if (int rc = fv_ew_transpose_ntc(ctx, params + L[0].w_off, w.wt[0], L[0].cout, 9, L[0].cin, L[0].cout)) return rc;
    if (int rc = transpose_weights(ctx, L, params, w.wt, 0)) return rc;

    // ---------------- head: x = relu(l2_normalize(ids)) . K^T + b, [batch][g][g][1024]
    // Three buffers: x (the running tensor), skip (kept while a residual block runs) and y (the normalised stage input).  A pending
    // subtract is folded into the next stage's normalise, which stores d = x - skip over x: that buffer becomes the skip, the old
    // skip buffer is free.
    int ix = 0, iskip = 0;
    bool pending = false;   // x - skip has not been formed yet
    if (int rc = fv_fid_recon_head(ctx, ids, batch, feat_floats(S), params + o.dense, params + o.bias, w.u, w.act[ix])) return rc;

    auto stage = [&](int l, bool keep_d, float* to) -> int {
        const auto& d = L[l];
        const int Ho = S / d.out_div, Hi = S / d.in_div;   // the transposed conv runs from the layer's output grid to its input grid
        const long long rows = (long long)batch * Ho * Ho;
        int iy = 0;
        while (iy == ix || iy == iskip) ++iy;
        const float* sk = pending ? w.act[iskip] : nullptr;
        if (int rc = fv_recon_l2norm_affine(ctx, w.act[ix], sk, pending && keep_d ? w.act[ix] : nullptr, w.scale + d.mean_off / 2,
                                            w.shift + d.mean_off / 2, w.act[iy], rows, d.cout, LEAKY)) return rc;
        int io;   // the conv's output: any buffer but y and the live skip
        if (pending) { io = iskip; if (keep_d) iskip = ix; pending = false; }   // the old skip has been consumed
        else if (ix != iskip) io = ix;                                           // x has been consumed
        else { io = 0; while (io == iy || io == iskip) ++io; }                   // x is the skip itself: leave it
        float* dst = to ? to : w.act[io];
        if (d.cin == 3) { if (int rc = fv_recon_convt_last(ctx, w.act[iy], w.wt[l], batch, Hi, Hi, dst)) return rc; }
        else if (int rc = fv_op_conv_dgrad(ctx, w.act[iy], w.wt[l], batch, Hi, Hi, d.cin, d.cout, d.ksize, d.stride, nullptr, dst, nullptr, 0)) return rc;
        ix = io;
        return FV_OK;
    };

    for (int l = NB - 1; l >= 2; --l) {
        if (L[l].stride == 2) {
            if (int rc = stage(l, false, nullptr)) return rc;
            iskip = ix;                                  // skip = x
        } else {
            // a residual block's 3x3 (role 2) and then its 1x1 (role 1); the subtract waits for the next normalise
            if (int rc = stage(l, true, nullptr)) return rc;
            if (int rc = stage(--l, true, nullptr)) return rc;
            pending = true;
        }
    }
    if (int rc = stage(1, false, nullptr)) return rc;
    return stage(0, false, out);
}

}  // extern "C"
