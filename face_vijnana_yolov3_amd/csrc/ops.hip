// Operator-level entry points of the C ABI: translate Keras-style conv descriptions into the
// gather-convolution tap lists of conv.h.
#include "conv.h"
#include "elementwise.h"
#include "fid.h"
#include "ops.h"

#include <cmath>

static void fwd_taps(int ksize, FvTaps& t) {
    if (ksize == 1) { t.n = 1; t.dh[0] = t.dw[0] = 0; t.wslot[0] = 0; return; }
    t.n = 9;
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) { int i = r * 3 + q; t.dh[i] = r - 1; t.dw[i] = q - 1; t.wslot[i] = i; }
}

static bool fwd_shape_ok(int H, int W, int ksize, int stride) {
    return ((ksize == 1 && stride == 1) || (ksize == 3 && (stride == 1 || stride == 2))) && H % stride == 0 && W % stride == 0;
}

// the launch description of a forward conv; the tensors and the inference-tiling choices are the caller's
static void fwd_args(FvConvArgs& a, int B, int H, int W, int cin, int cout, int ksize, int stride, int epi, int ksplit,
                     double* stat_slots, int stat_nslot) {
    a.B = B; a.Hin = H; a.Win = W; a.Cin = cin;
    a.Hl = H / stride; a.Wl = W / stride; a.Hout = a.Hl; a.Wout = a.Wl; a.Nout = cout;
    a.is = stride; a.os = 1; a.Tw = ksize * ksize; a.M = B * a.Hl * a.Wl;
    a.epi = epi; a.nclass = 1;
    fwd_taps(ksize, a.taps[0]);
    if (cin % 32 != 0) a.Tw = 1;  // packed [cout][32] first-layer weights
    a.alg_flops = 2.0 * a.M * cout * (double)(ksize * ksize * cin);
    a.ksplit = ksplit; a.split_stride = (long long)a.M * cout;
    a.stat_slots = stat_slots; a.stat_nslot = stat_nslot;
}

bool fv_op_conv_forward_takes_bn_in(fv_ctx* ctx, int B, int H, int W, int cin, int cout, int ksize, int stride) {
    if (!fwd_shape_ok(H, W, ksize, stride)) return false;
    static double any_slot;   // the predicate asks only whether slots are given
    FvConvArgs a{};
    fwd_args(a, B, H, W, cin, cout, ksize, stride, FV_EPI_STATS, 1, &any_slot, 1);
    // fv_conv_launch's own bound on the input tensor (one 2 GiB buffer descriptor), then its first dispatch
    return (long long)B * H * W * cin < (1ll << 29) && ctx->conv_halo && fv_conv9_fwd_ok(a);
}

bool fv_op_conv_forward_takes_bn_stats_in(int option, bool persist_on, int B, int H, int W, int cin, int cout, int ksize, int stride,
                                          bool with_skip) {
    if (option <= 0 || !persist_on || ksize != 1 || stride != 1 || B < 1 || H < 1 || W < 1 || cin < 1 || cout < 1) return false;
    if ((long long)B * H * W * cin >= (1ll << 29)) return false;
    static double any_slot;
    FvConvArgs a{};
    fwd_args(a, B, H, W, cin, cout, ksize, stride, FV_EPI_STATS, 1, &any_slot, 1);
    if (!fv_conv1x1_bn_in_ok(a)) return false;
    if (option >= 2) return true;
    return fv_conv1x1_bn_in_wins(a, with_skip);
}

int fv_op_conv_forward(fv_ctx* ctx, const float* x, const float* w, int B, int H, int W, int cin, int cout, int ksize,
                       int stride, int epi, const float* scale, const float* shift, float leaky, const float* addend,
                       float* out, float* psum, float* psq, int ksplit, double* stat_slots, int stat_nslot, const FvBnIn* bn_in,
                       const FvBnStatsIn* bn_stats_in) {
    FV_REQUIRE(ctx, (ksize == 1 && stride == 1) || (ksize == 3 && (stride == 1 || stride == 2)), "conv: unsupported k=%d s=%d", ksize, stride);
    FV_REQUIRE(ctx, H % stride == 0 && W % stride == 0, "conv: H,W must be divisible by the stride");
    FvConvArgs a{};
    a.x = x; a.w = w; a.out = out; a.addend = addend; a.scale = scale; a.shift = shift; a.psum = psum; a.psq = psq;
    a.leaky = leaky;
    if (bn_in) {
        FV_REQUIRE(ctx, bn_in->scale && bn_in->shift, "conv: BN-on-load needs scale and shift");
        a.in_scale = bn_in->scale; a.in_shift = bn_in->shift; a.in_leaky = bn_in->leaky;
    }
    if (const FvBnStatsIn* bi = bn_stats_in) {
        FV_REQUIRE(ctx, !bn_in, "conv: one BN-on-load form per launch");
        a.bi_slots = bi->slots; a.bi_nslot = bi->nslot; a.bi_count = bi->count; a.bi_gamma = bi->gamma; a.bi_beta = bi->beta;
        a.bi_eps = bi->eps; a.bi_leaky = bi->leaky;
        fv_ew_bn_ema_coeff(ctx, bi->momentum, &a.bi_ema_old, &a.bi_ema_new);
        a.bi_mean = bi->mean; a.bi_invstd = bi->invstd; a.bi_scale = bi->scale; a.bi_shift = bi->shift;
        a.bi_mmean = bi->moving_mean; a.bi_mvar = bi->moving_var; a.bi_skip = bi->skip; a.bi_a = bi->a_out;
        FV_REQUIRE(ctx, a.bi_slots, "conv: the BN-input mode needs the producing layer's statistics slots");
    }
    fwd_args(a, B, H, W, cin, cout, ksize, stride, epi, ksplit, stat_slots, stat_nslot);
    // inference epilogues only: the training forward keeps one tiling whatever the batch (its statistics are per-tile sums)
    a.small = (ctx->conv_small && ksplit <= 1 && !(epi & FV_EPI_STATS) && cin % 32 == 0) ? fv_conv_small_plan(a.M, cout, cin, ksize * ksize) : 0;
    a.narrow = (!a.small && ksize == 1 && ksplit <= 1 && !(epi & FV_EPI_STATS) && cin % 32 == 0 && fv_conv_narrow(a.M, cout, cin / 32)) ? 1 : 0;
    a.bm64 = (ctx->conv_bm64 && !a.small && !a.narrow && !(epi & FV_EPI_STATS) && cin % 32 == 0 && fv_conv_bm64(a.M, cout, ksize * ksize * cin / 32)) ? 1 : 0;
    return fv_conv_launch(ctx, a);
}

int fv_op_conv_dgrad(fv_ctx* ctx, const float* dy, const float* w_t, int B, int H, int W, int cin, int cout_pad, int ksize,
                     int stride, const float* addend, float* dx, const FvBnRed* bn, int s2_pad_lo) {
    FV_REQUIRE(ctx, (ksize == 1 && stride == 1) || (ksize == 3 && (stride == 1 || stride == 2)), "dgrad: unsupported k=%d s=%d", ksize, stride);
    FV_REQUIRE(ctx, s2_pad_lo == 0 || s2_pad_lo == 1, "dgrad: s2_pad_lo must be 0 or 1");
    FV_REQUIRE(ctx, cout_pad % 32 == 0, "dgrad: cout_pad must be a multiple of 32");
    FV_REQUIRE(ctx, H % stride == 0 && W % stride == 0, "dgrad: H,W must be divisible by the stride");
    FvConvArgs a{};
    a.x = dy; a.w = w_t; a.out = dx; a.addend = addend;
    a.B = B; a.Hin = H / stride; a.Win = W / stride; a.Cin = cout_pad;
    a.Hout = H; a.Wout = W; a.Nout = cin;
    a.is = 1; a.Tw = ksize * ksize;
    a.epi = addend ? FV_EPI_ADD : 0; a.leaky = 0.f;
    if (bn) {
        a.epi |= FV_EPI_BNRED;
        a.bn_z = bn->z; a.bn_scale = bn->scale; a.bn_shift = bn->shift; a.bn_mean = bn->mean; a.bn_invstd = bn->invstd;
        a.bn_slots = bn->slots; a.bn_nslot = bn->nslot; a.bn_leaky = bn->leaky;
    }
    if (stride == 1) {
        a.Hl = H; a.Wl = W; a.os = 1; a.nclass = 1;
        FvTaps& t = a.taps[0];
        if (ksize == 1) { t.n = 1; t.dh[0] = t.dw[0] = 0; t.wslot[0] = 0; }
        else {
            t.n = 9;   // dx[h] = sum_r dz[h + 1 - r] w[r]
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) { int i = r * 3 + q; t.dh[i] = 1 - r; t.dw[i] = 1 - q; t.wslot[i] = i; }
        }
    } else {
        // forward: z[oh] reads x[2 oh - 1 + r].  Output pixel h = 2a+ph receives from r with
        // (h+1-r) even: ph=0 -> r=1 (oh=a); ph=1 -> r=0 (oh=a+1), r=2 (oh=a).  One class per (ph,pw).
        // s2_pad_lo = 0: z[oh] reads x[2 oh + r]: ph=0 -> r=0 (oh=a), r=2 (oh=a-1); ph=1 -> r=1 (oh=a).
        const int p = s2_pad_lo;
        FV_REQUIRE(ctx, H % 2 == 0 && W % 2 == 0, "dgrad: stride 2 needs even H, W");
        a.Hl = H / 2; a.Wl = W / 2; a.os = 2; a.nclass = 4;
        for (int ph = 0; ph < 2; ++ph)
            for (int pw = 0; pw < 2; ++pw) {
                // class = blockIdx.z, dispatched in ascending order: the 4-tap class (ph = pw = 1) goes
                // first and the 1-tap class last, so the longest tiles are not left for the tail (p = 0: that class is ph = pw = 0)
                int c = p ? 3 - (ph * 2 + pw) : ph * 2 + pw;
                a.oph[c] = ph; a.opw[c] = pw;
                FvTaps& t = a.taps[c];
                t.n = 0;
                for (int r = 0; r < 3; ++r) {
                    if ((ph + p - r) % 2 != 0) continue;
                    for (int q = 0; q < 3; ++q) {
                        if ((pw + p - q) % 2 != 0) continue;
                        t.dh[t.n] = (ph + p - r) / 2; t.dw[t.n] = (pw + p - q) / 2; t.wslot[t.n] = r * 3 + q;
                        ++t.n;
                    }
                }
            }
    }
    a.M = B * a.Hl * a.Wl;
    // same MACs as the forward conv it differentiates (cout_real unknown here: padded channels are zeros)
    a.alg_flops = 2.0 * (double)B * (H / stride) * (W / stride) * cin * (double)(ksize * ksize * cout_pad);
    return fv_conv_launch(ctx, a);
}

static void wgrad_args(FvWgradArgs& a, int B, int H, int W, int cin, int cout, int dy_stride, int ksize, int stride) {
    a.B = B; a.Hin = H; a.Win = W; a.Cin = cin;
    a.Hl = H / stride; a.Wl = W / stride; a.N = cout; a.Ndy = dy_stride;
    a.is = stride; a.Tw = ksize * ksize; a.M = B * a.Hl * a.Wl;
    fwd_taps(ksize, a.taps);
    a.alg_flops = 2.0 * a.M * cout * (double)(ksize * ksize * cin);
}

// fv_wgrad_launch's own checks on the sizes (2 GiB buffer descriptors), which come before its dispatch
static bool wgrad_sizes_ok(const FvWgradArgs& a, int H, int W, int ksize, int stride) {
    return fwd_shape_ok(H, W, ksize, stride) && a.M > 0 && a.N > 0 && a.Ndy >= a.N && a.Ndy % 4 == 0 &&
           (long long)a.B * a.Hin * a.Win * a.Cin < (1ll << 29) && (long long)a.M * a.Ndy < (1ll << 29);
}

bool fv_op_conv_wgrad_takes_bn_in(fv_ctx* ctx, int B, int H, int W, int cin, int cout, int dy_stride, int ksize, int stride) {
    FvWgradArgs a{};
    wgrad_args(a, B, H, W, cin, cout, dy_stride, ksize, stride);
    return wgrad_sizes_ok(a, H, W, ksize, stride) && cin % 32 == 0 && ctx->wgrad_fused_taps && fv_wgrad9_ok(a);
}

bool fv_op_conv_wgrad_takes_bn_dy(fv_ctx* ctx, int B, int H, int W, int cin, int cout, int dy_stride, int ksize, int stride) {
    FvWgradArgs a{};
    wgrad_args(a, B, H, W, cin, cout, dy_stride, ksize, stride);
    // (the pointers of the mode are the caller's: what is asked here is the shape; 32 channels per pixel of g and z alike)
    return wgrad_sizes_ok(a, H, W, ksize, stride) && cin % 32 != 0 && 9 * cin <= 32 && dy_stride == cout && ctx->wgrad_fused_taps &&
           fv_wgrad0_ok(a);
}

int fv_op_conv_wgrad(fv_ctx* ctx, const float* x, const float* dy, int B, int H, int W, int cin, int cout, int dy_stride,
                     int ksize, int stride, float* dw, const FvBnIn* bn_in, const FvBnDy* bn_dy) {
    FV_REQUIRE(ctx, (ksize == 1 && stride == 1) || (ksize == 3 && (stride == 1 || stride == 2)), "wgrad: unsupported k=%d s=%d", ksize, stride);
    FvWgradArgs a{};
    a.x = x; a.dy = dy; a.dw = dw;
    wgrad_args(a, B, H, W, cin, cout, dy_stride, ksize, stride);
    if (bn_in) {
        FV_REQUIRE(ctx, bn_in->scale && bn_in->shift, "wgrad: BN-on-load needs scale and shift");
        a.x_scale = bn_in->scale; a.x_shift = bn_in->shift; a.x_leaky = bn_in->leaky;
    }
    if (bn_dy) {
        FV_REQUIRE(ctx, bn_dy->z && bn_dy->scale && bn_dy->shift && bn_dy->mean && bn_dy->invstd && bn_dy->slots && bn_dy->nslot >= 1 &&
                            bn_dy->dbeta && bn_dy->dgamma, "wgrad: the fused BN-backward apply needs its layer's tensors");
        a.bn_z = bn_dy->z; a.bn_scale = bn_dy->scale; a.bn_shift = bn_dy->shift; a.bn_mean = bn_dy->mean; a.bn_invstd = bn_dy->invstd;
        a.bn_slots = bn_dy->slots; a.bn_nslot = bn_dy->nslot; a.bn_leaky = bn_dy->leaky;
        a.bn_count = (double)a.M;                         // as fv_ew_bn_bwd passes it: rows = B * H * W
        a.bn_dbeta = bn_dy->dbeta; a.bn_dgamma = bn_dy->dgamma; a.bn_accumulate = bn_dy->accumulate ? 1 : 0;
    }
    return fv_wgrad_launch(ctx, a);
}

extern "C" {

int fv_conv2d_stat_rows(int64_t out_pixels) { return fv_conv_mtiles((int)out_pixels, 0); }

int fv_conv2d_forward(fv_ctx* ctx, const float* x, const float* w, int B, int H, int W, int cin, int cout, int ksize,
                      int stride, const float* scale, const float* shift, float leaky, const float* addend, float* out,
                      float* psum, float* psq) {
    if (!ctx) return FV_ERR_INVALID;
    int epi = 0;
    if (psum) {
        FV_REQUIRE(ctx, !scale && !shift && !addend && leaky < 0.f, "conv2d_forward: statistics mode stores the raw result");
        epi = FV_EPI_STATS;
    } else {
        if (scale || shift) epi |= FV_EPI_AFFINE;
        if (leaky >= 0.f) epi |= FV_EPI_LEAKY;
        if (addend) epi |= FV_EPI_ADD;
    }
    return fv_op_conv_forward(ctx, x, w, B, H, W, cin, cout, ksize, stride, epi, scale, shift, leaky, addend, out, psum, psq, 1);
}

int fv_conv2d_dgrad(fv_ctx* ctx, const float* dy, const float* w_t, int B, int H, int W, int cin, int cout_pad, int ksize,
                    int stride, const float* addend, float* dx) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_op_conv_dgrad(ctx, dy, w_t, B, H, W, cin, cout_pad, ksize, stride, addend, dx, nullptr);
}

int fv_conv2d_wgrad(fv_ctx* ctx, const float* x, const float* dy, int B, int H, int W, int cin, int cout, int dy_stride,
                    int ksize, int stride, float* dw) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_op_conv_wgrad(ctx, x, dy, B, H, W, cin, cout, dy_stride, ksize, stride, dw);
}

int fv_transpose_weights(fv_ctx* ctx, const float* w, int cout, int taps, int cin, int cout_pad, float* w_t) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, cout_pad >= cout, "transpose_weights: cout_pad < cout");
    return fv_ew_transpose_ntc(ctx, w, w_t, cout, taps, cin, cout_pad);
}

int fv_pack_first_layer(fv_ctx* ctx, const float* w, int cout, int k_elems, float* w_packed) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, k_elems <= 32, "pack_first_layer: k_elems > 32");
    return fv_ew_pad_rows(ctx, w, w_packed, cout, k_elems, 32);
}

int fv_bn_finalize(fv_ctx* ctx, const float* psum, const float* psq, int stat_rows, int C, int64_t count, const float* gamma,
                   const float* beta, float eps, float momentum, float* mean, float* invstd, float* scale, float* shift,
                   float* moving_mean, float* moving_var) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_ew_bn_finalize(ctx, psum, psq, stat_rows, C, (double)count, gamma, beta, eps, momentum, mean, invstd, scale, shift,
                             moving_mean, moving_var);
}

int fv_bn_act(fv_ctx* ctx, const float* z, const float* scale, const float* shift, const float* skip, float* out, int64_t rows,
              int C, float leaky) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_ew_bn_act(ctx, z, scale, shift, skip, out, rows, C, leaky);
}

int64_t fv_bn_bwd_scratch_floats(int64_t rows, int C) { return (int64_t)fv_ew_bn_bwd_chunks(rows, C) * C; }

int fv_bn_bwd(fv_ctx* ctx, const float* g, const float* z, const float* scale, const float* shift, const float* mean,
              const float* invstd, int64_t rows, int C, float leaky, float* scratch, float* dbeta, float* dgamma, float* dz) {
    if (!ctx) return FV_ERR_INVALID;
    int64_t half = fv_bn_bwd_scratch_floats(rows, C);
    return fv_ew_bn_bwd(ctx, g, z, scale, shift, mean, invstd, rows, C, leaky, scratch, scratch + half, dbeta, dgamma, dz);
}

int fv_bn_stat_slots(int C) { return fv_ew_bn_stat_slots(C); }

static int slots_ok(fv_ctx* ctx, const double* slots, int nslot, int C, const char* who) {
    FV_REQUIRE(ctx, slots && nslot >= 1 && C % 4 == 0 && C <= 1024 && (C >= 256 ? true : 256 % C == 0),
               "%s: needs accumulator slots, C %% 4 == 0, C <= 1024 and C dividing or divided by 256 (C=%d)", who, C);
    return FV_OK;
}

int fv_conv2d_forward_slots(fv_ctx* ctx, const float* x, const float* w, int B, int H, int W, int cin, int cout, int ksize,
                            int stride, float* z, double* slots, int nslot) {
    if (!ctx) return FV_ERR_INVALID;
    if (int rc = slots_ok(ctx, slots, nslot, cout, "conv2d_forward_slots")) return rc;
    return fv_op_conv_forward(ctx, x, w, B, H, W, cin, cout, ksize, stride, FV_EPI_STATS, nullptr, nullptr, 0.f, nullptr, z,
                              nullptr, nullptr, 1, slots, nslot);
}

int fv_bn_act_slots(fv_ctx* ctx, const float* z, const double* slots, int nslot, int64_t rows, int C, const float* gamma,
                    const float* beta, float eps, float momentum, float* mean, float* invstd, float* scale, float* shift,
                    float* moving_mean, float* moving_var, const float* skip, float* out, float leaky) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, slots && nslot >= 1 && C % 4 == 0 && C >= 4 && C <= 1024, "bn_act_slots: needs accumulator slots, C %% 4 == 0 and C <= 1024 (C=%d)", C);
    FV_REQUIRE(ctx, z && gamma && beta && mean && invstd && scale && shift && out && rows > 0, "bn_act_slots: NULL buffer");
    return fv_ew_bn_act_stats(ctx, z, slots, nslot, (double)rows, gamma, beta, eps, momentum, mean, invstd, scale, shift,
                              moving_mean, moving_var, skip, out, rows, C, leaky);
}

int fv_conv2d_dgrad_bnred(fv_ctx* ctx, const float* dy, const float* w_t, int B, int H, int W, int cin, int cout_pad, int ksize,
                          int stride, const float* addend, float* dx, const float* bn_z, const float* scale, const float* shift,
                          const float* mean, const float* invstd, float leaky, double* slots, int nslot) {
    if (!ctx) return FV_ERR_INVALID;
    if (int rc = slots_ok(ctx, slots, nslot, cin, "conv2d_dgrad_bnred")) return rc;
    FvBnRed b{bn_z, scale, shift, mean, invstd, slots, nslot, leaky};
    return fv_op_conv_dgrad(ctx, dy, w_t, B, H, W, cin, cout_pad, ksize, stride, addend, dx, &b);
}

int fv_bn_bwd_slots(fv_ctx* ctx, const float* g, const float* z, const float* scale, const float* shift, const float* mean,
                    const float* invstd, int64_t rows, int C, float leaky, double* slots, int nslot, int reduced, float* dbeta,
                    float* dgamma, float* dz) {
    if (!ctx) return FV_ERR_INVALID;
    if (int rc = slots_ok(ctx, slots, nslot, C, "bn_bwd_slots")) return rc;
    FV_REQUIRE(ctx, g && z && scale && shift && mean && invstd && dbeta && dgamma && dz && rows > 0, "bn_bwd_slots: NULL buffer");
    return fv_ew_bn_bwd(ctx, g, z, scale, shift, mean, invstd, rows, C, leaky, nullptr, nullptr, dbeta, dgamma, dz, slots, nslot,
                        reduced != 0);
}

int fv_conv2d_forward_slots_bn_in(fv_ctx* ctx, const float* z_in, const float* in_scale, const float* in_shift, float leaky,
                                  const float* w, int B, int H, int W, int cin, int cout, int ksize, int stride, float* z, double* slots,
                                  int nslot) {
    if (!ctx) return FV_ERR_INVALID;
    if (int rc = slots_ok(ctx, slots, nslot, cout, "conv2d_forward_slots_bn_in")) return rc;
    FV_REQUIRE(ctx, z_in && in_scale && in_shift && w && z, "conv2d_forward_slots_bn_in: NULL buffer");
    FV_REQUIRE(ctx, fv_op_conv_forward_takes_bn_in(ctx, B, H, W, cin, cout, ksize, stride),
               "conv2d_forward_slots_bn_in: only the halo kernel applies BN on load (3x3, 32 -> 64 channels, stride 1 or 2, option "
               "conv_halo); it does not take B=%d H=%d W=%d cin=%d cout=%d k=%d s=%d", B, H, W, cin, cout, ksize, stride);
    const FvBnIn bi{in_scale, in_shift, leaky};
    return fv_op_conv_forward(ctx, z_in, w, B, H, W, cin, cout, ksize, stride, FV_EPI_STATS, nullptr, nullptr, 0.f, nullptr, z, nullptr,
                              nullptr, 1, slots, nslot, &bi);
}

int fv_conv2d_forward_slots_bn_stats_in(fv_ctx* ctx, const float* z_in, const double* in_slots, int in_nslot, const float* gamma,
                                        const float* beta, float eps, float momentum, float* mean, float* invstd, float* scale,
                                        float* shift, float* moving_mean, float* moving_var, const float* skip, float* a_out,
                                        float leaky, const float* w, int B, int H, int W, int cin, int cout, float* z,
                                        double* slots, int nslot) {
    if (!ctx) return FV_ERR_INVALID;
    if (int rc = slots_ok(ctx, slots, nslot, cout, "conv2d_forward_slots_bn_stats_in")) return rc;
    FV_REQUIRE(ctx, z_in && in_slots && in_nslot >= 1 && gamma && beta && mean && invstd && scale && shift && a_out && w && z,
               "conv2d_forward_slots_bn_stats_in: NULL buffer");
    FV_REQUIRE(ctx, fv_op_conv_forward_takes_bn_stats_in(2, ctx->conv1x1_persist, B, H, W, cin, cout, 1, 1, skip != nullptr),
               "conv2d_forward_slots_bn_stats_in: only the persistent 1x1 kernel has the BN-input mode (cin %% 32 == 0, cin <= 512, "
               "cout %% 4 == 0, cout > 32, option conv1x1_persist); it does not take B=%d H=%d W=%d cin=%d cout=%d", B, H, W, cin, cout);
    const FvBnStatsIn bi{in_slots, in_nslot, (double)B * H * W, gamma, beta, eps, momentum, mean, invstd, scale, shift, moving_mean,
                         moving_var, skip, a_out, leaky};
    return fv_op_conv_forward(ctx, z_in, w, B, H, W, cin, cout, 1, 1, FV_EPI_STATS, nullptr, nullptr, 0.f, nullptr, z, nullptr,
                              nullptr, 1, slots, nslot, nullptr, &bi);
}

int fv_conv2d_wgrad_bn_in(fv_ctx* ctx, const float* z_in, const float* in_scale, const float* in_shift, float leaky, const float* dy,
                          int B, int H, int W, int cin, int cout, int dy_stride, int ksize, int stride, float* dw) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, z_in && in_scale && in_shift && dy && dw, "conv2d_wgrad_bn_in: NULL buffer");
    FV_REQUIRE(ctx, fv_op_conv_wgrad_takes_bn_in(ctx, B, H, W, cin, cout, dy_stride, ksize, stride),
               "conv2d_wgrad_bn_in: only the halo kernel applies BN on load (3x3, 32 -> 64 channels, stride 1 or 2, option "
               "wgrad_fused_taps); it does not take B=%d H=%d W=%d cin=%d cout=%d k=%d s=%d", B, H, W, cin, cout, ksize, stride);
    const FvBnIn bi{in_scale, in_shift, leaky};
    return fv_op_conv_wgrad(ctx, z_in, dy, B, H, W, cin, cout, dy_stride, ksize, stride, dw, &bi);
}

int fv_conv2d_wgrad_bn_bwd(fv_ctx* ctx, const float* x, const float* g, const float* z, const float* scale, const float* shift,
                           const float* mean, const float* invstd, float leaky, const double* slots, int nslot, int B, int H, int W,
                           int cin, int cout, int ksize, int stride, int accumulate, float* dbeta, float* dgamma, float* dw) {
    if (!ctx) return FV_ERR_INVALID;
    if (int rc = slots_ok(ctx, slots, nslot, cout, "conv2d_wgrad_bn_bwd")) return rc;
    FV_REQUIRE(ctx, x && g && z && scale && shift && mean && invstd && dbeta && dgamma && dw, "conv2d_wgrad_bn_bwd: NULL buffer");
    FV_REQUIRE(ctx, fv_op_conv_wgrad_takes_bn_dy(ctx, B, H, W, cin, cout, cout, ksize, stride),
               "conv2d_wgrad_bn_bwd: only the first layer's halo kernel applies the BN-backward on load (3x3 stride 1, 3 -> 32 channels, "
               "option wgrad_fused_taps); it does not take B=%d H=%d W=%d cin=%d cout=%d k=%d s=%d", B, H, W, cin, cout, ksize, stride);
    const FvBnDy bd{z, scale, shift, mean, invstd, slots, nslot, leaky, dbeta, dgamma, accumulate != 0};
    return fv_op_conv_wgrad(ctx, x, g, B, H, W, cin, cout, cout, ksize, stride, dw, nullptr, &bd);
}

int fv_mse_loss_grad(fv_ctx* ctx, const float* yp, const float* yt, int rows, int C, int c_pad, float* loss, float* dy,
                     float* dbias) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_ew_mse(ctx, yp, yt, rows, C, c_pad, loss, dy, dbias);
}

int fv_fd_loss_grad(fv_ctx* ctx, const float* yp, const float* yt, int cells, int c_pad, float* loss, float* dy) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_ew_fd_loss(ctx, yp, yt, cells, c_pad, loss, dy);
}

int fv_adam_step(fv_ctx* ctx, float* params, const float* grads, float* m, float* v, int64_t n, int64_t iteration, double lr,
                 double beta_1, double beta_2, double eps, double decay) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, params && grads && m && v && n > 0, "adam: NULL buffer");
    if (decay > 0.0) lr = lr * (1.0 / (1.0 + decay * (double)iteration));
    double t = (double)iteration + 1.0;
    double lr_t = lr * (sqrt(1.0 - pow(beta_2, t)) / (1.0 - pow(beta_1, t)));
    return fv_ew_adam(ctx, params, grads, m, v, n, (float)lr_t, (float)beta_1, (float)beta_2, (float)eps);
}

int fv_scale(fv_ctx* ctx, float* v, int64_t n, double alpha) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, v && n >= 0, "scale: NULL buffer");
    return fv_ew_scale(ctx, v, n, (float)alpha);
}

// ---- the three-scale helpers and the FaceIdentifier head, one call per operator: each forwards to the launcher the training
// steps call (elementwise.hip, fid.hip) and sizes its partial buffer with the same helper
int fv_upsample_concat(fv_ctx* ctx, const float* src, const float* skip, float* out, int B, int Hs, int Ws, int C1, int C2) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, src && skip && out && B >= 1 && Hs >= 1 && Ws >= 1 && C1 >= 4 && C2 >= 4, "upsample_concat: NULL buffer or empty shape");
    return fv_ew_upsample_concat(ctx, src, skip, out, B, Hs, Ws, C1, C2);
}

int fv_upsample_concat_bwd(fv_ctx* ctx, const float* g, float* g_up, float* g_skip, int B, int Hs, int Ws, int C1, int C2) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, g && g_up && g_skip && B >= 1 && Hs >= 1 && Ws >= 1 && C1 >= 4 && C2 >= 4, "upsample_concat_bwd: NULL buffer or empty shape");
    return fv_ew_upsample_concat_bwd(ctx, g, g_up, g_skip, B, Hs, Ws, C1, C2);
}

int64_t fv_colsum_partial_doubles(int64_t rows, int C) {
    if (rows < 1 || C < 1) return 0;
    return (int64_t)fv_ew_colsum_chunks(rows) * C;
}

int fv_colsum(fv_ctx* ctx, const float* dy, int64_t rows, int C, int c_pad, double* partial, float* out) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, dy && partial && out && rows >= 1 && C >= 1 && c_pad >= C, "colsum: NULL buffer, rows < 1 or c_pad < C");
    return fv_ew_colsum(ctx, dy, rows, C, c_pad, partial, out);
}

int64_t fv_yolo_loss_partial_doubles(const int64_t* cells3, int A) {
    if (!cells3 || A < 1) return 0;
    int64_t n = 0;
    for (int s = 0; s < 3; ++s) {
        if (cells3[s] < 1) return 0;
        n += fv_ew_yolo_loss_blocks(cells3[s] * A);
    }
    return n;
}

int fv_yolo_loss_grad(fv_ctx* ctx, const float* const* yp3, const float* const* yt3, const int64_t* cells3, int ncls, int A, int c_pad,
                      double grad_weight, double* partial, float* loss, float* const* dy3) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, yp3 && yt3 && cells3 && dy3 && partial && loss && ncls >= 1 && A >= 1, "yolo_loss_grad: NULL buffer or bad ncls / A");
    FV_REQUIRE(ctx, std::isfinite(grad_weight) && grad_weight > 0.0, "yolo_loss_grad: grad_weight must be finite and > 0");
    long long cells[3];
    for (int s = 0; s < 3; ++s) {
        FV_REQUIRE(ctx, yp3[s] && yt3[s] && dy3[s] && cells3[s] >= 1, "yolo_loss_grad: scale %d: NULL buffer or no cells", s);
        cells[s] = cells3[s];
    }
    int off = 0;   // the partial layout of fv_yolov3_train_step: the scales' block sums back to back
    for (int s = 0; s < 3; ++s) {
        if (int rc = fv_ew_yolo_loss_part(ctx, yp3[s], yt3[s], cells[s], ncls, A, c_pad, dy3[s], partial + off, grad_weight)) return rc;
        off += fv_ew_yolo_loss_blocks(cells[s] * A);
    }
    return fv_ew_yolo_loss_finish(ctx, partial, cells, A, loss);
}

static int fid_rows(fv_ctx* ctx, const float* r0, const float* r1, const float* r2, int per, int M, const char* who, FidRows& out) {
    FV_REQUIRE(ctx, per >= 1 && M >= 1 && M <= 3 * per, "%s: needs per >= 1 and 1 <= M <= 3 * per (M=%d, per=%d)", who, M, per);
    out = FidRows{{(float*)r0, (float*)r1, (float*)r2}, per};
    for (int t = 0; t * per < M; ++t) FV_REQUIRE(ctx, out.p[t], "%s: tower %d is NULL but M = %d reaches it", who, t, M);
    return FV_OK;
}

int fv_fid_towers_dense_l2(fv_ctx* ctx, const float* x0, const float* x1, const float* x2, int per, int M, int64_t F, const float* w,
                           const float* bias, float* partial, float* pre, float* out) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, w && bias && partial && out, "fid_towers_dense_l2: NULL buffer");
    FidRows X;
    if (int rc = fid_rows(ctx, x0, x1, x2, per, M, "fid_towers_dense_l2", X)) return rc;
    if (int rc = fv_fid_dense_fwd(ctx, X, M, F, w, partial)) return rc;
    return fv_fid_dense_finish(ctx, partial, fv_fid_chunks(F), M, bias, pre, out);
}

int fv_fid_triplet_loss_grad(fv_ctx* ctx, const float* pre, const float* u, int B, double grad_weight, float* loss, float* dE,
                             float* dbias) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_fid_triplet(ctx, pre, u, B, loss, dE, dbias, grad_weight);
}

int fv_fid_batch_triplet_loss_grad(fv_ctx* ctx, const float* pre, const float* u, const int32_t* subjects, int M, double margin,
                                   int mode, double loss_weight, float* loss, float* dE, float* dbias, int32_t* pos_index,
                                   int32_t* neg_index, int32_t* kind, double* d_ap, double* d_an) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_fid_batch_triplet(ctx, pre, u, subjects, M, margin, mode, loss_weight, loss, dE, dbias, pos_index, neg_index, kind, d_ap,
                                d_an);
}

size_t fv_fid_margin_workspace_bytes(int M, int C) { return fv_fid_margin_ws_bytes(M, C); }

int fv_fid_margin_softmax_loss_grad(fv_ctx* ctx, const float* pre, const float* u, const int32_t* labels, int M, const float* W, int C,
                                    int kind, double scale, double margin, double loss_weight, void* workspace, size_t workspace_bytes,
                                    float* loss, float* dE, float* dbias, float* dW, int32_t* pred, double* cos_t) {
    if (!ctx) return FV_ERR_INVALID;
    return fv_fid_margin_softmax(ctx, pre, u, labels, M, W, C, kind, scale, margin, loss_weight, workspace, workspace_bytes, loss, dE,
                                 dbias, dW, pred, cos_t);
}

int fv_fid_towers_dense_dgrad(fv_ctx* ctx, const float* dE, int M, int64_t F, const float* w, float* dx0, float* dx1, float* dx2,
                              int per) {
    if (!ctx) return FV_ERR_INVALID;
    FidRows dX;
    if (int rc = fid_rows(ctx, dx0, dx1, dx2, per, M, "fid_towers_dense_dgrad", dX)) return rc;
    return fv_fid_dense_dgrad(ctx, dE, M, F, w, dX);
}

int fv_fid_towers_dense_wgrad(fv_ctx* ctx, const float* x0, const float* x1, const float* x2, int per, const float* dE, int M,
                              int64_t F, float* dw) {
    if (!ctx) return FV_ERR_INVALID;
    FidRows X;
    if (int rc = fid_rows(ctx, x0, x1, x2, per, M, "fid_towers_dense_wgrad", X)) return rc;
    return fv_fid_dense_wgrad(ctx, X, dE, M, F, dw);
}

}  // extern "C"
