// Internal operator-level launchers (ops.hip), used by net.hip.
#pragma once
#include "common.h"

// BN-on-load: the input of a conv / weight-gradient is the raw conv output z of the producing BN layer, and the halo kernel forms
// LeakyReLU(z * scale + shift) while staging it (conv9_mfma.hip, wgrad9_mfma.hip); a launch those kernels do not take fails
struct FvBnIn { const float *scale, *shift; float leaky; };
// BN-backward apply on load of a weight-gradient's dy (wgrad0_mfma.hip): dy is g, and dz is formed while staging it; the kernel
// also writes (accumulate: adds) d-beta / d-gamma from the slots, as the apply pass (fv_ew_bn_bwd with reduced = true) would
struct FvBnDy { const float *z, *scale, *shift, *mean, *invstd; const double* slots; int nslot; float leaky; float *dbeta, *dgamma; bool accumulate; };
// The whole normalise pass of the producing layer inside its reader (the BN-input mode of conv1x1_mfma.hip, option "bn_in_1x1"):
// the conv's input x is that layer's z; the kernel sums `slots`, publishes mean / invstd / scale / shift and the moving
// statistics as fv_ew_bn_act_stats does, multiplies LeakyReLU(z * scale + shift) (+ skip) and writes it to a_out
struct FvBnStatsIn {
    const double* slots; int nslot; double count;
    const float *gamma, *beta; float eps, momentum;
    float *mean, *invstd, *scale, *shift, *moving_mean, *moving_var;
    const float* skip; float* a_out; float leaky;
};
int fv_op_conv_forward(fv_ctx* ctx, const float* x, const float* w, int B, int H, int W, int cin, int cout, int ksize,
                       int stride, int epi, const float* scale, const float* shift, float leaky, const float* addend,
                       float* out, float* psum, float* psq, int ksplit = 1,
                       double* stat_slots = nullptr, int stat_nslot = 0, const FvBnIn* bn_in = nullptr,
                       const FvBnStatsIn* bn_stats_in = nullptr);
// Would the training forward (statistics into slots) / the weight-gradient of this problem take the kernel that has the mode?
// The launchers' own predicates under the context's options, so the schedule decides before anything is enqueued.
bool fv_op_conv_forward_takes_bn_in(fv_ctx* ctx, int B, int H, int W, int cin, int cout, int ksize, int stride);
// The same question for FvBnStatsIn.  `option` is the value of "bn_in_1x1": 0 never, 1 the shape classes whose fused launch
// measured faster than the pair of launches it replaces, 2 every launch the kernel takes (measurements).  No
// context: the schedule's decision can be listed without a device (fv_train_bn_in_1x1_plan).
bool fv_op_conv_forward_takes_bn_stats_in(int option, bool persist_on, int B, int H, int W, int cin, int cout, int ksize, int stride,
                                          bool with_skip);
bool fv_op_conv_wgrad_takes_bn_in(fv_ctx* ctx, int B, int H, int W, int cin, int cout, int dy_stride, int ksize, int stride);
bool fv_op_conv_wgrad_takes_bn_dy(fv_ctx* ctx, int B, int H, int W, int cin, int cout, int dy_stride, int ksize, int stride);
// optional fused BN-backward reduction of the layer whose output gradient a data-gradient produces (conv.h FV_EPI_BNRED)
struct FvBnRed { const float *z, *scale, *shift, *mean, *invstd; double* slots; int nslot; float leaky; };
// s2_pad_lo: rows / columns of zero padding in FRONT of the input of the stride-2 forward conv this is the gradient of.  1: this
// network's ZeroPadding2D(1) + 'valid' layers (dx[h] = sum_{2i + r - 1 = h}); 0: a 'same'-padded stride-2 conv, which pads (0, 1) --
// Keras' Conv2DTranspose(strides=2, padding='same'), out[h] = sum_{2i + r = h} (the reconstruction model, net_recon.hip)
int fv_op_conv_dgrad(fv_ctx* ctx, const float* dy, const float* w_t, int B, int H, int W, int cin, int cout_pad, int ksize,
                     int stride, const float* addend, float* dx, const FvBnRed* bn = nullptr, int s2_pad_lo = 1);
int fv_op_conv_wgrad(fv_ctx* ctx, const float* x, const float* dy, int B, int H, int W, int cin, int cout, int dy_stride,
                     int ksize, int stride, float* dw, const FvBnIn* bn_in = nullptr, const FvBnDy* bn_dy = nullptr);
